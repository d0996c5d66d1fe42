"""The planner produces, plan for plan, what the commit named in tests/golden/plan_fingerprints.json produced: the digest of
tests/plan_fingerprint.py over every catalogue case in every element type, the random nested graphs and row ranges of
tests/test_plan_cpu.py, two fac_helm2 operands (RHS blocks, demoted, row blocks, row ranges) and a streamed butterfly.
A change to bfhip_plan.c that means to alter some plans records the goldens again from its parent first (see
tests/plan_fingerprint.py), then shows here exactly which operands it altered."""
import json

import numpy as np
import pytest

import plan_fingerprint as pf

GOLD = json.load(open(pf.GOLDEN))
OPERANDS = pf.operands()


def test_goldens_cover_the_operands():
    assert sorted(GOLD["plans"]) == sorted(OPERANDS)


@pytest.mark.parametrize("name", list(OPERANDS))
def test_plans_are_those_of_the_recorded_commit(helm2_cases, name):
    assert np.__version__ == GOLD["numpy"], (
        f"numpy {np.__version__} here, {GOLD['numpy']} when the goldens were recorded (random operands and SVD ranks follow it): "
        "record tests/golden/plan_fingerprints.json again from the parent commit (tests/plan_fingerprint.py)")
    got, want = OPERANDS[name](helm2_cases), GOLD["plans"][name]
    assert sorted(got) == sorted(want), f"{name}: the compiled variants differ from the recorded ones"
    changed = [v for v in want if got[v] != want[v]]
    assert not changed, f"{name}: plans differ from those of {GOLD['recorded_from']} for {', '.join(changed)}"
