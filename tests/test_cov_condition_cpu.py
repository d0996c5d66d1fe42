"""Conditioning on observations, the part that needs no GPU: the exported symbols, the size of
BfhipCovCondInfo, and the argument checks, which all come before the device is touched (a BFHIP_FLAG_PLAN_ONLY operator
reaches every check of bfhipCovCondCreate and is refused only afterwards; the entries that take a BfhipCovCond read nothing
through it before their own arguments are checked)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import randgraph
from butterfly_amd import _capi
from butterfly_amd.operator import CovCondition, HipOperator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, RUNTIME, RANGE, TYPE = 1, 2, 5, 7
NAMES = ("bfhipCovCondCreate", "bfhipCovCondFree", "bfhipCovCondGetInfo", "bfhipCovCondSampleBlockDevice", "bfhipCovCondMeanDevice",
         "bfhipCovCondDrawDevice", "bfhipCovCondMomentsDevice")


def test_the_new_symbols_are_exported():
    lib = _capi.load()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert callable(HipOperator.cov_condition)
    for name in ("sample_block", "mean", "draw", "moments", "close"):
        assert callable(getattr(CovCondition, name)), name
    assert isinstance(CovCondition.info, property)
    assert _capi.COND_MAX_OBS == 2048


def test_info_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bfhip.h"\nint main(void){printf("%zu %zu %zu %u\\n", sizeof(BfhipCovCondInfo), '
                   'offsetof(BfhipCovCondInfo, setupApplies), offsetof(BfhipCovCondInfo, factorSeconds), BFHIP_COND_MAX_OBS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_applies, off_factor, max_obs = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert size == C.sizeof(_capi.BfhipCovCondInfo) == 64
    assert off_applies == _capi.BfhipCovCondInfo.setupApplies.offset and off_factor == _capi.BfhipCovCondInfo.factorSeconds.offset
    assert max_obs == _capi.COND_MAX_OBS


@pytest.fixture(scope="module")
def plan_only_ops():
    rng = np.random.default_rng(77)
    desc, vals = randgraph.random_operand(rng, depth=3, size_hint=60, cplx=False, m=50, n=30)
    real = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_PLAN_ONLY | _capi.FLAG_ADJOINT)
    real_no_adjoint = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_PLAN_ONLY)
    cdesc, cvals = randgraph.random_operand(np.random.default_rng(78), depth=3, size_hint=60, cplx=True)
    cplx = HipOperator.from_desc(cdesc, cvals, flags=_capi.FLAG_PLAN_ONLY | _capi.FLAG_ADJOINT)
    yield real, real_no_adjoint, cplx
    for op in (real, real_no_adjoint, cplx):
        op.close()


def test_create_checks_come_before_the_device_in_order(plan_only_ops):
    lib = _capi.load()
    real, real_no_adjoint, cplx = plan_only_ops
    m = real.shape[0]
    assert m == 50

    def create(h, obs, noise=None, num=None, with_out=True):
        obs = np.asarray(obs, dtype=np.uint64)
        nv = None if noise is None else np.asarray(noise, dtype=np.float64)
        out = C.c_void_p(0x1234)
        rc = lib.bfhipCovCondCreate(h, None, None, obs.ctypes.data if obs.size else None, len(obs) if num is None else num,
                                    nv.ctypes.data if nv is not None else None, C.byref(out) if with_out else None, None)
        if with_out:
            assert not out.value          # *out is NULL after every failure
        return rc

    h = real.handle
    good = [3, 7, 49]
    # INVALID_ARGUMENTS: NULL operator, obs, out; numObs 0 and above the maximum
    assert create(None, good) == INVALID
    assert create(h, [], num=3) == INVALID
    assert create(h, good, with_out=False) == INVALID
    assert create(h, good, num=0) == INVALID
    assert create(h, np.arange(2049) % m, num=2049) == INVALID and b"numObs" in lib.bfhipLastErrorMessage()
    # a repeated observed index, then the noise variances
    assert create(h, [3, 7, 3]) == INVALID and b"repeated" in lib.bfhipLastErrorMessage()
    for bad in (-1.0, np.nan, np.inf):
        assert create(h, good, [0.1, bad, 0.0]) == INVALID and b"noiseVar[1]" in lib.bfhipLastErrorMessage()
    # the order: a repeated index wins over a bad variance and over an index out of range; a bad variance over the range
    assert create(h, [3, 3, 99], [0.1, -1.0, 0.0]) == INVALID and b"repeated" in lib.bfhipLastErrorMessage()
    assert create(h, [3, 7, 99], [0.1, -1.0, 0.0]) == INVALID and b"noiseVar" in lib.bfhipLastErrorMessage()
    # OUT_OF_RANGE: an observed index >= numRows, before the element type, the adjoint and the plan-only refusal
    assert create(h, [3, 7, m]) == RANGE
    assert create(cplx.handle, [3, 7, 10 ** 9]) == RANGE
    assert create(real_no_adjoint.handle, [3, 7, m]) == RANGE
    # TYPE_ERROR: a complex operator (it has an adjoint plan and is plan-only: neither is reached)
    assert create(cplx.handle, [0, 1, 2]) == TYPE
    # INVALID_ARGUMENTS: no adjoint plan, before the plan-only refusal
    assert create(real_no_adjoint.handle, good) == INVALID and b"BFHIP_FLAG_ADJOINT" in lib.bfhipLastErrorMessage()
    # everything in order: refused as plan-only, and only now; 2048 observations are allowed (m is too small for them: range)
    assert create(h, good) == RUNTIME and b"PLAN_ONLY" in lib.bfhipLastErrorMessage()
    assert create(h, good, [0.0, 0.5, 2.0]) == RUNTIME
    assert create(h, np.arange(m)) == RUNTIME
    assert create(h, np.arange(2048), num=2048) == RANGE


def test_call_checks_read_nothing_through_the_object():
    """No pointer below is ever dereferenced: every call ends in a check.  (0x1000 stands for "not NULL".)"""
    lib = _capi.load()
    p = C.c_void_p(0x1000)
    sample, mean, draw, moments = lib.bfhipCovCondSampleBlockDevice, lib.bfhipCovCondMeanDevice, lib.bfhipCovCondDrawDevice, lib.bfhipCovCondMomentsDevice
    assert sample(None, p, p, None, 4, p, None, None) == INVALID
    assert sample(p, None, p, None, 4, p, None, None) == INVALID
    assert sample(p, p, None, None, 4, p, None, None) == INVALID
    assert sample(p, p, p, None, 4, None, None, None) == INVALID
    assert sample(p, p, p, None, 0, p, None, None) == INVALID
    assert sample(p, p, p, None, 65536, p, None, None) == INVALID
    assert mean(None, p, p, None, None) == INVALID
    assert mean(p, None, p, None, None) == INVALID
    assert mean(p, p, None, None, None) == INVALID
    assert draw(None, p, 1, 2, 0, 4, p, None) == INVALID
    assert draw(p, None, 1, 2, 0, 4, p, None) == INVALID
    assert draw(p, p, 1, 2, 0, 4, None, None) == INVALID
    assert draw(p, p, 1, 2, 0, 0, p, None) == INVALID
    assert draw(p, p, 1, 2, 0, 65536, p, None) == INVALID
    assert moments(None, p, 1, 2, 0, 10, 0, p, p, None) == INVALID
    assert moments(p, None, 1, 2, 0, 10, 0, p, p, None) == INVALID
    assert moments(p, p, 1, 2, 0, 10, 0, None, None, None) == INVALID and b"both" in lib.bfhipLastErrorMessage()
    assert moments(p, p, 1, 2, 0, 10, 65, p, p, None) == INVALID and b"batch" in lib.bfhipLastErrorMessage()
    assert moments(p, p, 1, 2, 0, 0, 0, p, p, None) == INVALID and b"numSamples" in lib.bfhipLastErrorMessage()
    info = _capi.BfhipCovCondInfo()
    info.structSize = C.sizeof(info)
    assert lib.bfhipCovCondGetInfo(None, C.byref(info)) == INVALID
    info.structSize = 8
    assert lib.bfhipCovCondGetInfo(p, C.byref(info)) == INVALID
    none = C.c_void_p()
    lib.bfhipCovCondFree(C.byref(none))       # freeing nothing is allowed
    lib.bfhipCovCondFree(None)
