"""bfPlanBuild alone (tests/native/plan_oom.c: a fac_helm2 layout in complex128, a streamer layout in f64 and f32; forward for
1 and 64 right-hand sides, a row range, the shared and the packed adjoint) under AddressSanitizer + UBSan + LeakSanitizer
with the allocator wrapped:
* the digest of every host field of each BfPlan equals the one recorded in tests/golden/plan_fingerprints.json ("native":
  taken from the commit named there), what the inspection C-ABI does not show included;
* every allocation of every build fails once: MEMORY_ERROR, the BfPlan left zeroed, nothing leaked or freed twice."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "butterfly_amd", "csrc")
HOST = ["bfhip_ir.c", "bfhip_plan.c", "bfhip_api.c", "bfhip_file.c", "bfhip_shim.c", "bfhip_inspect.c", "bfhip_gmres.c", "bfhip_build.c", "bfhip_layout.c", "bfhip_streamer_layout.c"]


def test_planner_digests_and_every_allocation_failing_once(tmp_path):
    exe = str(tmp_path / "plan_oom")
    cmd = ["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-Wl,--wrap=malloc,--wrap=calloc,--wrap=realloc", "-I", os.path.join(ROOT, "include"), "-I", SRC,
           os.path.join(ROOT, "tests", "native", "plan_oom.c"), os.path.join(ROOT, "tests", "native", "device_stubs.c")] + \
          [os.path.join(SRC, f) for f in HOST] + ["-lm", "-ldl", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    # (only a missing sanitizer RUNTIME is a reason to skip: a compile error of the harness must fail, and the command line itself holds the word)
    if b.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", b.stderr) and "error:" not in b.stderr.replace("ld: error", ""):
        pytest.skip("no sanitizer runtime for gcc here")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(p.stdout)
    assert p.returncode == 0 and "planner clean" in p.stdout, (p.stdout + p.stderr)[-4000:]
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr
    lines = [ln.split() for ln in p.stdout.splitlines()]
    got = {ln[1]: ln[2] for ln in lines if ln[0] == "digest"}
    swept = {ln[1] for ln in lines if ln[0] == "sweep" and int(ln[2].split("=")[1]) > 0}
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_fingerprints.json")))
    want = gold["native"]
    assert sorted(got) == sorted(want) and swept == set(want)
    changed = [k for k in want if got[k] != want[k]]
    assert not changed, f"plans differ from those of {gold['recorded_from']}: {', '.join(changed)}"
