"""The device scope every host entry point uses (bfDevEnter / bfDevLeave, bfhip_internal.h) on the CPU: tests/native/dev_scope.c
drives it against recording fakes of bfdevGetDevice / bfdevSetDevice under AddressSanitizer + UBSan -- another device, the same
device, -1, a failing query, a failing set, leaving twice, leaving a zeroed scope."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "butterfly_amd", "csrc")


def test_device_scope_calls_and_restores(tmp_path):
    exe = str(tmp_path / "dev_scope")
    cmd = ["gcc", "-std=gnu11", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", SRC,
           os.path.join(ROOT, "tests", "native", "dev_scope.c"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    # (only a missing sanitizer RUNTIME is a reason to skip: a compile error of the harness must fail, and the command line itself holds the word)
    if b.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", b.stderr) and "error:" not in b.stderr.replace("ld: error", ""):
        pytest.skip("no sanitizer runtime for gcc here")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0 and "device scope clean" in p.stdout, (p.stdout + p.stderr)[-4000:]
    assert "runtime error" not in p.stderr and "ERROR: AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr
