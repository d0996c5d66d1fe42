#!/usr/bin/env python3
"""Records the reference's struct layouts for tests/test_abi_layout.py.

Compiles the probe of tests/test_abi_layout.py against the reference's own
headers (a checkout of sampotter/butterfly, release build: BF_DEBUG
undefined) and writes every sizeof / offsetof / vtable slot index / enum
value it prints to reference_abi_layout.json, so that the test compares
include/bfhip_abi.h with them without the reference tree.

Run from the repo root:  python tests/golden/make_abi_layout.py <reference>/include
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_abi_layout import PROBE_REF  # noqa: E402


def main():
    inc = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "ref.c"), os.path.join(tmp, "ref")
        with open(src, "w") as f:
            f.write(PROBE_REF)
        subprocess.check_call(["gcc", "-std=gnu11", "-DBF_DOUBLE", "-DBF_LINUX", f"-I{inc}", src, "-o", exe])
        out = subprocess.check_output([exe], text=True)
    layout = dict(line.split() for line in out.strip().splitlines())
    path = os.path.join(ROOT, "tests", "golden", "reference_abi_layout.json")
    with open(path, "w") as f:
        json.dump(layout, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(layout)} entries -> {path}")


if __name__ == "__main__":
    main()
