#!/usr/bin/env python3
"""Bit-level record of bfhipLstSqTruncated on the catalogue of tests/lstsq_catalogue.py, for comparing two builds of the
least-squares kernels (a refactor must leave every bit, and every sweep count, where it was).

    BFHIP_LIB_PATH=<libbfhip.so of build A> python tools/lstsq_bits.py a.npz      one process per library
    BFHIP_LIB_PATH=<libbfhip.so of build B> python tools/lstsq_bits.py b.npz
    python tools/lstsq_bits.py --compare a.npz b.npz                              exit 1 at the first difference

The dump runs every case on its declared route and on every alternative it lists, in the batches the GPU test uses, and
stores per (case, option set): X as raw float64 bits, sigma, and info as (sweeps, rank, notConverged, the eight route
fields).  The sweep count is in it, so a changed rotation order or convergence rule shows even where X survives it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

_ROUTE = ("qr", "qrLdsClass", "qrStreaming", "jacobi", "w", "threads", "ldsClass", "resident")


def dump(path):
    import lstsq_catalogue as cat
    from butterfly_amd.operator import lstsq_truncated
    groups = {}
    for c in cat.catalogue():
        for o in [c["opts"]] + c["alt"]:
            groups.setdefault(cat.opts_key(o), (o, []))[1].append(c)
    out = {}
    for key, (opts, cases) in sorted(groups.items(), key=lambda kv: repr(kv[0])):
        tag = ",".join(f"{k}={v}" for k, v in key) or "defaults"
        for c, (X, sig, info) in zip(cases, lstsq_truncated([(c["A"], c["B"]) for c in cases], **(opts or {}))):
            name = f"{c['name']}|{tag}"
            out[name + "|X"] = np.ascontiguousarray(X).view(np.float64).view(np.uint64)
            out[name + "|sigma"] = np.asarray(sig, dtype=np.float64).view(np.uint64)
            out[name + "|info"] = np.array([info["sweeps"], info["rank"], info["notConverged"]] + [info["route"][k] for k in _ROUTE],
                                           dtype=np.int64)
    np.savez(path, **out)
    print(f"{len(out) // 3} runs of {len(cat.catalogue())} cases -> {path}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    if sorted(A.files) != sorted(B.files):
        print("the two dumps hold different runs:", sorted(set(A.files) ^ set(B.files))[:4])
        return 1
    for k in A.files:
        if not np.array_equal(A[k], B[k]):
            print(f"DIFFERENT: {k}")
            if k.endswith("|info"):
                print("  ", A[k].tolist(), "\n  ", B[k].tolist())
            return 1
    print(f"{len(A.files) // 3} runs: X, sigma and info bit-equal")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    dump(sys.argv[1])
