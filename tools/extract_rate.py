"""Rate of the dense extraction on the N = 65536 device-built operand (k = 4096, the survey size of
tests/test_gpu_build.py): columns 0..ncols-1 of A, all rows,
  * through bfhipExtractDevice (panels of 64) against the same number of plain 64-RHS bfhipApplyDevice calls;
  * through bfhipExtract into registered and into pageable host memory.
Host clock around synchronised calls, medians of --reps.  One JSON line on stdout and in --out.

    python tools/extract_rate.py --ncols 8192 --reps 3 --out profiles/r8_extract_rate.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--k", type=float, default=4096.0)
    ap.add_argument("--ncols", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--c64", action="store_true", help="a complex64 operand: the synthetic headline layout (seed 1234, k = n / 16) compiled with demote_to_f32")
    ap.add_argument("--rhs-blocks", type=int, default=0, help="with --c64: bfhipSetRhsBlocks(min_rhs) on the operand (0 = off)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.operator import HipOperator
    n = a.n
    pts = hs.circle_points(n)
    if not a.c64:
        desc, _, perm = hs.helm2_multilevel_structure(pts, a.k, recipes=True, exact_sift=True)
    if a.c64:
        desc, perm = hs.native_multilevel_structure(pts, n / 16.0)
        op = HipOperator.from_desc(desc, None, seed=1234, demote_to_f32=True, max_rhs=64, rhs_blocks=a.rhs_blocks)
    else:
        op, st = HipOperator.build_helm2(desc, pts[perm], a.k)
    ct = torch.complex64 if a.c64 else torch.complex128
    esz = 8 if a.c64 else 16
    cols = np.arange(a.ncols, dtype=np.uint64)
    out = torch.empty((n, a.ncols), dtype=ct, device="cuda")
    x = torch.zeros((n, 64), dtype=ct, device="cuda")
    x[torch.arange(64, device="cuda"), torch.arange(64, device="cuda")] = 1
    y = torch.empty((n, 64), dtype=ct, device="cuda")
    panels = (a.ncols + 63) // 64

    def timed(fn):
        ts = []
        for _ in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts[1:]))

    def applies():
        for _ in range(panels):
            op.apply_device(x, y)

    t_apply = timed(applies)
    t_dev = timed(lambda: op.extract(None, cols, out=out))
    rec = {"n": n, "k": a.k, "ncols": a.ncols, "panels": panels, "reps": a.reps,
           "apply64_s": t_apply, "extract_device_s": t_dev,
           "apply64_cols_per_s": a.ncols / t_apply, "extract_device_cols_per_s": a.ncols / t_dev,
           "device_over_apply": t_apply / t_dev, "output_bytes": n * a.ncols * esz,
           "dtype": "c64" if a.c64 else "c128", "rhs_blocks": a.rhs_blocks}
    assert torch.equal(out[:, :64], op.extract(None, cols[:64]))
    del out
    torch.cuda.empty_cache()
    if not a.skip_host and not a.c64:
        host = np.empty((n, a.ncols), dtype=np.complex128)
        host[:] = 0
        HipOperator.host_register(host)
        try:
            t_reg = timed(lambda: op.extract(None, cols, device=False, out=host))
        finally:
            HipOperator.host_unregister(host)
        t_page = timed(lambda: op.extract(None, cols, device=False, out=host))
        rec.update({"extract_host_registered_s": t_reg, "extract_host_pageable_s": t_page,
                    "registered_over_device": t_reg / t_dev, "pageable_over_device": t_page / t_dev,
                    "host_registered_GBps": n * a.ncols * 16 / t_reg / 1e9, "host_pageable_GBps": n * a.ncols * 16 / t_page / 1e9})
    op.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
