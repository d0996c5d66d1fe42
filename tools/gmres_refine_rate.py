"""Time to a true relative residual of 1e-10 on the second-kind system I + alpha S of tests/bie.py (alpha = 4 pi / n,
S = the fac_helm2 single-layer operand of the CPU value builder, k = n / 16): plain complex128 GMRES
(solve_gmres_device) against mixed-precision refinement with the complex64 compile as the inner operator
(solve_gmres_refine_device, default inner tolerance).  The two solves alternate in one process after warm-up; host
clock around a synchronised solve; medians.  One JSON line per (n, nrhs) on stdout and in --out.

    python tools/gmres_refine_rate.py --n 16384 65536 --nrhs 1 8 --reps 5 --out profiles/r7_gmres_refine.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def system(n):
    import bie
    from butterfly_amd import helm2_structure as hs
    from oracle import helm2_build as hb
    k = n / 16
    pts = hs.circle_points(n)
    desc, root, perm = hs.helm2_multilevel_structure(pts, k, recipes=True)
    vals = hb.leaf_values(desc, k, pts[perm])
    root2 = bie.identity_plus(desc, vals, 2 * (2 * np.pi / n))
    return desc, root2, vals


def true_residual(op, b, x):
    import torch
    r = b - op.apply_device(x)
    rn = torch.linalg.vector_norm(r, dim=0) / torch.linalg.vector_norm(b, dim=0)
    return float(rn.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16384])
    ap.add_argument("--nrhs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-iter", type=int, default=200)
    ap.add_argument("--solvers", default="c128,refine", help="comma list of c128 / refine (one alone for a kernel trace)")
    ap.add_argument("--rhs-blocks", type=int, default=0, help="bfhipSetRhsBlocks(min_rhs) on the complex64 inner operator (0 = off)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd.operator import HipOperator
    recs = []
    for n in a.n:
        t0 = time.perf_counter()
        desc, root, vals = system(n)
        t_build = time.perf_counter() - t0
        mr = max(a.nrhs)
        op = HipOperator.from_desc(desc, vals, root=root, max_rhs=mr)
        low = HipOperator.from_desc(desc, vals, root=root, max_rhs=mr, demote_to_f32=True, rhs_blocks=a.rhs_blocks)
        for nrhs in a.nrhs:
            g = torch.Generator(device="cpu").manual_seed(1234 + nrhs)
            b = torch.randn((n, nrhs), dtype=torch.complex128, generator=g).to("cuda:0")

            def plain():
                x, it, res = op.solve_gmres_device(b, tol=a.tol, max_num_iter=a.max_iter)
                return x, {"iters": it, "reported_residual": res}

            def refine():
                x, k, inner, res, hist = op.solve_gmres_refine_device(b, low, tol=a.tol, max_outer=20, max_inner=a.max_iter)
                return x, {"outer": k, "inner": inner, "reported_residual": res, "history": [float(h) for h in hist]}

            runs = {k: f for k, f in (("c128", plain), ("refine", refine)) if k in a.solvers.split(",")}
            for _ in range(a.warmup):
                for f in runs.values():
                    f()
            torch.cuda.synchronize()
            times = {k: [] for k in runs}
            out = {}
            for _ in range(a.reps):
                for name, f in runs.items():
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    x, info = f()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t) * 1e3)
                    out[name] = (x, info)
            rec = {"n": n, "nrhs": nrhs, "k": n / 16, "tol": a.tol, "reps": a.reps, "value_build_s": round(t_build, 1)}
            for name in runs:
                x, info = out[name]
                rec[name] = dict(info, ms_median=float(np.median(times[name])), ms_all=[round(v, 3) for v in times[name]],
                                 true_residual=true_residual(op, b, x))
            if len(runs) == 2:
                xa, xb = out["c128"][0], out["refine"][0]
                rec["rel_diff_solutions"] = float(torch.linalg.vector_norm(xa - xb) / torch.linalg.vector_norm(xa))
                rec["refine_over_c128_time"] = rec["refine"]["ms_median"] / rec["c128"]["ms_median"]
            print(json.dumps(rec), flush=True)
            recs.append(rec)
        op.close()
        low.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(recs, fh, indent=1)


if __name__ == "__main__":
    main()
