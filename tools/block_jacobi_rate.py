"""Block-Jacobi preconditioner (bfhipBlockJacobi) on device-built BIE operands: what it costs to build and what it does to
GMRES.  Operands from fac_helm2_make_multilevel on the unit circle, k = n / 16:
  first     the first-kind single layer S (plain kernel, no weights, no correction);
  combined  the combined field  I/2 + (D - i k S) KR6 w  (self value 0.5, Kapur-Rokhlin order 6, weights 2 pi / n).
Per (system, n): the automatic blocks (count, size histogram, uncovered rows), the build time split into gather, inversion
and compile (medians of --reps builds, host clock, the call is synchronous), resident bytes of the result, and GMRES
(solve_gmres_device, CGS2, tol --tol, at most --max-iter Krylov vectors) without and with the preconditioner: iterations,
reported (preconditioned) residual, time, and the true residual ||b - A x|| / ||b||.  One JSON line per record on stdout and
the list in --out.

    python tools/block_jacobi_rate.py --n 65536 262144 --out profiles/r9_block_jacobi.json
    rocprofv3 --kernel-trace --stats -- python tools/block_jacobi_rate.py --n 65536 --systems combined --build-only --reps 1
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(system, n):
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.operator import HipOperator
    k = n / 16
    pts = hs.circle_points(n)
    if system == "first":
        op, perm, st = HipOperator.fac_helm2_make_multilevel(pts, k, device=0)
    else:
        w = np.full(n, 2 * np.pi / n)
        op, perm, st = HipOperator.fac_helm2_make_multilevel(pts, k, normals=pts.copy(), col_weights=w, layer_pot="combined", self_value=0.5,
                                                             kr_order=6, alpha=-1j * k, beta=1.0, device=0)
    return op, st


def merged_cuts(cuts, min_rows, max_block=128):
    out = [0]
    for i, c in enumerate(cuts[1:-1], start=1):
        if c - out[-1] < min_rows and cuts[i + 1] - out[-1] <= max_block:
            continue
        out.append(int(c))
    out.append(int(cuts[-1]))
    return np.array(out)


def true_residual(op, b, x):
    import torch
    return float(torch.linalg.vector_norm(b - op.apply_device(x)) / torch.linalg.vector_norm(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--systems", default="first,combined")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-rows", type=int, default=4, help="when the automatic blocks are singular: merge blocks smaller than this")
    ap.add_argument("--build-only", action="store_true", help="no GMRES (for a kernel trace of the build)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import _capi
    recs = []
    for n in a.n:
        for system in a.systems.split(","):
            t0 = time.perf_counter()
            op, bst = build(system, n)
            torch.cuda.synchronize()
            rec = {"system": system, "n": n, "k": n / 16, "operand_build_s": round(time.perf_counter() - t0, 2),
                   "operand_leaf_bytes": op.num_bytes()}
            cuts = op.block_jacobi_partition()
            user_cuts = None
            try:
                op.block_jacobi()[0].close()
            except _capi.BfhipError as e:
                if e.code != 2:
                    raise
                # a singular diagonal block (the plain S has a zero diagonal: a box of one point is a 1 x 1 zero block): the
                # caller's remedy, cuts that merge every block of fewer than --min-rows rows into the next one
                rec["automatic_cuts_singular"] = {"first_singular_block": int(e.info["firstSingularBlock"]), "message": str(e)}
                user_cuts = merged_cuts(cuts, a.min_rows)
                cuts = user_cuts
                rec["cuts"] = f"automatic, blocks of < {a.min_rows} rows merged into the next"
            infos, walls, pre = [], [], None
            for _ in range(a.reps):
                if pre is not None:
                    pre.close()
                torch.cuda.synchronize()
                t = time.perf_counter()
                pre, info = op.block_jacobi(cuts=user_cuts)
                walls.append(time.perf_counter() - t)
                infos.append(info)
            sizes = np.diff(cuts)
            hist = {int(s): int(c) for s, c in zip(*np.unique(sizes, return_counts=True))}
            st = pre.stats()
            med = lambda key: float(np.median([i[key] for i in infos]))
            rec.update({
                "blocks": int(infos[-1]["numBlocks"]), "max_block_rows": int(infos[-1]["maxBlockRows"]),
                "uncovered_rows": int(infos[-1]["uncoveredRows"]), "block_size_hist": hist,
                "min_pivot_rel": float(infos[-1]["minPivotRel"]),
                "build_ms": {"total": 1e3 * float(np.median(walls)), "gather": 1e3 * med("gatherSeconds"),
                             "invert": 1e3 * med("invertSeconds"), "compile": 1e3 * med("compileSeconds"), "reps": a.reps},
                "resident_bytes": {"leaf_arena": int(st["arenaBytes"]), "meta": int(st["metaBytes"]),
                                   "vector_arena": int(st["tempElems"]) * 16, "sum_mb2_x16": int(np.sum(sizes.astype(np.int64) ** 2) * 16)},
            })
            if not a.build_only:
                g = torch.Generator(device="cpu").manual_seed(99)
                b = torch.randn(n, dtype=torch.complex128, generator=g).to("cuda:0")
                for name, m in (("plain", None), ("block_jacobi", pre)):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    x, it, res = op.solve_gmres_device(b, tol=a.tol, max_num_iter=a.max_iter, precond=m)
                    torch.cuda.synchronize()
                    rec["gmres_" + name] = {"iters": it, "converged": bool(res <= a.tol), "reported_residual": res,
                                            "ms": 1e3 * (time.perf_counter() - t), "true_residual": true_residual(op, b, x)}
                    del x
                rec["gmres_tol"], rec["gmres_max_iter"] = a.tol, a.max_iter
            print(json.dumps(rec), flush=True)
            recs.append(rec)
            pre.close()
            op.close()
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(recs, fh, indent=1)


if __name__ == "__main__":
    main()
