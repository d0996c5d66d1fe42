"""Rate of the shared-leaf adjoint's block kernels (bfhipSetAdjointRhsBlocks, bfStageKernelTMfma) on two synthetic operands compiled
with BFHIP_FLAG_ADJOINT: the helm2 layout at --n-helm2 points (seed 1234, k = n / 16; complex128 and complex64) and the streamer
layout that `bench.py --workload streamer` builds at --n-streamer points (F64, F32).  Per element type and nrhs two timings of
bfhipApplyTransposeDevice on the SAME operator and arena, alternated in one process --
  * off: the switch off (the default kernels: bfStageKernelT walks every item once per right-hand side);
  * on:  the switch on (one pass per 64 right-hand sides).
Device events around each apply, --warmup untimed rounds, medians of --reps with min / max as the spread.  One JSON line on
stdout and in --out.  --only on (or off) runs that path alone, for a kernel trace or a counter run (counters in a run of their
own).  --packed also times the BFHIP_FLAG_ADJOINT_PACKED adjoint of the same operand at the largest nrhs, for information.

Recommended minRhs: the smallest nrhs from which "on" beats "off" beyond both spreads for every element type measured
("recommended_min_rhs" of the record).  Until a record exists it stands for 2 (operator.ADJOINT_RHS_BLOCKS_DEFAULT; DESIGN.md
section 17 says which).

    python tools/adjoint_rhs_rate.py --out profiles/r13_adjoint_rhs_blocks_n65536.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(torch, fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def _summary(t):
    return {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-helm2", type=int, default=65536)
    ap.add_argument("--n-streamer", type=int, default=1048576)
    ap.add_argument("--lmax", type=int, default=255)
    ap.add_argument("--dtype", nargs="+", default=["c128", "c64", "f64", "f32"], choices=["c128", "c64", "f64", "f32"])
    ap.add_argument("--nrhs", type=int, nargs="+", default=[2, 4, 8, 16, 32, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-rhs", type=int, default=2)
    ap.add_argument("--only", default=None, choices=["off", "on"], help="run that path alone")
    ap.add_argument("--packed", action="store_true", help="also time the packed adjoint (its own operator) at the largest nrhs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import _capi
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd import streamer_structure as ss
    from butterfly_amd.operator import HipOperator
    tdts = {"c128": torch.complex128, "c64": torch.complex64, "f64": torch.float64, "f32": torch.float32}
    descs = {}

    def layout(dt):
        kind = "helm2" if dt in ("c128", "c64") else "streamer"
        if kind not in descs:
            if kind == "helm2":
                descs[kind] = hs.native_multilevel_structure(hs.circle_points(a.n_helm2), a.n_helm2 / 16.0)[0]
            else:
                pts3 = ss.fibonacci_sphere(a.n_streamer)
                wmax = float(np.sqrt(a.lmax * (a.lmax + 1.0)) * 1.0001)
                fd = ss.octree_depth(pts3) - 3
                counts, _ = ss.sphere_band_columns(wmax, fd)
                descs[kind] = ss.native_stream_structure(pts3, wmax, fd, counts)[0]
        return kind, descs[kind]

    paths = [a.only] if a.only else ["off", "on"]
    rec = {"n_helm2": a.n_helm2, "n_streamer": a.n_streamer, "lmax": a.lmax, "seed": 1234, "min_rhs": a.min_rhs, "reps": a.reps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "dtypes": {}}
    for dt in a.dtype:
        kind, desc = layout(dt)
        tdt = tdts[dt]
        kw = dict(device=0, seed=1234, max_rhs=max(a.nrhs), demote_to_f32=dt in ("c64", "f32"))
        op = HipOperator.from_desc(desc, None, flags=_capi.FLAG_ADJOINT, **kw)
        m, n = op.shape
        st = op.stats()
        drec = {"layout": kind, "rows": m, "cols": n, "arena_bytes": st["arenaBytes"], "nrhs": {}}
        for nrhs in a.nrhs:
            x = torch.randn((m, nrhs), dtype=tdt, device="cuda:0")
            y = torch.empty((n, nrhs), dtype=tdt, device="cuda:0")
            times = {p: [] for p in paths}
            for r in range(a.warmup + a.reps):
                for p in paths:
                    op.set_adjoint_rhs_blocks(a.min_rhs if p == "on" else 0)
                    t = _timed(torch, lambda: op.apply_transpose_device(x, y))
                    if r >= a.warmup:
                        times[p].append(t)
            out = {p: _summary(t) for p, t in times.items()}
            if "on" in out and "off" in out:
                out["off_over_on"] = out["off"]["median_ms"] / out["on"]["median_ms"]
                out["on_beats_off_beyond_spread"] = out["on"]["max_ms"] < out["off"]["min_ms"]
                op.set_adjoint_rhs_blocks(a.min_rhs); op.apply_transpose_device(x, y); yon = y.clone()
                op.set_adjoint_rhs_blocks(0); op.apply_transpose_device(x, y)
                torch.cuda.synchronize()
                out["on_vs_off_rel_l2"] = float(torch.linalg.norm(yon - y) / torch.linalg.norm(y))
            drec["nrhs"][str(nrhs)] = out
            print(f"{dt} nrhs {nrhs}: " + json.dumps(out), file=sys.stderr, flush=True)
        wins = [q for q in a.nrhs if drec["nrhs"][str(q)].get("on_beats_off_beyond_spread")]
        losses = [q for q in a.nrhs if q not in wins]
        # the smallest nrhs from which on every measured nrhs "on" beats "off" beyond both spreads
        drec["smallest_winning_nrhs"] = min((q for q in wins if all(l < q for l in losses)), default=None)
        op.close()
        if a.packed and not a.only:
            nrhs = max(a.nrhs)
            pk = HipOperator.from_desc(desc, None, flags=_capi.FLAG_ADJOINT_PACKED, **kw)
            x = torch.randn((m, nrhs), dtype=tdt, device="cuda:0")
            y = torch.empty((n, nrhs), dtype=tdt, device="cuda:0")
            prec = {"nrhs": nrhs, "arena_bytes": pk.stats()["arenaBytes"]}
            for p in paths:
                pk.set_adjoint_rhs_blocks(a.min_rhs if p == "on" else 0)
                prec[p] = _summary([_timed(torch, lambda: pk.apply_transpose_device(x, y)) for _ in range(a.warmup + a.reps)][a.warmup:])
            drec["packed"] = prec
            print(f"{dt} packed: " + json.dumps(prec), file=sys.stderr, flush=True)
            pk.close()
        rec["dtypes"][dt] = drec
    if not a.only:
        s = [d["smallest_winning_nrhs"] for d in rec["dtypes"].values()]
        rec["recommended_min_rhs"] = None if any(v is None for v in s) else max(s)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
