"""Rate of the real element types' block kernels (bfhipSetRealRhsBlocks) on the streamer layout that `bench.py --workload streamer`
builds (fac_streamer butterfly of a sphere under the fitted rank model, synthetic values): per element type (F32, F64) and nrhs two
timings of bfhipApplyDevice on the SAME operator and arena, alternated in one process --
  * off: the switch off (the default kernels: the whole item once per right-hand side);
  * on:  the switch on (bfStageKernelRealMfma*).
Device events around each apply, --warmup untimed rounds, medians of --reps with min / max as the spread.  One JSON line on
stdout and in --out.  --only on (or off) runs that path alone, for a kernel trace or a counter run.  --extract N also times
bfhipExtractDevice of N rows x 256 columns (four 64-column unit panels), off and on.

    python tools/real_rhs_rate.py --n 1048576 --out profiles/r12_real_rhs_blocks_n1048576.json
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
    ap.add_argument("--n", type=int, default=1048576)
    ap.add_argument("--lmax", type=int, default=255)
    ap.add_argument("--dtype", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--nrhs", type=int, nargs="+", default=[2, 4, 8, 16, 32, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-rhs", type=int, default=2)
    ap.add_argument("--only", default=None, choices=["off", "on"], help="run that path alone")
    ap.add_argument("--extract", type=int, default=0, help="also time extract of this many rows x 256 columns, off and on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import streamer_structure as ss
    from butterfly_amd.operator import HipOperator
    n = a.n
    pts3 = ss.fibonacci_sphere(n)
    wmax = float(np.sqrt(a.lmax * (a.lmax + 1.0)) * 1.0001)
    fd = ss.octree_depth(pts3) - 3
    counts, _ = ss.sphere_band_columns(wmax, fd)
    desc, _, gstats = ss.native_stream_structure(pts3, wmax, fd, counts)
    ncols = int(desc.cols[desc.root])
    paths = [a.only] if a.only else ["off", "on"]
    rec = {"n": n, "num_cols": ncols, "lmax": a.lmax, "freq_depth": fd, "seed": 1234, "min_rhs": a.min_rhs, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "dtypes": {}}
    for dt in a.dtype:
        tdt = torch.float32 if dt == "f32" else torch.float64
        op = HipOperator.from_desc(desc, None, device=0, seed=1234, max_rhs=max(a.nrhs), demote_to_f32=(dt == "f32"))
        st = op.stats()
        drec = {"arena_bytes": st["arenaBytes"], "stages": st["numStages"], "items": st["numItems"], "nrhs": {}}
        for nrhs in a.nrhs:
            x = torch.randn((ncols, nrhs), dtype=tdt, device="cuda:0")
            y = torch.empty((n, nrhs), dtype=tdt, device="cuda:0")
            times = {p: [] for p in paths}
            for r in range(a.warmup + a.reps):
                for p in paths:
                    op.set_real_rhs_blocks(a.min_rhs if p == "on" else 0)
                    t = _timed(torch, lambda: op.apply_device(x, y))
                    if r >= a.warmup:
                        times[p].append(t)
            out = {p: _summary(t) for p, t in times.items()}
            if "on" in out and "off" in out:
                out["off_over_on"] = out["off"]["median_ms"] / out["on"]["median_ms"]
                out["on_beats_off_beyond_spread"] = out["on"]["max_ms"] < out["off"]["min_ms"]
                op.set_real_rhs_blocks(a.min_rhs); op.apply_device(x, y); yon = y.clone()
                op.set_real_rhs_blocks(0); op.apply_device(x, y)
                torch.cuda.synchronize()
                out["on_vs_off_rel_l2"] = float(torch.linalg.norm(yon - y) / torch.linalg.norm(y))
            drec["nrhs"][str(nrhs)] = out
            print(f"{dt} nrhs {nrhs}: " + json.dumps(out), file=sys.stderr, flush=True)
        wins = [q for q in a.nrhs if drec["nrhs"][str(q)].get("on_beats_off_beyond_spread")]
        losses = [q for q in a.nrhs if q not in wins]
        # the smallest nrhs from which on every measured nrhs "on" beats "off" beyond both spreads
        drec["smallest_winning_nrhs"] = min((q for q in wins if all(l < q for l in losses)), default=None)
        if a.extract and not a.only:
            rng = np.random.default_rng(5)
            rows, cols = rng.integers(0, n, size=a.extract), rng.integers(0, ncols, size=256)
            ex = {}
            for p in paths:
                op.set_real_rhs_blocks(a.min_rhs if p == "on" else 0)
                ts = [_timed(torch, lambda: op.extract(rows, cols)) for _ in range(a.warmup + 3)][a.warmup:]
                ex[p] = _summary(ts)
            ex["off_over_on"] = ex["off"]["median_ms"] / ex["on"]["median_ms"]
            drec["extract_rows_x_256"] = {"rows": a.extract, **ex}
            print(f"{dt} extract: " + json.dumps(ex), file=sys.stderr, flush=True)
        op.close()
        rec["dtypes"][dt] = drec
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
