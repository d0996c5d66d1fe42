"""Rate of the complex64 block kernels (bfhipSetRhsBlocks) on the synthetic headline layout (seed 1234, k = n / 16): per nrhs
three timings of bfhipApplyDevice, alternated in one process --
  * c64_off: the complex64 operator with the switch off (the default kernels: every leaf element once per right-hand side);
  * c64_on:  the SAME operator, same arena, with the switch on (bfStageKernelC64Mfma*);
  * c128:    the complex128 compile of the operand on its block kernels (bfStageKernelC128Mfma*).
Device events around each apply, --warmup untimed rounds, medians of --reps with min / max as the spread.  One JSON line on
stdout and in --out.  --only c64_on (or another path) runs that path alone, for a kernel trace or a counter run.

    python tools/c64_rhs_rate.py --n 65536 --out profiles/r11_c64_rhs_blocks_n65536.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--nrhs", type=int, nargs="+", default=[2, 4, 8, 16, 32, 64])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-rhs", type=int, default=2)
    ap.add_argument("--only", default=None, help="c64_off / c64_on / c128: run that path alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.operator import HipOperator
    n = a.n
    desc, perm = hs.native_multilevel_structure(hs.circle_points(n), n / 16.0)
    paths = [a.only] if a.only else ["c64_off", "c64_on", "c128"]
    mr = max(a.nrhs)
    c64 = HipOperator.from_desc(desc, None, seed=1234, demote_to_f32=True, max_rhs=mr) if any(p != "c128" for p in paths) else None
    c128 = HipOperator.from_desc(desc, None, seed=1234, max_rhs=mr) if "c128" in paths else None
    rec = {"n": n, "seed": 1234, "min_rhs": a.min_rhs, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "c64_arena_bytes": c64.stats()["arenaBytes"] if c64 else None, "c128_arena_bytes": c128.stats()["arenaBytes"] if c128 else None,
           "nrhs": {}}

    def run(path, x64, y64, x128, y128):
        if path == "c128":
            c128.apply_device(x128, y128)
        else:
            c64.set_rhs_blocks(a.min_rhs if path == "c64_on" else 0)
            c64.apply_device(x64, y64)

    for nrhs in a.nrhs:
        x64 = torch.randn((n, nrhs), dtype=torch.complex64, device="cuda:0")
        x128 = x64.to(torch.complex128)
        y64, y128 = torch.empty_like(x64), torch.empty_like(x128)
        times = {p: [] for p in paths}
        for r in range(a.warmup + a.reps):
            for p in paths:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                run(p, x64, y64, x128, y128)
                e.record()
                e.synchronize()
                if r >= a.warmup:
                    times[p].append(s.elapsed_time(e))
        out = {p: {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))} for p, t in times.items()}
        if "c64_on" in out and "c64_off" in out:
            out["off_over_on"] = out["c64_off"]["median_ms"] / out["c64_on"]["median_ms"]
            out["on_beats_off_beyond_spread"] = out["c64_on"]["max_ms"] < out["c64_off"]["min_ms"]
            c64.set_rhs_blocks(a.min_rhs); c64.apply_device(x64, y64); yon = y64.clone()
            c64.set_rhs_blocks(0); c64.apply_device(x64, y64)
            torch.cuda.synchronize()
            out["on_vs_off_rel_l2"] = float(torch.linalg.norm(yon - y64) / torch.linalg.norm(y64))
        if "c64_on" in out and "c128" in out:
            out["on_over_c128"] = out["c64_on"]["median_ms"] / out["c128"]["median_ms"]
        rec["nrhs"][str(nrhs)] = out
        print(f"nrhs {nrhs}: " + json.dumps(out), file=sys.stderr, flush=True)
    wins = [q for q in a.nrhs if rec["nrhs"][str(q)].get("on_beats_off_beyond_spread")]
    rec["smallest_winning_nrhs"] = min(wins) if wins else None
    for o in (c64, c128):
        if o:
            o.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
