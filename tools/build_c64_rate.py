#!/usr/bin/env python3
"""Device Helmholtz builder, complex64 output and the one-build pair, at N = 65536 and at the headline N = 262144, in one
process: wall time (BfhipBuildStats.seconds) of the complex128 build, the complex64 build (outDtype = BFHIP_C64) and the pair
(bfhipBuildHelm2Pair), `reps` repetitions each; arena bytes of each operator; matvec rate of the built complex64 operator beside
the built complex128 one; rel-l2 of one result against the other.  One JSON file per size: <out-dir>/r14_build_c64_n<N>.json.
usage: tools/build_c64_rate.py [--sizes 65536,262144] [--reps 5] [--steps 20] [--out-dir profiles]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def matvec_rate(op, x, steps):
    import torch
    y = op.apply_device(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        y = op.apply_device(x, y)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0), y


def measure(n, reps, steps):
    import torch
    from butterfly_amd import _capi
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.operator import HipOperator
    k = n / 16.0
    t0 = time.perf_counter()
    pts = hs.circle_points(n)
    desc, perm = hs.native_multilevel_structure(pts, k)
    tp = pts[perm]
    out = {"workload": f"fac_helm2 multilevel butterfly built on the device, unit circle, N={n}, k={k:g}", "n": n, "wavenumber": k,
           "structure_seconds": time.perf_counter() - t0, "reps": reps, "steps": steps}
    print(f"N={n}: structure {out['structure_seconds']:.1f} s", file=sys.stderr, flush=True)
    rng = np.random.default_rng(0)
    x = torch.from_numpy((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).cuda()
    secs = {"c128": [], "c64": [], "pair": []}
    y128 = None
    for r in range(reps):
        last = r == reps - 1
        op, st = HipOperator.build_helm2(desc, tp, k, device=0)
        secs["c128"].append(st["seconds"])
        if last:
            out["c128"] = {"arenaBytes": op.stats()["arenaBytes"], "leafBytes": op.stats()["leafBytes"], "build_stats": st}
            out["c128"]["matvec_per_s"], y128 = matvec_rate(op, x, steps)
        op.close()
        low, st = HipOperator.build_helm2(desc, tp, k, device=0, out_dtype=_capi.BFHIP_C64)
        secs["c64"].append(st["seconds"])
        if last:
            out["c64"] = {"arenaBytes": low.stats()["arenaBytes"], "leafBytes": low.stats()["leafBytes"], "build_stats": st}
            out["c64"]["matvec_per_s"], y64 = matvec_rate(low, x.to(torch.complex64), steps)
            out["c64"]["rel_l2_vs_c128"] = float((torch.linalg.norm(y64.to(torch.complex128) - y128) / torch.linalg.norm(y128)).item())
        low.close()
        op, low, st = HipOperator.build_helm2_pair(desc, tp, k, device=0)
        secs["pair"].append(st["seconds"])
        if last:
            out["pair"] = {"arenaBytes": [op.stats()["arenaBytes"], low.stats()["arenaBytes"]], "build_stats": st}
            yp = op.apply_device(x)
            out["pair"]["c128_half_equals_single_build"] = bool(torch.equal(yp, y128))
            out["pair"]["c64_half_equals_single_build"] = bool(torch.equal(low.apply_device(x.to(torch.complex64)), y64))
        op.close(); low.close()
        print(f"N={n} rep {r}: c128 {secs['c128'][-1]:.2f} s, c64 {secs['c64'][-1]:.2f} s, pair {secs['pair'][-1]:.2f} s", file=sys.stderr, flush=True)
    out["build_seconds"] = {name: spread(v) for name, v in secs.items()}
    out["build_seconds"]["sum_of_singles_median"] = out["build_seconds"]["c128"]["median"] + out["build_seconds"]["c64"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,262144")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    for n in (int(s) for s in args.sizes.split(",")):
        out = measure(n, args.reps, args.steps)
        path = os.path.join(args.out_dir, f"r14_build_c64_n{n}.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps({"n": n, "file": path, "build_seconds": {k: v["median"] if isinstance(v, dict) else v for k, v in out["build_seconds"].items()},
                          "matvec_per_s": [out["c128"]["matvec_per_s"], out["c64"]["matvec_per_s"]], "rel_l2": out["c64"]["rel_l2_vs_c128"]}), flush=True)


if __name__ == "__main__":
    main()
