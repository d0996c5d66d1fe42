"""Time of a conditioned draw next to a prior draw, and the setup time of conditioning, on the streamer layout that
`bench.py --workload streamer` builds (fac_streamer butterfly of a sphere under the fitted rank model, synthetic values), per
element type (F32, F64), on ONE operator and arena, the legs alternated in one process:
  prior_draw      bfhipCovDrawDevice at q = 64 (block switches on);
  cond_draw_k     bfhipCovCondDrawDevice at q = 64 for k in --obs observations (the same operator, arena and switches);
  setup_k         bfhipCovCondCreate for that k: wall time of the call, and its three phases from bfhipCovCondGetInfo.
Device events around each draw, --warmup untimed rounds, then --reps (>= 10) timed ones: median with min / max of the call
time in ms.  The figure of interest is cond_draw_k over prior_draw.  One JSON line on stdout and in --out.
--draw-only K runs K conditioned draws at the largest k and nothing else (for a kernel trace: rocprofv3 --kernel-trace
--stats; no counters in the same run).

    python tools/cov_condition_rate.py --n 1048576 --dtype f32 --out profiles/r16_cov_condition_f32.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

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
    t = np.asarray(t)
    return {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1048576)
    ap.add_argument("--lmax", type=int, default=255)
    ap.add_argument("--dtype", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--obs", type=int, nargs="+", default=[64, 512, 2048])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--draw-only", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import _capi, streamer_structure as ss
    from butterfly_amd.operator import HipOperator
    lib = _capi.load()
    n, q = a.n, 64
    pts3 = ss.fibonacci_sphere(n)
    wmax = float(np.sqrt(a.lmax * (a.lmax + 1.0)) * 1.0001)
    fd = ss.octree_depth(pts3) - 3
    counts, _ = ss.sphere_band_columns(wmax, fd)
    desc, _, _ = ss.native_stream_structure(pts3, wmax, fd, counts)
    ncols = int(desc.cols[desc.root])
    dev = torch.device("cuda", 0)
    rec = {"n": n, "num_cols": ncols, "lmax": a.lmax, "freq_depth": fd, "seed": 1234, "reps": a.reps, "warmup": a.warmup, "q": q,
           "unit": "ms per call of q columns", "device": torch.cuda.get_device_name(0), "dtypes": {}}
    rng = np.random.default_rng(3)
    perm = torch.from_numpy(rng.permutation(n).astype(np.int64)).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    for dt in a.dtype:
        tdt = torch.float32 if dt == "f32" else torch.float64
        op = HipOperator.from_desc(desc, None, device=0, seed=1234, max_rhs=q, demote_to_f32=(dt == "f32"), flags=_capi.FLAG_ADJOINT)
        op.set_real_rhs_blocks(2)
        op.set_adjoint_rhs_blocks(2)
        h = op.handle
        gam = (1.0 / (1.0 + 0.001 * torch.arange(ncols, device=dev, dtype=torch.float64))).to(tdt)
        Z = torch.empty((n, q), dtype=tdt, device=dev)
        # the noise level: 1 % of the mean prior variance, from the moments of 64 prior draws
        s2 = torch.zeros(n, dtype=torch.float64, device=dev)
        op.cov_moments_device(gam, perm, 1234, 0, q, q, None, s2)
        noise = 0.01 * float(s2.mean()) / q
        conds, setup = {}, {}
        for k in (a.obs if not a.draw_only else [max(a.obs)]):
            obs = rng.choice(n, size=k, replace=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            conds[k] = op.cov_condition(gam, perm, obs, np.full(k, noise))
            wall = time.perf_counter() - t0
            info = conds[k].info
            setup[k] = {"wall_ms": 1e3 * wall, "rows_ms": 1e3 * info["rowsSeconds"], "gram_ms": 1e3 * info["gramSeconds"], "factor_ms": 1e3 * info["factorSeconds"],
                        "setup_applies": info["setupApplies"], "factor_bytes": info["factorBytes"], "min_pivot": info["minPivot"], "max_pivot": info["maxPivot"]}
            print(f"{dt} setup_{k}: " + json.dumps(setup[k]), file=sys.stderr, flush=True)
        ys = {k: op.fill_normal(torch.empty(k, dtype=torch.float64, device=dev), 5) for k in conds}

        if a.draw_only:
            k = max(conds)
            for _ in range(a.draw_only):
                _capi.check(lib.bfhipCovCondDrawDevice(conds[k].handle, P(ys[k]), 1234, 4321, 0, q, P(Z), stream))
            torch.cuda.synchronize()
            op.close()
            continue

        legs = {"prior_draw": lambda: _capi.check(lib.bfhipCovDrawDevice(h, P(gam), P(perm), 1234, 0, q, P(Z), stream))}
        for k in conds:
            legs[f"cond_draw_{k}"] = lambda k=k: _capi.check(lib.bfhipCovCondDrawDevice(conds[k].handle, P(ys[k]), 1234, 4321, 0, q, P(Z), stream))
        times = {name: [] for name in legs}
        for r in range(a.warmup + a.reps):
            for name, fn in legs.items():
                t = _timed(torch, fn)
                if r >= a.warmup:
                    times[name].append(t)
        out = {name: _summary(times[name]) for name in legs}
        base = out["prior_draw"]
        for k in conds:
            o = out[f"cond_draw_{k}"]
            o["over_prior_draw"] = o["median_ms"] / base["median_ms"]
            o["spreads_overlap"] = o["min_ms"] <= base["max_ms"]
        st = op.stats()
        rec["dtypes"][dt] = {"arena_bytes": st["arenaBytes"], "stages": st["numStages"], "noise_var": noise, "legs": out,
                             "setup": {str(k): v for k, v in setup.items()}}
        for name, v in out.items():
            print(f"{dt} {name}: " + json.dumps(v), file=sys.stderr, flush=True)
        op.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
