"""Time of the log-likelihood with its gradients and of exact kriging variances, on the streamer layout that
`bench.py --workload streamer` builds (fac_streamer butterfly of a sphere under the fitted rank model, synthetic values), on ONE
operator and arena per element type, for k in --obs observations:
  value_k        bfhipCovCondLogLikelihoodDevice with both gradient outputs NULL (alpha, quad, logDet);
  gamma_k        the same with dGradLogGamma: the strip solve over the numCols rows of B^T, and u = B^T alpha;
  both_k         both gradients (adds the strip solve of the identity);
  variance64_k   bfhipCovCondVarianceDevice, 64 queries, prior and posterior (one adjoint panel apply, pack, B r, strip solve;
                 wall time of the call, which is synchronous).
The first call of each entry allocates its workspace and is not timed.  Device events around each likelihood call, --warmup
untimed rounds, then --reps timed ones, the legs alternated: median with min / max in ms.  The strip solve's rate is
numCols k (k + 1) / 2 + 32 numCols k FMAs (the contraction below the diagonal tiles and the product with their inverses, padding
not counted) over gamma_k - value_k.  Create's time at the same shape is recorded next to it.  One JSON line on stdout and in --out.
--solve-only K runs K likelihood calls with the gamma gradient at the largest k and nothing else (for a kernel trace).

    python tools/cov_likelihood_rate.py --dtype f64 --out profiles/r15_cov_likelihood_f64.json
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
    ap.add_argument("--dtype", nargs="+", default=["f64"], choices=["f32", "f64"])
    ap.add_argument("--obs", type=int, nargs="+", default=[256, 2048])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workspace-bytes", type=int, default=0)
    ap.add_argument("--solve-only", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import _capi, streamer_structure as ss
    from butterfly_amd.operator import HipOperator
    n, q = a.n, 64
    pts3 = ss.fibonacci_sphere(n)
    wmax = float(np.sqrt(a.lmax * (a.lmax + 1.0)) * 1.0001)
    fd = ss.octree_depth(pts3) - 3
    counts, _ = ss.sphere_band_columns(wmax, fd)
    desc, _, _ = ss.native_stream_structure(pts3, wmax, fd, counts)
    ncols = int(desc.cols[desc.root])
    dev = torch.device("cuda", 0)
    rec = {"n": n, "num_cols": ncols, "lmax": a.lmax, "freq_depth": fd, "seed": 1234, "reps": a.reps, "warmup": a.warmup,
           "workspace_bytes": a.workspace_bytes, "unit": "ms per call", "device": torch.cuda.get_device_name(0), "dtypes": {}}
    rng = np.random.default_rng(3)
    perm = torch.from_numpy(rng.permutation(n).astype(np.int64)).to(dev)
    for dt in a.dtype:
        tdt = torch.float32 if dt == "f32" else torch.float64
        op = HipOperator.from_desc(desc, None, device=0, seed=1234, max_rhs=q, demote_to_f32=(dt == "f32"), flags=_capi.FLAG_ADJOINT)
        op.set_real_rhs_blocks(2)
        op.set_adjoint_rhs_blocks(2)
        gam = (1.0 / (1.0 + 0.001 * torch.arange(ncols, device=dev, dtype=torch.float64))).to(tdt)
        # the noise level: 1 % of the mean prior variance, from the moments of 64 prior draws
        s2 = torch.zeros(n, dtype=torch.float64, device=dev)
        op.cov_moments_device(gam, perm, 1234, 0, q, q, None, s2)
        noise = 0.01 * float(s2.mean()) / q
        out = {}
        for k in (a.obs if not a.solve_only else [max(a.obs)]):
            obs = rng.choice(n, size=k, replace=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cond = op.cov_condition(gam, perm, obs, np.full(k, noise))
            create_ms = 1e3 * (time.perf_counter() - t0)
            y = op.fill_normal(torch.empty(k, dtype=torch.float64, device=dev), 5)
            ws = a.workspace_bytes
            if a.solve_only:
                for _ in range(a.solve_only):
                    cond.log_likelihood(y, grad_log_gamma=True, workspace_bytes=ws)
                torch.cuda.synchronize()
                cond.close()
                continue
            query = rng.choice(n, size=64, replace=False)
            legs = {"value": lambda: cond.log_likelihood(y, workspace_bytes=ws),
                    "gamma": lambda: cond.log_likelihood(y, grad_log_gamma=True, workspace_bytes=ws),
                    "both": lambda: cond.log_likelihood(y, grad_log_gamma=True, grad_noise=True, workspace_bytes=ws)}
            value, g, h = legs["both"]()                     # allocates; not timed
            cond.variance(query, prior=True)
            torch.cuda.synchronize()
            times = {name: [] for name in list(legs) + ["variance64"]}
            for r in range(a.warmup + a.reps):
                for name, fn in legs.items():
                    t = _timed(torch, fn)
                    if r >= a.warmup:
                        times[name].append(t)
                t0 = time.perf_counter()
                post, prior = cond.variance(query, prior=True)
                if r >= a.warmup:
                    times["variance64"].append(1e3 * (time.perf_counter() - t0))
            res = {name: _summary(t) for name, t in times.items()}
            fmas = ncols * k * (k + 1) / 2 + 32.0 * ncols * k
            solve_ms = res["gamma"]["median_ms"] - res["value"]["median_ms"]
            info = cond.info
            res.update({"create_wall_ms": create_ms, "create_rows_ms": 1e3 * info["rowsSeconds"], "create_gram_ms": 1e3 * info["gramSeconds"],
                        "create_factor_ms": 1e3 * info["factorSeconds"], "strip_solve_fmas": fmas, "strip_solve_ms": solve_ms,
                        "strip_solve_tfma_per_s": fmas / (solve_ms * 1e-3) / 1e12 if solve_ms > 0 else None,
                        "loglik": float(value[0]), "quad": float(value[1]), "logdet": float(value[2]),
                        "homogeneity_residual": float(abs(g.sum() / 2 + h.sum() * noise - (value[1] - k) / 2)),
                        "post_over_prior_min": float((post / prior).min()), "post_over_prior_max": float((post / prior).max())})
            out[str(k)] = res
            print(f"{dt} k={k}: " + json.dumps(res), file=sys.stderr, flush=True)
            cond.close()
        st = op.stats()
        rec["dtypes"][dt] = {"arena_bytes": st["arenaBytes"], "stages": st["numStages"], "noise_var": noise, "obs": out}
        op.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
