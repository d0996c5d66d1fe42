"""Setup phases and call times of conditioning the Chebyshev route on observations (bfhipChebCovCondCreate, DESIGN.md section
24) on the grid mesh of tools/cheb_cov_rate.py (n = 2^20 by default), order --order, for each numObs in --k:
  setup   bfhipChebCovCondCreate --setup-reps times (the object freed in between): rowsSeconds, gramSeconds, factorSeconds of
          BfhipCovCondInfo, and the host time of the whole call;
  draw    ms per sample of bfhipCovCondDrawDevice at q = 64, alternated in one process with bfhipChebCovDrawDevice at q = 64
          (the prior batch on the same object): the overhead of a conditional batch over a prior batch;
  lik     bfhipCovCondLogLikelihoodDevice, value only and with dGradNoise;
  var     bfhipCovCondVarianceDevice on 64 queries, prior and posterior (the call returns after its work is done).
Device events around each call, --warmup untimed rounds, then --reps (>= 10) timed ones, the legs alternated round by round;
every figure is a median with min / max.  The observed vertices are spread evenly over the mesh, the noise is 1 % of the mean
prior variance.  One JSON line on stdout and in --out.

    python tools/cheb_condition_rate.py --out profiles/r17_cheb_condition.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _timed(torch, fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def stats(values, per=1.0):
    t = np.asarray(values, dtype=np.float64) / per
    return {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--order", type=int, default=128)
    ap.add_argument("--k", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--q", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--setup-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import ChebCovariance, matern_density, trimesh_lbo_fem
    from cheb_cov_rate import grid_mesh
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    verts, faces = grid_mesh(a.side)
    rowptr, colind, data, mass = trimesh_lbo_fem(verts, faces)
    n, nnz = len(mass), len(data)
    obj = ChebCovariance.from_csr(rowptr, colind, data, mass, device=0)
    obj.set_density(matern_density(0.05, 2.0), a.order)
    dev = torch.device("cuda", 0)
    reps, q = max(a.reps, 10), a.q
    rec = {"n": n, "nnz": nnz, "order": a.order, "q": q, "reps": reps, "warmup": a.warmup, "setup_reps": a.setup_reps,
           "device": torch.cuda.get_device_name(0), "lib": os.environ.get("BFHIP_LIB_PATH", "libbfhip.so"),
           "unit": "setup in seconds; calls in ms (device events around the call: launches and enqueue gaps included); draw in ms per sample",
           "k": {}}
    for k in a.k:
        obs = (np.arange(k, dtype=np.uint64) * (n // k) + (n // k) // 2)
        # the noise scale: the prior variance at the observed vertices, from an object with unit noise
        probe = obj.condition(obs[:min(k, 64)], np.ones(min(k, 64)))
        prior = probe.variance(obs[:min(k, 64)], prior=True, post=False).cpu().numpy()
        probe.close()
        noise = np.full(k, 0.01 * float(prior.mean()))
        setup = {"rowsSeconds": [], "gramSeconds": [], "factorSeconds": [], "createSeconds": []}
        cond = None
        for _ in range(max(a.setup_reps, 1)):
            if cond is not None:
                cond.close()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cond = obj.condition(obs, noise)
            setup["createSeconds"].append(time.perf_counter() - t0)
            info = cond.info
            for name in ("rowsSeconds", "gramSeconds", "factorSeconds"):
                setup[name].append(info[name])
        # y: the values of one prior draw at the observed vertices, plus noise
        z0 = obj.draw_device(77, 0, 1)
        y = (z0[torch.from_numpy(obs.astype(np.int64)).to(dev), 0] + torch.from_numpy(np.sqrt(noise) * np.random.default_rng(k).standard_normal(k)).to(dev)).contiguous()
        query = (np.arange(64, dtype=np.uint64) * (n // 64) + 3)
        legs = {"cond_draw": lambda: cond.draw(y, 1234, 99, 0, q), "prior_draw": lambda: obj.draw_device(1234, 0, q),
                "lik_value": lambda: cond.log_likelihood(y), "lik_grad_noise": lambda: cond.log_likelihood(y, grad_noise=True),
                "variance_64": lambda: cond.variance(query, prior=True)}
        times = {name: [] for name in legs}
        for r in range(a.warmup + reps):
            for name, fn in legs.items():
                t = _timed(torch, fn)
                if r >= a.warmup:
                    times[name].append(t)
        out = {"factorBytes": info["factorBytes"], "setupApplies": info["setupApplies"], "minPivot": info["minPivot"], "maxPivot": info["maxPivot"],
               "setup_seconds": {name: stats(v) for name, v in setup.items()},
               "cond_draw_ms_per_sample": stats(times["cond_draw"], q), "prior_draw_ms_per_sample": stats(times["prior_draw"], q),
               "lik_value_ms": stats(times["lik_value"]), "lik_grad_noise_ms": stats(times["lik_grad_noise"]), "variance_64_ms": stats(times["variance_64"])}
        out["cond_over_prior_draw"] = out["cond_draw_ms_per_sample"]["median"] / out["prior_draw_ms_per_sample"]["median"]
        out["cond_over_prior_draw_beyond_spread"] = out["cond_draw_ms_per_sample"]["min"] > out["prior_draw_ms_per_sample"]["max"]
        med = {name: out["setup_seconds"][name]["median"] for name in ("rowsSeconds", "gramSeconds", "factorSeconds")}
        out["dominant_setup_phase"] = max(med, key=med.get)
        print(f"k={k}: " + json.dumps(out), file=sys.stderr, flush=True)
        rec["k"][str(k)] = out
        cond.close()
    obj.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
