"""Call times and phases of the likelihood's gradient in the density's parameters (bfhipChebCovCondLogLikGradDevice, DESIGN.md
section 26) on the grid mesh of tools/cheb_cov_rate.py (n = 2^20 by default), order --order, for each numObs in --k and each
number of parameters in --params:
  call    the whole call, device events around it, the legs (one per T, and a value-only bfhipCovCondLogLikelihoodDevice)
          alternated round by round in one process: --warmup untimed rounds, then --reps (>= 10) timed ones; median [min - max];
  phases  the same call with the library's profile switch on (bfChebGradProfile: the phases are then separated by stream
          synchronisations and timed by the host clock): alpha and value, the M panels (two triangular solves each), the
          contraction Y = X M[:, panel], the recurrences (unit panel included), the dot and the owner's sum; --phase-reps rounds
          after one untimed.
Set against: T x rowsSeconds of the same object's Create (the same number of polynomial applications) and the value-only
call.  The contraction's algorithmic rate is 2 n k 64 flop per panel over its phase time.  The derivative polynomials are those
of matern_density_grad at the order of p.  One JSON line on stdout and in --out.

    python tools/cheb_gradient_rate.py --out profiles/r20_cheb_gradient.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PHASES = ("alpha_value", "m_panels", "contract", "recurrence", "dot_sum")


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
    ap.add_argument("--params", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--phase-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import ChebCovariance, _capi, cheb_fit, matern_density, matern_density_grad, trimesh_lbo_fem
    from cheb_cov_rate import grid_mesh
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    lib = _capi.load()
    lib.bfChebGradProfile.argtypes, lib.bfChebGradProfile.restype = [C.c_int], None
    lib.bfChebGradLastPhases.argtypes, lib.bfChebGradLastPhases.restype = [C.POINTER(C.c_double * len(PHASES))], None
    verts, faces = grid_mesh(a.side)
    rowptr, colind, data, mass = trimesh_lbo_fem(verts, faces)
    n, nnz = len(mass), len(data)
    kappa, nu = 0.05, 2.0
    obj = ChebCovariance.from_csr(rowptr, colind, data, mass, device=0)
    obj.set_density(matern_density(kappa, nu), a.order)
    lam_max = obj.info()["lamMax"]
    grads = matern_density_grad(kappa, nu)
    all_coef = np.stack([cheb_fit(g, a.order, 0.0, lam_max) for g in grads])
    dev = torch.device("cuda", 0)
    reps = max(a.reps, 10)
    rec = {"n": n, "nnz": nnz, "order": a.order, "reps": reps, "warmup": a.warmup, "phase_reps": a.phase_reps,
           "device": torch.cuda.get_device_name(0), "lib": os.environ.get("BFHIP_LIB_PATH", "libbfhip.so"),
           "unit": "calls in ms (device events around the call); phases in ms (host clock between stream synchronisations, summed over the call); "
                   "rowsSeconds in seconds",
           "quoted_not_same_run": {"vector_fma_tile_kernel_tflops_section_24": 10.0, "eigs_rotation_tflops_section_25": [28.6, 34.1]},
           "k": {}}
    for k in a.k:
        obs = (np.arange(k, dtype=np.uint64) * (n // k) + (n // k) // 2)
        probe = obj.condition(obs[:min(k, 64)], np.ones(min(k, 64)))
        prior = probe.variance(obs[:min(k, 64)], prior=True, post=False).cpu().numpy()
        probe.close()
        noise = np.full(k, 0.01 * float(prior.mean()))
        cond = obj.condition(obs, noise)
        info = cond.info
        z0 = obj.draw_device(77, 0, 1)
        y = (z0[torch.from_numpy(obs.astype(np.int64)).to(dev), 0] + torch.from_numpy(np.sqrt(noise) * np.random.default_rng(k).standard_normal(k)).to(dev)).contiguous()
        panels = (k + 63) // 64
        legs = {f"grad_T{T}": (lambda T=T: cond.log_likelihood_grad_coef(y, all_coef[np.arange(T) % len(grads)])) for T in a.params}
        legs["lik_value"] = lambda: cond.log_likelihood(y)
        times = {name: [] for name in legs}
        for r in range(a.warmup + reps):
            for name, fn in legs.items():
                t = _timed(torch, fn)
                if r >= a.warmup:
                    times[name].append(t)
            print(f"k={k}: round {r + 1} of {a.warmup + reps}", file=sys.stderr, flush=True)
        out = {"rowsSeconds": info["rowsSeconds"], "setupApplies": info["setupApplies"], "panels": panels,
               "lik_value_ms": stats(times["lik_value"]), "T": {}}
        for T in a.params:
            phases = {p: [] for p in PHASES}
            buf = (C.c_double * len(PHASES))()
            lib.bfChebGradProfile(1)
            for r in range(1 + a.phase_reps):
                legs[f"grad_T{T}"]()
                torch.cuda.synchronize()
                lib.bfChebGradLastPhases(C.byref(buf))
                if r:
                    for p, v in zip(PHASES, buf):
                        phases[p].append(1e3 * v)
            lib.bfChebGradProfile(0)
            call = stats(times[f"grad_T{T}"])
            ph = {p: stats(v) for p, v in phases.items()}
            rows_ms = 1e3 * T * info["rowsSeconds"]
            res = {"call_ms": call, "phases_ms": ph, "T_x_rowsSeconds_ms": rows_ms, "call_over_T_x_rows": call["median"] / rows_ms,
                   "remainder_ms": call["median"] - rows_ms, "call_over_lik_value": call["median"] / out["lik_value_ms"]["median"],
                   "contract_tflops": 2.0 * n * k * 64 * panels / (ph["contract"]["median"] * 1e-3) / 1e12,
                   "phase_sum_ms": float(sum(v["median"] for v in ph.values()))}
            print(f"k={k} T={T}: " + json.dumps(res), file=sys.stderr, flush=True)
            out["T"][str(T)] = res
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
