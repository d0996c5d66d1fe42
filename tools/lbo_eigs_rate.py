"""Where the time of the device eigensolver goes (bfhipChebCovEigsDevice), on the structured triangle
mesh of tools/cheb_cov_rate.py (a --side x --side unit-spaced grid on a curved sheet: n = 2^20 by default), in ONE process
with the legs alternated:
  (a) eigs_p<P>:          the whole call at nev / guard of --blocks, --degree, stopped after --iters outer iterations (at this
                          n the lowest pairs do not converge at degree 20 within any sensible limit, see DESIGN.md section 25:
                          the legs measure rates, the iteration count is the limit), device events around the call;
  (b) eigs_p<P>_phases:   the same call with the library's phase clocks on (bfEigsProfile: the phases are then separated by
                          stream synchronisations and timed on the host clock): filter, S X, Gram, rotate, residual, host dense;
  (c) cheb_apply_q64:     bfhipChebCovApplyBlockDevice at q = 64 and order = --degree, the yardstick of a filter step.
--warmup untimed rounds, then --reps (>= 10) timed ones; median with min / max.  Derived per block size: a filter step per
column against a Clenshaw degree per column (relation 1), the dense launches of a Rayleigh-Ritz step against one filter
(relation 2), the algorithmic TFLOP/s of the Gram and rotate kernels (2 n p^2 each; 3 Gram and 4 rotate launches per
Rayleigh-Ritz step), and the host's share.  One JSON line on stdout and in --out.

    python tools/lbo_eigs_rate.py --out profiles/r19_lbo_eigs_f64.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cheb_cov_rate import _timed, grid_mesh          # noqa: E402

PHASES = ("filter", "sx", "gram", "rotate", "residual", "host")


def stats(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--degree", type=int, default=20)
    ap.add_argument("--iters", type=int, default=4, help="outer iterations per call (maxIter)")
    ap.add_argument("--blocks", type=int, nargs="+", default=[48, 16, 120, 8], help="nev guard pairs")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import ChebCovariance, _capi, trimesh_lbo_fem
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    lib = _capi.load()
    lib.bfEigsProfile.argtypes, lib.bfEigsProfile.restype = [C.c_int], None
    lib.bfEigsLastPhases.argtypes, lib.bfEigsLastPhases.restype = [C.POINTER(C.c_double * 6)], None
    verts, faces = grid_mesh(a.side)
    rowptr, colind, data, mass = trimesh_lbo_fem(verts, faces)
    n, nnz = len(mass), len(data)
    obj = ChebCovariance.from_csr(rowptr, colind, data, mass, device=0)
    obj.set_coefficients(np.ones(a.degree) / a.degree)             # any polynomial of that order: the yardstick is its time
    W = torch.randn((n, 64), dtype=torch.float64, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(3))
    blocks = [(a.blocks[i], a.blocks[i + 1]) for i in range(0, len(a.blocks), 2)]
    last = {}

    def eigs(nev, guard, profile):
        lib.bfEigsProfile(1 if profile else 0)
        try:
            lam, U, info = obj.eigs(nev, guard=guard, degree=a.degree, max_iter=a.iters, raise_on_limit=False)
        finally:
            lib.bfEigsProfile(0)
        ph = (C.c_double * 6)()
        if profile:
            lib.bfEigsLastPhases(C.byref(ph))
        last[(nev, guard)] = info
        return list(ph)

    legs = {}
    for nev, guard in blocks:
        legs[f"eigs_p{nev + guard}"] = lambda nev=nev, guard=guard: eigs(nev, guard, False)
        legs[f"eigs_p{nev + guard}_phases"] = lambda nev=nev, guard=guard: eigs(nev, guard, True)
    legs["cheb_apply_q64"] = lambda: obj.apply_block_device(W)
    times, phases = {k: [] for k in legs}, {k: [] for k in legs if k.endswith("_phases")}
    for r in range(a.warmup + max(a.reps, 10)):
        for k, fn in legs.items():
            got = []
            t = _timed(torch, lambda: got.append(fn()))
            if r >= a.warmup:
                times[k].append(t)
                if k in phases:
                    phases[k].append(got[0])
    out = {k: {"ms_per_call": stats(times[k])} for k in legs}
    cheb = np.asarray(times["cheb_apply_q64"]) / (a.degree * 64)            # ms per degree per column
    out["cheb_apply_q64"]["ms_per_degree_per_column"] = stats(cheb)
    for nev, guard in blocks:
        p, info = nev + guard, last[(nev, guard)]
        its, rr = info["iterations"], info["iterations"] + 1
        steps = (info["operatorColumns"] // p) - rr                            # filter launches: all applications of S but one per Rayleigh-Ritz step
        ph = np.asarray(phases[f"eigs_p{p}_phases"]) * 1e3                     # ms, [reps, 6]
        rec = out[f"eigs_p{p}_phases"]
        rec.update({"nev": nev, "guard": guard, "iterations": its, "converged": info["converged"], "filter_steps": int(steps),
                    "max_degree_used": info["maxDegreeUsed"], "workspace_bytes": info["workspaceBytes"], "code": info["code"]})
        rec["ms_per_call_by_phase"] = {name: stats(ph[:, i]) for i, name in enumerate(PHASES)}
        filt_iter = ph[:, 0] / max(its, 1)
        dense_rr = (ph[:, 2] + ph[:, 3] + ph[:, 4]) / rr
        rec["ms_per_outer_iteration"] = {"filter": stats(filt_iter), "sx": stats(ph[:, 1] / rr), "gram": stats(ph[:, 2] / rr), "rotate": stats(ph[:, 3] / rr),
                                         "residual": stats(ph[:, 4] / rr), "host_dense": stats(ph[:, 5] / rr)}
        rec["host_share_of_an_iteration"] = float(np.median(ph[:, 5] / rr) / np.median(filt_iter + ph[:, 1:].sum(axis=1) / rr))
        step_col = ph[:, 0] / max(steps, 1) / p
        rec["filter_ms_per_step_per_column"] = stats(step_col)
        rec["gram_tflops"] = float(2.0 * n * p * p / (np.median(ph[:, 2]) / (3 * rr) * 1e-3) / 1e12)
        rec["rotate_tflops"] = float(2.0 * n * p * p / (np.median(ph[:, 3]) / (4 * rr) * 1e-3) / 1e12)
        if p == 64:
            rec["relation1_filter_step_not_slower_than_a_clenshaw_degree_beyond_spread"] = bool(step_col.max() < cheb.min())
            rec["relation1_median_ratio"] = float(np.median(step_col) / np.median(cheb))
        rec["relation2_dense_launches_below_one_filter_beyond_spread"] = bool(dense_rr.max() < filt_iter.min())
        rec["relation2_median_ratio"] = float(np.median(dense_rr) / np.median(filt_iter))
    for k, v in out.items():
        print(f"{k}: " + json.dumps(v), file=sys.stderr, flush=True)
    rec = {"n": n, "nnz": nnz, "degree": a.degree, "iters": a.iters, "lam_max": obj.info()["lamMax"], "reps": max(a.reps, 10), "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "lib": os.environ.get("BFHIP_LIB_PATH", "libbfhip.so"),
           "unit": "ms; whole calls by device events, phases by the host clock between stream synchronisations", "legs": out}
    obj.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
