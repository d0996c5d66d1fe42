"""What deflation costs the device eigensolver (bfhipChebCovEigsBandDevice), on the structured triangle
mesh of tools/lbo_eigs_rate.py (n = 2^20 by default), in ONE process with the legs alternated:
  (a) the two new kernels, launched alone through bfdevEigsCrossGram (with its reduction) and bfdevEigsDeflate, and one whole
      projection pass through bfdevEigsProject, at p in --ps and m in --ms against a random Q [n, max m]; beside them the Gram
      and rotation kernels of section 25 at the same p (bfdevEigsGram, bfdevEigsRotate): those are the yardstick.  Algorithmic
      TFLOP/s: 2 n m p per contraction (a pass: twice that), 2 n p^2 for Gram and rotation.
  (b) + (c) converged runs: band 1 and band 2 at --nev / --guard with --degree large enough for the cap to decide, each once with
      the library's phase clocks on (the phases are then separated by stream synchronisations): iterations, the degree of every
      filter, the largest residual after every Rayleigh-Ritz step, wall time, and the projection's share of an outer iteration
      against the filter.  --skip-converged leaves this leg out; it has its own iteration limit (--max-iter).
--warmup untimed rounds, then --reps (>= 10) timed ones; median with min / max.  One JSON line on stdout and in --out.

    python tools/lbo_bands_rate.py --out profiles/r21_lbo_bands.json
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cheb_cov_rate import _timed, grid_mesh          # noqa: E402

PHASES = ("filter", "sx", "gram", "rotate", "residual", "host")


def stats(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def rate(flop, ms):
    """TFLOP/s from milliseconds: median [min - max] (the fastest time gives the largest rate)."""
    ms = np.asarray(ms, dtype=float)
    return {"median": float(flop / np.median(ms) / 1e9), "min": float(flop / ms.max() / 1e9), "max": float(flop / ms.min() / 1e9)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--ps", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--ms", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nev", type=int, default=48)
    ap.add_argument("--guard", type=int, default=16)
    ap.add_argument("--degree", type=int, default=4000)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--skip-converged", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import ChebCovariance, _capi, trimesh_lbo_fem
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    lib = _capi.load()
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    lib.bfEigsProfile.argtypes, lib.bfEigsProfile.restype = [C.c_int], None
    lib.bfEigsLastPhases.argtypes, lib.bfEigsLastPhases.restype = [C.POINTER(C.c_double * 6)], None
    lib.bfEigsLastProjectSeconds.argtypes, lib.bfEigsLastProjectSeconds.restype = [], C.c_double
    lib.bfEigsLastHistory.argtypes, lib.bfEigsLastHistory.restype = [vp, vp, u32], u32
    lib.bfdevEigsChunkRows.argtypes, lib.bfdevEigsChunkRows.restype = [u64, u32], u64
    lib.bfdevEigsCrossChunkRows.argtypes, lib.bfdevEigsCrossChunkRows.restype = [u64, u32], u64
    for name, args in (("bfdevEigsGram", [vp, vp, u64, u32, vp, vp, vp]), ("bfdevEigsRotate", [vp, vp, vp, u64, u32, vp]),
                       ("bfdevEigsCrossGram", [vp, u64, u64, u32, vp, u64, u32, vp, vp, vp]), ("bfdevEigsDeflate", [vp, u64, u64, u32, vp, vp, u64, u32, vp]),
                       ("bfdevEigsProject", [vp, u64, u64, vp, u64, u32, vp, vp, vp])):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, C.c_int
    n = a.side * a.side
    stream = lambda: C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    gen = torch.Generator(device="cuda:0").manual_seed(21)
    rand = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda:0", generator=gen)
    out = {}

    # ---- (a) the kernels ------------------------------------------------------------------------------------------------------
    mmax = max(a.ms)
    Q = rand(n, mmax)
    Q *= 1.0 / np.sqrt(n)                                  # columns of unit length on average: a pass leaves X finite round after round
    legs = {}
    for p in a.ps:
        X, Y, W = rand(n, p), rand(n, p), rand(p, p)
        O = torch.empty_like(X)
        chunks = -(-n // lib.bfdevEigsChunkRows(n, p))
        partG, G = torch.empty(chunks * p * p, dtype=torch.float64, device="cuda:0"), torch.empty(p * p, dtype=torch.float64, device="cuda:0")
        cchunks = -(-n // lib.bfdevEigsCrossChunkRows(n, p))
        partC, Cd = torch.zeros(cchunks * 256 * p, dtype=torch.float64, device="cuda:0"), torch.zeros(256 * p, dtype=torch.float64, device="cuda:0")
        keep = (X, Y, W, O, partG, G, partC, Cd)
        legs[f"gram_p{p}"] = (2.0 * n * p * p, lambda X=X, Y=Y, partG=partG, G=G, p=p: lib.bfdevEigsGram(X.data_ptr(), Y.data_ptr(), n, p, partG.data_ptr(), G.data_ptr(), stream()), keep)
        legs[f"rotate_p{p}"] = (2.0 * n * p * p, lambda X=X, W=W, O=O, p=p: lib.bfdevEigsRotate(X.data_ptr(), W.data_ptr(), O.data_ptr(), n, p, stream()), keep)
        for m in a.ms:
            def cross(X=X, partC=partC, Cd=Cd, p=p, m=m):
                rc = 0
                for m0 in range(0, m, 256):
                    rc |= lib.bfdevEigsCrossGram(Q.data_ptr(), mmax, m0, min(256, m - m0), X.data_ptr(), n, p, partC.data_ptr(), Cd.data_ptr(), stream())
                return rc

            def deflate(X=X, Cd=Cd, p=p, m=m):                 # C stays whatever the last cross-Gram left: the time does not depend on it
                rc = 0
                for m0 in range(0, m, 256):
                    rc |= lib.bfdevEigsDeflate(Q.data_ptr(), mmax, m0, min(256, m - m0), Cd.data_ptr(), X.data_ptr(), n, p, stream())
                return rc
            legs[f"cross_p{p}_m{m}"] = (2.0 * n * m * p, cross, keep)
            legs[f"deflate_p{p}_m{m}"] = (2.0 * n * m * p, deflate, keep)
            legs[f"pass_p{p}_m{m}"] = (4.0 * n * m * p, lambda X=X, partC=partC, Cd=Cd, p=p, m=m: lib.bfdevEigsProject(Q.data_ptr(), mmax, m, X.data_ptr(), n, p, partC.data_ptr(), Cd.data_ptr(), stream()), keep)
    times = {k: [] for k in legs}
    for r in range(a.warmup + max(a.reps, 10)):
        for k, (_, fn, _) in legs.items():
            rcs = []
            t = _timed(torch, lambda: rcs.append(fn()))
            assert rcs[0] == 0, k
            if r >= a.warmup:
                times[k].append(t)
    for k, (flop, _, _) in legs.items():
        out[k] = {"ms": stats(times[k]), "tflops": rate(flop, times[k])}
    for p in a.ps:
        g, ro = out[f"gram_p{p}"]["tflops"], out[f"rotate_p{p}"]["tflops"]
        for m in a.ms:
            c, d = out[f"cross_p{p}_m{m}"], out[f"deflate_p{p}_m{m}"]
            c["ratio_to_gram_median"] = c["tflops"]["median"] / g["median"]
            c["below_gram_beyond_spread"] = bool(c["tflops"]["max"] < g["min"])
            d["ratio_to_rotate_median"] = d["tflops"]["median"] / ro["median"]
            d["below_rotate_beyond_spread"] = bool(d["tflops"]["max"] < ro["min"])
    for k, v in out.items():
        print(f"{k}: " + json.dumps(v), file=sys.stderr, flush=True)
    del legs, Q
    torch.cuda.empty_cache()

    # ---- (b), (c) converged bands ---------------------------------------------------------------------------------------------
    rec = {"n": n, "reps": max(a.reps, 10), "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "unit": "ms by device events around each launch sequence; TFLOP/s algorithmic, median [min - max]", "legs": out}
    if not a.skip_converged:
        verts, faces = grid_mesh(a.side)
        rowptr, colind, data, mass = trimesh_lbo_fem(verts, faces)
        obj = ChebCovariance.from_csr(rowptr, colind, data, mass, device=0)
        rec["lam_max"], rec["nnz"] = obj.info()["lamMax"], len(data)
        total = 2 * a.nev
        U = torch.zeros((n, total), dtype=torch.float64, device="cuda:0")
        lam_all, bands = np.zeros(total), []
        for k in range(2):
            m = k * a.nev
            lib.bfEigsProfile(1)
            t0 = time.perf_counter()
            try:
                lam, _, info = obj.eigs_band(a.nev, (U, lam_all, m), guard=a.guard, degree=a.degree, max_iter=a.max_iter, out=U[:, m:m + a.nev], raise_on_limit=False)
            finally:
                lib.bfEigsProfile(0)
            wall = time.perf_counter() - t0
            ph, hist, deg = (C.c_double * 6)(), (C.c_double * 128)(), (C.c_uint32 * 128)()
            lib.bfEigsLastPhases(C.byref(ph))
            cnt = lib.bfEigsLastHistory(hist, deg, 128)
            proj = lib.bfEigsLastProjectSeconds()
            lam_all[m:m + a.nev] = lam
            its, rr, p = info["iterations"], info["iterations"] + 1, info["blockColumns"]
            steps = info["operatorColumns"] // p - rr
            b = {"locked": m, "nev": a.nev, "guard": a.guard, "degree_asked": a.degree, "code": info["code"], "converged": info["converged"], "iterations": its,
                 "filter_steps": int(steps), "degrees": list(deg[:cnt]), "max_residual_over_lam_max_per_step": list(hist[:cnt]), "wall_seconds": wall,
                 "seconds_by_phase": dict(zip(PHASES, ph)), "projection_seconds": proj, "workspace_bytes": info["workspaceBytes"],
                 "lam_first_last": [float(lam[0]), float(lam[-1])]}
            if its and steps:
                b["filter_ms_per_step"] = ph[0] / steps * 1e3
                b["per_outer_iteration_ms"] = {"filter": ph[0] / its * 1e3, "projection": proj / rr * 1e3}
                b["projection_share_of_filter"] = (proj / rr) / (ph[0] / its)
            bands.append(b)
            print(f"band {k}: " + json.dumps(b), file=sys.stderr, flush=True)
            if info["converged"] < a.nev:
                break                                       # the next band needs this one's vectors
        rec["converged_bands"] = bands
        obj.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
