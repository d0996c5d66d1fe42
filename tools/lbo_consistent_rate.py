"""What the consistent-mass pencil costs on the device (BFHIP_EIGS_CONSISTENT_MASS), on the structured
triangle mesh of tools/cheb_cov_rate.py (n = 2^20 by default) at p = 64 block columns, in ONE process with the legs alternated,
device events around each launch sequence, --warmup untimed rounds and --reps (>= 10) timed ones, median with min / max:
  eigs_step            one bfEigsStepKernel launch, out = alpha (S b1) + beta b1 + gamma b2 in place of b2: a lumped filter step
  mass_step            one bfEigsMassStepKernel launch, all four terms, in place of b2: one step of the mass solve
  mass_product         the same kernel as B X alone
  two_products         S X and B X by two launches (eigs_step form without b2, mass_product)
  dual_product         S X and B X from one gather (bfdevEigsDualProduct, when the library has it); its outputs are compared with the
                       two launches' bit for bit first
  filter_step_mass     a filter step of the consistent pencil: T = S Y, the mass solve of k steps, the combination
  call_lumped / call_consistent   the whole call at nev 48, guard 16, degree 20 stopped after --iters outer iterations, phase clocks on
Then, once each and not alternated (they take seconds to minutes): the first band of 48 pairs (guard 16, degree 4000 so that the cap
decides, tol 1e-10) on both pencils with the phase clocks and the history on: iterations, degrees, residual per step, wall time.
One JSON line on stdout and in --out.

    python tools/lbo_consistent_rate.py --out profiles/r22_lbo_consistent.json
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


class BfEigsStep(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("colind", C.c_void_p), ("val", C.c_void_p), ("n", C.c_uint64), ("p", C.c_uint32), ("ld", C.c_uint32),
                ("b1", C.c_void_p), ("b2", C.c_void_p), ("out", C.c_void_p), ("alpha", C.c_double), ("beta", C.c_double), ("gamma", C.c_double)]


class BfEigsMassStep(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("colind", C.c_void_p), ("val", C.c_void_p), ("n", C.c_uint64), ("p", C.c_uint32), ("ld", C.c_uint32),
                ("b1", C.c_void_p), ("b2", C.c_void_p), ("w", C.c_void_p), ("out", C.c_void_p), ("alpha", C.c_double), ("beta", C.c_double),
                ("gamma", C.c_double), ("delta", C.c_double)]


class BfEigsMassSolve(C.Structure):
    _fields_ = [("rowptr", C.c_void_p), ("colind", C.c_void_p), ("val", C.c_void_p), ("n", C.c_uint64), ("p", C.c_uint32), ("ld", C.c_uint32),
                ("t", C.c_void_p), ("z", C.c_void_p), ("work", C.c_void_p), ("lo", C.c_double), ("hi", C.c_double), ("steps", C.c_uint32),
                ("reserved", C.c_uint32)]


def stats(v):
    v = np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--p", type=int, default=64)
    ap.add_argument("--mass-steps", type=int, default=22, help="k of the filter-step leg (the default of tol 1e-10 on P1 masses)")
    ap.add_argument("--iters", type=int, default=2, help="outer iterations of the stopped calls")
    ap.add_argument("--band-degree", type=int, default=4000)
    ap.add_argument("--skip-bands", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import ChebCovariance, _capi, trimesh_lbo_fem, trimesh_lbo_fem_mass
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    lib = _capi.load()
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    lib.bfEigsProfile.argtypes, lib.bfEigsProfile.restype = [C.c_int], None
    lib.bfEigsLastPhases.argtypes, lib.bfEigsLastPhases.restype = [C.POINTER(C.c_double * 6)], None
    lib.bfEigsLastHistory.argtypes, lib.bfEigsLastHistory.restype = [vp, vp, u32], u32
    lib.bfdevEigsStep.argtypes, lib.bfdevEigsStep.restype = [C.POINTER(BfEigsStep), vp], C.c_int
    lib.bfdevEigsMassStep.argtypes, lib.bfdevEigsMassStep.restype = [C.POINTER(BfEigsMassStep), vp], C.c_int
    lib.bfdevEigsMassSolve.argtypes, lib.bfdevEigsMassSolve.restype = [C.POINTER(BfEigsMassSolve), vp], C.c_int
    lib.bfdevEigsCombine.argtypes, lib.bfdevEigsCombine.restype = [vp, vp, vp, vp, u64, u32, u32, C.c_double, C.c_double, C.c_double, vp], C.c_int
    has_dual = hasattr(lib, "bfdevEigsDualProduct")
    if has_dual:
        lib.bfdevEigsDualProduct.argtypes, lib.bfdevEigsDualProduct.restype = [vp, vp, vp, vp, u64, u32, u32, vp, vp, vp, vp], C.c_int

    verts, faces = grid_mesh(a.side)
    rowptr, colind, data, mass = trimesh_lbo_fem(verts, faces)
    mdata = trimesh_lbo_fem_mass(verts, faces, rowptr, colind)
    n, nnz = len(mass), len(data)
    obj = ChebCovariance.from_csr(rowptr, colind, data, mass, device=0)
    obj.set_consistent_mass(mdata)
    # the launches alone need S and B on the device in the kernels' layout: folded here as the object folds them
    d = 1 / np.sqrt(mass)
    rows = np.repeat(np.arange(n), np.diff(rowptr.astype(np.int64)))
    cols = colind.astype(np.int64)
    dev = torch.device("cuda", 0)
    dRow = torch.from_numpy(rowptr.astype(np.int64)).to(dev)
    dCol = torch.from_numpy(colind.astype(np.int32)).to(dev)
    dS = torch.from_numpy((d[rows] * data) * d[cols]).to(dev)
    dB = torch.from_numpy((d[rows] * mdata) * d[cols]).to(dev)
    p = a.p
    ld = -(-p // 16) * 16
    gen = torch.Generator(device="cuda:0").manual_seed(22)

    def block():
        t = torch.zeros((n, ld), dtype=torch.float64, device=dev)
        t[:, :p] = torch.randn((n, p), dtype=torch.float64, device=dev, generator=gen)
        return t
    b1, b2, w, o1, o2, o3, o4 = block(), block(), block(), block(), block(), block(), block()
    stream = lambda: C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    ptr = lambda t: t.data_ptr() if t is not None else None

    def eigs_step(x, y, out, al=0.3, be=-0.2, ga=-0.9):
        s = BfEigsStep(dRow.data_ptr(), dCol.data_ptr(), dS.data_ptr(), n, p, ld, ptr(x), ptr(y), ptr(out), al, be, ga)
        assert lib.bfdevEigsStep(C.byref(s), stream()) == 0

    def mass_step(x, y, ww, out, sc=(0.3, -0.2, -0.9, 0.1)):
        s = BfEigsMassStep(dRow.data_ptr(), dCol.data_ptr(), dB.data_ptr(), n, p, ld, ptr(x), ptr(y), ptr(ww), ptr(out), *sc)
        assert lib.bfdevEigsMassStep(C.byref(s), stream()) == 0

    def two_products():
        eigs_step(b1, None, o1, 1.0, 0.0, 0.0)
        mass_step(b1, None, None, o2, (1.0, 0.0, 0.0, 0.0))

    def dual_product():
        assert lib.bfdevEigsDualProduct(dRow.data_ptr(), dCol.data_ptr(), dS.data_ptr(), dB.data_ptr(), n, p, ld, b1.data_ptr(), o3.data_ptr(), o4.data_ptr(), stream()) == 0

    def filter_step_mass():
        eigs_step(b1, None, o1, 1.0, 0.0, 0.0)
        s = BfEigsMassSolve(dRow.data_ptr(), dCol.data_ptr(), dB.data_ptr(), n, p, ld, o1.data_ptr(), o2.data_ptr(), o3.data_ptr(), 0.25, 1.0, a.mass_steps, 0)
        assert lib.bfdevEigsMassSolve(C.byref(s), stream()) == 0
        assert lib.bfdevEigsCombine(o2.data_ptr(), b1.data_ptr(), b2.data_ptr(), b2.data_ptr(), n, p, ld, 0.3, -0.2, -0.9e-3, stream()) == 0

    dual_equal = None
    if has_dual:
        two_products(); dual_product()
        torch.cuda.synchronize()
        dual_equal = bool(torch.equal(o1, o3) and torch.equal(o2, o4))

    last = {}

    def call(consistent, profile=True, **kw):
        lib.bfEigsProfile(1 if profile else 0)
        try:
            lam, U, info = obj.eigs(48, guard=16, raise_on_limit=False, consistent_mass=consistent, **kw)
        finally:
            lib.bfEigsProfile(0)
        ph = (C.c_double * 6)()
        lib.bfEigsLastPhases(C.byref(ph))
        last[consistent] = (lam, info)
        return list(ph)

    legs = {"eigs_step": lambda: eigs_step(b1, b2, b2), "mass_step": lambda: mass_step(b1, b2, w, b2),
            "mass_product": lambda: mass_step(b1, None, None, o2, (1.0, 0.0, 0.0, 0.0)), "two_products": two_products}
    if has_dual:
        legs["dual_product"] = dual_product
    legs["filter_step_mass"] = filter_step_mass
    legs["call_lumped"] = lambda: call(False, degree=20, max_iter=a.iters)
    legs["call_consistent"] = lambda: call(True, degree=20, max_iter=a.iters, mass_steps=a.mass_steps)
    times, phases = {k: [] for k in legs}, {"call_lumped": [], "call_consistent": []}
    reps = max(a.reps, 10)
    for r in range(a.warmup + reps):
        for k, fn in legs.items():
            got = []
            t = _timed(torch, lambda: got.append(fn()))
            if r >= a.warmup:
                times[k].append(t)
                if k in phases:
                    phases[k].append(got[0])
    out = {k: {"ms": stats(times[k])} for k in legs}
    t = {k: np.asarray(v) for k, v in times.items()}
    out["mass_step"]["over_eigs_step"] = stats(t["mass_step"] / t["eigs_step"])
    out["filter_step_mass"]["over_eigs_step"] = stats(t["filter_step_mass"] / t["eigs_step"])
    out["filter_step_mass"]["mass_steps"] = a.mass_steps
    if has_dual:
        out["dual_product"]["over_two_products"] = stats(t["dual_product"] / t["two_products"])
        out["dual_product"]["bit_equal_to_the_two_launches"] = dual_equal
        out["dual_product"]["faster_beyond_spread"] = bool(t["dual_product"].max() < t["two_products"].min())
    for k, cons in (("call_lumped", False), ("call_consistent", True)):
        lam, info = last[cons]
        ph = np.asarray(phases[k]) * 1e3
        its, pcols = info["iterations"], info["blockColumns"]
        rec = out[k]
        rec.update({"iterations": its, "max_degree_used": info["maxDegreeUsed"], "operator_columns": info["operatorColumns"], "workspace_bytes": info["workspaceBytes"],
                    "lam_max": info["lamMax"], "code": info["code"], "ms_by_phase": {name: stats(ph[:, i]) for i, name in enumerate(PHASES)}})
        rec["filter_ms_per_step"] = stats(ph[:, 0] / max(its * info["maxDegreeUsed"], 1))
        rec["block_columns"] = pcols
    out["call_consistent"]["filter_step_over_lumped"] = float(out["call_consistent"]["filter_ms_per_step"]["median"] / out["call_lumped"]["filter_ms_per_step"]["median"])
    for k, v in out.items():
        print(f"{k}: " + json.dumps(v), file=sys.stderr, flush=True)

    bands = {}
    if not a.skip_bands:
        for name, cons in (("lumped", False), ("consistent", True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ph = call(cons, degree=a.band_degree, tol=1e-10, max_iter=40)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            hist, deg = (C.c_double * 128)(), (C.c_uint32 * 128)()
            cnt = lib.bfEigsLastHistory(hist, deg, 128)
            lam, info = last[cons]
            its, pcols = info["iterations"], info["blockColumns"]
            steps = sum(deg[:cnt])
            b = {"nev": 48, "guard": 16, "degree_asked": a.band_degree, "code": info["code"], "converged": info["converged"], "iterations": its,
                 "degrees": list(deg[:cnt]), "filter_steps": int(steps), "max_residual_over_lam_max_per_step": list(hist[:cnt]), "wall_seconds": wall,
                 "seconds_by_phase": dict(zip(PHASES, ph)), "operator_columns": info["operatorColumns"], "workspace_bytes": info["workspaceBytes"],
                 "lam_max": info["lamMax"], "lam_first_last": [float(lam[0]), float(lam[-1])]}
            if steps:
                b["filter_ms_per_step"] = ph[0] / steps * 1e3
            bands[name] = b
            print(f"band {name}: " + json.dumps(b), file=sys.stderr, flush=True)

    rec = {"n": n, "nnz": nnz, "p": p, "ld": ld, "reps": reps, "warmup": a.warmup, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "lib": os.environ.get("BFHIP_LIB_PATH", "libbfhip.so"),
           "unit": "ms by device events around each leg, legs alternated; phases of the calls by the host clock between stream synchronisations; "
                   "the bands once each, wall seconds by the host clock",
           "legs": out, "first_band": bands}
    obj.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
