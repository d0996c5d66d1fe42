"""Time per sample and achieved bytes per second of the matrix-free Chebyshev covariance (bfhipChebCov*, DESIGN.md section
22) on a structured triangle mesh generated in numpy (a --side x --side grid on a curved sheet: n = 2^20 by default, rows of
up to 7 nonzeros), order --order, on ONE object, the legs alternated in one process:
  (a) the single-vector way: a loop of bfhipChebCovSampleBlockDevice at q = 1 over vectors already on the device;
  (b) bfhipChebCovSampleBlockDevice at q in --q;
  (c) bfhipChebCovDrawDevice at the largest q (normals generated on the device).
Device events around each call, --warmup untimed rounds, then --reps (>= 10) timed ones; a figure is the time of the call
divided by the samples it makes: median with min / max.  Bytes are the algorithmic ones: per degree three block streams
(w, b_{k+2}, b_k), the matrix once (rowptr, colind, values) and the gather once (one block), times the order; the first two
degrees move less, which the count ignores.  One JSON line on stdout and in --out.

    python tools/cheb_cov_rate.py --out profiles/r16_cheb_cov_f64.json
A/B builds of the kernel (for instance -DBF_CHEB_GATHERS=4) are loaded through BFHIP_LIB_PATH, one process each.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_SPEC_BYTES_PER_S = 8.0e12


def grid_mesh(side):
    x, y = np.meshgrid(np.arange(side, dtype=float), np.arange(side, dtype=float), indexing="ij")
    z = 0.02 * side * np.sin(7.0 * x / side) * np.cos(5.0 * y / side)
    i, j = np.meshgrid(np.arange(side - 1), np.arange(side - 1), indexing="ij")
    a, b, c, d = (i * side + j).ravel(), ((i + 1) * side + j).ravel(), ((i + 1) * side + j + 1).ravel(), (i * side + j + 1).ravel()
    faces = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.uint64)
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1), faces


def _timed(torch, fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--order", type=int, default=128)
    ap.add_argument("--q", type=int, nargs="+", default=[8, 16, 64])
    ap.add_argument("--loop", type=int, default=4, help="q = 1 calls per timed window of leg (a)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import ChebCovariance, matern_density, trimesh_lbo_fem
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    verts, faces = grid_mesh(a.side)
    rowptr, colind, data, mass = trimesh_lbo_fem(verts, faces)
    n, nnz = len(mass), len(data)
    obj = ChebCovariance.from_csr(rowptr, colind, data, mass, device=0)
    obj.set_density(matern_density(0.05, 2.0), a.order)
    info = obj.info()
    dev = torch.device("cuda", 0)
    qmax = max(a.q)
    g = torch.Generator(device=dev).manual_seed(3)
    W = {q: torch.randn((n, q), dtype=torch.float64, device=dev, generator=g) for q in [1] + list(a.q)}
    matrix_bytes = (n + 1) * 8 + nnz * 12

    def bytes_of(q):
        return a.order * (4 * n * q * 8 + matrix_bytes)

    legs = {"loop_q1": (lambda: [obj.sample_block_device(W[1]) for _ in range(a.loop)], a.loop, a.loop * bytes_of(1))}
    for q in a.q:
        legs[f"block_q{q}"] = (lambda q=q: obj.sample_block_device(W[q]), q, bytes_of(q))
    legs[f"draw_q{qmax}"] = (lambda: obj.draw_device(1234, 0, qmax), qmax, bytes_of(qmax))
    times = {k: [] for k in legs}
    for r in range(a.warmup + max(a.reps, 10)):
        for k, (fn, _, _) in legs.items():
            t = _timed(torch, fn)
            if r >= a.warmup:
                times[k].append(t)
    out = {}
    for k, (_, per, nbytes) in legs.items():
        t = np.asarray(times[k])
        rate = nbytes / (np.median(t) * 1e-3)
        out[k] = {"median_ms_per_sample": float(np.median(t) / per), "min_ms_per_sample": float(t.min() / per), "max_ms_per_sample": float(t.max() / per),
                  "median_ms_per_call": float(np.median(t)), "algorithmic_bytes_per_call": int(nbytes), "bytes_per_s": float(rate),
                  "fraction_of_hbm_spec": float(rate / HBM_SPEC_BYTES_PER_S)}
        print(f"{k}: " + json.dumps(out[k]), file=sys.stderr, flush=True)
    base, best = out["loop_q1"], out.get("block_q64")
    rec = {"n": n, "nnz": nnz, "order": a.order, "lam_max": info["lamMax"], "reps": max(a.reps, 10), "warmup": a.warmup, "loop": a.loop,
           "device": torch.cuda.get_device_name(0), "lib": os.environ.get("BFHIP_LIB_PATH", "libbfhip.so"),
           "unit": "ms per sample: call time / columns of the call (events around the call: launches and enqueue gaps included)",
           "bytes": "order x (3 block streams + 1 gathered block + the matrix once)", "legs": out}
    if best:
        rec["block_q64_over_loop"] = base["median_ms_per_sample"] / best["median_ms_per_sample"]
        rec["block_q64_beats_loop_beyond_spread"] = best["max_ms_per_sample"] < base["min_ms_per_sample"]
    obj.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
