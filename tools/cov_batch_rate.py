"""Time per sample / per product of the batched covariance entries on the streamer layout that `bench.py --workload streamer`
builds (fac_streamer butterfly of a sphere under the fitted rank model, synthetic values), per element type (F32, F64), on ONE
operator and arena, the legs alternated in one process:
  sample  (a) the single-vector way: a loop of bfhipCovSampleDevice over vectors already on the device (the baseline);
          (b) bfhipCovSampleBlockDevice at nrhs in --nrhs with bfhipSetRealRhsBlocks off (the default kernels);
          (c) the same with the switch on (bfStageKernelRealMfma*);
          (d) bfhipCovDrawDevice (normals generated on the device) and bfhipCovMomentsDevice at the largest nrhs, switch on;
  matvec  the same three legs of bfhipCovMatvecDevice / bfhipCovMatvecBlockDevice; leg (c) switches the adjoint's block
          kernels on too (bfhipSetAdjointRhsBlocks), the product applies both A^T and A.
Device events around each call, --warmup untimed rounds, then --reps (>= 10) timed ones; every figure is the time of the call
divided by the samples it makes: median with min / max.  One JSON line on stdout and in --out.
--draw-only K runs K batched draws of the largest nrhs and nothing else (for a kernel trace: rocprofv3 --kernel-trace --stats).

    python tools/cov_batch_rate.py --n 1048576 --dtype f32 --out profiles/r15_cov_batch_f32.json
"""
import argparse
import ctypes as C
import json
import os
import sys

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


def _summary(t, per):
    t = np.asarray(t) / per
    return {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1048576)
    ap.add_argument("--lmax", type=int, default=255)
    ap.add_argument("--dtype", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--nrhs", type=int, nargs="+", default=[2, 8, 16, 64])
    ap.add_argument("--loop", type=int, default=16, help="single-vector calls per timed window of leg (a)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-matvec", action="store_true")
    ap.add_argument("--draw-only", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from butterfly_amd import _capi, streamer_structure as ss
    from butterfly_amd.operator import HipOperator
    lib = _capi.load()
    n = a.n
    pts3 = ss.fibonacci_sphere(n)
    wmax = float(np.sqrt(a.lmax * (a.lmax + 1.0)) * 1.0001)
    fd = ss.octree_depth(pts3) - 3
    counts, _ = ss.sphere_band_columns(wmax, fd)
    desc, _, gstats = ss.native_stream_structure(pts3, wmax, fd, counts)
    ncols = int(desc.cols[desc.root])
    qmax = max(a.nrhs)
    dev = torch.device("cuda", 0)
    rec = {"n": n, "num_cols": ncols, "lmax": a.lmax, "freq_depth": fd, "seed": 1234, "reps": a.reps, "warmup": a.warmup, "loop": a.loop,
           "unit": "ms per sample (sample legs) / per product (matvec legs): call time / columns of the call",
           "device": torch.cuda.get_device_name(0), "dtypes": {}}
    rng = np.random.default_rng(3)
    perm = torch.from_numpy(rng.permutation(n).astype(np.int64)).to(dev)
    rev = torch.empty_like(perm); rev[perm] = torch.arange(n, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    for dt in a.dtype:
        tdt = torch.float32 if dt == "f32" else torch.float64
        op = HipOperator.from_desc(desc, None, device=0, seed=1234, max_rhs=qmax, demote_to_f32=(dt == "f32"),
                                   flags=0 if a.no_matvec else _capi.FLAG_ADJOINT)
        h = op.handle
        gam = (1.0 / (1.0 + 0.001 * torch.arange(ncols, device=dev, dtype=torch.float64))).to(tdt)
        W = op.fill_normal(torch.empty((ncols, qmax), dtype=tdt, device=dev), 7)
        V = op.fill_normal(torch.empty((n, qmax), dtype=tdt, device=dev), 8)
        Z = torch.empty((n, qmax), dtype=tdt, device=dev)
        w1, v1, z1 = W[:, 0].contiguous(), V[:, 0].contiguous(), torch.empty(n, dtype=tdt, device=dev)
        s1, s2 = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)

        def switches(on, adjoint):
            op.set_real_rhs_blocks(2 if on else 0)
            if adjoint:
                op.set_adjoint_rhs_blocks(2 if on else 0)

        def block(q):      # leading q columns, repacked densely
            return W[:, :q].contiguous(), V[:, :q].contiguous(), torch.empty((n, q), dtype=tdt, device=dev)

        if a.draw_only:
            switches(True, False)
            for _ in range(a.draw_only):
                _capi.check(lib.bfhipCovDrawDevice(h, P(gam), P(perm), 1234, 0, qmax, P(Z), stream))
            torch.cuda.synchronize()
            op.close()
            continue

        legs = {}      # name -> (fn, columns per call, forward switch, is matvec)
        legs["sample_loop"] = (lambda: [lib.bfhipCovSampleDevice(h, P(gam), P(perm), P(w1), P(z1), stream) for _ in range(a.loop)], a.loop, False, False)
        if not a.no_matvec:
            legs["matvec_loop"] = (lambda: [lib.bfhipCovMatvecDevice(h, P(gam), P(perm), P(rev), P(v1), P(z1), stream) for _ in range(a.loop)], a.loop, False, True)
        blocks = {q: block(q) for q in a.nrhs}
        for q in a.nrhs:
            Wq, Vq, Zq = blocks[q]
            for on in (False, True):
                tag = "on" if on else "off"
                legs[f"sample_block_{tag}_{q}"] = (lambda Wq=Wq, Zq=Zq, q=q: _capi.check(lib.bfhipCovSampleBlockDevice(h, P(gam), P(perm), P(Wq), q, P(Zq), stream)), q, on, False)
                if not a.no_matvec:
                    legs[f"matvec_block_{tag}_{q}"] = (lambda Vq=Vq, Zq=Zq, q=q: _capi.check(lib.bfhipCovMatvecBlockDevice(h, P(gam), P(perm), P(rev), P(Vq), q, P(Zq), stream)), q, on, True)
        legs[f"draw_on_{qmax}"] = (lambda: _capi.check(lib.bfhipCovDrawDevice(h, P(gam), P(perm), 1234, 0, qmax, P(Z), stream)), qmax, True, False)
        legs[f"moments_on_{4 * qmax}"] = (lambda: _capi.check(lib.bfhipCovMomentsDevice(h, P(gam), P(perm), 1234, 0, 4 * qmax, min(qmax, 64), P(s1), P(s2), stream)), 4 * qmax, True, False)
        times = {k: [] for k in legs}
        for r in range(a.warmup + a.reps):
            for k, (fn, per, on, mv) in legs.items():
                switches(on, mv and not a.no_matvec)
                t = _timed(torch, fn)
                if r >= a.warmup:
                    times[k].append(t)
        out = {k: _summary(times[k], legs[k][1]) for k in legs}
        for kind in ("sample", "matvec"):
            base = out.get(f"{kind}_loop")
            for q in a.nrhs:
                k = f"{kind}_block_on_{q}"
                if base and k in out:
                    out[k]["loop_over_this"] = base["median_ms"] / out[k]["median_ms"]
                    out[k]["beats_loop_beyond_spread"] = out[k]["max_ms"] < base["min_ms"]
        st = op.stats()
        rec["dtypes"][dt] = {"arena_bytes": st["arenaBytes"], "stages": st["numStages"], "legs": out}
        for k, v in out.items():
            print(f"{dt} {k}: " + json.dumps(v), file=sys.stderr, flush=True)
        op.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
