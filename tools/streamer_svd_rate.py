"""Rate of the device truncated SVD (bfhipTruncSvdDevice) on the shapes the streamer asks for, against
numpy's gesdd on this machine's CPUs, and the split of a whole stream_butterfly build into SVD seconds and host seconds.

    python tools/streamer_svd_rate.py [--out profiles/r23_streamer_svd.json] [--build-n 32768 --build-lmax 63] [--budget-tb 10]

Shapes: from tests/golden/streamer_svd_records_n32768.npz and ...n65536.npz (the SVDs of the numpy-driven structures of
DESIGN_EXPERIMENTS.md section 12: rows, cols, kept k) the largest by rows x cols, the median, and the first with 20-60 rows of
each file.  The blocks themselves are not kept, so a matrix of the recorded shape and rank profile stands in: G1 diag(s) G2
with Gaussian G1 [m x r], G2 [r x n], r = min(m, n), s_j = 10^(-3.2 j / k), generated on the GPU from a seed; about k of its
singular values lie above tol = 1e-3.  Both sides factorize that same matrix; the reported k is the device's, gesdd's beside it.

Times: the device call on a matrix already on the GPU (host clock around the synchronous call; one warm-up, then --repeat
calls, all listed); gesdd on the host copy, BLAS threads as numpy finds them (one call above 1e7 elements, else as many as the
device).  A shape whose sweeps would move more than --budget-tb terabytes (24 M ld (tiles - 1) x 10 sweeps: Gram read, rotate read
and write) is listed as skipped with that estimate, not run.  The launch count of a call is 3 per step (Gram, solve, rotate),
(tiles - 1) steps per sweep, plus the load, the norms and at most six launches for U and W.

--batched builds with one bfhipTruncSvdBatchDevice call per frontier of the row tree and adds the
per-batch record (count, launches, synchronisations, seconds) to the build's figures.  --batch-family C times one batched call
on C stand-ins of the 20-60-row family of the n32768 records (numpy blocks in, numpy factors out: what the streamer pays) against
the loop of C single calls on the same blocks; the median of --repeat after a warm-up, every run listed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pick(records):
    m, n = records[:, 0], records[:, 1]
    order = np.argsort(m * n, kind="stable")
    out = [("largest", records[order[-1]]), ("median", records[order[len(order) // 2]])]
    small = np.flatnonzero((m >= 20) & (m <= 60))
    if len(small):
        out.append(("rows20to60", records[small[0]]))
    return out


def stand_in(m, n, k, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = min(m, n)
    s = 10.0 ** (-3.2 * torch.arange(r, dtype=torch.float64, device="cuda") / max(k, 1))
    g1 = torch.randn((m, r), generator=g, dtype=torch.float64, device="cuda") / np.sqrt(m)
    g2 = torch.randn((r, n), generator=g, dtype=torch.float64, device="cuda") / np.sqrt(n)
    return (g1 * s) @ g2


def time_shape(m, n, k, repeat, budget_tb, tol=1e-3):
    import torch
    from butterfly_amd.streamer_build import truncated_svd_device
    M, N = max(m, n), min(m, n)
    ld = (N + 31) // 32 * 32
    tiles = ld // 16
    est_tb = 24.0 * M * ld * (tiles - 1) * 10 / 1e12
    row = dict(m=int(m), n=int(n), k_recorded=int(k), tiles=tiles, estimated_sweep_traffic_tb=est_tb)
    if est_tb > budget_tb:
        row["skipped"] = "estimated traffic above the budget: not run, on either side"
        return row
    A = stand_in(m, n, k, 1000 + m + n)
    truncated_svd_device(A, tol)                                            # warm-up: code objects, allocator
    dev, info, kd = [], None, None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kd, sigma, U, W, info = truncated_svd_device(A, tol)
        torch.cuda.synchronize()
        dev.append(time.perf_counter() - t0)
    a = A.cpu().numpy()
    cpu = []
    for _ in range(1 if m * n > 1e7 else repeat):
        t0 = time.perf_counter()
        u, s, vt = np.linalg.svd(a, full_matrices=False)
        kc = int(np.sum(s >= tol * s[0]))
        w = s[:kc, None] * vt[:kc]
        cpu.append(time.perf_counter() - t0)
    sweeps = int(info["sweeps"])
    row.update(k_device=int(kd), k_gesdd=kc, sweeps=sweeps, launches=3 * (tiles - 1) * sweeps + 9, device_seconds=dev, gesdd_seconds=cpu,
               device_median=float(np.median(dev)), gesdd_median=float(np.median(cpu)), gesdd_over_device=float(np.median(cpu) / np.median(dev)),
               sigma_max_rel_diff=float(np.abs(sigma.cpu().numpy() - s).max() / s[0]), single_run=len(cpu) == 1)
    del u, vt, w, U, W
    return row


def family_blocks(count):
    """numpy stand-ins of the first `count` recorded SVDs with 20 to 60 rows (tests/golden/streamer_svd_records_n32768.npz)."""
    recs = np.load(os.path.join(ROOT, "tests", "golden", "streamer_svd_records_n32768.npz"))["records"]
    small = recs[(recs[:, 0] >= 20) & (recs[:, 0] <= 60)][:count]
    return [stand_in(int(r[0]), int(r[1]), int(r[4]), 2000 + i).cpu().numpy() for i, r in enumerate(small)]


def time_family(count, repeat, tol=1e-3):
    import torch
    from butterfly_amd.streamer_build import truncated_svd_batch_device, truncated_svd_device
    blocks = family_blocks(count)
    row = dict(count=len(blocks), shapes=[list(b.shape) for b in blocks[:3]], rows=[int(min(b.shape[0] for b in blocks)), int(max(b.shape[0] for b in blocks))],
               cols=[int(min(b.shape[1] for b in blocks)), int(max(b.shape[1] for b in blocks))])
    res = truncated_svd_batch_device(blocks, tol)                            # warm-up of both paths
    ref = [truncated_svd_device(b, tol) for b in blocks]
    row["identical"] = all(r[0] == q[0] and r[1].tobytes() == q[1].tobytes() and r[2].tobytes() == q[2].tobytes() and r[3].tobytes() == q[3].tobytes()
                           for r, q in zip(res, ref))
    batch, loop, inner = [], [], []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = truncated_svd_batch_device(blocks, tol)
        batch.append(time.perf_counter() - t0)
        inner.append(res[0][4]["batch"]["seconds"])
        t0 = time.perf_counter()
        ref = [truncated_svd_device(b, tol) for b in blocks]
        loop.append(time.perf_counter() - t0)
    b = res[0][4]["batch"]
    sweeps = [int(r[4]["sweeps"]) for r in ref]
    row.update(batch_seconds=batch, loop_seconds=loop, batch_call_seconds=inner, batch_median=float(np.median(batch)), loop_median=float(np.median(loop)),
               loop_over_batch=float(np.median(loop) / np.median(batch)), launches=int(b["launches"]), synchronisations=int(b["synchronisations"]),
               loop_synchronisations_at_least=int(sum(s + 3 for s in sweeps)), sweeps=[min(sweeps), max(sweeps)], workspace_bytes=int(b["workspaceBytes"]))
    return row


def whole_build(n, lmax, tol=1e-3, max_sweeps=None, freq_depth=None, batched=False):
    from butterfly_amd import streamer_build as sb
    from oracle import streamer_values as sv              # the sphere's eigenfunctions: test infrastructure used as an input generator
    t0 = time.perf_counter()
    pts, phi, freqs = sv.sphere_lbo_problem(n, lmax)
    t_input = time.perf_counter() - t0
    wmax = float(np.sqrt(lmax * (lmax + 1.0)) * 1.0001)
    class Progress(sb.DeviceSvdFactorizer):              # a line every 250 SVDs: a long build must not look dead
        def svd(self, *args):
            out = super().svd(*args)
            if len(self.record) % 250 == 0:
                print(json.dumps(dict(svds=len(self.record), svd_seconds=round(self.seconds, 2), elapsed=round(time.perf_counter() - t0, 1))), flush=True)
            return out

        def svd_many(self, requests):
            out = super().svd_many(requests)
            print(json.dumps(dict(svds=len(self.record), batch=len(requests), svd_seconds=round(self.seconds, 2), elapsed=round(time.perf_counter() - t0, 1))),
                  flush=True)
            return out

    print(json.dumps(dict(input_seconds=round(t_input, 1))), flush=True)
    op, perm, info = sb.stream_butterfly(pts, phi, freqs, wmax, freq_depth=freq_depth, tol=tol, check_columns=4, factorizer=Progress(tol, 0, [], max_sweeps),
                                         batched=batched)
    rec = np.asarray([(m, nn, k, s) for m, nn, k, s, _ in info["svd_records"]])
    out = dict(n=n, columns=int(info["columns"]), freq_depth=info["freq_depth"], svds=info["svds"], merges=info["merges"], feeds=info["feeds"],
               seconds=info["seconds"], svd_seconds=info["svd_seconds"], host_seconds=info["host_seconds"], compile_seconds=info["compile_seconds"],
               input_seconds=t_input, leaf_bytes=info["leaf_bytes"], acceptance=info["acceptance"], max_sweeps=int(rec[:, 3].max()), sweep_cap=30 if max_sweeps is None else int(max_sweeps), svds_above_30_sweeps=int(np.sum(rec[:, 3] > 30)),
               max_rows=int(rec[:, 0].max()), max_cols=int(rec[:, 1].max()), wide=int(np.sum(rec[:, 0] < rec[:, 1])), single_run=True)
    if batched:
        b = info["svd_batches"]
        out.update(batched=True, batches=len(b), largest_batch=max(c for c, *_ in b), launches=int(sum(x[1] for x in b)),
                   synchronisations=int(sum(x[2] for x in b)), batch_records=[list(x) for x in b])
    else:
        # per call: 3 launches per step of a sweep, 3 + 2 for the load and the two sums, at most 5 for U and W; one wait per sweep and three more
        tiles = (np.minimum(rec[:, 0], rec[:, 1]) + 31) // 32 * 2
        out.update(batched=False, launches_at_most=int(np.sum(3 * (tiles - 1) * rec[:, 3] + 10)), synchronisations_at_least=int(np.sum(rec[:, 3] + 3)))
    op.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--budget-tb", type=float, default=10.0)
    ap.add_argument("--build-n", type=int, default=32768)
    ap.add_argument("--build-lmax", type=int, default=63)
    ap.add_argument("--build-max-sweeps", type=int, default=None, help="sweep cap of the build's SVDs (default: the library's 30)")
    ap.add_argument("--build-freq-depth", type=int, default=None, help="levels of the frequency tree (default: row-tree depth - 3)")
    ap.add_argument("--batched", action="store_true", help="build with one batched device call per frontier of the row tree")
    ap.add_argument("--batch-family", type=int, default=0, help="time a batch of this many 20-60-row stand-ins against the loop of single calls")
    ap.add_argument("--no-build", action="store_true")
    ap.add_argument("--no-shapes", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("streamer_svd_rate.py measures on the GPU; none is visible")
    res = dict(tool="tools/streamer_svd_rate.py", device=torch.cuda.get_device_name(0), cpus=len(os.sched_getaffinity(0)), tol=1e-3, shapes=[])

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    if not a.no_shapes:
        for name in ("n32768", "n65536"):
            recs = np.load(os.path.join(ROOT, "tests", "golden", f"streamer_svd_records_{name}.npz"))["records"]
            for what, r in pick(recs):
                row = time_shape(int(r[0]), int(r[1]), int(r[4]), a.repeat, a.budget_tb)
                row.update(source=name, which=what)
                print(json.dumps(row), flush=True)
                res["shapes"].append(row)
                flush()
    if a.batch_family:
        res["batch_family"] = time_family(a.batch_family, a.repeat)
        print(json.dumps(res["batch_family"]), flush=True)
        flush()
    if not a.no_build:
        res["build"] = whole_build(a.build_n, a.build_lmax, max_sweeps=a.build_max_sweeps, freq_depth=a.build_freq_depth, batched=a.batched)
        print(json.dumps(res["build"]), flush=True)
    flush()
    print(json.dumps(dict(done=True, shapes=len(res["shapes"]), build="build" in res)))


if __name__ == "__main__":
    main()
