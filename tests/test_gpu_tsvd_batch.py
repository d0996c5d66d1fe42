"""bfhipTruncSvdBatchDevice on the device.  The oracle is the single call, bit for bit: a batched kernel
runs the single call's body on the problem's own parameters, and no sum's order depends on the other problems.  The batch is
every designed case of tests/tsvd_cases.cases() (tall and wide, 2 to 10 tiles, 1 to 9 row chunks, 1 to 8 sweeps: the problems
retire in different sweeps and skip different steps), the strided 48 x 40 view with lda = 56 and a 40 x 24 zero matrix, none
above 1025 x 130.  One call has one tolerance, so every problem is cut at 1e-3 here (the case graded_tol1e-6 is then the graded
matrix a second time; the tolerance enters the count rule alone, which tests/test_gpu_tsvd.py checks at 1e-6)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tsvd_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3


def single_call(a, m, n, lda, tol=TOL, cap_u=None, cap_w=None, max_sweeps=0):
    """bfhipTruncSvdDevice as tests/test_gpu_tsvd.raw_call runs it: outputs filled with -7 beforehand."""
    from test_gpu_tsvd import raw_call
    return raw_call(a, m, n, lda, tol, cap_u=cap_u, cap_w=cap_w, max_sweeps=max_sweeps)


def batch_call(views, tol=TOL, caps=None, max_sweeps=0, limit=0):
    """views: [(device tensor view, m, n, lda)].  Returns (rc, message, infos, status, batch info, [(sigma, U, W)]) with sigma
    filled with -1 and U, W with -7 beforehand, capacities min(m, n) unless caps[i] = (capU, capW) says otherwise."""
    import torch
    from butterfly_amd import _capi
    lib = _capi.load()
    count = len(views)
    probs = (_capi.BfhipTruncSvdProblem * count)()
    infos = (_capi.BfhipTruncSvdInfo * count)()
    status = (C.c_int32 * count)(*([-1] * count))
    outs = []
    for i, (a, m, n, lda) in enumerate(views):
        N = min(m, n)
        cap_u, cap_w = (N, N) if caps is None or caps[i] is None else caps[i]
        sigma = torch.full((N,), -1.0, dtype=torch.float64, device=a.device)
        U = torch.full((m, max(cap_u, 1)), -7.0, dtype=torch.float64, device=a.device)
        W = torch.full((max(cap_w, 1), n), -7.0, dtype=torch.float64, device=a.device)
        p = probs[i]
        p.dA, p.m, p.n, p.lda, p.dSigma = a.data_ptr(), m, n, lda, sigma.data_ptr()
        p.dU, p.ldu, p.capU, p.dW, p.ldw, p.capW = U.data_ptr(), max(cap_u, 1), cap_u, W.data_ptr(), n, cap_w
        infos[i].structSize = C.sizeof(_capi.BfhipTruncSvdInfo)
        outs.append((sigma, U, W))
    opt = _capi.BfhipTruncSvdOptions()
    opt.structSize, opt.tol, opt.maxSweeps = C.sizeof(opt), tol, max_sweeps
    bi = _capi.BfhipTruncSvdBatchInfo()
    bi.structSize = C.sizeof(bi)
    rc = lib.bfhipTruncSvdBatchDevice(0, probs, count, C.byref(opt), limit, infos, status, C.byref(bi), None)
    msg = lib.bfhipLastErrorMessage().decode() if rc else ""
    torch.cuda.synchronize()
    return rc, msg, infos, list(status), bi, outs


def single_launches(m, n, sweeps, k):
    """Kernel launches of one bfhipTruncSvdDevice call with U and W: load, two for the sums of squares, three per round-robin
    step, two for the final sums, and the recovery (tall: gather, copy, contraction and its store; wide: one more for the
    reload of A^T; none for k = 0)."""
    nt = (min(m, n) + 31) // 32 * 2
    return 3 + 3 * sweeps * (nt - 1) + 2 + (0 if k == 0 else 4 if m >= n else 5)


@pytest.fixture(scope="module")
def problems():
    """The device copies of the matrices, the single calls' results (computed once, left unchanged) and the one batch."""
    import torch
    mats = [(name, A) for name, A, _, _ in tc.cases()]
    views = []
    for _, A in mats:
        d = torch.from_numpy(np.ascontiguousarray(A)).cuda()
        views.append((d, A.shape[0], A.shape[1], A.shape[1]))
    big, _ = tc.strided_case()
    dbig = torch.from_numpy(big).cuda()
    keep = dbig.clone()
    views.append((dbig[2:50, 8:48], 48, 40, 56))
    views.append((torch.zeros((40, 24), dtype=torch.float64, device="cuda"), 40, 24, 24))
    names = [n for n, _ in mats] + ["strided_48x40", "zero_40x24"]
    singles = []
    for a, m, n, lda in views:
        rc, info, sigma, U, W = single_call(a, m, n, lda)
        assert rc == 0
        singles.append((info, sigma, U, W))
    batch = batch_call(views)
    return dict(names=names, views=views, singles=singles, batch=batch, big=dbig, keep=keep)


def assert_same(name, single, out, info=None):
    import torch
    sinfo, sigma, U, W = single
    assert torch.equal(out[0], sigma), name
    assert torch.equal(out[1], U), name
    assert torch.equal(out[2], W), name
    if info is not None:
        assert (info.k, info.sweeps, info.numSingular, info.transposed, info.offNorm) == \
               (sinfo.k, sinfo.sweeps, sinfo.numSingular, sinfo.transposed, sinfo.offNorm), name


def test_the_batch_is_the_loop_bit_for_bit(problems):
    import torch
    rc, msg, infos, status, bi, outs = problems["batch"]
    assert rc == 0 and status == [0] * len(outs), (rc, msg, status)
    sweeps = [int(s[0].sweeps) for s in problems["singles"]]
    tiles = [(min(m, n) + 31) // 32 * 2 for _, m, n, _ in problems["views"]]
    print("sweeps", dict(zip(problems["names"], sweeps)), "tiles", sorted(set(tiles)))
    # the mix the test is about: problems of 2 to 10 tiles that retire in different sweeps
    assert min(tiles) == 2 and max(tiles) == 10 and len(set(sweeps)) >= 4 and min(sweeps) == 1
    for i, name in enumerate(problems["names"]):
        assert_same(name, problems["singles"][i], outs[i], infos[i])
        k = int(infos[i].k)
        assert bool((outs[i][1][:, k:] == -7.0).all()) and bool((outs[i][2][k:] == -7.0).all()), name
        assert infos[i].seconds == 0 and infos[i].workspaceBytes == 0
    assert problems["names"][-1] == "zero_40x24" and int(infos[len(outs) - 1].k) == 0 and bool((outs[-1][0] == 0).all())
    assert torch.equal(problems["big"], problems["keep"])
    loop = sum(single_launches(m, n, int(s[0].sweeps), int(s[0].k)) for (_, m, n, _), s in zip(problems["views"], problems["singles"]))
    print(f"batch: {bi.launches} launches, {bi.synchronisations} synchronisations, {bi.seconds * 1e3:.2f} ms, workspace {bi.workspaceBytes / 1e6:.1f} MB; "
          f"the loop: {loop} launches, {sum(s + 3 for s in sweeps)} synchronisations at least")
    assert bi.groups == 1 and bi.failed == 0 and bi.maxSweeps == max(sweeps)
    assert bi.synchronisations == bi.maxSweeps + 3
    assert 0 < bi.launches < loop


def test_grouping_order_and_count_do_not_change_a_bit(problems):
    views, singles = problems["views"], problems["singles"]
    # a limit that forces several groups: the largest problem alone, the small ones a few per group
    rc, msg, infos, status, bi, outs = batch_call(views, limit=3 << 20)
    assert rc == 0 and 3 <= bi.groups < len(views), (rc, msg, bi.groups)
    for i, name in enumerate(problems["names"]):
        assert_same(name, singles[i], outs[i], infos[i])
    # the groups' own synchronisation counts add up: every group waits for its own largest sweep count + 3
    assert bi.synchronisations >= bi.maxSweeps + 3 * bi.groups
    # the problems in reverse
    rc, msg, infos, status, bi, outs = batch_call(views[::-1])
    assert rc == 0 and bi.groups == 1
    for i, name in enumerate(problems["names"]):
        assert_same(name, singles[i], outs[len(views) - 1 - i], infos[len(views) - 1 - i])
    # one problem per call
    for i, name in enumerate(problems["names"]):
        rc, msg, infos, status, bi, outs = batch_call(views[i:i + 1])
        assert rc == 0 and bi.synchronisations == singles[i][0].sweeps + 3
        assert_same(name, singles[i], outs[0], infos[0])


def test_failures_stay_local(problems):
    import torch
    names, views = problems["names"], problems["views"]
    trio = [views[names.index("orthonormal_120x40")], views[names.index("graded_tol1e-3")], views[-1]]
    rc, msg, infos, status, bi, outs = batch_call(trio, max_sweeps=1)
    assert status == [0, 2, 0] and rc == 2 and bi.failed == 1, (rc, msg, status)
    assert msg.startswith("problem 1:") and "did not converge" in msg
    assert infos[1].sweeps == 1 and infos[1].numSingular == 96 and infos[1].offNorm > 1e-10
    assert bool((outs[1][1] == -7.0).all()) and bool((outs[1][2] == -7.0).all()) and bool((outs[1][0] > 0).all())
    for i in (0, 2):
        a, m, n, lda = trio[i]
        src, sinfo, sigma, U, W = single_call(a, m, n, lda, max_sweeps=1)
        assert src == 0
        assert_same(i, (sinfo, sigma, U, W), outs[i], infos[i])
    # the same graded problem alone: what the single call leaves behind on non-convergence is what the batch leaves
    a, m, n, lda = trio[1]
    src, sinfo, sigma, U, W = single_call(a, m, n, lda, max_sweeps=1)
    assert src == 2 and torch.equal(sigma, outs[1][0]) and sinfo.offNorm == infos[1].offNorm
    # too little room for U in one problem: its status alone, its k reported, the others written
    k = int(problems["singles"][names.index("graded_tol1e-3")][0].k)
    rc, msg, infos, status, bi, outs = batch_call(trio, caps=[None, (k - 1, 96), None])
    assert status == [0, 5, 0] and rc == 5 and msg.startswith("problem 1:"), (rc, msg, status)
    assert infos[1].k == k and bool((outs[1][1] == -7.0).all()) and bool((outs[1][2] == -7.0).all())
    assert torch.equal(outs[1][0], problems["singles"][names.index("graded_tol1e-3")][1])
    for i, j in ((0, names.index("orthonormal_120x40")), (2, len(names) - 1)):
        assert_same(i, problems["singles"][j], outs[i], infos[i])


def test_python_batch_is_the_python_single_call(problems):
    """truncated_svd_batch_device on numpy blocks: what truncated_svd_device returns for each, bit for bit."""
    from butterfly_amd import _capi
    from butterfly_amd.streamer_build import truncated_svd_batch_device, truncated_svd_device
    blocks = [A for _, A, _, _ in tc.cases()[:5]] + [np.zeros((40, 24))]
    res = truncated_svd_batch_device(blocks, TOL)
    assert len(res) == 6 and res[0][4]["batch"]["count"] == 6 and res[0][4]["batch"] is res[5][4]["batch"]
    for A, (k, sigma, U, W, info) in zip(blocks, res):
        k1, s1, U1, W1, i1 = truncated_svd_device(A, TOL)
        assert k == k1 and sigma.tobytes() == s1.tobytes() and U.tobytes() == U1.tobytes() and W.tobytes() == W1.tobytes()
        assert U.shape == (A.shape[0], k) and W.shape == (k, A.shape[1]) and info["sweeps"] == i1["sweeps"]
    with pytest.raises(_capi.BfhipError) as ei:
        truncated_svd_batch_device([np.zeros((40, 24)), tc.graded_matrix()], TOL, max_sweeps=1)      # the zero matrix converges in one sweep
    assert ei.value.code == 2 and "problem 1:" in str(ei.value)


def test_the_pipeline_batched_is_the_pipeline():
    from butterfly_amd import streamer_build as sb
    from oracle import streamer_values as sv
    pts, phi, freqs = sv.sphere_lbo_problem(600, 11)
    wmax = float(np.sqrt(11 * 12.0) * 1.0001)
    op_a, perm_a, a = sb.stream_butterfly(pts, phi, freqs, wmax, freq_depth=2, tol=TOL, max_rhs=64)
    op_b, perm_b, b = sb.stream_butterfly(pts, phi, freqs, wmax, freq_depth=2, tol=TOL, max_rhs=64, batched=True, check_columns=8)
    try:
        d, e = b["desc"], a["desc"]
        assert d.root == e.root and d.kind == e.kind and d.rows == e.rows and d.cols == e.cols and d.block_kind == e.block_kind
        assert [[tuple(c) for c in ch] for ch in d.children] == [[tuple(c) for c in ch] for ch in e.children]
        assert sorted(b["leaf_values"]) == sorted(a["leaf_values"])
        for node, v in a["leaf_values"].items():
            assert b["leaf_values"][node].tobytes() == v.tobytes(), node
        assert np.array_equal(perm_a, perm_b)
        assert [c for c, _, _, _ in b["svd_batches"]] == [1, 8, 1, 8, 1, 8, 1, 8, 8, 8] and len(b["svd_records"]) == 52 == b["svds"]
        assert sorted(r[:4] for r in b["svd_records"]) == sorted(r[:4] for r in a["svd_records"])
        print(f"svd_seconds: one call per node {a['svd_seconds']:.4f} s, one call per frontier {b['svd_seconds']:.4f} s; "
              f"launches {sum(x[1] for x in b['svd_batches'])}, synchronisations {sum(x[2] for x in b['svd_batches'])}; acceptance {b['acceptance']:.3e}")
        assert b["acceptance"] <= TOL
    finally:
        op_a.close()
        op_b.close()


def test_the_batch_example_builds_and_runs(tmp_path):
    """examples/trunc_svd_batch_device.c: plain C against include/bfhip.h, -Wall -Werror, run in a child process of its own."""
    lib = os.path.join(ROOT, "butterfly_amd", "csrc")
    exe = str(tmp_path / "trunc_svd_batch_device")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "trunc_svd_batch_device.c"), "-L", lib, "-lbfhip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-lm", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and p.stdout.strip().endswith("ok")
