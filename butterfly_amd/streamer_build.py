"""Eigenbands to the butterfly of Phi, with the truncated SVDs on the device.

Step 2 of the reference's covariance pipeline (examples/covariance/lbo_cov.c:139-143, src/lbo.c:41-150): the eigenvector
columns are fed, leaf band by leaf band of the frequency tree, to the streamer (`streamer_structure.Streamer`, the
restatement of bfFacStreamerFeed and its merge-and-split recursion), whose one numerical step is a truncated SVD.

WHERE EACH PART RUNS.  The block algebra, the recursion, the conversion of a block to a dense matrix and the flat
descriptor stay on the host, in Python.  The GPU does the SVDs (`bfhipTruncSvdDevice`: one-sided block Jacobi on the FP64
matrix cores) and, afterwards, everything the compiled `HipOperator` is used for.  Every SVD is one synchronous call with
an upload of the block and a download of U and W around it.  The end-to-end build is therefore bounded by Python at N = 1M;
this module serves the range N <= 65536, where the SVD-driven structure exists at all (DESIGN_EXPERIMENTS.md section 12).
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import _capi
from . import streamer_structure as ss


def densify(block):
    """A node of the block algebra as a dense float64 array (bfMatDenseRealNewFromMatrix, src/mat_dense_real.c:711-799).
    The streamer hands the SVD blocks, never products of operators, so this is copies and no matrix multiplication."""
    t = type(block)
    if t is ss.Dense:
        if block.a is None:
            raise ValueError("value-free leaf")
        return np.asarray(block.a, dtype=np.float64)
    if t is ss.Identity:
        return np.eye(block.m)
    out = np.zeros((block.m, block.n))
    if t is ss.BlockDiag:
        for k, b in enumerate(block.blocks):
            out[block.ro[k]:block.ro[k] + b.m, block.co[k]:block.co[k] + b.n] = densify(b)
    elif t is ss.BlockDense:
        for p in range(block.nbr):
            for q in range(block.nbc):
                b = block.blocks[p * block.nbc + q]
                out[block.ro[p]:block.ro[p] + b.m, block.co[q]:block.co[q] + b.n] = densify(b)
    elif t is ss.BlockCoo:
        for i, j, b in zip(block.i0s, block.j0s, block.blocks):
            out[i:i + b.m, j:j + b.n] += densify(b)
    else:
        raise TypeError(f"the streamer does not hand a {t.__name__} to the SVD")
    return out


def truncated_svd_device(A, tol, device=0, max_sweeps=None, want_uw=True, stream=None):
    """bfhipTruncSvdDevice on a 2-D float64 array: numpy (uploaded; U and W come back as numpy) or a torch tensor on the GPU
    with unit column stride (used in place, any row stride >= n; U and W stay on the GPU).  Returns (k, sigma [min(m, n)], U
    [m, k], W [k, n] = S_k V_k^T, info dict); U and W are None with want_uw=False.  Small problems get room for every term and one
    call; large ones a values-only call that sizes U and W and a second one that fills them (the call is deterministic: both see
    the same k)."""
    import torch
    host = isinstance(A, np.ndarray)
    dev = torch.device("cuda", int(device))
    if host:
        a = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).to(dev)
    else:
        a = A
        if a.dtype != torch.float64 or a.device != dev or a.dim() != 2:
            raise ValueError(f"A: a 2-D float64 tensor on {dev}")
        if a.shape[1] > 1 and a.stride(1) != 1:
            raise ValueError("A: rows must be contiguous (column stride 1)")
    m, n = int(a.shape[0]), int(a.shape[1])
    lda = int(a.stride(0)) if m > 1 else n
    lib = _capi.load()
    opt = _capi.BfhipTruncSvdOptions()
    opt.structSize, opt.tol, opt.maxSweeps = C.sizeof(opt), float(tol), 0 if max_sweeps is None else int(max_sweeps)
    info = _capi.BfhipTruncSvdInfo()
    info.structSize = C.sizeof(info)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if stream is None else stream
    sigma = torch.empty(max(min(m, n), 1), dtype=torch.float64, device=dev)

    def call(u, w, cap):
        return lib.bfhipTruncSvdDevice(int(device), C.c_void_p(a.data_ptr()), m, n, lda, C.byref(opt), C.c_void_p(sigma.data_ptr()),
                                       C.c_void_p(u.data_ptr()) if u is not None else None, int(u.stride(0)) if u is not None else 0, cap,
                                       C.c_void_p(w.data_ptr()) if w is not None else None, n, cap, C.byref(info), s)

    N = min(m, n)
    U = W = None
    if not want_uw:
        _capi.check(call(None, None, 0))
        k, seconds = int(info.k), info.seconds
    elif (m + n) * N <= 1 << 27:
        # room for every term costs little: one call
        U = torch.empty((m, max(N, 1)), dtype=torch.float64, device=dev)
        W = torch.empty((max(N, 1), n), dtype=torch.float64, device=dev)
        _capi.check(call(U, W, N))
        k, seconds = int(info.k), info.seconds
        U, W = U[:, :k], W[:k]
    else:
        _capi.check(call(None, None, 0))
        k, seconds = int(info.k), info.seconds
        U = torch.empty((m, max(k, 1)), dtype=torch.float64, device=dev)
        W = torch.empty((max(k, 1), n), dtype=torch.float64, device=dev)
        if k:
            _capi.check(call(U, W, k))
            seconds += info.seconds
        U, W = U[:, :k], W[:k]
    d = info.as_dict()
    d["seconds"] = seconds
    sig = sigma[:min(m, n)]
    if host:
        return k, sig.cpu().numpy(), None if U is None else U.cpu().numpy(), None if W is None else W.cpu().numpy(), d
    return k, sig, U, W, d


class DeviceSvdFactorizer:
    """The streamer's truncated SVD (the contract `streamer_structure.Streamer` documents) on the device: the block is made
    dense on the host, uploaded, factorized by bfhipTruncSvdDevice, and U, W = S V^T are downloaded.  record: an optional list
    that receives (m, n, k, sweeps, seconds) per call, seconds being the device calls' own wall clock.  max_sweeps: the cap of
    every call (None: the library's 30); a block that does not converge within it raises, it is never answered silently."""

    def __init__(self, tol=1e-3, device=0, record=None, max_sweeps=None):
        self.tol, self.device, self.record, self.max_sweeps = float(tol), int(device), record, max_sweeps
        self.seconds = 0.0

    def svd(self, block, row_node, col_node, tree):
        a = densify(block)
        k, sigma, U, W, info = truncated_svd_device(a, self.tol, self.device, max_sweeps=self.max_sweeps)
        self.seconds += info["seconds"]
        if self.record is not None:
            self.record.append((a.shape[0], a.shape[1], k, int(info["sweeps"]), float(info["seconds"])))
        return k, len(sigma), ss.Dense(a.shape[0], k, np.ascontiguousarray(U)), ss.Dense(k, a.shape[1], np.ascontiguousarray(W))


def stream_butterfly(points, phi, freqs, wmax, freq_depth=None, tol=1e-3, wmin=0.0, min_rows=20, min_cols=20, max_cols=None, factorizer=None,
                     device=0, dtype="f64", check_columns=0, **compile_opts):
    """The butterfly of Phi from its columns: (HipOperator, row_perm, info).

    points [N, 3]; phi [N, J], rows in the order of `points`, numpy or a torch tensor on the GPU (any row stride: what
    ChebCovariance.eigs_bands returns) -- it is copied to the host once; freqs [J] ascending (sqrt of the eigenvalues,
    src/lbo.c:20-30); the frequency tree spans [wmin, wmax] with `freq_depth` levels (None: the row tree's depth - 3,
    lbo_cov.c:97-98), its two outermost leaves open-ended (src/lbo.c:41-68).  The loop is lbo_cov.c:139-143: Octree(points, 1),
    the rows put in tree order, then per leaf band feed; it stops when the tree is exhausted or `max_cols` columns went in.
    Then get_mat, to_desc, HipOperator.from_desc.  The operator's rows are in TREE order: row_perm (int64 [N]) is the
    permutation cov_sample_block_device and cov_condition take (row i of the operator is point row_perm[i]).

    factorizer: None for DeviceSvdFactorizer(tol, device); any object with the streamer's .svd is accepted.  dtype "f64" or
    "f32" (the leaves demoted at compile time).  compile_opts go to HipOperator.from_desc (flags, max_rhs, ...).
    check_columns = c > 0 adds the streamer's own acceptance figure (src/fac_streamer.c:286-301) to info: the relative error
    of the operator on c standard-normal vectors against the dense Phi, on the host.

    The recursion and the block algebra run on the host in Python, the SVDs on the GPU (see the module's docstring).
    info: the streamer's counters ("svds", "merges", "feeds"), "columns", "freq_depth", "leaf_bytes", "svd_records" (the
    factorizer's list, when it keeps one), "svd_seconds" (the device factorizer's own sum), "seconds" (the whole build),
    "host_seconds" = seconds - svd_seconds, "compile_seconds", "desc" and "leaf_values" (what was compiled)."""
    from .operator import HipOperator
    t0 = time.perf_counter()
    if dtype not in ("f64", "f32"):
        raise ValueError("dtype: 'f64' or 'f32'")
    pts = np.ascontiguousarray(points, dtype=np.float64)
    phi_h = phi if isinstance(phi, np.ndarray) else phi.detach().cpu().numpy()
    phi_h = np.asarray(phi_h, dtype=np.float64)
    freqs = np.asarray(freqs, dtype=np.float64)
    if phi_h.ndim != 2 or phi_h.shape[0] != len(pts) or phi_h.shape[1] != len(freqs):
        raise ValueError("phi must be [len(points), len(freqs)]")
    tree = ss.Octree(pts, 1)
    if freq_depth is None:
        freq_depth = tree.max_depth - 3                    # examples/covariance/lbo_cov.c:97-98
    if freq_depth < 0:
        raise ValueError("freq_depth is negative: too few points for the default (row-tree depth - 3)")
    record = None
    if factorizer is None:
        record = []
        factorizer = DeviceSvdFactorizer(tol, device, record)
    else:
        record = getattr(factorizer, "record", None)
    st = ss.Streamer(tree, int(freq_depth), factorizer, min_rows, min_cols, 0)
    a_phi = np.ascontiguousarray(phi_h[tree.perm])
    j0, J = 0, phi_h.shape[1]
    while not st.is_done():
        leaf = st.current_col_node()
        a, b, left, right = st.cols.leaf_interval(leaf, wmin, wmax)        # bfIntervalTreeInitEmpty(tree, a, b, 2, depth)
        lo = -np.inf if left else a
        hi = np.inf if right else b
        j1 = j0
        while j1 < J and lo <= freqs[j1] < hi:
            j1 += 1
        st.feed(ss.Dense(len(pts), j1 - j0, a_phi[:, j0:j1]))
        j0 = j1
        if max_cols is not None and j0 >= max_cols:
            break
    graph = st.get_mat()
    desc, vals = ss.to_desc(graph)
    t1 = time.perf_counter()
    op = HipOperator.from_desc(desc, vals, device=device, demote_to_f32=dtype == "f32", **compile_opts)
    t2 = time.perf_counter()
    info = dict(st.stats)
    info.update(columns=j0, freq_depth=int(freq_depth), leaf_bytes=ss.graph_stats(graph)["leafBytes"], svd_records=record,
                svd_seconds=float(getattr(factorizer, "seconds", 0.0)), compile_seconds=t2 - t1, desc=desc, leaf_values=vals)
    if check_columns:
        x = np.random.default_rng(0).standard_normal((j0, int(check_columns)))
        want = a_phi[:, :j0] @ x
        got = np.asarray(op.apply_host(x), dtype=np.float64)
        info["acceptance"] = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    info["seconds"] = time.perf_counter() - t0
    info["host_seconds"] = info["seconds"] - info["svd_seconds"]
    return op, tree.perm.astype(np.int64), info
