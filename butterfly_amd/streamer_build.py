"""Eigenbands to the butterfly of Phi, with the truncated SVDs on the device.

Step 2 of the reference's covariance pipeline (examples/covariance/lbo_cov.c:139-143, src/lbo.c:41-150): the eigenvector
columns are fed, leaf band by leaf band of the frequency tree, to the streamer (`streamer_structure.Streamer`, the
restatement of bfFacStreamerFeed and its merge-and-split recursion), whose one numerical step is a truncated SVD.

WHERE EACH PART RUNS.  The block algebra, the recursion, the conversion of a block to a dense matrix and the flat
descriptor stay on the host, in Python.  The GPU does the SVDs (`bfhipTruncSvdDevice`: one-sided block Jacobi on the FP64
matrix cores) and, afterwards, everything the compiled `HipOperator` is used for.  Every SVD is one synchronous call with
an upload of the block and a download of U and W around it.  The end-to-end build is therefore bounded by Python at N = 1M;
this module serves the range N <= 65536, where the SVD-driven structure exists at all (DESIGN_EXPERIMENTS.md section 12).

BATCHED (`stream_butterfly(..., batched=True)`).  The answer of a row node's SVD decides only whether its
own children are visited, so all nodes of one depth of a feed, and of one merge across its whole cut, can be factorized
together: `FrontierStreamer` walks the row tree breadth first and hands every frontier to `DeviceSvdFactorizer.svd_many`, which
is ONE `bfhipTruncSvdBatchDevice` call with one upload and three downloads.  The factors are those of the depth-first walk bit
for bit; only the order of the factorizer's record differs.
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


def truncated_svd_batch_device(blocks, tol, device=0, max_sweeps=None, workspace_limit=None):
    """bfhipTruncSvdBatchDevice on a list of 2-D float64 numpy arrays: the blocks are packed into one host buffer and uploaded
    with one copy; sigma, U (room for min(m, n) columns each) and W live in one packed device buffer each, are filled by ONE
    call and come back with one copy each.  Returns [(k, sigma, U [m, k], W [k, n], info dict)] in the order of `blocks`, each
    bit for bit what `truncated_svd_device` returns for that block; info["seconds"] is the call's wall clock shared out by
    rows x columns, info["batch"] the call's own figures (count, groups, maxSweeps, launches, synchronisations, workspaceBytes,
    seconds), one dict shared by the batch.  A problem that fails raises BfhipError with its index in the message.
    workspace_limit: bytes of device workspace per group of problems (None: the library's 1 GiB).  A batch whose packed U and W,
    sum of (m + n) min(m, n), pass 2^27 doubles is served problem by problem through `truncated_svd_device` (the threshold at
    which that path stops giving U and W room for every term)."""
    blocks = [np.ascontiguousarray(b, dtype=np.float64) for b in blocks]
    if any(b.ndim != 2 for b in blocks):
        raise ValueError("blocks: 2-D arrays")
    count = len(blocks)
    if not count:
        return []
    shapes = [(int(b.shape[0]), int(b.shape[1])) for b in blocks]
    area = float(sum(m * n for m, n in shapes)) or 1.0
    if sum((m + n) * min(m, n) for m, n in shapes) > 1 << 27:
        out, total = [], 0.0
        for b in blocks:
            out.append(truncated_svd_device(b, tol, device, max_sweeps=max_sweeps))
            total += out[-1][4]["seconds"]
        batch = dict(count=count, groups=count, maxSweeps=max(r[4]["sweeps"] for r in out), launches=0, synchronisations=0, workspaceBytes=0,
                     seconds=total, fallback=True)
        for r in out:
            r[4]["batch"] = batch
        return out
    import torch
    dev = torch.device("cuda", int(device))
    lib = _capi.load()
    off_a = np.concatenate([[0], np.cumsum([m * n for m, n in shapes])]).astype(np.int64)
    off_s = np.concatenate([[0], np.cumsum([min(m, n) for m, n in shapes])]).astype(np.int64)
    off_u = np.concatenate([[0], np.cumsum([m * min(m, n) for m, n in shapes])]).astype(np.int64)
    off_w = np.concatenate([[0], np.cumsum([min(m, n) * n for m, n in shapes])]).astype(np.int64)
    d_a = torch.from_numpy(np.concatenate([b.ravel() for b in blocks])).to(dev)
    d_s = torch.empty(max(int(off_s[-1]), 1), dtype=torch.float64, device=dev)
    d_u = torch.empty(max(int(off_u[-1]), 1), dtype=torch.float64, device=dev)
    d_w = torch.empty(max(int(off_w[-1]), 1), dtype=torch.float64, device=dev)
    probs = (_capi.BfhipTruncSvdProblem * count)()
    infos = (_capi.BfhipTruncSvdInfo * count)()
    status = (C.c_int32 * count)()
    pa, ps, pu, pw = d_a.data_ptr(), d_s.data_ptr(), d_u.data_ptr(), d_w.data_ptr()
    for i, (m, n) in enumerate(shapes):
        N = min(m, n)
        p = probs[i]
        p.dA, p.m, p.n, p.lda = pa + 8 * int(off_a[i]), m, n, n
        p.dSigma = ps + 8 * int(off_s[i])
        p.dU, p.ldu, p.capU = pu + 8 * int(off_u[i]), N, N
        p.dW, p.ldw, p.capW = pw + 8 * int(off_w[i]), n, N
        infos[i].structSize = C.sizeof(_capi.BfhipTruncSvdInfo)
    opt = _capi.BfhipTruncSvdOptions()
    opt.structSize, opt.tol, opt.maxSweeps = C.sizeof(opt), float(tol), 0 if max_sweeps is None else int(max_sweeps)
    bi = _capi.BfhipTruncSvdBatchInfo()
    bi.structSize = C.sizeof(bi)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _capi.check(lib.bfhipTruncSvdBatchDevice(int(device), probs, count, C.byref(opt), 0 if workspace_limit is None else int(workspace_limit), infos, status,
                                             C.byref(bi), stream))
    sig, U, W = d_s.cpu().numpy(), d_u.cpu().numpy(), d_w.cpu().numpy()
    batch = bi.as_dict()
    batch["count"] = count
    out = []
    for i, (m, n) in enumerate(shapes):
        N, k = min(m, n), int(infos[i].k)
        d = infos[i].as_dict()
        d["seconds"] = bi.seconds * (m * n) / area
        d["batch"] = batch
        out.append((k, sig[off_s[i]:off_s[i + 1]].copy(), U[off_u[i]:off_u[i + 1]].reshape(m, N)[:, :k].copy(),
                    W[off_w[i]:off_w[i + 1]].reshape(N, n)[:k].copy(), d))
    return out


class DeviceSvdFactorizer:
    """The streamer's truncated SVD (the contract `streamer_structure.Streamer` documents) on the device: the block is made
    dense on the host, uploaded, factorized by bfhipTruncSvdDevice, and U, W = S V^T are downloaded.  record: an optional list
    that receives (m, n, k, sweeps, seconds) per call, seconds being the device calls' own wall clock.  max_sweeps: the cap of
    every call (None: the library's 30); a block that does not converge within it raises, it is never answered silently.
    svd_many serves a whole frontier of the breadth-first streamer with one bfhipTruncSvdBatchDevice call; batch_record receives
    (count, launches, synchronisations, seconds) per such call."""

    def __init__(self, tol=1e-3, device=0, record=None, max_sweeps=None, workspace_limit=None):
        self.tol, self.device, self.record, self.max_sweeps = float(tol), int(device), record, max_sweeps
        self.workspace_limit = workspace_limit
        self.seconds = 0.0
        self.batch_record = []

    def svd(self, block, row_node, col_node, tree):
        a = densify(block)
        k, sigma, U, W, info = truncated_svd_device(a, self.tol, self.device, max_sweeps=self.max_sweeps)
        self.seconds += info["seconds"]
        if self.record is not None:
            self.record.append((a.shape[0], a.shape[1], k, int(info["sweeps"]), float(info["seconds"])))
        return k, len(sigma), ss.Dense(a.shape[0], k, np.ascontiguousarray(U)), ss.Dense(k, a.shape[1], np.ascontiguousarray(W))


    def svd_many(self, requests):
        """requests: [(block, row_node, col_node, tree)]; returns [(k, numSingular, U, W)] in their order, each what `.svd` gives."""
        dense = [densify(r[0]) for r in requests]
        res = truncated_svd_batch_device(dense, self.tol, self.device, max_sweeps=self.max_sweeps, workspace_limit=self.workspace_limit)
        out = []
        for a, (k, sigma, U, W, info) in zip(dense, res):
            if self.record is not None:
                self.record.append((a.shape[0], a.shape[1], k, int(info["sweeps"]), float(info["seconds"])))
            out.append((k, len(sigma), ss.Dense(a.shape[0], k, np.ascontiguousarray(U)), ss.Dense(k, a.shape[1], np.ascontiguousarray(W))))
        if res:
            b = res[0][4]["batch"]
            self.seconds += b["seconds"]
            self.batch_record.append((len(res), int(b["launches"]), int(b["synchronisations"]), float(b["seconds"])))
        return out


class FrontierStreamer(ss.Streamer):
    """`streamer_structure.Streamer` with the row tree walked breadth first: the SVDs of one depth of a feed, and of one depth of
    a merge across all nodes of its cut, are independent (a node's answer decides only whether its own children are visited),
    so each frontier goes to `factorizer.svd_many(requests)` in one call.  Every rule is the base class's -- the skinny and
    short blocks answered without an SVD, the sparsity fix, `truncated and compressed` -- and the partial factorizations are
    those of the depth-first walk; `stats` counts as the base class does.  A factorizer without `svd_many` is served by `.svd`
    per request."""

    def _svd_many(self, requests):
        if not requests:
            return []
        many = getattr(self.fz, "svd_many", None)
        res = many(requests) if many is not None else [self.fz.svd(*r) for r in requests]
        self.stats["svds"] += len(requests)
        return res

    def feed(self, phi):
        col_node = self.current_col_node()
        assert self.cols.is_leaf(col_node)
        t = self.tree
        if phi.m != t.num_points:
            raise ValueError("Phi has the wrong number of rows")
        done, frontier = {}, list(t.level(self.init_depth))
        while frontier:
            reqs, nodes = [], []
            for v in frontier:
                i0, i1 = int(t.first[v]), int(t.last[v])
                block = phi.row_range_copy(i0, i1)
                if phi.n < self.min_cols:                   # getPsiAndW_skinny
                    done[v] = (block.copy(), ss.Identity(phi.n))
                elif i1 - i0 < self.min_rows:
                    done[v] = (ss.Identity(i1 - i0), block.copy())
                else:
                    reqs.append((block, v, col_node, t))
                    nodes.append(v)
            frontier = []
            for v, (k, ns, U, SVt) in zip(nodes, self._svd_many(reqs)):
                if k < ns:
                    done[v] = (U, SVt)
                    continue
                kids = t.children(v)
                assert kids, "uncompressed leaf row node (src/fac_streamer.c:447)"
                frontier.extend(kids)
        row_nodes = sorted(done, key=lambda v: int(t.first[v]))
        self.partial.append(ss.Fac(col_node, row_nodes, ss.BlockDiag([done[v][0] for v in row_nodes]),
                                   [ss.BlockDense.col([done[v][1] for v in row_nodes])]))
        self.stats["feeds"] += 1
        self.pos += 1
        self._continue()

    def _merge_and_split(self, facs, col_node):
        num_w = len(facs[0].W)
        if any(len(f.W) != num_w for f in facs):
            raise RuntimeError("partial factorizations differ in depth (src/fac.c:1100-1106)")
        t = self.tree
        roots, stars, W1s = self._merge_cut(facs), [], []
        for v in roots:
            i0, i1 = int(t.first[v]), int(t.last[v])
            pw = [self._psi_w0_of_fac(f, i0, i1) for f in facs]
            stars.append(ss.BlockDense.row(p for p, _ in pw))
            W1s.append(ss.BlockDiag(w for _, w in pw))
            assert stars[-1].n == W1s[-1].m and stars[-1].m == t.rows(v)
        done = [{} for _ in roots]
        frontier = [(r, v) for r, v in enumerate(roots)]
        while frontier:
            reqs, where = [], []
            for r, v in frontier:
                i0 = int(t.first[roots[r]])
                sub = stars[r].row_range_copy(int(t.first[v]) - i0, int(t.last[v]) - i0)
                if sub.m < self.min_rows:
                    done[r][v] = (ss.Identity(sub.m), sub)
                elif sub.n < self.min_cols:
                    done[r][v] = (sub, ss.Identity(sub.n))
                else:
                    reqs.append((sub, v, col_node, t))
                    where.append((r, v))
            frontier = []
            for (r, v), (sub, _, _, _), (k, ns, U, W0) in zip(where, reqs, self._svd_many(reqs)):
                ranges = sub.nonzero_col_ranges()
                if len(ranges) > 1 or ranges[0][0] > 0 or ranges[0][1] < sub.n:          # shouldFixSparsity
                    W0 = ss.BlockCoo(W0.m, W0.n, [(0, j0, W0.col_range_copy(j0, j1)) for j0, j1 in ranges])
                if k < ns and W0.num_bytes() < sub.num_bytes():                          # truncated and compressed
                    done[r][v] = (U, W0)
                else:
                    frontier.extend((r, c) for c in t.children(v))
        row_nodes, Ps, W0s = [], [], []
        for r in range(len(roots)):
            cut = sorted(done[r], key=lambda v: int(t.first[v]))
            row_nodes += cut
            Ps.append(ss.BlockDiag([done[r][v][0] for v in cut]))
            W0s.append(ss.BlockDense.col([done[r][v][1] for v in cut]))
        W = [ss.BlockDiag(W0s), ss.BlockDense.col(W1s)]
        for k in range(1, num_w):
            W.append(ss.BlockDiag(f.W[k] for f in facs))
        return ss.Fac(col_node, row_nodes, ss.BlockDiag(Ps), W)


def stream_butterfly(points, phi, freqs, wmax, freq_depth=None, tol=1e-3, wmin=0.0, min_rows=20, min_cols=20, max_cols=None, factorizer=None,
                     device=0, dtype="f64", check_columns=0, batched=False, **compile_opts):
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

    batched=True walks the row tree breadth first (`FrontierStreamer`): one bfhipTruncSvdBatchDevice call per frontier instead of
    one bfhipTruncSvdDevice call per row node; the operator is the same bit for bit, only the order of "svd_records" differs;
    info gains "svd_batches": the factorizer's (count, launches, synchronisations, seconds) per call.

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
    st = (FrontierStreamer if batched else ss.Streamer)(tree, int(freq_depth), factorizer, min_rows, min_cols, 0)
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
    if batched:
        info["svd_batches"] = getattr(factorizer, "batch_record", None)
    if check_columns:
        x = np.random.default_rng(0).standard_normal((j0, int(check_columns)))
        want = a_phi[:, :j0] @ x
        got = np.asarray(op.apply_host(x), dtype=np.float64)
        info["acceptance"] = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    info["seconds"] = time.perf_counter() - t0
    info["host_seconds"] = info["seconds"] - info["svd_seconds"]
    return op, tree.perm.astype(np.int64), info
