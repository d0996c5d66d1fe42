"""The sharded C-ABI step (butterfly_amd/csrc/bfhip_shard.hip) with 2, 3 and 5 ranks on ONE GPU.

The ranks are host threads of one child process; libbfhip.so resolves its collectives from tests/native/stub_ccl.c
(BFHIP_RCCL_LIBRARY), an in-process stand-in whose all-gather is a device copy of every peer's slot and whose all-reduce
adds the ranks' buffers in rank order 0..W-1 in the buffer's own scalar type.  Everything the step does besides the
collective's transport -- slot arithmetic, the segment scatter / gather / sum kernels, the abort path, GMRES over the
sharded matvec -- is the product's own code.

This module is three things:
  * the numpy ASSEMBLY of what a step must return from each rank's operator applied alone (place_segments, range_sums,
    rank_order_sum, gather_rows) -- also checked against the oracle on the CPU (tests/test_shard_ranks_cpu.py);
  * the operands and partitions of the cases (complex_operand, real_operand, partition);
  * the child process (`python shard_ranks.py --stub LIB --case NAME --out FILE.npz`) and `run_child`, which the GPU
    tests use to start it.  A test starts ONE child per (dtype, mode); the child covers every world and nrhs of it.
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

WORLDS = (2, 3, 5)
REAL_WORLDS = (2, 3)
REAL_SEEDS = (33, 41)
REAL_BLOCK_ROWS, REAL_BLOCK_COLS = (85, 1, 130, 47, 99, 64), (37, 26)
REAL_BLOCK_OWNERS = {2: [0, 1, 0, 1, 0, 1], 3: [1, 2, 0, 1, 2, 0]}       # no rank owns one run of rows; row counts 314 / 112 and 194 / 132 / 100
NRHS = (1, 3)
MODES = ("rows", "rowblocks", "rowsum", "blocks")
DTYPES = {"c128": (np.complex128, False), "c64": (np.complex64, True), "f64": (np.float64, False), "f32": (np.float32, True)}
GMRES_N, GMRES_K, GMRES_TOL, GMRES_MAX_ITER = 2048, 128, 1e-9, 40
STUB_DEADLINE_SECONDS = 20
STUB_FUNCS = {"GetUniqueId": 0, "CommInitRank": 1, "CommDestroy": 2, "CommAbort": 3, "AllGather": 4, "AllReduce": 5}


# ---------------------------------------------------------------------------------------------------------------------
# the numpy assembly: what a sharded step returns, from every rank's operator applied alone
# ---------------------------------------------------------------------------------------------------------------------
def my_rows(layout, rank, mode):
    """Global row indices of rank's entries of a length-n vector, in the order its local operator holds them."""
    if mode == "blocks":
        return np.arange(layout.n, dtype=np.int64)
    parts = [np.arange(layout.row_offsets[rb], layout.row_offsets[rb] + layout.top_rows[rb], dtype=np.int64) for rb in layout.blocks_of[rank]]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def gather_rows(layout, rank, mode, v):
    """The rows of v the adjoint step hands rank's operator (bfGatherSegmentsKernel, or v in place for one run)."""
    return np.ascontiguousarray(v[my_rows(layout, rank, mode)])


def place_segments(layout, local):
    """rows / rowblocks: every rank's compact local result put at its global rows (each row has exactly one owner)."""
    y = np.empty((layout.n,) + local[0].shape[1:], dtype=local[0].dtype)
    filled = np.zeros(layout.n, dtype=bool)
    for r in range(layout.world):
        idx = my_rows(layout, r, "rows")
        assert local[r].shape[0] == len(idx) and not filled[idx].any()
        y[idx] = local[r]
        filled[idx] = True
    assert filled.all()
    return y


def range_sums(layout, local):
    """rowsum: a range with one owner is a copy; a shared range is ((p0 + p1) + ...) over the segment LIST order, added in
    the storage scalar type (numpy adds complex numbers part by part, in the parts' own precision)."""
    y = np.empty((layout.n,) + local[0].shape[1:], dtype=local[0].dtype)
    pos = [0] * layout.world
    seen = set()
    for rb, r in layout.segments:
        g0, m = int(layout.row_offsets[rb]), layout.top_rows[rb]
        part = local[r][pos[r]:pos[r] + m]
        assert part.shape[0] == m
        pos[r] += m
        y[g0:g0 + m] = (y[g0:g0 + m] + part) if rb in seen else part
        seen.add(rb)
    assert all(pos[r] == local[r].shape[0] for r in range(layout.world)) and len(seen) == len(layout.top_rows)
    return y


def rank_order_sum(partials):
    """blocks, and every adjoint: the full-length partials added in rank order 0..W-1 in the storage scalar type."""
    acc = partials[0].copy()
    for p in partials[1:]:
        assert p.dtype == acc.dtype and p.shape == acc.shape
        acc = acc + p
    return acc


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(np.ravel(a).astype(np.complex128) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


# ---------------------------------------------------------------------------------------------------------------------
# operands and partitions
# ---------------------------------------------------------------------------------------------------------------------
class Operand:
    def __init__(self, desc, vals, seed, root=None):
        self.desc, self.vals, self.seed = desc, vals, seed
        self.root = desc.root if root is None else root
        self.m, self.n = int(desc.rows[self.root]), int(desc.cols[self.root])
        self.cplx = desc.dtype == 0


def complex_operand():
    """1024 points on a circle, k = 64: 12 top-level block rows of 85 / 86 rows, 144 blocks; leaves seeded on the device."""
    from butterfly_amd import helm2_structure as hs
    desc, _ = hs.native_multilevel_structure(hs.circle_points(1024), 64.0)
    return Operand(desc, None, 5)


def real_operand(seed):
    """(operand, the generator right behind it: the cov_matvec vectors are drawn from it)."""
    import randgraph
    rng = np.random.default_rng(seed)
    desc, vals = randgraph.random_real_operand(rng, depth=3, size_hint=150)
    return Operand(desc, vals, 0), rng


def real_block_rows_operand():
    """A real 426 x 63 operand of 6 ragged block rows (one of a single row) by 2 block columns of dense leaves, with the block-row
    bookkeeping hs.shard_desc needs: dealt by REAL_BLOCK_OWNERS every rank's rows are several runs, so the adjoint step gathers
    them (bfGatherSegmentsKernel on 8- and 4-byte units; more than one workgroup of it)."""
    from butterfly_amd import helm2_structure as hs
    rng = np.random.default_rng(57)
    d, vals, ch, trb = hs.Desc(dtype=1), {}, [], []
    ro, co = np.concatenate([[0], np.cumsum(REAL_BLOCK_ROWS)]), np.concatenate([[0], np.cumsum(REAL_BLOCK_COLS)])
    for i, m in enumerate(REAL_BLOCK_ROWS):
        for j, n in enumerate(REAL_BLOCK_COLS):
            node = d.add(hs.NODE_DENSE, m, n)
            vals[node] = rng.standard_normal((m, n)) / np.sqrt(n)
            ch.append((node, int(ro[i]), int(co[j])))
            trb.append(i)
    d.root = d.add(hs.NODE_BLOCK, int(ro[-1]), int(co[-1]), ch, hs.BF_TYPE_BLOCK_DENSE)
    d.top_row_block, d.meta = trb, dict(top_rows=list(REAL_BLOCK_ROWS))
    return Operand(d, vals, 0)


def gmres_operand():
    """I + alpha S on the unit circle (tests/bie.py), N = 2048."""
    import bie
    desc, root, vals, dense = bie.second_kind_case(GMRES_N, GMRES_K)
    return Operand(desc, vals, 0, root=root)


def _leaf_elems(desc, node):
    from butterfly_amd import helm2_structure as hs
    tot, stack = 0, [node]
    while stack:
        v = stack.pop()
        if desc.kind[v] == hs.NODE_DENSE:
            tot += int(desc.rows[v]) * int(desc.cols[v])
        stack.extend(c for c, _, _ in desc.children[v])
    return tot


def partition(opd, mode, world, owner=None):
    """(ShardLayout, [per rank: dict(root=, row_range=)]) of `opd` dealt to `world` ranks in `mode`.  Adds the shards' root
    nodes to the descriptor: call it on one thread.  owner (rowblocks only): deal the block rows this way instead of LPT."""
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.dist import (ShardLayout, assign_row_blocks, block_weights, row_block_weights, row_partition,
                                    rowsum_partition)
    desc = opd.desc
    if mode == "rows":
        cuts, _ = row_partition(desc, world, root=None if opd.root == desc.root else opd.root)
        layout = ShardLayout([cuts[r + 1] - cuts[r] for r in range(world)], list(range(world)), world)
        layout.cuts = cuts
        return layout, [dict(root=opd.root, row_range=(cuts[r], cuts[r + 1])) for r in range(world)]
    if opd.root != desc.root:
        # (row, col) blocks of a root other than the descriptor's own (I + alpha S): dealt by LPT on leaf elements
        assert mode == "blocks"
        ch = desc.children[opd.root]
        bowner, _ = assign_row_blocks([_leaf_elems(desc, c) for c, _, _ in ch], world)
        layout = ShardLayout([opd.m], [0], world)
        roots = [desc.add(hs.NODE_BLOCK, opd.m, opd.n, [ch[i] for i in range(len(ch)) if bowner[i] == r], hs.BF_TYPE_BLOCK_DENSE) for r in range(world)]
        return layout, [dict(root=rt, row_range=None) for rt in roots]
    top_rows = desc.meta["top_rows"]
    if mode == "rowblocks":
        if owner is None:
            owner, _ = assign_row_blocks(row_block_weights(desc), world)
        layout = ShardLayout(top_rows, owner, world)
        shards = []
        for r in range(world):
            root, rows = hs.shard_desc(desc, layout.blocks_of[r])
            assert rows == layout.rows_of[r]
            shards.append(dict(root=root, row_range=None))
        return layout, shards
    if mode == "rowsum":
        bowner, _, segs = rowsum_partition(desc, world)
        layout = ShardLayout(top_rows, [0] * len(top_rows), world, segments=segs)
        shards = []
        for r in range(world):
            root, touched, rows = hs.shard_desc_children(desc, [i for i in range(len(bowner)) if bowner[i] == r])
            assert rows == layout.rows_of[r] and touched == layout.blocks_of[r]
            shards.append(dict(root=root, row_range=None))
        return layout, shards
    assert mode == "blocks"
    bowner, _ = assign_row_blocks(block_weights(desc), world)
    layout = ShardLayout(top_rows, [0] * len(top_rows), world)
    return layout, [dict(root=hs.shard_desc_blocks(desc, [i for i in range(len(bowner)) if bowner[i] == r]), row_range=None) for r in range(world)]


def vectors(opd, np_dtype, nrhs, seed):
    """(x [n(, nrhs)], v [m(, nrhs)]) in the storage type: the right-hand sides of the forward and the adjoint step."""
    rng = np.random.default_rng(seed)

    def draw(rows):
        shape = (rows,) if nrhs == 1 else (rows, nrhs)
        a = rng.standard_normal(shape)
        if opd.cplx:
            a = (a + 1j * rng.standard_normal(shape)) / np.sqrt(2)
        return np.ascontiguousarray(a.astype(np_dtype))
    return draw(opd.n), draw(opd.m)


def cov_inputs(opd, rng, np_dtype):
    """gamma, the row permutation with its inverse, and v of the cov_matvec case (as the one-rank test draws them)."""
    gam = (rng.random(opd.n) + 0.1).astype(np_dtype)
    row_perm = rng.permutation(opd.m).astype(np.int64)
    rev = np.empty(opd.m, dtype=np.int64)
    rev[row_perm] = np.arange(opd.m)
    return gam, row_perm, rev, rng.standard_normal(opd.m).astype(np_dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the child process
# ---------------------------------------------------------------------------------------------------------------------
class IdBox:
    """Ships the 128-byte communicator id from rank 0's thread to the others (RcclShardedApply's `bcast`)."""

    def __init__(self):
        import threading
        self._ev, self.value = threading.Event(), None

    def __call__(self, payload):
        if payload is not None:
            self.value = payload
            self._ev.set()
            return payload
        if not self._ev.wait(60):
            raise TimeoutError("rank 0 never published the communicator id")
        return self.value


def run_ranks(world, body, join_seconds=200):
    """body(rank) on one thread per rank, each with its own torch stream; returns the list of results.  An exception on a
    rank is re-raised here once every thread has ended; a thread that does not end is a deadlock: the process exits."""
    import threading
    import traceback

    import torch
    results, errors = [None] * world, [None] * world

    def main(r):
        try:
            torch.cuda.set_device(0)
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                results[r] = body(r)
                stream.synchronize()
        except BaseException:
            errors[r] = traceback.format_exc()
    threads = [threading.Thread(target=main, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    import time
    deadline = time.monotonic() + join_seconds            # ONE bound for all ranks, below the parent's 300 s
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in threads):
        sys.stderr.write(f"shard_ranks: ranks {[r for r, t in enumerate(threads) if t.is_alive()]} of {world} did not return\n")
        sys.stderr.flush()
        os._exit(3)
    bad = [f"rank {r}:\n{e}" for r, e in enumerate(errors) if e]
    if bad:
        raise RuntimeError("\n".join(bad))
    return results


def _compile(opd, shard, demote, max_rhs, adjoint=True):
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    return HipOperator.from_desc(opd.desc, opd.vals, root=shard["root"], seed=opd.seed, max_rhs=max_rhs, device=0,
                                 flags=_capi.FLAG_ADJOINT if adjoint else 0, demote_to_f32=demote, row_range=shard["row_range"])


def _apply_operand(out, tag, opd, dtype, mode, worlds, owners=None):
    """Forward and adjoint steps of one operand in one mode: every world, nrhs 1 and 3.  Records, per (world, nrhs, rank):
    the step's y and z, and the rank's operator applied ALONE (its compact rows; its partial A_r^T v_r)."""
    import torch
    from butterfly_amd.dist import RcclShardedApply
    np_dtype, demote = DTYPES[dtype]
    dev = torch.device("cuda", 0)
    vec = {nrhs: tuple(torch.from_numpy(a).to(dev) for a in vectors(opd, np_dtype, nrhs, 100 + nrhs)) for nrhs in NRHS}
    full = _compile(opd, dict(root=opd.root, row_range=None), demote, max(NRHS))
    for nrhs in NRHS:
        x, v = vec[nrhs]
        out[f"{tag}_n{nrhs}_full_y"] = full.apply_device(x).cpu().numpy()
        out[f"{tag}_n{nrhs}_full_z"] = full.apply_transpose_device(v).cpu().numpy()
    full.close()
    torch.cuda.synchronize()
    for world in worlds:
        layout, shards = partition(opd, mode, world, owner=owners.get(world) if owners else None)
        boxes = {nrhs: IdBox() for nrhs in NRHS}
        rows_idx = [torch.from_numpy(my_rows(layout, r, mode)).to(dev) for r in range(world)]
        torch.cuda.synchronize()

        def body(rank):
            op = _compile(opd, shards[rank], demote, max(NRHS))
            res = {}
            for nrhs in NRHS:
                x, v = vec[nrhs]
                step = RcclShardedApply(layout, rank, op, 0, nrhs=nrhs, mode=mode, bcast=boxes[nrhs])
                vr = v.index_select(0, rows_idx[rank]).contiguous()
                if vr.shape[0]:
                    res[f"n{nrhs}_r{rank}_loc_y"] = op.apply_device(x).cpu().numpy()
                    res[f"n{nrhs}_r{rank}_loc_z"] = op.apply_transpose_device(vr).cpu().numpy()
                else:
                    # a rank without rows: its operator alone has nothing to write (an empty tensor's pointer is NULL, which
                    # bfhipApplyDevice refuses), so its rows are none and its adjoint partial is zeros
                    res[f"n{nrhs}_r{rank}_loc_y"] = np.zeros((0,) + tuple(x.shape[1:]), dtype=np_dtype)
                    res[f"n{nrhs}_r{rank}_loc_z"] = np.zeros((opd.n,) + tuple(v.shape[1:]), dtype=np_dtype)
                res[f"n{nrhs}_r{rank}_y"] = step(x).cpu().numpy()
                res[f"n{nrhs}_r{rank}_z"] = step.apply_transpose(v).cpu().numpy()
                res[f"n{nrhs}_r{rank}_y_again"] = step(x).cpu().numpy()
                step.close()
            op.close()
            return res
        for res in run_ranks(world, body):
            for k, a in res.items():
                out[f"{tag}_w{world}_{k}"] = a


def case_apply(out, dtype, mode):
    if dtype in ("c128", "c64"):
        _apply_operand(out, "c", complex_operand(), dtype, mode, WORLDS)
        return
    if mode == "rowblocks":
        _apply_operand(out, "b", real_block_rows_operand(), dtype, mode, REAL_WORLDS, owners=REAL_BLOCK_OWNERS)
        return
    assert mode == "rows"
    import torch
    from butterfly_amd.dist import RcclShardedApply
    np_dtype, demote = DTYPES[dtype]
    dev = torch.device("cuda", 0)
    for seed in REAL_SEEDS:
        opd, rng = real_operand(seed)
        _apply_operand(out, f"s{seed}", opd, dtype, mode, REAL_WORLDS)
        # cov_matvec over the sharded operator: z = P A G G A^T P' v (bfhipShardedCovMatvecDevice)
        gam, row_perm, rev, v = cov_inputs(opd, rng, np_dtype)
        dgam, dperm, drev, dv = (torch.from_numpy(a).to(dev) for a in (gam, row_perm, rev, v))
        for world in REAL_WORLDS:
            layout, shards = partition(opd, "rows", world)
            box = IdBox()
            torch.cuda.synchronize()

            def body(rank):
                op = _compile(opd, shards[rank], demote, 1)
                step = RcclShardedApply(layout, rank, op, 0, nrhs=1, mode="rows", bcast=box)
                z = step.cov_matvec(dgam, dperm, drev, dv).cpu().numpy()
                step.close()
                op.close()
                return z
            for r, z in enumerate(run_ranks(world, body)):
                out[f"s{seed}_w{world}_r{r}_cov"] = z


def case_norows(out):
    """World 3 over whole block rows with rank 2 owning none: its operator has zero rows."""
    _apply_operand(out, "c", complex_operand(), "c128", "rowblocks", (3,), owners={3: [0, 1] * 6})


def case_gmres(out, mode):
    import torch
    from butterfly_amd import _capi
    from butterfly_amd.dist import RcclShardedApply
    opd = gmres_operand()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4)
    rhs = {}
    for nrhs in (1, 2):
        b = rng.standard_normal((opd.n, nrhs)) + 1j * rng.standard_normal((opd.n, nrhs))
        rhs[nrhs] = np.ascontiguousarray(b[:, 0] if nrhs == 1 else b)
        out[f"b_n{nrhs}"] = rhs[nrhs]
    drhs = {nrhs: torch.from_numpy(b).to(dev) for nrhs, b in rhs.items()}
    orths = (("mgs", _capi.GMRES_ORTH_MGS), ("cgs2", _capi.GMRES_ORTH_CGS2))
    full = _compile(opd, dict(root=opd.root, row_range=None), False, 2, adjoint=False)
    for nrhs in (1, 2):
        for name, _ in orths:
            x, it, res = full.solve_gmres_device(drhs[nrhs], tol=GMRES_TOL, max_num_iter=GMRES_MAX_ITER, orth=name)
            out[f"full_n{nrhs}_{name}_x"], out[f"full_n{nrhs}_{name}_it"], out[f"full_n{nrhs}_{name}_res"] = x.cpu().numpy(), it, res
    full.close()
    for world in (2, 3):
        layout, shards = partition(opd, mode, world)
        box = IdBox()
        torch.cuda.synchronize()

        def body(rank):
            op = _compile(opd, shards[rank], False, 2, adjoint=False)
            step = RcclShardedApply(layout, rank, op, 0, nrhs=2, mode=mode, bcast=box)
            res = {}
            for nrhs in (1, 2):
                for name, orth in orths:
                    x, it, r = step.solve_gmres(drhs[nrhs], tol=GMRES_TOL, max_num_iter=GMRES_MAX_ITER, orthogonalization=orth)
                    res[f"n{nrhs}_{name}_r{rank}_x"], res[f"n{nrhs}_{name}_r{rank}_it"], res[f"n{nrhs}_{name}_r{rank}_res"] = x.cpu().numpy(), it, r
            step.close()
            op.close()
            return res
        for res in run_ranks(world, body):
            for k, a in res.items():
                out[f"w{world}_{k}"] = a


def _stub_lib(path):
    import ctypes as C
    lib = C.CDLL(path)                     # the copy libbfhip.so opened: one instance, one table of worlds
    lib.stubCclFailNext.argtypes, lib.stubCclFailNext.restype = [C.c_char_p, C.c_int], C.c_int
    lib.stubCclCalls.argtypes, lib.stubCclCalls.restype = [C.c_char_p, C.c_int, C.c_int], C.c_long
    return lib


def _counters(stub, ident, world):
    return np.array([[stub.stubCclCalls(ident, r, f) for f in range(len(STUB_FUNCS))] for r in range(world)], dtype=np.int64)


def case_abort(out, stub_path):
    """World 3, rows: rank 1's next all-gather fails on the host (the stub returns an error code; nothing on the GPU is
    made to fault).  Records every rank's return code, message and time for that step and for the next one."""
    import threading
    import time

    import torch
    from butterfly_amd import _capi
    from butterfly_amd.dist import RcclShardedApply
    stub = _stub_lib(stub_path)
    opd = complex_operand()
    world = 3
    layout, shards = partition(opd, "rows", world)
    x = torch.from_numpy(vectors(opd, np.complex128, 1, 7)[0]).to("cuda:0")
    box, ready = IdBox(), threading.Barrier(world, timeout=120)
    torch.cuda.synchronize()

    def attempt(step):
        t0 = time.monotonic()
        try:
            step(x)
            return 0, "", time.monotonic() - t0
        except _capi.BfhipError as e:
            return e.code, str(e), time.monotonic() - t0

    def body(rank):
        op = _compile(opd, shards[rank], False, 1)
        step = RcclShardedApply(layout, rank, op, 0, nrhs=1, mode="rows", bcast=box)
        good = step(x).cpu().numpy()              # a first step goes through on every rank
        ready.wait()
        if rank == 1:
            assert stub.stubCclFailNext(box.value, 1) == 0
        first, second = attempt(step), attempt(step)
        step.close()                               # bfhipShardedFree, then bfhipCommDestroy on the aborted communicator
        op.close()
        return good, first, second
    res = run_ranks(world, body)
    out["codes"] = np.array([[r[1][0], r[2][0]] for r in res], dtype=np.int64)
    out["seconds"] = np.array([[r[1][2], r[2][2]] for r in res])
    out["messages"] = np.array([[r[1][1], r[2][1]] for r in res])
    out["good_agree"] = np.array([same_bits(r[0], res[0][0]) for r in res])
    out["calls"] = _counters(stub, box.value, world)


def case_refuse(out, stub_path):
    """Create-time refusals with three ranks: (a) rank 2 brings an operator whose row count is not its segments' (rank 1's
    shard: 340 rows for 342), (b) rank 1 is handed an owner list that names rank 3.  The other ranks create their step."""
    import torch
    from butterfly_amd import _capi
    from butterfly_amd.dist import RcclShardedApply, ShardLayout
    stub = _stub_lib(stub_path)
    opd = complex_operand()
    world = 3
    layout, shards = partition(opd, "rows", world)
    assert layout.rows_of[1] != layout.rows_of[2]
    bad_owner = ShardLayout(layout.top_rows, [0, 1, 3], world)
    for name, shard_of, layout_of in (("rows", lambda r: shards[1] if r == 2 else shards[r], lambda r: layout),
                                      ("owner", lambda r: shards[r], lambda r: bad_owner if r == 1 else layout)):
        box = IdBox()
        torch.cuda.synchronize()

        def body(rank):
            op = _compile(opd, shard_of(rank), False, 1)
            try:
                step = RcclShardedApply(layout_of(rank), rank, op, 0, nrhs=1, mode="rows", bcast=box)
            except _capi.BfhipError as e:
                # (the refused rank's communicator, initialised before bfhipShardedCreate, goes with the child process)
                op.close()
                return e.code, str(e)
            step.close()
            op.close()
            return 0, ""
        res = run_ranks(world, body)
        out[f"{name}_codes"] = np.array([r[0] for r in res], dtype=np.int64)
        out[f"{name}_messages"] = np.array([r[1] for r in res])
        out[f"{name}_calls"] = _counters(stub, box.value, world)


def main(argv):
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--stub", required=True)
    ap.add_argument("--case", required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    os.environ["BFHIP_RCCL_LIBRARY"] = args.stub
    import ctypes as C

    import torch
    from butterfly_amd import _capi
    assert torch.cuda.is_available(), "the child needs a GPU"
    torch.cuda.set_device(0)
    # settle loadRccl's global before any thread exists
    _capi.check(_capi.load().bfhipCommGetUniqueId(C.create_string_buffer(128)))
    out = {}
    kind, _, rest = args.case.partition(":")
    if kind == "apply":
        case_apply(out, *rest.split(":"))
    elif kind == "norows":
        case_norows(out)
    elif kind == "gmres":
        case_gmres(out, rest)
    elif kind == "abort":
        case_abort(out, args.stub)
    elif kind == "refuse":
        case_refuse(out, args.stub)
    else:
        raise SystemExit(f"unknown case {args.case}")
    torch.cuda.synchronize()
    np.savez(args.out, **out)
    return 0


# ---------------------------------------------------------------------------------------------------------------------
# what the tests call
# ---------------------------------------------------------------------------------------------------------------------
STUB_SOURCE = os.path.join(HERE, "native", "stub_ccl.c")


def compile_stub(out_dir, shared=True):
    """gcc tests/native/stub_ccl.c into out_dir (-Wall -Werror); shared=False stops at the object file (no HIP library needed)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    base = ["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), STUB_SOURCE]
    if not shared:
        path = os.path.join(str(out_dir), "stub_ccl.o")
        subprocess.check_call(base + ["-c", "-o", path])
        return path
    path = os.path.join(str(out_dir), "libstub_ccl.so")
    subprocess.check_call(base + ["-shared", "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-lpthread", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", path])
    return path


def run_child(stub, case, out_dir):
    """One child process for `case`; returns the loaded .npz.  Not retried; the bound is the plain-C example's."""
    path = os.path.join(str(out_dir), case.replace(":", "_") + ".npz")
    env = dict(os.environ, STUB_CCL_DEADLINE_SECONDS=str(STUB_DEADLINE_SECONDS))       # the tests' time bounds are against THIS deadline
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--stub", stub, "--case", case, "--out", path],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert p.returncode == 0, f"child {case} exited {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-6000:]}"
    return np.load(path)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
