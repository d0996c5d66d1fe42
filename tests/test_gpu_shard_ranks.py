"""The multi-GPU step of the C-ABI (butterfly_amd/csrc/bfhip_shard.hip) with 2, 3 and 5 ranks on one GPU.

Every other GPU test that reaches bfhipSharded* uses a 1-rank communicator, where `owner * maxRows`, the slot base, unequal
row counts, interleaved ownership, several sources per sum group and the abort path are all degenerate.  Here the ranks
are threads of ONE child process per test (tests/shard_ranks.py) over an in-process stand-in for the collectives
(tests/native/stub_ccl.c, named through BFHIP_RCCL_LIBRARY).  The three segment kernels are copies and fixed-order sums
and the stub's all-reduce adds in rank order in the storage type, so the expected results are assembled in numpy from each
rank's operator applied ALONE and compared BIT FOR BIT; the higher-precision checks use the tolerances the project already
has for these operands (1e-12 for f64 / c128, 2e-5 for f32 / c64, 1e-8 for the GMRES solution).

Not covered: RCCL's own transport over xGMI, and any scaling figure."""
import functools

import numpy as np
import pytest

import shard_ranks as sr

pytestmark = pytest.mark.gpu
TOL = {"c128": 1e-12, "f64": 1e-12, "c64": 2e-5, "f32": 2e-5}


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    return sr.compile_stub(tmp_path_factory.mktemp("stub_ccl"))


@functools.lru_cache(maxsize=None)
def _complex_reference():
    """The oracle's whole operator, once: A (for A x) and its dense form (the oracle cannot transpose this graph)."""
    from oracle import bfref
    opd = sr.complex_operand()
    A = bfref.from_desc(opd.desc, None, seed=opd.seed)
    dense = np.concatenate([bfref.mat_mul(A, np.eye(opd.n, 256, -c0, dtype=complex)) for c0 in range(0, opd.n, 256)], axis=1)
    return A, dense


@functools.lru_cache(maxsize=None)
def _real_reference(seed):
    from oracle import bfref
    opd, _ = sr.real_operand(seed)
    return bfref.from_desc(opd.desc, opd.vals)


@functools.lru_cache(maxsize=None)
def _real_block_rows_reference():
    from oracle import bfref
    opd = sr.real_block_rows_operand()
    return bfref.from_desc(opd.desc, opd.vals)


def _reference(opd, tag, x, v):
    """(A x, A^T v) of the whole operator from the oracle, in double precision, for the storage-type vectors x and v."""
    from oracle import bfref
    if opd.cplx:
        A, dense = _complex_reference()
        return bfref.mat_mul(A, x.astype(np.complex128)), dense.T @ v.astype(np.complex128)
    A = _real_block_rows_reference() if tag == "b" else _real_reference(int(tag[1:]))
    cols = lambda a: a[:, None] if a.ndim == 1 else a
    y = np.stack([bfref.mat_mul_vec(A, c) for c in cols(x.astype(np.float64)).T], axis=1)
    z = np.stack([bfref.mat_rmul_vec(A, c) for c in cols(v.astype(np.float64)).T], axis=1)
    return y.reshape((opd.m,) + x.shape[1:]), z.reshape((opd.n,) + v.shape[1:])


def _check_apply(data, tag, opd, dtype, mode, worlds, owners=None):
    np_dtype, _ = sr.DTYPES[dtype]
    for nrhs in sr.NRHS:
        x, v = sr.vectors(opd, np_dtype, nrhs, 100 + nrhs)
        full_y, full_z = data[f"{tag}_n{nrhs}_full_y"], data[f"{tag}_n{nrhs}_full_z"]
        y_ref, z_ref = _reference(opd, tag, x, v)
        assert sr.rel(full_y, y_ref) <= TOL[dtype] and sr.rel(full_z, z_ref) <= TOL[dtype]
        for world in worlds:
            where = f"{dtype} {mode} {tag} world {world} nrhs {nrhs}"
            layout, _ = sr.partition(opd, mode, world, owner=owners.get(world) if owners else None)
            key = lambda r, what: data[f"{tag}_w{world}_n{nrhs}_r{r}_{what}"]
            loc_y = [key(r, "loc_y") for r in range(world)]
            loc_z = [key(r, "loc_z") for r in range(world)]
            assert all(a.dtype == np_dtype for a in loc_y + loc_z), where
            if mode in ("rows", "rowblocks"):
                want_y = sr.place_segments(layout, loc_y)
                assert sr.same_bits(want_y, full_y), where + ": the shards' rows are not the one-GPU rows"      # include/bfhip.h: ROWS is bit-identical
            elif mode == "rowsum":
                want_y = sr.range_sums(layout, loc_y)
            else:
                want_y = sr.rank_order_sum(loc_y)
            want_z = sr.rank_order_sum(loc_z)
            for r in range(world):
                assert sr.same_bits(key(r, "y"), want_y), f"{where}: forward, rank {r}"
                assert sr.same_bits(key(r, "y_again"), want_y), f"{where}: forward after the adjoint, rank {r}"
                assert sr.same_bits(key(r, "z"), want_z), f"{where}: adjoint, rank {r}"
            err_y, err_z = sr.rel(want_y, y_ref), sr.rel(want_z, z_ref)
            print(f"{where}: rel-l2 forward {err_y:.2e} adjoint {err_z:.2e}")
            assert err_y <= TOL[dtype] and err_z <= TOL[dtype], where


@pytest.mark.parametrize("mode", sr.MODES)
@pytest.mark.parametrize("dtype", ["c128", "c64"])
def test_complex_sharded_steps_with_2_3_and_5_ranks(stub, tmp_path, dtype, mode):
    """Forward and adjoint step of the 1024-point operand (12 block rows of 85 / 86 rows, 144 blocks) in every sharding
    mode, worlds 2, 3 and 5, nrhs 1 and 3 (rows of 16 / 48 bytes in complex128, 8 / 24 in complex64).
    rows / rowblocks: every rank's y is the ranks' local rows at their global places AND the unsharded apply, bit for bit
    (rowblocks with 3 ranks is the interleaved [1,2,0,1,1,2,0,1,2,0,2,0]); rowsum: one-owner rows copied, a shared range
    (5 ranks share block rows 10 and 11 five ways) the list-order sum in the storage type; blocks and every adjoint: the
    rank-order sum of the full-length partials; all bit for bit, identical on every rank, and within the element type's
    tolerance of the oracle."""
    data = sr.run_child(stub, f"apply:{dtype}:{mode}", tmp_path)
    opd = sr.complex_operand()
    if mode == "rowsum":
        shared = {w: len(sr.partition(opd, mode, w)[0].segments) - 12 for w in sr.WORLDS}
        assert shared[5] == 8 and shared[2] == 0 and shared[3] == 0        # groups of 5 sources; and the sort-then-scatter branch
    _check_apply(data, "c", opd, dtype, mode, sr.WORLDS)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_real_sharded_steps_and_cov_matvec_with_2_and_3_ranks(stub, tmp_path, dtype):
    """Row ranges of the random real operands (seeds 33 and 41; 3 ranks leave the last rank ONE row: cuts [0,82,271,272]
    and [0,28,223,224]), f64 and f32, nrhs 1 and 3 (rows of 8 / 24 and 4 / 12 bytes: the 8- and 4-byte scatter kernels; a
    row range is ONE run of v, so the adjoint reads it in place and no gather kernel runs here -- see the next test):
    forward and adjoint as above, and cov_matvec with a row permutation and gamma against the oracle's own sequence,
    identical on every rank."""
    from oracle import bfref
    data = sr.run_child(stub, f"apply:{dtype}:rows", tmp_path)
    np_dtype, _ = sr.DTYPES[dtype]
    for seed in sr.REAL_SEEDS:
        opd, rng = sr.real_operand(seed)
        assert sr.partition(opd, "rows", 3)[0].rows_of[2] == 1
        _check_apply(data, f"s{seed}", opd, dtype, "rows", sr.REAL_WORLDS)
        gam, row_perm, rev, v = (a.astype(np.float64) if a.dtype == np_dtype else a for a in sr.cov_inputs(opd, rng, np_dtype))
        A = _real_reference(seed)

        def permute(a, perm):
            o = np.empty_like(a); o[perm] = a
            return o
        z_ref = permute(bfref.mat_mul_vec(A, gam * (gam * bfref.mat_rmul_vec(A, permute(v, rev)))), row_perm)
        for world in sr.REAL_WORLDS:
            got = [data[f"s{seed}_w{world}_r{r}_cov"] for r in range(world)]
            assert all(sr.same_bits(g, got[0]) for g in got), (seed, world)
            err = sr.rel(got[0], z_ref)
            print(f"{dtype} cov_matvec seed {seed} world {world}: rel-l2 {err:.2e}")
            assert got[0].dtype == np_dtype and err <= TOL[dtype], (seed, world)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_real_interleaved_block_rows_with_2_and_3_ranks(stub, tmp_path, dtype):
    """A real operand of 6 ragged block rows (85, 1, 130, 47, 99, 64) dealt [0,1,0,1,0,1] and [1,2,0,1,2,0]: every rank's rows
    are several runs of v, so the adjoint step compacts them with bfGatherSegmentsKernel on 8-byte (f64) and 4-byte (f32)
    units -- 314 rows on rank 0 of 2 is more than one workgroup -- and the forward step scatters interleaved 8- / 4-byte
    segments from slots of unequal fill.  Same assertions as the complex row-block cases."""
    data = sr.run_child(stub, f"apply:{dtype}:rowblocks", tmp_path)
    opd = sr.real_block_rows_operand()
    for world, rows in ((2, [314, 112]), (3, [194, 132, 100])):
        layout, _ = sr.partition(opd, "rowblocks", world, owner=sr.REAL_BLOCK_OWNERS[world])
        assert layout.rows_of == rows and all(len(layout.blocks_of[r]) > 1 for r in range(world))
    _check_apply(data, "b", opd, dtype, "rowblocks", sr.REAL_WORLDS, owners=sr.REAL_BLOCK_OWNERS)


def test_a_rank_without_rows_contributes_zeros(stub, tmp_path):
    """Three ranks over whole block rows with rank 2 owning none: its operator has zero rows, its slot of the gather buffer
    is padding only, and its adjoint partial is the hipMemsetAsync of bfhipShardedApplyTransposeDevice."""
    data = sr.run_child(stub, "norows", tmp_path)
    owners = {3: [0, 1] * 6}
    opd = sr.complex_operand()
    assert sr.partition(opd, "rowblocks", 3, owner=owners[3])[0].rows_of[2] == 0
    _check_apply(data, "c", opd, "c128", "rowblocks", (3,), owners=owners)


@pytest.mark.parametrize("mode", ["rows", "blocks"])
def test_gmres_over_the_sharded_matvec_with_2_and_3_ranks(stub, tmp_path, mode):
    """bfhipShardedSolveGMRESDevice on I + alpha S (N = 2048), MGS and CGS2, 1 and 2 right-hand sides: every rank returns the
    same iteration count, residual and solution bits; with row ranges these are those of the unsharded solve (the matvec is
    bit-identical); in both modes the solution is within 1e-8 of the numpy restatement of bfSolveGMRES over the oracle."""
    from oracle import bfref, linalg_ref
    data = sr.run_child(stub, f"gmres:{mode}", tmp_path)
    opd = sr.gmres_operand()
    A = bfref.from_desc(opd.desc, opd.vals, root=opd.root)
    for nrhs in (1, 2):
        b = data[f"b_n{nrhs}"]
        want, iters, _ = linalg_ref.solve_gmres(lambda X: bfref.mat_mul(A, X), b, tol=sr.GMRES_TOL, max_num_iter=sr.GMRES_MAX_ITER)
        for orth in ("mgs", "cgs2"):
            for world in (2, 3):
                key = lambda r, what: data[f"w{world}_n{nrhs}_{orth}_r{r}_{what}"]
                for r in range(world):
                    assert int(key(r, "it")) == int(key(0, "it")) and float(key(r, "res")) == float(key(0, "res")), (nrhs, orth, world, r)
                    assert sr.same_bits(key(r, "x"), key(0, "x")), (nrhs, orth, world, r)
                if mode == "rows":
                    assert int(key(0, "it")) == int(data[f"full_n{nrhs}_{orth}_it"]) and float(key(0, "res")) == float(data[f"full_n{nrhs}_{orth}_res"])
                    assert sr.same_bits(key(0, "x"), data[f"full_n{nrhs}_{orth}_x"]), (nrhs, orth, world)
                if orth == "mgs":
                    assert int(key(0, "it")) == iters, (nrhs, world)
                err = sr.rel(key(0, "x"), want)
                print(f"gmres {mode} nrhs {nrhs} {orth} world {world}: {int(key(0, 'it'))} iterations, rel-l2 {err:.2e}")
                assert err <= 1e-8, (nrhs, orth, world)


def test_a_step_that_fails_on_one_rank_aborts_every_rank(stub, tmp_path):
    """World 3, row ranges: rank 1's all-gather returns an error on the host.  All three calls return non-zero within the
    stub's deadline (rank 1 aborts its communicator, which releases the peers from the collective), every rank's next
    step is refused at once with the "communicator was aborted" error, and bfhipCommDestroy does not hand the aborted
    communicators to ncclCommDestroy."""
    data = sr.run_child(stub, "abort", tmp_path)
    f = sr.STUB_FUNCS
    assert data["good_agree"].all()
    codes, secs, msgs, calls = data["codes"], data["seconds"], data["messages"], data["calls"]
    print("return codes", codes.tolist(), "seconds", np.round(secs, 3).tolist(), "calls", calls.tolist())
    # released by the abort, not by the barrier's deadline (pinned to sr.STUB_DEADLINE_SECONDS in the child): a quarter of it is ample
    assert (codes[:, 0] != 0).all() and (secs[:, 0] < sr.STUB_DEADLINE_SECONDS / 4).all()
    assert "ncclAllGather" in str(msgs[1, 0])
    assert (codes[:, 1] == 2).all() and all("communicator was aborted" in str(m) for m in msgs[:, 1]) and (secs[:, 1] < 1.0).all()
    assert (calls[:, f["CommAbort"]] == 1).all() and (calls[:, f["CommDestroy"]] == 0).all()
    assert (calls[:, f["AllGather"]] == 2).all() and (calls[:, f["AllReduce"]] == 0).all()     # the refused step never reached a collective


def test_create_time_refusals_with_three_ranks(stub, tmp_path):
    """A rank whose operator's row count is not its segments' (INCOMPATIBLE_SHAPES) and a rank handed an owner index >= nranks
    (INVALID_ARGUMENTS) are refused in bfhipShardedCreate, on that rank only and before any collective."""
    data = sr.run_child(stub, "refuse", tmp_path)
    f = sr.STUB_FUNCS
    assert data["rows_codes"].tolist() == [0, 0, 8] and "this rank's segments hold 342" in str(data["rows_messages"][2])
    assert data["owner_codes"].tolist() == [0, 1, 0] and "bad owner" in str(data["owner_messages"][1])
    for name in ("rows", "owner"):
        calls = data[f"{name}_calls"]
        assert (calls[:, f["CommInitRank"]] == 1).all() and (calls[:, f["AllGather"]] == 0).all() and (calls[:, f["AllReduce"]] == 0).all()
