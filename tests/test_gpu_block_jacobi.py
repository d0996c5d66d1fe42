"""Block-Jacobi preconditioner on the device (bfhipBlockJacobi): gathered blocks, inverses, the preconditioned solvers,
determinism, refusals and memory."""
import copy

import numpy as np
import pytest

from butterfly_amd import _capi, helm2_structure as hs
from butterfly_amd.operator import HipOperator
from oracle import bfref, helm2_build as hb, linalg_ref
import bie

pytestmark = pytest.mark.gpu
N, K = 2048, 128


def rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def blockdiag_of(dense, cuts):
    out = np.zeros_like(dense)
    for a, b in zip(cuts[:-1], cuts[1:]):
        out[a:b, a:b] = dense[a:b, a:b]
    return out


@pytest.fixture(scope="module")
def first_kind():
    from conftest import helm2_case
    desc, tp, vals = helm2_case(N, K)
    return desc, vals


@pytest.fixture(scope="module")
def second_kind():
    desc, root, vals, dense = bie.second_kind_case(N, K)
    return desc, root, vals, dense


def real_square_operand():
    """The helm2 2048 structure as an f64 operand: random real leaf values, the identity blocks of tests/bie.py."""
    from conftest import helm2_case
    desc, _, _ = helm2_case(N, K, recipes=False)
    d = copy.deepcopy(desc)
    d.dtype = 1
    rng = np.random.default_rng(11)
    vals = {i: rng.standard_normal((d.rows[i], d.cols[i])) / np.sqrt(d.cols[i]) for i in range(d.num_nodes) if d.kind[i] == hs.NODE_DENSE}
    root = bie.identity_plus(d, vals, 0.5)
    return d, root, vals


@pytest.mark.parametrize("which", ["c128", "c64", "f64"])
def test_gathered_blocks_equal_the_diagonal_blocks(first_kind, which):
    desc, vals = first_kind
    if which == "f64":
        d, root, rv = real_square_operand()
        op = HipOperator.from_desc(d, rv, root=root)
    else:
        op = HipOperator.from_desc(desc, vals, demote_to_f32=(which == "c64"))
    cuts = op.block_jacobi_partition()
    dense = op.to_dense()
    pre, info = op.block_jacobi(invert=False)
    assert pre.dtype == op.dtype and pre.shape == op.shape
    assert info["numBlocks"] == len(cuts) - 1 and info["uncoveredRows"] == 0 and info["maxBlockRows"] == np.diff(cuts).max()
    got = pre.to_dense()
    ref = blockdiag_of(dense, cuts)
    assert rel(got, ref) <= 1e-15
    assert not np.any(got[ref == 0])                      # nothing outside the blocks
    pre.close(); op.close()


@pytest.mark.parametrize("case", ["first", "second"])
def test_inverses(first_kind, second_kind, case):
    if case == "first":
        desc, vals = first_kind
        op = HipOperator.from_desc(desc, vals)
    else:
        desc, root, vals, _ = second_kind
        op = HipOperator.from_desc(desc, vals, root=root)
    dense = op.to_dense()
    cuts = op.block_jacobi_partition()
    pre, info = op.block_jacobi()
    assert info["firstSingularBlock"] == -1 and 0 < info["minPivotRel"] <= 1
    m = pre.to_dense()
    for a, b in zip(cuts[:-1], cuts[1:]):
        blk, mb = dense[a:b, a:b], m[a:b, a:b]
        assert np.linalg.norm(blk @ mb - np.eye(b - a)) <= 1e-10
        inv = np.linalg.inv(blk)
        assert rel(mb, inv) <= 1e-10
    assert not np.any(m[blockdiag_of(np.ones_like(m), cuts) == 0])
    pre.close(); op.close()


def test_preconditioned_gmres_follows_the_corrected_restatement(second_kind):
    import torch
    desc, root, vals, dense = second_kind
    A = bfref.from_desc(desc, vals, root=root)
    op = HipOperator.from_desc(desc, vals, root=root)
    cuts = op.block_jacobi_partition()
    pre, _ = op.block_jacobi()
    minv = np.zeros_like(dense)
    for a, b in zip(cuts[:-1], cuts[1:]):
        minv[a:b, a:b] = np.linalg.inv(dense[a:b, a:b])
    rng = np.random.default_rng(12)
    bb = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    x_ref, it_ref, hist = linalg_ref.solve_gmres(lambda v: bfref.mat_mul(A, v), bb, tol=1e-10, max_num_iter=80, msolve=lambda v: minv @ v)
    _, it_plain, _ = linalg_ref.solve_gmres(lambda v: bfref.mat_mul(A, v), bb, tol=1e-10, max_num_iter=80)
    assert it_ref <= it_plain
    x, it, res = op.solve_gmres_device(torch.from_numpy(bb).cuda(), tol=1e-10, max_num_iter=80, precond=pre, orth="mgs")
    assert it == it_ref and abs(res - hist[-1]) <= 1e-6 * hist[-1] + 1e-16
    assert rel(x.cpu().numpy(), x_ref) < 1e-9
    pre.close(); op.close()


def test_device_built_first_kind_system_needs_fewer_iterations():
    import torch
    n = 16384
    k = n / 16
    op, perm, _ = HipOperator.fac_helm2_make_multilevel(hs.circle_points(n), k, device=0)
    pre, info = op.block_jacobi()
    assert info["numBlocks"] > n // 128 and info["maxBlockRows"] < 128 and info["uncoveredRows"] == 0
    rng = np.random.default_rng(7)
    b = torch.from_numpy(rng.standard_normal(n) + 1j * rng.standard_normal(n)).cuda()
    x0, it0, r0 = op.solve_gmres_device(b, tol=1e-8, max_num_iter=4000)
    x1, it1, r1 = op.solve_gmres_device(b, tol=1e-8, max_num_iter=4000, precond=pre)
    assert r1 <= 1e-8 and it1 < it0, (it0, it1, r0, r1)
    # the solution solves the unpreconditioned system too
    ax = op.apply_device(x1)
    assert float(torch.linalg.norm(ax - b) / torch.linalg.norm(b)) <= 1e-6
    pre.close(); op.close()


def test_complex64_preconditioner_drives_the_refinement(second_kind):
    import torch
    desc, root, vals, dense = second_kind
    op = HipOperator.from_desc(desc, vals, root=root)
    low = HipOperator.from_desc(desc, vals, root=root, demote_to_f32=True)
    pre64, info = op.block_jacobi(dtype=_capi.BFHIP_C64)
    assert pre64.dtype == _capi.BFHIP_C64
    pre128, _ = op.block_jacobi()
    assert rel(pre64.to_dense(), pre128.to_dense()) < 1e-6
    rng = np.random.default_rng(4)
    b = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    x, outer, inner, res, hist = op.solve_gmres_refine_device(torch.from_numpy(b).cuda(), low, tol=1e-11, inner_tol=1e-5, max_outer=10,
                                                              max_inner=80, precond=pre64)
    assert res <= 1e-11
    assert rel(x.cpu().numpy(), np.linalg.solve(dense, b)) < 1e-8
    pre64.close(); pre128.close(); low.close(); op.close()


def test_builds_are_bit_identical_and_survive_save_load(second_kind, tmp_path):
    import torch
    desc, root, vals, _ = second_kind
    op = HipOperator.from_desc(desc, vals, root=root)
    p1, _ = op.block_jacobi()
    p2, _ = op.block_jacobi()
    p3, _ = op.block_jacobi(cuts=op.block_jacobi_partition())
    d1 = p1.to_dense(device=True)
    assert torch.equal(d1, p2.to_dense(device=True)) and torch.equal(d1, p3.to_dense(device=True))
    # the preconditioner saved and loaded, and a preconditioner of the operator saved and loaded
    p1.save(tmp_path / "pre.bfhip")
    p4 = HipOperator.load(tmp_path / "pre.bfhip")
    op.save(tmp_path / "op.bfhip")
    op2 = HipOperator.load(tmp_path / "op.bfhip")
    p5, _ = op2.block_jacobi()
    assert torch.equal(d1, p4.to_dense(device=True)) and torch.equal(d1, p5.to_dense(device=True))
    for p in (p1, p2, p3, p4, p5, op2, op):
        p.close()


def test_singular_block_is_refused():
    d = hs.Desc(dtype=0)
    rng = np.random.default_rng(2)
    leaves = [d.add(hs.NODE_DENSE, 8, 8) for _ in range(3)]
    vals = {c: rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8)) for c in leaves}
    vals[leaves[1]] = np.ones((8, 8), dtype=np.complex128)             # rank one
    d.root = d.add(hs.NODE_BLOCK, 24, 24, [(c, 8 * i, 8 * i) for i, c in enumerate(leaves)], hs.BF_TYPE_BLOCK_DIAG)
    op = HipOperator.from_desc(d, vals)
    with pytest.raises(_capi.BfhipError) as e:
        op.block_jacobi()
    assert e.value.code == 2 and e.value.info["firstSingularBlock"] == 1
    pre, info = op.block_jacobi(invert=False)       # the blocks themselves are fine
    assert info["firstSingularBlock"] == -1
    pre.close()
    vals[leaves[1]] = rng.standard_normal((8, 8)) + 0j
    vals[leaves[2]] = vals[leaves[1]].copy()
    vals[leaves[2]][3, 3] = np.nan
    op2 = HipOperator.from_desc(d, vals)
    with pytest.raises(_capi.BfhipError) as e:
        op2.block_jacobi()
    assert e.value.code == 2 and e.value.info["firstSingularBlock"] == 2
    op.close(); op2.close()


def test_no_device_memory_is_leaked(second_kind):
    import torch
    desc, root, vals, _ = second_kind
    op = HipOperator.from_desc(desc, vals, root=root)
    pre, _ = op.block_jacobi()          # warm-up: the runtime's own first-use allocations
    pre.close()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    pre, _ = op.block_jacobi()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    st = pre.stats()
    own = pre.num_bytes() + st["tempElems"] * 16 + st["metaBytes"] + 4096
    assert free0 - free1 <= own + (4 << 20), (free0 - free1, own)
    pre.close()
    with pytest.raises(_capi.BfhipError):
        op.block_jacobi(cuts=[0, 5, 3, N])
    for _ in range(3):
        p, _ = op.block_jacobi()
        p.close()
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info()
    assert abs(free2 - free0) <= (4 << 20), (free0, free2)
    op.close()
