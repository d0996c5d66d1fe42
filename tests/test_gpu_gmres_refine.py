"""Mixed-precision GMRES refinement on the GPU (bfhipSolveGMRESRefine[Device]): the second-kind system of
tests/bie.py compiled twice, complex128 (true residuals) and demote_to_f32 (the inner operator)."""
import numpy as np
import pytest

from oracle import bfref
import bie
import refine_ref

pytestmark = pytest.mark.gpu
N = 2048


def rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


@pytest.fixture(scope="module")
def system():
    from butterfly_amd.operator import HipOperator
    desc, root, vals, dense = bie.second_kind_case(N, 128)
    A = bfref.from_desc(desc, vals, root=root)
    op = HipOperator.from_desc(desc, vals, root=root, max_rhs=3)
    low = HipOperator.from_desc(desc, vals, root=root, max_rhs=3, demote_to_f32=True)
    rng = np.random.default_rng(7)
    b = rng.standard_normal((N, 3)) + 1j * rng.standard_normal((N, 3))
    yield desc, root, vals, dense, A, op, low, b
    op.close()
    low.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("nrhs", [1, 3])
def test_refinement_reaches_complex128_accuracy(system, nrhs):
    desc, root, vals, dense, A, op, low, b = system
    bb = b[:, 0] if nrhs == 1 else b
    x, k, inner, res, hist = op.solve_gmres_refine_device(_dev(bb), low, tol=1e-12)
    x = x.cpu().numpy()
    true = refine_ref.true_residual(lambda v: bfref.mat_mul(A, v), bb, x)
    print(f"nrhs={nrhs} outer={k} inner={inner} res={res:.3e} host={true:.3e} hist={hist}")
    assert res <= 1e-12
    assert abs(res - true) <= 1e-3 * true + 1e-15          # (+ the floor of a complex128 residual evaluation)
    assert rel(x, np.linalg.solve(dense, bb)) <= 1e-10
    assert 1 <= k <= refine_ref.OUTER_STEPS_2048 + 1 and len(hist) == k + 1 and inner > 0
    assert hist[0] == 1.0 and hist[-1] == res


def test_the_outer_loop_does_the_work(system):
    desc, root, vals, dense, A, op, low, b = system
    _, k1, _, res1, hist1 = op.solve_gmres_refine_device(_dev(b), low, tol=1e-12, max_outer=1)
    assert k1 == 1 and res1 >= 1e-9 and hist1[1] == res1            # one step stops at the complex64 operator's accuracy
    _, k, _, res, hist = op.solve_gmres_refine_device(_dev(b), low, tol=1e-12)
    assert hist[0] == 1.0 and all(hist[i + 1] < 0.5 * hist[i] for i in range(k))


def test_zero_column_and_x0(system):
    desc, root, vals, dense, A, op, low, b = system
    mv = lambda v: bfref.mat_mul(A, v)
    bz = b.copy()
    bz[:, 1] = 0
    x, k, _, res, hist = op.solve_gmres_refine_device(_dev(bz), low, tol=1e-12)
    x = x.cpu().numpy()
    assert np.all(np.isfinite(x)) and np.all(x[:, 1] == 0) and not np.any(np.signbit(x[:, 1].real))
    assert res <= 1e-12 and np.all(np.isfinite(hist))
    x0 = 0.5 * np.linalg.solve(dense, b)
    x, k, _, res, hist = op.solve_gmres_refine_device(_dev(b), low, x0=_dev(x0), tol=1e-12)
    r0 = refine_ref.true_residual(mv, b, x0)
    assert abs(hist[0] - r0) <= 1e-6 * r0 and res <= 1e-12
    assert rel(x.cpu().numpy(), np.linalg.solve(dense, b)) <= 1e-10


def test_stagnation_returns_the_best_iterate(system, helm2_cases):
    """The inner operator is the complex64 compile of a different system (I - 30 alpha S): a step makes things worse."""
    from butterfly_amd.operator import HipOperator
    desc, root, vals, dense, A, op, low, b = system
    d2, tp, v2 = helm2_cases(N, 128)
    v2 = {nd: v.copy() for nd, v in v2.items()}
    root2 = bie.identity_plus(d2, v2, -30 * 2 * (2 * np.pi / N))
    wrong = HipOperator.from_desc(d2, v2, root=root2, max_rhs=3, demote_to_f32=True)
    x, k, inner, res, hist = op.solve_gmres_refine_device(_dev(b), wrong, tol=1e-12, max_outer=10)
    x = x.cpu().numpy()
    print(f"stagnation: outer={k} inner={inner} res={res:.3e} hist={hist}")
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(hist))
    assert 1 <= k < 10 and res > 1e-12
    assert res == min(hist) and not hist[-1] < 0.5 * hist[-2]
    true = refine_ref.true_residual(lambda v: bfref.mat_mul(A, v), b, x)
    assert abs(res - true) <= 1e-6 * true
    wrong.close()


def test_preconditioners_complex128_and_complex64(system):
    """The block-Jacobi inverse of test_gmres.py::test_left_preconditioned_gmres_follows_the_corrected_restatement as the
    inner solveM, compiled as complex128 and as complex64.  At inner_tol = 1e-10 (the default 1e-6 takes three iterations per correction with or without it)."""
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.operator import HipOperator
    desc, root, vals, dense, A, op, low, b = system
    nb = 16
    d = hs.Desc(dtype=0)
    pv, ch = {}, []
    for i in range(nb):
        sl = slice(i * N // nb, (i + 1) * N // nb)
        leaf = d.add(hs.NODE_DENSE, sl.stop - sl.start, sl.stop - sl.start)
        pv[leaf] = np.linalg.inv(dense[sl, sl])
        ch.append((leaf, sl.start, sl.start))
    d.root = d.add(hs.NODE_BLOCK, N, N, ch, hs.BF_TYPE_BLOCK_DIAG)
    pre128 = HipOperator.from_desc(d, pv, max_rhs=3)
    pre64 = HipOperator.from_desc(d, pv, max_rhs=3, demote_to_f32=True)
    _, _, inner_plain, res, _ = op.solve_gmres_refine_device(_dev(b), low, tol=1e-12, inner_tol=1e-10)
    assert res <= 1e-12
    for pre in (pre128, pre64):
        x, k, inner, res, hist = op.solve_gmres_refine_device(_dev(b), low, tol=1e-12, inner_tol=1e-10, precond=pre)
        print(f"precond dtype={pre.dtype}: outer={k} inner={inner} (plain {inner_plain}) res={res:.3e}")
        assert res <= 1e-12 and inner < inner_plain
        assert rel(x.cpu().numpy(), np.linalg.solve(dense, b)) <= 1e-10
    pre128.close()
    pre64.close()


def test_deterministic_and_host_entry_equals_device_entry(system):
    import torch
    desc, root, vals, dense, A, op, low, b = system
    r1 = op.solve_gmres_refine_device(_dev(b), low, tol=1e-12)
    r2 = op.solve_gmres_refine_device(_dev(b), low, tol=1e-12)
    assert torch.equal(r1[0], r2[0]) and r1[1:4] == r2[1:4] and np.array_equal(r1[4], r2[4])
    xh, kh, ih, resh, histh = op.solve_gmres_refine(b, low, tol=1e-12)
    assert np.array_equal(xh, r1[0].cpu().numpy()) and (kh, ih, resh) == r1[1:4] and np.array_equal(histh, r1[4])
    for orth in ("cgs2", "mgs"):
        x, k, _, res, _ = op.solve_gmres_refine_device(_dev(b), low, tol=1e-12, orth=orth)
        assert res <= 1e-12
    with pytest.raises(ValueError, match="complex128"):
        op.solve_gmres_refine_device(_dev(b).to(torch.complex64), low)


def test_plain_gmres_still_refuses_complex64(system):
    import torch
    from butterfly_amd import _capi
    desc, root, vals, dense, A, op, low, b = system
    with pytest.raises(_capi.BfhipError) as e:
        low.solve_gmres(b[:, 0])
    assert e.value.code == 3 and "complex64" in str(e.value)
    with pytest.raises(_capi.BfhipError) as e:
        op.solve_gmres_device(torch.ones(N, dtype=torch.complex128, device="cuda:0"), precond=low)
    assert e.value.code == 3 and "complex64" in str(e.value)
    # and plain complex128 GMRES is unchanged by the shared workspace: it still solves the system
    x, it, res = op.solve_gmres_device(_dev(b), tol=1e-12, max_num_iter=80)
    assert res < 1e-12 and rel(x.cpu().numpy(), np.linalg.solve(dense, b)) <= 1e-10
