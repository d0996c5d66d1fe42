"""The device GMRES (bfhip_gmres.c around the bfGmres* kernels of bfhip_gmres.hip) on every case of tests/gmres_catalogue.py, under both
orthogonalisations and through both entries, against the long-double reference and bounds of tests/gmres_highprec.py:
finite X, the residual, forward and consistency bounds at the reported numIter, zero-residual columns returned bit for bit,
bit-identical repeats, host entry = device entry, and exact 2^k equivariance."""
import functools

import numpy as np
import pytest

import gmres_catalogue as cat
import gmres_highprec as gh

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _operator(key):
    from butterfly_amd.operator import HipOperator
    op = cat.operator(key)
    return HipOperator.from_desc(op.desc, op.vals, max_rhs=8)


@functools.lru_cache(maxsize=None)
def _precond(key, kind):
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.operator import HipOperator
    if kind == "block_jacobi":
        pre, _ = _operator(key).block_jacobi()
        return pre, pre.to_dense()
    P = cat.dense_block_inverse(key)[0]
    n, nb = P.shape[0], 16
    d = hs.Desc(dtype=0)
    pv, ch = {}, []
    for i in range(nb):
        a, b = i * n // nb, (i + 1) * n // nb
        leaf = d.add(hs.NODE_DENSE, b - a, b - a)
        pv[leaf] = np.ascontiguousarray(P[a:b, a:b])
        ch.append((leaf, a, a))
    d.root = d.add(hs.NODE_BLOCK, n, n, ch, hs.BF_TYPE_BLOCK_DIAG)
    return HipOperator.from_desc(d, pv), P


_KRYLOV = {}


def _krylov(c, P=None):
    if c.name not in _KRYLOV:
        _KRYLOV[c.name] = gh.Krylov(cat.problem(c, P), c.B, c.X0)
    return _KRYLOV[c.name]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _solve(c, orth, B=None):
    op = _operator(c.op)
    pre = _precond(c.op, c.precond)[0] if c.precond else None
    B = c.B if B is None else B
    x, it, res = op.solve_gmres_device(_dev(B), x0=None if c.X0 is None else _dev(c.X0), tol=c.tol, max_num_iter=c.m,
                                       precond=pre, orth=orth)
    return x.cpu().numpy(), it, res


@pytest.mark.parametrize("orth", cat.ORTHS)
@pytest.mark.parametrize("name", cat.names())
def test_device_gmres_within_the_long_double_bounds(name, orth, monkeypatch):
    c = cat.case(name)
    X, it, res = _solve(c, orth)
    assert np.all(np.isfinite(X)), name
    if c.iters is not None:
        assert it == c.iters, (name, it)
    assert 1 <= it <= c.m
    # a second run is bit-identical
    X2, it2, res2 = _solve(c, orth)
    assert it2 == it and res2 == res and np.array_equal(_bits(X2), _bits(X))
    # the host entry (no preconditioner argument; the environment picks the orthogonalisation) gives the same bits
    if c.precond is None:
        monkeypatch.setenv("BFHIP_GMRES_MGS", "1" if orth == "mgs" else "0")
        Xh, ith, resh = _operator(c.op).solve_gmres(c.B, x0=c.X0, tol=c.tol, max_num_iter=c.m)
        assert ith == it and resh == res and np.array_equal(_bits(Xh), _bits(X))
    # a zero-residual column is x0 (zeros without one), bit for bit
    for p in c.zero_cols:
        want = np.zeros(c.n, dtype=np.complex128) if c.X0 is None else c.X0[:, p]
        assert np.array_equal(_bits(X[:, p]), _bits(want)), (name, p)
    P = _precond(c.op, c.precond)[1] if c.precond == "block_jacobi" else None
    fails = gh.check(_krylov(c, P), X, it, res)
    assert not fails, (name, orth, it, res, fails)


@pytest.mark.parametrize("orth", cat.ORTHS)
@pytest.mark.parametrize("name", cat.SCALE_BASES)
def test_scaling_b_by_a_power_of_two_scales_x_exactly(name, orth):
    c = cat.case(name)
    if c.X0 is not None:                         # x0 is not scaled with b: start from zero
        c = cat.Case(c.name + "_nox0", c.op, c.B, None, c.m, c.tol)
    X, it, res = _solve(c, orth)
    for k in (-600, -300, 300, 600):
        Bk = np.ldexp(c.B.real, k) + 1j * np.ldexp(c.B.imag, k)
        Xk, itk, resk = _solve(c, orth, Bk)
        assert itk == it and resk == res, (k, it, itk, res, resk)
        want = np.ldexp(X.real, k) + 1j * np.ldexp(X.imag, k)
        assert np.array_equal(_bits(Xk), _bits(want)), k
