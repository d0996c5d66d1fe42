"""The device refinement (bfhip_refine.c around bfRefineDemote/Promote/Scale/UpdateKernel of bfhip_gmres.hip) on every case of
tests/refine_catalogue.py, under both orthogonalisations and through both entries, against the long-double checks of
tests/refine_highprec.py: finite results, reported residuals consistent with the long-double ones at every iterate, the best
iterate returned, the stop rule, zero-residual columns bit for bit, bit-identical repeats, host entry = device entry (also with
padded leading dimensions), exact 2^k equivariance, and a NaN in b.

The device returns the best iterate only: X_j comes from a run with max_outer = j, whose history must be a prefix of the full
one bit for bit.  `blockdiag262145_k1_inv` runs under one orthogonalisation and without those re-runs."""
import ctypes as C
import functools

import numpy as np
import pytest

import gmres_catalogue as cat
import refine_catalogue as rcat
import refine_highprec as rh

pytestmark = pytest.mark.gpu
SENTINEL = -7.25 + 3.5j


@functools.lru_cache(maxsize=None)
def _system(key):
    from butterfly_amd.operator import HipOperator
    op = cat.operator(key)
    return HipOperator.from_desc(op.desc, op.vals, max_rhs=8)


@functools.lru_cache(maxsize=None)
def _inner(key):
    from butterfly_amd.operator import HipOperator
    op = cat.operator(key)
    return HipOperator.from_desc(op.desc, op.vals, max_rhs=8, demote_to_f32=True)


@functools.lru_cache(maxsize=None)
def _precond(key, kind):
    from butterfly_amd.operator import HipOperator
    d, pv, _ = rcat.precond_desc(key, kind)
    return HipOperator.from_desc(d, pv, max_rhs=8, demote_to_f32=(kind == "c64"))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _kw(c, orth, max_outer=None):
    return dict(tol=c.tol, inner_tol=c.inner_tol, max_outer=max_outer or c.max_outer, max_inner=c.max_inner,
                precond=_precond(c.op, c.precond) if c.precond else None, orth=orth)


def _solve(c, orth, B=None, max_outer=None):
    B = c.B if B is None else B
    x, k, inner, res, hist = _system(c.op).solve_gmres_refine_device(_dev(B), _inner(c.low_key), x0=None if c.X0 is None else _dev(c.X0),
                                                                    **_kw(c, orth, max_outer))
    return x.cpu().numpy(), k, inner, res, hist


def _same(a, b):
    return (np.array_equal(_bits(a[0]), _bits(b[0])) and a[1:3] == b[1:3] and _bits(a[3]) == _bits(b[3])
            and np.array_equal(_bits(a[4]), _bits(b[4])))


def _host_padded(c, orth):
    """bfhipSolveGMRESRefine with ldb = nrhs + 3, ldx = nrhs + 2, ldx0 = nrhs + 1 and the padding filled with a sentinel."""
    from butterfly_amd import _capi
    n, nrhs = c.B.shape
    pad = lambda A, extra: np.concatenate([A, np.full((n, extra), SENTINEL)], axis=1).copy()
    Bp, Xp = pad(c.B, 3), np.full((n, nrhs + 2), SENTINEL)
    X0p = None if c.X0 is None else pad(c.X0, 1)
    op = _system(c.op)
    kw = _kw(c, orth)
    o = op._refine_options(kw["tol"], kw["inner_tol"], kw["max_outer"], kw["max_inner"], kw["precond"], orth)
    no, ni, res = C.c_size_t(0), C.c_size_t(0), C.c_double(0)
    hist = np.full(c.max_outer + 1, np.nan)
    rc = _capi.load().bfhipSolveGMRESRefine(op.handle, _inner(c.low_key).handle, C.byref(o), Bp.ctypes.data, nrhs + 3, nrhs,
                                            None if X0p is None else X0p.ctypes.data, nrhs + 1, C.byref(no), C.byref(ni), C.byref(res),
                                            hist.ctypes.data_as(C.POINTER(C.c_double)), Xp.ctypes.data, nrhs + 2)
    assert rc == 0
    assert np.array_equal(_bits(Xp[:, nrhs:]), _bits(np.full((n, 2), SENTINEL))), "the padding of X was written"
    assert np.array_equal(_bits(Bp[:, nrhs:]), _bits(np.full((n, 3), SENTINEL)))
    return Xp[:, :nrhs], int(no.value), int(ni.value), float(res.value), hist[:int(no.value) + 1].copy()


def _params():
    return [(n, o) for n in rcat.names() for o in (("cgs2",) if rcat.case(n).slow else rcat.ORTHS)]


@pytest.mark.parametrize("name,orth", _params())
def test_device_refinement_meets_the_long_double_checks(name, orth):
    c = rcat.case(name)
    full = _solve(c, orth)
    X, k, inner, res, hist = full
    # a second run is bit-identical: X, counts, residual and history
    assert _same(_solve(c, orth), full), name
    # X_j from a run of j steps; its history is a prefix of the full one
    iterates = None
    if not c.slow:
        iterates = []
        for j in range(1, k):
            Xj, kj, _, resj, histj = _solve(c, orth, max_outer=j)
            assert kj == j and np.array_equal(_bits(histj), _bits(hist[:j + 1])), (name, j, histj, hist)
            iterates.append(Xj if resj == histj[-1] else None)
        if k:
            iterates.append(X if res == hist[-1] else None)
    # the host entry gives the same bits, with tight and with padded leading dimensions
    host = _system(c.op).solve_gmres_refine(c.B, _inner(c.low_key), x0=c.X0, **_kw(c, orth))
    assert _same(host, full), name
    assert _same(_host_padded(c, orth), full), name
    fails = rh.check(rcat.problem(c), c.B, c.X0, full, c.tol, c.max_outer, iterates=iterates, xstar=rcat.solution(name),
                     zero_cols=c.zero_cols, converges=c.converges)
    ko, ki = rcat.RESTATED.get(name, (None, None))
    print(f"{name} {orth}: outer={k} inner={inner} (restatement: outer={ko} inner={ki}) residual={res:.3e} history={list(hist)}")
    assert not fails, (name, orth, k, inner, res, list(hist), fails)
    if name in rcat.HISTORY1:                    # X_1 is worse than x0 and not returned: history[1] against the restatement's
        assert k == 1 and abs(hist[1] - rcat.HISTORY1[name]) <= rcat.history1_tolerance(c), (name, hist[1])
    if c.converges:                              # the device may take one outer step more than the restatement
        assert res <= c.tol and (ko is None or k <= ko + 1), (name, k, ko, res)


@pytest.mark.parametrize("orth", rcat.ORTHS)
@pytest.mark.parametrize("name", rcat.SCALE_BASES)
def test_scaling_b_by_a_power_of_two_scales_x_exactly(name, orth):
    """R / ||R|| and the inner solve see identical bits, and every other operation is scaled by an exact power of two."""
    c = rcat.case(name)
    base = _solve(c, orth)
    assert base[1] >= 1
    for k in rcat.SCALE_EXPONENTS:
        got = _solve(c, orth, rcat.ldexp(c.B, k))
        want = (rcat.ldexp(base[0], k),) + base[1:]
        assert _same(got, want), (name, k, base[1:], got[1:])
    if name == "dense257_k2":               # 2^-600 next to 2^+600: each column has its own exponent
        m = rcat.case("dense257_mixed_2^-600_2^600")
        got = _solve(m, orth)
        want = (np.stack([rcat.ldexp(base[0][:, 0], -600), rcat.ldexp(base[0][:, 1], 600)], axis=1),) + base[1:]
        assert _same(got, want), (base[1:], got[1:])


@pytest.mark.parametrize("orth", rcat.ORTHS)
def test_a_nan_in_b_makes_the_residual_nan_and_the_call_return(orth):
    c = rcat.case("dense257_k3")
    B = c.B.copy()
    B[100, 1] = complex(np.nan, 0.0)
    X, k, inner, res, hist = _solve(c, orth, B)             # rc 0: a non-zero rc raises
    assert np.isnan(res) and k == 0 and inner == 0 and len(hist) == 1 and np.isnan(hist[0])
    assert not X.any()                                      # no step was taken: x0 = zeros comes back
    Xh, kh, _, resh, _ = _system(c.op).solve_gmres_refine(B, _inner(c.low_key), **_kw(c, orth))
    assert np.isnan(resh) and kh == 0 and not Xh.any()
