"""Conditioning the Chebyshev route on observations, without a GPU: the exports and prototypes, every
refusal of bfhipChebCovCondCreate that needs the arguments alone (a BfhipChebCov lives on a device, so the refusals that read it
-- an index >= n, no coefficients -- are in tests/test_gpu_cheb_condition.py), and what tests/chebcond_cases.py claims of its
cases on the long-double reference alone."""
import ctypes as C

import numpy as np
import pytest

import chebcond_cases as cq
from butterfly_amd import _capi

INVALID = 1


@pytest.fixture(scope="module")
def mats():
    return cq.matrices()


def test_the_new_symbols_are_exported():
    import butterfly_amd
    from butterfly_amd.operator import ChebCovCondition, CovCondition
    lib = _capi.load()
    fn = lib.bfhipChebCovCondCreate
    assert fn.restype is C.c_int and len(fn.argtypes) == 6 and fn.argtypes[2] is C.c_size_t
    assert callable(butterfly_amd.ChebCovariance.condition)
    assert issubclass(ChebCovCondition, CovCondition) and butterfly_amd.ChebCovCondition is ChebCovCondition
    for name in ("sample_block", "mean", "draw", "moments", "log_likelihood", "variance", "info", "close"):
        assert getattr(ChebCovCondition, name) is getattr(CovCondition, name), name     # a thin subclass: the entries are shared


def test_argument_refusals_read_nothing_through_the_object():
    """0x1000 stands for "not NULL": no pointer below is dereferenced, the stand-in BfhipChebCov least of all.  The order is
    bfhipCovCondCreate's: NULLs, numObs, a repeated index, noiseVar.  *out is NULL after every refusal."""
    lib = _capi.load()
    create, msg = lib.bfhipChebCovCondCreate, lib.bfhipLastErrorMessage
    p = C.c_void_p(0x1000)
    obs = np.array([3, 7, 11], dtype=np.uint64)

    def refused(cheb, o, k, noise, want, has_out=True):
        out = C.c_void_p(0x1234)
        rc = create(cheb, o, k, noise, C.byref(out) if has_out else None, None)
        assert rc == INVALID and want in msg(), (rc, msg())
        assert not has_out or not out.value

    refused(None, obs.ctypes.data, 3, None, b"NULL")
    refused(p, None, 3, None, b"NULL")
    refused(p, obs.ctypes.data, 3, None, b"NULL", has_out=False)
    refused(p, obs.ctypes.data, 0, None, b"numObs")
    refused(p, obs.ctypes.data, 2049, None, b"numObs")
    refused(None, obs.ctypes.data, 0, None, b"NULL")                          # a NULL wins over a bad numObs
    rep = np.array([3, 7, 3, 10 ** 12], dtype=np.uint64)                      # repeated, and far outside any mesh: the repetition is found first
    refused(p, rep.ctypes.data, 4, None, b"repeated")
    for bad in (-1e-300, np.nan, np.inf, -np.inf):
        noise = np.array([0.0, bad, 1.0])
        refused(p, obs.ctypes.data, 3, noise.ctypes.data, b"noiseVar[1]")
    bad_both = np.array([np.nan, 1.0, 1.0, 1.0])
    refused(p, rep.ctypes.data, 4, bad_both.ctypes.data, b"repeated")         # the repetition wins over the noise


def test_entries_refuse_a_null_object():
    lib = _capi.load()
    p = C.c_void_p(0x1000)
    assert lib.bfhipCovCondSampleBlockDevice(None, p, p, None, 1, p, None, None) == INVALID
    assert lib.bfhipCovCondMeanDevice(None, p, p, None, None) == INVALID
    assert lib.bfhipCovCondDrawDevice(None, p, 1, 2, 0, 1, p, None) == INVALID
    assert lib.bfhipCovCondMomentsDevice(None, p, 1, 2, 0, 1, 1, p, p, None) == INVALID
    assert lib.bfhipCovCondLogLikelihoodDevice(None, p, p, None, p, None, None) == INVALID
    q = np.array([1], dtype=np.uint64)
    assert lib.bfhipCovCondVarianceDevice(None, q.ctypes.data, 1, p, p, None) == INVALID
    info = _capi.BfhipCovCondInfo()
    info.structSize = C.sizeof(info)
    assert lib.bfhipCovCondGetInfo(None, C.byref(info)) == INVALID
    lib.bfhipCovCondFree(None)
    h = C.c_void_p()
    lib.bfhipCovCondFree(C.byref(h))


def test_the_case_shapes_are_the_ones_the_kernels_branch_on(mats):
    m = mats["mesh4099"]
    assert m.n == 4099 and cq.num_chunks(m.n) == 5 and m.n - 4 * cq.CHUNK == 3          # the last chunk: the three ears
    assert cq.num_chunks(mats["mesh63"].n) == 1 and mats["n1"].n == 1
    assert cq.cases_of("n1") == [(1, o) for o in cq.ORDERS]
    for k in (33, 130):
        obs = m.observed(k)
        assert len(set(obs.tolist())) == k and set(cq.EARS) <= set(obs.tolist())
        q = m.queries(obs)
        assert len(q) == 70 == len(set(q.tolist())) and len(set(q.tolist()) & set(obs.tolist())) == 8
    assert set(m.observed(33).tolist()) <= set(m.observed(130).tolist())
    assert (130 + 63) // 64 == 3 and 130 > 64 and 130 > 2 * 32                            # panels 64 + 64 + 2; Gram tiles and Cholesky blocks
    assert cq.QS[-1] == 70 and cq.MAXQ - 64 == 6                                          # passes 64 + 6


@pytest.mark.parametrize("k,order", [(33, 1), (33, 2), (33, 64), (130, 1), (130, 2), (130, 64)])
def test_every_chunk_of_n_moves_alpha(mats, k, order):
    """On the reference alone: leaving any one of the five chunks out of G, or out of X^T W, moves alpha by at least 1e3
    tolerances in every column -- a kernel that drops or misplaces a chunk, the three-row one included, cannot pass."""
    case = mats["mesh4099"].case(k, order)
    sens = cq.every_chunk_matters(case)
    need = 1e3 * cq.TOL
    print(f"mesh4099 k={k} order={order}: cond(G + D) = {case.kappa:.2f}; alpha moves by at least "
          + ", ".join(f"{what}[{c}] {v:.2e}" for (c, what), v in sens.items()) + f" (needed {need:.0e})")
    assert len(sens) == 10
    assert min(sens.values()) >= need
    assert case.kappa <= case.kappa_bound
    lo, hi = case.noise.min() * k / float(np.trace(case.G)), case.noise.max() * k / float(np.trace(case.G))
    assert 0.5 * cq.RHO <= lo and hi <= 1.5 * cq.RHO


def test_the_float64_sequence_is_within_the_floor_of_its_reference(mats):
    """The yardstick itself, on the small mesh: the float64 sequence's errors are finite, and the bound a device result is held
    to is never below fwd_bound(n, k, cond)."""
    case = mats["mesh63"].case(33, 64)
    ref, f64 = case.results()
    for name in ("alpha", "Z", "mean", "value", "grad_noise", "prior", "post"):
        e = cq.rel_errs(name, f64[name], ref[name])
        assert np.isfinite(e).all() and e.max() < 1e-10, (name, e.max())
        assert (case.allowed(name) >= case.bound).all()
    # posterior variance at the observed queries is below the noise there (and positive); elsewhere it is below the prior
    post, prior = ref["post"].astype(np.float64), ref["prior"].astype(np.float64)
    assert (post[:8] > 0).all() and (post[:8] <= case.noise[:8]).all() and (post <= prior).all()
