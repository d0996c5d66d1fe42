"""Batched covariance sampling, the part that needs no GPU: the exported symbols, the host twin of
the device normals (bfhipNormalValue = bfhip_normal_value of include/bfhip_synth.h) against an independent numpy
restatement, its first four moments, and the argument checks of the six entries, which all come before the device is
touched (a BFHIP_FLAG_PLAN_ONLY operator reaches every one of them and is refused only afterwards)."""
import ctypes as C

import numpy as np
import pytest

import randgraph
from butterfly_amd import _capi
from butterfly_amd.operator import HipOperator

INVALID, RUNTIME, TYPE = 1, 2, 7
ULP_BOUND = 8          # libm and numpy log / cos each stay within a few ulp (measured maximum here: 2)


def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def normal_restated(seed, idx):
    """include/bfhip_synth.h's formula in numpy: uint64 arithmetic wraps as in C."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed = np.uint64(seed)
    c = np.uint64(0x9e3779b97f4a7c15) * (idx + np.uint64(1))
    z1 = mix64((seed ^ np.uint64(0xd1b54a32d192ed03)) + c)
    z2 = mix64((seed ^ np.uint64(0x8cb92ba72f3d8dd7)) + c)
    u1 = ((z1 >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (z2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def host_normals(seed, idx):
    lib = _capi.load()
    return np.array([lib.bfhipNormalValue(int(seed), int(i)) for i in idx])


def test_the_new_symbols_are_exported():
    lib = _capi.load()
    for name in ("bfhipCovSampleBlockDevice", "bfhipCovMatvecBlockDevice", "bfhipNormalValue", "bfhipFillNormalDevice",
                 "bfhipCovDrawDevice", "bfhipCovMomentsDevice"):
        assert hasattr(lib, name), name
    for name in ("cov_sample_block_device", "cov_matvec_block_device", "cov_draw_device", "cov_moments_device", "fill_normal"):
        assert callable(getattr(HipOperator, name)), name


def test_host_normals_match_an_independent_restatement():
    worst = 0.0
    seen = []
    with np.errstate(over="ignore"):
        for seed in (0, 7, 2 ** 63 + 5):
            idx = np.arange(4096, dtype=np.uint64)
            got, want = host_normals(seed, idx), normal_restated(seed, idx)
            assert np.isfinite(got).all()
            ulps = np.abs(got - want) / np.spacing(np.abs(want))
            worst = max(worst, float(ulps.max()))
            seen.append(got)
        # the far end of the index range: idx + 1 wraps, the logarithm's argument stays in (0, 1]
        far = np.array([2 ** 64 - 1, 2 ** 64 - 2, 2 ** 63, 2 ** 53 + 1], dtype=np.uint64)
        got = host_normals(3, far)
        assert np.isfinite(got).all() and np.abs(got - normal_restated(3, far)).max() <= ULP_BOUND * np.spacing(np.abs(got)).max()
    print(f"bfhipNormalValue vs numpy: max {worst} ulp")
    assert worst <= ULP_BOUND
    assert all(len(set(s)) == len(s) for s in seen)                       # one normal per index
    assert not np.any(seen[0] == seen[1]) and not np.any(seen[1] == seen[2])      # distinct across seeds
    lib = _capi.load()
    assert lib.bfhipNormalValue(7, 5) == lib.bfhipNormalValue(7, 5)


def test_host_normals_have_the_moments_of_a_standard_normal():
    """2^18 values, each moment at a 5 sigma bound of its sampling distribution."""
    n = 1 << 18
    with np.errstate(over="ignore"):
        x = normal_restated(11, np.arange(n, dtype=np.uint64))
    # the restatement is the host function to ULP_BOUND ulp (the test above); spot-check that it is the same stream here too
    pick = np.arange(0, n, 4099)
    assert np.abs(host_normals(11, pick) - x[pick]).max() <= ULP_BOUND * np.spacing(np.abs(x[pick])).max()
    mean = x.mean()
    var = ((x - mean) ** 2).mean()
    skew = ((x - mean) ** 3).mean() / var ** 1.5
    kurt = ((x - mean) ** 4).mean() / var ** 2
    print(f"mean {mean:.3e} var-1 {var - 1:.3e} skew {skew:.3e} kurt-3 {kurt - 3:.3e}")
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1) < 5 * np.sqrt(2 / n)
    assert abs(skew) < 5 * np.sqrt(6 / n)
    assert abs(kurt - 3) < 5 * np.sqrt(24 / n)


@pytest.fixture(scope="module")
def plan_only_ops():
    rng = np.random.default_rng(77)
    desc, vals = randgraph.random_operand(rng, depth=3, size_hint=60, cplx=False, m=50, n=30)
    real = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_PLAN_ONLY | _capi.FLAG_ADJOINT)
    real_no_adjoint = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_PLAN_ONLY)
    cdesc, cvals = randgraph.random_operand(np.random.default_rng(78), depth=3, size_hint=60, cplx=True)
    cplx = HipOperator.from_desc(cdesc, cvals, flags=_capi.FLAG_PLAN_ONLY | _capi.FLAG_ADJOINT)
    yield real, real_no_adjoint, cplx
    for op in (real, real_no_adjoint, cplx):
        op.close()


def test_argument_checks_come_before_the_device(plan_only_ops):
    """No pointer below is ever dereferenced: every call ends in a check.  (0x1000 stands for "not NULL".)"""
    lib = _capi.load()
    real, real_no_adjoint, cplx = plan_only_ops
    p, h = C.c_void_p(0x1000), real.handle
    sample, matvec, draw, moments, fill = (lib.bfhipCovSampleBlockDevice, lib.bfhipCovMatvecBlockDevice, lib.bfhipCovDrawDevice,
                                           lib.bfhipCovMomentsDevice, lib.bfhipFillNormalDevice)
    # INVALID_ARGUMENTS, each reached although the operator has no device side
    assert sample(None, None, None, p, 4, p, None) == INVALID
    assert sample(h, None, None, None, 4, p, None) == INVALID
    assert sample(h, None, None, p, 4, None, None) == INVALID
    assert sample(h, None, None, p, 0, p, None) == INVALID
    assert sample(h, None, None, p, 65536, p, None) == INVALID
    assert matvec(None, None, None, None, p, 4, p, None) == INVALID
    assert matvec(h, None, None, None, None, 4, p, None) == INVALID
    assert matvec(h, None, None, None, p, 4, None, None) == INVALID
    assert matvec(h, None, None, None, p, 0, p, None) == INVALID
    assert matvec(h, None, None, None, p, 65536, p, None) == INVALID
    assert matvec(real_no_adjoint.handle, None, None, None, p, 4, p, None) == INVALID
    assert b"BFHIP_FLAG_ADJOINT" in lib.bfhipLastErrorMessage()
    assert draw(None, None, None, 1, 0, 4, p, None) == INVALID
    assert draw(h, None, None, 1, 0, 4, None, None) == INVALID
    assert draw(h, None, None, 1, 0, 0, p, None) == INVALID
    assert draw(h, None, None, 1, 0, 65536, p, None) == INVALID
    assert moments(None, None, None, 1, 0, 10, 0, p, p, None) == INVALID
    assert moments(h, None, None, 1, 0, 10, 0, None, None, None) == INVALID
    assert moments(h, None, None, 1, 0, 10, 65, p, p, None) == INVALID
    assert moments(h, None, None, 1, 0, 0, 0, p, p, None) == INVALID
    assert fill(None, 10, 0, _capi.BFHIP_F64, 1, None) == INVALID
    # with everything in order: the plan-only operator is refused, and only now
    assert sample(h, None, None, p, 4, p, None) == RUNTIME
    assert sample(h, None, None, p, 65535, p, None) == RUNTIME
    assert matvec(h, None, None, None, p, 4, p, None) == RUNTIME
    assert draw(h, None, None, 1, 0, 4, p, None) == RUNTIME
    assert moments(h, None, None, 1, 0, 10, 0, p, None, None) == RUNTIME
    assert moments(h, None, None, 1, 0, 10, 64, None, p, None) == RUNTIME
    assert b"PLAN_ONLY" in lib.bfhipLastErrorMessage()
    # TYPE_ERROR: complex operators, and fills that are not real
    ch = cplx.handle
    assert sample(ch, None, None, p, 4, p, None) == TYPE
    assert matvec(ch, None, None, None, p, 4, p, None) == TYPE
    assert draw(ch, None, None, 1, 0, 4, p, None) == TYPE
    assert moments(ch, None, None, 1, 0, 10, 0, p, p, None) == TYPE
    for dt in (_capi.BFHIP_C128, _capi.BFHIP_C64, 9):
        assert fill(p, 10, 0, dt, 1, None) == TYPE
