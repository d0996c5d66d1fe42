"""The likelihood's gradient in the density's parameters on the Chebyshev route, without a GPU: the
exports and prototypes, every refusal of bfhipChebCovCondLogLikGradDevice that needs the arguments alone, in the header's order
(the refusals that read the object -- not a Chebyshev object, a stale one -- are in tests/test_gpu_cheb_gradient.py), and what
tests/chebgrad_cases.py claims of its cases on the long-double reference alone."""
import ctypes as C

import numpy as np
import pytest

import chebgrad_cases as cg
from butterfly_amd import _capi

INVALID = 1
LD = np.longdouble


@pytest.fixture(scope="module")
def mats():
    return cg.matrices()


@pytest.fixture(scope="module")
def grad_cases(mats):
    made = {}

    def get(name, k, order):
        if (name, k, order) not in made:
            made[name, k, order] = cg.GradCase(mats[name].case(k, order))
        return made[name, k, order]
    return get


def test_the_new_symbols_are_exported():
    import butterfly_amd
    from butterfly_amd.operator import ChebCovCondition, CovCondition
    lib = _capi.load()
    fn = lib.bfhipChebCovCondLogLikGradDevice
    assert fn.restype is C.c_int and len(fn.argtypes) == 10 and fn.argtypes[4] is C.c_size_t and fn.argtypes[5] is C.c_size_t
    for name in ("bfdevLikGradContract", "bfdevLikGradDot", "bfdevLikGradSum", "bfdevLikGradM", "bfdevLikGradUnit"):
        assert hasattr(lib, name), name
    for name in ("log_likelihood_grad", "log_likelihood_grad_coef", "grad_log_scale"):
        assert callable(getattr(ChebCovCondition, name)) and not hasattr(CovCondition, name), name
    assert callable(butterfly_amd.matern_density_grad)
    assert len(butterfly_amd.matern_density_grad(2.0, 2.0)) == 2 and len(butterfly_amd.matern_density_grad(0.5, 0)) == 1


def test_the_density_derivatives_are_the_derivatives_of_the_density():
    """matern_density_grad against central differences of matern_density, in both families."""
    from butterfly_amd import matern_density, matern_density_grad
    lam, h = np.linspace(0.0, 7.0, 29), 1e-5
    for kappa, nu in ((2.0, 2.0), (0.7, 5.0), (1.3, 0.0)):
        grads = matern_density_grad(kappa, nu)
        fd = [(matern_density(kappa + h, nu)(lam) - matern_density(kappa - h, nu)(lam)) / (2 * h)]
        if nu:
            fd.append((matern_density(kappa, nu + h)(lam) - matern_density(kappa, nu - h)(lam)) / (2 * h))
        assert len(grads) == len(fd)
        for g, want in zip(grads, fd):
            assert np.abs(g(lam) - want).max() <= 1e-8, (kappa, nu)


def test_argument_refusals_in_order_read_nothing_through_the_object():
    """0x1000 stands for "not NULL": the stand-in object and dY and dGrad are never dereferenced.  The order is the header's:
    NULLs, numParams, the orders, the coefficients, structSize."""
    lib = _capi.load()
    fn, msg = lib.bfhipChebCovCondLogLikGradDevice, lib.bfhipLastErrorMessage
    p = C.c_void_p(0x1000)
    coef = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    orders = np.array([3, 2], dtype=np.uintp)
    good = _capi.BfhipCovCondLikOptions()
    good.structSize = C.sizeof(good)
    bad = _capi.BfhipCovCondLikOptions()
    bad.structSize = C.sizeof(bad) + 8

    def refused(want, c=p, y=p, cf=coef, od=orders, num=2, ld=3, grad=p, opt=good):
        rc = fn(c, y, cf.ctypes.data if cf is not None else None, od.ctypes.data if od is not None else None, num, ld, grad, None, C.byref(opt), None)
        assert rc == INVALID and want in msg(), (rc, msg())

    refused(b"NULL", c=None)
    refused(b"NULL", y=None)
    refused(b"NULL", cf=None)
    refused(b"NULL", od=None)
    refused(b"NULL", grad=None)
    refused(b"NULL", c=None, num=0)                                           # a NULL wins over a bad numParams
    refused(b"numParams", num=0)
    refused(b"numParams", num=65)
    refused(b"numParams", num=0, od=np.array([0, 0], dtype=np.uintp))          # numParams wins over the orders
    refused(b"orders[1]", od=np.array([3, 0], dtype=np.uintp))
    refused(b"orders[0]", od=np.array([4, 2], dtype=np.uintp))
    for v in (np.nan, np.inf, -np.inf):
        cf = coef.copy()
        cf[1, 1] = v
        refused(b"coefficient 1 of parameter 1", cf=cf)
        refused(b"orders[0]", cf=cf, od=np.array([0, 2], dtype=np.uintp))      # the orders win over the coefficients
        refused(b"coefficient 1 of parameter 1", cf=cf, opt=bad)               # the coefficients win over structSize
    cf = coef.copy()
    cf[1, 2] = np.nan                                                          # beyond orders[1]: not read
    refused(b"structSize", cf=cf, opt=bad)
    refused(b"structSize", opt=bad)


def test_central_differences_of_the_long_double_likelihood_converge_to_the_gradient(mats, grad_cases):
    """mesh63, k = 33, order 64: |FD(h) - grad| falls by 4 from h = 1e-2 to 5e-3, in kappa and in nu -- the formula is the
    derivative of the discrete likelihood, coefficient fit included."""
    mat, order = mats["mesh63"], 64
    gc = grad_cases("mesh63", 33, order)
    from butterfly_amd import cheb_fit, matern_density

    def lik(kappa, nu):
        return cg.likelihood_ld(mat, gc.case, cheb_fit(matern_density(kappa, nu), order, 0.0, mat.lam_max))

    for name, step in (("kappa", (1, 0)), ("nu", (0, 1))):
        ref = gc.terms(name, order, LD)[0]
        errs = []
        for h in (1e-2, 5e-3):
            fd = (lik(cg.KAPPA + h * step[0], cg.NU + h * step[1]) - lik(cg.KAPPA - h * step[0], cg.NU - h * step[1])) / (2 * LD(h))
            errs.append(float(abs(fd - ref)))
        print(f"mesh63 k=33 order=64 d/d{name}: grad {float(ref):.12e}, |FD(1e-2) - grad| {errs[0]:.3e}, |FD(5e-3) - grad| {errs[1]:.3e}, ratio {errs[0] / errs[1]:.3f}")
        assert 3 <= errs[0] / errs[1] <= 5


@pytest.mark.parametrize("name,k,order", cg.cases())
def test_the_scale_identity_and_the_float64_sequence(grad_cases, name, k, order):
    """For q = p / 2 the gradient is (quad - k) / 2 - sum noiseVar gradNoise, in long double to the floor and in the float64
    sequence within its yardstick; and the float64 sequence passes every bound the device is held to."""
    gc = grad_cases(name, k, order)
    ref = gc.terms("scale", order, LD)[0]
    closed = gc.closed_form_scale(LD)
    e_ld = float(abs(closed - ref)) / gc.scale("scale", order)
    e_64 = gc.error("scale", order, gc.closed_form_scale(np.float64))
    print(f"{name} k={k} order={order}: scale identity in long double {e_ld:.2e}, float64 closed form {e_64:.2e} (allowed {gc.allowed('scale', order):.2e})")
    assert e_ld <= 1e-15 * max(1.0, gc.case.kappa)
    assert e_64 <= gc.allowed("scale", order)
    for pset in cg.PARAM_SETS:
        for nm, o in cg.param_set(pset, order):
            e, allowed = gc.f64_error(nm, o), gc.allowed(nm, o)
            assert np.isfinite(e) and e <= allowed and allowed >= gc.case.bound, (nm, o, e, allowed)


@pytest.mark.parametrize("k,order", [(33, 1), (33, 2), (33, 64), (130, 1), (130, 2), (130, 64)])
def test_every_chunk_tile_and_k_step_moves_the_gradient(grad_cases, k, order):
    """On the reference alone, mesh4099: leaving any one of the five chunks of rows out of the dot, any live 16-column tile of Y,
    or the last k-step of the contraction (33 = 32 + 1, 130 = 128 + 2) moves d/d kappa by at least 1e3 times the allowed error."""
    gc = grad_cases("mesh4099", k, order)
    allowed = gc.allowed("kappa", order)
    om = gc.omissions("kappa", order)
    print(f"mesh4099 k={k} order={order}: allowed {allowed:.2e}; " + ", ".join(f"{'-'.join(map(str, w))} {v:.2e}" for w, v in om.items()))
    assert sum(1 for w in om if w[0] == "chunk") == 5 and sum(1 for w in om if w[0] == "tile") == -(-k // 16)
    assert sum(1 for w in om if w[0] == "kstep") == 1 and k % 4
    assert min(om.values()) >= 1e3 * allowed
