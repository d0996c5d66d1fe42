"""The likelihood's gradient in the density's parameters on the device (bfhipChebCovCondLogLikGradDevice),
whole calls against the long-double reference of tests/chebgrad_cases.py.

Bounds.  |got - ref| / (|t1| + |t2|), t1 = (X alpha) . (X' alpha), t2 = <X K^-1, X'>, is held to 8 times the error the same
sequence makes in plain float64 numpy against the same reference, floored at fwd_bound(n, k, cond(K)) (the yardstick and floor
of DESIGN.md section 22).  Everything else here is an identity of bits, or a refusal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chebcond_cases as cq
import chebgrad_cases as cg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


class Ctx:
    """The matrices of the cases with one ChebCovariance each; the references are made on demand, once."""
    def __init__(self):
        import torch
        from butterfly_amd import ChebCovariance
        self.dev = torch.device("cuda", 0)
        self.mats = cg.matrices()
        self.objs = {name: ChebCovariance.from_csr(m.spec["rowptr"], m.spec["colind"], m.spec["data"], m.spec["mass"], device=0)
                     for name, m in self.mats.items()}
        self._grad = {}

    def to_dev(self, x):
        import torch
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(self.dev)

    def make(self, name, k, order, noise=True):
        """(GradCase, ChebCovariance, its condition), the coefficients of `order` set just before."""
        mat, obj = self.mats[name], self.objs[name]
        case = mat.case(k, order, noise)
        if (name, k, order, noise) not in self._grad:
            self._grad[name, k, order, noise] = cg.GradCase(case)
        obj.set_coefficients(mat.coef(order))
        return self._grad[name, k, order, noise], obj, obj.condition(case.obs, case.noise if noise else None)

    def close(self):
        for o in self.objs.values():
            o.close()


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = Ctx()
    yield c
    c.close()


def grad_of(ctx, cond, gc, params, value=False):
    coef, orders = cg.coef_block(gc.mat, params)
    return cond.log_likelihood_grad_coef(ctx.to_dev(gc.case.y), coef, orders, value=value)


@pytest.mark.parametrize("name,k,order", cg.cases())
def test_every_parameter_set_against_the_long_double_reference(ctx, name, k, order):
    import torch
    gc, obj, cond = ctx.make(name, k, order)
    y = ctx.to_dev(gc.case.y)
    want_value = cond.log_likelihood(y)
    record = []
    single = {}
    for pset in cg.PARAM_SETS:
        params = cg.param_set(pset, order)
        g, v = grad_of(ctx, cond, gc, params, value=True)
        assert torch.equal(v, want_value)                                      # dValue: the likelihood entry's bits
        got = g.cpu().numpy()
        assert got.shape == (len(params),) and np.isfinite(got).all()
        for t, (nm, o) in enumerate(params):
            err, allowed = gc.error(nm, o, got[t]), gc.allowed(nm, o)
            record.append(f"{pset}:{nm}@{o}={err:.2e}({err / allowed:.2f})")
            single.setdefault((nm, o), []).append(got[t])
    print(f"RECORD {name} k={k} order={order} cond={gc.case.kappa:.2f} floor={gc.case.bound:.2e}: " + " ".join(record))
    for pset in cg.PARAM_SETS:
        for nm, o in cg.param_set(pset, order):
            for got in single[nm, o]:
                assert gc.error(nm, o, got) <= gc.allowed(nm, o), (pset, nm, o)
    # the scale identity, on the device's own outputs: the entry at q = p / 2 against the closed form
    g_scale = single["scale", order][0]
    closed = float(cond.grad_log_scale(y).cpu())
    e = abs(g_scale - closed) / gc.scale("scale", order)
    print(f"RECORD {name} k={k} order={order}: scale identity on the device {e:.2e} (allowed {2 * gc.allowed('scale', order):.2e})")
    assert gc.error("scale", order, closed) <= gc.allowed("scale", order)
    assert e <= 2 * gc.allowed("scale", order)                                 # each side within its bound of the reference
    cond.close()


@pytest.mark.parametrize("name,k,order", [("mesh4099", 130, 64), ("mesh63", 33, 2)])
def test_bitwise_identities(ctx, name, k, order):
    """Two calls and two objects give equal bits; dGrad[t] alone equals dGrad[t] inside a set of three, first and last."""
    import torch
    gc, obj, cond = ctx.make(name, k, order)
    three = cg.param_set("all", order)                                         # kappa, nu, scale
    g1 = grad_of(ctx, cond, gc, three)
    g2 = grad_of(ctx, cond, gc, three)
    again = obj.condition(gc.case.obs, gc.case.noise)
    g3 = grad_of(ctx, again, gc, three)
    assert torch.equal(g1, g2) and torch.equal(g1, g3)
    alone = grad_of(ctx, cond, gc, three[:1])
    assert torch.equal(alone[0], g1[0])
    moved = grad_of(ctx, cond, gc, [three[1], three[2], three[0]])              # kappa last
    assert torch.equal(moved[2], g1[0]) and torch.equal(moved[0], g1[1]) and torch.equal(moved[1], g1[2])
    mixed = grad_of(ctx, cond, gc, [("nu", 1), three[0], ("scale", 2)])          # among other orders, with another ldCoef
    assert torch.equal(mixed[1], g1[0])
    # the Python fit: the same coefficients, the same bits
    from butterfly_amd import matern_density_grad
    gp = cond.log_likelihood_grad(ctx.to_dev(gc.case.y), matern_density_grad(cg.KAPPA, cg.NU))
    assert torch.equal(gp, g1[:2])
    again.close(); cond.close()


def test_without_noise(ctx):
    gc, obj, cond = ctx.make("mesh63", 33, 64, noise=False)
    g = grad_of(ctx, cond, gc, cg.param_set("all", 64)).cpu().numpy()
    for t, (nm, o) in enumerate(cg.param_set("all", 64)):
        assert gc.error(nm, o, g[t]) <= gc.allowed(nm, o), nm
    closed = float(cond.grad_log_scale(ctx.to_dev(gc.case.y)).cpu())
    assert gc.error("scale", 64, closed) <= gc.allowed("scale", 64)
    cond.close()


def test_a_stale_object_is_refused_and_a_new_one_works(ctx):
    import torch
    from butterfly_amd import _capi
    gc, obj, cond = ctx.make("mesh63", 33, 2)
    params = cg.param_set("kappa", 2)
    before = grad_of(ctx, cond, gc, params)
    obj.set_coefficients(gc.mat.coef(2))                                       # the same numbers: still a new generation
    with pytest.raises(_capi.BfhipError) as ei:
        grad_of(ctx, cond, gc, params)
    assert ei.value.code == INVALID and "stale" in str(ei.value), str(ei.value)
    fresh = obj.condition(gc.case.obs, gc.case.noise)
    assert torch.equal(grad_of(ctx, fresh, gc, params), before)
    cond.close(); fresh.close()


def test_an_operator_made_condition_is_refused_and_undisturbed(ctx):
    """The seam: a CovCondition of the butterfly route refuses the entry, and gives the same bits before and after gradient
    calls on a Chebyshev object in the same process."""
    import torch
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from cond_cases import dense_leaf
    from oracle import bfref
    rng = np.random.default_rng(31)
    m, n, k, q = 90, 70, 40, 70
    desc, vals = dense_leaf(rng.standard_normal((m, n)) / np.sqrt(n))
    A = bfref.from_desc(desc, vals)
    op = HipOperator.from_bfmat(A.ptr.value, flags=_capi.FLAG_ADJOINT)
    gam = ctx.to_dev(rng.random(n) + 0.1)
    perm = torch.from_numpy(rng.permutation(m).astype(np.int64)).to(ctx.dev)
    obs, noise = rng.choice(m, size=k, replace=False), 0.05 + rng.random(k)
    y, W, E = ctx.to_dev(rng.standard_normal(k)), ctx.to_dev(rng.standard_normal((n, q))), ctx.to_dev(rng.standard_normal((k, q)))

    def run(cond):
        z, a = cond.sample_block(y, W, E, return_alpha=True)
        v, g, h = cond.log_likelihood(y, grad_log_gamma=True, grad_noise=True)
        return z, a, cond.mean(y), cond.draw(y, 5, 6, 0, q), v, g, h, cond.variance(obs[:9])

    cond = op.cov_condition(gam, perm, obs, noise)
    before = run(cond)
    lib = _capi.load()
    coef, orders = np.array([[1.0, 0.5]]), np.array([2], dtype=np.uintp)
    grad = torch.full((1,), -7.25, dtype=torch.float64, device=ctx.dev)
    rc = lib.bfhipChebCovCondLogLikGradDevice(cond.handle, C.c_void_p(y.data_ptr()), coef.ctypes.data, orders.ctypes.data, 1, 2, C.c_void_p(grad.data_ptr()),
                                              None, None, None)
    assert rc == INVALID and b"bfhipChebCovCondCreate" in lib.bfhipLastErrorMessage()
    torch.cuda.synchronize()
    assert float(grad.cpu()) == -7.25                                         # nothing was enqueued
    gc, obj, cheb_cond = ctx.make("mesh63", 33, 64)
    grad_of(ctx, cheb_cond, gc, cg.param_set("all", 64))
    after = run(cond)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    cheb_cond.close(); cond.close(); op.close()


def test_a_chebyshev_objects_samples_are_undisturbed(ctx):
    """The gradient shares cheb's workspace and the object's W' block with the sample path: its bits before and after."""
    import torch
    gc, obj, cond = ctx.make("mesh4099", 130, 2)
    case = gc.case
    y, W, E = ctx.to_dev(case.y), ctx.to_dev(case.W), ctx.to_dev(case.E)

    def run():
        z, a = cond.sample_block(y, W, E, return_alpha=True)
        v, _, h = cond.log_likelihood(y, grad_noise=True)
        return z, a, cond.mean(y), cond.draw(y, 5, 6, 0, 70), v, h, cond.variance(case.query)

    before = run()
    g = grad_of(ctx, cond, gc, cg.param_set("mixed", 2))
    after = run()
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert torch.equal(grad_of(ctx, cond, gc, cg.param_set("mixed", 2)), g)    # and the other way round
    cond.close()


def test_the_c_driver_builds_with_werror_and_exits_zero(tmp_path):
    """examples/cheb_gradient_device.c: d logLik / d kappa on the 1154-vertex sphere against central differences of the library's
    own likelihood over four more Creates; exit 0 only if |grad - FD(h)| <= |FD(h) - FD(2h)|."""
    lib = os.path.join(ROOT, "butterfly_amd", "csrc")
    exe = str(tmp_path / "cheb_gradient_device")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cheb_gradient_device.c"), "-L", lib, "-lbfhip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-lm", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0
    assert "FD(h)" in p.stdout and "FD(2h)" in p.stdout and "grad" in p.stdout
