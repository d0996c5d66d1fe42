"""Conditioning the Chebyshev route on observations, on the device (bfhipChebCovCondCreate), against the
long-double reference of tests/chebcond_cases.py: X = p(S) D E_obs by the reference's forward recurrence, then G, the Cholesky
factor, the solves and Z = D p(S) (W + X alpha) in numpy.longdouble.

Bounds.  Per column, the relative l2 error of alpha, mean, Z, grad_noise and the prior and posterior variances (the three
likelihood values entry by entry) is held to 8 times the error the same sequence makes in plain float64 numpy against the same
reference (the yardstick of DESIGN.md section 22; 8 is its allowance for another summation order), floored at
fwd_bound(n, k, cond(G + D)) of tests/test_gpu_cov_condition.py.  The backward error of alpha in G + D is held to 1e-12, the
project's float64 tolerance (it carries no condition number).  The moments are held to K 2^-52 sum |z|."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chebcond_cases as cq
from test_gpu_cov_condition import check_moments

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, OUT_OF_RANGE = 1, 5
CASES = [(name, k, order) for name in ("mesh4099", "mesh63", "n1") for k, order in cq.cases_of(name)]


class Ctx:
    """The matrices of the cases with one ChebCovariance each; the references are made on demand, once."""
    def __init__(self):
        import torch
        from butterfly_amd import ChebCovariance
        self.dev = torch.device("cuda", 0)
        self.mats = cq.matrices()
        self.objs = {name: ChebCovariance.from_csr(m.spec["rowptr"], m.spec["colind"], m.spec["data"], m.spec["mass"], device=0)
                     for name, m in self.mats.items()}

    def to_dev(self, x):
        import torch
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(self.dev)

    def make(self, name, k, order, noise=True):
        """(case, ChebCovariance, its CovCondition), the coefficients of `order` set just before."""
        mat, obj = self.mats[name], self.objs[name]
        case = mat.case(k, order, noise)
        obj.set_coefficients(mat.coef(order))
        return case, obj, obj.condition(case.obs, case.noise if noise else None)

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


def held(case, name, got, cols=None):
    """Asserts the device's `name` within its bound; returns (worst error, worst error / bound) for the record."""
    ref, _ = case.results()
    want, allowed = ref[name], case.allowed(name)
    if cols is not None:
        want, allowed = want[:, cols], allowed[cols]
    err = cq.rel_errs(name, got, want)
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all() and (err <= allowed).all(), (name, float((err / allowed).max()))
    return float(np.max(err)), float(np.max(err / allowed))


def sample(ctx, cond, case, q):
    z, a = cond.sample_block(ctx.to_dev(case.y), ctx.to_dev(case.W[:, :q]), ctx.to_dev(case.E[:, :q]), return_alpha=True)
    return z.cpu().numpy(), a.cpu().numpy()


@pytest.mark.parametrize("name,k,order", CASES)
def test_every_entry_against_the_long_double_reference(ctx, name, k, order):
    import torch
    case, obj, cond = ctx.make(name, k, order)
    n, mat = case.mat.n, case.mat
    info = cond.info
    chunks = cq.num_chunks(n)
    assert info["numObs"] == k and info["setupApplies"] == (k + 63) // 64 and 0 < info["minPivot"] <= info["maxPivot"]
    # X, L, R and E blocks, the draw's normals, the partial sums, the object's own W' block, the noise and its roots
    assert info["factorBytes"] == 8 * (n * k + k * k + 2 * k * 64 + n * 64 + chunks * k * 64 + n * 64 + 2 * k)
    assert case.kappa <= case.kappa_bound
    worst = {}
    full_z, full_a = sample(ctx, cond, case, cq.MAXQ)
    for q in cq.QS:
        z, a = (full_z, full_a) if q == cq.MAXQ else sample(ctx, cond, case, q)
        assert z.shape == (n, q) and a.shape == (k, q)
        # a column does not depend on nrhs or on the pass it falls in: the bits of the 70-column call
        assert np.array_equal(z, full_z[:, :q]) and np.array_equal(a, full_a[:, :q]), q
        be = case.backward_error(a, case.residual(case.y, case.W[:, :q], case.E[:, :q]))
        assert be <= 1e-12, be
        zc = mat.zcols[mat.zcols < q]
        for nm, got, cols in (("alpha", a, np.arange(q)), ("Z", z[:, zc], np.arange(len(zc)))):
            worst[nm] = max(worst.get(nm, (0, 0)), held(case, nm, got, cols))
        worst["backward"] = max(worst.get("backward", (0, 0)), (be, be / 1e-12))
    y = ctx.to_dev(case.y)
    mean, a1 = cond.mean(y, return_alpha=True)
    worst["mean"] = held(case, "mean", mean.cpu().numpy())
    held(case, "alpha_y", a1.cpu().numpy())
    z0, a0 = cond.sample_block(y, torch.zeros((n, 1), dtype=torch.float64, device=ctx.dev), None, return_alpha=True)
    assert torch.equal(mean, z0[:, 0]) and torch.equal(a1, a0[:, 0])          # the mean is the block entry with W = 0, bit for bit
    value, g, h = cond.log_likelihood(y, grad_noise=True)
    assert g is None
    worst["value"] = held(case, "value", value.cpu().numpy())
    worst["grad_noise"] = held(case, "grad_noise", h.cpu().numpy())
    assert torch.equal(cond.log_likelihood(y), value)
    post, prior = cond.variance(case.query, prior=True)
    worst["prior"] = held(case, "prior", prior.cpu().numpy())
    worst["post"] = held(case, "post", post.cpu().numpy())
    assert torch.equal(cond.variance(case.query, prior=True, post=False), prior)
    print(f"RECORD {name} k={k} order={order} cond={case.kappa:.2f} floor={case.bound:.2e}: "
          + " ".join(f"{nm}={e:.2e}({r:.2f})" for nm, (e, r) in worst.items()))
    cond.close()


def device_blocks(ctx, n, k, sd, seed, noise_seed, first, q):
    """The blocks a draw is defined by: W[j, s] = N(seed, (first + s) n + j), E[a, s] = sd[a] N(noise_seed, (first + s) k + a):
    sample-major streams of bfhipFillNormalDevice, transposed into the block layout."""
    import torch
    from butterfly_amd import _capi
    lib = _capi.load()
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    out = []
    for rows, sd_, s_ in ((n, None, seed), (k, sd, noise_seed)):
        t = torch.empty((q, rows), dtype=torch.float64, device=ctx.dev)
        with torch.cuda.device(0):
            assert lib.bfhipFillNormalDevice(C.c_void_p(t.data_ptr()), q * rows, first * rows, _capi.BFHIP_F64, s_, stream) == 0
        t = t.t().contiguous()
        out.append(t if sd_ is None else (sd_[:, None] * t).contiguous())
    return out


@pytest.mark.parametrize("name,k,order", [("mesh4099", 130, 2), ("mesh63", 33, 64)])
def test_bitwise_identities(ctx, name, k, order):
    """Two objects made the same way give the same bits; draw is sample_block on the blocks of the device's normal streams,
    whatever the split into calls."""
    import torch
    case, obj, cond = ctx.make(name, k, order)
    n = case.mat.n
    y, sd = ctx.to_dev(case.y), ctx.to_dev(np.sqrt(case.noise))
    seed, nseed, first = 99, 1234, 5
    for q in cq.QS:
        W, E = device_blocks(ctx, n, k, sd, seed, nseed, first, q)
        assert torch.equal(cond.draw(y, seed, nseed, first, q), cond.sample_block(y, W, E)), q
    whole = cond.draw(y, seed, nseed, 0, 70)
    parts = torch.cat([cond.draw(y, seed, nseed, 0, 3), cond.draw(y, seed, nseed, 3, 67)], dim=1)
    assert torch.equal(parts, whole)
    # the W stream is bfhipChebCovDrawDevice's
    W, _ = device_blocks(ctx, n, k, sd, seed, nseed, 7, 3)
    assert torch.equal(obj.draw_device(seed, 7, 3), obj.sample_block_device(W))
    W, E = device_blocks(ctx, n, k, sd, seed, nseed, first, 70)
    z1, a1 = cond.sample_block(y, W, E, return_alpha=True)
    z1b, a1b = cond.sample_block(y, W, E, return_alpha=True)
    again = obj.condition(case.obs, case.noise)                                # no set_coefficients in between: both stay live
    z2, a2 = again.sample_block(y, W, E, return_alpha=True)
    assert torch.equal(z1, z1b) and torch.equal(a1, a1b) and torch.equal(z1, z2) and torch.equal(a1, a2)
    v1, _, h1 = cond.log_likelihood(y, grad_noise=True)
    v2, _, h2 = again.log_likelihood(y, grad_noise=True)
    assert torch.equal(v1, v2) and torch.equal(h1, h2)
    assert torch.equal(cond.variance(case.query), again.variance(case.query))
    again.close(); cond.close()


@pytest.mark.parametrize("name,k,order", [("mesh4099", 33, 2), ("mesh63", 33, 64)])
def test_streaming_moments_of_conditioned_draws(ctx, name, k, order):
    """150 samples as 64 + 64 + 22 against the stored draws; += into sums that are not zero; a NULL output."""
    import torch
    case, obj, cond = ctx.make(name, k, order)
    n, K = case.mat.n, 150
    y = ctx.to_dev(case.y)
    seed, nseed = 4242, 77
    Z = torch.cat([cond.draw(y, seed, nseed, f, b) for f, b in ((0, 64), (64, 64), (128, 22))], dim=1).cpu().numpy()
    s, q = torch.zeros(n, dtype=torch.float64, device=ctx.dev), torch.zeros(n, dtype=torch.float64, device=ctx.dev)
    cond.moments(y, seed, nseed, 0, K, 64, s, q)
    check_moments(Z, s.cpu().numpy(), q.cpu().numpy(), K)
    s2, q2 = torch.zeros_like(s), torch.zeros_like(q)
    cond.moments(y, seed, nseed, 0, K, 0, s2, q2)                              # batch 0 means 64; two runs, the same bits
    assert torch.equal(s, s2) and torch.equal(q, q2)
    s3, q3 = torch.zeros_like(s), torch.zeros_like(q)
    cond.moments(y, seed, nseed, 0, K, 64, s3, None)
    cond.moments(y, seed, nseed, 0, K, 64, None, q3)
    assert torch.equal(s3, s) and torch.equal(q3, q)
    rng = np.random.default_rng(12)
    base_s, base_q = rng.standard_normal(n), rng.random(n)
    s4, q4 = ctx.to_dev(base_s), ctx.to_dev(base_q)
    cond.moments(y, seed, nseed, 0, K, 64, s4, q4)
    check_moments(Z, s4.cpu().numpy(), q4.cpu().numpy(), K + 1, base_s, base_q)
    with pytest.raises(Exception) as ei:
        cond.moments(y, seed, nseed, 0, K, 64, None, None)
    assert ei.value.code == INVALID
    cond.close()


def test_without_noise(ctx):
    """noise_var=None on mesh63, k = 33: G = X^T X alone is factored; the observed values are reproduced by the mean."""
    case, obj, cond = ctx.make("mesh63", 33, 64, noise=False)
    assert not case.noise.any()
    z, a = sample(ctx, cond, case, cq.MAXQ)
    e_a, e_z = held(case, "alpha", a), held(case, "Z", z)
    y = ctx.to_dev(case.y)
    mean = cond.mean(y).cpu().numpy()
    e_m = held(case, "mean", mean)
    e_v = held(case, "value", cond.log_likelihood(y).cpu().numpy())
    post, prior = cond.variance(case.query, prior=True)
    e_p, e_q = held(case, "prior", prior.cpu().numpy()), held(case, "post", post.cpu().numpy())
    ref, _ = case.results()
    misfit = float(np.linalg.norm(mean[case.obs] - case.y))
    print(f"RECORD mesh63 k=33 order=64 no noise cond={case.kappa:.2f} floor={case.bound:.2e}: alpha={e_a[0]:.2e}({e_a[1]:.2f}) Z={e_z[0]:.2e}({e_z[1]:.2f}) "
          f"mean={e_m[0]:.2e}({e_m[1]:.2f}) value={e_v[0]:.2e}({e_v[1]:.2f}) prior={e_p[0]:.2e}({e_p[1]:.2f}) post={e_q[0]:.2e}({e_q[1]:.2f}); "
          f"|mean at the observed vertices - y| / |y| = {misfit / np.linalg.norm(case.y):.2e}")
    # the reference mean interpolates (G alpha = y), so the misfit at the observed vertices is part of the mean's error, which
    # the bound above holds to allowed * ||mean||; the second term is the long-double reference's own residual
    mean_ref = ref["mean"]
    assert misfit <= float(case.allowed("mean")[0] * np.linalg.norm(mean_ref.astype(np.float64)) + np.linalg.norm((mean_ref[case.obs] - case.y).astype(np.float64)))
    cond.close()


def test_stale_coefficients_refuse_every_entry_and_a_new_object_works(ctx):
    import torch
    from butterfly_amd import _capi
    case, obj, cond = ctx.make("mesh63", 33, 2)
    n, k = case.mat.n, case.k
    y, W = ctx.to_dev(case.y), ctx.to_dev(case.W[:, :3])
    z_before = cond.sample_block(y, W)
    obj.set_coefficients(case.mat.coef(2))                                     # the same numbers: still a new generation
    s = torch.zeros(n, dtype=torch.float64, device=ctx.dev)
    calls = (lambda: cond.sample_block(y, W), lambda: cond.mean(y), lambda: cond.draw(y, 1, 2, 0, 3), lambda: cond.moments(y, 1, 2, 0, 3, 64, s, None),
             lambda: cond.log_likelihood(y), lambda: cond.log_likelihood(y, grad_noise=True), lambda: cond.variance(case.query))
    for call in calls:
        with pytest.raises(_capi.BfhipError) as ei:
            call()
        assert ei.value.code == INVALID and "stale" in str(ei.value), str(ei.value)
    assert not s.any()                                                         # nothing was enqueued
    info = cond.info
    assert info["numObs"] == k and info["factorBytes"] > 8 * n * k
    fresh = obj.condition(case.obs, case.noise)
    assert torch.equal(fresh.sample_block(y, W), z_before)
    cond.close(); fresh.close()


def test_refusals_that_read_the_object(ctx):
    from butterfly_amd import ChebCovariance, _capi
    case, obj, cond = ctx.make("mesh63", 33, 2)
    n, k = case.mat.n, case.k
    y = ctx.to_dev(case.y)
    with pytest.raises(_capi.BfhipError) as ei:
        cond.log_likelihood(y, grad_log_gamma=True)
    assert ei.value.code == INVALID and "per-column weights" in str(ei.value)
    with pytest.raises(_capi.BfhipError) as ei:
        cond.log_likelihood(y, grad_log_gamma=True, grad_noise=True)
    assert ei.value.code == INVALID
    with pytest.raises(_capi.BfhipError) as ei:
        cond.variance(np.array([0, n]))
    assert ei.value.code == OUT_OF_RANGE
    with pytest.raises(_capi.BfhipError) as ei:
        cond.variance(np.array([3, 5, 3]))
    assert ei.value.code == INVALID and "repeated" in str(ei.value)
    cond.close()
    with pytest.raises(_capi.BfhipError) as ei:
        obj.condition(np.array([0, n]), None)
    assert ei.value.code == OUT_OF_RANGE
    with pytest.raises(_capi.BfhipError) as ei:
        obj.condition(np.array([0, 1]), np.array([0.1, -0.1]))
    assert ei.value.code == INVALID and "noiseVar[1]" in str(ei.value)
    m = case.mat
    bare = ChebCovariance.from_csr(m.spec["rowptr"], m.spec["colind"], m.spec["data"], m.spec["mass"], device=0)
    with pytest.raises(_capi.BfhipError) as ei:
        bare.condition(case.obs, case.noise)
    assert ei.value.code == INVALID and "no coefficients" in str(ei.value)
    bare.close()
    obj.condition(case.obs, case.noise).close()                                # the object is as it was


def test_an_operator_made_condition_is_undisturbed(ctx):
    """The seam: a CovCondition of the butterfly route on a small dense leaf gives the same bits before and after a Chebyshev
    object is created and used in the same process."""
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
        s = torch.zeros(m, dtype=torch.float64, device=ctx.dev)
        cond.moments(y, 5, 6, 0, 70, 64, s, None)
        return z, a, cond.mean(y), cond.draw(y, 5, 6, 0, q), s, v, g, h, cond.variance(obs[:9])

    cond = op.cov_condition(gam, perm, obs, noise)
    before = run(cond)
    info = cond.info
    assert info["factorBytes"] == 8 * (n * k + k * k + 2 * k * 64 + n * 64 + k * 64 + 2 * k)      # what it was: no W' block of its own
    case, obj, cheb_cond = ctx.make("mesh63", 33, 64)
    sample(ctx, cheb_cond, case, cq.MAXQ)
    cheb_cond.variance(case.query)
    after = run(cond)
    other = op.cov_condition(gam, perm, obs, noise)
    new = run(other)
    for a, b, c in zip(before, after, new):
        assert torch.equal(a, b) and torch.equal(a, c)
    cheb_cond.close(); other.close(); cond.close(); op.close()


def test_the_c_driver_builds_with_werror_and_exits_zero(tmp_path):
    """examples/cheb_condition_device.c: a lat-lon sphere made in the program; with a tiny noise the kriging mean reproduces the
    observed values of a prior draw and the posterior variance there is at most the noise variance -- exit 0 only if both hold."""
    lib = os.path.join(ROOT, "butterfly_amd", "csrc")
    exe = str(tmp_path / "cheb_condition_device")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cheb_condition_device.c"), "-L", lib, "-lbfhip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-lm", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe, "24", "48", "32", "40"], capture_output=True, text=True, timeout=120)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0
    assert "kriging mean" in p.stdout and "posterior variance" in p.stdout
