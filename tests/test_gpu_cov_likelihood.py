"""Log-likelihood with gradients and exact kriging variances of a conditioned field, on the device,
against the long-double reference of tests/test_cov_likelihood_cpu.py (whose formulas that file checks against central
differences).

The operand is the one of tests/test_gpu_cov_condition.py, restated: 211 x 93, gamma in [0.1, 1.1) -- here with three
entries set to zero --, a random row permutation; one operator per element type (F64, F32 by demote_to_f32) and per switch
state (block switches off, and on at minRhs = 2).  F64: rho = 0.01, k in {1, 5, 64, 65, 130}; F32: rho = 1, k in {5, 65}.
noiseVar[a] = rho trace(G) / k (0.5 + u_a), so cond(K) <= 1 + 3 k / rho, which every case asserts first.

Bounds, with tol = 1e-12 (F64) / 2e-5 (F32), the project's apply tolerances, and kappa, lambda_min, alpha, quad, p, b_j taken
from the reference (first-order perturbation bounds for rows of B accurate to tol: ||dK|| <= 2 tol ||K||, B^T K^-1 B <= I,
constants rounded up):
  |logLik - ref| <= 4 tol kappa (quad + k),  |quad - ref| <= 4 tol kappa quad,  |logDet - ref| <= 4 tol kappa k
  |gradLogGamma_j - ref| <= 8 tol kappa (||alpha||^2 + 1 / lambda_min) ||b_j||^2
  |gradNoise_a - ref|    <= 8 tol kappa (||alpha||^2 + 1 / lambda_min)
  |dPost_t - ref| <= 8 tol kappa p_t,  |dPrior_t - ref| <= 4 tol p_t
Every figure is printed before it is asserted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_cov_likelihood_cpu import LD, LikReference, forward_ld
from test_gpu_cov_condition import Oracle, Reference, input_of, permute_rows, tol_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N = 211, 93
ZERO_COLS = (7, 40, 92)
RHO = {False: 0.01, True: 1.0}
KS = {False: (1, 5, 64, 65, 130), True: (5, 65)}
CASES = [(demote, k) for demote in (False, True) for k in KS[demote]]


@pytest.fixture(scope="module")
def case():
    import torch
    import randgraph
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from oracle import bfref
    rng = np.random.default_rng(77)
    desc, vals = randgraph.random_operand(rng, depth=4, size_hint=120, cplx=False, m=M, n=N)
    A = bfref.from_desc(desc, vals)
    gam = rng.random(N) + 0.1
    gam[list(ZERO_COLS)] = 0.0
    row_perm = rng.permutation(M)
    rev = np.empty(M, dtype=np.int64); rev[row_perm] = np.arange(M)
    dev = torch.device("cuda", 0)
    c = dict(dev=dev, rev=rev, row_perm=row_perm, perm=torch.from_numpy(row_perm.astype(np.int64)).to(dev), ops={}, gam={}, ref={}, lik={}, rows={}, rng=rng)
    phi = Oracle(A, gam, row_perm).apply(np.eye(N))                        # dense Phi, from the oracle
    for demote in (False, True):
        g = input_of(gam, demote)
        c["gam"][demote] = torch.from_numpy(g).to(dev).to(torch.float32 if demote else torch.float64)
        c["rows"][demote] = permute_rows(phi.astype(LD) * g.astype(LD), row_perm)   # P Phi Gamma, [m x n]: row o is r_o
        for blocks in (False, True):
            op = HipOperator.from_bfmat(A.ptr.value, flags=_capi.FLAG_ADJOINT, demote_to_f32=demote)
            if blocks:
                op.set_real_rhs_blocks(2)
                op.set_adjoint_rhs_blocks(2)
            c["ops"][demote, blocks] = op
        for k in KS[demote]:
            krng = np.random.default_rng(1000 + k)
            obs = krng.choice(M, size=k, replace=False)
            ref = Reference(phi[rev[obs], :].T, g, obs, RHO[demote], krng, phi=phi, row_perm=row_perm)
            ref.y = np.asarray(ref.Bt.T @ krng.standard_normal(N) + np.sqrt(ref.noise) * krng.standard_normal(k), dtype=np.float64)
            ref.lam_min = float(np.linalg.eigvalsh(ref.A.astype(np.float64))[0])
            c["ref"][demote, k] = ref
            c["lik"][demote, k] = LikReference(ref.Bt, ref.noise, ref.y)        # computed once, shared, never changed
    yield c
    for op in c["ops"].values():
        op.close()


def to_dev(c, x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(c["dev"])


def make_cond(c, demote, blocks, k):
    ref = c["ref"][demote, k]
    return c["ops"][demote, blocks].cov_condition(c["gam"][demote], c["perm"], ref.obs, ref.noise), ref


def lik_bounds(ref, lik, tol):
    """(value bounds [3], gradLogGamma bounds [n], gradNoise bound) from the reference alone."""
    kap, k = ref.kappa, ref.k
    quad, a2 = float(lik.quad), float(lik.alpha @ lik.alpha)
    val = np.array([4 * tol * kap * (quad + k), 4 * tol * kap * quad, 4 * tol * kap * k])
    grad = 8 * tol * kap * (a2 + 1 / ref.lam_min)
    return val, grad * lik.bnorm2.astype(np.float64), grad


def err(got, want):
    return np.abs(np.asarray((got.cpu().numpy().astype(LD) - want), dtype=np.float64))


@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("demote,k", CASES)
def test_values_and_gradients(case, demote, k, blocks):
    """Value and both gradients against the reference at the default workspace and at a workspace of exactly one strip (one
    workgroup walks both strips of n = 93 and the three of k = 130); the two agree within the same bounds; each is bit for
    bit repeatable; homogeneity on device outputs alone; the zero weights give exact zeros; NULL gradients change nothing."""
    import torch
    c, tol = case, tol_of(demote)
    cond, ref = make_cond(c, demote, blocks, k)
    lik = c["lik"][demote, k]
    print(f"demote={demote} k={k} blocks={blocks}: cond(K) = {ref.kappa:.3e} (bound {ref.kappa_bound:.3e}), lambda_min = {ref.lam_min:.3e}, quad = {float(lik.quad):.6e}")
    assert ref.kappa <= ref.kappa_bound
    bv, bg, bh = lik_bounds(ref, lik, tol)
    want_v = np.array([lik.loglik, lik.quad, lik.logdet], dtype=LD)
    y = to_dev(c, ref.y)
    d = ref.noise.astype(LD)
    out = {}
    for name, ws in (("default", 0), ("one strip", k * 64 * 8)):
        v, g, h = cond.log_likelihood(y, grad_log_gamma=True, grad_noise=True, workspace_bytes=ws)
        ev, eg, eh = err(v, want_v), err(g, lik.g), err(h, lik.h)
        nz = bg > 0
        print(f"  {name}: |value err| / bound = {np.array2string(ev / bv, precision=3)}; gradLogGamma max err/bound {np.max(eg[nz] / bg[nz]):.3e} "
              f"(max err {eg.max():.3e}); gradNoise max err/bound {eh.max() / bh:.3e} (max err {eh.max():.3e})")
        assert np.all(ev <= bv)
        assert np.all(eg <= bg)
        assert np.all(eh <= bh)
        # zero weights: exactly zero (the bound is zero there too)
        assert all(float(g[j]) == 0.0 and not np.signbit(float(g[j])) for j in ZERO_COLS)
        # homogeneity, device outputs alone
        gv, hv, vv = g.cpu().numpy().astype(LD), h.cpu().numpy().astype(LD), v.cpu().numpy().astype(LD)
        hom, hb = float(abs(gv.sum() / 2 + hv @ d - (vv[1] - k) / 2)), 8 * tol * ref.kappa * (float(lik.quad) + k)
        print(f"  {name}: homogeneity residual {hom:.3e} (bound {hb:.3e})")
        assert hom <= hb
        v2, g2, h2 = cond.log_likelihood(y, grad_log_gamma=True, grad_noise=True, workspace_bytes=ws)
        assert torch.equal(v, v2) and torch.equal(g, g2) and torch.equal(h, h2)
        out[name] = (v, g, h)
    (v0, g0, h0), (v1, g1, h1) = out["default"], out["one strip"]
    dv, dg, dh = (np.abs((a - b).cpu().numpy()) for a, b in ((v0, v1), (g0, g1), (h0, h1)))
    print(f"  default vs one strip: max |diff| value {dv.max():.3e} gradLogGamma {dg.max():.3e} gradNoise {dh.max():.3e}")
    assert np.all(dv <= bv) and np.all(dg <= bg) and np.all(dh <= bh)
    # NULL gradient outputs: the value alone, the same bits; one gradient at a time, the same bits
    assert torch.equal(cond.log_likelihood(y), v0)
    vg, gg, none = cond.log_likelihood(y, grad_log_gamma=True)
    assert none is None and torch.equal(vg, v0) and torch.equal(gg, g0)
    vh, none, hh = cond.log_likelihood(y, grad_noise=True)
    assert none is None and torch.equal(vh, v0) and torch.equal(hh, h0)
    cond.close()


def query_sets(ref, rng):
    """1, 64 and 65 indices and all 211 rows in a shuffled order; observed points lead the short ones."""
    rest = np.setdiff1d(np.arange(M), ref.obs)
    some = np.concatenate([ref.obs[:8], rng.permutation(rest)])
    return [some[:1], some[:64][::-1].copy(), some[:65], rng.permutation(M)]


def variance_reference(c, ref, demote, q):
    r = c["rows"][demote][q, :]                                             # [t x n]
    p = (r ** 2).sum(axis=1)
    return p, p - (forward_ld(ref.L, ref.Bt.T @ r.T) ** 2).sum(axis=0)


@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("demote,k", CASES)
def test_variances(case, demote, k, blocks):
    import torch
    c, tol = case, tol_of(demote)
    cond, ref = make_cond(c, demote, blocks, k)
    assert ref.kappa <= ref.kappa_bound
    for q in query_sets(ref, np.random.default_rng(5000 + k)):
        post, prior = cond.variance(q, prior=True)
        p_ref, v_ref = variance_reference(c, ref, demote, q)
        p64 = p_ref.astype(np.float64)
        bpost, bprior = 8 * tol * ref.kappa * p64, 4 * tol * p64
        ep, ev = err(prior, p_ref), err(post, v_ref)
        print(f"demote={demote} k={k} blocks={blocks} {len(q)} queries: prior max err/bound {np.max(ep / bprior):.3e}, post max err/bound {np.max(ev / bpost):.3e}; "
              f"post / prior in [{float((post / prior).min()):.4f}, {float((post / prior).max()):.4f}]")
        assert np.all(ep <= bprior) and np.all(ev <= bpost)
        po, pr = post.cpu().numpy(), prior.cpu().numpy()
        assert np.all(po <= pr + bpost) and np.all(po >= -bpost)
        assert torch.equal(cond.variance(q), post)                          # post only
        assert torch.equal(cond.variance(q, prior=True, post=False), prior) # prior only
    cond.close()


@pytest.mark.parametrize("demote,k", CASES)
def test_variance_agrees_with_the_sampler(case, demote, k):
    """Matheron's rule and the variance entry describe the same posterior: with y = 0, the 93 unit columns as W (E = 0) and the
    k columns E = -I (W = 0), sum_j Z_W[o, j]^2 + sum_a noiseVar[a] Z_E[o, a]^2 = dPost[o] within 8 tol kappa p_o, every row."""
    import torch
    c, tol = case, tol_of(demote)
    cond, ref = make_cond(c, demote, False, k)
    assert ref.kappa <= ref.kappa_bound
    dt = torch.float32 if demote else torch.float64
    y0 = torch.zeros(k, dtype=torch.float64, device=c["dev"])
    zw = cond.sample_block(y0, torch.eye(N, dtype=dt, device=c["dev"]).contiguous(), torch.zeros((k, N), dtype=torch.float64, device=c["dev"]))
    ze = cond.sample_block(y0, torch.zeros((N, k), dtype=dt, device=c["dev"]), (-torch.eye(k, dtype=torch.float64, device=c["dev"])).contiguous())
    total = (zw.cpu().numpy().astype(LD) ** 2).sum(axis=1) + (ze.cpu().numpy().astype(LD) ** 2) @ ref.noise.astype(LD)
    post = cond.variance(np.arange(M))
    p_ref, _ = variance_reference(c, ref, demote, np.arange(M))
    bound = 8 * tol * ref.kappa * p_ref.astype(np.float64)
    e = err(post, total)
    print(f"demote={demote} k={k}: sampler vs variance entry, max err/bound {np.max(e / bound):.3e} (max err {e.max():.3e})")
    assert np.all(e <= bound)
    cond.close()


def test_refusals_on_the_device(case):
    """The two checks that read the object, in the header's order after the argument-only ones, and a permutation that
    misses a query index."""
    import torch
    from butterfly_amd import _capi
    c, k = case, 5
    lib = _capi.load()
    cond, ref = make_cond(c, False, False, k)
    y = to_dev(c, ref.y)
    v = torch.empty(3, dtype=torch.float64, device=c["dev"])
    opt = _capi.BfhipCovCondLikOptions(16, 0, k * 64 * 8 - 1)
    assert lib.bfhipCovCondLogLikelihoodDevice(cond.handle, C.c_void_p(y.data_ptr()), C.c_void_p(v.data_ptr()), None, None, C.byref(opt), None) == 1
    assert b"strip" in lib.bfhipLastErrorMessage()
    with pytest.raises(_capi.BfhipError) as ei:
        cond.log_likelihood(y, workspace_bytes=8)
    assert ei.value.code == 1
    with pytest.raises(_capi.BfhipError) as ei:
        cond.variance([3, M, 9])
    assert ei.value.code == 5
    with pytest.raises(_capi.BfhipError) as ei:
        cond.variance([3, M, 3])                                       # a repeated index wins over the range
    assert ei.value.code == 1 and "repeated" in str(ei.value)
    cond.close()
    missing = c["row_perm"].copy()
    other = (c["rev"][4] + 1) % M
    missing[c["rev"][4]] = missing[other]                              # no row lands on index 4 any more
    obs = np.array([o for o in (100, 17, 60, 33) if o != missing[other]][:3])   # (the index now hit twice is not observed)
    bad = c["ops"][False, False].cov_condition(c["gam"][False], torch.from_numpy(missing.astype(np.int64)).to(c["dev"]), obs, np.full(3, 0.1))
    with pytest.raises(_capi.BfhipError) as ei:
        bad.variance([obs[0], 4])
    assert ei.value.code == 1 and "exactly once" in str(ei.value)
    assert bad.variance(obs[:2]).shape == (2,)                          # the object is as it was
    bad.close()


def test_the_likelihood_example_builds_and_runs(tmp_path):
    """examples/cov_likelihood_device.c, plain C against include/bfhip*.h, -Wall -Werror, in a child process."""
    lib = os.path.join(ROOT, "butterfly_amd", "csrc")
    exe = str(tmp_path / "cov_likelihood_device")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cov_likelihood_device.c"), "-L", lib, "-lbfhip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-lm", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0
    assert "logLik" in p.stdout and "homogeneity" in p.stdout
