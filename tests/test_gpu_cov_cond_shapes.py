"""The conditioning kernels (DESIGN.md sections 20 and 21) on the device at the shapes tests/test_gpu_cov_condition.py and
tests/test_gpu_cov_likelihood.py leave out, on the designed cases of tests/cond_cases.py (whose claims
tests/test_cov_cond_cases_cpu.py checks without a GPU).  The references, bounds and helpers are those two files' own.

A. More than one chunk of BF_COND_CHUNK = 1024 columns: the random graph 157 x 2085 (three chunks; F64 and F32, block switches
   off and on at minRhs 2), dense leaves 140 x 1024 (exactly one chunk) and 140 x 1025 (one chunk and one column); k in {33, 130},
   q in {1, 70}.  Each case first asserts, on the reference alone, that any chunk left out of G or of B^T W moves alpha by 1e3
   tolerances; then everything test_sample_block_against_the_long_double_reference asserts, the likelihood with both gradients
   under lik_bounds, and prior and posterior variances at 70 indices (two panels): |dPost - ref| <= 8 tol kappa p,
   |dPrior - ref| <= 4 tol p.
B. Designed spectra, F64, switches off: (k, n, kappa) = (161, 200, 1e10), (300, 333, 1e6), (513, 1100, 1e2), (513, 1100, 1e10).
   Backward error of alpha <= 1e-12 whatever kappa.  Forward error of alpha per column and of logLik, quad, logDet against the
   long-double result: at most max(8 x the error of the same operation in plain float64 on the host, 1e-12) -- 8 is what the
   Chebyshev tests grant a device whose order of summation differs from the host's.  (Measured on an MI355X: 0.6 - 2.0 for
   alpha, at most 3.3 for the values above the floor.  The host figure is one draw of a rounding error and moves with the
   host's BLAS; a ratio above 8 is to be explained, not widened.)  lambda_min (1 - 1e-6) <= minPivot <=
   maxPivot <= lambda_max (1 + 1e-6).  Gradients under lik_bounds for kappa <= 1e6; at 1e10, where that bound exceeds the
   values, finite and homogeneous.
C. Phi = L0 (integers), k = m = n in {97, 2048}, F64 and F32, no noise: alpha, the pivots, quad and the prior variances are the
   integers of the design bit for bit; |logDet - 2 k log 2| <= 4 k 2^-52 |logDet|; Z at the apply tolerances.
Every figure is printed before it is asserted."""
import numpy as np
import pytest

import cond_cases as cc
from test_gpu_cov_condition import LD, Oracle, col_errs, fwd_bound, input_of, tol_of
from test_gpu_cov_likelihood import err, lik_bounds

pytestmark = pytest.mark.gpu

A_CASES = [("graph", demote, blocks, k) for demote in (False, True) for blocks in (False, True) for k in cc.A_KS] + \
          [(name, False, False, k) for name in ("one", "one_row") for k in cc.A_KS]


def device():
    import torch
    return torch.device("cuda", 0)


def to_dev(x, demote=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(device()).to(torch.float32 if demote else torch.float64).contiguous()


def perm_to_dev(perm):
    import torch
    return torch.from_numpy(np.asarray(perm, dtype=np.int64)).to(device())


def make_operator(A, demote=False, blocks=False):
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    op = HipOperator.from_bfmat(A.ptr.value, flags=_capi.FLAG_ADJOINT, demote_to_f32=demote)
    if blocks:
        op.set_real_rhs_blocks(2)
        op.set_adjoint_rhs_blocks(2)
    return op


# ---------------------------------------------------------------------------
# A. more than one chunk of n
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunked():
    c = dict(operands=cc.chunk_operands(), ops={}, gam={}, perm={})
    for name, o in c["operands"].items():
        c["perm"][name] = perm_to_dev(o.row_perm)
        for demote in o.demotes:
            c["gam"][name, demote] = to_dev(input_of(o.gam, demote), demote)
            for blocks in o.blocks:
                c["ops"][name, demote, blocks] = make_operator(o.A, demote, blocks)
    yield c
    for op in c["ops"].values():
        op.close()


def make_cond(c, name, demote, blocks, k):
    ref, lik, query = c["operands"][name].case(demote, k)
    return c["ops"][name, demote, blocks].cov_condition(c["gam"][name, demote], c["perm"][name], ref.obs, ref.noise), ref, lik, query


@pytest.mark.parametrize("name,demote,blocks,k", A_CASES)
def test_sample_block_over_chunks(chunked, name, demote, blocks, k):
    import torch
    c, o, tol = chunked, chunked["operands"][name], tol_of(demote)
    for q in cc.A_QS:                                     # on the reference alone, before the device is touched
        cc.assert_every_chunk_matters(o, demote, k, q)
    cond, ref, _, _ = make_cond(c, name, demote, blocks, k)
    info = cond.info
    print(f"{name} demote={demote} blocks={blocks} k={k}: info {info}")
    assert info["numObs"] == k and info["setupApplies"] == (k + 63) // 64 and 0 < info["minPivot"] <= info["maxPivot"]
    y, ora = to_dev(ref.y), o.oracle(demote)
    for q in cc.A_QS:
        W, E = input_of(o.W[:, :q], demote), ref.E[:, :q]
        z, alpha = cond.sample_block(y, to_dev(W, demote), to_dev(E), return_alpha=True)
        z, alpha = z.cpu().numpy(), alpha.cpu().numpy()
        be = ref.backward_error(alpha, ref.residual(ref.y, W, E))
        Wp = np.asarray(W.astype(LD) + ref.Bt @ alpha.astype(LD), dtype=np.float64)
        e2 = col_errs(z, ora.sample(Wp))
        print(f"  q={q}: backward error of alpha {be:.3e}; Z vs the oracle sequence on W + B^T alpha_dev, max rel-l2 {e2.max():.3e} (tol {tol:.0e})")
        assert be <= tol
        assert e2.max() <= tol
        if not demote:
            a_ref, z_ref = ref.posterior(ref.y, W, E)
            ea, ez, bound = col_errs(alpha, a_ref), col_errs(z, z_ref), fwd_bound(o.n, k, ref.kappa)
            print(f"  q={q}: forward error, max rel-l2: alpha {ea.max():.3e} Z {ez.max():.3e} (bound {bound:.3e})")
            assert ea.max() <= bound and ez.max() <= bound
    # the mean is the block entry with W = 0, E = 0, one column: the same bits, alpha included
    mean, a1 = cond.mean(y, return_alpha=True)
    zeros = torch.zeros((o.n, 1), dtype=mean.dtype, device=device())
    z0, a0 = cond.sample_block(y, zeros, None, return_alpha=True)
    assert torch.equal(mean, z0[:, 0]) and torch.equal(a1, a0[:, 0])
    assert torch.equal(z0, cond.sample_block(y, zeros, torch.zeros((k, 1), dtype=torch.float64, device=device())))
    cond.close()


@pytest.mark.parametrize("name,demote,blocks,k", A_CASES)
def test_likelihood_and_variances_over_chunks(chunked, name, demote, blocks, k):
    c, o, tol = chunked, chunked["operands"][name], tol_of(demote)
    cond, ref, lik, query = make_cond(c, name, demote, blocks, k)
    assert ref.kappa <= ref.kappa_bound
    bv, bg, bh = lik_bounds(ref, lik, tol)
    v, g, h = cond.log_likelihood(to_dev(ref.y), grad_log_gamma=True, grad_noise=True)
    ev, eg, eh = err(v, np.array([lik.loglik, lik.quad, lik.logdet], dtype=LD)), err(g, lik.g), err(h, lik.h)
    nz = bg > 0                                            # (a column of zeros has a zero bound and an exact zero gradient)
    print(f"{name} demote={demote} blocks={blocks} k={k}: cond(K) = {ref.kappa:.3e}; |value err| / bound = {np.array2string(ev / bv, precision=3)}; "
          f"gradLogGamma max err/bound {np.max(eg[nz] / bg[nz]):.3e} (max err {eg.max():.3e}); gradNoise max err/bound {eh.max() / bh:.3e} (max err {eh.max():.3e})")
    assert np.all(ev <= bv)
    assert np.all(eg <= bg)
    assert np.all(eh <= bh)
    assert len(query) == cc.NQUERY
    post, prior = cond.variance(query, prior=True, post=True)
    p_ref, v_ref = cc.variance_reference(o.rows(demote), ref, query)
    p64 = p_ref.astype(np.float64)
    bpost, bprior = 8 * tol * ref.kappa * p64, 4 * tol * p64
    ep, epost = err(prior, p_ref), err(post, v_ref)
    print(f"  {len(query)} queries: prior max err/bound {np.max(ep / bprior):.3e}, post max err/bound {np.max(epost / bpost):.3e}")
    assert np.all(ep <= bprior) and np.all(epost <= bpost)
    cond.close()


# ---------------------------------------------------------------------------
# B. designed spectra
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spectra():
    """Each long-double reference is formed once, here."""
    return {key: cc.SpectrumCase(*key) for key in cc.SPECTRUM_CASES}


def within(dev_err, host_err):
    return dev_err <= np.maximum(8 * host_err, 1e-12)


@pytest.mark.parametrize("k,n,kappa", cc.SPECTRUM_CASES)
def test_designed_spectrum(spectra, k, n, kappa):
    import torch
    from oracle import bfref
    case = spectra[k, n, kappa]
    ref, lik = case.ref, case.ref.lik
    print(f"k={k} n={n}: cond(K) designed {kappa:.1e}, of the reference {ref.kappa:.6e}; lambda in [{ref.lam_min:.6e}, {ref.lam_max:.6e}]")
    assert abs(ref.kappa / kappa - 1) <= 1e-3
    desc, vals = cc.dense_leaf(case.phi)
    A = bfref.from_desc(desc, vals)
    op = make_operator(A)
    cond = op.cov_condition(torch.ones(n, dtype=torch.float64, device=device()), perm_to_dev(case.row_perm), case.obs, ref.noise)
    info = cond.info
    print(f"  info {info}")
    assert info["numObs"] == k and info["setupApplies"] == (k + 63) // 64
    assert ref.lam_min * (1 - 1e-6) <= info["minPivot"] <= info["maxPivot"] <= ref.lam_max * (1 + 1e-6)
    y = to_dev(case.y)
    # alpha: backward error, and forward error per column against the float64 host pipeline's own
    _, alpha = cond.sample_block(y, to_dev(case.W), to_dev(case.E), return_alpha=True)
    alpha = alpha.cpu().numpy()
    be = ref.backward_error(alpha, ref.residual(case.y, case.W, case.E))
    ed, eh = col_errs(alpha, case.alpha), col_errs(case.alpha64, case.alpha)
    print(f"  backward error of alpha {be:.3e}; forward error per column: device {np.array2string(ed, precision=3)}, float64 host "
          f"{np.array2string(eh, precision=3)}, ratio {np.array2string(ed / eh, precision=3)}")
    assert be <= 1e-12
    assert np.all(within(ed, eh))
    # the value
    v, g, h = cond.log_likelihood(y, grad_log_gamma=True, grad_noise=True)
    scale = np.abs(case.values).astype(np.float64)
    vd, vh = err(v, case.values) / scale, np.abs((case.values64.astype(LD) - case.values).astype(np.float64)) / scale
    print(f"  relative error of (logLik, quad, logDet): device {np.array2string(vd, precision=3)}, float64 host {np.array2string(vh, precision=3)}, "
          f"ratio {np.array2string(vd / np.maximum(vh, 1e-300), precision=3)}")
    assert np.all(within(vd, vh))
    # the gradients
    gv, hv = g.cpu().numpy(), h.cpu().numpy()
    assert np.all(np.isfinite(gv)) and np.all(np.isfinite(hv))
    vv = v.cpu().numpy().astype(LD)
    hom = float(abs(gv.astype(LD).sum() / 2 + hv.astype(LD) @ ref.noise.astype(LD) - (vv[1] - k) / 2))
    hb = 8 * 1e-12 * ref.kappa * (float(lik.quad) + k)
    print(f"  homogeneity residual {hom:.3e} (bound {hb:.3e}; (quad - k) / 2 = {float((vv[1] - k) / 2):.6e})")
    assert hom <= hb
    if kappa <= 1e6:
        _, bg, bh = lik_bounds(ref, lik, 1e-12)
        eg, eh = err(g, lik.g), err(h, lik.h)
        print(f"  gradLogGamma max err/bound {np.max(eg / bg):.3e} (max err {eg.max():.3e}); gradNoise max err/bound {eh.max() / bh:.3e} (max err {eh.max():.3e})")
        assert np.all(eg <= bg)
        assert np.all(eh <= bh)
    cond.close()
    op.close()


# ---------------------------------------------------------------------------
# C. exact integers, up to the maximum k
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("demote", [False, True])
@pytest.mark.parametrize("k", cc.INTEGER_KS)
def test_integer_case_bit_for_bit(k, demote):
    import torch
    from oracle import bfref
    case, tol = cc.IntegerCase(k), tol_of(demote)
    desc, vals = case.operand()
    A = bfref.from_desc(desc, vals)
    op = make_operator(A, demote)
    dt = torch.float32 if demote else torch.float64
    cond = op.cov_condition(torch.ones(k, dtype=dt, device=device()), perm_to_dev(case.row_perm), case.obs, None)
    info = cond.info
    print(f"k={k} demote={demote}: info {info}")
    assert info["numObs"] == k and info["setupApplies"] == (k + 63) // 64
    assert info["minPivot"] == 4.0 and info["maxPivot"] == 4.0
    y, ora, Bt = to_dev(case.y), Oracle(A, np.ones(k), case.row_perm), case.L0.T.astype(np.float64)
    # the mean: alpha is x0
    mean, alpha = cond.mean(y, return_alpha=True)
    alpha = alpha.cpu().numpy()
    print(f"  mean: entries of alpha that differ from x0: {int(np.count_nonzero(alpha != case.x0))}")
    assert np.array_equal(alpha, case.x0.astype(np.float64))
    e = col_errs(mean.cpu().numpy()[:, None], ora.sample((Bt @ alpha)[:, None]))
    # the block, two passes: alpha is X
    z, alpha = cond.sample_block(y, to_dev(case.W, demote), to_dev(case.E), return_alpha=True)
    alpha = alpha.cpu().numpy()
    print(f"  block: entries of alpha that differ from X: {int(np.count_nonzero(alpha != case.X))}")
    assert np.array_equal(alpha, case.X.astype(np.float64))
    e2 = col_errs(z.cpu().numpy(), ora.sample(case.W + Bt @ alpha))
    print(f"  Z vs the oracle sequence, max rel-l2: mean {e.max():.3e}, block {e2.max():.3e} (tol {tol:.0e})")
    assert e.max() <= tol and e2.max() <= tol
    # the value: quad is an integer, logDet = 2 k log 2
    v = cond.log_likelihood(y).cpu().numpy()
    want = 2 * k * np.log(2.0)
    print(f"  quad {v[1]!r} (design {case.quad}); logDet {v[2]!r}, off 2 k log 2 by {abs(v[2] - want) / want:.3e} relative (bound {4 * k * 2.0 ** -52:.3e})")
    assert v[1] == float(case.quad)
    assert abs(v[2] - want) <= 4 * k * 2.0 ** -52 * abs(v[2])
    # the prior variances at 70 indices: diag(G) through the permutation
    prior = cond.variance(case.query, prior=True, post=False).cpu().numpy()
    assert np.array_equal(prior, case.prior.astype(np.float64))
    cond.close()
    op.close()
