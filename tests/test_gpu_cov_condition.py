"""Conditioning covariance samples on observations by a direct solve, on the device, against a
long-double dense reference: Phi is obtained from the oracle (bfref) column by column, and B, G, R, alpha, W' and Z are
formed from it in numpy's long double with the Cholesky factorization written below.

The operand is the one of the batched covariance tests (tests/test_gpu_cov_batch.py), restated: 211 x 93, gamma in
[0.1, 1.1), a random row permutation; one operator per element type (F64, F32 by demote_to_f32) and per switch state
(block switches off, and on at minRhs = 2).  k in {1, 5, 64, 65, 130} observations (64 | 65: the setup panel width; 130:
three panels and more observations than columns, so G alone is singular), q in {1, 3, 64, 70} columns (70: two passes).
noiseVar[a] = rho trace(G) / k (0.5 + u_a), rho = 0.01: lambda_max(G) <= trace(G) and lambda_min(G + D) >= min D give
cond(G + D) <= 1 + 3 k / rho, which every case asserts on its reference matrix.

Bounds.  (1) the backward error of the device's alpha, ||(G + D) alpha - R||_F / (||G + D||_F ||alpha||_F + ||R||_F), and
(2) Z against the oracle's step-by-step sequence on W + B^T alpha_dev, per column: 1e-12 (F64), 2e-5 (F32), the project's apply
tolerances (a backward error carries no condition number).  (3) F64 forward error of alpha and Z against the long-double
results, per column: 1e-12 + 16 (n + k) 2^-53 cond_ref.  The two switch states are also compared with each other, per
column, at the tolerances of (2)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N = 211, 93
KS = (1, 5, 64, 65, 130)
QS = (1, 3, 64, 70)
MAXQ = max(QS)
RHO = 0.01
LD = np.longdouble


def tol_of(demote):
    return 2e-5 if demote else 1e-12


def fwd_bound(n, k, kappa):
    return 1e-12 + 16 * (n + k) * 2.0 ** -53 * kappa


def col_errs(got, want):
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    return (np.linalg.norm(got - want, axis=0) / np.linalg.norm(want, axis=0)).astype(np.float64)


def fro(x):
    return float(np.sqrt((np.asarray(x, dtype=LD) ** 2).sum()))


def permute_rows(x, perm):        # bfVecRealPermute on every column: out[perm[i], :] = in[i, :]
    out = np.empty_like(x); out[perm] = x
    return out


def cholesky_ld(a):
    """Lower Cholesky factor in long double, column by column."""
    a = np.array(a, dtype=LD)
    k = a.shape[0]
    l = np.zeros_like(a)
    for c in range(k):
        d = a[c, c] - (l[c, :c] ** 2).sum()
        assert d > 0
        l[c, c] = np.sqrt(d)
        if c + 1 < k:
            l[c + 1:, c] = (a[c + 1:, c] - l[c + 1:, :c] @ l[c, :c]) / l[c, c]
    return l


def solve_ld(l, r):
    """(L L^T)^-1 R in long double: forward, then backward substitution."""
    k = l.shape[0]
    x = np.array(r, dtype=LD)
    for c in range(k):
        x[c] = (x[c] - l[c, :c] @ x[:c]) / l[c, c]
    for c in range(k - 1, -1, -1):
        x[c] = (x[c] - l[c + 1:, c] @ x[c + 1:]) / l[c, c]
    return x


class Oracle:
    """The reference sequence of the prior sample, column by column (bfref.mat_mul_vec + numpy scatter)."""
    def __init__(self, A, gam, row_perm):
        self.A, self.gam, self.row_perm = A, gam, row_perm

    def apply(self, X):
        from oracle import bfref
        return np.stack([bfref.mat_mul_vec(self.A, np.ascontiguousarray(X[:, q])) for q in range(X.shape[1])], axis=1)

    def rapply(self, X):
        from oracle import bfref
        return np.stack([bfref.mat_rmul_vec(self.A, np.ascontiguousarray(X[:, q])) for q in range(X.shape[1])], axis=1)

    def sample(self, W):
        return permute_rows(self.apply(self.gam[:, None] * W), self.row_perm)


class Reference:
    """Everything of one (operand, gamma, perm, obs, rho) in long double.  rows_t [n x k] = Phi[i_a, :]^T from the oracle."""
    def __init__(self, rows_t, gam, obs, rho, rng, phi=None, row_perm=None):
        k = len(obs)
        self.k, self.obs = k, obs
        self.Bt = rows_t.astype(LD) * gam.astype(LD)[:, None]                 # [n x k]
        self.G = self.Bt.T @ self.Bt
        self.noise = (rho * float(np.trace(self.G)) / k * (0.5 + rng.random(k))).astype(np.float64)
        self.A = self.G + np.diag(self.noise.astype(LD))
        ev = np.linalg.eigvalsh(self.A.astype(np.float64))
        self.kappa = float(ev[-1] / ev[0])
        self.kappa_bound = 1 + 3 * k / rho
        self.L = cholesky_ld(self.A) if phi is not None else None
        self.phi, self.gam, self.row_perm = phi, gam, row_perm

    def residual(self, y, W, E):
        return y.astype(LD)[:, None] - self.Bt.T @ W.astype(LD) - E.astype(LD)

    def posterior(self, y, W, E):
        """(alpha, Z) in long double."""
        alpha = solve_ld(self.L, self.residual(y, W, E))
        Wp = W.astype(LD) + self.Bt @ alpha
        return alpha, permute_rows(self.phi.astype(LD) @ (self.gam.astype(LD)[:, None] * Wp), self.row_perm)

    def backward_error(self, alpha_dev, R):
        a = np.asarray(alpha_dev, dtype=LD)
        return fro(self.A @ a - R) / (fro(self.A) * fro(a) + fro(R))


def input_of(x, demote):
    """What the device is given: the values rounded to the operator's element type, widened again."""
    return x.astype(np.float32).astype(np.float64) if demote else x


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
    row_perm = rng.permutation(M)
    rev = np.empty(M, dtype=np.int64); rev[row_perm] = np.arange(M)
    dev = torch.device("cuda", 0)
    c = dict(dev=dev, rev=rev, row_perm=row_perm, perm=torch.from_numpy(row_perm.astype(np.int64)).to(dev), ops={}, gam={}, ora={}, ref={},
             W=rng.standard_normal((N, MAXQ)), rng=rng)
    phi = Oracle(A, gam, row_perm).apply(np.eye(N))                        # dense Phi, from the oracle
    for demote in (False, True):
        g = input_of(gam, demote)
        c["ora"][demote] = Oracle(A, g, row_perm)
        c["gam"][demote] = torch.from_numpy(g).to(dev).to(torch.float32 if demote else torch.float64)
        for blocks in (False, True):
            op = HipOperator.from_bfmat(A.ptr.value, flags=_capi.FLAG_ADJOINT, demote_to_f32=demote)
            if blocks:
                op.set_real_rhs_blocks(2)
                op.set_adjoint_rhs_blocks(2)
            c["ops"][demote, blocks] = op
        for k in KS:
            krng = np.random.default_rng(1000 + k)
            obs = krng.choice(M, size=k, replace=False)
            ref = Reference(phi[rev[obs], :].T, g, obs, RHO, krng, phi=phi, row_perm=row_perm)
            ref.y = np.asarray(ref.Bt.T @ krng.standard_normal(N) + np.sqrt(ref.noise) * krng.standard_normal(k), dtype=np.float64)
            ref.E = np.sqrt(ref.noise)[:, None] * krng.standard_normal((k, MAXQ))
            c["ref"][demote, k] = ref
    yield c
    for op in c["ops"].values():
        op.close()


def to_dev(c, x, demote=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(c["dev"]).to(torch.float32 if demote else torch.float64).contiguous()


def make_cond(c, demote, blocks, k):
    ref = c["ref"][demote, k]
    return c["ops"][demote, blocks].cov_condition(c["gam"][demote], c["perm"], ref.obs, ref.noise), ref


@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("demote", [False, True])
def test_sample_block_against_the_long_double_reference(case, demote, k, blocks):
    """Items 1 - 3 for every q, and the mean (item 4).  Both switch states run the same assertions (item 8)."""
    import torch
    c, tol = case, tol_of(demote)
    cond, ref = make_cond(c, demote, blocks, k)
    print(f"demote={demote} k={k} blocks={blocks}: cond(G + D) = {ref.kappa:.3e} (bound {ref.kappa_bound:.3e}); info {cond.info}")
    assert ref.kappa <= ref.kappa_bound
    info = cond.info
    assert info["numObs"] == k and info["setupApplies"] == (k + 63) // 64 and 0 < info["minPivot"] <= info["maxPivot"]
    y = to_dev(c, ref.y)
    for q in QS:
        W, E = input_of(c["W"][:, :q], demote), ref.E[:, :q]
        z, alpha = cond.sample_block(y, to_dev(c, W, demote), to_dev(c, E), return_alpha=True)
        z, alpha = z.cpu().numpy(), alpha.cpu().numpy()
        be = ref.backward_error(alpha, ref.residual(ref.y, W, E))
        Wp = np.asarray(W.astype(LD) + ref.Bt @ alpha.astype(LD), dtype=np.float64)
        e2 = col_errs(z, c["ora"][demote].sample(Wp))
        print(f"  q={q}: backward error of alpha {be:.3e}; Z vs the oracle sequence on W + B^T alpha_dev, max rel-l2 {e2.max():.3e} (tol {tol:.0e})")
        assert be <= tol
        assert e2.max() <= tol
        if not demote:
            a_ref, z_ref = ref.posterior(ref.y, W, E)
            ea, ez, bound = col_errs(alpha, a_ref), col_errs(z, z_ref), fwd_bound(N, k, ref.kappa)
            print(f"  q={q}: forward error, max rel-l2: alpha {ea.max():.3e} Z {ez.max():.3e} (bound {bound:.3e})")
            assert ea.max() <= bound and ez.max() <= bound
    # the mean is the block entry with W = 0, E = 0, one column: the same bits, alpha included
    mean, a1 = cond.mean(y, return_alpha=True)
    z0, a0 = cond.sample_block(y, torch.zeros((N, 1), dtype=mean.dtype, device=c["dev"]), None, return_alpha=True)
    assert torch.equal(mean, z0[:, 0]) and torch.equal(a1, a0[:, 0])
    assert torch.equal(z0, cond.sample_block(y, torch.zeros((N, 1), dtype=mean.dtype, device=c["dev"]), torch.zeros((k, 1), dtype=torch.float64, device=c["dev"])))
    cond.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("demote", [False, True])
def test_switch_states_agree(case, demote, k):
    """Item 8, directly: the two switch states against each other, per column, at the tolerances of item 2."""
    c, tol = case, tol_of(demote)
    off, ref = make_cond(c, demote, False, k)
    on, _ = make_cond(c, demote, True, k)
    y, W, E = to_dev(c, ref.y), to_dev(c, c["W"], demote), to_dev(c, ref.E)
    e = col_errs(on.sample_block(y, W, E).cpu().numpy(), off.sample_block(y, W, E).cpu().numpy())
    print(f"demote={demote} k={k}: switches on vs off, max rel-l2 {e.max():.3e} (tol {tol:.0e})")
    assert e.max() <= tol
    on.close(); off.close()


def device_blocks(c, op, cond_k, sd, seed, noise_seed, first, q, demote):
    """The blocks a draw is defined by: W[j, s] = N(seed, (first + s) n + j) in the operator's type, E[a, s] =
    sd[a] N(noise_seed, (first + s) k + a) in double -- sample-major streams, transposed into the block layout."""
    import torch
    dt = torch.float32 if demote else torch.float64
    W = op.fill_normal(torch.empty((q, N), dtype=dt, device=c["dev"]), seed, first * N).t().contiguous()
    E = op.fill_normal(torch.empty((q, cond_k), dtype=torch.float64, device=c["dev"]), noise_seed, first * cond_k).t().contiguous()
    return W, (sd[:, None] * E).contiguous()


@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("demote", [False, True])
def test_draw_is_the_sample_block_of_the_device_normals(case, demote, blocks):
    """Item 5 (k = 65), and item 6: a second object made the same way gives the same bits."""
    import torch
    c, k = case, 65
    op = c["ops"][demote, blocks]
    cond, ref = make_cond(c, demote, blocks, k)
    y, sd = to_dev(c, ref.y), to_dev(c, np.sqrt(ref.noise))
    seed, nseed, first = 99, 1234, 5
    for q in QS:
        W, E = device_blocks(c, op, k, sd, seed, nseed, first, q, demote)
        assert torch.equal(cond.draw(y, seed, nseed, first, q), cond.sample_block(y, W, E)), q
    whole = cond.draw(y, seed, nseed, 0, 70)
    parts = torch.cat([cond.draw(y, seed, nseed, 0, 3), cond.draw(y, seed, nseed, 3, 67)], dim=1)
    diff = col_errs(parts.cpu().numpy(), whole.cpu().numpy())
    print(f"demote={demote} blocks={blocks}: draws (0, 3) ++ (3, 67) vs (0, 70): max rel-l2 {diff.max():.3e}, columns that differ: {np.flatnonzero(diff).tolist()}")
    assert torch.equal(parts, whole)
    # repeatability: the same create and the same call, the same bits
    W, E = device_blocks(c, op, k, sd, seed, nseed, first, 70, demote)
    z1, a1 = cond.sample_block(y, W, E, return_alpha=True)
    again, _ = make_cond(c, demote, blocks, k)
    z2, a2 = again.sample_block(y, W, E, return_alpha=True)
    assert torch.equal(z1, z2) and torch.equal(a1, a2)
    again.close(); cond.close()


def check_moments(Z, got_sum, got_sq, K, base_sum=0.0, base_sq=0.0):
    """|sum - sum_s z_s| <= K 2^-52 sum_s |z_s| per row, likewise for the squares (Z widened to double exactly)."""
    Z = Z.astype(np.float64)
    bound = K * 2.0 ** -52
    if got_sum is not None:
        err, scale = np.abs(got_sum - (base_sum + Z.sum(axis=1))), np.abs(base_sum) + np.abs(Z).sum(axis=1)
        print(f"moments: max |sum err| / sum|z| = {np.max(err / scale):.3e} (bound {bound:.3e})")
        assert np.all(err <= bound * scale)
    if got_sq is not None:
        err, scale = np.abs(got_sq - (base_sq + (Z * Z).sum(axis=1))), np.abs(base_sq) + (Z * Z).sum(axis=1)
        print(f"moments: max |sumsq err| / sum z^2 = {np.max(err / scale):.3e} (bound {bound:.3e})")
        assert np.all(err <= bound * scale)


@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("demote", [False, True])
def test_streaming_moments_of_conditioned_draws(case, demote, blocks):
    """Item 7: 150 samples as 64 + 64 + 22 against the stored draws; += into sums that are not zero; a NULL output."""
    import torch
    c, k, K = case, 64, 150
    cond, ref = make_cond(c, demote, blocks, k)
    y = to_dev(c, ref.y)
    seed, nseed = 4242, 77
    Z = torch.cat([cond.draw(y, seed, nseed, f, b) for f, b in ((0, 64), (64, 64), (128, 22))], dim=1).cpu().numpy()
    s, q = torch.zeros(M, dtype=torch.float64, device=c["dev"]), torch.zeros(M, dtype=torch.float64, device=c["dev"])
    cond.moments(y, seed, nseed, 0, K, 64, s, q)
    check_moments(Z, s.cpu().numpy(), q.cpu().numpy(), K)
    s2, q2 = torch.zeros_like(s), torch.zeros_like(q)
    cond.moments(y, seed, nseed, 0, K, 0, s2, q2)                      # batch 0 means 64; two runs, the same bits
    assert torch.equal(s, s2) and torch.equal(q, q2)
    s3, q3 = torch.zeros_like(s), torch.zeros_like(q)
    cond.moments(y, seed, nseed, 0, K, 64, s3, None)
    cond.moments(y, seed, nseed, 0, K, 64, None, q3)
    assert torch.equal(s3, s) and torch.equal(q3, q)
    base_s, base_q = c["rng"].standard_normal(M), c["rng"].random(M)  # += into what is there
    s4, q4 = to_dev(c, base_s), to_dev(c, base_q)
    cond.moments(y, seed, nseed, 0, K, 64, s4, q4)
    check_moments(Z, s4.cpu().numpy(), q4.cpu().numpy(), K + 1, base_s, base_q)
    # the posterior mean of the draws is near the kriging mean: a sanity figure, printed only
    mean = cond.mean(y).cpu().numpy().astype(np.float64)
    print(f"demote={demote} blocks={blocks}: |mean of {K} draws - posterior mean| / |posterior mean| = {np.linalg.norm(s.cpu().numpy() / K - mean) / np.linalg.norm(mean):.3e}")
    cond.close()


def test_refusals_on_the_device(case):
    """Item 9: an exact zero first pivot (gamma = 0, no noise) is a RUNTIME_ERROR naming step 0 and leaves *out NULL; a
    permutation that maps two rows to one observed index is INVALID_ARGUMENTS."""
    import torch
    from butterfly_amd import _capi
    c = case
    lib = _capi.load()
    op = c["ops"][False, False]
    obs = np.array([4, 100, 17], dtype=np.uint64)
    zero = torch.zeros(N, dtype=torch.float64, device=c["dev"])
    out = C.c_void_p(0x1234)
    rc = lib.bfhipCovCondCreate(op.handle, C.c_void_p(zero.data_ptr()), C.c_void_p(c["perm"].data_ptr()), obs.ctypes.data, 3, None, C.byref(out), None)
    msg = lib.bfhipLastErrorMessage()
    print(rc, msg)
    assert rc == 2 and b"step 0" in msg and not out.value
    with pytest.raises(_capi.BfhipError) as ei:
        op.cov_condition(zero, c["perm"], obs, None)
    assert ei.value.code == 2
    twice = c["row_perm"].copy()
    other = (c["rev"][4] + 1) % M
    twice[other] = 4                                  # rows rev[4] and rev[4] + 1 both land on observed index 4
    with pytest.raises(_capi.BfhipError) as ei:
        op.cov_condition(c["gam"][False], torch.from_numpy(twice.astype(np.int64)).to(c["dev"]), obs, np.full(3, 0.1))
    assert ei.value.code == 1 and "exactly once" in str(ei.value)
    missing = c["row_perm"].copy()
    missing[c["rev"][4]] = missing[other]             # no row lands on observed index 4 any more
    with pytest.raises(_capi.BfhipError) as ei:
        op.cov_condition(c["gam"][False], torch.from_numpy(missing.astype(np.int64)).to(c["dev"]), obs, np.full(3, 0.1))
    assert ei.value.code == 1
    # the operator is as it was: a good object still comes out
    op.cov_condition(c["gam"][False], c["perm"], obs, np.full(3, 0.1)).close()


def test_a_larger_shape_once():
    """Item 10: 4099 x 515 in F32, k = 300, q = 64, rho = 1 -- rows over many workgroups, ten Cholesky blocks, five setup
    panels, the last of them partial; items 1 and 2."""
    import torch
    import randgraph
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from oracle import bfref
    m, n, k, q, rho = 4099, 515, 300, 64, 1.0
    rng = np.random.default_rng(78)
    desc, vals = randgraph.random_operand(rng, depth=4, size_hint=120, cplx=False, m=m, n=n)
    A = bfref.from_desc(desc, vals)
    gam = input_of(rng.random(n) + 0.1, True)
    row_perm = rng.permutation(m)
    rev = np.empty(m, dtype=np.int64); rev[row_perm] = np.arange(m)
    ora = Oracle(A, gam, row_perm)
    obs = rng.choice(m, size=k, replace=False)
    units = np.zeros((m, k)); units[rev[obs], np.arange(k)] = 1.0
    ref = Reference(ora.rapply(units), gam, obs, rho, rng)
    print(f"larger shape: cond(G + D) = {ref.kappa:.3e} (bound {ref.kappa_bound:.3e})")
    assert ref.kappa <= ref.kappa_bound
    y = np.asarray(ref.Bt.T @ rng.standard_normal(n) + np.sqrt(ref.noise) * rng.standard_normal(k), dtype=np.float64)
    W, E = input_of(rng.standard_normal((n, q)), True), np.sqrt(ref.noise)[:, None] * rng.standard_normal((k, q))
    dev = torch.device("cuda", 0)
    op = HipOperator.from_bfmat(A.ptr.value, flags=_capi.FLAG_ADJOINT, demote_to_f32=True)
    op.set_real_rhs_blocks(2)
    op.set_adjoint_rhs_blocks(2)
    g = torch.from_numpy(gam).to(dev).to(torch.float32)
    p = torch.from_numpy(row_perm.astype(np.int64)).to(dev)
    cond = op.cov_condition(g, p, obs, ref.noise)
    print(cond.info)
    z, alpha = cond.sample_block(torch.from_numpy(y).to(dev), torch.from_numpy(W).to(dev).to(torch.float32).contiguous(), torch.from_numpy(E).to(dev).contiguous(),
                                 return_alpha=True)
    z, alpha = z.cpu().numpy(), alpha.cpu().numpy()
    be = ref.backward_error(alpha, ref.residual(y, W, E))
    e2 = col_errs(z, ora.sample(np.asarray(W.astype(LD) + ref.Bt @ alpha.astype(LD), dtype=np.float64)))
    print(f"larger shape: backward error of alpha {be:.3e}; Z vs the oracle sequence, max rel-l2 {e2.max():.3e}")
    assert be <= 2e-5 and e2.max() <= 2e-5
    cond.close()
    op.close()


def test_the_conditioning_example_builds_and_runs(tmp_path):
    """Item 11: examples/cov_condition_device.c, plain C against include/bfhip*.h, -Wall -Werror, in a child process."""
    lib = os.path.join(ROOT, "butterfly_amd", "csrc")
    exe = str(tmp_path / "cov_condition_device")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cov_condition_device.c"), "-L", lib, "-lbfhip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-lm", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0
    assert "rms misfit" in p.stdout
