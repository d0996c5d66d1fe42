"""Batched covariance sampling on the device: the block forms of the two covariance products, the
device normals, the draw that needs no input vector and the streaming moments, against the oracle's step-by-step sequence
(bfref.mat_mul_vec / mat_rmul_vec + numpy scatter: the reference of test_fused_covariance_products_match_the_oracle_sequence)
on that test's operand.

Tolerances are the project's own: rel-l2 per column <= 1e-12 (F64), <= 2e-5 (F32 operators: fp32 storage and arithmetic).
The moments' bound holds for any summation order: accumulation is in double from exactly widened values."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N = 211, 93
NRHS = (1, 2, 3, 17, 64, 70)      # 3, 17: the scalar path; 64: 16-byte rows; 70: two passes of the block kernels
MAXQ = max(NRHS)
ULP_BOUND = 8                     # device log / cos against libm's


def tol_of(demote):
    return 2e-5 if demote else 1e-12


def col_errs(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.linalg.norm(got - want, axis=0) / np.linalg.norm(want, axis=0)


def permute_rows(x, perm):        # bfVecRealPermute on every column: out[perm[i], :] = in[i, :]
    out = np.empty_like(x); out[perm] = x
    return out


class Oracle:
    """The reference sequence, column by column, computed once per operand."""
    def __init__(self, A, gam, row_perm, rev):
        self.A, self.gam, self.row_perm, self.rev = A, gam, row_perm, rev

    def apply(self, X):
        from oracle import bfref
        return np.stack([bfref.mat_mul_vec(self.A, np.ascontiguousarray(X[:, q])) for q in range(X.shape[1])], axis=1)

    def rapply(self, X):
        from oracle import bfref
        return np.stack([bfref.mat_rmul_vec(self.A, np.ascontiguousarray(X[:, q])) for q in range(X.shape[1])], axis=1)

    def sample(self, W, identity=False):
        if identity:
            return self.apply(W)
        return permute_rows(self.apply(self.gam[:, None] * W), self.row_perm)

    def matvec(self, V, identity=False):
        if identity:
            return self.apply(self.rapply(V))
        t = self.rapply(permute_rows(V, self.rev))
        return permute_rows(self.apply(self.gam[:, None] * (self.gam[:, None] * t)), self.row_perm)


@pytest.fixture(scope="module")
def case():
    """Operand, inputs and oracle results of the widest block (narrower blocks are its leading columns), and one
    operator per (element type, switches)."""
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
    ora = Oracle(A, gam, row_perm, rev)
    W, V = rng.standard_normal((N, MAXQ)), rng.standard_normal((M, MAXQ))
    dev = torch.device("cuda", 0)
    c = dict(ora=ora, W=W, V=V, dev=dev,
             z_sample=ora.sample(W), z_cov=ora.matvec(V), z_sample_id=ora.sample(W, True), z_cov_id=ora.matvec(V, True),
             perm=torch.from_numpy(row_perm.astype(np.int64)).to(dev), rev=torch.from_numpy(rev).to(dev), ops={}, gam={})
    for demote in (False, True):
        dt = torch.float32 if demote else torch.float64
        c["gam"][demote] = torch.from_numpy(gam).to(dev).to(dt)
        for blocks in (False, True):
            op = HipOperator.from_bfmat(A.ptr.value, flags=_capi.FLAG_ADJOINT, demote_to_f32=demote)
            if blocks:
                op.set_real_rhs_blocks(2)
                op.set_adjoint_rhs_blocks(2)
            c["ops"][demote, blocks] = op
    yield c
    for op in c["ops"].values():
        op.close()


def to_dev(c, x, demote):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(c["dev"]).to(torch.float32 if demote else torch.float64).contiguous()


@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("demote", [False, True])
def test_block_products_match_the_oracle_sequence_column_for_column(case, demote, nrhs, blocks):
    c, op, tol = case, case["ops"][demote, blocks], tol_of(demote)
    W, V = to_dev(c, c["W"][:, :nrhs], demote), to_dev(c, c["V"][:, :nrhs], demote)
    g, p, r = c["gam"][demote], c["perm"], c["rev"]
    e = col_errs(op.cov_sample_block_device(g, p, W).cpu().numpy(), c["z_sample"][:, :nrhs])
    print(f"sample demote={demote} nrhs={nrhs} blocks={blocks}: max rel-l2 {e.max():.3e}")
    assert e.max() <= tol
    e = col_errs(op.cov_matvec_block_device(g, p, r, V).cpu().numpy(), c["z_cov"][:, :nrhs])
    print(f"matvec demote={demote} nrhs={nrhs} blocks={blocks}: max rel-l2 {e.max():.3e}")
    assert e.max() <= tol
    if nrhs == 17:      # identity diagonal and permutations: plain A W and A A^T V
        e = col_errs(op.cov_sample_block_device(None, None, W).cpu().numpy(), c["z_sample_id"][:, :nrhs])
        assert e.max() <= tol
        e = col_errs(op.cov_matvec_block_device(None, None, None, V).cpu().numpy(), c["z_cov_id"][:, :nrhs])
        assert e.max() <= tol


@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("demote", [False, True])
def test_a_column_of_the_block_result_is_the_single_vector_result(case, demote, nrhs):
    """Switches off.  At one column the block entries run the single-vector entries' arithmetic: bit for bit."""
    import torch
    c, op, tol = case, case["ops"][demote, False], tol_of(demote)
    W, V = to_dev(c, c["W"][:, :nrhs], demote), to_dev(c, c["V"][:, :nrhs], demote)
    g, p, r = c["gam"][demote], c["perm"], c["rev"]
    zs, zc = op.cov_sample_block_device(g, p, W), op.cov_matvec_block_device(g, p, r, V)
    one_s = torch.stack([op.cov_sample_device(g, p, W[:, q].contiguous()) for q in range(nrhs)], dim=1)
    one_c = torch.stack([op.cov_matvec_device(g, p, r, V[:, q].contiguous()) for q in range(nrhs)], dim=1)
    if nrhs == 1:
        assert torch.equal(zs, one_s) and torch.equal(zc, one_c)
    es, ec = col_errs(zs.cpu().numpy(), one_s.cpu().numpy()), col_errs(zc.cpu().numpy(), one_c.cpu().numpy())
    print(f"demote={demote} nrhs={nrhs}: block vs single-vector, max rel-l2 sample {es.max():.3e} matvec {ec.max():.3e}")
    assert es.max() <= tol and ec.max() <= tol


def host_normals(seed, first, count):
    from butterfly_amd import _capi
    lib = _capi.load()
    return np.array([lib.bfhipNormalValue(seed, first + i) for i in range(count)])


def test_fill_normal_is_the_host_stream(case):
    import torch
    c, op = case, case["ops"][False, False]
    seed, first, count = 2024, 12345678901, N * 70
    want = host_normals(seed, first, count)
    d64 = op.fill_normal(torch.empty(count, dtype=torch.float64, device=c["dev"]), seed, first).cpu().numpy()
    ulps = np.abs(d64 - want) / np.spacing(np.abs(want))
    print(f"fill_normal F64 vs bfhipNormalValue: max {ulps.max()} ulp")
    assert ulps.max() <= ULP_BOUND
    d32 = op.fill_normal(torch.empty(count, dtype=torch.float32, device=c["dev"]), seed, first).cpu().numpy()
    w32 = want.astype(np.float32)
    ulps32 = np.abs(d32.astype(np.float64) - w32.astype(np.float64)) / np.spacing(np.abs(w32)).astype(np.float64)
    print(f"fill_normal F32 vs the rounded host value: max {ulps32.max()} float ulp")
    assert ulps32.max() <= 1
    # a range is its pieces: [0, a + b) = [0, a) ++ [a, a + b), for both element types
    a, b = 1000, 777
    for dt in (torch.float64, torch.float32):
        whole = op.fill_normal(torch.empty(a + b, dtype=dt, device=c["dev"]), seed, 0)
        lo = op.fill_normal(torch.empty(a, dtype=dt, device=c["dev"]), seed, 0)
        hi = op.fill_normal(torch.empty(b, dtype=dt, device=c["dev"]), seed, a)
        assert torch.equal(whole, torch.cat([lo, hi]))


def device_w(c, op, seed, first, nrhs, demote):
    """W[j, s] = N(seed, (first + s) * n + j): the sample-major stream, transposed into the block layout."""
    import torch
    dt = torch.float32 if demote else torch.float64
    t = op.fill_normal(torch.empty((nrhs, N), dtype=dt, device=c["dev"]), seed, first * N)
    return t.t().contiguous()


@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("demote", [False, True])
def test_draw_is_the_block_sample_of_the_device_normals(case, demote, blocks):
    import torch
    c, op, tol = case, case["ops"][demote, blocks], tol_of(demote)
    g, p = c["gam"][demote], c["perm"]
    seed, first = 99, 5
    for nrhs in (1, 3, 64, 70):
        z = op.cov_draw_device(g, p, seed, first, nrhs)
        assert torch.equal(z, op.cov_sample_block_device(g, p, device_w(c, op, seed, first, nrhs, demote)))
    # no diagonal, no permutation
    assert torch.equal(op.cov_draw_device(None, None, seed, first, 17), op.cov_sample_block_device(None, None, device_w(c, op, seed, first, 17, demote)))
    # against the oracle on the host's normals
    nrhs = 70
    Wh = host_normals(seed, first * N, nrhs * N).reshape(nrhs, N).T
    e = col_errs(op.cov_draw_device(g, p, seed, first, nrhs).cpu().numpy(), c["ora"].sample(Wh))
    print(f"draw demote={demote} blocks={blocks}: max rel-l2 vs the oracle on host normals {e.max():.3e}")
    assert e.max() <= tol
    # a sample does not depend on the call it is drawn in: its W is the same bits (the apply may sum in another order)
    za, zb = op.cov_draw_device(g, p, seed, 0, 40), op.cov_draw_device(g, p, seed, 40, 30)
    e = col_errs(torch.cat([za, zb], dim=1).cpu().numpy(), op.cov_draw_device(g, p, seed, 0, 70).cpu().numpy())
    assert e.max() <= tol


def check_moments(Z, got_sum, got_sq, K):
    """|sum - sum_s z_s| <= K 2^-52 sum_s |z_s| per row, likewise for the squares (Z widened to double exactly)."""
    Z = Z.astype(np.float64)
    bound = K * 2.0 ** -52
    if got_sum is not None:
        err, scale = np.abs(got_sum - Z.sum(axis=1)), np.abs(Z).sum(axis=1)
        print(f"moments: max |sum err| / sum|z| = {np.max(err / scale):.3e} (bound {bound:.3e})")
        assert np.all(err <= bound * scale)
    if got_sq is not None:
        err, scale = np.abs(got_sq - (Z * Z).sum(axis=1)), (Z * Z).sum(axis=1)
        print(f"moments: max |sumsq err| / sum z^2 = {np.max(err / scale):.3e} (bound {bound:.3e})")
        assert np.all(err <= bound * scale)


@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("demote", [False, True])
def test_streaming_moments(case, demote, blocks):
    import torch
    c, op = case, case["ops"][demote, blocks]
    g, p = c["gam"][demote], c["perm"]
    seed, K = 4242, 150
    # the samples the moments run forms, drawn with its own splits: batches of 64, 64 and 22
    Z = torch.cat([op.cov_draw_device(g, p, seed, f, b) for f, b in ((0, 64), (64, 64), (128, 22))], dim=1).cpu().numpy()
    s, q = torch.zeros(M, dtype=torch.float64, device=c["dev"]), torch.zeros(M, dtype=torch.float64, device=c["dev"])
    op.cov_moments_device(g, p, seed, 0, K, 64, s, q)
    check_moments(Z, s.cpu().numpy(), q.cpu().numpy(), K)
    # two identical runs are bit-identical
    s2, q2 = torch.zeros_like(s), torch.zeros_like(q)
    op.cov_moments_device(g, p, seed, 0, K, 64, s2, q2)
    assert torch.equal(s, s2) and torch.equal(q, q2)
    # sumsq = None: the sums alone, the same bits
    s3 = torch.zeros_like(s)
    op.cov_moments_device(g, p, seed, 0, K, 64, s3, None)
    assert torch.equal(s3, s)
    q3 = torch.zeros_like(q)
    op.cov_moments_device(g, p, seed, 0, K, 64, None, q3)
    assert torch.equal(q3, q)
    # a second call adds to what is there: samples 150 .. 299 in batches of 64, 64, 22
    op.cov_moments_device(g, p, seed, K, K, 64, s, q)
    Z2 = torch.cat([op.cov_draw_device(g, p, seed, K + f, b) for f, b in ((0, 64), (64, 64), (128, 22))], dim=1).cpu().numpy()
    check_moments(np.concatenate([Z, Z2], axis=1), s.cpu().numpy(), q.cpu().numpy(), 2 * K)
    # batch = 0 means 64; a small odd batch (the scalar path of the moments kernel) meets the same bound on its own splits
    s4, q4 = torch.zeros_like(s), torch.zeros_like(q)
    op.cov_moments_device(g, p, seed, 0, K, 0, s4, q4)
    assert torch.equal(s4, s2) and torch.equal(q4, q2)
    s5, q5 = torch.zeros_like(s), torch.zeros_like(q)
    op.cov_moments_device(None, None, seed, 0, 20, 7, s5, q5)
    Z5 = torch.cat([op.cov_draw_device(None, None, seed, f, b) for f, b in ((0, 7), (7, 7), (14, 6))], dim=1).cpu().numpy()
    check_moments(Z5, s5.cpu().numpy(), q5.cpu().numpy(), 20)


def test_a_larger_shape_once():
    """m = 4099, n = 515, 64 columns, F32: rows span many workgroups and m * nrhs is no multiple of the block size."""
    import torch
    import randgraph
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from oracle import bfref
    m, n, nrhs = 4099, 515, 64
    rng = np.random.default_rng(78)
    desc, vals = randgraph.random_operand(rng, depth=4, size_hint=120, cplx=False, m=m, n=n)
    A = bfref.from_desc(desc, vals)
    gam = rng.random(n) + 0.1
    row_perm = rng.permutation(m)
    ora = Oracle(A, gam, row_perm, None)
    W = rng.standard_normal((n, nrhs))
    dev = torch.device("cuda", 0)
    op = HipOperator.from_bfmat(A.ptr.value, flags=_capi.FLAG_ADJOINT, demote_to_f32=True)
    op.set_real_rhs_blocks(2)
    g = torch.from_numpy(gam).to(dev).to(torch.float32)
    p = torch.from_numpy(row_perm.astype(np.int64)).to(dev)
    z = op.cov_sample_block_device(g, p, torch.from_numpy(W).to(dev).to(torch.float32).contiguous())
    e = col_errs(z.cpu().numpy(), ora.sample(W))
    print(f"larger shape: sample max rel-l2 {e.max():.3e}")
    assert e.max() <= 2e-5
    seed, K = 7, 150
    Z = torch.cat([op.cov_draw_device(g, p, seed, f, b) for f, b in ((0, 64), (64, 64), (128, 22))], dim=1).cpu().numpy()
    s, q = torch.zeros(m, dtype=torch.float64, device=dev), torch.zeros(m, dtype=torch.float64, device=dev)
    op.cov_moments_device(g, p, seed, 0, K, 64, s, q)
    check_moments(Z, s.cpu().numpy(), q.cpu().numpy(), K)
    op.close()


def test_the_sampling_example_builds_and_runs(tmp_path):
    """examples/cov_sampling_device.c: plain C against include/bfhip*.h, -Wall -Werror, run at its smallest size in a
    child process of its own."""
    lib = os.path.join(ROOT, "butterfly_amd", "csrc")
    exe = str(tmp_path / "cov_sampling_device")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "cov_sampling_device.c"), "-L", lib, "-lbfhip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-lm", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = subprocess.run([exe, "4096", "15", "64"], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0
    assert "per sample" in p.stdout
