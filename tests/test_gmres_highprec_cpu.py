"""The long-double GMRES reference (tests/gmres_highprec.py) and its bounds, without a GPU: the reference against
np.linalg.solve, the fp64 restatement (oracle/linalg_ref.py) within every bound on every catalogue case, each deliberately
wrong restatement (a mutant) outside at least one, and the catalogue's reach over the kernels' edges."""
import numpy as np
import pytest

from oracle import linalg_ref
import gmres_catalogue as cat
import gmres_highprec as gh


def _cpu_names():
    return [n for n in cat.names() if not n.endswith("block_jacobi")]


def restated(c, **kw):
    op = cat.operator(c.op)
    msolve = None
    if c.precond == "dense":
        P = cat.dense_block_inverse(c.op)[0]
        msolve = lambda v: P @ v
    return linalg_ref.solve_gmres(op.mv64, c.B, X0=c.X0, tol=c.tol, max_num_iter=c.m, msolve=msolve, **kw)


def test_reference_agrees_with_a_dense_solve():
    for name in ("bie2048_k2", "normal300_kappa10_m17_x0", "cI255_random"):
        c = cat.case(name)
        op = cat.operator(c.op)
        kry = gh.Krylov(cat.problem(c), c.B, c.X0)
        m = c.n if c.n <= 300 else 60          # converged: the whole space, or the BIE system's few dozen steps
        x, r = kry.iterate(m)
        want = np.linalg.solve(op.dense, c.B)
        err = np.linalg.norm(x.astype(np.complex128) - want) / np.linalg.norm(want)
        assert err <= 1e-12 * op.kappa, (name, err)
        assert float(r.max()) <= 1e-12 * float(np.linalg.norm(c.B)), (name, r)


@pytest.mark.parametrize("name", _cpu_names())
def test_restatement_meets_every_bound(name):
    c = cat.case(name)
    X, it, hist = restated(c)
    if c.iters is not None:
        assert it == c.iters
    reported = hist[-1] if hist else 0.0
    kry = gh.Krylov(cat.problem(c), c.B, c.X0)
    fails = gh.check(kry, X, it, reported)
    assert not fails, (name, it, fails)
    X = X if X.ndim == 2 else X[:, None]
    for p in c.zero_cols:
        want = np.zeros(c.n, dtype=np.complex128) if c.X0 is None else c.X0[:, p]
        assert np.array_equal(np.ascontiguousarray(X[:, p]).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))


def test_restatement_keeps_the_reference_quirk_on_request():
    """reference_quirk=True is the reference's loop: on convergence at iteration j, j basis vectors and numIter = j.  With b an
    eigenvector it converges at j = 0 and returns x0."""
    c = cat.case("normal300_eigenvector_alone")
    op = cat.operator(c.op)
    X, it, hist = linalg_ref.solve_gmres(op.mv64, c.B, tol=c.tol, max_num_iter=c.m, reference_quirk=True)
    assert it == 0 and len(hist) == 1 and hist[0] < 1e-10 and np.all(X == 0)
    X, it, hist = linalg_ref.solve_gmres(op.mv64, c.B, tol=c.tol, max_num_iter=c.m)
    assert it == 1 and np.linalg.norm(op.mv64(X) - c.B) <= 1e-13 * np.linalg.norm(c.B)
    # a converged solve uses one vector more than the quirk does, and numIter counts it
    c = cat.case("bie2048_k2")
    op = cat.operator(c.op)
    Xq, itq, _ = linalg_ref.solve_gmres(op.mv64, c.B, tol=c.tol, max_num_iter=c.m, reference_quirk=True)
    X, it, _ = linalg_ref.solve_gmres(op.mv64, c.B, tol=c.tol, max_num_iter=c.m)
    assert it == itq + 1
    rq = np.linalg.norm(op.mv64(Xq) - c.B, axis=0).max()
    r = np.linalg.norm(op.mv64(X) - c.B, axis=0).max()
    assert r < rq


def _drop_row(n):
    """the last row of the ragged last row block (every catalogue n but 256 has one)"""
    def dot(U, W):
        return linalg_ref._dot(U[:n - 1], W[:n - 1])

    def sumsq(W):
        return linalg_ref._sumsq(W[:n - 1])
    return dot, sumsq


MUTANTS = {
    "reference_quirk": (lambda n: dict(reference_quirk=True), ("normal300_eigenvector_alone", "cI255_random", "bie2048_k2")),
    "no_conjugate": (lambda n: dict(dot=lambda U, W: np.einsum("ij,ij->j", U, W)), ("dense257_k3_m17", "dense3_k3_m8")),
    "dropped_row": (lambda n: dict(zip(("dot", "sumsq"), _drop_row(n))), ("dense1_k1_m1", "dense255_k8_m9", "dense3_k3_m8")),
    "float32_dots": (lambda n: dict(dot=lambda U, W: np.einsum("ij,ij->j", U.conj().astype(np.complex64), W.astype(np.complex64))
                                    .astype(np.complex128)), ("dense257_k3_m17", "bie2048_k2")),
    "unscaled_norms": (lambda n: dict(scaled=False), ("dense257_scaled_2^-600", "dense257_scaled_2^600", "dense257_mixed_2^-600_2^600")),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_every_mutant_breaks_a_bound(mutant):
    make, names = MUTANTS[mutant]
    broken = []
    for name in names:
        c = cat.case(name)
        with np.errstate(all="ignore"):
            X, it, hist = restated(c, **make(c.n))
        reported = hist[-1] if hist else 0.0
        fails = gh.check(gh.Krylov(cat.problem(c), c.B, c.X0), X, max(it, 1), reported)
        if fails:
            broken.append(name)
    assert broken, f"mutant {mutant} met every bound on {names}"


def test_catalogue_reaches_the_kernel_edges():
    ns = set()
    for name in cat.names():
        c = cat.case(name)
        ns.add(c.n)
    assert any(n % 256 for n in ns) and any(n < 256 for n in ns) and 256 in ns
    nb, per, blocks = cat.row_blocks(262145)
    assert nb == 1024 and per > 256 and 262145 in ns
    assert blocks[-1][0] == blocks[-1][1] == 262145 and sum(r1 - r0 for r0, r1 in blocks) == 262145
    # CGS2 reduces numVec = j + 1 dots for j < m: the groups of 8 are crossed at numVec % 8 in {0, 1, 7}
    num_vec = {v % 8 for name in cat.names() for v in range(1, cat.case(name).m + 1)}
    assert {0, 1, 7} <= num_vec
    assert {1, 7, 8, 9, 16, 17} <= {cat.case(name).m for name in cat.names()}
    assert {1, 2, 3, 8} <= {cat.case(name).B.shape[1] for name in cat.names()}
    # every special column kind runs under both orthogonalisations (the GPU tests take every case with each)
    kinds = {k for name in cat.names() for k in cat.case(name).kinds}
    assert set(cat.KINDS) <= kinds and cat.ORTHS == ("mgs", "cgs2")
    assert {cat.case(name).precond for name in cat.names()} == {None, "dense", "block_jacobi"}
    assert any(cat.case(name).X0 is not None for name in cat.names())
