"""What the builders of tests/cond_cases.py claim, checked without a GPU, so that tests/test_gpu_cov_cond_shapes.py can be read as
a statement about the device alone:
  A. the random graph of seed 79 is not a zero operator and its three chunks of columns carry the Frobenius norms 8.80, 8.78, 1.69;
     every chunk of every operand, left out of G or of B^T W, moves the reference alpha by at least 1e3 tolerances;
  B. the measured cond(K) of every designed spectrum is within 1e-3 (relative) of the design; the float64 host pipeline that the
     device's forward error is measured against solves a well-conditioned system to rounding;
  C. the integer case is exact: a float64 right-looking factorization of G returns L0 and both substitutions return x0, bit for bit."""
import numpy as np
import pytest

import cond_cases as cc


@pytest.fixture(scope="module")
def operands():
    return cc.chunk_operands()


def test_the_graph_operand_fills_its_three_chunks(operands):
    op = operands["graph"]
    assert (op.m, op.n) == (157, 2085)
    norms = [float(np.linalg.norm(op.phi[:, sl])) for sl in cc.chunk_slices(op.n)]
    print(f"graph operand: Frobenius norms of the chunks {np.array2string(np.array(norms), precision=4)}")
    assert len(norms) == 3 and all(v > 0 for v in norms)
    for got, want in zip(norms, cc.GRAPH_CHUNK_NORMS):
        assert abs(got - want) <= 0.01 * want
    # the dense form is the operator's: the numpy densifier of the descriptor agrees with the oracle's rows
    dense = cc.randgraph.densify(op.desc, op.vals, op.desc.root)
    assert np.linalg.norm(dense - op.phi) <= 1e-13 * np.linalg.norm(dense)


def test_the_dense_leaves_are_one_chunk_and_one_chunk_plus_a_column(operands):
    one, one_row = operands["one"], operands["one_row"]
    assert (one.m, one.n) == (140, cc.CHUNK) and len(cc.chunk_slices(one.n)) == 1
    assert (one_row.m, one_row.n) == (140, cc.CHUNK + 1) and cc.chunk_slices(one_row.n)[1] == slice(cc.CHUNK, cc.CHUNK + 1)
    assert one_row.gam[cc.CHUNK] == cc.ONE_ROW_GAMMA and one_row.gam[:cc.CHUNK].max() < 1.1
    for op in (one, one_row):                    # a one-leaf operand: the oracle's rows are the leaf's values, exactly
        assert np.array_equal(op.phi, op.vals[op.desc.root])


@pytest.mark.parametrize("q", cc.A_QS)
@pytest.mark.parametrize("k", cc.A_KS)
@pytest.mark.parametrize("name,demote", [("graph", False), ("graph", True), ("one", False), ("one_row", False)])
def test_every_chunk_moves_the_reference(operands, name, demote, k, q):
    cc.assert_every_chunk_matters(operands[name], demote, k, q)
    ref, _, query = operands[name].case(demote, k)
    assert len(ref.obs) == k and len(query) == len(set(query)) == cc.NQUERY        # 70 distinct query indices: two panels


@pytest.mark.parametrize("k,n,kappa", cc.SPECTRUM_CASES)
def test_the_designed_spectrum_is_the_measured_one(k, n, kappa):
    case = cc.SpectrumCase(k, n, kappa, with_reference=False)
    got = case.measured_kappa()
    print(f"k={k} n={n}: designed kappa {kappa:.1e}, measured {got:.6e} (relative difference {abs(got / kappa - 1):.2e})")
    assert case.phi.shape == (k, n) and sorted(case.obs) == list(range(k)) and sorted(case.row_perm) == list(range(k))
    assert case.lam[0] == 1.0 and abs(case.lam[-1] * kappa - 1) <= 1e-12 and np.all(case.lam > case.delta)
    assert abs(got / kappa - 1) <= 1e-3


def test_the_float64_host_pipeline_on_a_small_system():
    """host_float64 against numpy's own solve and slogdet at cond(K) = 1e2: rounding, nothing else."""
    case = cc.SpectrumCase(40, 60, 1e2, with_reference=False)
    noise = np.full(40, case.delta)
    alpha, values = cc.host_float64(case.Bt, noise, case.y, case.W, case.E)
    K = case.Bt.T @ case.Bt + np.diag(noise)
    want = np.linalg.solve(K, case.y[:, None] - case.Bt.T @ case.W - case.E)
    quad, logdet = case.y @ np.linalg.solve(K, case.y), np.linalg.slogdet(K)[1]
    assert cc.col_errs(alpha, want).max() <= 1e-13
    assert abs(values[1] - quad) <= 1e-13 * quad and abs(values[2] - logdet) <= 1e-13 * abs(logdet)
    assert abs(values[0] - (-quad / 2 - logdet / 2 - 20 * np.log(2 * np.pi))) <= 1e-13 * abs(values[0])


@pytest.mark.parametrize("k", [97, 300])
def test_the_integer_case_is_exact_in_float64(k):
    case = cc.IntegerCase(k)
    L0, G = case.L0, case.G
    assert np.all(np.diag(L0) == 2) and np.all(np.triu(L0, 1) == 0)
    off = L0 - 2 * np.eye(k, dtype=np.int64)
    assert np.all(np.abs(off).sum(axis=1)[3:] == 3) and set(np.unique(off)) == {-1, 0, 1}
    rows, cols = np.nonzero(off)
    assert np.all(rows - cols <= 40) and np.any(rows // 32 != cols // 32) and np.any(rows // 64 != cols // 64)   # entries cross the tile edges
    assert np.abs(G).max() <= 7 and np.all(np.diag(G) <= 7)
    # the factorization, in another order than the reference's, and both substitutions: the integers, bit for bit
    L = cc.cholesky_f64_right_looking(G)
    assert np.array_equal(L, L0.astype(np.float64))
    assert np.array_equal(np.linalg.cholesky(G.astype(np.float64)), L0.astype(np.float64))
    assert np.array_equal(cc.solve_f64(L, case.y.astype(np.float64)), case.x0.astype(np.float64))
    R = case.y[:, None] - L0 @ case.W - case.E
    assert np.array_equal(R, G @ case.X)
    assert np.array_equal(cc.solve_f64(L, R.astype(np.float64)), case.X.astype(np.float64))
    # float32 holds every input of the demoted run exactly
    for x in (L0, case.W):
        assert np.array_equal(x.astype(np.float32).astype(np.int64), x)
    assert np.abs(case.E).max() < 2 ** 24 and case.quad == int(case.x0 @ G @ case.x0) < 2 ** 53
    assert np.array_equal(case.prior, (L0[cc.inverse_perm(case.row_perm)[case.query]] ** 2).sum(axis=1))
    assert sorted(case.obs) == list(range(k))
