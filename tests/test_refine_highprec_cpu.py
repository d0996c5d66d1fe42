"""The long-double checks of a refinement result (tests/refine_highprec.py) without a GPU: the restatement
(tests/refine_ref.py, with the plan emulator's complex64 model of a plan-only inner operator and the fp64 matvec as the
system) meets every check on every case of tests/refine_catalogue.py, each deliberately wrong restatement (a mutant) breaks a
named check on a named case, and the catalogue reaches the edges it is there for.

`blockdiag262145_k1_inv` is left to the GPU: the plan emulator walks its 16385 leaves in Python for every apply, which takes
far more than a few seconds.  Its operator shape is covered here by `blockdiag65537_k2_inv`."""
import numpy as np
import pytest

import gmres_catalogue as cat
import refine_catalogue as rcat
import refine_highprec as rh
import refine_ref

restated = rcat.restated


def _cpu_names():
    return [n for n in rcat.names() if not rcat.case(n).slow]


def checked(c, **kw):
    result, its = restated(c, **kw)
    return result, rh.check(rcat.problem(c), c.B, c.X0, result, c.tol, c.max_outer, iterates=its, xstar=rcat.solution(c.name),
                            zero_cols=c.zero_cols, converges=c.converges)


@pytest.mark.parametrize("name", _cpu_names())
def test_restatement_meets_every_check(name):
    c = rcat.case(name)
    result, fails = checked(c)
    print(f"{name}: outer={result[1]} inner={result[2]} residual={result[3]:.3e} history={result[4]}")
    assert not fails, (name, fails)
    if name in rcat.HISTORY1:
        assert abs(result[4][1] - rcat.HISTORY1[name]) <= 1e-9 * rcat.HISTORY1[name]
    if c.converges:
        assert result[1:3] == rcat.RESTATED[name]
    else:                                     # the catalogue's claim, both ways: these cases are there because they do not converge
        assert result[3] > c.tol and name not in rcat.RESTATED, (name, result[3])


def test_the_solution_is_a_solution():
    for name in ("dense257_k2", "dense257_mixed_2^-600_2^600", "blockdiag65537_k2", "normal300_k2"):
        c = rcat.case(name)
        pb = rcat.problem(c)
        r = rh._norm(c.B.astype(rh.LD) - pb.plain(rcat.solution(name))) / rh._norm(c.B)
        assert float(r.max()) <= 64 * pb.kappa * rh.gh.U_LD * np.sqrt(c.n), (name, r)


def test_restatement_keeps_its_results_on_ordinary_input():
    """The scaled norms are the unscaled ones bit for bit where nothing leaves the range."""
    c = rcat.case("dense257_k3_x0")
    (X, k, inner, res, hist), _ = restated(c)
    (Xu, ku, iu, resu, histu), _ = restated(c, scaled=False)
    assert np.array_equal(X.view(np.uint64), Xu.view(np.uint64)) and (k, inner, hist) == (ku, iu, histu)
    R = c.B - cat.operator(c.op).mv64(c.X0)
    Rs, rs, e = refine_ref.column_norms(R)
    assert np.array_equal(np.ldexp(rs, e), np.linalg.norm(R, axis=0))


def _drop_last_row(X, s, D):
    Y = X + s * D
    Y[-1] = X[-1]
    return Y


# mutant -> (keywords of refine_ref.solve_refine, cases, the checks one of which must fail on EVERY one of the cases).
# The three wrong updates leave a result whose reported residual is still the true residual of the X they return, and the
# forward bound holds for any X (tests/refine_highprec.py): what they break is convergence.  That has power only on cases that
# converge, which is why every row-block shape has a converging case and the wrong updates are held to them too.
MUTANTS = {
    "unscaled_norms": (dict(scaled=False), ("dense257_scaled_2^-600", "dense257_scaled_2^600", "dense257_mixed_2^-600_2^600"),
                       ("consistency", "finite")),
    "residual_from_the_low_operator": (dict(residual_matmul="low"), ("dense257_k3", "dense1000_k1_inv"), ("consistency",)),
    "last_iterate_returned": (dict(keep_best=False), ("normal300_unrelated_inner_operator",), ("best", "consistency")),
    "update_without_the_scale": (dict(update=lambda X, s, D: X + (s > 0) * D), ("dense257_k3", "dense256_k2", "dense255_k8", "dense1000_k1_inv", "blockdiag65537_k2_inv"), ("converged",)),
    "update_in_float32": (dict(update=lambda X, s, D: (X + s * D).astype(np.complex64).astype(np.complex128)),
                          ("dense257_k3", "normal300_k2", "dense1000_k1_inv", "blockdiag65537_k2_inv"), ("converged",)),
    "zero_column_divided": (dict(guard_zero=False), ("dense257_zero_first", "dense257_zero_middle", "dense257_zero_last"), ("finite",)),
    "dropped_row_in_the_update": (dict(update=_drop_last_row), ("dense257_k3", "dense1_k1", "dense255_k8", "dense1000_k1_inv", "blockdiag65537_k2_inv"), ("converged",)),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_every_mutant_breaks_a_named_check(mutant):
    kw, names, expected = MUTANTS[mutant]
    broken = {}
    for name in names:
        c = rcat.case(name)
        k = dict(kw)
        if k.get("residual_matmul") == "low":
            k["residual_matmul"] = rcat.low_model(c.low_key)
        _, fails = checked(c, **k)
        hit = sorted({f.split(":")[0] for f in fails} & set(expected))
        if hit:
            broken[name] = hit
    print(mutant, broken)
    assert set(broken) == set(names), f"mutant {mutant} met every one of {expected} on {sorted(set(names) - set(broken))}"


def test_the_unscaled_mutant_is_the_silent_wrong_answer():
    """b of 2^-600 with unscaled squares: every |r|^2 flushes to zero, the column passes for a zero column, x = 0 comes back with
    residual 0; b of 2^+600: the sum is inf, the residual inf / inf."""
    (X, k, _, res, hist), _ = restated(rcat.case("dense257_scaled_2^-600"), scaled=False)
    assert k == 0 and res == 0.0 and not X.any()
    (X, k, _, res, hist), _ = restated(rcat.case("dense257_scaled_2^600"), scaled=False)
    assert k == 0 and np.isnan(res) and not X.any()


def test_catalogue_reaches_the_kernel_edges():
    cases = [rcat.case(n) for n in rcat.names()]
    ns = {c.n for c in cases}
    assert {1, 2, 3, 255, 256, 257, 1000, 65537, 262145} <= ns
    assert [c.name for c in cases if c.slow] == ["blockdiag262145_k1_inv"]
    # every row-block shape has a case that is held to convergence
    assert {255, 256, 257, 1000, 65537, 262145} <= {c.n for c in cases if c.converges}
    nb, per, blocks = cat.row_blocks(65537)
    assert nb == 257 and blocks[-1][1] - blocks[-1][0] < per
    nb, per, blocks = cat.row_blocks(262145)
    assert nb == 1024 and blocks[-1][0] == blocks[-1][1] == 262145
    counts = {c.n * c.B.shape[1] for c in cases}
    assert any(v < 256 for v in counts) and any(v % 256 == 0 for v in counts) and any(v % 256 == 1 for v in counts)
    assert {c.max_inner for c in cases} >= {1, 3, 8, 16, rcat.FULL}
    assert {c.precond for c in cases} == {None, "c128", "c64", "inverse"}
    assert {c.zero_cols for c in cases if c.name.startswith("dense257_zero_")} == {(0,), (1,), (2,)}
    assert any(c.X0 is not None and not c.B[:, 0].any() for c in cases) and any(c.low for c in cases)
    for base in rcat.SCALE_BASES:
        assert rcat.case(base).X0 is None and rcat.case(base).B.shape[1] == 2
    assert rcat.ORTHS == ("mgs", "cgs2")
