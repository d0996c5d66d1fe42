"""bfEvalKernel and bfHelm2DenseKernel (bfhip_build.hip) entry by entry against mpmath at 50 digits.

The truth is the committed fixture tests/golden/helm2_eval_mp.npz; the cases and the error unit are in
tests/helm2_eval_cases.py:  err = |got - truth| / (u (1 + kr) scale), the factor 1 + kr dropped on the axis cases, whose
arguments are exact.  The yardstick is the float64 restatement of bfKernelEntry with the host C library's Bessel
functions (what the reference calls): the device may be at most 8 times worse than it, or than one unit where the
restatement is better than that -- the project's standing margin (tests/test_gpu_cheb_cov.py)."""
import math

import numpy as np
import pytest

import helm2_eval_cases as cat

pytestmark = pytest.mark.gpu

MARGIN = 8.0


def build_leaf(points, k, recipe, **kw):
    from butterfly_amd.operator import helm2_build_leaf
    return helm2_build_leaf(points, k, recipe, **kw)


# --------------------------------------------------------------------------
# axis leaves: J0, Y0, J1, Y1 at designed arguments and nothing else
# --------------------------------------------------------------------------
_AXIS = {}


def axis_leaf(leaf, k):
    """The device's N x 1 axis leaf, built once per (leaf, k)."""
    if (leaf, k) not in _AXIS:
        pot, _ = cat.AXIS_LEAVES[leaf]
        pts, recipe = cat.axis_problem(k)
        kw = {} if pot == "S" else dict(normals=cat.axis_normals(leaf, len(pts)))
        got = build_leaf(pts, k, recipe, layer_pot=pot, **kw)
        assert got.shape == (len(pts) - 1, 1) and got.size > 1024          # several evaluation tiles
        _AXIS[(leaf, k)] = got
    return _AXIS[(leaf, k)]


@pytest.mark.parametrize("leaf", list(cat.AXIS_LEAVES))
def test_axis_leaf_per_decade(leaf):
    pot, _ = cat.AXIS_LEAVES[leaf]
    order = 0 if pot == "S" else 1
    x = cat.fixture()["axis/x"]
    primary = cat.axis_dot_signs(leaf).index(1.0)
    dev = cat.axis_errors(cat.axis_blocks(leaf, 1.0, axis_leaf(leaf, 1.0))[primary], order)
    ref = cat.axis_errors(cat.axis_blocks(leaf, 1.0, cat.restate(cat.axis_operands(leaf, 1.0)))[primary], order)
    failures = []
    print(f"\n{leaf}: decade | err J{order} (device, C library) | err Y{order} (device, C library)")
    tables = [(cat.decade_max(d, x), cat.decade_max(r, x)) for d, r in zip(dev, ref)]
    for dec in sorted(tables[0][0]):
        row = []
        for fn, (td, tr) in zip(("J", "Y"), tables):
            row.append(f"{td[dec]:8.2f} {tr[dec]:6.2f}")
            if not td[dec] <= MARGIN * max(tr[dec], 1.0):
                failures.append((f"{fn}{order}", dec, td[dec], tr[dec]))
        print(f"  1e{dec:+03d} | " + " | ".join(row))
    assert not failures, failures


@pytest.mark.parametrize("leaf", list(cat.AXIS_LEAVES))
def test_axis_directions_and_wavenumber_scaling(leaf):
    blocks = cat.axis_blocks(leaf, 1.0, axis_leaf(leaf, 1.0))
    signs = cat.axis_dot_signs(leaf)
    primary = signs.index(1.0)
    assert np.all(np.isfinite(blocks))
    for b, s in enumerate(signs):              # (0, x), (-x, 0): the same magnitudes, the sign of n.d (0 where n.d == 0)
        assert np.array_equal(blocks[b], s * blocks[primary]), (leaf, b)
    # k = 32 with every coordinate divided by 32: the same arguments, the same bits (S' and D carry the factor k)
    assert np.array_equal(cat.axis_blocks(leaf, 32.0, axis_leaf(leaf, 32.0)), blocks)


# --------------------------------------------------------------------------
# geometry leaves: every branch of bfKernelEntry
# --------------------------------------------------------------------------
def geom_leaf(name):
    case = cat.geom_cases()[name]
    pts = cat.geom_curve()[0]
    return build_leaf(pts, cat.GEOM_K, case["recipe"], **cat.problem_kwargs(case["pot"], case["deco"]))


@pytest.mark.parametrize("name", list(cat.geom_cases()))
def test_geometry_leaf_entrywise(name):
    got = geom_leaf(name)
    o = cat.geom_operands(name)
    e_dev = cat.geom_err(name, got)
    e_ref = float(cat.geom_err(name, cat.restate(o)).max())
    worst = np.unravel_index(int(np.argmax(e_dev)), e_dev.shape)
    print(f"\n{name}: max err device {e_dev.max():.2f} at {worst}, C library {e_ref:.2f}")
    assert e_dev.max() <= MARGIN * max(e_ref, 1.0), (name, float(e_dev.max()), e_ref, worst)
    mask = o["self_mask"]
    assert np.all(got[mask] == o["self_value"])                            # self entries: bit exact
    assert mask.sum() == (5 if case_is_node_to_node(name) else 0)


def case_is_node_to_node(name):
    rc = cat.geom_cases()[name]["recipe"]
    return rc[1][0] == "node" and rc[2][0] == "node"


@pytest.mark.parametrize("pot", cat.POTENTIALS)
def test_leaf_alone_equals_leaf_as_second_recipe(pot):
    """The same leaf as the second of two recipes of one build: its tiles follow the two tiles of a 40 x 40 leaf in the
    flat tile list, so the tile prefix and the binary search over it decide where every entry goes."""
    from butterfly_amd import _capi, helm2_structure as hs
    from butterfly_amd.operator import HipOperator
    case = cat.geom_cases()[f"{pot}/circle_to_node"]
    pts = cat.geom_curve()[0]
    kw = cat.problem_kwargs(pot, case["deco"])
    alone = build_leaf(pts, cat.GEOM_K, case["recipe"], **kw)
    first = ("kernel", ("node", 0, cat.GEOM_N), ("node", 0, cat.GEOM_N))
    d = hs.Desc()
    a = d.add(hs.NODE_DENSE, cat.GEOM_N, cat.GEOM_N)
    b = d.add(hs.NODE_DENSE, *alone.shape)
    d.root = d.add(hs.NODE_BLOCK, cat.GEOM_N + alone.shape[0], cat.GEOM_N + alone.shape[1], [(a, 0, 0), (b, cat.GEOM_N, cat.GEOM_N)],
                   hs.BF_TYPE_BLOCK_DIAG)
    d.recipe = {a: first, b: case["recipe"]}
    # exact complex products: the extraction multiplies by unit vectors, which Gauss's three multiplications do not
    # return bit for bit
    op, st = HipOperator.build_helm2(d, pts, cat.GEOM_K, flags=_capi.FLAG_EXACT_COMPLEX, **kw)
    try:
        assert st["kernelLeaves"] == 2 and st["numBatches"] == 1
        dense = op.to_dense()
    finally:
        op.close()
    assert np.array_equal(dense[cat.GEOM_N:, cat.GEOM_N:], alone)
    assert np.array_equal(dense[:cat.GEOM_N, :cat.GEOM_N], build_leaf(pts, cat.GEOM_K, first, **kw))
    assert not dense[:cat.GEOM_N, cat.GEOM_N:].any() and not dense[cat.GEOM_N:, :cat.GEOM_N].any()


@pytest.mark.parametrize("name", list(cat.geom_reexp_cases()))
def test_reexpansion_is_made_of_an_undecorated_and_a_weighted_matrix(name):
    """X = Z_equiv \\ Z_orig with Z_equiv evaluated with decorate = 0 (no weights, 0 where a check point is an equivalent
    source, not the self value) and Z_orig with the column weights: the residual test of
    test_reexpansion_leaf_matches_truncated_svd_least_squares, with both matrices taken from the truth."""
    from oracle import helm2_build as hb
    case = cat.geom_reexp_cases()[name]
    pts = cat.geom_curve()[0]
    X = build_leaf(pts, cat.GEOM_K, case["recipe"], **cat.problem_kwargs(case["pot"], case["deco"]))
    z_eq, z_or = cat.geom_truth(f"{name}/z_equiv")[0], cat.geom_truth(f"{name}/z_orig")[0]
    want = hb.lstsq_truncated(z_eq, z_or)
    assert X.shape == want.shape
    res_gpu = np.linalg.norm(z_eq @ X - z_or) / np.linalg.norm(z_or)
    res_ref = np.linalg.norm(z_eq @ want - z_or) / np.linalg.norm(z_or)
    print(f"\n{name}: residual device {res_gpu:.3e}, reference {res_ref:.3e}, cond {np.linalg.cond(z_eq):.1e}")
    assert res_gpu <= 2 * res_ref + 1e-13, (res_gpu, res_ref)
    assert np.linalg.norm(z_eq @ X - z_eq @ want) <= 1e-10 * np.linalg.norm(z_eq @ want)
    assert np.linalg.norm(X) <= 1.5 * np.linalg.norm(want)


# --------------------------------------------------------------------------
# Kapur-Rokhlin end to end on the unit circle
# --------------------------------------------------------------------------
def kr_circle_device_error(n, order, perm=None):
    from butterfly_amd.operator import helm2_dense_apply
    pts, x, w = cat.kr_circle_problem(n)
    orig = np.arange(n) if perm is None else perm
    y = helm2_dense_apply(pts[orig], cat.KR_CIRCLE_K, x[orig], col_weights=w[orig], kr_order=order, orig_index=orig.astype(np.uint64))
    return y, float(np.max(np.abs(y - cat.KR_CIRCLE_EIGENVALUE * x[orig])) / abs(cat.KR_CIRCLE_EIGENVALUE))


@pytest.mark.parametrize("order", cat.KR_ORDERS)
def test_kr_dense_apply_converges_at_its_order(order):
    errs = []
    for n in cat.KR_CIRCLE_NS:
        y, e = kr_circle_device_error(n, order)
        e_np = cat.kr_circle_error(n, order)
        print(f"\norder {order} n {n}: device {e:.3e}, numpy {e_np:.3e}")
        assert e <= 2 * e_np + 1e-13, (order, n, e, e_np)
        errs.append(e)
        # the points in another order, orig_index set accordingly: the same values up to the order of summation
        perm = (7 * np.arange(n) + 3) % n
        yp, _ = kr_circle_device_error(n, order, perm)
        pts, x, w = cat.kr_circle_problem(n)
        o = cat.operands("S", ("node", 0, n), ("node", 0, n), True, pts, col_weights=w, k=cat.KR_CIRCLE_K)
        absrow = (np.abs(cat.restate(o)) * np.abs(cat.kr_factors(order, np.arange(n), np.arange(n), n))) @ np.abs(x)
        bound = math.sqrt(2) * (2 * n + 16) * cat.U * absrow[perm]       # each of the two sums is within it of the exact one
        assert np.all(np.abs(yp - y[perm]) <= 2 * bound), (order, n, float(np.max(np.abs(yp - y[perm]) / bound)))
    rates = cat.observed_orders(errs)
    print(f"order {order}: observed {rates}")
    assert min(rates) >= order - 1, (errs, rates)


# --------------------------------------------------------------------------
# dense apply: several source slices, a short last slice, a partial target block, a non-square call
# --------------------------------------------------------------------------
def dense_variants(name):
    pts, nrm, orig, w, x, tp, tn = cat.dense_problem(name)
    tgt = {} if tp is None else dict(tgt_points=tp, tgt_normals=tn)
    out = {"S": dict(layer_pot="S", **tgt),
           "combined_weights": dict(layer_pot="combined", normals=nrm, alpha=cat.GEOM_ALPHA, beta=cat.GEOM_BETA, col_weights=w, **tgt)}
    if tp is None:
        out["combined_kr10_self"] = dict(layer_pot="combined", normals=nrm, alpha=cat.GEOM_ALPHA, beta=cat.GEOM_BETA, col_weights=w,
                                         kr_order=10, orig_index=orig, self_value=cat.GEOM_SELF)
    return out


@pytest.mark.parametrize("name", list(cat.DENSE_SHAPES))
def test_dense_apply_shapes(name):
    """Reference: the device-built full leaf (validated entry by entry above, same bfKernelValue) times x in long double.
    Per row |y - y_ld|_i <= sqrt(2) (2 n + 16) u (|A| |x|)_i: Higham's bound for n complex fused multiply-adds, plus the
    sum over slices and the few roundings by which the two kernels assemble an entry differently.  It bounds summation
    only: a wrong slice edge or a dropped source misses it by orders of magnitude."""
    from butterfly_amd.operator import helm2_dense_apply
    n, m = cat.DENSE_SHAPES[name]
    pts, nrm, orig, w, x, tp, tn = cat.dense_problem(name)
    for label, kw in dense_variants(name).items():
        y = helm2_dense_apply(pts, cat.DENSE_K, x, **kw)
        recipe = ("kernel", ("node", 0, n), ("tnode", 0, m) if m else ("node", 0, n))
        A = build_leaf(pts, cat.DENSE_K, recipe, **kw)
        assert A.shape == (m or n, n) and y.shape == (m or n,)
        Al, xl = A.astype(np.clongdouble), x.astype(np.clongdouble)
        y_ld = Al @ xl
        absrow = np.abs(A) @ np.abs(x)
        bound = math.sqrt(2) * (2 * n + 16) * cat.U * absrow
        ratio = np.abs(y.astype(np.clongdouble) - y_ld).astype(np.float64) / bound
        print(f"\n{name} {label}: max |y - y_ld| / bound = {ratio.max():.3f}")
        assert np.all(np.isfinite(y)) and ratio.max() <= 1.0, (name, label, float(ratio.max()), int(ratio.argmax()))
        if "self_value" in kw:
            assert np.all(np.diag(A) == cat.GEOM_SELF)
