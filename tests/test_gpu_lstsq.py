"""The device builder's least-squares kernels (bfhip_lstsq.hip: bfQrcpKernel, bfJacobiKernel<W>, bfJacobiGramKernel, bfJacobiGlobalKernel,
bfGemmKernel) through bfhipLstSqTruncated, on the designed cases of tests/lstsq_catalogue.py: every case on its declared
route and on the forced alternatives it fits, against the long-double reference and the bounds of tests/lstsq_ref.py."""
import numpy as np
import pytest

import lstsq_catalogue as cat
import lstsq_ref as ref

pytestmark = pytest.mark.gpu

_CASES = cat.catalogue()
_REF = {}


def _reference(c):
    if c["name"] not in _REF:
        if c["ref"] == "ld":
            _REF[c["name"]] = ref.reference(c["A"], c["B"])
        else:
            s = np.linalg.svd(c["A"], compute_uv=False)[:c["rank"]]
            _REF[c["name"]] = (c["X_design"], s, c["rank"])
    return _REF[c["name"]]


def _run(cases, opts, **kw):
    from butterfly_amd.operator import lstsq_truncated
    return lstsq_truncated([(c["A"], c["B"]) for c in cases], **(opts or {}), **kw)


def _runs():
    """(option set, cases) of every declared and alternative route."""
    groups = {}
    for c in _CASES:
        for o in [c["opts"]] + c["alt"]:
            groups.setdefault(cat.opts_key(o), (o, []))[1].append(c)
    return list(groups.values())


def _check(c, X, sig, info, declared):
    Xr, sr, kr = _reference(c)
    assert info["notConverged"] == 0, c["name"]
    assert np.all(np.isfinite(X)), c["name"]
    assert info["rank"] == c["rank"] == kr, (c["name"], info["rank"], c["rank"], kr)
    if declared:
        for k, v in c["route"].items():
            assert info["route"][k] == v, (c["name"], k, info["route"])
    assert len(sig) == kr
    if kr:
        assert np.max(np.abs(sig - sr)) <= ref.sigma_bound(c["A"], sr), (c["name"], sig[:4], sr[:4])
    if c["gap"]:
        err = float(np.linalg.norm(X - np.asarray(Xr, dtype=np.complex128)))
        assert err <= ref.x_bound(c["A"], c["B"], Xr, sr), (c["name"], err, ref.x_bound(c["A"], c["B"], Xr, sr))


def test_every_case_on_every_route_meets_the_bounds_and_is_repeatable():
    for opts, cases in _runs():
        first = _run(cases, opts)
        again = _run(cases, opts)
        for c, (X, sig, info), (X2, sig2, info2) in zip(cases, first, again):
            _check(c, X, sig, info, declared=opts is c["opts"])
            assert np.array_equal(X.view(np.float64), X2.view(np.float64)), c["name"]
            assert np.array_equal(sig, sig2) and info == info2, c["name"]


def test_alone_equals_inside_a_mixed_batch():
    for opts, cases in _runs():
        batch = _run(cases, opts)
        for c, (X, sig, info) in list(zip(cases, batch))[::3]:
            (Xa, siga, infoa), = _run([c], opts)
            assert np.array_equal(X.view(np.float64), Xa.view(np.float64)), c["name"]
            assert np.array_equal(sig, siga) and info == infoa, c["name"]


def test_power_of_two_scaling_leaves_x_bit_identical():
    for opts, cases in _runs():
        use = []
        for c in cases:
            if not c["gap"] or c["rank"] == 0:
                continue
            _, sr, _ = _reference(c)
            dim = max(c["A"].shape)
            # the "+ eps" of the rule is not scaled: only cases whose kept sigma stay 4x above tol at 2^-40 qualify
            if sr[-1] * 2.0 ** -40 >= 4 * ref.truncation_tol(sr[0] * 2.0 ** -40, dim):
                use.append(c)
        if not use:
            continue
        base = _run(use, opts)
        for s in (-40, 40):
            f = 2.0 ** s
            scaled = _run([dict(c, A=c["A"] * f, B=c["B"] * f) for c in use], opts)
            for c, (X, sig, info), (Xs, sigs, infos) in zip(use, base, scaled):
                assert np.array_equal(X.view(np.float64), Xs.view(np.float64)), (c["name"], s)
                assert np.array_equal(sig * f, sigs), (c["name"], s)
                assert info["rank"] == infos["rank"] and info["sweeps"] == infos["sweeps"], (c["name"], s)


_ALL_ROUTES = [cat.PLAIN, cat.GRAM, cat.GLOBAL, cat.QR]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_is_reported_on_every_route(bad):
    picks = [c for c in _CASES if c["name"] in ("gemm-49x33x31", "me2-9x2", "wide-12x30-odd", "suspect1-many-subthreshold-columns",
                                                "qr-duplicate-columns-40x10", "zero-30x20")]
    for opts in _ALL_ROUTES:
        probs = []
        for c in picks:
            A, B = c["A"].copy(), c["B"].copy()
            A[A.shape[0] // 2, A.shape[1] - 1] = bad
            probs.append(dict(c, A=A))
            A, B = c["A"].copy(), c["B"].copy()
            B[0, B.shape[1] - 1] = complex(0, bad)
            probs.append(dict(c, B=B))
        for p, (X, sig, info) in zip(probs, _run(probs, opts)):
            assert info["notConverged"] == 1 or not np.all(np.isfinite(X)), (p["name"], opts)
            assert info["notConverged"] == 1, (p["name"], opts)


def test_zero_and_underflowing_matrices_give_zero_on_every_route():
    picks = [c for c in _CASES if c["name"] in ("zero-30x20", "underflow-30x20")]
    for opts in _ALL_ROUTES:
        for c, (X, sig, info) in zip(picks, _run(picks, opts)):
            assert info["notConverged"] == 0 and info["rank"] == 0 and len(sig) == 0, (c["name"], opts, info)
            assert np.array_equal(X, np.zeros_like(X)), (c["name"], opts)


def test_reexpansion_leaf_is_the_least_squares_entry_on_its_kernel_leaves():
    """helm2_build_leaf's re-expansion = bfhipLstSqTruncated on the two kernel leaves it solves with, bit for bit
    (single layer, circle points: no decoration differs between the two evaluations)."""
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.operator import helm2_build_leaf, lstsq_truncated
    pts = hs.circle_points(16)
    for m, n, k in [(17, 23, 60.0), (45, 31, 400.0), (150, 170, 1500.0)]:
        src, eq, tgt = ("circle", 0.55, 0.05, 0.08, n), ("circle", 0.5, 0.0, 0.16, m), ("circle", -0.6, 0.1, 0.2, m)
        X = helm2_build_leaf(pts, k, ("reexp", src, eq, tgt))
        z_eq = helm2_build_leaf(pts, k, ("kernel", eq, tgt))
        z_or = helm2_build_leaf(pts, k, ("kernel", src, tgt))
        (Xl, sig, info), = lstsq_truncated([(z_eq, z_or)])
        assert info["notConverged"] == 0
        assert np.array_equal(X.view(np.float64), Xl.view(np.float64)), (m, n, k)


def test_argument_errors():
    from butterfly_amd import _capi
    from butterfly_amd.operator import lstsq_truncated
    with pytest.raises(ValueError):
        lstsq_truncated([(np.zeros((3, 0)), np.zeros((3, 1)))])
    with pytest.raises(ValueError):
        lstsq_truncated([(np.zeros((3, 2)), np.zeros((4, 1)))])
    assert lstsq_truncated([]) == []
    lib = _capi.load()
    sh = np.array([3, 2, 1], dtype=np.uint32)
    assert lib.bfhipLstSqTruncated(1, sh.ctypes.data, None, None, None, None, None, None, -1) != 0
