"""The catalogue of the kernel-evaluation tests (tests/helm2_eval_cases.py) is sound before the device is held against it:
conditions on the inputs and on the float64 restatement, not measurements of a kernel."""
import os
import sys

import numpy as np
import pytest

import helm2_eval_cases as cat

# The restatement with the C library's Bessel functions stays within this many error units of the mpmath truth on every
# entry of every case (measured: <= 3.3 on the axis sample, <= 2.0 on the kite).  A case that exceeds it is a badly
# conditioned input and is to be changed; the cap is not.
RESTATEMENT_CAP = 4.0


def test_restatement_is_within_the_cap_on_every_geometry_entry():
    worst = {}
    for name in cat.geom_matrix_names():
        e = cat.geom_err(name, cat.restate(cat.geom_operands(name)))
        worst[name] = float(e.max())
    print({k: round(v, 2) for k, v in worst.items()})
    assert max(worst.values()) <= RESTATEMENT_CAP, worst


@pytest.mark.parametrize("k", cat.AXIS_WAVENUMBERS)
def test_restatement_is_within_the_cap_on_every_axis_argument(k):
    x = cat.fixture()["axis/x"]
    for leaf, (pot, _) in cat.AXIS_LEAVES.items():
        blocks = cat.axis_blocks(leaf, k, cat.restate(cat.axis_operands(leaf, k)))
        signs = cat.axis_dot_signs(leaf)
        primary = signs.index(1.0)
        for name, e in zip(("J", "Y"), cat.axis_errors(blocks[primary], 0 if pot == "S" else 1)):
            assert e.max() <= RESTATEMENT_CAP, (leaf, name, x[int(e.argmax())], float(e.max()))
        for b, s in enumerate(signs):                         # the other directions: the same magnitudes, the sign of n.d
            assert np.array_equal(blocks[b], s * blocks[primary]), (leaf, b)


def test_axis_arguments_are_exact_under_both_wavenumbers():
    x = cat.axis_arguments()
    assert len(x) >= 500 and np.all(np.diff(x) > 0)
    for k in cat.AXIS_WAVENUMBERS:
        pts, _ = cat.axis_problem(k)
        r = np.hypot(pts[1:, 0], pts[1:, 1])
        assert np.array_equal(k * r, np.tile(x, 3))              # hypot and k * r are exact
    dec = cat.axis_decades(x)
    assert dec.min() == -13 and dec.max() == 6 and len(np.unique(dec)) >= 10


def test_self_entries_and_undecorated_zeros_are_exact():
    for name in cat.geom_matrix_names():
        o = cat.geom_operands(name)
        z = cat.restate(o)
        hi, lo, scale, _ = cat.geom_truth(name)
        mask = o["self_mask"]
        if "node_kr" in name or name.endswith("node_plain"):
            assert mask.sum() == 5
            assert o["self_value"] == (cat.GEOM_SELF if "node_kr" in name else 0)      # plain: the self value is 0
        assert np.all(z[mask] == o["self_value"]) and np.all(hi[mask] == o["self_value"]) and np.all(lo[mask] == 0)
        r0 = (o["tx"] == o["sx"]) & (o["ty"] == o["sy"]) & ~mask
        if name.endswith("/z_equiv"):
            assert r0.sum() == 8 and not mask.any()             # check points 24..31 are equivalent sources: decorate = 0
            assert np.all(o["w"] == 1) and np.all(o["f"] == 1)
        if name.endswith("/z_orig"):
            assert not r0.any() and not mask.any() and np.any(o["w"] != 1)
        assert np.all(z[r0] == 0) and np.all(hi[r0] == 0) and np.all(scale[r0] == 0)


def test_kr_tables_sum_to_one_half():
    from oracle import helm2_build as hb
    for p in cat.KR_ORDERS:
        assert len(cat.KR_WEIGHTS[p]) == p
        assert abs(float(np.sum(np.asarray(cat.KR_WEIGHTS[p], dtype=np.longdouble))) - 0.5) <= 1e-11, p
        assert hb.KR_WEIGHTS[p] == cat.KR_WEIGHTS[p]            # the oracle's copy of the tables
    assert abs(sum(cat.KR10_AS_PRINTED) + 4.48) < 0.01            # what the restored table replaces


def test_product_table_matches_the_catalogue():
    """bfKrWeights in bfhip_build.hip, read from the source: the third copy of the tables."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "butterfly_amd", "csrc", "bfhip_build.hip")).read()
    body = re.search(r"bfKrWeights\[18\]\s*=\s*\{([^}]*)\}", src).group(1)
    vals = [float(v) for v in body.replace("\n", " ").split(",")]
    assert vals == cat.KR_WEIGHTS[2] + cat.KR_WEIGHTS[6] + cat.KR_WEIGHTS[10]


@pytest.mark.parametrize("order", cat.KR_ORDERS)
def test_kr_converges_at_its_order_on_the_unit_circle(order):
    errs = [cat.kr_circle_error(n, order) for n in cat.KR_CIRCLE_NS]
    rates = cat.observed_orders(errs)
    print(order, errs, rates)
    assert min(rates) >= order - 1, (errs, rates)


def test_kr_as_printed_by_the_reference_does_not_converge_at_order_ten():
    errs = [cat.kr_circle_error(n, 10, cat.KR10_AS_PRINTED) for n in cat.KR_CIRCLE_NS]
    assert errs[0] > 0.5 and max(cat.observed_orders(errs)) < 2


@pytest.mark.parametrize("order", cat.KR_ORDERS)
def test_kr_factor_count_and_wrap_around(order):
    _, _, orig, _ = cat.geom_curve()
    assert sorted(orig.tolist()) == list(range(cat.GEOM_N)) and not np.array_equal(orig, np.arange(cat.GEOM_N))
    full = cat.kr_factors(order, orig, orig, cat.GEOM_N)
    assert int((full != 1).sum()) == 2 * order * cat.GEOM_N
    # the KR leaf: pairs whose original indices are close only across the wrap 39 -> 0 are met, at every distance
    ot, os_ = orig[slice(*cat.TGT_RANGE)].astype(int), orig[slice(*cat.SRC_RANGE)].astype(int)
    assert set(range(10)) & set(ot) and set(range(30, 40)) & set(os_) and set(range(10)) & set(os_) and set(range(30, 40)) & set(ot)
    plain = np.abs(ot[:, None] - os_[None, :])
    d = np.minimum(plain, cat.GEOM_N - plain)
    wrapped = (d != plain) & (d >= 1) & (d <= order)
    assert wrapped.any()
    f = cat.geom_operands(f"S/node_kr{order}")["f"]
    assert np.all(f[wrapped] != 1) and np.array_equal(f != 1, (d >= 1) & (d <= order))


def test_fixture_inputs_equal_the_catalogue_bit_for_bit():
    fx = cat.fixture()
    assert os.path.getsize(cat.FIXTURE) <= 256 * 1024
    assert np.array_equal(fx["axis/x"], cat.axis_arguments())
    names = cat.geom_matrix_names()
    for name in names:
        o = cat.geom_operands(name)
        for key, arr in cat.matrix_inputs(o).items():
            got = fx[f"{name}/{key}"]
            assert got.dtype == arr.dtype and got.shape == arr.shape and got.tobytes() == arr.tobytes(), (name, key)
        assert fx[f"{name}/hi"].shape == o["f"].shape
        assert max(o["f"].shape) <= 24
    keys = {"axis/x"} | {f"axis/{fn}_{part}" for fn in ("j0", "y0", "j1", "y1") for part in ("hi", "lo")}
    keys |= {f"{name}/{key}" for name in names for key in ("src", "tgt", "nrm", "f", "w", "hi", "lo", "unit")}
    assert set(fx) == keys


def test_fixture_truth_is_reproduced_by_mpmath():
    """Twenty entries recomputed by the generator's own code: bit for bit what the file holds."""
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_helm2_eval_golden as gen
    fx = cat.fixture()
    names = cat.geom_matrix_names()
    for q in range(16):
        name = names[(5 * q) % len(names)]
        o = cat.geom_operands(name)
        m, n = o["f"].shape
        i, j = (3 * q + 1) % m, (7 * q + 2) % n
        z, scale, kr = gen.entry_truth(o, i, j)
        (rh, rl), (ih, il) = gen.split(z.real), gen.split(z.imag)
        assert fx[f"{name}/hi"][i, j] == complex(rh, ih) and fx[f"{name}/lo"][i, j] == np.complex64(complex(rl, il)), (name, i, j)
        assert fx[f"{name}/unit"][0, i, j] == np.float32(float(scale)) and fx[f"{name}/unit"][1, i, j] == np.float32(float(kr))
    x = fx["axis/x"]
    idx = [0, len(x) // 3, len(x) // 2, len(x) - 1]
    truth = gen.axis_truth(x[idx])
    for fn, vals in truth.items():
        for t, (hi, lo) in zip(idx, vals):
            assert fx[f"axis/{fn}_hi"][t] == hi and fx[f"axis/{fn}_lo"][t] == lo, (fn, x[t])
