"""The block-Jacobi test infrastructure checked against itself (no GPU): the catalogue's conditions (tests/bj_catalogue.py),
the fp64 restatement of the inversion kernel against the extended-precision inverse and the bound (tests/bj_ref.py), the wrong
variants the bound and the exact cases must catch, the refusal contract, and the gather cases on plan-only twins."""
import numpy as np
import pytest

import bj_catalogue as cat
import bj_ref
from butterfly_amd import _capi
from butterfly_amd.operator import HipOperator

INV = [(c.name, dt) for c in cat.INVERSION for dt in c.dtypes]
INV_IDS = [f"{n}-{cat.DTYPE_NAMES[dt]}" for n, dt in INV]
ROOM = 1.0 / 8.0
_worst = {}


_out_types = cat.out_types


@pytest.mark.parametrize("name,dtype", INV, ids=INV_IDS)
def test_reference_is_far_inside_the_bound(name, dtype):
    """A condition on the catalogue: the reference's own error (||X|| ||I - B X||) is at most 2^-8 of the bound."""
    for i, (b, _, x, res, g) in enumerate(cat.inv_references(cat.INV_BY_NAME[name], dtype)):
        bnd = bj_ref.bound(b, x, g, cat.WORK_NP[dtype])
        assert g >= 1.0 and bnd.ref_norm * res <= 2.0 ** -8 * bnd.limit, (i, b.shape, res, g, bnd.limit)


@pytest.mark.parametrize("name,dtype", INV, ids=INV_IDS)
def test_restatement_meets_the_bound_with_room(name, dtype):
    case = cat.INV_BY_NAME[name]
    worst = 0.0
    for i, (b, exact, x, res, g) in enumerate(cat.inv_references(case, dtype)):
        r = bj_ref.gje_fp64(b)
        assert r.status == 0 and np.isfinite(r.inverse).all(), (i, r.step)
        assert 0.0 < r.min_pivot_rel <= 1.0
        for out in _out_types(case, dtype):
            got = r.inverse.astype(cat.STORAGE_NP[out])
            ratio = bj_ref.error_ratio(got, x, bj_ref.bound(b, x, g, cat.STORAGE_NP[out]))
            worst = max(worst, ratio)
            assert ratio <= ROOM, (i, b.shape, cat.DTYPE_NAMES[out], ratio)
        if case.exact:
            assert np.array_equal(r.inverse, exact), (i, b.shape)
            # the designed inverse is the inverse: it differs from the reference by the reference's own error at most
            assert bj_ref.error_ratio(exact, x, bj_ref.bound(b, x, g, cat.WORK_NP[dtype])) <= 2.0 ** -8
    _worst[(name, dtype)] = worst
    print(f"bj restatement {name} {cat.DTYPE_NAMES[dtype]}: largest error / bound = {worst:.3g}")


def test_largest_ratio_over_the_catalogue(capsys):
    """The figure quoted in tests/bj_ref.py and DESIGN.md section 13 (computed here when the cases above did not run)."""
    for name, dtype in INV:
        if (name, dtype) not in _worst:
            test_restatement_meets_the_bound_with_room(name, dtype)
    worst = max(_worst.values())
    with capsys.disabled():
        print(f"\nblock-Jacobi restatement: largest error / bound over the catalogue = {worst:.3g} "
              f"(at {max(_worst, key=_worst.get)})")
    assert worst <= ROOM


def test_scaled_cases_are_exact_copies():
    for dt in (cat.C128, cat.F64):
        base = cat.inv_blocks(cat.INV_BY_NAME["scale_base"], dt)
        for name, k in (("scale_up_600", 600), ("scale_down_600", -600)):
            for (b, _), (s, _) in zip(base, cat.inv_blocks(cat.INV_BY_NAME[name], dt)):
                assert np.isfinite(s).all() and np.array_equal(s * 2.0 ** -k, b)
                r0, r1 = bj_ref.gje_fp64(b), bj_ref.gje_fp64(s)
                assert np.array_equal(r1.inverse * 2.0 ** k, r0.inverse)              # the algorithm is equivariant bit for bit


# variant -> (case, element type, what it breaks there)
CAUGHT = {
    "no_pivoting": ("permutations", cat.C128, "refuses"),
    "search_from_row0": ("cond_1e3", cat.F64, "bound"),
    "swap_back_forward": ("permutations", cat.F64, "exact"),
    "jk_not_zeroed": ("dyadic", cat.F64, "exact"),
    "recip_float32": ("cond_1e3", cat.C128, "bound"),
    "update_float32": ("cond_1e3", cat.F64, "bound"),
    "hypot_ties_larger": ("pivot_key_exact", cat.C128, "exact"),
}


@pytest.mark.parametrize("variant", [v for v in bj_ref.VARIANTS if v != "device"])
def test_wrong_variants_are_caught(variant):
    name, dtype, how = CAUGHT[variant]
    refs = cat.inv_references(cat.INV_BY_NAME[name], dtype)
    broken = []
    for i, (b, exact, x, res, g) in enumerate(refs):
        good, bad = bj_ref.gje_fp64(b), bj_ref.gje_fp64(b, variant)
        bnd = bj_ref.bound(b, x, g, cat.WORK_NP[dtype])
        assert good.status == 0 and bj_ref.error_ratio(good.inverse, x, bnd) <= ROOM
        if how == "refuses":
            broken.append(bad.status != 0)
        elif how == "exact":
            assert np.array_equal(good.inverse, exact)
            broken.append(bad.status != 0 or not np.array_equal(bad.inverse, exact))
        else:
            broken.append(bad.status != 0 or bj_ref.error_ratio(bad.inverse, x, bnd) > 1.0)
    assert any(broken), (variant, name)
    print(f"{variant}: caught on {sum(broken)} of {len(broken)} blocks of {name}")


def test_every_variant_has_a_case():
    assert set(CAUGHT) == set(bj_ref.VARIANTS) - {"device"}


@pytest.mark.parametrize("name", [c.name for c in cat.REFUSAL])
def test_refusals_report_the_designed_block_and_step(name):
    case = cat.REF_BY_NAME[name]
    for dt in case.dtypes:
        blocks = [b for b, _ in cat.inv_blocks(case, dt)]
        res, first, step, mpr = bj_ref.gje_blocks(blocks)
        assert (first, step) == (case.block, case.step), (cat.DTYPE_NAMES[dt], first, step)
        assert all(r.status == 0 and np.isfinite(r.inverse).all() for r in res[:first])
        assert res[first].inverse is None and res[first].min_pivot == 0.0


def test_subnormal_pivots_would_pass_the_modulus_test_alone():
    """What the reciprocal test is for: 2^-1074 is finite and non-zero, its reciprocal is not."""
    with np.errstate(over="ignore"):
        assert 0.0 < cat.SUB <= bj_ref.DBL_MAX and np.isinf(np.float64(1.0) / np.float64(cat.SUB))
        assert np.isfinite(cat.HUGE) and np.isinf(np.hypot(cat.HUGE, cat.HUGE))


# ---- gather cases on plan-only twins --------------------------------------------------------------------------------------
GATHER = [(c.name, dt) for c in cat.GATHER for dt in cat.DTYPES]


@pytest.mark.parametrize("name,dtype", GATHER, ids=[f"{n}-{cat.DTYPE_NAMES[dt]}" for n, dt in GATHER])
def test_gather_cases_on_plan_only_twins(name, dtype):
    case = cat.GATHER_BY_NAME[name]
    desc, vals, demote = cat.materialize_gather(case, dtype)
    op = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_PLAN_ONLY, demote_to_f32=demote)
    assert op.dtype == dtype
    n = op.shape[0]
    if case.cuts is None:
        cuts = op.block_jacobi_partition(max_block=case.max_block)
        np.testing.assert_array_equal(cuts, bj_ref.self_leaf_cuts(desc, desc.root, n))
    else:
        cuts = np.asarray(case.cuts)
    expected, uncovered = cat.gather_expected(case, dtype, cuts)
    total, count, mod, covered = cat.direct_dense(desc, vals, dtype)
    got = bj_ref.direct_blocks(op, cuts)
    assert len(got) == len(cuts) - 1
    for (a, b), blk in zip(zip(cuts[:-1], cuts[1:]), got):
        cat.assert_gathered(blk, (total[a:b, a:b], count[a:b, a:b], mod[a:b, a:b]), (name, a, b))
    # uncovered rows: nothing direct on their diagonal, and the expectation the device is held to carries a 1 there
    idx = np.nonzero(~covered)[0]
    assert not np.any(total[idx, idx]) and uncovered == idx.size
    for (a, b), (ref, _, _) in zip(zip(cuts[:-1], cuts[1:]), expected):
        d = np.diagonal(ref)
        assert np.all(d[~covered[a:b]] == 1)
    # the counts the build reports (filled in before the plan-only refusal)
    with pytest.raises(_capi.BfhipError) as e:
        op.block_jacobi(cuts=case.cuts, max_block=case.max_block, invert=False)
    assert e.value.code == 3
    info = e.value.info
    assert (info["numBlocks"], info["maxBlockRows"], info["uncoveredRows"]) == (len(cuts) - 1, int(np.diff(cuts).max()), uncovered)
    if case.product:
        whole = cat.direct_dense(desc, vals, dtype, products=True)[0]
        left_out = [float(np.abs(whole[a:b, a:b] - total[a:b, a:b]).max()) for a, b in zip(cuts[:-1], cuts[1:])]
        assert max(left_out) > 0.05, left_out              # the product has entries inside a block; the direct part leaves them out
    op.close()


def test_wide_first_row_reaches_y_through_a_reduce():
    """The case exists for the tmap path: its forward plan has an item that does not write y and a y-reduce."""
    import ctypes as C
    case = cat.GATHER_BY_NAME["wide_first_row"]
    desc, vals, _ = cat.materialize_gather(case, cat.F64)
    op = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_PLAN_ONLY)
    lib = _capi.load()
    info = _capi.BfhipPlanInfo()
    info.structSize = C.sizeof(info)
    _capi.check(lib.bfhipPlanGetInfo(op.handle, C.byref(info)))
    via_temp = y_reduces = 0
    for s in range(int(info.numStages)):
        sv = _capi.BfhipStageView()
        sv.structSize = C.sizeof(sv)
        _capi.check(lib.bfhipPlanGetStage(op.handle, s, C.byref(sv)))
        items = bj_ref._view(sv.items, int(sv.numItems), _capi.ITEM_DTYPE)
        via_temp += int(np.sum((items["mrFlags"] & bj_ref.BF_ITEM_OUT_Y) == 0))
        for r in range(int(sv.numReduce)):
            rv = _capi.BfhipReduceView()
            rv.structSize = C.sizeof(rv)
            _capi.check(lib.bfhipPlanGetReduce(op.handle, s, r, C.byref(rv)))
            y_reduces += bool(rv.destIsY)
    assert via_temp >= 2 and y_reduces >= 1
    op.close()
