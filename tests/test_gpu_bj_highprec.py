"""The block-Jacobi kernels (bfhip_precond.hip) on designed blocks: the gather against the direct-part rule, the inversion
against an extended-precision inverse with the derived bound of tests/bj_ref.py (the same function and constants as
tests/test_bj_highprec_cpu.py), the exact cases bit for bit, demotion, scaling, determinism, and the refusal contract.

Every operand is built once per (case, element type, result type) and kept for the module; results are read back with
panels of ONE unit vector, so that an extracted entry is the stored entry (the complex128 matrix-core kernels that serve
wider panels form complex products with three multiplications and would round it).  A refusal is a host-side status: no
case here makes the device fault."""
import ctypes as C
import time

import numpy as np
import pytest

import bj_catalogue as cat
import bj_ref
import highprec
from butterfly_amd import _capi
from butterfly_amd.operator import HipOperator

pytestmark = pytest.mark.gpu

INV = [(c.name, dt) for c in cat.INVERSION for dt in c.dtypes]
INV_IDS = [f"{n}-{cat.DTYPE_NAMES[dt]}" for n, dt in INV]
_T0 = time.time()
_ratio = {}         # result element type -> largest error / bound


_out_types = cat.out_types


def _read(pre):
    return pre.extract(device=False, panel=1)


@pytest.fixture(scope="module")
def builds():
    """(case name, source type, result type) -> (preconditioner, its dense matrix, info, cuts): one build each."""
    cache, ops = {}, []

    def get(name, src, out):
        key = (name, src, out)
        if key not in cache:
            blocks = [b for b, _ in cat.inv_blocks(cat.INV_BY_NAME[name], src)]
            desc, vals, demote, cuts = cat.block_diag_operand(blocks, src)
            op = HipOperator.from_desc(desc, vals, demote_to_f32=demote)
            assert op.dtype == src
            pre, info = op.block_jacobi(max_block=256, dtype=None if out == src else out)
            assert pre.dtype == out and pre.shape == op.shape
            ops.extend([op, pre])
            cache[key] = (pre, _read(pre), info, cuts)
        return cache[key]

    yield get
    for o in ops:
        o.close()


def _blocks_of(dense, cuts):
    mask = np.zeros(dense.shape, dtype=bool)
    for a, b in zip(cuts[:-1], cuts[1:]):
        mask[a:b, a:b] = True
    assert not np.any(dense[~mask]), "non-zero outside the diagonal blocks"
    return [dense[a:b, a:b] for a, b in zip(cuts[:-1], cuts[1:])]


FEW_ULP = 8 * np.finfo(np.float64).eps


def _pivot_tolerance(case, ref):
    """Relative tolerance of a block's smallest pivot modulus against the restatement's.  Where the elimination is exact (the
    exact cases) the two differ by hypot's rounding alone: a few ulp.  Elsewhere a pivot is a COMPUTED entry of the reduced
    block, and the device (which contracts a - f r into fused multiply-adds) and numpy (which cannot) round it differently:
    each carries the elimination's relative perturbation, which the analysis behind bj_ref.bound puts at
    C(m) u64 g kappa_inf(B) for an entry of size |B| / kappa and above.  Measured on an MI355X the two differ by 1e-14
    (kappa 1e3), 2e-11 (1e6) and 1e-7 (1e10) relative: rounding amplified by kappa, not a few ulp."""
    b, exact, x, res, g = ref
    if case.exact:
        return FEW_ULP
    kappa = float(np.abs(b).sum(axis=1).max() * np.abs(x).sum(axis=1).max())
    return FEW_ULP + bj_ref.c_of_m(b.shape[0], np.iscomplexobj(b)) * bj_ref.U64 * g * kappa


@pytest.mark.parametrize("name,src", INV, ids=INV_IDS)
def test_inverses_meet_the_bound(builds, name, src):
    case = cat.INV_BY_NAME[name]
    refs = cat.inv_references(case, src)
    _, _, _, mpr_ref = bj_ref.gje_blocks([r[0] for r in refs])
    mpr_tol = max(_pivot_tolerance(case, r) for r in refs)
    full = None
    for out in _out_types(case, src):
        pre, dense, info, cuts = builds(name, src, out)
        assert np.isfinite(dense).all()
        assert info["firstSingularBlock"] == -1 and info["numBlocks"] == len(refs) and info["uncoveredRows"] == 0
        assert info["maxBlockRows"] == max(r[0].shape[0] for r in refs)
        assert 0.0 < info["minPivotRel"] <= 1.0 and abs(info["minPivotRel"] - mpr_ref) <= mpr_tol * mpr_ref, (info["minPivotRel"], mpr_ref, mpr_tol)
        worst = 0.0
        for i, (got, (b, exact, x, res, g)) in enumerate(zip(_blocks_of(dense, cuts), refs)):
            ratio = bj_ref.error_ratio(got.astype(cat.STORAGE_NP[out]), x, bj_ref.bound(b, x, g, cat.STORAGE_NP[out]))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (i, b.shape, cat.DTYPE_NAMES[out], ratio)
            if case.exact:
                assert np.array_equal(got, exact.astype(cat.STORAGE_NP[out]).astype(got.dtype)), (i, b.shape, cat.DTYPE_NAMES[out])
        print(f"bj device {name} {cat.DTYPE_NAMES[src]} -> {cat.DTYPE_NAMES[out]}: largest error / bound = {worst:.3g}")
        _ratio[out] = max(_ratio.get(out, 0.0), worst)
        if out == src:
            full = dense
        else:
            # the working copy is shared and the fill rounds once: the demoted result is the full one rounded
            assert np.array_equal(dense, full.astype(cat.STORAGE_NP[out]).astype(dense.dtype)), cat.DTYPE_NAMES[out]


@pytest.mark.parametrize("src", [cat.C128, cat.F64], ids=["c128", "f64"])
def test_power_of_two_scaling_is_exact(builds, src):
    _, base, info0, _ = builds("scale_base", src, src)
    for name, k in (("scale_up_600", 600), ("scale_down_600", -600)):
        _, dense, info, _ = builds(name, src, src)
        assert np.array_equal(dense * 2.0 ** k, base), name
        assert abs(info["minPivotRel"] - info0["minPivotRel"]) <= FEW_ULP * info0["minPivotRel"]      # the same arithmetic, scaled


@pytest.mark.parametrize("name,src,out", [("cond_1e6", cat.C128, cat.C128), ("permutations", cat.F64, cat.F32), ("growth", cat.C64, cat.C64)],
                         ids=["cond_1e6-c128", "permutations-f64-f32", "growth-c64"])
def test_a_second_build_is_bit_identical(builds, name, src, out):
    _, first, info0, _ = builds(name, src, out)
    blocks = [b for b, _ in cat.inv_blocks(cat.INV_BY_NAME[name], src)]
    desc, vals, demote, _ = cat.block_diag_operand(blocks, src)
    op = HipOperator.from_desc(desc, vals, demote_to_f32=demote)
    pre, info = op.block_jacobi(max_block=256, dtype=None if out == src else out)
    assert np.array_equal(_read(pre), first) and info["minPivotRel"] == info0["minPivotRel"]
    pre.close(); op.close()


@pytest.mark.parametrize("src", cat.DTYPES, ids=[cat.DTYPE_NAMES[d] for d in cat.DTYPES])
def test_apply_meets_the_apply_bound_of_the_extracted_blocks(builds, src):
    rng = np.random.default_rng(70 + src)
    case = cat.INV_BY_NAME["cond_1e3"]
    for out in _out_types(case, src):
        pre, dense, _, cuts = builds("cond_1e3", src, out)
        desc, vals, _, _ = cat.block_diag_operand(_blocks_of(dense, cuts), out)
        ref = highprec.Reference(desc, vals, out)
        n = dense.shape[0]
        for nrhs in (1, 3):
            x = rng.standard_normal((n, nrhs))
            if cat.is_complex(out):
                x = x + 1j * rng.standard_normal((n, nrhs))
            ref.check(pre.apply_host(x), x)


def _refused(op, max_block=256, invert=True):
    """bfhipBlockJacobi called directly: (status, handle, info, message)."""
    lib = _capi.load()
    o = _capi.BfhipBlockJacobiOptions()
    o.structSize = C.sizeof(o)
    o.flags = 0 if invert else _capi.BFHIP_BJ_NO_INVERT
    o.maxBlock = max_block
    o.device = -1
    info = _capi.BfhipBlockJacobiInfo()
    info.structSize = C.sizeof(info)
    h = C.c_void_p()
    rc = lib.bfhipBlockJacobi(op.handle, C.byref(o), C.byref(h), C.byref(info))
    return rc, h, info.as_dict(), lib.bfhipLastErrorMessage().decode() if rc else ""


@pytest.mark.parametrize("name", [c.name for c in cat.REFUSAL])
def test_refusals(name):
    """Fails without the reciprocal / scaled-row tests of bfBjInvertKernel on subnormal_1x1, subnormal_inside,
    subnormal_complex and scaled_row_overflow: those builds then succeed with infinities in the preconditioner."""
    case = cat.REF_BY_NAME[name]
    for dt in case.dtypes:
        blocks = [b for b, _ in cat.inv_blocks(case, dt)]
        desc, vals, demote, cuts = cat.block_diag_operand(blocks, dt)
        op = HipOperator.from_desc(desc, vals, demote_to_f32=demote)
        rc, h, info, msg = _refused(op)
        if h.value:
            HipOperator(h.value).close()
        assert rc == 2 and not h.value, (cat.DTYPE_NAMES[dt], rc, msg)                    # RUNTIME_ERROR and no operator
        assert info["firstSingularBlock"] == case.block, (cat.DTYPE_NAMES[dt], info, msg)
        assert f"block {case.block} (rows {cuts[case.block]}..{cuts[case.block + 1]})" in msg and msg.endswith(f"at step {case.step}"), msg
        # the blocks themselves are gathered all the same
        pre, info = op.block_jacobi(max_block=256, invert=False)
        assert info["firstSingularBlock"] == -1 and info["numBlocks"] == len(blocks)
        if all(np.isfinite(b).all() for b in blocks):
            for got, b in zip(_blocks_of(_read(pre), cuts), blocks):
                assert np.array_equal(got, b)
        pre.close(); op.close()


GATHER = [(c.name, dt) for c in cat.GATHER for dt in cat.DTYPES]


@pytest.mark.parametrize("name,dtype", GATHER, ids=[f"{n}-{cat.DTYPE_NAMES[dt]}" for n, dt in GATHER])
def test_gathered_blocks(name, dtype):
    case = cat.GATHER_BY_NAME[name]
    desc, vals, demote = cat.materialize_gather(case, dtype)
    op = HipOperator.from_desc(desc, vals, demote_to_f32=demote)
    twin = HipOperator.from_desc(desc, vals, demote_to_f32=demote, flags=_capi.FLAG_PLAN_ONLY)
    cuts = twin.block_jacobi_partition(max_block=case.max_block) if case.cuts is None else np.asarray(case.cuts)
    expected, uncovered = cat.gather_expected(case, dtype, cuts)
    pre, info = op.block_jacobi(cuts=case.cuts, max_block=case.max_block, invert=False)
    assert pre.dtype == dtype and pre.shape == op.shape
    assert (info["numBlocks"], info["maxBlockRows"], info["uncoveredRows"]) == (len(cuts) - 1, int(np.diff(cuts).max()), uncovered)
    got = _blocks_of(_read(pre), cuts)
    covered = cat.direct_dense(desc, vals, dtype)[3]
    for i, (blk, exp, rule) in enumerate(zip(got, expected, bj_ref.direct_blocks(twin, cuts))):
        cat.assert_gathered(blk, exp, (name, i), out_dtype=dtype)
        # and against the rule restated over the twin's plan, which leaves out the 1s of uncovered rows
        idx = np.nonzero(~covered[cuts[i]:cuts[i + 1]])[0]
        rule = rule.copy()
        rule[idx, idx] += 1
        one = exp[1] <= 1
        assert np.array_equal(blk[one], rule[one]), (name, i)
    pre.close(); twin.close(); op.close()


def test_report(capsys):
    """The figures the change's description quotes (run last: file order)."""
    with capsys.disabled():
        print("\nblock-Jacobi device inverses, largest error / bound per result type: "
              + ", ".join(f"{cat.DTYPE_NAMES[k]} {v:.3g}" for k, v in sorted(_ratio.items()))
              + f"; wall time of this file so far {time.time() - _T0:.1f} s")
    assert all(v <= 1.0 for v in _ratio.values())
