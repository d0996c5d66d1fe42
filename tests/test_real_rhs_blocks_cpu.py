"""bfhipSetRealRhsBlocks without a GPU: the switch of the real element types (F64, F32), the dispatch it changes and the
kernels behind it.

* default: every catalogue case as an F64 and an F32 plan reports the same kernels before and after a round trip of the switch;
* switched on: every forward stage with items is one launch of the block kernel of its element type and tile count
  (72 + 3 (dtype == F32) + tile; tile 0 / 1 / 2 at nrhs <= 16 / <= 32 / more) followed by its unchanged reduce launches; nrhs
  below minRhs, and every transposed stage, are unchanged;
* refusals, the keyword of the constructors, and the second extension range of kernel ids;
* the code objects of the six block kernels: no scratch, no spills, FP64 matrix instructions (fed by exact widening converts
  for F32), no FP32 or reduced-precision matrix instruction, the wavefronts per SIMD each was built for;
* the tight F32 bound of the block path (item sums in double, one rounding per stored level) tells float from double
  accumulation apart, and the catalogue cases it applies to (forward plans without a reduce) are listed here for the GPU test."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from butterfly_amd import _capi
from butterfly_amd import helm2_structure as hs
from butterfly_amd.operator import HipOperator
import kernel_catalogue as kc
from highprec import U32, U64, Reference, _gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = _capi.FLAG_PLAN_ONLY
NRHS = (1, 2, 16, 17, 33, 64, 80)
REDUCE_IDS = set(range(54, 61))
REAL = (kc.F64, kc.F32)
CASE_DTYPES = [(c.name, dt) for c in kc.CASES for dt in REAL]
CASE_IDS = [f"{n}-{kc.DTYPE_NAMES[dt]}" for n, dt in CASE_DTYPES]


def _plan_ops(case, dtype, **kw):
    desc, vals, demote = kc.materialize(case, dtype)
    for flags in kc.flag_sets(case, dtype):
        op = HipOperator.from_desc(desc, vals, flags=PLAN | flags, demote_to_f32=demote, **kw)
        assert op.stats()["dtype"] == dtype
        yield op
        op.close()


def _num_forward_stages(op):
    info = _capi.BfhipPlanInfo()
    info.structSize = C.sizeof(info)
    _capi.check(_capi.load().bfhipPlanGetInfo(op.handle, C.byref(info)))
    return int(info.numStages)


def block_id(dtype, nrhs):
    return 72 + 3 * (dtype == kc.F32) + (0 if nrhs <= 16 else 1 if nrhs <= 32 else 2)


# ---- the tight F32 bound (shared with tests/test_gpu_real_rhs_blocks.py) -----------------------------------------------------
def gamma_tight(ref):
    """The forward bound of an F32 result whose item sums are formed in double and rounded to float once per stored level, with
    no float reduce in between: the complex64 formula of tests/highprec.py without the sqrt(2) and with K for 2K."""
    assert ref.dtype == kc.F32
    return _gamma(2 * (ref.S + 1), U32) + _gamma(ref.K, U64)


def check_tight(ref, y, x):
    """Assert |y - A x| <= gamma_tight |A||x| + tiny componentwise; returns the worst ratio."""
    err = np.abs(np.asarray(y).astype(np.longdouble) - ref.apply(x)).astype(np.longdouble)
    lim = np.longdouble(gamma_tight(ref)) * ref.apply_abs(x) + np.longdouble(ref.tiny())
    worst = float((err / lim).max(initial=0.0))
    assert np.isfinite(np.asarray(y)).all(), "non-finite output"
    assert worst <= 1.0, f"tight bound violated: worst |y - ref| / (gamma_tight |A||x| + tiny) = {worst:.3g} (K = {ref.K}, S = {ref.S}, gamma_tight = {gamma_tight(ref):.3g})"
    return worst


def reduce_free_cases():
    """Names of the catalogue cases whose F32 forward plan at nrhs = 2 launches no reduce kernel (under every flag set)."""
    names = []
    for case in kc.CASES:
        free = True
        for op in _plan_ops(case, kc.F32):
            nf = _num_forward_stages(op)
            free = free and not any(i in REDUCE_IDS for ids in op.stage_kernels(2)[:nf] for i in ids)
        if free:
            names.append(case.name)
    return names


# ---- dispatch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", CASE_DTYPES, ids=CASE_IDS)
def test_default_dispatch_is_untouched(name, dtype):
    for op in _plan_ops(kc.BY_NAME[name], dtype):
        before = {nrhs: op.stage_kernels(nrhs) for nrhs in NRHS}
        for lists in before.values():
            assert all(i < _capi.KERNEL_COUNT for ids in lists for i in ids), lists
        op.set_real_rhs_blocks(2)
        op.set_real_rhs_blocks(0)
        assert {nrhs: op.stage_kernels(nrhs) for nrhs in NRHS} == before


@pytest.mark.parametrize("name,dtype", CASE_DTYPES, ids=CASE_IDS)
def test_switched_on_dispatch(name, dtype):
    for op in _plan_ops(kc.BY_NAME[name], dtype):
        nf = _num_forward_stages(op)
        before = {nrhs: op.stage_kernels(nrhs) for nrhs in NRHS}
        op.set_real_rhs_blocks(2)
        for nrhs in NRHS:
            now = op.stage_kernels(nrhs)
            assert len(now) == len(before[nrhs])
            assert now[nf:] == before[nrhs][nf:], f"nrhs {nrhs}: a transposed stage changed"
            if nrhs == 1:
                assert now == before[nrhs]
                continue
            for s in range(nf):
                old_stage = [i for i in before[nrhs][s] if i not in REDUCE_IDS]
                old_reduce = [i for i in before[nrhs][s] if i in REDUCE_IDS]
                assert before[nrhs][s] == old_stage + old_reduce
                if old_stage:
                    assert now[s] == [block_id(dtype, nrhs)] + old_reduce, (nrhs, s, now[s], before[nrhs][s])
                else:
                    assert now[s] == before[nrhs][s]
        op.set_real_rhs_blocks(17)
        assert op.stage_kernels(16) == before[16]
        assert op.stage_kernels(17)[:nf] != before[17][:nf] or not any(i not in REDUCE_IDS for ids in before[17][:nf] for i in ids)
        assert all(i >= _capi.KERNEL_REAL_EXT_BASE or i in REDUCE_IDS for ids in op.stage_kernels(33)[:nf] for i in ids)


def test_refusals_and_extension_ids():
    lib = _capi.load()
    INVALID, NOT_IMPLEMENTED = 1, 3
    assert lib.bfhipErrorString(INVALID) == b"BF_ERROR_INVALID_ARGUMENTS" and lib.bfhipErrorString(NOT_IMPLEMENTED) == b"BF_ERROR_NOT_IMPLEMENTED"
    assert lib.bfhipSetRealRhsBlocks(None, 2) == INVALID
    case = kc.BY_NAME["forward_both"]
    for dt in REAL:
        for op in _plan_ops(case, dt):
            with pytest.raises(_capi.BfhipError) as e:
                op.set_real_rhs_blocks(1)
            assert e.value.code == INVALID
            op.set_real_rhs_blocks(2)
            op.set_real_rhs_blocks(0xffff)
            op.set_real_rhs_blocks(0)
    for dt in (kc.C128, kc.C64):
        for op in _plan_ops(case, dt):
            with pytest.raises(_capi.BfhipError) as e:
                op.set_real_rhs_blocks(2)
            assert e.value.code == NOT_IMPLEMENTED
            assert "bfhipSetRhsBlocks" in str(e.value) and "complex128" in str(e.value)
    # the keyword of the constructors: True = the recommended minRhs; a refusal closes the operator and raises
    desc, vals, demote = kc.materialize(case, kc.F64)
    op = HipOperator.from_desc(desc, vals, flags=PLAN, real_rhs_blocks=True)
    assert op.stage_kernels(2)[0][0] == 72 and op.stage_kernels(1)[0][0] < _capi.KERNEL_COUNT
    op.close()
    desc, vals, demote = kc.materialize(case, kc.C64)
    with pytest.raises(_capi.BfhipError):
        HipOperator.from_desc(desc, vals, flags=PLAN, demote_to_f32=demote, real_rhs_blocks=2)
    assert (_capi.KERNEL_COUNT, _capi.KERNEL_EXT_BASE, _capi.KERNEL_EXT_END) == (61, 64, 67)
    assert (_capi.KERNEL_REAL_EXT_BASE, _capi.KERNEL_REAL_EXT_END) == (72, 78)
    assert (_capi.KERNEL_F64_MFMA1, _capi.KERNEL_F64_MFMA2, _capi.KERNEL_F64_MFMA4) == (72, 73, 74)
    assert (_capi.KERNEL_F32_MFMA1, _capi.KERNEL_F32_MFMA2, _capi.KERNEL_F32_MFMA4) == (75, 76, 77)
    names = [_capi.kernel_name(i) for i in range(72, 78)]
    assert all(names) and len(set(names)) == 6 and all(n.startswith("bfStageKernelRealMfma<") for n in names)
    assert all("F64" in n for n in names[:3]) and all("F32" in n for n in names[3:])
    assert names[1] == "bfStageKernelRealMfma<F64, 2 tiles>"
    others = {_capi.kernel_name(i) for i in (*range(_capi.KERNEL_COUNT), *range(_capi.KERNEL_EXT_BASE, _capi.KERNEL_EXT_END))}
    assert not set(names) & others
    for i in (67, 68, 69, 70, 71, 78, 1000):
        assert _capi.kernel_name(i) is None, i


# ---- the code objects --------------------------------------------------------------------------------------------------------
def test_block_kernels_use_no_scratch_and_contract_in_double():
    import asm_audit
    asm, usage = asm_audit.device_code_object()
    # template arguments <DT, MAXNT, WAVES>
    mine = {}
    for sym, v in usage.items():
        m = re.match(r"_Z\d+bfStageKernelRealMfmaILi(\d+)ELi(\d+)ELi(\d+)EE", sym)
        if m:
            mine[(int(m.group(1)), int(m.group(2)))] = (sym, int(m.group(3)), v)
    assert sorted(mine) == [(dt, nt) for dt in sorted(REAL) for nt in (1, 2, 4)], sorted(mine)
    for (dt, nt), (sym, waves, v) in mine.items():
        print(sym, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (sym, v)
        body = "\n".join(asm_audit.function_body(asm, sym))
        assert "v_mfma_f64_16x16x4" in body, sym
        assert ("v_cvt_f64_f32" in body) or dt == kc.F64, sym
        assert not re.search(r"v_mfma_f32|v_mfma_\w*(f16|bf16|f8|bf8|i8|xf32)", body), sym
        # the wavefronts per SIMD it was built for: registers (512 per lane of a SIMD) and LDS (160 KiB per CU of 4 SIMDs)
        assert v["Occupancy"] >= waves and (v["VGPRs"] + v.get("AGPRs", 0)) * waves <= 512, (sym, v)
        assert v["LDS Size"] * v["Occupancy"] * 4 <= 160 * 1024, (sym, v)


# ---- the tight F32 bound -----------------------------------------------------------------------------------------------------
def test_tight_f32_bound_tells_float_from_double_accumulation():
    """One F32 leaf of ones, 8 x 1000; x = 1.0 in row 0 and 2^-25 elsewhere: every term but the first is below half an ulp of
    the first in float.  Sequential float accumulation drops all 999 (error 999 x 2^-25 ~ 3e-5 against a bound of ~ 1.2e-7);
    the same sum in double, rounded once, meets the bound."""
    d = hs.Desc(dtype=1)
    d.root = d.add(hs.NODE_DENSE, 8, 1000)
    vals = {d.root: np.ones((8, 1000))}
    ref = Reference(d, vals, kc.F32)
    assert (ref.K, ref.S) == (1000, 0)
    assert gamma_tight(ref) == _gamma(2, U32) + _gamma(1000, U64) and gamma_tight(ref) < ref.gamma() / 400
    x = np.full(1000, 2.0 ** -25)
    x[0] = 1.0
    x = ref.rounded(x)
    a = vals[d.root].astype(np.float32)
    y = np.zeros(8, dtype=np.float32)
    for j in range(1000):                        # sequential float accumulation
        y += a[:, j] * x[j]
    ref.check(y, x)                              # (the float bound of tests/highprec.py accepts it)
    with pytest.raises(AssertionError, match="tight bound violated"):
        check_tight(ref, y, x)
    check_tight(ref, (a.astype(np.float64) @ x.astype(np.float64)).astype(np.float32), x)


def test_catalogue_cases_without_a_forward_reduce():
    """The cases the GPU test holds to the tight bound: expected are the column, diag and forward cases (and whichever random
    graphs have no reduce); the reduce_* and absorb_reduce_33 cases have reduces by construction."""
    names = reduce_free_cases()
    print(len(names), "of", len(kc.CASES), "cases without a forward reduce:", names)
    assert not [n for n in names if n.startswith("reduce_") or n == "absorb_reduce_33"]
    assert len(names) >= 16, (len(names), names)
