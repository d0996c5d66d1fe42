"""bfhipSetAdjointRhsBlocks without a GPU: the adjoint plan's switch, the dispatch it changes and the kernels behind it.

* default: every catalogue case in all four element types reports the same kernels before and after a round trip of the switch;
* switched on, shared-leaf plan: every transposed stage with items is one launch of bfStageKernelTMfma of its element type and
  tile count (80 + 3 d + tile, d in the order C128, F64, F32, C64; tile 0 / 1 / 2 at nrhs <= 16 / <= 32 / more) followed by its
  unchanged reduce launches; forward stages, nrhs = 1 and nrhs below minRhs are unchanged;
* switched on, packed plan (a forward plan): complex64 stages run ids 64 - 66, F64 / F32 72 - 77, complex128 is unchanged;
* the forward switches and this one do not touch each other's stages; refusals; ids and names; the constructors' keyword;
* the code objects of the twelve kernels: no scratch, no spills, the wavefronts per SIMD each was built for, FP64 matrix
  instructions and no FP32 or reduced-precision ones;
* the tight F32 bound of A^T on the block path (item sums in double, one rounding per stored level) tells float from double
  accumulation apart, and the catalogue cases it applies to (transposed plans without a reduce) are listed for the GPU test."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from butterfly_amd import _capi
from butterfly_amd.operator import HipOperator
import kernel_catalogue as kc
from highprec import U32, U64, Reference, _gamma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = _capi.FLAG_PLAN_ONLY
NRHS = (1, 2, 16, 17, 33, 64, 80)
REDUCE_IDS = set(range(54, 61))
D_INDEX = {kc.C128: 0, kc.F64: 1, kc.F32: 2, kc.C64: 3}
CASE_DTYPES = [(c.name, dt) for c in kc.CASES for dt in kc.DTYPES]
CASE_IDS = [f"{n}-{kc.DTYPE_NAMES[dt]}" for n, dt in CASE_DTYPES]


def _info(op):
    info = _capi.BfhipPlanInfo()
    info.structSize = C.sizeof(info)
    _capi.check(_capi.load().bfhipPlanGetInfo(op.handle, C.byref(info)))
    return info


def _plan_ops(case, dtype, only=None, **kw):
    """(operator, number of forward stages, adjoint plan is packed) per flag set of the case."""
    desc, vals, demote = kc.materialize(case, dtype)
    for flags in kc.flag_sets(case, dtype):
        op = HipOperator.from_desc(desc, vals, flags=PLAN | flags, demote_to_f32=demote, **kw)
        assert op.stats()["dtype"] == dtype
        info = _info(op)
        packed = int(info.reserved) == 1
        assert packed == bool(flags & _capi.FLAG_ADJOINT_PACKED) and int(info.numStagesT) > 0
        if only is None or only == packed:
            yield op, int(info.numStages), packed
        op.close()


def tile(nrhs):
    return 0 if nrhs <= 16 else 1 if nrhs <= 32 else 2


def t_block_id(dtype, nrhs):
    return 80 + 3 * D_INDEX[dtype] + tile(nrhs)


def packed_block_id(dtype, nrhs):
    return {kc.C64: 64, kc.F64: 72, kc.F32: 75}[dtype] + tile(nrhs)


def _split(ids):
    stage = [i for i in ids if i not in REDUCE_IDS]
    reduce = [i for i in ids if i in REDUCE_IDS]
    assert ids == stage + reduce
    return stage, reduce


# ---- the tight F32 bound of A^T (shared with tests/test_gpu_adjoint_rhs_blocks.py) ---------------------------------------------
def gamma_tight_T(ref):
    """The bound of an F32 transposed result whose item sums are formed in double and rounded to float once per stored level,
    with no float reduce in between: gamma_tight of tests/test_real_rhs_blocks_cpu.py with the transposed chain lengths."""
    assert ref.dtype == kc.F32
    return _gamma(2 * (ref.ST + 1), U32) + _gamma(ref.KT, U64)


def check_tight_T(ref, y, x):
    """Assert |y - A^T x| <= gamma_tight_T |A^T||x| + tiny componentwise; returns the worst ratio."""
    err = np.abs(np.asarray(y).astype(np.longdouble) - ref.apply(x, True)).astype(np.longdouble)
    lim = np.longdouble(gamma_tight_T(ref)) * ref.apply_abs(x, True) + np.longdouble(ref.tiny(True))
    worst = float((err / lim).max(initial=0.0))
    assert np.isfinite(np.asarray(y)).all(), "non-finite output"
    assert worst <= 1.0, f"tight bound violated: worst |y - ref| / (gamma_tight_T |A^T||x| + tiny) = {worst:.3g} (KT = {ref.KT}, ST = {ref.ST}, gamma_tight_T = {gamma_tight_T(ref):.3g})"
    return worst


def reduce_free_cases_T():
    """Names of the catalogue cases (with a shared-leaf adjoint) whose F32 transposed plan at nrhs = 2 launches no reduce kernel."""
    names = []
    for case in kc.CASES:
        if "shared" not in case.adjoint:
            continue
        free = True
        for op, nf, _ in _plan_ops(case, kc.F32, only=False):
            free = free and not any(i in REDUCE_IDS for ids in op.stage_kernels(2)[nf:] for i in ids)
        if free:
            names.append(case.name)
    return names


# ---- dispatch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", CASE_DTYPES, ids=CASE_IDS)
def test_default_dispatch_is_untouched(name, dtype):
    for op, nf, packed in _plan_ops(kc.BY_NAME[name], dtype):
        before = {nrhs: op.stage_kernels(nrhs) for nrhs in NRHS}
        for lists in before.values():
            assert all(i < _capi.KERNEL_COUNT for ids in lists for i in ids), lists
        op.set_adjoint_rhs_blocks(2)
        op.set_adjoint_rhs_blocks(0)
        assert {nrhs: op.stage_kernels(nrhs) for nrhs in NRHS} == before


@pytest.mark.parametrize("name,dtype", CASE_DTYPES, ids=CASE_IDS)
def test_switched_on_dispatch(name, dtype):
    for op, nf, packed in _plan_ops(kc.BY_NAME[name], dtype):
        before = {nrhs: op.stage_kernels(nrhs) for nrhs in NRHS}
        op.set_adjoint_rhs_blocks(2)
        block_id = packed_block_id if packed else t_block_id
        changes = not (packed and dtype == kc.C128)          # a packed complex128 adjoint already runs block kernels
        for nrhs in NRHS:
            now = op.stage_kernels(nrhs)
            assert len(now) == len(before[nrhs])
            assert now[:nf] == before[nrhs][:nf], f"nrhs {nrhs}: a forward stage changed"
            if nrhs == 1 or not changes:
                assert now == before[nrhs]
                continue
            for s in range(nf, len(now)):
                old_stage, old_reduce = _split(before[nrhs][s])
                if old_stage:
                    assert now[s] == [block_id(dtype, nrhs)] + old_reduce, (packed, nrhs, s, now[s], before[nrhs][s])
                else:
                    assert now[s] == before[nrhs][s]
        op.set_adjoint_rhs_blocks(17)
        assert op.stage_kernels(16) == before[16]
        has_items = any(_split(ids)[0] for ids in before[17][nf:])
        assert (op.stage_kernels(17)[nf:] != before[17][nf:]) == (changes and has_items)
        if changes:
            lo, hi = (_capi.KERNEL_EXT_BASE, _capi.KERNEL_REAL_EXT_END) if packed else (_capi.KERNEL_T_EXT_BASE, _capi.KERNEL_T_EXT_END)
            assert all(lo <= i < hi or i in REDUCE_IDS for ids in op.stage_kernels(33)[nf:] for i in ids)


@pytest.mark.parametrize("dtype", [kc.F64, kc.F32, kc.C64], ids=["f64", "f32", "c64"])
def test_the_switches_are_independent(dtype):
    for name in ("few_row_with_tall", "randgraph5"):
        for op, nf, packed in _plan_ops(kc.BY_NAME[name], dtype):
            before = {nrhs: op.stage_kernels(nrhs) for nrhs in NRHS}
            forward_switch = op.set_rhs_blocks if dtype == kc.C64 else op.set_real_rhs_blocks
            forward_switch(2)
            fwd_on = {nrhs: op.stage_kernels(nrhs) for nrhs in NRHS}
            for nrhs in NRHS:
                assert fwd_on[nrhs][nf:] == before[nrhs][nf:], "the forward switch changed an adjoint stage"
            assert fwd_on[17][:nf] != before[17][:nf]
            op.set_adjoint_rhs_blocks(2)
            both = {nrhs: op.stage_kernels(nrhs) for nrhs in NRHS}
            for nrhs in NRHS:
                assert both[nrhs][:nf] == fwd_on[nrhs][:nf], "the adjoint switch changed a forward stage"
            assert both[17][nf:] != before[17][nf:]
            forward_switch(0)
            for nrhs in NRHS:
                now = op.stage_kernels(nrhs)
                assert now[:nf] == before[nrhs][:nf] and now[nf:] == both[nrhs][nf:]


def test_refusals_ids_names_and_keyword():
    lib = _capi.load()
    INVALID = 1
    assert lib.bfhipErrorString(INVALID) == b"BF_ERROR_INVALID_ARGUMENTS"
    assert lib.bfhipSetAdjointRhsBlocks(None, 2) == INVALID
    case = kc.BY_NAME["few_row_with_tall"]
    for dt in kc.DTYPES:
        for op, nf, packed in _plan_ops(case, dt):
            with pytest.raises(_capi.BfhipError) as e:
                op.set_adjoint_rhs_blocks(1)
            assert e.value.code == INVALID
            op.set_adjoint_rhs_blocks(2)
            op.set_adjoint_rhs_blocks(0xffff)
            op.set_adjoint_rhs_blocks(0)
        desc, vals, demote = kc.materialize(case, dt)
        op = HipOperator.from_desc(desc, vals, flags=PLAN, demote_to_f32=demote)          # no adjoint plan
        for min_rhs in (0, 2):
            with pytest.raises(_capi.BfhipError) as e:
                op.set_adjoint_rhs_blocks(min_rhs)
            assert e.value.code == INVALID and "adjoint" in str(e.value)
        op.close()
        # the keyword of the constructors: True = the recommended minRhs; a refusal closes the operator and raises
        op = HipOperator.from_desc(desc, vals, flags=PLAN | _capi.FLAG_ADJOINT, demote_to_f32=demote, adjoint_rhs_blocks=True)
        nf = int(_info(op).numStages)
        assert op.stage_kernels(2)[nf][0] == t_block_id(dt, 2) and op.stage_kernels(1)[nf][0] < _capi.KERNEL_COUNT
        op.close()
        with pytest.raises(_capi.BfhipError):
            HipOperator.from_desc(desc, vals, flags=PLAN, demote_to_f32=demote, adjoint_rhs_blocks=2)
    for ctor in (HipOperator.from_desc, HipOperator.from_bfmat, HipOperator.build_helm2, HipOperator.fac_helm2_make_multilevel, HipOperator.load):
        assert "adjoint_rhs_blocks" in inspect.signature(ctor).parameters, ctor
    assert (_capi.KERNEL_COUNT, _capi.KERNEL_T_EXT_BASE, _capi.KERNEL_T_EXT_END) == (61, 80, 92)
    assert (_capi.KERNEL_T_C128_MFMA1, _capi.KERNEL_T_C128_MFMA2, _capi.KERNEL_T_C128_MFMA4) == (80, 81, 82)
    assert (_capi.KERNEL_T_F64_MFMA1, _capi.KERNEL_T_F64_MFMA2, _capi.KERNEL_T_F64_MFMA4) == (83, 84, 85)
    assert (_capi.KERNEL_T_F32_MFMA1, _capi.KERNEL_T_F32_MFMA2, _capi.KERNEL_T_F32_MFMA4) == (86, 87, 88)
    assert (_capi.KERNEL_T_C64_MFMA1, _capi.KERNEL_T_C64_MFMA2, _capi.KERNEL_T_C64_MFMA4) == (89, 90, 91)
    names = [_capi.kernel_name(i) for i in range(80, 92)]
    assert all(names) and len(set(names)) == 12 and all(n.startswith("bfStageKernelTMfma<") for n in names)
    for d, tag in enumerate(("C128", "F64", "F32", "C64")):
        assert all(tag + "," in n for n in names[3 * d:3 * d + 3]), names
    assert names[4] == "bfStageKernelTMfma<F64, 2 tiles>"
    others = {_capi.kernel_name(i) for i in (*range(_capi.KERNEL_COUNT), *range(_capi.KERNEL_EXT_BASE, _capi.KERNEL_EXT_END),
                                             *range(_capi.KERNEL_REAL_EXT_BASE, _capi.KERNEL_REAL_EXT_END))}
    assert not set(names) & others
    for i in (78, 79, 92, 1000):
        assert _capi.kernel_name(i) is None, i


# ---- the code objects --------------------------------------------------------------------------------------------------------
def test_block_kernels_use_no_scratch_and_contract_in_double():
    import asm_audit
    asm, usage = asm_audit.device_code_object()
    # template arguments <DT, MAXNT, WAVES>
    mine = {}
    for sym, v in usage.items():
        m = re.match(r"_Z\d+bfStageKernelTMfmaILi(\d+)ELi(\d+)ELi(\d+)EE", sym)
        if m:
            mine[(int(m.group(1)), int(m.group(2)))] = (sym, int(m.group(3)), v)
    assert sorted(mine) == [(dt, nt) for dt in sorted(kc.DTYPES) for nt in (1, 2, 4)], sorted(mine)
    for (dt, nt), (sym, waves, v) in mine.items():
        print(sym, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (sym, v)
        body = "\n".join(asm_audit.function_body(asm, sym))
        assert "v_mfma_f64_16x16x4" in body, sym
        assert not re.search(r"v_mfma_f32|v_mfma_\w*(f16|bf16|f8|bf8|i8|xf32)", body), sym
        # the wavefronts per SIMD it was built for: registers (512 per lane of a SIMD) and LDS (160 KiB per CU of 4 SIMDs)
        assert v["Occupancy"] >= waves and (v["VGPRs"] + v.get("AGPRs", 0)) * waves <= 512, (sym, v)
        assert v["LDS Size"] * v["Occupancy"] * 4 <= 160 * 1024, (sym, v)


# ---- the tight F32 bound -----------------------------------------------------------------------------------------------------
def _run_transposed(op, x, acc_dtype):
    """The shared-leaf transposed plan of an F32 plan-only operator in numpy, step by step, with accumulators (and reduce
    sums) of `acc_dtype`; every stored value is rounded to float.  The semantics are those of tests/plan_emulator.py."""
    from plan_emulator import _view, BF_ITEM_OUT_Y, BF_PIECE_IN_X, BF_PIECE_IDENTITY, BF_PIECE_ROWMAJOR
    lib = _capi.load()
    info = _info(op)
    assert info.dtype == kc.F32 and int(info.reserved) == 0 and int(info.numStagesT) > 0
    arena = np.zeros(int(info.arenaElems), dtype=np.float32)
    _capi.check(lib.bfhipPlanPackArena(op.handle, arena.ctypes.data))
    x = np.asarray(x, dtype=np.float32)
    nrhs = x.shape[1]
    y = np.full((int(info.numCols), nrhs), np.nan, dtype=np.float32)
    temp = np.full((int(max(info.tempElems, info.tempElemsT)), nrhs), np.nan, dtype=np.float32)
    for s in range(int(info.numStages), int(info.numStages) + int(info.numStagesT)):
        sv = _capi.BfhipStageView()
        sv.structSize = C.sizeof(sv)
        _capi.check(lib.bfhipPlanGetStage(op.handle, s, C.byref(sv)))
        items = _view(sv.items, int(sv.numItems), _capi.ITEM_DTYPE)
        pieces = _view(sv.pieces, int(sv.numPieces), _capi.PIECE_DTYPE)
        for it in items:
            mr = int(it["mrFlags"]) & 0xFFFF
            acc = np.zeros((mr, nrhs), dtype=acc_dtype)
            for pc in pieces[int(it["pieceBegin"]):int(it["pieceBegin"]) + int(it["numPieces"])]:
                src = x if (int(pc["flags"]) & BF_PIECE_IN_X) else temp
                io, n, d0, ld = int(pc["inOff"]), int(pc["ncols"]), int(pc["dataOff"]), int(pc["ld"])
                if int(pc["flags"]) & BF_PIECE_IDENTITY:
                    acc += src[io:io + mr].astype(acc_dtype)
                    continue
                for st in range(n):
                    col = arena[d0 + st * ld + np.arange(mr)] if int(pc["flags"]) & BF_PIECE_ROWMAJOR else arena[d0 + np.arange(mr) * ld + st]
                    acc += col.astype(acc_dtype)[:, None] * src[io + st].astype(acc_dtype)[None, :]
            dst = y if (int(it["mrFlags"]) & BF_ITEM_OUT_Y) else temp
            dst[int(it["outOff"]):int(it["outOff"]) + mr] = acc.astype(np.float32)
        for r in range(int(sv.numReduce)):
            rv = _capi.BfhipReduceView()
            rv.structSize = C.sizeof(rv)
            _capi.check(lib.bfhipPlanGetReduce(op.handle, s, r, C.byref(rv)))
            row_iv = _view(rv.rowInterval, int(rv.numRows), np.dtype("<u4"))
            iv_begin = _view(rv.ivBegin, int(rv.numIntervals) + 1, np.dtype("<u4"))
            bias = _view(rv.srcBias, int(rv.numSrc), np.dtype("<i8"))
            dest = y if rv.destIsY else temp[int(rv.destOff):]
            for row in range(int(rv.numRows)):
                if row_iv[row] == 0xFFFFFFFF:
                    continue
                out = np.zeros(nrhs, dtype=acc_dtype)
                for k in range(int(iv_begin[row_iv[row]]), int(iv_begin[row_iv[row] + 1])):
                    out += temp[int(bias[k]) + row].astype(acc_dtype)
                dest[row] = out.astype(np.float32)
    return y


def test_tight_f32_bound_tells_float_from_double_accumulation():
    """absorb_chain_70 as an F32 operand: 70 leaves of ones, 8 x 64, stacked; x = 1.0 in row 0 and 2^-25 elsewhere.  Every
    output of A^T x is 1 + 559 x 2^-25.  A float accumulator that has taken the 1.0 in drops every other term (error ~ 1.7e-5
    against a bound of ~ 1.2e-7); the same sums in double, rounded once, meet the bound."""
    case = kc.BY_NAME["absorb_chain_70"]
    desc, vals, demote = kc.materialize(case, kc.F32)
    ref = Reference(desc, vals, kc.F32)
    assert (ref.KT, ref.ST) == (77, 0)               # a leaf's 8 rows, then the 70 leaves of the block column
    assert gamma_tight_T(ref) == _gamma(2, U32) + _gamma(77, U64) and gamma_tight_T(ref) < ref.gamma(True) / 30
    op = HipOperator.from_desc(desc, vals, flags=PLAN | _capi.FLAG_ADJOINT, demote_to_f32=demote)
    x = ref.rounded(kc.draw_x(case, kc.F32, op.shape[0], 2, np.random.default_rng(0)))
    y32 = _run_transposed(op, x, np.float32)
    with pytest.raises(AssertionError, match="tight bound violated"):
        check_tight_T(ref, y32, x)
    check_tight_T(ref, _run_transposed(op, x, np.float64), x)
    op.close()


def test_catalogue_cases_without_a_transposed_reduce():
    """The cases the GPU test holds to the tight bound: a block column's transposed plan is one item chain per column group,
    so the plain column cases (tall_column_*, coop_chain_97, absorb_chain_70) are expected among them."""
    names = reduce_free_cases_T()
    print(len(names), "of", len(kc.CASES), "cases without a transposed reduce:", names)
    assert "absorb_chain_70" in names and "tall_column_w17" in names and "coop_chain_97" in names, names
    assert len(names) >= 12, (len(names), names)
