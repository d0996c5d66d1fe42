"""bfhipSetRhsBlocks without a GPU: the switch, the dispatch it changes and the kernels behind it.

* default: every catalogue case as a complex64 plan reports only ids below BFHIP_KERNEL_COUNT, before and after a round trip of
  the switch;
* switched on: every forward stage with items is one launch of the block kernel of its tile count (64 / 65 / 66 at nrhs <= 16 /
  <= 32 / more) followed by its unchanged reduce launches; nrhs below minRhs, and every transposed stage, are unchanged;
* refusals, and the extension range of kernel ids;
* the code objects of the three block kernels: no scratch, no spills, FP64 matrix instructions fed by exact widening converts,
  no FP32 matrix instruction."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from butterfly_amd import _capi
from butterfly_amd.operator import HipOperator
import kernel_catalogue as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = _capi.FLAG_PLAN_ONLY
NRHS = (1, 2, 16, 17, 33, 64, 80)
REDUCE_IDS = set(range(54, 61))


def _plan_ops(case, dtype=kc.C64):
    desc, vals, demote = kc.materialize(case, dtype)
    for flags in kc.flag_sets(case, dtype):
        op = HipOperator.from_desc(desc, vals, flags=PLAN | flags, demote_to_f32=demote)
        assert op.stats()["dtype"] == dtype
        yield op
        op.close()


def _num_forward_stages(op):
    info = _capi.BfhipPlanInfo()
    info.structSize = C.sizeof(info)
    _capi.check(_capi.load().bfhipPlanGetInfo(op.handle, C.byref(info)))
    return int(info.numStages)


def _block_id(nrhs):
    return 64 if nrhs <= 16 else 65 if nrhs <= 32 else 66


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_default_dispatch_is_untouched(name):
    for op in _plan_ops(kc.BY_NAME[name]):
        before = {nrhs: op.stage_kernels(nrhs) for nrhs in NRHS}
        for lists in before.values():
            assert all(i < _capi.KERNEL_COUNT for ids in lists for i in ids), lists
        op.set_rhs_blocks(2)
        op.set_rhs_blocks(0)
        assert {nrhs: op.stage_kernels(nrhs) for nrhs in NRHS} == before


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_switched_on_dispatch(name):
    for op in _plan_ops(kc.BY_NAME[name]):
        nf = _num_forward_stages(op)
        before = {nrhs: op.stage_kernels(nrhs) for nrhs in NRHS}
        op.set_rhs_blocks(2)
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
                    assert now[s] == [_block_id(nrhs)] + old_reduce, (nrhs, s, now[s], before[nrhs][s])
                else:
                    assert now[s] == before[nrhs][s]
        op.set_rhs_blocks(17)
        assert op.stage_kernels(16) == before[16]
        assert op.stage_kernels(17)[:nf] != before[17][:nf] or not any(i not in REDUCE_IDS for ids in before[17][:nf] for i in ids)
        assert all(i >= 64 or i in REDUCE_IDS for ids in op.stage_kernels(33)[:nf] for i in ids)


def test_refusals_and_extension_ids():
    lib = _capi.load()
    INVALID, NOT_IMPLEMENTED = 1, 3
    assert lib.bfhipErrorString(INVALID) == b"BF_ERROR_INVALID_ARGUMENTS" and lib.bfhipErrorString(NOT_IMPLEMENTED) == b"BF_ERROR_NOT_IMPLEMENTED"
    assert lib.bfhipSetRhsBlocks(None, 2) == INVALID
    case = kc.BY_NAME["forward_both"]
    for op in _plan_ops(case, kc.C64):
        with pytest.raises(_capi.BfhipError) as e:
            op.set_rhs_blocks(1)
        assert e.value.code == INVALID
        op.set_rhs_blocks(2)
        op.set_rhs_blocks(0xffff)
        op.set_rhs_blocks(0)
    for dt in (kc.C128, kc.F64, kc.F32):
        for op in _plan_ops(case, dt):
            with pytest.raises(_capi.BfhipError) as e:
                op.set_rhs_blocks(2)
            assert e.value.code == NOT_IMPLEMENTED
            assert "complex128" in str(e.value) and "real" in str(e.value)
    # the keyword of the constructors: True = the recommended minRhs; a refusal closes the operator and raises
    desc, vals, demote = kc.materialize(case, kc.C64)
    op = HipOperator.from_desc(desc, vals, flags=PLAN, demote_to_f32=demote, rhs_blocks=True)
    assert op.stage_kernels(2)[0][0] == 64 and op.stage_kernels(1)[0][0] < _capi.KERNEL_COUNT
    op.close()
    desc, vals, demote = kc.materialize(case, kc.F64)
    with pytest.raises(_capi.BfhipError):
        HipOperator.from_desc(desc, vals, flags=PLAN, rhs_blocks=2)
    assert _capi.KERNEL_COUNT == 61
    names = [_capi.kernel_name(i) for i in (64, 65, 66)]
    assert all(names) and len(set(names)) == 3 and all(n.startswith("bfStageKernelC64Mfma") for n in names)
    assert not set(names) & {_capi.kernel_name(i) for i in range(_capi.KERNEL_COUNT)}
    for i in (61, 62, 63, 67, 68, 1000):
        assert _capi.kernel_name(i) is None, i


def test_block_kernels_use_no_scratch_and_contract_in_double():
    import asm_audit
    asm, usage = asm_audit.device_code_object()
    mine = {k: v for k, v in usage.items() if re.match(r"_Z\d+bfStageKernelC64MfmaI", k)}
    assert len(mine) == 3, sorted(mine)
    for sym, v in mine.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (sym, v)
        body = "\n".join(asm_audit.function_body(asm, sym))
        assert "v_mfma_f64_16x16x4" in body and "v_cvt_f64_f32" in body, sym
        assert not re.search(r"v_mfma_f32|v_mfma_\w*(f16|bf16|f8|bf8|i8|xf32)", body), sym
        assert not re.search(r"scratch_|buffer_atomic|global_atomic|flat_atomic|ds_\w*(add|cmpst|inc|dec)", body), sym
    # the 4-tile instantiation leaves room for two wavefronts per SIMD: 512 registers per lane of a SIMD, 160 KiB of LDS per CU
    four = next(v for k, v in mine.items() if "ILi4E" in k)
    assert four["VGPRs"] + four.get("AGPRs", 0) <= 256 and four["Occupancy"] >= 2, four
    assert four["LDS Size"] * 8 <= 160 * 1024, four
