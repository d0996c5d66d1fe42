"""Complex64 operators (BFHIP_C64: demoteToF32 on a complex128 operand) without a GPU.

A complex64 element is 8 bytes like an F64 one, so a C64 operator must get exactly the plan of the F64 operator of the same
structure -- items, pieces, reduce tables, arena and vector sizes -- and an arena that holds each component of the
complex128 value rounded once to float."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from butterfly_amd import _capi, helm2_structure as hs
from butterfly_amd.operator import HipOperator
from oracle import helm2_build as hb
import randgraph
from test_decorations import decorated_complex_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = _capi.FLAG_PLAN_ONLY
WIDE = 1


def _info(op):
    info = _capi.BfhipPlanInfo()
    info.structSize = C.sizeof(info)
    _capi.check(_capi.load().bfhipPlanGetInfo(op.handle, C.byref(info)))
    return info


def _bytes(ptr, n):
    return bytes((C.c_char * n).from_address(ptr)) if n else b""


def _plan_tables(op):
    """Everything of the flattened plan that is not a value: per stage (forward and adjoint) items, pieces, reduce views."""
    lib = _capi.load()
    info = _info(op)
    out = [int(info.numStages), int(info.numStagesT), int(info.arenaElems), int(info.tempElems), int(info.arenaElemsT),
           int(info.tempElemsT), int(info.reserved)]
    for s in range(int(info.numStages) + int(info.numStagesT)):
        sv = _capi.BfhipStageView()
        sv.structSize = C.sizeof(sv)
        _capi.check(lib.bfhipPlanGetStage(op.handle, s, C.byref(sv)))
        out += [_bytes(sv.items, int(sv.numItems) * 16), _bytes(sv.pieces, int(sv.numPieces) * 24), int(sv.numReduce)]
        for r in range(int(sv.numReduce)):
            rv = _capi.BfhipReduceView()
            rv.structSize = C.sizeof(rv)
            _capi.check(lib.bfhipPlanGetReduce(op.handle, s, r, C.byref(rv)))
            out += [int(rv.destIsY), int(rv.destOff), int(rv.numRows), int(rv.numIntervals), int(rv.numSrc),
                    _bytes(rv.rowInterval, int(rv.numRows) * 4), _bytes(rv.ivBegin, (int(rv.numIntervals) + 1) * 4),
                    _bytes(rv.srcBias, int(rv.numSrc) * 8)]
    return out


def _item_flags(op):
    lib = _capi.load()
    info = _info(op)
    flags = 0
    for s in range(int(info.numStages) + int(info.numStagesT)):
        sv = _capi.BfhipStageView()
        sv.structSize = C.sizeof(sv)
        _capi.check(lib.bfhipPlanGetStage(op.handle, s, C.byref(sv)))
        items = np.frombuffer(_bytes(sv.items, int(sv.numItems) * 16), dtype=_capi.ITEM_DTYPE)
        flags |= int(np.bitwise_or.reduce(items["mrFlags"] & 0xFFFF0000)) if len(items) else 0
        if s >= int(info.numStages) and len(items) and (items["mrFlags"] & 0xFFFF).max() > 16:
            flags |= WIDE    # a transposed item of more than 16 columns: the 4-row-lane (wide) tiling
    return flags


def _arenas(op):
    info = _info(op)
    lib = _capi.load()
    dt = {0: np.complex128, 1: np.float64, 2: np.float32, 3: np.complex64}[int(info.dtype)]
    a = np.zeros(int(info.arenaElems), dtype=dt)
    _capi.check(lib.bfhipPlanPackArena(op.handle, a.ctypes.data))
    t = None
    if int(info.reserved) == 1:       # packed adjoint
        t = np.zeros(int(info.arenaElemsT), dtype=dt)
        _capi.check(lib.bfhipPlanPackArenaT(op.handle, t.ctypes.data))
    return a, t


def _real_twin(desc):
    """The same structure as an F64 descriptor (nodes are shared; only the element type differs)."""
    twin = hs.Desc(dtype=1)
    for k in range(len(desc.kind)):
        twin.add(desc.kind[k], desc.rows[k], desc.cols[k], list(desc.children[k]), desc.block_kind[k])
    twin.root = desc.root
    twin.top_row_block = desc.top_row_block
    return twin


def _complexify(rng, desc, vals):
    d = hs.Desc(dtype=0)
    for k in range(len(desc.kind)):
        d.add(desc.kind[k], desc.rows[k], desc.cols[k], list(desc.children[k]), desc.block_kind[k])
    d.root = desc.root
    return d, {k: v + 1j * rng.standard_normal(v.shape) for k, v in vals.items()}


def _cases():
    rng = np.random.default_rng(64)
    n, k = 2048, 128
    pts = hs.circle_points(n)
    desc, _, perm = hs.helm2_multilevel_structure(pts, k, recipes=True)
    yield "helm2_multilevel_n2048_k128", desc, hb.leaf_values(desc, k, pts[perm])
    for seed in range(3):
        d, v = randgraph.random_operand(np.random.default_rng(300 + seed), depth=4, cplx=True)
        yield f"randgraph{seed}", d, v
    d, v, _ = randgraph.few_row_operand(rng)
    yield ("few_row",) + _complexify(rng, d, v)
    d, v, _ = randgraph.narrow_items_operand(rng)
    yield ("narrow_items",) + _complexify(rng, d, v)
    d, v, _ = randgraph.few_row_column_operand(rng, 40, 2100)
    yield ("wide_tall_column",) + _complexify(rng, d, v)
    d, v, _, _ = randgraph.long_contraction_operand(rng, 0)
    yield "long_contraction", d, v


CASES = list(_cases())


@pytest.mark.parametrize("adjoint", [_capi.FLAG_ADJOINT, _capi.FLAG_ADJOINT_PACKED])
@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_c64_plan_equals_the_f64_plan_and_arena_rounds_once(case, adjoint):
    name, desc, vals = CASES[case]
    op = HipOperator.from_desc(desc, vals, flags=PLAN | adjoint, demote_to_f32=True)
    info = _info(op)
    assert (int(info.dtype), int(info.elemSize), int(info.epl)) == (_capi.BFHIP_C64, 8, 2)
    assert op.stats()["dtype"] == _capi.BFHIP_C64
    twin = _real_twin(desc)
    re_vals = {k: np.ascontiguousarray(v.real) for k, v in vals.items()}
    im_vals = {k: np.ascontiguousarray(v.imag) for k, v in vals.items()}
    op_re = HipOperator.from_desc(twin, re_vals, flags=PLAN | adjoint)
    op_im = HipOperator.from_desc(twin, im_vals, flags=PLAN | adjoint)
    assert _plan_tables(op) == _plan_tables(op_re)
    a, t = _arenas(op)
    a_re, t_re = _arenas(op_re)
    a_im, t_im = _arenas(op_im)
    np.testing.assert_array_equal(a.view(np.float32), (a_re + 1j * a_im).astype(np.complex64).view(np.float32))
    if t is not None:
        np.testing.assert_array_equal(t.view(np.float32), (t_re + 1j * t_im).astype(np.complex64).view(np.float32))
    for o in (op, op_re, op_im):
        o.close()


def test_the_cases_cover_every_item_class():
    flags = 0
    for _, desc, vals in CASES:
        op = HipOperator.from_desc(desc, vals, flags=PLAN | _capi.FLAG_ADJOINT, demote_to_f32=True)
        flags |= _item_flags(op)
        op.close()
    from plan_emulator import BF_ITEM_MERGED, BF_ITEM_ROWMAJOR, BF_ITEM_SMALL, BF_ITEM_TNARROW
    for f in (BF_ITEM_ROWMAJOR, BF_ITEM_MERGED, BF_ITEM_SMALL, BF_ITEM_TNARROW, WIDE):
        assert flags & f, hex(f)


def _synthetic_values(desc, seed):
    """The complex128 values the engine synthesizes for `seed`: leaf i's element (r, c) is stream entry base_i + r * cols + c,
    base_i = the elements of the dense leaves before it, scaled by sqrt(3 / (2 cols))."""
    lib = _capi.load()
    vals, base = {}, 0
    for k in range(len(desc.kind)):
        if desc.kind[k] != hs.NODE_DENSE:
            continue
        m, n = desc.rows[k], desc.cols[k]
        idx = base + np.arange(m * n, dtype=np.uint64)
        re = np.array([lib.bfhipSyntheticValue(seed, int(i), 0) for i in idx])
        im = np.array([lib.bfhipSyntheticValue(seed, int(i), 1) for i in idx])
        vals[k] = ((re + 1j * im) * np.sqrt(3.0 / (2.0 * n))).reshape(m, n)
        base += m * n
    return vals


def test_synthetic_c64_leaves_are_the_rounded_c128_values():
    desc, _ = randgraph.random_operand(np.random.default_rng(77), depth=3, cplx=True)
    host = _synthetic_values(desc, 1234)
    c128_syn = _arenas(HipOperator.from_desc(desc, None, seed=1234, flags=PLAN))[0]
    c128_host = _arenas(HipOperator.from_desc(desc, host, flags=PLAN))[0]
    np.testing.assert_array_equal(c128_syn, c128_host)           # the values above are the synthetic operand's
    for flags in (PLAN, PLAN | _capi.FLAG_ADJOINT_PACKED):
        syn = _arenas(HipOperator.from_desc(desc, None, seed=1234, flags=flags, demote_to_f32=True))
        hst = _arenas(HipOperator.from_desc(desc, host, flags=flags, demote_to_f32=True))
        for a, b in zip(syn, hst):
            if a is not None:
                np.testing.assert_array_equal(a.view(np.float32), b.view(np.float32))


def test_decorations_are_added_in_double_then_rounded_once():
    G, dense = decorated_complex_graph(np.random.default_rng(3))
    op = HipOperator.from_bfmat(G.ptr.value, flags=PLAN, demote_to_f32=True)
    op128 = HipOperator.from_bfmat(G.ptr.value, flags=PLAN)
    a, _ = _arenas(op)
    a128, _ = _arenas(op128)
    # the complex128 plan lays the leaves out differently: the same values, each component rounded once from the double sum
    np.testing.assert_array_equal(np.sort(a[a != 0]), np.sort(a128[a128 != 0].astype(np.complex64)))


def test_helm2_builders_refuse_complex64():
    n, k = 1024, 64.0
    pts = hs.circle_points(n)
    desc, _, perm = hs.helm2_multilevel_structure(pts, k, recipes=True)
    with pytest.raises(_capi.BfhipError) as e:
        HipOperator.build_helm2(desc, pts[perm], 2 * np.pi * k, demote_to_f32=True)
    assert e.value.code == 3 and "complex64" in str(e.value)
    with pytest.raises(_capi.BfhipError) as e:
        HipOperator.fac_helm2_make_multilevel(pts, 2 * np.pi * k, demote_to_f32=True)
    assert e.value.code == 3 and "complex64" in str(e.value)


def test_c64_kernels_use_no_scratch_and_spill_nothing():
    import asm_audit
    _, usage = asm_audit.device_code_object()
    c64 = {k: v for k, v in usage.items() if "ILi3E" in k or "bfReduceKernelIfLi2E" in k}
    names = " ".join(c64)
    for family in ("bfStageKernelReal", "bfStageKernelRealBoth", "bfStageKernelSmall", "bfStageKernelT", "bfStageKernelTBoth",
                   "bfSynthKernel", "bfReduceKernel"):
        assert re.search(rf"\d{{2}}{family}I", names), family
    for k, v in c64.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
