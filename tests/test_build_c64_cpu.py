"""Complex64 output of the device Helmholtz builder (BfhipHelm2Problem.outDtype, bfhipBuildHelm2Pair), the part that needs no
GPU: the argument checks, and that the operands of tests/test_gpu_build_c64.py put every piece layout of a complex64 plan in
front of the pack kernel."""
import ctypes as C
import os

import numpy as np
import pytest

from butterfly_amd import _capi
from butterfly_amd import helm2_structure as hs
from butterfly_amd.operator import HipOperator

import build_c64_cases as bc


def _small_case():
    n, k = 1024, 64.0
    pts = hs.circle_points(n)
    desc, _, perm = hs.helm2_multilevel_structure(pts, k, recipes=True)
    return desc, pts[perm], 2 * np.pi * k


def test_pair_entry_is_declared_and_exported():
    lib = _capi.load()
    assert hasattr(lib, "bfhipBuildHelm2Pair")
    from conftest import ROOT
    with open(os.path.join(ROOT, "include", "bfhip_build.h")) as f:
        assert "bfhipBuildHelm2Pair(" in f.read()
    assert dict(_capi.BfhipHelm2Problem._fields_)["outDtype"] is C.c_uint32
    assert _capi.BfhipHelm2Problem.outDtype.offset == _capi.BfhipHelm2Problem.krOrder.offset + 4


def test_unknown_out_dtype_is_refused_before_any_device_work():
    desc, tp, k = _small_case()
    for entry in (lambda: HipOperator.build_helm2(desc, tp, k, out_dtype=7),
                  lambda: _pair_with_dtype(desc, tp, k, 7),
                  lambda: HipOperator.fac_helm2_make_multilevel(tp, k, out_dtype=7)):
        with pytest.raises(_capi.BfhipError) as e:
            entry()
        assert e.value.code == 1 and "outDtype" in str(e.value)
    # real storage types are no output of a complex builder either
    for dt in (_capi.BFHIP_F64, _capi.BFHIP_F32):
        with pytest.raises(_capi.BfhipError) as e:
            HipOperator.build_helm2(desc, tp, k, out_dtype=dt)
        assert e.value.code == 1


def _pair_with_dtype(desc, tp, k, out_dtype, low_opts=None, **opts):
    """bfhipBuildHelm2Pair with a problem whose outDtype is set (HipOperator.build_helm2_pair has no such keyword)."""
    from butterfly_amd.operator import _options
    lib = _capi.load()
    da = _capi.DescArrays(desc)
    prob = _capi.Helm2Problem(tp, k, desc.recipe, out_dtype=out_dtype)
    st = _capi.BfhipBuildStats()
    st.structSize = C.sizeof(st)
    h, hl = C.c_void_p(), C.c_void_p()
    o = _options(**opts)
    ol = None if low_opts is None else _options(**low_opts)
    _capi.check(lib.bfhipBuildHelm2Pair(da.byref(), prob.byref(), C.byref(o), None if ol is None else C.byref(ol), C.byref(h), C.byref(hl),
                                        C.byref(st)))
    return h, hl


def test_pair_refuses_complex64_through_the_problem_and_two_devices():
    desc, tp, k = _small_case()
    with pytest.raises(_capi.BfhipError) as e:
        _pair_with_dtype(desc, tp, k, _capi.BFHIP_C64)
    assert e.value.code == 1 and "outDtype" in str(e.value)
    with pytest.raises(_capi.BfhipError) as e:
        _pair_with_dtype(desc, tp, k, None, low_opts=dict(device=1), device=0)
    assert e.value.code == 1 and "one device" in str(e.value)
    # demoteToF32 stays refused on the pair entry as on the others, in either options
    for kw in (dict(demote_to_f32=True), dict(low_opts=dict(demote_to_f32=True))):
        with pytest.raises(_capi.BfhipError) as e:
            HipOperator.build_helm2_pair(desc, tp, k, **kw)
        assert e.value.code == 3 and "complex64" in str(e.value)
    with pytest.raises(_capi.BfhipError) as e:
        HipOperator.build_helm2_pair(desc, tp, k, flags=_capi.FLAG_PLAN_ONLY)
    assert e.value.code == 1


def test_thin_leaf_block_has_every_piece_layout_of_a_complex64_plan():
    desc, pts = bc.thin_leaf_block()
    assert (desc.rows[desc.root], desc.cols[desc.root]) == (132, 1553) and len(desc.recipe) == 40 and len(pts) == 1600
    op = HipOperator.from_desc(desc, flags=_capi.FLAG_PLAN_ONLY | _capi.FLAG_ADJOINT, demote_to_f32=True)
    stages, dtype, census = bc.piece_census(op)
    assert stages == 1 and dtype == _capi.BFHIP_C64
    assert {k: len(v) for k, v in census.items()} == {"plain": 63, "merged": 4, "rowmajor": 20, "small": 4}
    rm = census["rowmajor"] + census["small"]
    assert {r for r, _, _ in rm} == {1, 2, 3, 4}
    # padded row strides, and the 1100-column leaf cut into 1024 + 76
    assert {(n, ld) for _, n, ld in rm} == {(3, 4), (20, 20), (130, 144), (300, 304), (1024, 1024), (76, 76)}
    assert {r for r, _, _ in census["small"]} == {1, 2, 3, 4}
    # column-major pieces whose row count is odd (one padding row of complex64) and even
    assert {r % 2 for r, _, _ in census["plain"]} == {0, 1} and {r % 2 for r, _, _ in census["merged"]} == {0, 1}
    op.close()
    # the complex128 plan of the same descriptor has none of the real family's layouts: the control of the GPU test packs plain pieces
    op = HipOperator.from_desc(desc, flags=_capi.FLAG_PLAN_ONLY)
    _, dtype, census = bc.piece_census(op)
    assert dtype == _capi.BFHIP_C128 and not census["merged"] and not census["rowmajor"] and not census["small"]
    op.close()


def test_butterfly_case_has_three_stages_with_plain_merged_and_rowmajor_pieces(helm2_cases):
    desc, _, _ = helm2_cases(2048, 64.0)
    op = HipOperator.from_desc(desc, flags=_capi.FLAG_PLAN_ONLY, demote_to_f32=True)
    stages, dtype, census = bc.piece_census(op)
    assert stages == 3 and dtype == _capi.BFHIP_C64
    assert {k: len(v) for k, v in census.items()} == {"plain": 1200, "merged": 792, "rowmajor": 128, "small": 0}
    assert any(ld > n for _, n, ld in census["rowmajor"])
    op.close()
