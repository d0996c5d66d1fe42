"""Dense extraction (bfhipExtract[Device], bfhipExtractWorkspaceBytes), the host-apply panel width and the shim's ToType slot
without a GPU: every refusal on plan-only operators, the workspace formula, the panel-width rule, the slot index against the
reference's headers, and the new kernels' resources."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from butterfly_amd import _capi
from butterfly_amd.operator import HipOperator
from fixtures import load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PLAN = _capi.FLAG_PLAN_ONLY
INVALID, RUNTIME, MEMORY, OUT_OF_RANGE = 1, 2, 4, 5


@pytest.fixture(scope="module")
def ops():
    desc, vals, _ = load_fixture(os.path.join(GOLD, "real_nested_small.npz"))
    fwd = HipOperator.from_desc(desc, vals, flags=PLAN)
    adj = HipOperator.from_desc(desc, vals, flags=PLAN | _capi.FLAG_ADJOINT)
    yield fwd, adj
    fwd.close()
    adj.close()


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


def _call(op, rows, nr, cols, nc, ld, flags=0, panel=0, host=False):
    lib = _capi.load()
    o = _capi.BfhipExtractOptions(flags, panel)
    ra, rp = _u64(rows) if rows is not None else (None, None)
    ca, cp = _u64(cols) if cols is not None else (None, None)
    out = C.c_void_p(0x1000)        # never touched: every call here is refused (or a no-op) before any access
    if host:
        return lib.bfhipExtract(op.handle, rp, nr, cp, nc, out, ld, C.byref(o))
    return lib.bfhipExtractDevice(op.handle, rp, nr, cp, nc, out, ld, C.byref(o), None)


@pytest.mark.parametrize("host", [False, True])
def test_arguments_are_checked_before_the_plan_only_refusal(ops, host):
    fwd, adj = ops
    m, n = fwd.shape
    rows, cols = np.array([0, m - 1, 3, 3]), np.array([n - 1, 0, 2])
    assert _call(fwd, rows, 4, cols, 3, 3, host=host) == RUNTIME                     # valid: only then refused for having no device
    assert _call(fwd, [0, m], 2, cols, 3, 3, host=host) == OUT_OF_RANGE               # row index out of range
    assert _call(fwd, rows, 4, [n], 1, 3, host=host) == OUT_OF_RANGE                  # column index out of range
    assert _call(fwd, rows, 4, cols, 3, 2, host=host) == INVALID                      # ldOut < numCols
    assert _call(fwd, rows, 4, cols, 3, 3, panel=65, host=host) == INVALID            # panel > 64
    assert _call(fwd, rows, 4, cols, 3, 3, panel=64, host=host) == RUNTIME
    assert _call(fwd, rows, 4, cols, 3, 3, flags=_capi.BFHIP_EXTRACT_VIA_ADJOINT, host=host) == INVALID   # no adjoint plan
    assert _call(adj, rows, 4, cols, 3, 3, flags=_capi.BFHIP_EXTRACT_VIA_ADJOINT, host=host) == RUNTIME
    assert _call(fwd, rows, 4, cols, 3, 3, flags=2, host=host) == INVALID             # unknown flag
    assert _call(fwd, None, m - 1, cols, 3, 3, host=host) == INVALID                  # NULL set with a wrong count
    assert _call(fwd, rows, 4, None, n + 1, n + 1, host=host) == INVALID
    assert _call(fwd, None, m, None, n, n, host=host) == RUNTIME
    # nothing to extract: a no-op, even without a device
    assert _call(fwd, rows, 0, cols, 3, 3, host=host) == 0
    assert _call(fwd, rows, 4, cols, 0, 0, host=host) == 0
    assert _call(fwd, [0, 2 * m], 2, cols, 3, 3, host=host) == OUT_OF_RANGE and "rows[1]" in _capi.load().bfhipLastErrorMessage().decode()


def test_python_wrapper_refuses_a_plan_only_operator(ops):
    fwd, _ = ops
    with pytest.raises(_capi.BfhipError) as ei:
        fwd.extract(rows=[0], cols=[0], device=False)
    assert ei.value.code == RUNTIME


def test_workspace_bytes_follow_the_formula_and_scale_with_the_panel(ops):
    fwd, adj = ops
    m, n = fwd.shape
    st = adj.stats()
    es = 8                                      # f64 operand
    te = max(st["tempElems"], adj_plan_temp(adj))
    for op in (fwd, adj):
        te_op = max(op.stats()["tempElems"], adj_plan_temp(op))
        for p in (1, 17, 64):
            for nr, nc in ((5, 7), (m, n), (3, 100000)):
                got = op.extract_workspace_bytes(nr, nc, panel=p)
                assert got == (m + n) * p * es + (nr + nc) * 8 + te_op * p * es + 2 * nr * p * es
        assert op.extract_workspace_bytes(5, 7, panel=0) == op.extract_workspace_bytes(5, 7, panel=64)
    # the adjoint route gathers blocks of the column set
    assert adj.extract_workspace_bytes(5, 7, via_adjoint=True, panel=8) == (m + n) * 8 * es + 12 * 8 + te * 8 * es + 2 * 7 * 8 * es
    # the panel terms do not grow with the number of columns extracted: only the 8-byte index copies do
    a, b = fwd.extract_workspace_bytes(10, 1000), fwd.extract_workspace_bytes(10, 2000)
    assert b - a == 1000 * 8
    with pytest.raises(_capi.BfhipError):
        fwd.extract_workspace_bytes(1, 1, panel=65)


def adj_plan_temp(op):
    info = _capi.BfhipPlanInfo()
    info.structSize = C.sizeof(info)
    _capi.check(_capi.load().bfhipPlanGetInfo(op.handle, C.byref(info)))
    return int(info.tempElemsT)


def _panel_width(nrhs, per_col, budget):
    lib = _capi.load()
    fn = lib.bfhipHostApplyPanelWidth
    fn.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    fn.restype = C.c_int
    w = C.c_uint64(12345)
    rc = fn(nrhs, per_col, budget, C.byref(w))
    return rc, int(w.value)


def test_host_apply_panel_width_rule():
    # fits: one piece, whatever the width
    assert _panel_width(128, 1000, 128 * 1000) == (0, 128)
    assert _panel_width(3, 1000, 3000) == (0, 3)
    assert _panel_width(65535, 1, 1 << 40) == (0, 65535)
    # does not fit: the widest multiple of 64 that does
    assert _panel_width(128, 1000, 128 * 1000 - 1) == (0, 64)
    assert _panel_width(192, 1000, 191 * 1000) == (0, 128)
    assert _panel_width(100000, 1000, 1000 * 1000) == (0, 960)
    # more than one apply takes: panels of at most 65472 (the largest multiple of 64 below 65536)
    assert _panel_width(70000, 1, 1 << 40) == (0, 65472)
    assert _panel_width(70000, 0, 0) == (0, 65472)
    # not even one 64-column panel fits: refused, naming the need
    rc, w = _panel_width(128, 1000, 63 * 1000)
    assert rc == MEMORY and w == 0
    assert "64" in _capi.load().bfhipLastErrorMessage().decode()
    assert _panel_width(10, 1000, 9999)[0] == MEMORY


def test_set_host_apply_budget_is_host_only(ops):
    fwd, _ = ops
    fwd.set_host_apply_budget(1 << 20)
    fwd.set_host_apply_budget(0)
    assert _capi.load().bfhipSetHostApplyBudget(None, 0) == INVALID


def _slot_of_ours():
    src = '#include <stdio.h>\n#include "bfhip_abi.h"\nint main(void) { printf("%d\\n", (int)BFABI_SLOT_ToType); return 0; }\n'
    return src


def test_totype_slot_index_matches_the_reference(tmp_path):
    c = tmp_path / "ours.c"
    c.write_text(_slot_of_ours())
    subprocess.check_call(["gcc", "-std=gnu11", f"-I{ROOT}/include", str(c), "-o", str(tmp_path / "ours")])
    ours = int(subprocess.check_output([str(tmp_path / "ours")], text=True))
    # recorded from the reference's include/bf/mat.h (offsetof(BfMatVtable, ToType) / sizeof(void *))
    assert ours == json.load(open(os.path.join(GOLD, "reference_totype_slot.json")))["slot_ToType"] == 54


def test_totype_slot_index_against_the_reference_headers(tmp_path):
    """Compiled against the reference's own headers, as tests/test_abi_layout.py's probe; BF_REFERENCE_INCLUDE names them."""
    inc = os.environ.get("BF_REFERENCE_INCLUDE", "")
    if not inc or not os.path.exists(os.path.join(inc, "bf", "mat.h")):
        pytest.skip("reference headers not available (set BF_REFERENCE_INCLUDE to <reference>/include)")
    c = tmp_path / "ref.c"
    c.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <bf/mat.h>\n"
                 'int main(void) { printf("%zu\\n", offsetof(BfMatVtable, ToType) / sizeof(void *)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=gnu11", "-DBF_DOUBLE", "-DBF_LINUX", f"-I{inc}", str(c), "-o", str(tmp_path / "ref")])
    ref = int(subprocess.check_output([str(tmp_path / "ref")], text=True))
    c2 = tmp_path / "ours.c"
    c2.write_text(_slot_of_ours())
    subprocess.check_call(["gcc", "-std=gnu11", f"-I{ROOT}/include", str(c2), "-o", str(tmp_path / "ours")])
    assert int(subprocess.check_output([str(tmp_path / "ours")], text=True)) == ref


def test_extract_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path / "ex.s"
    subprocess.check_call([hipcc, "-O3", "-g", "-fPIC", "--offload-arch=gfx950", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(ROOT, "butterfly_amd", "csrc", "bfhip_extract.hip")], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    names = re.findall(r"\.name:\s+(_Z\w*bfExtract\w+)", txt)
    assert sum("UnitKernel" in s for s in names) == 4 and sum("GatherKernel" in s for s in names) == 3 and sum("GatherTKernel" in s for s in names) == 3
    blocks = txt.split("amdhsa.kernels:")[1].split("\n  - .agpr_count:")[1:]      # one metadata entry per kernel
    for sym in names:
        meta = [blk for blk in blocks if re.search(r"\.name:\s+" + sym + r"\s", blk)][0]
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", meta).group(1))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0, sym
        assert get("group_segment_fixed_size") <= 34 * 1024, sym
    # no atomics, no scalar memory writes
    isa = txt.split(".amdgpu_metadata")[0]
    assert not re.search(r"\b(global|flat|buffer)_atomic", isa)
