"""Mixed-precision GMRES refinement (bfhipSolveGMRESRefine[Device]) without a GPU: the numpy restatement
(tests/refine_ref.py) on a complex64 model of the operator, every refusal on plan-only operators, and the
options struct against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from butterfly_amd import _capi, helm2_structure as hs
from butterfly_amd.operator import HipOperator
from oracle import bfref
import bie
import refine_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = _capi.FLAG_PLAN_ONLY


@pytest.fixture(scope="module")
def system():
    desc, root, vals, dense = bie.second_kind_case(2048, 128)
    A = bfref.from_desc(desc, vals, root=root)
    rng = np.random.default_rng(7)
    b = rng.standard_normal((2048, 3)) + 1j * rng.standard_normal((2048, 3))
    return desc, root, vals, dense, A, b


def test_restatement_converges_in_a_few_steps_and_one_step_stalls(system):
    desc, root, vals, dense, A, b = system
    low = HipOperator.from_desc(desc, vals, root=root, flags=PLAN, demote_to_f32=True)
    mv, mv_low = (lambda v: bfref.mat_mul(A, v)), refine_ref.c64_model(low)
    rel = np.linalg.norm(mv_low(b) - mv(b)) / np.linalg.norm(mv(b))
    assert 1e-9 < rel < 1e-6                                   # the inner operator is a complex64 approximation
    x, k, inner, hist = refine_ref.solve_refine(mv, mv_low, b, tol=1e-12)
    assert hist[-1] <= 1e-12 and k == refine_ref.OUTER_STEPS_2048
    assert all(hist[i + 1] < 0.5 * hist[i] for i in range(k))
    assert refine_ref.true_residual(mv, b, x) == hist[-1]
    assert np.linalg.norm(x - np.linalg.solve(dense, b)) / np.linalg.norm(np.linalg.solve(dense, b)) < 1e-10
    # one step, its correction solved as far as the complex64 operator allows: the outer loop is what reaches 1e-12
    _, k1, _, hist1 = refine_ref.solve_refine(mv, mv_low, b, tol=1e-12, inner_tol=1e-14, max_outer=1)
    assert k1 == 1 and hist1[1] >= 1e-9
    # a zero column stays exactly zero
    bz = b.copy()
    bz[:, 1] = 0
    xz, _, _, histz = refine_ref.solve_refine(mv, mv_low, bz, tol=1e-12)
    assert histz[-1] <= 1e-12 and np.all(xz[:, 1] == 0) and np.all(np.isfinite(xz))
    low.close()


def _real_diag(n, dtype, demote=False):
    d = hs.Desc(dtype=dtype)
    ch = [(d.add(hs.NODE_IDENTITY, min(s + 64, n) - s, min(s + 64, n) - s), s, s) for s in range(0, n, 64)]
    d.root = d.add(hs.NODE_BLOCK, n, n, ch, hs.BF_TYPE_BLOCK_DIAG)
    return HipOperator.from_desc(d, None, flags=PLAN, demote_to_f32=demote)


def test_every_refusal_needs_no_gpu(helm2_cases):
    desc, tp, vals = helm2_cases(1024, 64)
    n = 1024
    op = HipOperator.from_desc(desc, vals, flags=PLAN)
    low = HipOperator.from_desc(desc, vals, flags=PLAN, demote_to_f32=True)
    d2, tp2, v2 = helm2_cases(2048, 128)
    low_other_n = HipOperator.from_desc(d2, v2, flags=PLAN, demote_to_f32=True)
    f64, f32 = _real_diag(n, 1), _real_diag(n, 1, demote=True)
    b = np.ones((n, 2), dtype=np.complex128)

    def code(a=op, lo=low, bb=b, **kw):
        with pytest.raises(_capi.BfhipError) as e:
            a.solve_gmres_refine(bb, lo, **kw)
        return e.value.code

    # every argument is checked before the device is: with all of them right, the plan-only operator is what is refused
    assert code() == 2
    assert code(precond=op) == 2 and code(precond=low) == 2
    assert code(a=low) == 7 and code(a=f64) == 7                    # the system operator must be complex128
    assert code(lo=op) == 7 and code(lo=f32) == 7                   # the inner operator must be complex64
    assert code(lo=low_other_n) == 1                                # n mismatch
    assert code(precond=f64) == 7 and code(precond=low_other_n) == 1
    assert code(max_outer=0) == 1 and code(max_inner=0) == 1
    assert code(tol=0.0) == 1 and code(tol=-1e-12) == 1 and code(tol=float("nan")) == 1
    assert code(inner_tol=-1.0) == 1
    assert code(bb=np.ones((n, 0), dtype=np.complex128)) == 1        # nrhs = 0
    # structSize too small, on both entries
    lib = _capi.load()
    o = op._refine_options(1e-12, 0.0, 10, 100, None, "default")
    o.structSize = C.sizeof(o) - 8
    out = np.empty((n, 2), dtype=np.complex128)
    assert lib.bfhipSolveGMRESRefine(op.handle, low.handle, C.byref(o), b.ctypes.data, 2, 2, None, 2, None, None, None, None,
                                     out.ctypes.data, 2) == 1
    assert lib.bfhipSolveGMRESRefineDevice(op.handle, low.handle, C.byref(o), b.ctypes.data, 2, None, None, None, None, None,
                                           out.ctypes.data, None) == 1
    assert lib.bfhipSolveGMRESRefineDevice(op.handle, low.handle, None, b.ctypes.data, 2, None, None, None, None, None,
                                           out.ctypes.data, None) == 1
    o.structSize = C.sizeof(o)
    o.orthogonalization = 7
    assert lib.bfhipSolveGMRESRefineDevice(op.handle, low.handle, C.byref(o), b.ctypes.data, 2, None, None, None, None, None,
                                           out.ctypes.data, None) == 1
    # complex64 vectors are refused in Python: the complex64 work is internal
    with pytest.raises(ValueError, match="complex128"):
        op.solve_gmres_refine(b.astype(np.complex64), low)
    for o_ in (op, low, low_other_n, f64, f32):
        o_.close()


def test_refine_options_struct_matches_the_header(tmp_path):
    fields = [f for f, _ in _capi.BfhipGmresRefineOptions._fields_]
    src = tmp_path / "sz.c"
    body = "".join(f'printf("%zu ", offsetof(BfhipGmresRefineOptions, {f}));' for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bfhip.h"\nint main(void){' + body +
                   'printf("%zu\\n", sizeof(BfhipGmresRefineOptions));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [getattr(_capi.BfhipGmresRefineOptions, f).offset for f in fields] + [C.sizeof(_capi.BfhipGmresRefineOptions)]
    assert got == want
    assert fields == ["structSize", "orthogonalization", "tol", "innerTol", "maxOuter", "maxInner", "solveM"]
