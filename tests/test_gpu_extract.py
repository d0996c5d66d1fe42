"""Dense extraction on the GPU (bfhipExtract[Device], HipOperator.extract / to_dense), panelled wide host applies
(bfhipSetHostApplyBudget) and the shim's ToType slot: against the oracle, and bit for bit against the apply on unit panels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def helm2(helm2_cases):
    from oracle import bfref
    desc, tp, vals = helm2_cases(2048, 128)
    A = bfref.from_desc(desc, vals)
    dense = bfref.mat_mul(A, np.eye(2048, dtype=complex))
    return desc, vals, A, dense


def _operands(helm2):
    """(name, operator) for complex128, complex64, f64 and f32, each with an adjoint plan"""
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from fixtures import load_fixture
    desc, vals, _, _ = helm2
    rdesc, rvals, _ = load_fixture(os.path.join(GOLD, "real_nested_small.npz"))
    f = _capi.FLAG_ADJOINT
    return [("c128", HipOperator.from_desc(desc, vals, flags=f)), ("c64", HipOperator.from_desc(desc, vals, flags=f, demote_to_f32=True)),
            ("f64", HipOperator.from_desc(rdesc, rvals, flags=f)), ("f32", HipOperator.from_desc(rdesc, rvals, flags=f, demote_to_f32=True))]


def _unit_panel_apply(op, idx, transpose):
    """A (or A^T) applied to the host-built unit panel of the indices `idx`: the reference the extraction must match bit for bit"""
    torch = _torch()
    m, n = op.shape
    ext = m if transpose else n
    x = torch.zeros((ext, len(idx)), dtype=op._torch_dtype(), device="cuda")
    x[torch.as_tensor(idx, device="cuda"), torch.arange(len(idx), device="cuda")] = 1
    y = op.apply_transpose_device(x) if transpose else op.apply_device(x)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def test_whole_operator_equals_the_oracle_densified(helm2):
    import bie
    from butterfly_amd.operator import HipOperator
    from oracle import bfref
    desc, vals, A, dense = helm2
    op = HipOperator.from_desc(desc, vals)
    got = op.to_dense()
    assert got.dtype == np.complex128 and got.shape == (2048, 2048)
    assert rel(got, dense) <= 1e-12
    dev = op.to_dense(device=True)
    assert np.array_equal(dev.cpu().numpy(), got)
    op.close()
    bdesc, broot, bvals, _ = bie.second_kind_case(2048, 128)
    B = bfref.from_desc(bdesc, bvals, root=broot)
    bop = HipOperator.from_desc(bdesc, bvals, root=broot)
    assert rel(bop.to_dense(), bfref.mat_mul(B, np.eye(2048, dtype=complex))) <= 1e-12
    bop.close()


def test_blocks_equal_the_apply_on_unit_panels_bit_for_bit(helm2):
    rng = np.random.default_rng(11)
    for name, op in _operands(helm2):
        m, n = op.shape
        rows = rng.integers(0, m, size=min(m, 300))
        rows[:5] = rows[5]                                         # repeats
        cols = rng.integers(0, n, size=150)                        # panels of 64, 64 and a ragged 22
        cols[10] = cols[11]
        blk = op.extract(rows, cols).cpu().numpy()
        assert blk.shape == (len(rows), len(cols))
        for p in (64, 37):
            if p != 64:
                blk = op.extract(rows, cols, panel=p).cpu().numpy()
            for c0 in range(0, len(cols), p):
                y = _unit_panel_apply(op, cols[c0:c0 + p], False)
                assert np.array_equal(blk[:, c0:c0 + p], y[rows]), (name, p, c0)
        op.close()


def test_adjoint_route_equals_the_transposed_apply_bit_for_bit(helm2):
    rng = np.random.default_rng(12)
    for name, op in _operands(helm2):
        m, n = op.shape
        rows = rng.integers(0, m, size=100)                        # panels of 64 and a ragged 36 over the ROW set
        cols = rng.integers(0, n, size=min(n, 333))
        via = op.extract(rows, cols, via_adjoint=True).cpu().numpy()
        for r0 in range(0, len(rows), 64):
            p = _unit_panel_apply(op, rows[r0:r0 + 64], True)      # A^T E: n x pw
            assert np.array_equal(via[r0:r0 + 64, :], p[cols].T), (name, r0)
        fwd = op.extract(rows, cols).cpu().numpy()
        tol = 1e-13 if name in ("c128", "f64") else 1e-5
        assert rel(via, fwd) <= tol, name
        op.close()


def test_host_entry_equals_the_device_entry_pageable_and_registered(helm2):
    from butterfly_amd.operator import HipOperator
    rng = np.random.default_rng(13)
    for name, op in _operands(helm2):
        m, n = op.shape
        rows, cols = rng.integers(0, m, size=77), rng.integers(0, n, size=130)
        for via in (False, True):
            dev = op.extract(rows, cols, via_adjoint=via).cpu().numpy()
            want = dev.astype(np.complex128 if np.iscomplexobj(dev) else np.float64)
            host = op.extract(rows, cols, via_adjoint=via, device=False)
            assert host.dtype == want.dtype and np.array_equal(host, want), (name, via)
            big = np.full((len(rows), len(cols) + 9), 7.0, dtype=want.dtype)      # ldOut > numCols: the padding stays untouched
            op.extract(rows, cols, via_adjoint=via, device=False, out=big[:, :len(cols)])
            assert np.array_equal(big[:, :len(cols)], want) and np.all(big[:, len(cols):] == 7.0)
            reg = np.full((len(rows), len(cols) + 5), 3.0, dtype=want.dtype)
            HipOperator.host_register(reg)
            try:
                op.extract(rows, cols, via_adjoint=via, device=False, out=reg[:, :len(cols)])
            finally:
                HipOperator.host_unregister(reg)
            assert np.array_equal(reg[:, :len(cols)], want) and np.all(reg[:, len(cols):] == 3.0), (name, via)
        op.close()


def test_extraction_memory_stays_within_the_workspace_bound(helm2):
    torch = _torch()
    from butterfly_amd.operator import HipOperator
    desc, vals, _, _ = helm2
    op = HipOperator.from_desc(desc, vals)
    rows, cols = np.arange(0, 2048, 3), np.arange(2047, -1, -2)
    out = torch.empty((len(rows), len(cols)), dtype=torch.complex128, device="cuda")
    hout = np.empty((len(rows), len(cols)), dtype=np.complex128)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    op.extract(rows, cols, out=out)
    op.extract(rows, cols, device=False, out=hout)
    torch.cuda.synchronize()
    drop = free0 - torch.cuda.mem_get_info()[0]
    bound = op.extract_workspace_bytes(len(rows), len(cols))
    assert drop <= bound + 8 * (2 << 20), (drop, bound)       # + allocation granularity of the ~8 buffers
    assert np.array_equal(out.cpu().numpy(), hout)
    op.close()


def _kernel_ids(desc, vals, nrhs):
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    p = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_PLAN_ONLY)
    ids = p.stage_kernels(nrhs)
    p.close()
    return ids


def test_panelled_host_apply_matches_the_one_piece_apply(helm2):
    from butterfly_amd.operator import HipOperator
    desc, vals, _, _ = helm2
    rng = np.random.default_rng(14)
    ref = HipOperator.from_desc(desc, vals)
    st = ref.stats()
    per_col = (2 * 2048 + st["tempElems"]) * 16
    for nrhs in (128, 192):
        x = rng.standard_normal((2048, nrhs)) + 1j * rng.standard_normal((2048, nrhs))
        want = ref.apply_host(x)
        op = HipOperator.from_desc(desc, vals)
        op.set_host_apply_budget(per_col * 64 + 100)             # panels of 64 columns
        got = op.apply_host(x)
        if _kernel_ids(desc, vals, 64) == _kernel_ids(desc, vals, nrhs):
            assert np.array_equal(got, want), nrhs
        else:
            assert rel(got, want) <= 1e-14, nrhs
        op.set_host_apply_budget(per_col * 63)                   # not even one panel fits
        with pytest.raises(Exception):
            op.apply_host(x)
        op.close()
    ref.close()


def test_host_apply_of_70000_columns(helm2_cases):
    from butterfly_amd.operator import HipOperator
    from oracle import bfref
    desc, tp, vals = helm2_cases(1024, 64)
    A = bfref.from_desc(desc, vals)
    op = HipOperator.from_desc(desc, vals)
    rng = np.random.default_rng(15)
    nrhs = 70000
    x = np.empty((1024, nrhs), dtype=np.complex128)
    x.real = rng.standard_normal((1024, nrhs))
    x.imag = rng.standard_normal((1024, nrhs))
    y = op.apply_host(x)
    sample = np.concatenate([[0, 1, 65471, 65472, 65473, nrhs - 1], rng.integers(0, nrhs, size=26)])
    assert rel(y[:, sample], bfref.mat_mul(A, np.ascontiguousarray(x[:, sample]))) <= 1e-12
    op.close()


def _zeros_helper(tmp_path):
    """The oracle exports bfMatDenseComplexNewZeros; the shim looks for the reference's bfMatDenseComplexZeros."""
    from oracle import bfref
    bfref.load()
    src = tmp_path / "zeros.c"
    src.write_text("#include <stddef.h>\nvoid *bfMatDenseComplexNewZeros(size_t, size_t);\n"
                   "void *bfMatDenseComplexZeros(size_t m, size_t n) { return bfMatDenseComplexNewZeros(m, n); }\n")
    so = tmp_path / "libzeros.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    return C.CDLL(str(so), mode=C.RTLD_GLOBAL)


def _to_type(mat, type_):
    vtbl = C.cast(C.c_void_p(mat), C.POINTER(C.c_void_p))[0]
    fn = C.cast(vtbl, C.POINTER(C.c_void_p))[54]
    assert fn
    return C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int)(fn)(mat, type_)


def test_shim_mul_by_the_identity_and_to_type(helm2, tmp_path):
    from butterfly_amd import _capi
    from butterfly_amd.operator import HipOperator
    from oracle import bfref
    desc, vals, A, dense = helm2
    lib = bfref.load()
    op = HipOperator.from_bfmat(A.ptr.value, flags=_capi.FLAG_ADJOINT)
    st = op.stats()
    op.set_host_apply_budget((2 * 2048 + st["tempElems"]) * 16 * 256)       # bfMatMul(A_hip, I_N) in panels of 256
    a_hip = op.as_bfmat()
    I = bfref.dense_complex(np.eye(2048, dtype=complex))
    r = lib.bfMatMul(C.c_void_p(a_hip), I.ptr)
    assert r
    assert rel(bfref.Mat(r).to_numpy(), dense) <= 1e-12
    keep = _zeros_helper(tmp_path)
    r = _to_type(a_hip, 19)                                                    # BF_TYPE_MAT_DENSE_COMPLEX
    assert r
    Y = bfref.Mat(r)
    assert Y.type == 19 and rel(Y.to_numpy(), dense) <= 1e-12
    assert np.array_equal(Y.to_numpy(), op.to_dense())
    lib.bfClearError()
    assert not _to_type(a_hip, 20)                                             # any other type: NOT_IMPLEMENTED
    assert lib.bfGetError() == 3
    lib.bfClearError()
    lib.bfMatTranspose(C.c_void_p(a_hip))                                      # now A^H
    r = _to_type(a_hip, 19)
    assert r and rel(bfref.Mat(r).to_numpy(), dense.conj().T) <= 1e-12
    p = C.c_void_p(a_hip)
    lib.bfMatDelete(C.byref(p))
    op.close()
    del keep


def test_to_type_refuses_a_real_operator(tmp_path):
    from butterfly_amd.operator import HipOperator
    from fixtures import load_fixture
    from oracle import bfref
    lib = bfref.load()
    keep = _zeros_helper(tmp_path)
    rdesc, rvals, _ = load_fixture(os.path.join(GOLD, "real_nested_small.npz"))
    op = HipOperator.from_desc(rdesc, rvals)
    a_hip = op.as_bfmat()
    lib.bfClearError()
    assert not _to_type(a_hip, 19)
    assert lib.bfGetError() == 3
    lib.bfClearError()
    p = C.c_void_p(a_hip)
    lib.bfMatDelete(C.byref(p))
    op.close()
    del keep


def test_full_size_columns_match_single_column_applies():
    torch = _torch()
    from butterfly_amd import helm2_structure as hs
    from butterfly_amd.operator import HipOperator
    n, k = 65536, 4096.0
    pts = hs.circle_points(n)
    desc, _, perm = hs.helm2_multilevel_structure(pts, k, recipes=True, exact_sift=True)
    op, st = HipOperator.build_helm2(desc, pts[perm], k)
    cols = np.random.default_rng(16).choice(n, size=256, replace=False)
    blk = op.extract(None, cols)
    torch.cuda.synchronize()
    for j in range(256):
        e = torch.zeros(n, dtype=torch.complex128, device="cuda")
        e[int(cols[j])] = 1
        y = op.apply_device(e)
        err = float((torch.linalg.norm(blk[:, j] - y) / torch.linalg.norm(y)).item())
        assert err <= 1e-13, (j, err)
    op.close()
