"""Block-Jacobi preconditioner, host side (no GPU): the automatic partition, a numpy restatement of the direct-part rule read
through the plan-inspection C-ABI (FLAG_PLAN_ONLY), the argument checks, the kernels' resources, and the iteration count the
GPU tests rely on."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from butterfly_amd import _capi, helm2_structure as hs
from butterfly_amd.operator import HipOperator
from oracle import helm2_build as hb, linalg_ref
import bie
from bj_ref import direct_blocks, self_leaf_cuts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K = 2048, 128

@pytest.fixture(scope="module")
def operands():
    from conftest import helm2_case
    desc, tp, vals = helm2_case(N, K)
    dense_s = hb.kernel_matrix(K, tp, tp)
    d2, root2, v2, dense2 = bie.second_kind_case(N, K)
    first = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_PLAN_ONLY)
    second = HipOperator.from_desc(d2, v2, root=root2, flags=_capi.FLAG_PLAN_ONLY)
    yield {"first": (first, desc, desc.root, dense_s), "second": (second, d2, root2, dense2)}
    first.close()
    second.close()


@pytest.mark.parametrize("case", ["first", "second"])
def test_automatic_cuts_are_the_diagonal_self_leaves(operands, case):
    op, desc, root, _ = operands[case]
    cuts = op.block_jacobi_partition()
    ref = self_leaf_cuts(desc, root, N)
    assert cuts[0] == 0 and cuts[-1] == N
    np.testing.assert_array_equal(cuts, ref)
    sizes = np.diff(cuts)
    assert sizes.max() < 128 and sizes.min() > 1       # leaf boxes (m * m < 128^2), no uncovered rows on the circle


@pytest.mark.parametrize("case", ["first", "second"])
def test_direct_part_reproduces_the_dense_diagonal_blocks(operands, case):
    op, _, _, dense = operands[case]
    cuts = op.block_jacobi_partition()
    blocks = direct_blocks(op, cuts)
    for (a, b), blk in zip(zip(cuts[:-1], cuts[1:]), blocks):
        ref = dense[a:b, a:b]
        assert np.linalg.norm(blk - ref) <= 1e-15 * np.linalg.norm(ref), (a, b)


def _small_with_product():
    """8 x 8: two dense 4 x 4 diagonal leaves and a product (4 x 2)(2 x 8) over rows 0..3, all columns -- it covers the first
    diagonal block and reaches the second."""
    rng = np.random.default_rng(3)
    d = hs.Desc(dtype=0)
    vals = {}
    a = d.add(hs.NODE_DENSE, 4, 4)
    b = d.add(hs.NODE_DENSE, 4, 4)
    f1 = d.add(hs.NODE_DENSE, 2, 8)
    f0 = d.add(hs.NODE_DENSE, 4, 2)
    for leaf in (a, b, f1, f0):
        vals[leaf] = rng.standard_normal((d.rows[leaf], d.cols[leaf])) + 1j * rng.standard_normal((d.rows[leaf], d.cols[leaf]))
    p = d.add(hs.NODE_PRODUCT, 4, 8, [(f0, 0, 0), (f1, 0, 0)])
    d.root = d.add(hs.NODE_BLOCK, 8, 8, [(a, 0, 0), (b, 4, 4), (p, 0, 0)], hs.BF_TYPE_BLOCK_COO)
    return d, vals, a, b, f0, f1


def test_products_inside_a_diagonal_block_are_left_out():
    d, vals, a, b, f0, f1 = _small_with_product()
    op = HipOperator.from_desc(d, vals, flags=_capi.FLAG_PLAN_ONLY)
    cuts = op.block_jacobi_partition()
    np.testing.assert_array_equal(cuts, [0, 4, 8])            # the product does not join the two blocks
    blocks = direct_blocks(op, cuts)
    np.testing.assert_allclose(blocks[0], vals[a], rtol=0, atol=0)
    np.testing.assert_allclose(blocks[1], vals[b], rtol=0, atol=0)
    full = np.zeros((8, 8), dtype=np.complex128)
    full[:4, :4] += vals[a]
    full[4:, 4:] += vals[b]
    full[:4, :] += vals[f0] @ vals[f1]
    assert np.linalg.norm(full[:4, :4] - vals[a]) > 0.1       # ... although it has entries there
    op.close()


def _bj(op, **kw):
    o = _capi.BfhipBlockJacobiOptions()
    o.structSize = kw.pop("structSize", C.sizeof(o))
    o.flags = kw.pop("flags", 0)
    o.maxBlock = kw.pop("maxBlock", 0)
    o.outDtype = kw.pop("outDtype", 0)
    cuts = kw.pop("cuts", None)
    keep = None
    if cuts is not None:
        keep = np.ascontiguousarray(cuts, dtype=np.uint64)
        o.cuts = keep.ctypes.data
        o.numBlocks = kw.pop("numBlocks", keep.size - 1)
    o.device = -1
    info = _capi.BfhipBlockJacobiInfo()
    info.structSize = C.sizeof(info)
    h = C.c_void_p()
    rc = _capi.load().bfhipBlockJacobi(op.handle, C.byref(o), C.byref(h), C.byref(info))
    assert not h.value
    return rc


def test_refusals(operands):
    lib = _capi.load()
    op = operands["first"][0]
    cuts = op.block_jacobi_partition()
    # valid arguments on a plan-only operator: NOT_IMPLEMENTED, after every check
    assert _bj(op) == 3
    assert _bj(op, cuts=cuts) == 3
    assert _bj(op, cuts=[0, N]) == 1                                   # a block over maxBlock (128)
    assert _bj(op, cuts=[0, N], maxBlock=256) == 1
    c = cuts.copy(); c[3], c[4] = c[4], c[3]
    assert _bj(op, cuts=c) == 1                                        # not increasing
    c = cuts.copy(); c[5] = c[4]
    assert _bj(op, cuts=c) == 1                                        # an empty block
    assert _bj(op, cuts=cuts[:-1]) == 1                                # does not reach n
    assert _bj(op, cuts=np.concatenate([[1], cuts[1:]])) == 1          # does not start at 0
    assert _bj(op, maxBlock=257) == 1
    assert _bj(op, maxBlock=50) == 1                                   # an automatic interval over maxBlock: pass cuts
    assert _bj(op, maxBlock=50, cuts=np.arange(0, N + 1, 32)) == 3     # ... which the caller did
    assert _bj(op, flags=2) == 1
    assert _bj(op, structSize=8) == 1
    assert _bj(op, outDtype=_capi.BFHIP_F32) == 7                      # complex128 -> f32
    assert _bj(op, outDtype=_capi.BFHIP_F64) == 7
    assert _bj(op, outDtype=9) == 7
    assert _bj(op, outDtype=_capi.BFHIP_C64) == 3                      # the demotion is allowed
    nb = C.c_uint64(0)
    buf = np.zeros(N + 1, dtype=np.uint64)
    p = buf.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.bfhipBlockJacobiPartition(op.handle, 257, p, buf.size, C.byref(nb)) == 1
    assert lib.bfhipBlockJacobiPartition(op.handle, 50, p, buf.size, C.byref(nb)) == 1
    assert lib.bfhipBlockJacobiPartition(op.handle, 0, p, buf.size, C.byref(nb)) == 0 and nb.value == len(cuts) - 1
    with pytest.raises(_capi.BfhipError) as e:
        op.block_jacobi_partition(max_block=50)
    assert e.value.code == 1 and "cuts" in str(e.value)
    with pytest.raises(_capi.BfhipError) as e:
        op.block_jacobi()
    assert e.value.code == 3


def test_refusals_by_shape_and_dtype():
    from conftest import helm2_case
    desc, tp, vals = helm2_case(N, K)
    # a row shard is not square
    shard = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_PLAN_ONLY, row_range=(0, 1024))
    assert shard.shape == (1024, N)
    assert _bj(shard) == 8
    with pytest.raises(_capi.BfhipError) as e:
        shard.block_jacobi_partition()
    assert e.value.code == 8
    shard.close()
    d = hs.Desc(dtype=1)
    d.root = d.add(hs.NODE_DENSE, 4, 6)
    rect = HipOperator.from_desc(d, {d.root: np.ones((4, 6))}, flags=_capi.FLAG_PLAN_ONLY)
    assert _bj(rect) == 8
    rect.close()
    # complex64 storage: only complex64 out (outDtype 0 = BFHIP_C128 means "the operator's"); f64 storage: f64 or f32
    low = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_PLAN_ONLY, demote_to_f32=True)
    assert low.dtype == _capi.BFHIP_C64
    assert _bj(low, outDtype=_capi.BFHIP_F32) == 7 and _bj(low, outDtype=_capi.BFHIP_F64) == 7 and _bj(low) == 3 and _bj(low, outDtype=_capi.BFHIP_C64) == 3
    np.testing.assert_array_equal(low.block_jacobi_partition(), self_leaf_cuts(desc, desc.root, N))
    low.close()
    dr = hs.Desc(dtype=1)
    ch = []
    for s in range(0, 64, 16):
        ch.append((dr.add(hs.NODE_DENSE, 16, 16), s, s))
    dr.root = dr.add(hs.NODE_BLOCK, 64, 64, ch, hs.BF_TYPE_BLOCK_DIAG)
    real = HipOperator.from_desc(dr, {c: np.eye(16) + 0.1 for c, _, _ in ch}, flags=_capi.FLAG_PLAN_ONLY)
    np.testing.assert_array_equal(real.block_jacobi_partition(), [0, 16, 32, 48, 64])
    assert _bj(real, outDtype=_capi.BFHIP_F32) == 3 and _bj(real, outDtype=_capi.BFHIP_C64) == 7 and _bj(real) == 3
    real.close()


def test_uncovered_rows_are_blocks_of_their_own():
    d = hs.Desc(dtype=0)
    a = d.add(hs.NODE_DENSE, 3, 3)
    off = d.add(hs.NODE_DENSE, 2, 2)
    d.root = d.add(hs.NODE_BLOCK, 8, 8, [(a, 1, 1), (off, 5, 0)], hs.BF_TYPE_BLOCK_COO)
    vals = {a: np.ones((3, 3)) + 0j, off: np.ones((2, 2)) + 0j}
    op = HipOperator.from_desc(d, vals, flags=_capi.FLAG_PLAN_ONLY)
    np.testing.assert_array_equal(op.block_jacobi_partition(), [0, 1, 4, 5, 6, 7, 8])
    op.close()


def test_precond_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path / "bj.s"
    subprocess.check_call([hipcc, "-O3", "-g", "-fPIC", "--offload-arch=gfx950", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(ROOT, "butterfly_amd", "csrc", "bfhip_precond.hip")], stderr=subprocess.DEVNULL)
    txt = open(out).read()
    names = re.findall(r"\.name:\s+(_Z\w*bfBj\w+)", txt)
    assert sum("GatherKernel" in s for s in names) == 4 and sum("InvertKernel" in s for s in names) == 2 and sum("FillKernel" in s for s in names) == 4
    blocks = txt.split("amdhsa.kernels:")[1].split("\n  - .agpr_count:")[1:]      # one metadata entry per kernel
    for sym in names:
        meta = [blk for blk in blocks if re.search(r"\.name:\s+" + sym + r"\s", blk)][0]
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", meta).group(1))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0, sym
        assert get("group_segment_fixed_size") <= 16 * 1024, sym
    isa = txt.split(".amdgpu_metadata")[0]
    assert not re.search(r"\b(global|flat|buffer)_atomic", isa)


def test_block_jacobi_cuts_iterations_on_the_first_kind_system(operands):
    """What the GPU test of the device-built first-kind system relies on: on the dense S (n = 2048, k = 128), GMRES left-
    preconditioned by the block-Jacobi inverse over the automatic cuts converges in fewer iterations than without."""
    op, _, _, dense = operands["first"]
    cuts = op.block_jacobi_partition()
    minv = np.zeros_like(dense)
    for a, b in zip(cuts[:-1], cuts[1:]):
        minv[a:b, a:b] = np.linalg.inv(dense[a:b, a:b])
    rng = np.random.default_rng(5)
    rhs = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    x0, it0, h0 = linalg_ref.solve_gmres(lambda v: dense @ v, rhs, tol=1e-8, max_num_iter=600)
    x1, it1, h1 = linalg_ref.solve_gmres(lambda v: dense @ v, rhs, tol=1e-8, max_num_iter=600, msolve=lambda v: minv @ v)
    assert h1[-1] <= 1e-8 and it1 < it0, (it0, it1)
    assert np.linalg.norm(dense @ x1 - rhs) <= 1e-6 * np.linalg.norm(rhs)
