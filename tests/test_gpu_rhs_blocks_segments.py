"""The segment builder of the forward block kernels (bfBlkSegment, butterfly_amd/csrc/bfhip_stage_mfma_blocks.h) on leaves wider
than its LDS table of 768 columns, F64, F32 and complex64, switch on, nrhs 2, 17 and 65.

The planner (seen with FLAG_PLAN_ONLY; `_check_plan` asserts it before any result is looked at) cuts an item's columns at 1024
per task and a column-major leaf into pieces of 256 columns, so a single piece wider than the table exists only row-major (leaves
of <= 4 rows; <= 8 in F32), it is at most 1024 columns wide, and is cut once, not twice.  The operands:

* `few_rows`: a 3 x 1000 leaf: ONE row-major piece of 1000 columns: a segment of 768 and, with pj = 768, one of 232;
* `few_rows_tasks`: a 5 x 1600 leaf: two tasks (1024 + 576 columns) and a reduce; F32 has a row-major piece of 1024 columns,
  F64 and complex64 four column-major pieces that fill the table exactly at a piece boundary;
* `mid_piece`: a block row of a 40 x 100 and a 40 x 800 leaf: column-major pieces of 100, 256, 256, 256 and 32 columns in one item:
  the table is full 156 columns into the fourth piece (pj = 156).  F32 keeps the 40 rows in one item: a pass of two slabs, then
  one of one; F64 and complex64 items have at most 32 rows (items of 32 and 8);
* `two_level`: [A | B C] with A 3 x 800, B 3 x 200, C 200 x 6: the item of the last stage reads A's rows from x and B's from the
  vector arena: the input base changes between segments, after A's piece was cut at 768.

Leaf entries and x are integers in -3..3 (both components of complex ones), so every product, every Gauss sum and every partial
sum is an integer below 2^24: exact in float and in double whatever the order of summation, and so is every stored intermediate.
The expectation is the exact product from numpy; the assertion is bit equality, switch on and switch off."""
import ctypes as C
import functools

import numpy as np
import pytest

from butterfly_amd import _capi, helm2_structure as hs
import kernel_catalogue as kc
import randgraph

pytestmark = pytest.mark.gpu

NRHS = (2, 17, 65)
DTYPES = (kc.F64, kc.F32, kc.C64)
TABCAP = 768                      # BF_M64_TABCAP
IN_X, IDENTITY, ROWMAJOR = 1, 2, 4
OPERANDS = ("few_rows", "few_rows_tasks", "mid_piece", "two_level")


def _ints(rng, shape, cplx):
    v = rng.integers(-3, 4, size=shape).astype(np.float64)
    return v + 1j * rng.integers(-3, 4, size=shape) if cplx else v


@functools.lru_cache(maxsize=None)
def _operand(name, dtype):
    """(desc, vals, demote, dense) with dense the exact matrix"""
    cplx = dtype == kc.C64
    rng = np.random.default_rng(len(name) + 10 * dtype)
    d, vals = hs.Desc(dtype=0 if cplx else 1), {}

    def leaf(m, n):
        k = d.add(hs.NODE_DENSE, m, n)
        vals[k] = _ints(rng, (m, n), cplx)
        return k
    if name == "few_rows":
        d.root = leaf(3, 1000)
    elif name == "few_rows_tasks":
        d.root = leaf(5, 1600)
    elif name == "mid_piece":
        d.root = d.add(hs.NODE_BLOCK, 40, 900, [(leaf(40, 100), 0, 0), (leaf(40, 800), 0, 100)], hs.BF_TYPE_BLOCK_DENSE)
    else:
        bc = d.add(hs.NODE_PRODUCT, 3, 6, [(leaf(3, 200), 0, 0), (leaf(200, 6), 0, 0)])
        d.root = d.add(hs.NODE_BLOCK, 3, 806, [(leaf(3, 800), 0, 0), (bc, 0, 800)], hs.BF_TYPE_BLOCK_DENSE)
    return d, vals, dtype in (kc.F32, kc.C64), randgraph.densify(d, vals, d.root)


def _switch(dtype):
    return {"rhs_blocks": 2} if dtype == kc.C64 else {"real_rhs_blocks": 2}


def _forward_items(op):
    """per forward stage the list of items as (mr, [(ncols, flags) of its pieces])"""
    lib = _capi.load()
    info = _capi.BfhipPlanInfo()
    info.structSize = C.sizeof(info)
    _capi.check(lib.bfhipPlanGetInfo(op.handle, C.byref(info)))
    out = []
    for s in range(int(info.numStages)):
        sv = _capi.BfhipStageView()
        sv.structSize = C.sizeof(sv)
        _capi.check(lib.bfhipPlanGetStage(op.handle, s, C.byref(sv)))
        items = np.frombuffer(bytes((C.c_char * (int(sv.numItems) * 16)).from_address(sv.items)), dtype=_capi.ITEM_DTYPE)
        pieces = np.frombuffer(bytes((C.c_char * (int(sv.numPieces) * 24)).from_address(sv.pieces)), dtype=_capi.PIECE_DTYPE)
        out.append([(int(it["mrFlags"]) & 0xFFFF, [(int(p["ncols"]), int(p["flags"])) for p in pieces[it["pieceBegin"]:it["pieceBegin"] + it["numPieces"]]])
                    for it in items])
    return out


@functools.lru_cache(maxsize=None)
def _check_plan(name, dtype):
    """The operand reaches the path it is here for -- asserted on the plan, before any result."""
    from butterfly_amd.operator import HipOperator
    desc, vals, demote, _ = _operand(name, dtype)
    op = HipOperator.from_desc(desc, vals, flags=_capi.FLAG_PLAN_ONLY, demote_to_f32=demote, **_switch(dtype))
    stages = _forward_items(op)
    first = {kc.C64: 64, kc.F64: 72, kc.F32: 75}[dtype]
    for nrhs in NRHS:
        ks = op.stage_kernels(nrhs)[:len(stages)]
        want = first + (0 if nrhs <= 16 else 1 if nrhs <= 32 else 2)
        assert all(k and k[0] == want for k in ks), (nrhs, ks)      # (a reduce kernel may follow)
    op.close()
    items = [it for st in stages for it in st]
    dense = lambda ps: [(n, f) for n, f in ps if not f & IDENTITY]
    assert any(sum(n for n, _ in dense(ps)) > TABCAP for _, ps in items), items         # an item of more than one table
    if name == "few_rows" or (name == "few_rows_tasks" and dtype == kc.F32):
        assert any(n > TABCAP and f & ROWMAJOR for _, ps in items for n, f in ps), items   # a dense piece wider than the table
    if name == "few_rows_tasks":
        assert len(items) == 2 and not (dtype != kc.F32 and any(f & ROWMAJOR for _, ps in items for _, f in ps)), items
    if name == "mid_piece":
        cut = False
        for mr, ps in items:
            edges = np.cumsum([n for n, _ in dense(ps)])
            cut = cut or (edges[-1] > TABCAP and TABCAP not in edges and not any(f & ROWMAJOR for _, f in ps))
        assert cut, items                                                                  # the table fills inside a piece
        assert dtype != kc.F32 or any(32 < mr <= 48 for mr, _ in items), items             # two slabs, then one
    if name == "two_level":
        assert any(len({f & IN_X for _, f in dense(ps)}) == 2 and dense(ps)[0][0] > TABCAP for _, ps in items), items


def _torch_dtype(dtype):
    import torch
    return {kc.F64: torch.float64, kc.F32: torch.float32, kc.C64: torch.complex64}[dtype]


def _device_apply(op, x, dtype):
    import torch
    xd = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    yd = torch.full((op.shape[0], x.shape[1]), float("nan"), dtype=_torch_dtype(dtype), device="cuda:0")
    op.apply_device(xd, yd)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=[kc.DTYPE_NAMES[d] for d in DTYPES])
@pytest.mark.parametrize("name", OPERANDS)
def test_cut_segments_give_the_exact_product(name, dtype):
    from butterfly_amd.operator import HipOperator
    _check_plan(name, dtype)
    desc, vals, demote, dense = _operand(name, dtype)
    st = kc.STORAGE_NP[dtype]
    op = HipOperator.from_desc(desc, vals, max_rhs=max(NRHS), demote_to_f32=demote, device=0, **_switch(dtype))
    plain = HipOperator.from_desc(desc, vals, max_rhs=max(NRHS), demote_to_f32=demote, device=0)
    try:
        rng = np.random.default_rng(7)
        for nrhs in NRHS:
            x = _ints(rng, (dense.shape[1], nrhs), dtype == kc.C64)
            want = dense @ x
            assert np.abs(want.real).max() < 2 ** 24 and np.abs(want.imag).max() < 2 ** 24
            want = want.astype(st)
            y = _device_apply(op, x.astype(st), dtype)
            bad = y.view(np.uint8) != want.view(np.uint8)
            assert not bad.any(), f"nrhs {nrhs}, switch on: {int((y != want).sum())} of {y.size} outputs are not the exact product"
            y0 = _device_apply(plain, x.astype(st), dtype)
            assert np.array_equal(y0.view(np.uint8), want.view(np.uint8)), f"nrhs {nrhs}, switch off: {int((y0 != want).sum())} outputs differ"
    finally:
        op.close(); plain.close()
