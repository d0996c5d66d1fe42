"""Test infrastructure of the complex64 device builder (tests/test_build_c64_cpu.py, tests/test_gpu_build_c64.py): the
thin-leaf block operand and a census of a plan's pieces by the layout the pack kernel has to write."""
from __future__ import annotations

import ctypes as C

import numpy as np

from butterfly_amd import _capi
from butterfly_amd import helm2_structure as hs

from plan_emulator import _view, BF_ITEM_MERGED, BF_ITEM_ROWMAJOR, BF_ITEM_SMALL, BF_PIECE_IDENTITY, BF_PIECE_ROWMAJOR

THIN_ROWS = [1, 2, 3, 4, 5, 7, 40, 70]
THIN_COLS = [3, 20, 130, 300, 1100]
THIN_POINTS = 1600


def thin_leaf_block():
    """One BLOCK of 8 x 5 dense kernel leaves, 132 x 1553, over 1600 points on the unit circle: the row heights put pieces of
    every layout of a complex64 plan side by side (row-major ones of 1 - 4 rows, column-major ones above), the column widths
    give row strides that are padded (3, 130, 300) and a leaf wider than one piece (1100).  Target and source point ranges
    overlap, so the self value and the column weights land in the leaves.  Returns (desc, points)."""
    desc = hs.Desc(dtype=0)
    ch = []
    r0 = 0
    for h in THIN_ROWS:
        c0 = 0
        for w in THIN_COLS:
            node = desc.add(hs.NODE_DENSE, h, w)
            desc.recipe[node] = ("kernel", ("node", c0, c0 + w), ("node", r0, r0 + h))
            ch.append((node, r0, c0))
            c0 += w
        r0 += h
    desc.root = desc.add(hs.NODE_BLOCK, sum(THIN_ROWS), sum(THIN_COLS), ch, hs.BF_TYPE_BLOCK_DENSE)
    return desc, hs.circle_points(THIN_POINTS)


def thin_leaf_problem():
    """The decorations the thin-leaf block is built with: S' with the points as normals, random column weights, a self value."""
    _, pts = thin_leaf_block()
    w = 0.5 + np.random.default_rng(14).random(THIN_POINTS)
    return dict(layer_pot="Sp", normals=pts, col_weights=w, self_value=0.5 - 0.25j)


def piece_census(op):
    """The forward plan's dense pieces of a FLAG_PLAN_ONLY operator: (number of stages, storage dtype, {kind: [(rows, ncols,
    ld)]}) with kind in plain / merged / rowmajor / small (the item's layout; small items are row-major ones that run four
    to a wavefront)."""
    lib = _capi.load()
    info = _capi.BfhipPlanInfo()
    info.structSize = C.sizeof(info)
    _capi.check(lib.bfhipPlanGetInfo(op.handle, C.byref(info)))
    out = {"plain": [], "merged": [], "rowmajor": [], "small": []}
    for s in range(int(info.numStages)):
        sv = _capi.BfhipStageView()
        sv.structSize = C.sizeof(sv)
        _capi.check(lib.bfhipPlanGetStage(op.handle, s, C.byref(sv)))
        items = _view(sv.items, int(sv.numItems), _capi.ITEM_DTYPE)
        pieces = _view(sv.pieces, int(sv.numPieces), _capi.PIECE_DTYPE)
        for it in items:
            fl = int(it["mrFlags"])
            kind = "small" if fl & BF_ITEM_SMALL else "rowmajor" if fl & BF_ITEM_ROWMAJOR else "merged" if fl & BF_ITEM_MERGED else "plain"
            for pc in pieces[int(it["pieceBegin"]):int(it["pieceBegin"]) + int(it["numPieces"])]:
                if int(pc["flags"]) & BF_PIECE_IDENTITY:
                    continue
                assert bool(int(pc["flags"]) & BF_PIECE_ROWMAJOR) == (kind in ("rowmajor", "small"))
                out[kind].append((fl & 0xFFFF, int(pc["ncols"]), int(pc["ld"])))
    return int(info.numStages), int(info.dtype), out
