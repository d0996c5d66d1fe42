"""Test infrastructure: a catalogue of small operands that together reach every stage and reduce kernel of the apply path
(BfhipKernelId, include/bfhip.h) at the edges where such kernels go wrong.

A case is a seeded real (F64) structure with values; `materialize(case, dtype)` turns it into the operand of any element
type: F64 as built, F32 by demotion, C128 by adding an imaginary part, C64 by demoting that.  Leaves are standard normal
(scaled): no exact zeros, so the structural dependency set of an output is exactly the set of inputs it reads.

Each case declares, per element type, the kernel ids it exists to reach (`reaches`); tests/test_kernel_coverage_cpu.py
checks those and that the union over the catalogue is every id but the ones the dispatch cannot emit (UNREACHABLE)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from butterfly_amd import _capi
from butterfly_amd import helm2_structure as hs
import randgraph

C128, F64, F32, C64 = _capi.BFHIP_C128, _capi.BFHIP_F64, _capi.BFHIP_F32, _capi.BFHIP_C64
DTYPES = (C128, F64, F32, C64)
DTYPE_NAMES = {C128: "c128", F64: "f64", F32: "f32", C64: "c64"}
NRHS_ALL = (1, 2, 3, 16, 17, 32, 33, 64, 65)

# ---- kernel ids (the order of BfhipKernelId) ----------------------------------------------------------------------------
K_C128, K_MFMA1, K_MFMA2, K_MFMA4, K_MFMA1_EXACT, K_MFMA2_EXACT, K_MFMA4_EXACT = range(7)
_REAL_IDX = {F64: 0, F32: 1, C64: 2}


def k_real(dt):
    return 7 + _REAL_IDX[dt]


def k_realboth(dt):
    return 10 + _REAL_IDX[dt]


def k_small(dt):
    return 13 + _REAL_IDX[dt]


def k_t(dt, wide, coop, one):
    return 16 + 8 * (0 if dt == C128 else 1 + _REAL_IDX[dt]) + 4 * bool(wide) + 2 * bool(coop) + bool(one)


def k_tboth(dt, one):
    return 48 + 2 * _REAL_IDX[dt] + bool(one)


def k_reduce(dt, long=False):
    return {C128: 54, F64: 56 if long else 55, F32: 58 if long else 57, C64: 60 if long else 59}[dt]


def k_t_all(dt, wide, coop):
    """both nrhs instantiations (ONE and N) of a transposed kernel"""
    return {k_t(dt, wide, coop, False), k_t(dt, wide, coop, True)}


# ids bfSelectStageKernels cannot emit, with the reason
UNREACHABLE = {
    k_t(C128, False, True, False): "complex128 16-column transposed kernel: the dispatch forces nc = 0 (98 VGPRs with the shared-item code)",
    k_t(C128, False, True, True): "complex128 16-column transposed kernel: the dispatch forces nc = 0 (98 VGPRs with the shared-item code)",
}


@dataclass
class Case:
    name: str
    build: object                   # rng -> (desc (dtype F64), vals)
    seed: int
    nrhs: tuple = (1, 2)
    adjoint: tuple = ("shared", "packed")
    reaches: dict = field(default_factory=dict)     # dtype -> set of kernel ids this case exists to reach
    exact: bool = False             # also run complex128 with FLAG_EXACT_COMPLEX
    absorb: bool = False            # leaves of ones, x of one 1.0 among 2^-25 entries (see draw_x)


# ---- structures ---------------------------------------------------------------------------------------------------------
def _leaf(d, vals, rng, m, n):
    k = d.add(hs.NODE_DENSE, m, n)
    vals[k] = rng.standard_normal((m, n)) / np.sqrt(n) + np.sign(rng.standard_normal((m, n))) * 1e-3   # never exactly 0
    return k


def column(heights, width, identity=False):
    """A block column: leaves heights[i] x width stacked.  Transposed, an item is <= 64 (wide) or <= 16 (narrow: tall leaves)
    columns with one piece per leaf -- few-row leaves are row-major pieces.  identity: an Identity term on every few-row
    block row (an identity piece in the item's chain)."""
    def build(rng):
        d = hs.Desc(dtype=1)
        vals, ch, r0 = {}, [], 0
        for i, h in enumerate(heights):
            ch.append((_leaf(d, vals, rng, h, width), r0, 0))
            if identity and h <= 8:
                c0 = (5 * i) % (width - h + 1)
                ch.append((d.add(hs.NODE_IDENTITY, h, h), r0, c0))
            r0 += h
        d.root = d.add(hs.NODE_BLOCK, r0, width, ch, hs.BF_TYPE_BLOCK_COO if identity else hs.BF_TYPE_BLOCK_DENSE)
        return d, vals
    return build


def wide_row(rows, sources):
    """One rows x (1024 sources) leaf: forward, each row is a reduce list of `sources` partial sums (one per 1024-column task)."""
    def build(rng):
        d = hs.Desc(dtype=1)
        vals = {}
        d.root = _leaf(d, vals, rng, rows, 1024 * sources)
        return d, vals
    return build


def diag(shapes):
    """BlockDiag of leaves of the given (rows, cols): forward items of few rows and < 384 columns are small."""
    def build(rng):
        d = hs.Desc(dtype=1)
        vals, ch, r0, c0 = {}, [], 0, 0
        for m, n in shapes:
            ch.append((_leaf(d, vals, rng, m, n), r0, c0))
            r0 += m; c0 += n
        d.root = d.add(hs.NODE_BLOCK, r0, c0, ch, hs.BF_TYPE_BLOCK_DIAG)
        return d, vals
    return build


def random_graph(seed, depth):
    def build(rng):
        d, v = randgraph.random_operand(np.random.default_rng(seed), depth=depth, cplx=False)
        return d, {k: a + np.sign(a) * 1e-3 for k, a in v.items()}      # shift away from 0
    return build


def materialize(case, dtype):
    """(desc, vals, demote) of `case` as an operand of element type `dtype`."""
    rng = np.random.default_rng(case.seed)
    desc, vals = case.build(rng)
    if case.absorb:
        vals = {k: np.ones_like(v) for k, v in vals.items()}
    if dtype in (C128, C64):
        c = hs.Desc(dtype=0)
        for k in range(desc.num_nodes):
            c.add(desc.kind[k], desc.rows[k], desc.cols[k], list(desc.children[k]), desc.block_kind[k])
        c.root = desc.root
        irng = np.random.default_rng(case.seed + 1000)
        vals = {k: v + 1j * (irng.standard_normal(v.shape) / np.sqrt(v.shape[1]) + np.sign(irng.standard_normal(v.shape)) * 1e-3)
                for k, v in vals.items()}
        if case.absorb:
            vals = {k: np.ones(v.shape) + 0.5j for k, v in vals.items()}
        desc = c
    return desc, vals, dtype in (F32, C64)


# ---- the catalogue ------------------------------------------------------------------------------------------------------
def _t_narrow(dts, coop):
    return {dt: k_t_all(dt, False, coop and dt != C128) for dt in dts}


def _t_wide(dts, coop):
    return {dt: k_t_all(dt, True, coop) for dt in dts}


def _union(*ds):
    out = {}
    for d in ds:
        for k, v in d.items():
            out.setdefault(k, set()).update(v)
    return out


REAL = (F64, F32, C64)


def _cases():
    cs = []
    # transposed item widths: a block column of ten tall leaves `w` columns wide, cut into narrow items of <= 16 columns
    # (17 = 16 + 1, 63 = 3 x 16 + 15); the leading items that stream >= 32 KiB in >= 8 pieces on average are shared (coop)
    # -- not a 1-column item (600 rows), and never on complex128's narrow kernel
    for w in (1, 15, 16, 17, 63, 64):
        cs.append(Case(f"tall_column_w{w}", column([60] * 10, w), 100 + w, nrhs=(1, 3), reaches=_t_narrow(DTYPES, coop=w >= 15)))
    # coop thresholds (64-column items of few-row pieces, 8-byte elements: 32 KiB = 64 rows): exactly 64 rows in 8 pieces
    # (shared), 63 rows in 8 pieces (alone: bytes), 70 rows in 7 pieces (alone: pieces)
    cs.append(Case("coop_bytes_at", column([8] * 8, 64), 201, nrhs=(1, 2), reaches=_t_wide((F64, C64), coop=True)))
    cs.append(Case("coop_bytes_below", column([8] * 7 + [7], 64), 202, nrhs=(1, 2), reaches=_t_wide((F64, C64), coop=False)))
    cs.append(Case("coop_pieces_below", column([10] * 7, 64), 203, nrhs=(1, 2), reaches=_t_wide((F64, C64), coop=False)))
    # long chains: > 64 pieces per item (the 64-piece window loop), piece counts not a multiple of 4, an odd number of
    # row-major pieces between identity pieces (the dual-piece step)
    rng = np.random.default_rng(7)
    cs.append(Case("coop_chain_97", column([int(h) for h in rng.integers(1, 9, 97)], 130), 204, nrhs=(1, 17, 65),
                   reaches=_t_wide(DTYPES, coop=True)))
    cs.append(Case("coop_chain_67_identity", column([int(h) for h in rng.integers(1, 9, 67)], 100, identity=True), 205,
                   nrhs=(1, 2, 33), reaches=_t_wide(DTYPES, coop=True)))
    cs.append(Case("coop_chain_9_odd", column([3, 5, 1, 7, 2, 8, 4, 6, 3], 80, identity=True), 206, nrhs=(1, 16),
                   reaches=_union(_t_wide(REAL, coop=False), _t_wide((C128,), coop=True))))      # 39 rows: 40 KiB at 16 bytes
    # few-row column next to tall leaves: narrow and wide items in one stage (TBoth; complex128 wide coop)
    cs.append(Case("few_row_with_tall", column([3, 7, 100, 2, 5, 1, 8, 130] + [int(h) for h in rng.integers(1, 9, 60)], 90), 207,
                   nrhs=(1, 3), reaches=_union({dt: {k_tboth(dt, False), k_tboth(dt, True)} for dt in REAL},
                                               {C128: k_t_all(C128, True, True) | k_t_all(C128, False, False)})))
    # F32 pieces of ncols 1, 2, 3, 5 (four elements per lane): forward small items and transposed tall columns
    for n in (1, 2, 3, 5):
        cs.append(Case(f"f32_ncols{n}", diag([(2, n), (3, n), (1, n), (4, n)] * 3), 300 + n, nrhs=(1, 2),
                       reaches={dt: {k_small(dt)} for dt in REAL}))
    # forward real family: stages of only ordinary items, only small items, both
    cs.append(Case("forward_ordinary_only", diag([(64, 70), (40, 300)]), 401, nrhs=(1, 2, 17),
                   reaches={dt: {k_real(dt)} for dt in REAL}))
    cs.append(Case("forward_small_only", diag([(2, 40), (3, 100), (1, 7), (4, 200)] * 5), 402, nrhs=(1, 2),
                   reaches={dt: {k_small(dt)} for dt in REAL}))
    cs.append(Case("forward_both", diag([(64, 70), (2, 40), (3, 100), (40, 300), (1, 7)]), 403, nrhs=(1, 2),
                   reaches={dt: {k_realboth(dt)} for dt in REAL}))
    # reduce lists of s partial sums (a row of 1024 s columns); >= 64: the long-list kernel
    for s in (31, 32, 33, 63, 64, 65, 97):
        cs.append(Case(f"reduce_{s}", wide_row(4 if s > 60 else 8, s), 500 + s, nrhs=(1, 2), adjoint=("shared",),
                       reaches={dt: {k_reduce(dt, s >= 64 and dt != C128)} for dt in DTYPES}))
    # absorption: every term but one is below half an ulp of that one in float -- a float accumulator that has taken it in
    # drops the rest, a double one (complex64's, Traits<C64>::A and the reduce's TA) keeps them.  The componentwise bound
    # of tests/highprec.py for C64 tells the two apart; random data would not (float rounding errors of random sign
    # stay within it on chains of a few hundred terms)
    cs.append(Case("absorb_reduce_33", wide_row(8, 33), 533, nrhs=(1, 2), adjoint=("shared",), absorb=True,
                   reaches={dt: {k_reduce(dt)} for dt in DTYPES}))
    cs.append(Case("absorb_chain_70", column([8] * 70, 64), 534, nrhs=(1, 2), absorb=True,
                   reaches=_t_wide((F64, C64), coop=True)))
    # complex128 forward: the GEMV kernel and the matrix-core kernels of 1, 2 and 4 RHS tiles, with and without
    # FLAG_EXACT_COMPLEX, at every tile edge
    cs.append(Case("mfma_tiles", random_graph(4, 4), 600, nrhs=NRHS_ALL, adjoint=("packed",), exact=True,
                   reaches={C128: {K_C128, K_MFMA1, K_MFMA2, K_MFMA4, K_MFMA1_EXACT, K_MFMA2_EXACT, K_MFMA4_EXACT}}))
    # random expression graphs: products of blocks of products, identity leaves, ragged sizes
    cs.append(Case("randgraph5", random_graph(5, 4), 601, nrhs=(1, 3), reaches={}))
    cs.append(Case("randgraph1", random_graph(1, 4), 602, nrhs=(1, 2), reaches={}))
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def flag_sets(case, dtype):
    """The compile flags a case runs under for `dtype`: one per adjoint mode (+ FLAG_EXACT_COMPLEX for complex128)."""
    out = []
    for a in case.adjoint:
        f = _capi.FLAG_ADJOINT if a == "shared" else _capi.FLAG_ADJOINT_PACKED
        out.append(f)
        if case.exact and dtype == C128:
            out.append(f | _capi.FLAG_EXACT_COMPLEX)
    return out


STORAGE_NP = {C128: np.complex128, F64: np.float64, F32: np.float32, C64: np.complex64}


def draw_x(case, dtype, rows, nrhs, rng):
    """A test input: standard normal (complex for complex operands); for `absorb` cases real, 1.0 in row 0 (where a
    contraction is likely to start) and 2^-25 elsewhere -- exact in every element type."""
    if case.absorb:
        x = np.full((rows, nrhs), 2.0 ** -25)
        x[0] = 1.0
        return x + 0j if dtype in (C128, C64) else x
    x = rng.standard_normal((rows, nrhs))
    if dtype in (C128, C64):
        x = x + 1j * rng.standard_normal((rows, nrhs))
    return x
