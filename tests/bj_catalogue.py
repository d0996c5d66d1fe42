"""Test infrastructure: a catalogue of designed operands for the block-Jacobi kernels (bfhip_precond.hip), in the style of
tests/kernel_catalogue.py.  Every case is seeded and materialises to an operand of any element type it declares.

* INVERSION: BlockDiag operators of many dense leaves of mixed sizes (one inversion launch over all of them; the automatic
  cuts are the leaves, so nothing but dense values enters a block and scaling the values by 2^k scales the inverses by 2^-k
  exactly).  Designed condition numbers, permutations (a swap at every step, exact), dyadic / unimodular blocks whose
  elimination is exact, pivot-key ties and |re| + |im| against modulus orders, a growth-prone block, triangular blocks, the
  identity, and 2^+-600 copies.
* REFUSAL: blocks of exactly representable values that the inversion must refuse, with the block and the step it reports.
* GATHER: operands whose direct pieces meet user cuts in every way the host's task builder distinguishes.

`seen(vals, dtype)` is what the kernels read: the values rounded to the storage type."""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from butterfly_amd import _capi
from butterfly_amd import helm2_structure as hs

C128, F64, F32, C64 = _capi.BFHIP_C128, _capi.BFHIP_F64, _capi.BFHIP_F32, _capi.BFHIP_C64
DTYPES = (C128, C64, F64, F32)
DTYPE_NAMES = {C128: "c128", F64: "f64", F32: "f32", C64: "c64"}
STORAGE_NP = {C128: np.complex128, F64: np.float64, F32: np.float32, C64: np.complex64}
WORK_NP = {C128: np.complex128, C64: np.complex128, F64: np.float64, F32: np.float64}      # the working copy's type
DEMOTED = {C128: C64, F64: F32}
SIZES = (1, 2, 3, 5, 7, 8, 9, 16, 17, 63, 64, 65, 100, 127, 128, 129)        # every condition case; + one of 200, 255, 256


def is_complex(dtype):
    return dtype in (C128, C64)


def seen(v, dtype):
    """v as the engine stores it, widened back to the working type."""
    v = np.asarray(v, dtype=WORK_NP[dtype])
    return v.astype(STORAGE_NP[dtype]).astype(WORK_NP[dtype])


# ---- inversion cases ----------------------------------------------------------------------------------------------------
@dataclass
class InvCase:
    name: str
    build: object                   # (rng, cplx) -> [(block, exact inverse or None)]
    seed: int
    dtypes: tuple = DTYPES
    exact: bool = False             # every block has an exactly representable inverse the kernel must hit bit for bit
    scale_of: tuple = None          # (base case name, k): the base case's blocks times 2^k
    demote: bool = True             # also build the complex64 / float32 result from the double-precision operand


def _unitary(rng, m, cplx):
    z = rng.standard_normal((m, m))
    if cplx:
        z = z + 1j * rng.standard_normal((m, m))
    q, r = np.linalg.qr(z)
    return q


def designed_condition(kappa, sizes):
    """U diag(sigma) V^H, sigma log-spaced from 1 down to 1 / kappa (orthogonal U, V for the real family)."""
    def build(rng, cplx):
        out = []
        for m in sizes:
            sig = np.logspace(0.0, -np.log10(kappa), m) if m > 1 else np.array([0.75])
            out.append(((_unitary(rng, m, cplx) * sig) @ np.conj(_unitary(rng, m, cplx)).T, None))
        return out
    return build


def _units(rng, m, cplx):
    return np.array([1, 1j, -1, -1j])[rng.integers(0, 4, m)] if cplx else np.array([1.0, -1.0])[rng.integers(0, 2, m)]


def _perm_matrix(perm, units):
    m = len(perm)
    b = np.zeros((m, m), dtype=units.dtype)
    b[np.arange(m), perm] = units
    return b


def permutations(rng, cplx):
    """Permutation matrices with unit entries (1, -1 and, complex, +-i): the 2 x 2 exchange, cyclic shifts (zero leading
    diagonal: every step swaps and the exchanges do not commute) and random permutations.  The inverse is the conjugate
    transpose, and every operation of the elimination is exact."""
    out = []
    perms = [np.array([1, 0])]
    perms += [(np.arange(m) + 1) % m for m in (3, 5, 8, 17, 64, 100, 129, 256)]
    perms += [(np.arange(m) - 1) % m for m in (4, 65)]
    perms += [rng.permutation(m) for m in (7, 16, 63, 127, 200)]
    for p in perms:
        b = _perm_matrix(p, _units(rng, len(p), cplx))
        out.append((b, np.conj(b).T.copy()))
    return out


def exact_inverse(b):
    """The inverse of a real block in rational arithmetic; asserts that it is representable in fp64."""
    m = b.shape[0]
    a = [[Fraction(float(v)) for v in row] + [Fraction(int(i == j)) for j in range(m)] for i, row in enumerate(b)]
    for k in range(m):
        p = next(i for i in range(k, m) if a[i][k] != 0)
        a[k], a[p] = a[p], a[k]
        a[k] = [v / a[k][k] for v in a[k]]
        for i in range(m):
            if i != k and a[i][k] != 0:
                f = a[i][k]
                a[i] = [v - f * w for v, w in zip(a[i], a[k])]
    inv = np.array([[float(v) for v in row[m:]] for row in a])
    assert all(Fraction(float(v)) == v for row in a for v in row[m:]), "inverse not representable"
    return inv


def dyadic(rng, cplx):
    """Blocks whose elimination is exact in fp64: P D with D a diagonal of powers of two; the identity; and L U with L unit
    lower triangular with entries in {-1, 0, 1} (column k's candidates are l_ik u_kk: exact ties of the pivot key, which go
    to the smaller row, so no row is exchanged) and U upper triangular with a diagonal of +-1, +-2, +-1/2 and small
    integers above it -- every pivot is a power of two and every intermediate a small dyadic rational."""
    out = []
    for m in (1, 9, 40):
        d = 2.0 ** rng.integers(-30, 31, m) * _units(rng, m, cplx)
        p = rng.permutation(m)
        b = np.zeros((m, m), dtype=d.dtype)
        b[p, np.arange(m)] = d
        inv = np.zeros_like(b)
        inv[np.arange(m), p] = 1.0 / d
        out.append((b, inv))
    for m in (1, 64):
        out.append((np.eye(m) + (0j if cplx else 0.0), np.eye(m) + (0j if cplx else 0.0)))
    for m in (2, 3, 5, 8, 9, 16):
        lo = np.tril(rng.integers(-1, 2, (m, m)) * (rng.random((m, m)) < 0.5), -1) + np.eye(m)
        up = np.triu(rng.integers(-1, 2, (m, m)) * (rng.random((m, m)) < 0.5), 1) + np.diag(rng.choice([1, -1, 2, -2, 0.5, -0.5], m))
        b = lo @ up
        inv = exact_inverse(b)
        out.append((b + 0j, inv + 0j) if cplx else (b, inv))
    return out


# |re| + |im| against the modulus, exact.  [[3, 2+i], [2+2i, 1+2i]] (det 1): column 0 holds 3 (key 3, modulus 3) and 2+2i
# (key 4, modulus 2.83): the kernel's key takes 2+2i, whose scaled reciprocal (1-i)/4 is exact; the modulus order takes 3,
# and 1/3 is not.  [[4, i], [3+i, i]] (det 1+i): 4 and 3+i tie in the key; the smaller row's 1/4 is exact, 1/(3+i) is not.
_K1 = np.array([[3, 2 + 1j], [2 + 2j, 1 + 2j]])
_K1_INV = np.array([[1 + 2j, -2 - 1j], [-2 - 2j, 3]])
_K2 = np.array([[4, 1j], [3 + 1j, 1j]])
_K2_INV = np.array([[0.5 + 0.5j, -0.5 - 0.5j], [-2 + 1j, 2 - 2j]])


def _direct_sum(blocks):
    m = sum(b.shape[0] for b in blocks)
    out = np.zeros((m, m), dtype=np.complex128)
    r = 0
    for b in blocks:
        out[r:r + b.shape[0], r:r + b.shape[0]] = b
        r += b.shape[0]
    return out


def pivot_key_exact(rng, cplx):
    assert cplx
    return [(_K1.copy(), _K1_INV.copy()), (_K2.copy(), _K2_INV.copy()),
            (_direct_sum([_K1, _K2, _K1]), _direct_sum([_K1_INV, _K2_INV, _K1_INV])),
            (_direct_sum([_K2] * 5), _direct_sum([_K2_INV] * 5))]


def pivot_key_generic(rng, cplx):
    """Random complex blocks whose entries lie on the real axis or on the diagonal re = im, moduli close together: in most
    columns the largest |re| + |im| and the largest modulus are different rows."""
    assert cplx
    out = []
    for m in (6, 31, 70):
        r = 1.0 + 0.2 * rng.random((m, m))
        th = np.where(rng.random((m, m)) < 0.5, 0.0, np.pi / 4) + 0.01 * rng.standard_normal((m, m))
        out.append((r * np.exp(1j * th) * np.sign(rng.standard_normal((m, m))), None))
    return out


def growth(rng, cplx):
    """Wilkinson's growth matrix (1 on the diagonal and in the last column, -1 below the diagonal: no exchanges, the last
    column doubles at every step, g = 2^(m-1)), plain and with a small perturbation below the diagonal."""
    out = []
    for m, eps in ((8, 0.0), (24, 1e-3), (54, 0.0), (40, 1e-3)):
        b = np.eye(m) - np.tril(np.ones((m, m)), -1) + np.tril(eps * rng.random((m, m)), -1)
        b[:, -1] = 1.0
        out.append((b * _units(rng, m, True)[None, :] if cplx else b, None))
    return out


def triangular(rng, cplx):
    out = []
    for m, upper in ((33, True), (20, False), (130, True)):
        z = rng.standard_normal((m, m)) / np.sqrt(m)
        if cplx:
            z = z + 1j * rng.standard_normal((m, m)) / np.sqrt(m)
        z = np.triu(z, 1) if upper else np.tril(z, -1)
        out.append((z + np.diag(1.0 + rng.random(m)), None))
    return out


BIG = {1.0: 256, 1e3: 200, 1e6: 255, 1e10: 256}
SCALE_SIZES = (1, 2, 5, 8, 17, 64, 65)
INVERSION = [InvCase(f"cond_1e{int(np.log10(k))}", designed_condition(k, SIZES + (BIG[k],)), 10 + i) for i, k in enumerate(BIG)]
INVERSION += [
    InvCase("permutations", permutations, 20, exact=True),
    InvCase("dyadic", dyadic, 21, exact=True),
    InvCase("pivot_key_exact", pivot_key_exact, 22, dtypes=(C128, C64), exact=True),
    InvCase("pivot_key_generic", pivot_key_generic, 23, dtypes=(C128, C64)),
    InvCase("growth", growth, 24),
    InvCase("triangular", triangular, 25),
    InvCase("scale_base", designed_condition(1e3, SCALE_SIZES), 26, dtypes=(C128, F64)),
    InvCase("scale_up_600", None, 26, dtypes=(C128, F64), scale_of=("scale_base", 600), demote=False),
    InvCase("scale_down_600", None, 26, dtypes=(C128, F64), scale_of=("scale_base", -600), demote=False),      # 2^600 is no float
]
INV_BY_NAME = {c.name: c for c in INVERSION}


def out_types(case, dtype):
    """The result types a `dtype` operand of the case is built to: its own and, from a double-precision one, the demotion."""
    return [dtype] + ([DEMOTED[dtype]] if dtype in DEMOTED and getattr(case, "demote", True) else [])


def inv_blocks(case, dtype):
    """[(block as the kernel reads it, exact inverse or None)] of an inversion or refusal case for `dtype`."""
    if getattr(case, "scale_of", None):
        base, k = case.scale_of
        return [(b * 2.0 ** k, None if x is None else x * 2.0 ** -k) for b, x in inv_blocks(INV_BY_NAME[base], dtype)]
    raw = case.build(np.random.default_rng(case.seed), is_complex(dtype))
    out = []
    for b, x in raw:
        s = seen(b, dtype)
        assert x is None or np.array_equal(s, np.asarray(b, dtype=WORK_NP[dtype]), equal_nan=True), case.name      # exact cases survive the storage type
        out.append((s, None if x is None else np.asarray(x, dtype=WORK_NP[dtype])))
    return out


def block_diag_operand(blocks, dtype):
    """(desc, vals, demote, cuts) of the BlockDiag of `blocks` (dense leaves) in element type `dtype`."""
    d = hs.Desc(dtype=0 if is_complex(dtype) else 1)
    vals, ch, r = {}, [], 0
    for b in blocks:
        m = b.shape[0]
        leaf = d.add(hs.NODE_DENSE, m, m)
        vals[leaf] = np.asarray(b, dtype=WORK_NP[dtype])
        ch.append((leaf, r, r))
        r += m
    d.root = d.add(hs.NODE_BLOCK, r, r, ch, hs.BF_TYPE_BLOCK_DIAG)
    return d, vals, dtype in (F32, C64), np.concatenate([[0], np.cumsum([b.shape[0] for b in blocks])])


# ---- refusal cases --------------------------------------------------------------------------------------------------------
@dataclass
class RefusalCase:
    name: str
    build: object                   # (rng, cplx) -> [(block, None)]
    seed: int
    block: int                      # the first block the inversion refuses
    step: int                       # and the step it reports
    dtypes: tuple = (C128, F64)


def _good(rng, m):
    """A small integer block that inverts (diagonally dominant)."""
    return rng.integers(-2, 3, (m, m)).astype(np.float64) + np.diag(np.full(m, 4.0 * m))


def rank_deficient(m, k):
    """L U with unit lower triangular L ({-1, 0, 1} below the diagonal) and integer upper triangular U whose diagonal is +-1
    before k and 0 at k: integer arithmetic throughout, column k is exactly zero at and below the diagonal at step k and
    nowhere earlier."""
    def make(rng):
        lo = np.tril(rng.integers(-1, 2, (m, m)), -1) + np.eye(m)
        up = np.triu(rng.integers(-2, 3, (m, m)), 1) + np.diag(rng.choice([1.0, -1.0], m))
        up[k, k] = 0.0
        return lo @ up
    return make


def _among(make, position, count=5, m_good=6):
    """`make(rng)` at `position` among `count` blocks, the others invertible."""
    def build(rng, cplx):
        out = [_good(rng, m_good + i) for i in range(count)]
        out[position] = make(rng)
        return [(b + 0j if cplx else b, None) for b in out]
    return build


def _poison(pos, value):
    def make(rng):
        b = _good(rng, 4)
        b[pos] = value
        return b
    return make


def _complex_block(b):
    def build(rng, cplx):
        assert cplx
        return [(_good(rng, 3) + 0j, None), (np.asarray(b, dtype=np.complex128), None), (_good(rng, 5) + 0j, None)]
    return build


def _both_deficient(rng, cplx):
    out = [_good(rng, 5), rank_deficient(7, 4)(rng), _good(rng, 3), rank_deficient(6, 1)(rng)]
    return [(b + 0j if cplx else b, None) for b in out]


HUGE = 1.5 * 2.0 ** 1023            # finite; hypot(HUGE, HUGE) overflows
SUB = 2.0 ** -1074                  # the smallest subnormal: finite, non-zero, 1 / SUB overflows
REFUSAL = [
    RefusalCase("deficient_step0_first", _among(rank_deficient(6, 0), 0), 40, 0, 0),
    RefusalCase("deficient_step3_middle", _among(rank_deficient(9, 3), 2), 41, 2, 3),
    RefusalCase("deficient_last_step_last", _among(rank_deficient(8, 7), 4), 42, 4, 7),
    RefusalCase("deficient_m17_step16", _among(rank_deficient(17, 16), 1), 43, 1, 16),
    RefusalCase("two_deficient_blocks", _both_deficient, 44, 1, 4),
    # a NaN or infinity is taken as the pivot of its column (key = infinity) when it sits at or below the diagonal at that
    # step; above the diagonal it is in a pivot row first, which the scaled-row test refuses at that row's step
    RefusalCase("nan_below_diagonal", _among(_poison((3, 0), np.nan), 1), 45, 1, 0),
    RefusalCase("nan_on_diagonal", _among(_poison((1, 1), np.nan), 3), 46, 3, 1),
    RefusalCase("nan_above_diagonal", _among(_poison((0, 2), np.nan), 2), 47, 2, 0),
    RefusalCase("inf_below_diagonal", _among(_poison((2, 1), np.inf), 0), 48, 0, 1),
    RefusalCase("inf_on_diagonal", _among(_poison((3, 3), -np.inf), 4), 49, 4, 3),
    RefusalCase("inf_above_diagonal", _among(_poison((1, 3), np.inf), 2), 50, 2, 1),
    RefusalCase("hypot_overflow", _complex_block(np.diag([1.0, HUGE * (1 + 1j), 1.0])), 51, 1, 1, dtypes=(C128,)),
    RefusalCase("subnormal_1x1", _among(lambda rng: np.array([[SUB]]), 2), 52, 2, 0),
    RefusalCase("subnormal_inside", _among(lambda rng: np.diag([1.0, 1.0, SUB, 1.0]), 3), 53, 3, 2),
    RefusalCase("subnormal_complex", _complex_block(np.diag([1.0, 1.0, SUB * (1 - 1j)])), 54, 1, 2, dtypes=(C128,)),
    # a finite reciprocal (2^1000) and a finite row whose product overflows
    RefusalCase("scaled_row_overflow", _among(lambda rng: np.array([[2.0 ** -1000, 2.0 ** 100], [0.0, 1.0]]), 1), 55, 1, 0),
]
REF_BY_NAME = {c.name: c for c in REFUSAL}


# ---- gather cases ---------------------------------------------------------------------------------------------------------
@dataclass
class GatherCase:
    name: str
    build: object                   # rng -> (desc (dtype F64), vals)
    seed: int
    cuts: object = None             # None: automatic
    max_block: int = 128
    product: bool = False           # a product overlaps a diagonal block (and is left out)


def _leaf(d, vals, rng, m, n):
    k = d.add(hs.NODE_DENSE, m, n)
    vals[k] = rng.standard_normal((m, n)) / np.sqrt(n) + np.sign(rng.standard_normal((m, n))) * 1e-3       # never exactly 0
    return k


def dense_2x2(rng):
    d, vals = hs.Desc(dtype=1), {}
    ch = [(_leaf(d, vals, rng, 40, 40), r, c) for r in (0, 40) for c in (0, 40)]
    d.root = d.add(hs.NODE_BLOCK, 80, 80, ch, hs.BF_TYPE_BLOCK_DENSE)
    return d, vals


SMALL_LEAVES = (3, 8, 1, 5, 2, 7, 1, 2, 3, 5, 4, 6, 8, 1)


def small_leaves(rng):
    """Square leaves of <= 8 rows (row-major pieces), the column counts 1, 2, 3, 5 among them."""
    d, vals, ch, r = hs.Desc(dtype=1), {}, [], 0
    for m in SMALL_LEAVES:
        ch.append((_leaf(d, vals, rng, m, m), r, r))
        r += m
    d.root = d.add(hs.NODE_BLOCK, r, r, ch, hs.BF_TYPE_BLOCK_DIAG)
    return d, vals


def wide_first_row(rng):
    """n = 2048: a 64 x 2048 leaf over the first 64 rows (forward, two 1024-column tasks whose partial sums a y-reduce
    adds), then 31 diagonal leaves of 64 x 64."""
    d, vals = hs.Desc(dtype=1), {}
    ch = [(_leaf(d, vals, rng, 64, 2048), 0, 0)]
    ch += [(_leaf(d, vals, rng, 64, 64), r, r) for r in range(64, 2048, 64)]
    d.root = d.add(hs.NODE_BLOCK, 2048, 2048, ch, hs.BF_TYPE_BLOCK_COO)
    return d, vals


WIDE_CUTS = np.concatenate([[0, 256, 320, 448, 640, 896], np.arange(960, 2049, 64)])       # blocks of 64 ... 256 rows


def coo_identity(rng):
    """n = 48: an identity leaf on rows 0..9 of the diagonal, a dense 16 x 16 leaf on rows 4..19 (they overlap on 4..9), an
    identity leaf of 8 rows at (24, 27) -- off the diagonal by 3 -- and nothing else: rows 20..47 are uncovered."""
    d, vals = hs.Desc(dtype=1), {}
    ch = [(d.add(hs.NODE_IDENTITY, 10, 10), 0, 0), (_leaf(d, vals, rng, 16, 16), 4, 4), (d.add(hs.NODE_IDENTITY, 8, 8), 24, 27)]
    d.root = d.add(hs.NODE_BLOCK, 48, 48, ch, hs.BF_TYPE_BLOCK_COO)
    return d, vals


def product_over_diagonal(rng):
    """n = 24: two dense 12 x 12 diagonal leaves and a product (8 x 3)(3 x 24) over rows 2..9, all columns."""
    d, vals = hs.Desc(dtype=1), {}
    a, b = _leaf(d, vals, rng, 12, 12), _leaf(d, vals, rng, 12, 12)
    f1, f0 = _leaf(d, vals, rng, 3, 24), _leaf(d, vals, rng, 8, 3)
    p = d.add(hs.NODE_PRODUCT, 8, 24, [(f0, 0, 0), (f1, 0, 0)])
    d.root = d.add(hs.NODE_BLOCK, 24, 24, [(a, 0, 0), (b, 12, 12), (p, 2, 0)], hs.BF_TYPE_BLOCK_COO)
    return d, vals


GATHER = [
    GatherCase("dense2x2_auto", dense_2x2, 60),
    GatherCase("dense2x2_merged", dense_2x2, 60, cuts=[0, 80]),                        # the off-diagonal leaves land inside the block
    GatherCase("dense2x2_split", dense_2x2, 60, cuts=[0, 13, 40, 57, 58, 80]),         # cuts through the leaves
    GatherCase("small_leaves_auto", small_leaves, 61),
    GatherCase("small_leaves_merged", small_leaves, 61, cuts=[0, 11, 12, 30, sum(SMALL_LEAVES)]),
    GatherCase("wide_first_row", wide_first_row, 62, cuts=WIDE_CUTS, max_block=256),
    GatherCase("coo_identity_auto", coo_identity, 63),
    GatherCase("coo_identity_cut", coo_identity, 63, cuts=[0, 7, 20, 30, 48]),         # the off-diagonal identity straddles 30
    GatherCase("product_auto", product_over_diagonal, 64, product=True),
    GatherCase("product_merged", product_over_diagonal, 64, cuts=[0, 5, 24], product=True),
]
GATHER_BY_NAME = {c.name: c for c in GATHER}


def materialize_gather(case, dtype):
    """(desc, vals, demote) of a gather case as an operand of element type `dtype` (complex: an imaginary part is added)."""
    desc, vals = case.build(np.random.default_rng(case.seed))
    if is_complex(dtype):
        c = hs.Desc(dtype=0)
        for k in range(desc.num_nodes):
            c.add(desc.kind[k], desc.rows[k], desc.cols[k], list(desc.children[k]), desc.block_kind[k])
        c.root = desc.root
        irng = np.random.default_rng(case.seed + 1000)
        vals = {k: v + 1j * (irng.standard_normal(v.shape) / np.sqrt(v.shape[1]) + np.sign(irng.standard_normal(v.shape)) * 1e-3)
                for k, v in vals.items()}
        desc = c
    return desc, vals, dtype in (F32, C64)


def direct_dense(desc, vals, dtype, products=False):
    """The direct part from the descriptor alone, in extended precision: (sum, number of contributions, sum of moduli,
    covered rows).  Dense and identity leaves reached through BLOCK nodes only; with `products` the products are multiplied
    out and added too (the whole operand).  A row is covered when a dense leaf whose rectangle meets the diagonal spans it
    (rows and columns) or a diagonal identity leaf holds it."""
    cplx = is_complex(dtype)
    W = np.clongdouble if cplx else np.longdouble
    n = desc.rows[desc.root]
    total, count, mod = np.zeros((n, n), dtype=W), np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.longdouble)
    covered = np.zeros(n, dtype=bool)

    def dense_of(node):
        k = desc.kind[node]
        if k == hs.NODE_DENSE:
            return seen(vals[node], dtype).astype(W)
        if k == hs.NODE_IDENTITY:
            return np.eye(desc.rows[node], dtype=W)
        if k == hs.NODE_PRODUCT:
            out = None
            for c, _, _ in desc.children[node]:
                out = dense_of(c) if out is None else out @ dense_of(c)
            return out
        out = np.zeros((desc.rows[node], desc.cols[node]), dtype=W)
        for c, r0, c0 in desc.children[node]:
            out[r0:r0 + desc.rows[c], c0:c0 + desc.cols[c]] += dense_of(c)
        return out

    def walk(node, r0, c0):
        k, m, w = desc.kind[node], desc.rows[node], desc.cols[node]
        if k == hs.NODE_BLOCK:
            for c, dr, dc in desc.children[node]:
                walk(c, r0 + dr, c0 + dc)
        elif k == hs.NODE_DENSE:
            v = seen(vals[node], dtype).astype(W)
            total[r0:r0 + m, c0:c0 + w] += v
            count[r0:r0 + m, c0:c0 + w] += 1
            mod[r0:r0 + m, c0:c0 + w] += np.abs(v)
            if max(r0, c0) < min(r0 + m, c0 + w):
                covered[min(r0, c0):max(r0 + m, c0 + w)] = True
        elif k == hs.NODE_IDENTITY:
            i = np.arange(m)
            total[r0 + i, c0 + i] += 1
            count[r0 + i, c0 + i] += 1
            mod[r0 + i, c0 + i] += 1
            if r0 == c0:
                covered[r0:r0 + m] = True
        elif products:
            total[r0:r0 + m, c0:c0 + w] += dense_of(node)

    walk(desc.root, 0, 0)
    return total, count, mod, covered


def gather_expected(case, dtype, cuts):
    """Per block of `cuts`: (B_b in extended precision with the 1s of uncovered rows, contributions per entry, sum of moduli);
    and the number of uncovered rows."""
    desc, vals, _ = materialize_gather(case, dtype)
    total, count, mod, covered = direct_dense(desc, vals, dtype)
    idx = np.nonzero(~covered)[0]
    total[idx, idx] += 1
    count[idx, idx] += 1
    mod[idx, idx] += 1
    out = [(total[a:b, a:b], count[a:b, a:b], mod[a:b, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return out, int(idx.size)


def assert_gathered(got, expected, where="", out_dtype=None):
    """`got` (a block in the working type) against gather_expected's (B_b, contributions, moduli): bit for bit where an entry
    has at most one contribution (a stored value, 1 or 0: representable in every element type); where it has t, within
    (t - 1) fp64 roundings of the sum of moduli, per component -- plus, in a complex64 / float32 result (`out_dtype`), the one
    rounding of the fp64 sum to float that the fill kernel's store makes."""
    ref, count, mod = expected
    got = np.asarray(got)
    assert got.shape == ref.shape, (where, got.shape, ref.shape)
    one = count <= 1
    back = ref.astype(got.dtype)
    assert np.array_equal(got[one], back[one]), (where, "entries with one contribution differ")
    diff = got.astype(ref.dtype) - ref
    lim = (np.maximum(count - 1, 0) * np.longdouble(2.0 ** -53)) * mod
    low = out_dtype in (F32, C64)
    for part, val in ((diff.real, ref.real), (diff.imag, ref.imag)):
        allow = lim + (np.longdouble(2.0 ** -24) * (np.abs(val) + lim) * (count > 1) if low else 0)
        assert np.all(np.abs(part) <= allow), (where, float(np.max(np.abs(part) - allow)))
    assert not np.any(got[count == 0]), (where, "non-zero where nothing contributes")


# ---- references, computed once per (case, element type) -------------------------------------------------------------------
_REFS = {}


def inv_references(case, dtype):
    """[(B, exact inverse or None, X_ref, residual, g)] of an inversion case as the kernels of `dtype` read it."""
    from bj_ref import inverse_ref
    key = (case.name, dtype)
    if key not in _REFS:
        _REFS[key] = [(b, x) + inverse_ref(b) for b, x in inv_blocks(case, dtype)]
    return _REFS[key]
