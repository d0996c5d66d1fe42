"""Test infrastructure for the block-Jacobi kernels (bfhip_precond.hip): the direct-part rule restated in numpy, an
extended-precision inverse, a numpy restatement of the inversion kernel in fp64 with named wrong variants, and the forward
error bound every inverse must meet.

`inverse_ref(B)` inverts in `np.longdouble` / `np.clongdouble` (64-bit mantissa, u = 2^-64, exponents to 2^+-16383): Gauss-
Jordan elimination with partial pivoting in the form without row scaling (Higham, Accuracy and Stability, Algorithm 14.4:
row i of the whole array loses multiplier * row k, the diagonal is divided out at the end), then Newton steps
X <- X (2 I - B X) until ||I - B X||_inf stops decreasing.  It returns X, that residual, and the growth factor
g = (largest modulus of any entry of any intermediate array of the elimination) / max |B|, g >= 1.

`gje_fp64(B, variant)` restates the kernel: fp64 working copy; step k takes the pivot of the largest |re| + |im| of column
k at or below row k, ties to the smaller row; refuses (status 1, step k) a pivot whose modulus (hypot) is zero or not
finite, or whose scaled reciprocal (bjRecip) is not finite; swaps rows k and p; forms the scaled pivot row by MULTIPLYING
with the reciprocal (entry k = the reciprocal) and refuses a non-finite entry in it; updates A(i, j) = [j != k] A(i, j) -
colF(i) rowK(j) for i != k, A(k, .) = rowK; and at the end swaps the columns back, last step first.  numpy has no fused
multiply-add, the device contracts a - f r: the two agree to rounding, and bit for bit where the arithmetic is exact.

The bound.  The kernel computes column j of the inverse as Gauss-Jordan elimination applied to B x = e_j.  For GJE with
partial pivoting Higham's Corollary 14.7 (section 14.4) gives, to first order in u,

    ||x - x_hat||_inf / ||x||_inf  <=  2 m u ( || |B^-1| |L_hat| |U_hat| ||_inf + 3 kappa_inf(U_hat) ),

L_hat, U_hat the LU factors the first stage produces.  Both matrix terms are taken in the form in which the stability of
Gaussian elimination is stated in practice (Higham 9.3-9.4): |L_hat| |U_hat| of the size of the largest intermediate,
|| |L_hat| |U_hat| ||_inf <= mu g ||B||_inf, and kappa_inf(U_hat) <= mu g kappa_inf(B), where mu bounds the multipliers: 1 for
real blocks, sqrt(2) for complex ones (the |re| + |im| key picks a pivot of at least 1 / sqrt(2) of the largest modulus).
The worst case carries a further m^2 (every partial sum of |L||U| at the largest intermediate); it is attained only
together with g = 2^(m-1), and the catalogue's growth-prone block is covered by g itself.  So the bracket is at most
4 mu g kappa_inf(B) and the real-arithmetic constant is 8 m.  The kernel differs from Higham's algorithm in one respect:
it multiplies by a reciprocal instead of dividing, so the row scaling rounds twice (three times with the rounding of 1 /
pivot in the real case; the complex bjRecip rounds each of its seven operations) where a division rounds once.  Doubling the
constant covers that: C(m) = 16 m for real blocks.  Complex blocks, as tests/highprec.py counts them: one complex multiply-
add is two real ones per component (x 2), the modulus of a complex error is at most sqrt(2) times its larger component
(x sqrt(2)), and mu = sqrt(2): C(m) = 64 m.  The forward-error bound of a result X_hat is then

    || max(|X_hat - X_ref| - e, 0) ||_inf  <=  C(m) u64 g kappa_inf(B) ||X_ref||_inf,      kappa_inf(B) = ||B||_inf ||X_ref||_inf,

with the entrywise allowance e = (m + 1) tiny for underflow (tiny = the smallest normal of the result's element type: an
entry that leaves the normal range is rounded to a multiple of the subnormal spacing at each of m steps), plus one rounding
to the result's type, u32 |X_ref|, when the result is complex64 / float32 (the fill kernel rounds the fp64 working copy
once on the store).  Nothing here was tuned to device output.

Measured (tests/test_bj_highprec_cpu.py): over the inversion catalogue and the four element types the largest
error / bound of gje_fp64("device") is 0.031 (1/32, on a 1 x 1 real block: half an ulp of 1 / x against 16 u),
a factor 32 of room, and the reference's own ||X_ref||_inf ||I - B X_ref||_inf is below 2^-8 of
the bound everywhere."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from butterfly_amd import _capi, helm2_structure as hs

BF_ITEM_OUT_Y = 1 << 16
BF_PIECE_IN_X, BF_PIECE_IDENTITY, BF_PIECE_ROWMAJOR = 1, 2, 4


def _view(ptr, count, dtype):
    if count == 0:
        return np.zeros(0, dtype=dtype)
    return np.frombuffer((C.c_char * (count * dtype.itemsize)).from_address(ptr), dtype=dtype)


def direct_blocks(op, cuts):
    """Numpy restatement of the direct-part rule: the pieces that read x and write y, or write vector-arena rows a reduce of
    the same stage sums into y; identity pieces are identity entries.  Returns [B_b] with B_b = A_dir[D_b, D_b]."""
    lib = _capi.load()
    info = _capi.BfhipPlanInfo()
    info.structSize = C.sizeof(info)
    _capi.check(lib.bfhipPlanGetInfo(op.handle, C.byref(info)))
    dt = {0: np.complex128, 1: np.float64, 2: np.float32, 3: np.complex64}[info.dtype]
    arena = np.zeros(int(info.arenaElems), dtype=dt)
    _capi.check(lib.bfhipPlanPackArena(op.handle, arena.ctypes.data))
    n, epl = int(info.numRows), int(info.epl)
    adir = np.zeros((n, n), dtype=np.complex128 if np.iscomplexobj(arena) else np.float64)
    for s in range(int(info.numStages)):
        sv = _capi.BfhipStageView()
        sv.structSize = C.sizeof(sv)
        _capi.check(lib.bfhipPlanGetStage(op.handle, s, C.byref(sv)))
        items = _view(sv.items, int(sv.numItems), _capi.ITEM_DTYPE)
        pieces = _view(sv.pieces, int(sv.numPieces), _capi.PIECE_DTYPE)
        tmap = {}          # vector-arena row -> y row, from this stage's y-reduces
        for r in range(int(sv.numReduce)):
            rv = _capi.BfhipReduceView()
            rv.structSize = C.sizeof(rv)
            _capi.check(lib.bfhipPlanGetReduce(op.handle, s, r, C.byref(rv)))
            if not rv.destIsY:
                continue
            row_iv = _view(rv.rowInterval, int(rv.numRows), np.dtype("<u4"))
            iv_begin = _view(rv.ivBegin, int(rv.numIntervals) + 1, np.dtype("<u4"))
            bias = _view(rv.srcBias, int(rv.numSrc), np.dtype("<i8"))
            for row in range(int(rv.numRows)):
                iv = int(row_iv[row])
                if iv == 0xFFFFFFFF:
                    continue
                for q in range(int(iv_begin[iv]), int(iv_begin[iv + 1])):
                    tmap[int(bias[q]) + row] = row
        for it in items:
            mr = int(it["mrFlags"]) & 0xFFFF
            mr_pad = (mr + epl - 1) // epl * epl
            if int(it["mrFlags"]) & BF_ITEM_OUT_Y:
                yrows = np.arange(int(it["outOff"]), int(it["outOff"]) + mr)
            else:
                yrows = np.array([tmap.get(int(it["outOff"]) + i, -1) for i in range(mr)])
            keep = yrows >= 0
            if not keep.any():
                continue
            for pc in pieces[int(it["pieceBegin"]):int(it["pieceBegin"]) + int(it["numPieces"])]:
                fl = int(pc["flags"])
                if not fl & BF_PIECE_IN_X:
                    continue
                io, nc, d0 = int(pc["inOff"]), int(pc["ncols"]), int(pc["dataOff"])
                if fl & BF_PIECE_IDENTITY:
                    rows = np.nonzero(keep)[0]
                    np.add.at(adir, (yrows[rows], io + rows), 1.0)
                    continue
                if fl & BF_PIECE_ROWMAJOR:
                    ld = int(pc["ld"])
                    blk = arena[d0:d0 + mr * ld].reshape(mr, ld)[:, :nc]
                else:
                    blk = arena[d0:d0 + mr_pad * nc].reshape(nc, mr_pad).T[:mr]
                adir[yrows[keep], io:io + nc] += blk[keep]
    return [adir[a:b, a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def self_leaf_cuts(desc, root, n):
    """The diagonal dense self-leaves, from the descriptor alone: dense leaves reached through BLOCK nodes (never a product)
    that sit on the diagonal; identity leaves cover single rows.  Merged into intervals the way the rule merges pieces."""
    reach = -np.ones(n, dtype=np.int64)

    def walk(node, r0, c0):
        kind = desc.kind[node]
        if kind == hs.NODE_BLOCK:
            for c, dr, dc in desc.children[node]:
                walk(c, r0 + dr, c0 + dc)
        elif kind == hs.NODE_DENSE and r0 == c0 and desc.rows[node] == desc.cols[node]:
            reach[r0] = max(reach[r0], r0 + desc.rows[node])
        elif kind == hs.NODE_IDENTITY and r0 == c0:
            for i in range(desc.rows[node]):
                reach[r0 + i] = max(reach[r0 + i], r0 + i + 1)
    walk(root, 0, 0)
    cuts, i = [0], 0
    while i < n:
        end = i + 1 if reach[i] < 0 else int(reach[i])
        j = i + 1
        while j < end:
            end = max(end, int(reach[j]))
            j += 1
        cuts.append(end)
        i = end
    return np.array(cuts)


# ---- extended-precision inverse ---------------------------------------------------------------------------------------
U64, U32 = 2.0 ** -53, 2.0 ** -24
DBL_MAX = float(np.finfo(np.float64).max)


def _work(B):
    return np.clongdouble if np.iscomplexobj(B) else np.longdouble


def _norm_inf(a):
    return np.abs(a).sum(axis=1).max(initial=0) if a.size else np.longdouble(0)


def inverse_ref(B):
    """(X, residual, g): the inverse of B in extended precision, ||I - B X||_inf, and the growth factor of the elimination."""
    W = _work(B)
    B = np.asarray(B).astype(W)
    m = B.shape[0]
    A, X = B.copy(), np.eye(m, dtype=W)
    scale = np.abs(B).max()
    big = scale
    for k in range(m):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            X[[k, p]] = X[[p, k]]
        f = A[:, k] / A[k, k]
        f[k] = 0
        A -= np.outer(f, A[k])
        X -= np.outer(f, X[k])
        big = max(big, np.abs(A).max())
    X /= np.diagonal(A)[:, None]
    eye = np.eye(m, dtype=W)
    R = eye - B @ X
    res = _norm_inf(R)
    for _ in range(8):
        Xn = X + X @ R
        Rn = eye - B @ Xn
        rn = _norm_inf(Rn)
        if not rn < res:
            break
        X, R, res = Xn, Rn, rn
    return X, float(res), float(big / scale)


# ---- the kernel's algorithm in fp64 ---------------------------------------------------------------------------------------
VARIANTS = ("device", "no_pivoting", "search_from_row0", "swap_back_forward", "jk_not_zeroed", "recip_float32", "update_float32",
            "hypot_ties_larger")


@dataclass
class GjeResult:
    inverse: object          # None when refused
    status: int
    step: int
    min_pivot: float         # smallest pivot modulus (0 when refused)
    max_abs: float           # largest modulus of B (inf with a NaN or infinity)

    @property
    def min_pivot_rel(self):
        return self.min_pivot / self.max_abs if self.max_abs > 0 else 0.0


def _finite(re, im):
    return bool(np.all(np.abs(re) <= DBL_MAX) and np.all(np.abs(im) <= DBL_MAX))


def gje_fp64(B, variant="device"):
    """The inversion kernel restated on one block (see the module docstring); `variant` names a deliberately wrong version."""
    assert variant in VARIANTS, variant
    cplx = np.iscomplexobj(B)
    B = np.asarray(B, dtype=np.complex128 if cplx else np.float64)
    m = B.shape[0]
    re, im = np.array(B.real, dtype=np.float64), np.array(B.imag if cplx else np.zeros_like(B.real), dtype=np.float64)
    with np.errstate(all="ignore"):
        mod = np.hypot(re, im)
        max_abs = float(np.inf if np.isnan(mod).any() else mod.max(initial=0.0))
        perm, min_piv = [], np.inf
        for k in range(m):
            key = np.hypot(re[:, k], im[:, k]) if variant == "hypot_ties_larger" else np.abs(re[:, k]) + np.abs(im[:, k])
            key = np.where(np.isnan(key), np.inf, key)
            if variant == "no_pivoting":
                p = k
            else:
                lo = 0 if variant == "search_from_row0" else k
                hit = np.nonzero(key[lo:] == key[lo:].max())[0]
                p = lo + int(hit[-1] if variant == "hypot_ties_larger" else hit[0])
            pr, pi = re[p, k], im[p, k]
            pa = float(np.hypot(pr, pi))
            if cplx:
                s = max(abs(pr), abs(pi))
                a, b = pr / s, pi / s
                d = a * a + b * b
                ir, ii = a / d / s, -b / d / s
            else:
                ir, ii = 1.0 / pr, 0.0
            if not pa > 0.0 or not pa <= DBL_MAX or not _finite(ir, ii):
                return GjeResult(None, 1, k, 0.0, max_abs)
            if variant == "recip_float32":
                ir, ii = float(np.float32(ir)), float(np.float32(ii))
            min_piv = min(min_piv, pa)
            if p != k:
                re[[k, p]] = re[[p, k]]
                im[[k, p]] = im[[p, k]]
            perm.append(p)
            rkr = re[k] * ir - im[k] * ii
            rki = re[k] * ii + im[k] * ir
            rkr[k], rki[k] = ir, ii
            if not _finite(rkr, rki):
                return GjeResult(None, 1, k, 0.0, max_abs)
            fr, fi = re[:, k].copy(), im[:, k].copy()
            fr[k] = fi[k] = 0.0
            if variant != "jk_not_zeroed":
                re[:, k] = 0.0
                im[:, k] = 0.0
            if variant == "update_float32":
                f32 = lambda v: v.astype(np.float32)
                pr_ = (np.outer(f32(fr), f32(rkr)) - np.outer(f32(fi), f32(rki))).astype(np.float64)
                pi_ = (np.outer(f32(fr), f32(rki)) + np.outer(f32(fi), f32(rkr))).astype(np.float64)
            else:
                pr_ = np.outer(fr, rkr) - np.outer(fi, rki)
                pi_ = np.outer(fr, rki) + np.outer(fi, rkr)
            re -= pr_
            im -= pi_
            re[k], im[k] = rkr, rki
        order = range(m) if variant == "swap_back_forward" else range(m - 1, -1, -1)
        for k in order:
            p = perm[k]
            if p != k:
                re[:, [k, p]] = re[:, [p, k]]
                im[:, [k, p]] = im[:, [p, k]]
    out = re + 1j * im if cplx else re
    return GjeResult(out, 0, 0, float(min_piv) if m else 0.0, max_abs)


def gje_blocks(blocks, variant="device"):
    """The host's part over many blocks: (results, firstSingularBlock or -1, step of that block, minPivotRel)."""
    res = [gje_fp64(b, variant) for b in blocks]
    first = next((i for i, r in enumerate(res) if r.status), -1)
    mpr = np.inf
    for r in res:
        v = r.min_pivot_rel
        if not v >= mpr:
            mpr = v
    return res, first, (res[first].step if first >= 0 else 0), (mpr if res else np.nan)


# ---- the bound ------------------------------------------------------------------------------------------------------------
def c_of_m(m, cplx):
    """C(m) of the module docstring."""
    return (64.0 if cplx else 16.0) * m


@dataclass
class Bound:
    limit: float             # on || max(|X_hat - X_ref| - allow, 0) ||_inf
    allow: object            # entrywise allowance (long double)
    ref_norm: float


def bound(B, X_ref, g, out_dtype):
    """The forward-error bound a fp64 Gauss-Jordan inverse of B, stored as `out_dtype` (a numpy type), must meet."""
    cplx = np.iscomplexobj(X_ref)
    m = X_ref.shape[0]
    out_dtype = np.dtype(out_dtype)
    low = out_dtype in (np.dtype(np.complex64), np.dtype(np.float32))
    nb, nx = float(_norm_inf(np.asarray(B).astype(_work(X_ref)))), float(_norm_inf(X_ref))
    tiny = float(np.finfo(np.float32 if low else np.float64).tiny)
    allow = np.full(X_ref.shape, (m + 1) * tiny, dtype=np.longdouble)
    if low:
        allow = allow + np.longdouble(U32) * np.abs(X_ref)
    return Bound(c_of_m(m, cplx) * U64 * g * (nb * nx) * nx, allow, nx)


def error_ratio(X_hat, X_ref, bnd):
    """|| max(|X_hat - X_ref| - allow, 0) ||_inf / limit (inf for a non-finite result)."""
    X_hat = np.asarray(X_hat)
    if not np.isfinite(X_hat).all():
        return np.inf
    err = np.abs(X_hat.astype(X_ref.dtype) - X_ref) - bnd.allow
    err = np.where(err > 0, err, 0)
    return float(_norm_inf(err) / np.longdouble(bnd.limit))
