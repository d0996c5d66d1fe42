"""Test infrastructure: an extended-precision reference for the apply path, with componentwise error bounds.

`Reference(desc, vals, dtype)` evaluates the `Desc` tree (dense, identity, block, product) recursively in `np.longdouble` /
`np.clongdouble` (a 64-bit mantissa on x86-64: u = 2^-64, far below every precision under test).  It computes

    A x,   A^T x   (the plain transpose, no conjugation: what bfhipApplyTranspose documents),
    |A| |x|, |A^T| |x|   through the same tree (moduli of the leaves and of x, products and sums as in A),

and `check(y, x, transpose)` turns the last into the componentwise error bound that every engine result must meet:

    |y_hat - y|_i  <=  gamma * (|A| |x|)_i + tiny.

Derivation.  Let u be the unit roundoff of the arithmetic an output element goes through and gamma_k = k u / (1 - k u).
* A sum of k products (a dot product, fma or not, in any order, in any tree of partial sums) has |error| <= gamma_k times
  the sum of the moduli of its terms (Higham, Accuracy and Stability, 3.1 and 3.5).  The engine's item / piece / reduce
  split of a row only changes the order of the sum.
* A block node adds the outputs of the children that cover a row: c such children add c - 1 roundings to the longest
  child chain.  A product node feeds one factor's rounded output to the next: to first order the relative errors add, and
  the bound of F1 (F2 x) is gamma_{k1 + k2} |F1| |F2| |x| -- hence |A| |x| evaluated through the tree, not |A x|.
* So K(node) -- the longest accumulation chain -- is n for an m x n dense leaf (m in A^T), 0 for an identity, the sum over the
  factors of a product, and max over children + (children covering one output - 1) for a block.  Every stored intermediate
  (a stage output in the vector arena, a partial sum in temp, the reduce's result) is one more rounding to the storage
  type: S(node) = stored levels, and R = 2 (S + 1) (an item's write and a reduce's write per level).
* Complex elements: one complex multiply-add is two real fmas per component, so K counts 2 per term; and the modulus of a
  complex error is at most sqrt(2) times its larger component.

Per element type (u64 = 2^-53, u32 = 2^-24):
* F64:  gamma = (K + R) u64.       C128: gamma = sqrt(2) (2K + R) u64.
* F32:  gamma = (K + R) u32        (the kernels accumulate in float).
* C64:  gamma = sqrt(2) (R u32 + 2K u64), with the leaves and x rounded to complex64 first (what the kernels see): the
  products of widened floats are exact in double, the accumulation is in double (Traits<C64>::A, the reduce's TA), and only
  the R stores round to float.  Float accumulation would pay 2K u32: on a contraction of K ~ 2000 terms that is ~60x the
  bound, so an accumulator narrowed to float fails it.
`tiny` covers underflow: K + 1 times the smallest normal of the storage type.

These are worst-case bounds: rounding errors of random sign stay far inside them, so a test that must tell float from
double accumulation apart needs data that makes the errors add up (tests/kernel_catalogue.py, the absorb cases)."""
from __future__ import annotations

import math

import numpy as np

from butterfly_amd.helm2_structure import NODE_BLOCK, NODE_DENSE, NODE_IDENTITY, NODE_PRODUCT

BFHIP_C128, BFHIP_F64, BFHIP_F32, BFHIP_C64 = 0, 1, 2, 3
U64, U32 = 2.0 ** -53, 2.0 ** -24
STORAGE = {BFHIP_C128: np.complex128, BFHIP_F64: np.float64, BFHIP_F32: np.float32, BFHIP_C64: np.complex64}


def _gamma(k, u):
    assert k * u < 0.5, (k, u)
    return k * u / (1.0 - k * u)


class Reference:
    """desc: a helm2_structure.Desc; vals: leaf node -> 2-D array; dtype: the engine element type (BFHIP_*) the results are
    judged for.  For F32 / C64 the leaves are rounded to the storage type first, as the engine stores them."""

    def __init__(self, desc, vals, dtype):
        self.d, self.dtype = desc, int(dtype)
        self.cplx = self.dtype in (BFHIP_C128, BFHIP_C64)
        self.work = np.clongdouble if self.cplx else np.longdouble
        st = STORAGE[self.dtype]
        self.leaf = {}
        for k in range(desc.num_nodes):
            if desc.kind[k] == NODE_DENSE:
                v = np.asarray(vals[k])
                v = v.astype(st) if not self.cplx else np.asarray(v, dtype=np.complex128).astype(st)
                self.leaf[k] = v.astype(self.work)
        self._chain = {}
        self.K, self.S = self._chains(desc.root, False)
        self.KT, self.ST = self._chains(desc.root, True)

    # ---- what the kernels see -----------------------------------------------------------------------------------------
    def rounded(self, x):
        """x as the engine holds it (the storage type)."""
        return np.asarray(x).astype(STORAGE[self.dtype])

    # ---- evaluation ------------------------------------------------------------------------------------------------------
    def _eval(self, node, x, transpose, absval):
        d = self.d
        k = d.kind[node]
        if k == NODE_DENSE:
            a = self.leaf[node]
            if absval:
                a = np.abs(a)
            a = a.T if transpose else a
            return a @ x
        if k == NODE_IDENTITY:
            return x.copy()
        if k == NODE_PRODUCT:
            fs = [c for c, _, _ in d.children[node]]
            order = fs if transpose else fs[::-1]          # A = F1 F2 ... Fk: A x applies Fk first; A^T x applies F1^T first
            v = x
            for f in order:
                v = self._eval(f, v, transpose, absval)
            return v
        assert k == NODE_BLOCK, k
        m, n = (d.cols[node], d.rows[node]) if transpose else (d.rows[node], d.cols[node])
        out = np.zeros((m,) + x.shape[1:], dtype=x.dtype)
        for c, r0, c0 in d.children[node]:
            if transpose:
                out[c0:c0 + d.cols[c]] += self._eval(c, x[r0:r0 + d.rows[c]], True, absval)
            else:
                out[r0:r0 + d.rows[c]] += self._eval(c, x[c0:c0 + d.cols[c]], False, absval)
        return out

    def apply(self, x, transpose=False):
        """A x (or A^T x) in extended precision, of x rounded to the storage type."""
        x = self.rounded(x).astype(self.work)
        return self._eval(self.d.root, x, transpose, False)

    def apply_abs(self, x, transpose=False):
        """|A| |x| (or |A^T| |x|) through the tree, in extended precision."""
        x = np.abs(self.rounded(x)).astype(np.longdouble)
        return self._eval(self.d.root, x, transpose, True).real.astype(np.longdouble)

    def structural(self, j, transpose=False):
        """Boolean mask of the outputs that depend on input j through the tree (no exact zeros in the leaves assumed)."""
        n = self.d.rows[self.d.root] if transpose else self.d.cols[self.d.root]
        e = np.zeros(n, dtype=np.float64)
        e[j] = 1.0
        save = self.leaf
        self.leaf = {k: np.ones(v.shape, dtype=np.longdouble) for k, v in save.items()}
        try:
            return self._eval(self.d.root, e.astype(np.longdouble), transpose, True) != 0
        finally:
            self.leaf = save

    # ---- bounds ----------------------------------------------------------------------------------------------------------
    def _chains(self, node, transpose):
        """(K, S): longest accumulation chain and stored levels below `node` in A (or A^T), see the module docstring."""
        if (node, transpose) in self._chain:
            return self._chain[(node, transpose)]
        d = self.d
        k = d.kind[node]
        if k == NODE_DENSE:
            r = (d.rows[node] if transpose else d.cols[node], 0)
        elif k == NODE_IDENTITY:
            r = (0, 0)
        elif k == NODE_PRODUCT:
            ch = [self._chains(c, transpose) for c, _, _ in d.children[node]]
            r = (sum(c[0] for c in ch), sum(c[1] for c in ch) + len(ch) - 1)
        else:
            ch = d.children[node]
            sub = [self._chains(c, transpose) for c, _, _ in ch]
            # children covering one output: one row (A x) / one column (A^T x)
            cover = np.zeros((d.cols[node] if transpose else d.rows[node]) + 1, dtype=np.int64)
            for c, r0, c0 in ch:
                o0, w = (c0, d.cols[c]) if transpose else (r0, d.rows[c])
                cover[o0] += 1; cover[o0 + w] -= 1
            cover = max(int(np.cumsum(cover).max(initial=0)), 1)
            r = (max(s[0] for s in sub) + cover - 1 if sub else 0, max(s[1] for s in sub) if sub else 0)
        self._chain[(node, transpose)] = r
        return r

    def gamma(self, transpose=False):
        K, S = (self.KT, self.ST) if transpose else (self.K, self.S)
        R = 2 * (S + 1)
        if self.dtype == BFHIP_F64:
            return _gamma(K + R, U64)
        if self.dtype == BFHIP_F32:
            return _gamma(K + R, U32)
        if self.dtype == BFHIP_C128:
            return math.sqrt(2.0) * _gamma(2 * K + R, U64)
        return math.sqrt(2.0) * (_gamma(R, U32) + _gamma(2 * K, U64))

    def tiny(self, transpose=False):
        return ((self.KT if transpose else self.K) + 1) * float(np.finfo(np.float32 if self.dtype in (BFHIP_F32, BFHIP_C64) else np.float64).tiny)

    def check(self, y, x, transpose=False):
        """Assert the componentwise bound for an engine result y of x; returns the worst ratio error / bound."""
        y = np.asarray(y)
        ref = self.apply(x, transpose)
        ab = self.apply_abs(x, transpose)
        err = np.abs(y.astype(self.work) - ref).astype(np.longdouble)
        lim = np.longdouble(self.gamma(transpose)) * ab + np.longdouble(self.tiny(transpose))
        ratio = err / lim
        worst = float(ratio.max(initial=0.0))
        assert np.isfinite(y).all(), "non-finite output"
        assert worst <= 1.0, (f"componentwise bound violated: worst |y - ref| / (gamma |A||x| + tiny) = {worst:.3g} "
                              f"at {np.unravel_index(int(np.argmax(ratio)), ratio.shape)} (transpose {transpose}, K = {self.KT if transpose else self.K}, "
                              f"S = {self.ST if transpose else self.S}, gamma = {self.gamma(transpose):.3g})")
        return worst
