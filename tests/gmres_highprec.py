"""Test infrastructure: a long-double GMRES reference, and the bounds a complex128 GMRES must meet against it.

For a problem (A, b, x0) and a number of Arnoldi steps m, `Krylov` computes in `np.clongdouble` (a 64-bit mantissa on x86-64:
u_ld = 2^-64, 2^11 times below the complex128 u = 2^-53 under test, and an exponent range of 2^+-16382, so data of 2^+-600 need no
scaling):

* the exact GMRES iterate x_m = argmin ||b - A x|| over x0 + K_m(A, r0), r0 = b - A x0: Arnoldi with full reorthogonalisation
  (classical Gram-Schmidt, twice) and a long-double Givens least-squares solve of the (m+1) x m Hessenberg problem.  When the
  Krylov space is invariant (h_{k+1,k} <= 64 u_ld ||A v_k||: an exact breakdown, to long-double accuracy) the iterate is the
  solution and later steps add nothing;
* its residual ||b - A x_m||;
* the true residual ||b - A X|| of any complex128 X, evaluated in long double.
A x goes through `highprec.Reference`'s evaluation of the same `Desc` tree the device compiles, in long double, with no rounding
of the vector to complex128 in between.  A left preconditioner is a matrix P (the action of M^-1, as the device holds it): the
problem is then (P A, P b), the preconditioned residual the one GMRES minimises and reports.

Bounds.  Modified Gram-Schmidt GMRES and CGS2 GMRES are normwise backward stable (Paige, Rozloznik and Strakos, SIAM J. Matrix
Anal. Appl. 28 (2006); Giraud, Langou and Rozloznik for CGS2): the computed X is the exact GMRES iterate of a problem
(A + dA, b + db) with ||dA|| <= eps ||A||, ||db|| <= eps ||b||, eps = c m sqrt(n) u to first order -- m Arnoldi steps, each a
matvec (a sum of n products) and 2(j + 1) dot products and axpys of length n, whose normwise errors are sqrt(n) u per operation.
Column p, with X0 the start (0 without one), has the floor

    f_p = c m sqrt(n) u (||b_p|| + ||A|| (||X_p|| + ||X0_p||))

(the X0 term covers r0 = b - A x0, which the device forms before the scaling), and must meet

    residual:     ||b_p - A X_p||  <=  ||r_m,p|| + f_p
    forward:      ||X_p - x_m,p||  <=  kappa(A) f_p / ||A||
    consistency:  ||b_p - A X_p|| / beta  <=  reported + f_p / beta,   beta = max_q ||r0_q||

The forward bound is the perturbation bound of the least-squares solution with the Krylov space held fixed.  It, and the
residual bound, hold where the iterate is well determined: a converged solve, or a stagnating one (||r_m|| close to ||r_0||).
Between the two an MGS basis loses orthogonality in proportion to ||r_0|| / ||r_m|| (Greenbaum, Rozloznik and Strakos, BIT 37
(1997)) and an unconverged x_m can move far more than eps: the catalogue's capped cases therefore use operators on which GMRES
converges fast or stagnates (kappa <= 1e3, known by design or by an SVD).  c = C_BOUND = 32, fixed
once for every case: the fp64 restatement meets every bound with it (tests/test_gmres_highprec_cpu.py), and each of its mutants
-- a dropped conjugate, a dropped row, float32 dots, unscaled norms, the reference's j-vector quirk -- breaks at least one.
u = 2^-53; complex arithmetic adds a small constant that c absorbs."""
from __future__ import annotations

import math

import numpy as np

import highprec

U = 2.0 ** -53
U_LD = float(np.finfo(np.longdouble).eps) / 2
C_BOUND = 32
LD = np.clongdouble


def _norm(v):
    """2-norm of the columns of a long-double array (no scaling needed in long double's range)."""
    v = np.asarray(v)
    return np.sqrt((v.real.astype(np.longdouble) ** 2 + v.imag.astype(np.longdouble) ** 2).sum(axis=0))


def _cols(a):
    a = np.asarray(a)
    return a[:, None] if a.ndim == 1 else a


class Problem:
    """The operator as GMRES sees it: `desc`, `vals` (the tree the device compiles), an optional left preconditioner `P` (n x n
    complex128 matrix, the action of M^-1), and ||P A||, kappa(P A) (designed, or from an SVD)."""

    def __init__(self, desc, vals, norm_a, kappa, P=None):
        self.ref = highprec.Reference(desc, vals, highprec.BFHIP_C128)
        self.n = desc.rows[desc.root]
        self.norm_a, self.kappa = float(norm_a), float(kappa)
        self.P = None if P is None else np.asarray(P, dtype=np.complex128).astype(LD)

    def plain(self, x):
        """A x in long double, x n x k."""
        return self.ref._eval(self.ref.d.root, np.asarray(x).astype(LD), False, False)

    def precond(self, x):
        return x if self.P is None else self.P @ x

    def matvec(self, x):
        return self.precond(self.plain(x))

    def residual(self, B, X):
        """P (B - A X) in long double, column by column: what GMRES minimises."""
        B, X = _cols(B), _cols(X)
        return self.precond(B.astype(LD) - self.plain(X))


def _lstsq_hessenberg(H, beta, k):
    """min || beta e_1 - H[:k+1, :k] y || by Givens rotations in long double; returns y (k)."""
    R = H[:k + 1, :k].copy()
    g = np.zeros(k + 1, dtype=LD)
    g[0] = beta
    for j in range(k):
        a, b = R[j, j], R[j + 1, j]
        r = np.sqrt(abs(a) ** 2 + abs(b) ** 2)
        if r == 0:
            continue
        c, s = a / r, b / r
        top = np.conj(c) * R[j, j:] + np.conj(s) * R[j + 1, j:]
        bot = -s * R[j, j:] + c * R[j + 1, j:]
        R[j, j:], R[j + 1, j:] = top, bot
        g[j], g[j + 1] = np.conj(c) * g[j] + np.conj(s) * g[j + 1], -s * g[j] + c * g[j + 1]
    y = np.zeros(k, dtype=LD)
    for r in range(k - 1, -1, -1):
        y[r] = (g[r] - R[r, r + 1:k] @ y[r + 1:k]) / R[r, r]
    return y


class Krylov:
    """Exact GMRES iterates of one problem and right-hand-side block, for any m; each column's Arnoldi basis is built once, as
    far as the largest m asked for."""

    def __init__(self, problem, B, X0=None):
        self.pb = problem
        self.B = _cols(np.asarray(B, dtype=np.complex128))
        self.X0 = np.zeros_like(self.B) if X0 is None else _cols(np.asarray(X0, dtype=np.complex128))
        self.R0 = problem.residual(self.B, self.X0)
        self.beta = _norm(self.R0)
        self._basis = [None] * self.B.shape[1]      # per column: [V list, H, invariant length or None]

    def _extend(self, p, m):
        st = self._basis[p]
        if st is None:
            b = self.beta[p]
            st = self._basis[p] = [[self.R0[:, p] / b] if b > 0 else [], np.zeros((1, 0), dtype=LD), 0 if b == 0 else None]
        V, H, inv = st
        while inv is None and H.shape[1] < m:
            j = H.shape[1]
            w = self.pb.matvec(V[j][:, None])[:, 0]
            scale = _norm(w[:, None])[0]
            h = np.zeros(j + 2, dtype=LD)
            Vm = np.stack(V, axis=1)
            for _ in range(2):
                c = Vm.conj().T @ w
                w = w - Vm @ c
                h[:j + 1] += c
            h[j + 1] = _norm(w[:, None])[0]
            Hn = np.zeros((j + 2, j + 1), dtype=LD)
            Hn[:H.shape[0], :j] = H
            Hn[:, j] = h
            H = Hn
            if h[j + 1] <= 64 * U_LD * scale:
                inv = j + 1
            else:
                V.append(w / h[j + 1])
        st[1], st[2] = H, inv
        return st

    def iterate(self, m):
        """(x_m as a complex long-double n x k array, ||r_m|| per column)."""
        X = self.X0.astype(LD)
        for p in range(self.B.shape[1]):
            V, H, inv = self._extend(p, m)
            kk = min(m, H.shape[1]) if inv is None else min(m, inv)
            if kk == 0:
                continue
            y = _lstsq_hessenberg(H, self.beta[p], kk)
            X[:, p] = X[:, p] + np.stack(V[:kk], axis=1) @ y
        return X, _norm(self.pb.residual(self.B, X))

    def true_residual(self, X):
        return _norm(self.pb.residual(self.B, np.asarray(X, dtype=np.complex128)))


def check(kry, X, m, reported):
    """Every bound of the module docstring for the complex128 result X of m Arnoldi steps and its reported residual.  Returns a
    list of failures (empty: all met)."""
    pb = kry.pb
    X = _cols(np.asarray(X, dtype=np.complex128))
    n, k = X.shape
    if not np.all(np.isfinite(X)):
        return [f"non-finite X in columns {sorted(set(np.nonzero(~np.isfinite(X))[1].tolist()))}"]
    xm, rm = kry.iterate(m)
    tr = kry.true_residual(X)
    fwd = _norm(X.astype(LD) - xm)
    eps = C_BOUND * max(m, 1) * math.sqrt(n) * U
    beta = float(kry.beta.max())
    out = []
    for p in range(k):
        nb, nx, nx0 = (float(_norm(a[:, p:p + 1])[0]) for a in (kry.B, X, kry.X0))
        f = eps * (nb + pb.norm_a * (nx + nx0))
        t, r = float(tr[p]), float(rm[p])
        if not t <= r + f:
            out.append(f"col {p}: residual {t:.3e} > r_m {r:.3e} + floor {f:.3e}")
        if not float(fwd[p]) <= pb.kappa * f / pb.norm_a:
            out.append(f"col {p}: forward {float(fwd[p]):.3e} > kappa floor / ||A|| = {pb.kappa * f / pb.norm_a:.3e}")
        if beta > 0 and not t / beta <= reported + f / beta:
            out.append(f"col {p}: true residual / beta {t / beta:.3e} > reported {reported:.3e} + {f / beta:.3e}")
    return out
