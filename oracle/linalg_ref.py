"""ORACLE (test infrastructure, not product code).

Numpy restatement of the reference's GMRES, the production caller of the
apply path:

  bfSolveGMRES                       reference src/linalg.c:47-317
  column dots (zdotc: conj(V_i)^T W) src/mat_dense_complex.c:88-131
  Givens rotation (SciPy/templates)  src/vec_complex.c:230-292
  applying a rotation                src/vec_complex.c:155-168
  back substitution (ztrsv, upper)   src/mat_dense_complex.c:1306-1325

Kept from the reference, so that the device solver can be compared iteration
for iteration:
  * no restarts; modified Gram-Schmidt in the order i = 0..j;
  * beta = max over right-hand sides of ||r_p||, residual = max_p |s_{j+1,p}| / beta.

Where the device solver (butterfly_amd/csrc/bfhip_gmres.c) departs from the
reference, this restatement departs with it:
  * on convergence at iteration j the solution is built from V_0..V_j, the
    vectors the estimate |s_{j+1}| describes, and numIter = j + 1: the number of
    Arnoldi steps, as numIter = maxNumIter is when the test never passes.  The
    reference breaks before j is incremented and builds the solution from j
    vectors (linalg.c:228-243 use `j`); `reference_quirk=True` restates that;
  * each residual column is scaled by 2^-e_p (its largest component then lies in
    [1/2, 1)) before its norm is taken, and its coefficients are scaled back by
    2^e_p: no sum of squares underflows or overflows (the reference's dznrm2 is
    scaled too);
  * a column whose residual is zero, or whose H[j+1, j] is exactly 0, stops: its
    next basis vector is 0, not 0/0, and its solution uses its own vectors only.
    When every column has stopped the solve ends, whatever tol is.

`dot`, `sumsq` and `scaled` exist for tests/test_gmres_highprec_cpu.py: it
checks that deliberately wrong kernels (its mutants) break the bounds of
tests/gmres_highprec.py.

PARITY STATUS: see oracle/bfref.h.
"""
from __future__ import annotations

import numpy as np


def givens(a, b):
    """bfVecComplexGetGivensRotation, src/vec_complex.c:275-286."""
    if abs(b) == 0:
        return 1.0 + 0j, 0.0 + 0j
    if abs(b) > abs(a):
        tmp = -a / b
        s = 1 / np.sqrt(1 + abs(tmp) ** 2)
        return tmp * s, s + 0j
    tmp = -b / a
    c = 1 / np.sqrt(1 + abs(tmp) ** 2)
    return c + 0j, tmp * c


def apply_givens(vec, i0, i1, c, s):
    """mulInplace_givensComplex, src/vec_complex.c:155-168."""
    z0, z1 = vec[i0], vec[i1]
    vec[i0] = np.conj(c) * z0 - s * z1
    vec[i1] = s * z0 + c * z1


def _dot(U, W):
    """zdotc per column: sum_r conj(U[r, p]) W[r, p]."""
    return np.einsum("ij,ij->j", U.conj(), W)


def _sumsq(W):
    """sum_r |W[r, p]|^2 per column, unscaled (what the device kernels accumulate)."""
    return (W.real ** 2 + W.imag ** 2).sum(axis=0)


def _ldexp(z, e):
    return np.ldexp(z.real, e) + 1j * np.ldexp(z.imag, e)


def solve_gmres(matmul, B, X0=None, tol=1e-12, max_num_iter=100, msolve=None, reference_quirk=False, dot=None, sumsq=None,
                scaled=True):
    """Returns (X, num_iter, residual_history).  `matmul(X)` is bfMatMul(A, X)
    for an n x nrhs complex array; `msolve(X)` is bfMatSolve(M, X) for the left
    preconditioner M (src/linalg.c:90-97,131-135,157-163), None without one."""
    dot = dot or _dot
    sumsq = sumsq or _sumsq
    if msolve is not None:
        plain = matmul
        matmul = lambda X: msolve(plain(X))                 # W = M^{-1} (A V[j])  :157-163
    B = np.asarray(B, dtype=np.complex128)
    one_d = B.ndim == 1
    if one_d:
        B = B[:, None]
    n, nrhs = B.shape
    X0 = np.zeros_like(B) if X0 is None else np.asarray(X0, dtype=np.complex128).reshape(n, nrhs)
    R = B - matmul(X0) if msolve is None else msolve(B - plain(X0))   # :127-135
    # R_p *= 2^-e_p exactly, e_p = the binary exponent of the largest component (0 for a zero column)
    big = np.maximum(np.abs(R.real), np.abs(R.imag)).max(axis=0)
    e = np.zeros(nrhs, dtype=np.int64)
    if scaled:
        ok = (big > 0) & np.isfinite(big)
        e[ok] = np.frexp(big[ok])[1]
    R = _ldexp(R, -e[None, :])
    rnorm = np.sqrt(sumsq(R))                            # :139
    live = rnorm > 0
    E = int(e[live].max()) if live.any() else 0
    beta = float(np.ldexp(rnorm, e - E).max())           # :142, in units of 2^E
    X = X0.copy()
    if not beta > 0:                                     # zero residual: x0 solves the system
        return (X[:, 0] if one_d else X), 0, []
    length = np.where(live, -1, 0)                       # -1: running; else the number of vectors its solution uses
    V = [np.where(live, R / np.where(live, rnorm, 1), 0)]   # :145-146
    S = np.zeros((max_num_iter + 1, nrhs), dtype=np.complex128)
    S[0] = rnorm                                         # :150-151
    H = []
    J = {}
    history = []
    converged = False
    j = 0
    for j in range(max_num_iter):
        W = matmul(V[j])                                 # :157
        Hj = np.zeros((j + 2, nrhs), dtype=np.complex128)
        for i in range(j + 1):                           # modified Gram-Schmidt :174-184
            hij = dot(V[i], W)                           # zdotc
            Hj[i] = hij
            W = W - V[i] * hij
        wnorm = np.sqrt(sumsq(W))                        # :186
        Hj[j + 1] = wnorm
        V.append(np.where(wnorm > 0, W / np.where(wnorm > 0, wnorm, 1), 0))   # :197-198; a zero column stays 0
        resmax = 0.0
        for p in range(nrhs):
            if length[p] >= 0:
                continue
            col = Hj[:, p]
            if not abs(col[j + 1]) > 0:
                length[p] = j + 1                        # exact breakdown: K_{j+1} is invariant, this column's solve exact
            for i in range(j):                           # earlier rotations :206-212
                apply_givens(col, i, i + 1, *J[(i, p)])
            J[(j, p)] = givens(col[j], col[j + 1])       # new rotation :214-219
            apply_givens(col, j, j + 1, *J[(j, p)])
            scol = S[:, p]
            apply_givens(scol, j, j + 1, *J[(j, p)])     # :222-228
            resmax = max(resmax, float(np.ldexp(abs(S[j + 1, p]), int(e[p]) - E)))
        H.append(Hj)
        residual = resmax / beta                         # :230-231
        history.append(float(residual))
        if residual < tol or (length >= 0).all():        # :235-241
            converged = True
            break
    used = (j if reference_quirk else j + 1) if converged else max_num_iter
    for p in range(nrhs):                                # :245-285
        k = used if length[p] < 0 else min(int(length[p]), used)
        y = np.zeros(k, dtype=np.complex128)
        for r in range(k - 1, -1, -1):                   # ztrsv, upper, non-unit
            acc = S[r, p]
            for c in range(r + 1, k):
                acc = acc - H[c][r, p] * y[c]
            y[r] = acc / H[r][r, p]
        y = _ldexp(y, int(e[p]))
        x = X0[:, p].copy()
        for i in range(k):
            if y[i] != 0:                                # a zero coefficient adds nothing, as on the device
                x = x + V[i][:, p] * y[i]
        X[:, p] = x
    return (X[:, 0] if one_d else X), used, history
