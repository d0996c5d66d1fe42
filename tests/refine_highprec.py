"""Test infrastructure: what a mixed-precision GMRES refinement result (bfhipSolveGMRESRefine[Device], bfhip_refine.c, or its
restatement tests/refine_ref.py) must meet, judged in long double.

Every norm and residual here is `np.clongdouble` through `gmres_highprec.Problem.plain` (the operator the device compiles,
evaluated in long double; 2^+-600 needs no scaling in its exponent range).  The problem is the plain one: the refinement's left
preconditioner acts inside the correction solves only, the residuals it reports are those of A x = b.

With u = 2^-53, c = gmres_highprec.C_BOUND and x0 = 0 where there is none, one complex128 evaluation of b_p - A X_p has the
normwise floor

    f_p = c sqrt(n) u (||b_p|| + ||A|| ||X_p||)

(a matvec and a subtraction: sums of n products, sqrt(n) u each; the norm and the division that follow add a few u to a
quantity the floor dominates).  t_p = ||b_p - A X_p|| in long double, and as bfhip_refine.c documents

    rho(X) = max_p t_p / ||b_p||   (a column with b_p = 0: t_p itself),      phi(X) = max_p f_p / ||b_p||   (b_p = 0: f_p).

|max_p a_p - max_p b_p| <= max_p |a_p - b_p|, so a reported rho computed in complex128 lies within phi of the long-double one.

`check` returns a list of failures, each starting with the name of its check:

  finite       X is finite wherever B and X0 are, and with them finite so are the residual and the history (an iterate that
               went non-finite is never returned, being never the best: the history is where it shows);
  consistency  |residual - rho(X)| <= phi(X); with the iterates X_1..X_k given, |history[j] - rho(X_j)| <= phi(X_j) for every j
               that has one, history[0] judged against X0;
  best         residual == min(history) as floats, and history[-1] == residual unless the last step stagnated;
  stop         len(history) == k + 1 <= max_outer + 1; every step that was continued started above tol and halved,
               history[j+1] < 0.5 history[j] for j < k - 1; the last step meets tol, or fails to halve, or k == max_outer; with
               k == 0, history[0] <= tol;
  forward      ||X_p - x*_p|| <= kappa / ||A|| (t_p + f_p), x* the solution to long-double accuracy (`solution`).  The bound
               holds for ANY X when x* and t_p are right (||x - x*|| <= ||A^-1|| ||b - A x||): it ties the long-double residual,
               the designed ||A|| and kappa and the independently computed x* to one another, and cannot tell a poor iterate
               from a good one.  That is the next check's part;
  converged    (cases the catalogue marks as converging) residual <= tol;
  untouched    a column whose initial residual is exactly zero is x0 (or +0.0 zeros) bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

import gmres_highprec as gh
from gmres_highprec import LD, _cols, _norm

CHECKS = ("finite", "consistency", "best", "stop", "forward", "converged", "untouched")


def rho_phi(pb, B, X):
    """(rho, phi, t, f): the long-double relative residual of X, its complex128 floor, and per column t_p and f_p."""
    B, X = _cols(B), _cols(X)
    t = _norm(B.astype(LD) - pb.plain(X))
    nb, nx = _norm(B), _norm(X)
    f = np.longdouble(gh.C_BOUND * math.sqrt(B.shape[0]) * gh.U) * (nb + np.longdouble(pb.norm_a) * nx)
    den = np.where(nb > 0, nb, np.longdouble(1))
    return (t / den).max(), (f / den).max(), t, f


def solution(pb, op, B):
    """x* with A x* = b to long-double accuracy: the fp64 solve (the dense matrix, or for the block-diagonal operators of
    unitary blocks the conjugate transposes) corrected by long-double residuals until the long-double residual stops falling."""
    B = _cols(B)
    if op.dense is not None:
        solve = lambda R: np.linalg.solve(op.dense, R)
    else:                                       # blockdiag:*: 16 x 16 unitary leaves in order, then the ragged tail
        leaves = [op.vals[k] for k in sorted(op.vals)]

        def solve(R):
            out, r0 = np.empty_like(R), 0
            full = [v for v in leaves if v.shape == (16, 16)]
            nfull = len(full)
            Q = np.stack(full).conj().transpose(0, 2, 1)
            out[:16 * nfull] = np.einsum("bij,bjk->bik", Q, R[:16 * nfull].reshape(nfull, 16, -1)).reshape(16 * nfull, -1)
            r0 = 16 * nfull
            for v in leaves[nfull:]:
                out[r0:r0 + v.shape[0]] = np.linalg.solve(v, R[r0:r0 + v.shape[0]])
                r0 += v.shape[0]
            return out
    # columns of 2^+-600: solve the column scaled into range, scale the correction back (exact)
    big = np.maximum(np.abs(B.real), np.abs(B.imag)).max(axis=0)
    e = np.where(big > 0, np.frexp(np.where(big > 0, big, 1))[1], 0)
    ldexp = lambda Z, s: (np.ldexp(Z.real, s) + 1j * np.ldexp(Z.imag, s))
    X = np.zeros(B.shape, dtype=LD)
    R = B.astype(LD)
    best = _norm(R)
    for _ in range(8):
        # long double has no ldexp of complex arrays worth the name: scale through float64 parts, which are exact powers of two
        Rs = (R * np.ldexp(np.longdouble(1), -e)[None, :]).astype(np.complex128)
        D = solve(Rs).astype(LD) * np.ldexp(np.longdouble(1), e)[None, :]
        Xn = X + D
        Rn = B.astype(LD) - pb.plain(Xn)
        nn = _norm(Rn)
        if not np.any(nn < best):
            break
        keep = nn < best
        X = np.where(keep[None, :], Xn, X)
        R = np.where(keep[None, :], Rn, R)
        best = np.where(keep, nn, best)
    return X


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check(pb, B, X0, result, tol, max_outer, iterates=None, xstar=None, zero_cols=(), converges=False):
    """`result` = (X, num_outer, num_inner, residual, history).  `iterates`: [X_1, ..., X_k], an entry None where it is not
    known (the device returns the best iterate only).  `xstar`: `solution(...)`, computed once per case by the caller."""
    X, k, _, residual, history = result
    B = _cols(np.asarray(B, dtype=np.complex128))
    X = _cols(np.asarray(X, dtype=np.complex128))
    n, nrhs = B.shape
    X0 = np.zeros_like(B) if X0 is None else _cols(np.asarray(X0, dtype=np.complex128))
    history = [float(h) for h in history]
    out = []
    ok_in = np.isfinite(B).all(axis=0) & np.isfinite(X0).all(axis=0)
    bad = [p for p in range(nrhs) if ok_in[p] and not np.isfinite(X[:, p]).all()]
    if bad:
        return [f"finite: non-finite X in columns {bad}"]
    if ok_in.all() and not (np.isfinite(history).all() and np.isfinite(residual)):
        return [f"finite: residual {residual!r}, history {history} of finite input"]

    # stop rule
    if len(history) != k + 1 or k > max_outer:
        out.append(f"stop: len(history) = {len(history)}, num_outer = {k}, max_outer = {max_outer}")
    else:
        for j in range(k):
            if not history[j] > tol:
                out.append(f"stop: step {j + 1} was taken from history[{j}] = {history[j]:.3e} <= tol")
        for j in range(k - 1):
            if not history[j + 1] < 0.5 * history[j]:
                out.append(f"stop: continued after history[{j + 1}] = {history[j + 1]:.3e} >= half of {history[j]:.3e}")
        if k == 0:
            if not history[0] <= tol:
                out.append(f"stop: no step taken from history[0] = {history[0]:.3e} > tol")
        elif not (history[k] <= tol or not history[k] < 0.5 * history[k - 1] or k == max_outer):
            out.append(f"stop: stopped after {k} < {max_outer} steps at {history[k]:.3e}, halved and above tol")

    # best iterate
    if history and not residual == min(history):
        out.append(f"best: residual {residual!r} != min(history) {min(history)!r}")
    if len(history) >= 2 and history[-1] < 0.5 * history[-2] and not history[-1] == residual:
        out.append(f"best: the last step improved to {history[-1]!r} but {residual!r} is reported")

    # consistency
    rho, phi, t, f = rho_phi(pb, B, X)
    if not abs(np.longdouble(residual) - rho) <= phi:
        out.append(f"consistency: residual {residual:.6e} against rho(X) = {float(rho):.6e}, phi = {float(phi):.3e}")
    steps = [X0] + list(iterates) if iterates is not None else [X0]
    for j, Xj in enumerate(steps[:len(history)]):
        if Xj is None:
            continue
        rj, pj, _, _ = rho_phi(pb, B, Xj)
        if not abs(np.longdouble(history[j]) - rj) <= pj:
            out.append(f"consistency: history[{j}] = {history[j]:.6e} against rho(X_{j}) = {float(rj):.6e}, phi = {float(pj):.3e}")

    # forward
    if xstar is not None:
        fwd = _norm(X.astype(LD) - xstar)
        for p in range(nrhs):
            lim = np.longdouble(pb.kappa / pb.norm_a) * (t[p] + f[p])
            if not fwd[p] <= lim:
                out.append(f"forward: col {p}: ||X - x*|| = {float(fwd[p]):.3e} > kappa / ||A|| (t + f) = {float(lim):.3e}")

    if converges and not residual <= tol:
        out.append(f"converged: residual {residual:.3e} > tol {tol:.1e} after {k} steps, history {history}")

    for p in zero_cols:
        if not np.array_equal(_bits(X[:, p]), _bits(X0[:, p])):
            out.append(f"untouched: column {p} is not x0 bit for bit")
    return out
