"""Test infrastructure: a numpy restatement of mixed-precision GMRES refinement
(butterfly_amd/csrc/bfhip_refine.c).  The outer loop computes true residuals
with a complex128 matvec; each correction is solved by oracle/linalg_ref.py's
GMRES on a complex64 model of the operator, on the residual scaled to unit norm
per column; the solve stops at tol, after max_outer steps, or when a step does
not halve the residual, and returns the iterate of the smallest residual.
Every norm is taken of the column scaled by a power of two (`column_norms`), as
the device takes it: right-hand sides of 2^-600 or 2^+600 neither vanish nor
overflow."""
from __future__ import annotations

import numpy as np

from oracle import linalg_ref

INNER_TOL_DEFAULT = 1e-6          # BfhipGmresRefineOptions.innerTol = 0
# outer steps the restatement needs on bie.second_kind_case(2048, 128), three random columns (seed 7), tol 1e-12,
# default inner tolerance (tests/test_gmres_refine_cpu.py checks it; the GPU tests allow one more).  3 while the inner
# GMRES kept the reference's quirk of building a converged solution from one basis vector fewer than its estimate describes
OUTER_STEPS_2048 = 2


def c64_model(plan_only_c64_op):
    """The complex64 operator as the device applies it inside refinement: the input rounded to complex64, the plan
    run with double accumulation (tests/plan_emulator.py), the result stored as complex64, promoted back."""
    import plan_emulator

    def mv(v):
        v = np.asarray(v)
        v2 = v if v.ndim == 2 else v[:, None]
        y = plan_emulator.run_plan(plan_only_c64_op, v2.astype(np.complex64)).astype(np.complex128)
        return y if v.ndim == 2 else y[:, 0]
    return mv


def true_residual(matmul, B, X):
    """max_p ||b_p - A x_p|| / ||b_p|| (a column with b_p = 0: ||A x_p||)."""
    B = B if B.ndim == 2 else B[:, None]
    X = X if X.ndim == 2 else X[:, None]
    rn = np.linalg.norm(B - matmul(X), axis=0)
    bn = np.linalg.norm(B, axis=0)
    return float(np.max(np.where(bn > 0, rn / np.where(bn > 0, bn, 1), rn)))


def _ldexp(z, e):
    return np.ldexp(z.real, e) + 1j * np.ldexp(z.imag, e)


def column_norms(R, scaled=True):
    """(R 2^-e, ||R 2^-e||, e) per column, e = the binary exponent of the column's largest component (0 for a zero or
    non-finite column, and everywhere with scaled=False): the sum of squares neither underflows nor overflows, and where it
    would not have anyway the norm 2^e ||R 2^-e|| is the unscaled one bit for bit (a power of two commutes with every
    rounding on the way)."""
    big = np.maximum(np.abs(R.real), np.abs(R.imag)).max(axis=0)
    e = np.zeros(R.shape[1], dtype=np.int64)
    if scaled:
        ok = (big > 0) & np.isfinite(big)
        e[ok] = np.frexp(big[ok])[1]
    Rs = _ldexp(R, -e[None, :])
    return Rs, np.linalg.norm(Rs, axis=0), e


def solve_refine(matmul, matmul_low, B, X0=None, tol=1e-12, inner_tol=INNER_TOL_DEFAULT, max_outer=10, max_inner=100, msolve=None,
                 return_iterates=False, scaled=True, residual_matmul=None, update=None, keep_best=True, guard_zero=True):
    """Returns (X, num_outer, num_inner, history), and with return_iterates the list [X_1, ..., X_k] after them.

    The remaining keywords exist for tests/test_refine_highprec_cpu.py, whose deliberately wrong restatements (mutants)
    must break the checks of tests/refine_highprec.py: `scaled=False` takes the norms from unscaled squares,
    `residual_matmul` replaces the operator of the residual, `update(X, s, D)` replaces X + s D, `keep_best=False`
    returns the last iterate, `guard_zero=False` divides a zero column by its norm and lets the result through."""
    B = np.asarray(B, dtype=np.complex128)
    one_d = B.ndim == 1
    if one_d:
        B = B[:, None]
    n, nrhs = B.shape
    X = np.zeros_like(B) if X0 is None else np.asarray(X0, dtype=np.complex128).reshape(n, nrhs).copy()
    rmat = residual_matmul or matmul
    update = update or (lambda X, s, D: X + s * D)
    _, bs, be = column_norms(B, scaled)
    bn = np.ldexp(bs, be)

    def residual(X):
        Rs, rs, e = column_norms(B - rmat(X), scaled)
        rn = np.ldexp(rs, e)
        return Rs, rs, rn, float(np.max(np.where(bn > 0, rn / np.where(bn > 0, bn, 1), rn)))

    Rs, rs, rn, r = residual(X)
    history = [r]
    iterates = []
    best, best_res = X, r
    k = inner = 0
    while k < max_outer and not r <= tol and np.isfinite(r):
        live = rs > 0 if guard_zero else np.ones(nrhs, dtype=bool)
        with np.errstate(all="ignore"):
            Rhat = np.where(live, Rs / np.where(live, rs, 1), 1 / np.sqrt(n))   # zero column: unit right-hand side, scale 0
        D, it, _ = linalg_ref.solve_gmres(matmul_low, Rhat, tol=inner_tol, max_num_iter=max_inner, msolve=msolve)
        inner += it
        # linalg_ref treats a non-finite column as a dead one and returns zeros for it, and 0 * 0 would hide the 0/0.  The mutant
        # models a device without either guard: the solve of a NaN right-hand side is NaN and the update forms 0 * NaN
        if not guard_zero:
            D = np.where(np.isfinite(Rhat).all(axis=0), D, np.nan)
        X = update(X, np.where(rs > 0, rn, 0) if guard_zero else rn, D)
        iterates.append(X)
        k += 1
        Rs, rs, rn, rk = residual(X)
        history.append(rk)
        if rk < best_res or not keep_best:
            best, best_res = X, rk
        stagnated = not rk < 0.5 * r
        r = rk
        if stagnated:
            break
    out = (best[:, 0] if one_d else best), k, inner, history
    return out + (iterates,) if return_iterates else out
