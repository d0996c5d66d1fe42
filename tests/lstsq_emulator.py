"""A numpy fp64 restatement of what the device does for one least-squares problem (bfhip_lstsq.hip: bfQrcpKernel,
bfJacobiKernel / bfJacobiFinish, bfJacobiFreeze, the two GEMMs), in the manner of tests/plan_emulator.py: the round-robin
order, the rotation of bfJacobiAngle, the freezing of columns below dim eps x the largest column, the QR stop rule and
the truncation rule.  The arithmetic is numpy's (not the device's summation order), so results agree with the device to
rounding, not bit for bit; what the emulator settles is the behaviour of the RULES, on the CPU:

* `freeze="each"` / `qr_stop="max"` are the rules before the sum rule (every column below the threshold frozen; QR stopped
  at the first step whose largest trailing column is below it), `"sum"` the ones the kernels use now;
* `finish="fmax"` is the finish that let a NaN through (an fmax that ignores it, no flag), `"finite"` the one that flags it;
* `qr_rank0="fail"` counted a QR rank of 0 as a failure, `"nonfinite"` only a matrix that is not finite.

Mutants (`mutant=`) for the bound tests: "phase" (e^{+i phi} instead of e^{-i phi}), "short" (one rotating sweep fewer),
"thresh2x" (the truncation tol doubled), "drop" (the smallest kept sigma dropped)."""
from __future__ import annotations

import numpy as np

from lstsq_ref import EPS, round_robin, rotate_step

MAX_SWEEPS = 40


def _freeze(s2, dead2, rule):
    """(frozen mask, the dead2 bfJacobiAngle gets) -- bfJacobiFreeze, or the older per-column rule."""
    if rule == "each":
        return ~(s2 >= dead2), dead2
    small = s2 < dead2
    if np.sum(s2[small]) < dead2:
        return ~(s2 >= dead2), dead2
    frozen = np.zeros(len(s2), dtype=bool)
    acc = 0.0
    for j in range(len(s2)):
        if s2[j] < dead2 and acc + s2[j] < dead2:
            acc += s2[j]
            frozen[j] = True
    return frozen, 0.0


def jacobi(A, dim, freeze="sum", finish="finite", mutant=None, max_sweeps=MAX_SWEEPS):
    """bfJacobiKernel (resident schedule) on A (mt x me): (W = A V, V, scale, sweeps, converged)."""
    mt, me = A.shape
    S = np.zeros((mt + me, me), dtype=np.complex128)
    S[:mt] = A
    S[mt:] = np.eye(me)
    tol2 = mt * EPS * EPS
    with np.errstate(invalid="ignore", over="ignore"):
        n2 = np.sum(A.real ** 2 + A.imag ** 2, axis=0)
        mx = np.max(n2) if me else 0.0                           # the device's atomicMax on the bit pattern: NaN wins
        if np.any(np.isnan(n2)):
            mx = np.nan
    dead2 = (dim * EPS) ** 2 * mx
    sweep, converged = 0, False
    sweeps_cap = max_sweeps
    if mutant == "short":
        _, _, _, full, _ = jacobi(A, dim, freeze, finish, None, max_sweeps)
        sweeps_cap = max(full - 2, 0)
    while sweep < sweeps_cap:
        with np.errstate(invalid="ignore", over="ignore"):
            s2 = np.sum(S[:mt].real ** 2 + S[:mt].imag ** 2, axis=0)
            frozen, adead = _freeze(s2, dead2, freeze)
        live = np.nonzero(~frozen)[0]
        if len(live) < 2:
            converged = True
            break
        M = len(live) + (len(live) & 1)
        rotated = False
        for s in range(M - 1):
            p, q = round_robin(M, s)
            keep = q < len(live)
            if np.any(keep):
                with np.errstate(invalid="ignore", over="ignore"):
                    rotated |= rotate_step(S, mt, live[p[keep]], live[q[keep]], tol2, adead, conj_phase=mutant == "phase")
        if not rotated:
            converged = True
            break
        sweep += 1
    if mutant == "short":
        converged = True
    W, V = S[:mt], S[mt:]
    with np.errstate(invalid="ignore", over="ignore"):
        s2 = np.sum(W.real ** 2 + W.imag ** 2, axis=0)
    finite = bool(np.all(np.isfinite(s2)))
    smax = np.sqrt(np.nanmax(s2)) if me and not np.all(np.isnan(s2)) else 0.0
    if finish == "finite" and not finite:
        converged = False
    tol = dim * EPS * smax + EPS
    if mutant == "thresh2x":
        tol *= 2
    with np.errstate(invalid="ignore", divide="ignore"):
        keep = np.sqrt(s2) >= tol
        scale = np.where(keep, 1.0 / s2, 0.0)
    if mutant == "drop" and np.any(keep):
        j = np.nonzero(keep)[0][np.argmin(s2[keep])]
        scale[j] = 0.0
    return W, V, scale, sweep + (1 if converged else 0), converged


def qrcp(A, B, dim, stop="sum"):
    """bfQrcpKernel: (Xq = (R[0:r] P^T)^H (me x r), Q^H B, r, nonfinite)."""
    A = A.copy()
    B = B.copy()
    mt, me = A.shape
    with np.errstate(invalid="ignore", over="ignore"):
        cn = np.sum(A.real ** 2 + A.imag ** 2, axis=0)
    nonfinite = not np.all(np.isfinite(cn))
    perm = np.arange(me)
    mx = np.max(np.where(np.isnan(cn), -1, cn)) if me else 0.0
    dead2 = (dim * EPS) ** 2 * mx
    steps = 0 if nonfinite else min(mt, me)
    j = 0
    while j < steps:
        rest = cn[j:]
        p = j + int(np.argmax(rest))
        best, total = cn[p], float(np.sum(rest))
        crit = total if stop == "sum" else best
        if not (crit >= dead2) or best <= 0:
            break
        if p != j:
            A[:, [j, p]] = A[:, [p, j]]
            cn[[j, p]] = cn[[p, j]]
            perm[[j, p]] = perm[[p, j]]
        x = A[j:, j].copy()
        nx = np.sqrt(best)
        a0 = abs(x[0])
        ph = x[0] / a0 if a0 > 0 else 1.0
        u = x.copy()
        u[0] += ph * nx
        coef = 1.0 / (nx * (nx + a0))
        A[j, j] = -ph * nx
        A[j + 1:, j] = 0
        for M in (A[:, j + 1:], B):
            M[j:] -= coef * np.outer(u, np.conj(u) @ M[j:])
        cn[j + 1:] = np.sum(np.abs(A[j + 1:, j + 1:]) ** 2, axis=0)
        j += 1
    r = j
    Xq = np.zeros((me, r), dtype=np.complex128)
    R = np.triu(A[:r])
    Xq[perm] = np.conj(R).T
    return Xq, B, r, nonfinite


def solve(A, B, qr=False, freeze="sum", qr_stop="sum", finish="finite", qr_rank0="nonfinite", mutant=None):
    """(X, sigma kept descending, rank, flagged) as the device computes them."""
    A = np.asarray(A, dtype=np.complex128)
    B = np.asarray(B, dtype=np.complex128)
    mt, me = A.shape
    dim = max(mt, me)
    flagged = False
    if qr:
        Xq, QB, r, nonfinite = qrcp(A, B, dim, qr_stop)
        flagged = nonfinite or (qr_rank0 == "fail" and r == 0)
        if nonfinite:
            r = 0
            Xq = Xq[:, :0]
        W, V1, scale, _, conv = jacobi(Xq, dim, freeze, finish, mutant)
        T = (np.conj(V1).T @ QB[:r]) * scale[:, None]
        X = W @ T if r else np.zeros((me, B.shape[1]), dtype=np.complex128)
    else:
        W, V, scale, _, conv = jacobi(A, dim, freeze, finish, mutant)
        with np.errstate(invalid="ignore", over="ignore"):
            T = (np.conj(W).T @ B) * scale[:, None]
            X = V @ T
    flagged = flagged or not conv
    kept = scale > 0
    sig = np.sort(np.sqrt(1.0 / scale[kept]))[::-1]
    return X, sig, int(np.count_nonzero(kept)), flagged
