"""A numpy fp64 restatement of bfhipTruncSvdDevice (butterfly_amd/csrc/bfhip_tsvd.c / .hip), in the
manner of tests/lstsq_emulator.py: the orientation and the padding to an even number of 16-column tiles, the round-robin
order of the tile pairs, the Gram-based pair solve (cyclic two-sided Jacobi on the pair's 32 x 32 Gram matrix, in the
parallel ordering the kernel uses, eigenvalues sorted so that the larger column norm comes first), the two thresholds and
the noise rule, the stop rule, the sort, the count rule and the recovery of U and W.  The arithmetic is numpy's, not the
device's summation order: results agree with the device to rounding, not bit for bit.  What the emulator settles, on the
CPU, is that the RULES converge and how many sweeps they need."""
from __future__ import annotations

import numpy as np

EPS = 2.0 ** -52
TILE = 16
PAIR = 2 * TILE
INNER_SWEEPS = 12          # BF_TSVD_INNER_SWEEPS
THR_IN = 2 * EPS           # the pair solve rotates an entry above this (relative)
DEFAULT_MAX_SWEEPS = 30


def thr_out(M):
    """An entry of a pair's Gram matrix counts as converged at or below this, relative (bfTsvdThreshold)."""
    return max(32.0, float(np.sqrt(float(M)))) * EPS


def noise_level(N):
    """A column whose norm is at or below this times the largest column norm of the block as it was loaded takes no part in a
    rotation (bfTsvdNoise): what the rotations' own rounding leaves in a column that is zero in exact arithmetic, which grows
    with the number of updates.  The level is global: relative to its pair's own largest column, a ladder of ever smaller
    noise columns (1e-14, 1e-15, ... of the largest) is live wherever no large column sits beside it, and converges linearly."""
    return (32.0 + N) * EPS


def padded_ld(N):
    """Columns rounded up to an even number of 16-column tiles (bfTsvdLd)."""
    return (N + PAIR - 1) // PAIR * PAIR


def round_robin_pair(nt, step, p):
    """Tile pair p of step `step` among nt (even) tiles, smaller index first (bfTsvdPair)."""
    r = nt - 1
    if p == 0:
        a, b = r, step % r
    else:
        a, b = (step + p) % r, (step + r - p) % r
    return (a, b) if a < b else (b, a)


def pair_solve(G, thr, noise):
    """The pair kernel on one 32 x 32 Gram matrix: (rotate?, Q, largest relative off-diagonal entry).  noise: the squared
    column norm at or below which a column is left alone."""
    n = G.shape[0]
    G = np.triu(G) + np.triu(G, 1).T
    d = np.diag(G).copy()
    den = np.sqrt(np.outer(d, d))
    live = (np.minimum.outer(d, d) > noise) & ~np.eye(n, dtype=bool)
    ratio = np.where(live, np.abs(G) / np.where(den > 0, den, 1.0), 0.0)
    off = float(ratio.max())
    if not off > thr:
        return False, None, off
    V = np.eye(n)
    steps = [np.array([round_robin_pair(n, step, k) for k in range(n // 2)]) for step in range(n - 1)]
    for _ in range(INNER_SWEEPS):
        rotated = False
        for pq in steps:
            p, q = pq[:, 0], pq[:, 1]               # 16 disjoint rotations, as the kernel's 16 lanes take them
            a, dd, b = G[p, p], G[q, q], G[p, q]
            go = (np.minimum(a, dd) > noise) & (np.abs(b) > THR_IN * np.sqrt(np.abs(a * dd)))
            if not go.any():
                continue
            rotated = True
            tau = (dd - a) / (2 * np.where(go, b, 1.0))
            t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1 + tau * tau))
            c = np.where(go, 1 / np.sqrt(1 + t * t), 1.0)
            s = np.where(go, t * c, 0.0)
            gp, gq = G[p].copy(), G[q].copy()       # rows: G <- J^T G
            G[p], G[q] = c[:, None] * gp - s[:, None] * gq, s[:, None] * gp + c[:, None] * gq
            gp, gq = G[:, p].copy(), G[:, q].copy() # columns: G <- G J, V <- V J
            G[:, p], G[:, q] = c * gp - s * gq, s * gp + c * gq
            vp, vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
        if not rotated:
            break
    order = np.argsort(-np.diag(G), kind="stable")
    return True, V[:, order], off


def block_jacobi(B, N, max_sweeps=DEFAULT_MAX_SWEEPS):
    """One-sided block Jacobi on B (M x ld, ld an even number of tiles, N columns in use), in place: (sweeps, converged, offNorm of the last sweep)."""
    M, ld = B.shape
    nt = ld // TILE
    thr = thr_out(M)
    noise = noise_level(N) ** 2 * float(np.max(np.sum(B * B, axis=0)))
    sweeps, off = 0, 0.0
    while sweeps < max_sweeps:
        sweeps += 1
        rotated, off = 0, 0.0
        for step in range(nt - 1):
            for p in range(nt // 2):
                ti, tj = round_robin_pair(nt, step, p)
                cols = np.r_[TILE * ti:TILE * ti + TILE, TILE * tj:TILE * tj + TILE]
                P = B[:, cols]
                need, Q, o = pair_solve(P.T @ P, thr, noise)
                off = max(off, o)
                if need:
                    B[:, cols] = P @ Q
                    rotated += 1
        if not rotated:
            return sweeps, True, off
    return sweeps, False, off


def trunc_svd(A, tol, max_sweeps=DEFAULT_MAX_SWEEPS):
    """bfhipTruncSvdDevice in numpy: dict(k, sigma, U, W, sweeps, transposed, converged, offNorm)."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    transposed = m < n
    T = A.T if transposed else A
    M, N = T.shape
    B = np.zeros((M, padded_ld(N)))
    B[:, :N] = T
    sweeps, conv, off = block_jacobi(B, N, max_sweeps)
    norms = np.sqrt(np.sum(B[:, :N] * B[:, :N], axis=0))
    order = np.argsort(-norms, kind="stable")
    sigma = norms[order]
    k = 0
    if sigma[0] > 0:
        while k < N and sigma[k] >= tol * sigma[0]:
            k += 1
    Bk = B[:, order[:k]]
    if transposed:
        W = np.ascontiguousarray(Bk.T)
        U = A @ (Bk / (sigma[:k] * sigma[:k]))
    else:
        U = Bk / sigma[:k]
        W = U.T @ A
    return dict(k=k, sigma=sigma, U=U, W=W, sweeps=sweeps, transposed=transposed, converged=conv, offNorm=off)
