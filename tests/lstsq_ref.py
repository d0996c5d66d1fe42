"""Test infrastructure: an extended-precision reference for the builder's truncated-SVD least-squares solve
(bfhipLstSqTruncated: X = pinv_k(A) B with the reference's truncation rule, src/mat_dense_complex.c:1767-1849), and the
error bounds every device result must meet.

The reference.  `reference(A, B)` runs a one-sided (Hestenes) Jacobi SVD to full convergence in `np.clongdouble` (u_ld =
2^-64 on x86-64) on the STORED fp64 matrix -- no column is ever frozen, rotations stop only when every pair is orthogonal to
~mt u_ld -- and applies the reference's rule: sigma_j is kept iff sigma_j >= tol = max(mt, me) eps sigma_max + eps
(eps = 2^-52).  It does not lean on the factors a case was designed from: rounding A to fp64 has already moved those by
u ||A||, which at kappa ~ 1e8 is far more than the device's own error.  Its rotation is the device's formula
(bfJacobiAngle), so `tests/test_lstsq_cpu.py` checks it two independent ways: against designed factors (A = U S V^H from
long-double Householder products, `designed`) and against numpy's LAPACK (`oracle.helm2_build.lstsq_truncated`).

The bounds (u = 2^-53; dim = max(mt, me); sigma_1 >= ... >= sigma_k the kept singular values; kappa = sigma_1 / sigma_k;
r = B - A X the reference residual).
* Backward error of the device.  A one-sided Jacobi SVD in fp64 returns the exact SVD of A + dA with ||dA|| <= c1 dim u ||A||
  per sweep set (each rotation is a backward-stable 2 x 2 unitary, Demmel & Veselic 1992, Drmac 1997); the QR stage adds the
  same order (Householder QR, Higham 19.3); columns frozen below the threshold are dropped with ||dropped||_2 <=
  ||dropped||_F < dim eps sigma_max = 2 dim u sigma_1 -- the sum rule of bfJacobiFreeze and the QR stop guarantee exactly
  that.  So ||dA|| <= eta sigma_1 with eta = C dim u.  The two GEMMs add dim u relative to |W^H| |B| and |V| |T|.
* Singular values (Weyl): |sigma_j(device) - sigma_j(ref)| <= eta sigma_1.  `sigma_bound` uses C_SIGMA = 8.
* Rank.  If the spectrum keeps a gap of >= 4x on each side of tol (sigma_k >= 4 tol, sigma_{k+1} <= tol / 4), a
  perturbation of eta sigma_1 << tol cannot move any sigma across tol, so the rank is determined and must be equal.
* X (Wedin's theorem for the rank-k truncated least-squares problem, Higham 20.1 / Stewart & Sun III.3): with dA as above
  and dB of norm <= dim u ||B||,
      ||X_dev - X_ref|| <= c eta (kappa ||X|| + kappa ||B|| / sigma_1 + kappa^2 ||r|| / sigma_1),
  to first order in eta kappa.  `x_bound` uses C_X = 8 (2-norms bounded by Frobenius norms on the right).
The constants were set from the emulator (tests/lstsq_emulator.py) on every catalogue case: its measured ratio to the bound
stays below 0.25, and the deliberate mutants of the emulator (phase conjugated the wrong way, one sweep short, threshold off
by 2x, one kept sigma dropped) exceed it -- tests/test_lstsq_cpu.py checks both."""
from __future__ import annotations

import numpy as np

EPS = 2.0 ** -52          # DBL_EPSILON, the eps of the truncation rule
U = 2.0 ** -53
C_SIGMA = 8.0
C_X = 8.0
LD = np.clongdouble


def round_robin(M, s):
    """(p, q) of step s of the device's round-robin tournament over M (even) players (bfRoundRobin)."""
    kk = np.arange(M // 2)
    p = np.where(kk == 0, M - 1, (s + kk) % (M - 1))
    q = np.where(kk == 0, s, (s + (M - 1) - kk) % (M - 1))
    return np.minimum(p, q), np.maximum(p, q)


def rotate_step(S, mt, p, q, tol2, dead2, conj_phase=False):
    """One round-robin step of disjoint pairs on the stacked columns S = [A; V] (bfJacobiKernel's rotatePair and
    bfJacobiAngle), vectorised over the pairs; S's dtype sets the arithmetic.  Returns whether any pair rotated."""
    x, y = S[:mt, p], S[:mt, q]
    alpha = np.sum(x.real ** 2 + x.imag ** 2, axis=0)
    beta = np.sum(y.real ** 2 + y.imag ** 2, axis=0)
    g = np.sum(np.conj(x) * y, axis=0)
    g2 = g.real ** 2 + g.imag ** 2
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = ~((alpha < dead2) | (beta < dead2)) & (g2 > tol2 * alpha * beta) & (g2 != 0)
    if not np.any(ok):
        return False
    p, q, alpha, beta, g, g2 = p[ok], q[ok], alpha[ok], beta[ok], g[ok], g2[ok]
    gabs = np.sqrt(g2)
    zeta = (beta - alpha) / (2 * gabs)
    t = np.copysign(np.ones_like(zeta), zeta) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
    c = 1 / np.sqrt(1 + t * t)
    sn = c * t
    e = np.conj(g) / gabs if not conj_phase else g / gabs          # e^{-i phi}
    X, Y = S[:, p], S[:, q] * e
    S[:, p] = c * X - sn * Y
    S[:, q] = sn * X + c * Y
    return True


def reference(A, B, max_sweeps=60):
    """(X, sigma kept descending, rank) of the stored fp64 problem, in long double, to full convergence."""
    A = np.asarray(A, dtype=np.complex128)
    mt, me = A.shape
    dim = max(mt, me)
    S = np.zeros((mt + me, me), dtype=LD)
    S[:mt] = A.astype(LD)
    S[mt:] = np.eye(me, dtype=LD)
    M = me + (me & 1)
    uld = float(np.finfo(np.longdouble).eps)
    tol2 = (mt * uld) ** 2
    # columns below dim u_ld x the largest are zero at this precision (2^11 below anything the fp64 rule could keep);
    # rotating them only chases long-double noise (wide problems end with me - mt of them)
    n2 = np.sum(S[:mt].real ** 2 + S[:mt].imag ** 2, axis=0)
    dead2 = (dim * uld) ** 2 * (np.max(n2) if me else 0)
    for _ in range(max_sweeps):
        rotated = False
        for s in range(M - 1):
            p, q = round_robin(M, s)
            keep = q < me
            if np.any(keep):
                rotated |= rotate_step(S, mt, p[keep], q[keep], tol2, dead2)
        if not rotated:
            break
    else:
        raise AssertionError("long-double Jacobi did not converge")
    W, V = S[:mt], S[mt:]
    sig = np.sqrt(np.sum(W.real ** 2 + W.imag ** 2, axis=0))
    smax = float(np.max(sig)) if me else 0.0
    tol = dim * EPS * smax + EPS
    kept = sig >= tol
    T = (np.conj(W[:, kept]).T @ np.asarray(B, dtype=np.complex128).astype(LD)) / (sig[kept] ** 2)[:, None]
    X = V[:, kept] @ T
    return X, np.sort(sig[kept].astype(np.float64))[::-1], int(np.count_nonzero(kept))


def truncation_tol(sigma_max, dim):
    return dim * EPS * sigma_max + EPS


def householder_basis(m, k, rng):
    """First k columns of a product of k random complex Householder reflectors, formed in long double (orthonormal to
    ~u_ld)."""
    Q = np.zeros((m, k), dtype=LD)
    Q[np.arange(k), np.arange(k)] = 1
    for j in reversed(range(k)):
        v = (rng.standard_normal(m - j) + 1j * rng.standard_normal(m - j)).astype(LD)
        v /= np.sqrt(np.sum(np.abs(v) ** 2))
        Q[j:] -= 2 * np.outer(v, np.conj(v) @ Q[j:])
    return Q


def designed(mt, me, n, sigmas, seed, rhs="range"):
    """A = U diag(sigmas) V^H (long double factors, rounded to fp64 once) and B: rhs = "range" (B = U C: zero residual),
    "random" (a generic B).  Returns (A, B, X_designed) -- X from the factors, in long double."""
    rng = np.random.default_rng(seed)
    sigmas = np.asarray(sigmas, dtype=np.longdouble)
    k = len(sigmas)
    Uf, Vf = householder_basis(mt, k, rng), householder_basis(me, k, rng)
    A_ld = (Uf * sigmas) @ np.conj(Vf).T
    if rhs == "range":
        B_ld = Uf @ (rng.standard_normal((k, n)) + 1j * rng.standard_normal((k, n))).astype(LD)
    else:
        B_ld = (rng.standard_normal((mt, n)) + 1j * rng.standard_normal((mt, n))).astype(LD)
    B = B_ld.astype(np.complex128)
    X = (Vf / sigmas) @ (np.conj(Uf).T @ B.astype(LD))
    return A_ld.astype(np.complex128), B, X


def x_bound(A, B, X_ref, sigma_ref):
    """The allowed ||X_dev - X_ref||_F (module docstring)."""
    mt, me = A.shape
    dim = max(mt, me)
    if len(sigma_ref) == 0:
        return 4 * dim * U * float(np.linalg.norm(np.asarray(X_ref, dtype=np.complex128))) + 1e-300
    s1, sk = float(sigma_ref[0]), float(sigma_ref[-1])
    kappa = s1 / sk
    Xr = np.asarray(X_ref, dtype=np.complex128)
    r = np.asarray(B, dtype=np.complex128).astype(LD) - A.astype(LD) @ np.asarray(X_ref, dtype=LD)
    nr = float(np.linalg.norm(r.astype(np.complex128)))
    eta = C_X * dim * U
    return eta * (kappa * float(np.linalg.norm(Xr)) + kappa * float(np.linalg.norm(B)) / s1 + kappa ** 2 * nr / s1)


def sigma_bound(A, sigma_ref):
    dim = max(A.shape)
    return C_SIGMA * dim * U * (float(sigma_ref[0]) if len(sigma_ref) else 0.0)


def has_gap(sigma_all, dim, factor=4.0):
    """The rank is determined: no singular value within `factor` of tol on either side."""
    s = np.sort(np.asarray(sigma_all, dtype=np.float64))[::-1]
    if len(s) == 0 or s[0] == 0:
        return True
    tol = truncation_tol(s[0], dim)
    return bool(np.all((s >= factor * tol) | (s <= tol / factor)))
