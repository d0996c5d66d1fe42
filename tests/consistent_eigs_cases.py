"""Shared by tests/test_consistent_eigs_cpu.py and tests/test_gpu_consistent_eigs.py: the cases of the
consistent-mass pencil S u = theta B u of the device eigensolver (BFHIP_EIGS_CONSISTENT_MASS), their true spectra from a dense
generalised eigensolve, a numpy assembly of the P1 mass, and a float64 restatement of the algorithm
(reference_eigs_consistent): section 25's iteration with A = B^-1 S applied by a fixed number of Chebyshev semi-iterations,
Rayleigh-Ritz in the B inner product and the residual S u - theta B u.  Builders only: numpy, no GPU."""
import functools
import os

import numpy as np

import cheb_cases as cc
import eigs_cases as ec

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-10
U53 = 2.0 ** -53


# ---- the P1 mass, restated -------------------------------------------------------------------------------------------------------
def mass_dense(verts, faces):
    """(M, mass_lumped, area): per triangle of area A, A / 6 on the diagonal and A / 12 off it."""
    n = len(verts)
    M, lumped, area = np.zeros((n, n)), np.zeros(n), 0.0
    for f in faces.astype(np.int64):
        A = 0.5 * np.linalg.norm(np.cross(verts[f[1]] - verts[f[0]], verts[f[2]] - verts[f[0]]))
        for a in range(3):
            for b in range(3):
                M[f[a], f[b]] += A / 6 if a == b else A / 12
            lumped[f[a]] += A / 3
        area += A
    return M, lumped, area


def on_pattern(rowptr, colind, A):
    """The entries of the dense A at the CSR pattern's positions."""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr.astype(np.int64)))
    return np.ascontiguousarray(A[rows, colind.astype(np.int64)])


def fold_mass(rowptr, colind, mdata, d):
    """B[k] = (d[i] M[k]) d[col[k]], as bfhipChebCovSetConsistentMass folds."""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr.astype(np.int64)))
    return (d[rows] * mdata) * d[colind.astype(np.int64)]


# ---- the mass solve --------------------------------------------------------------------------------------------------------------
def default_mass_steps(lo, hi, tol):
    """The smallest k with 2 rho^k <= tol, rho = (sqrt(hi / lo) - 1) / (sqrt(hi / lo) + 1); at most 64."""
    sk = np.sqrt(hi / lo)
    rho = (sk - 1) / (sk + 1)
    k, bound = 1, 2 * rho
    while k < 64 and bound > tol:
        bound *= rho
        k += 1
    return k


def mass_solve(bmul, t, lo, hi, steps):
    """z ~ B^-1 t: `steps` steps of the three-term Chebyshev semi-iteration on [lo, hi] from z = 0 (the first has no product),
    the operations of bfdevEigsMassSolve in numpy."""
    theta = (hi + lo) / 2
    sigma = theta / ((hi - lo) / 2)
    inv = 1 / theta
    prev, cur = None, inv * t
    omega = 1.0
    for j in range(1, steps):
        omega = 2 * sigma * sigma / (2 * sigma * sigma - 1) if j == 1 else 1 / (1 - omega / (4 * sigma * sigma))
        nxt = (-omega * inv) * bmul(cur) + omega * cur
        if prev is not None:
            nxt = nxt + (1 - omega) * prev
        nxt = nxt + (omega * inv) * t
        prev, cur = cur, nxt
    return cur


# ---- matrices --------------------------------------------------------------------------------------------------------------------
class Pencil:
    """L and M on one CSR pattern, the lumped mass, what the object folds from them (S, B, d, lamMax) and [lo, hi] (None: the P1
    bounds, which the object must accept)."""
    def __init__(self, name, rowptr, colind, data, mass, mdata, bounds=None):
        self.name, self.rowptr, self.colind, self.data, self.mass, self.mdata = name, rowptr, colind, data, mass, np.ascontiguousarray(mdata)
        self.n = len(rowptr) - 1
        self.val, self.d, self.lam_max = cc.fold(rowptr, colind, data, mass)
        self.bval = fold_mass(rowptr, colind, self.mdata, self.d)
        self.bounds = bounds
        self.lo, self.hi = (0.25, 1.0) if bounds is None else bounds
        self.lam_max_g = self.lam_max / self.lo
        self.s_ell = cc.Ell(rowptr, colind, self.val, np.float64)
        self.b_ell = cc.Ell(rowptr, colind, self.bval, np.float64)
        self._truth = None

    def dense(self):
        S = cc.csr_to_dense(self.rowptr, self.colind, self.val, self.n)
        B = cc.csr_to_dense(self.rowptr, self.colind, self.bval, self.n)
        return (S + S.T) / 2, (B + B.T) / 2

    def truth(self, count=None):
        """(lam, U) of S u = lam B u, lowest first, U^T B U = I: Cholesky of B, numpy.linalg.eigh of C^-1 S C^-T."""
        if self._truth is None:
            S, B = self.dense()
            C = np.linalg.cholesky(B)
            A = np.linalg.solve(C, np.linalg.solve(C, S).T)
            lam, V = np.linalg.eigh((A + A.T) / 2)
            self._truth = lam, np.linalg.solve(C.T, V)
        count = self.n if count is None else count
        return self._truth[0][:count], self._truth[1][:, :count]


def sphere_fixture():
    mesh = np.load(os.path.join(HERE, "golden", "sphere_mesh_500.npz"))
    fix = np.load(os.path.join(HERE, "golden", "sphere_phi_500x32.npz"))
    return mesh["verts"], mesh["faces"], fix["lam"], fix["phi"]


def _p1(name, verts, faces):
    from butterfly_amd import trimesh_lbo_fem, trimesh_lbo_fem_mass
    rowptr, colind, data, mass = trimesh_lbo_fem(verts, faces)
    return Pencil(name, rowptr, colind, data, mass, trimesh_lbo_fem_mass(verts, faces, rowptr, colind))


@functools.lru_cache(maxsize=None)
def pencils():
    out = {}
    verts, faces, _, _ = sphere_fixture()
    out["sphere"] = _p1("sphere", verts, faces)
    out["n1"] = Pencil("n1", np.array([0, 1], dtype=np.uint64), np.array([0], dtype=np.uint64), np.array([3.0]), np.array([0.7]), np.array([0.7]))
    # the path of eigs_cases with the P1 mass of its four elements (lengths 1, 2, 0.5, 1.5) on the tridiagonal pattern; the object
    # has no lumped mass (D = I), so the row sums are not 1 and the bounds are the caller's
    p5 = cc.catalogue()["path5"]
    h = np.array([1.0, 2.0, 0.5, 1.5])
    M = np.zeros((5, 5))
    for e in range(4):
        M[e, e] += h[e] / 3; M[e + 1, e + 1] += h[e] / 3; M[e, e + 1] += h[e] / 6; M[e + 1, e] += h[e] / 6
    out["path5"] = _with_bounds("path5", p5["rowptr"], p5["colind"], p5["data"], None, on_pattern(p5["rowptr"], p5["colind"], M))
    out["mesh63"] = _p1("mesh63", *cc.jittered_grid_mesh())
    out["two_grids"] = _p1("two_grids", *ec.two_grids())
    # a caller's mass that is not the P1 one: half the P1 mass plus a diagonal that varies over the mesh
    g = _p1("grid33", *ec.regular_grid())
    extra = g.mass * (0.5 + 0.2 * np.sin(0.37 * np.arange(g.n)))
    md = 0.5 * g.mdata.copy()
    rows = np.repeat(np.arange(g.n), np.diff(g.rowptr.astype(np.int64)))
    diag = rows == g.colind.astype(np.int64)
    md[diag] += extra
    out["grid33"] = _with_bounds("grid33", g.rowptr, g.colind, g.data, g.mass, md)
    return out


def _with_bounds(name, rowptr, colind, data, mass, mdata):
    """explicit [lo, hi] from numpy.linalg.eigvalsh of B, widened by 1 %"""
    probe = Pencil(name, rowptr, colind, data, mass, mdata, bounds=(1.0, 2.0))
    ev = np.linalg.eigvalsh(probe.dense()[1])
    return Pencil(name, rowptr, colind, data, mass, mdata, bounds=(float(ev[0]) * 0.99, float(ev[-1]) * 1.01))


# (pencil, nev, guard (None: the default), locked count): p == n (exact first step, no filter), 2 + 1 on the path, the mesh, lambda = 0
# twice, the caller's mass
SMALL_CASES = [
    ("n1", 1, None, 0),
    ("path5", 5, None, 0),
    ("path5", 2, 1, 0),
    ("mesh63", 8, 8, 0),
    ("two_grids", 16, 8, 0),
    ("grid33", 33, 16, 0),
]
SPHERE_NEV, SPHERE_LOCKED, SPHERE_BAND = 81, 49, 32
# outer iterations reference_eigs_consistent took when the cases were made (tests/test_consistent_eigs_cpu.py prints them and holds the restatement to them); the device gets twice these
MEASURED_ITERS = {"sphere-81@1e-10": 6, "sphere-81@1e-12": 7, "sphere-band-32": 10, "n1-1-d": 0, "path5-5-d": 0, "path5-2-1": 2, "mesh63-8-8": 4,
                  "two_grids-16-8": 14, "grid33-33-16": 9}


def case_id(case):
    name, nev, guard, m = case
    return f"{name}-{nev}-{'d' if guard is None else guard}"


# ---- the algorithm in float64 ----------------------------------------------------------------------------------------------------
def _cholqr2_b(X, bmul, n, p):
    plain, shifted = 2, False
    while plain > 0:
        G = X.T @ bmul(X)
        try:
            L = np.linalg.cholesky(G)
            plain -= 1
        except np.linalg.LinAlgError:
            if shifted:
                return None
            shifted = True
            s = 11.0 * (n * p + p * (p + 1)) * 2.0 ** -53 * np.linalg.norm(G)
            L = np.linalg.cholesky(G + s * np.eye(p))
            plain = 2
        X = np.linalg.solve(L, X.T).T
    return X


def _rayleigh_ritz_b(smul, bmul, X, n, p, Q):
    if Q is not None:
        for _ in range(2):
            X = X - Q @ (Q.T @ bmul(X))
    X = _cholqr2_b(X, bmul, n, p)
    if X is None:
        return None
    Y = smul(X)
    H = X.T @ Y
    theta, W = np.linalg.eigh((H + H.T) / 2)
    X, Y = X @ W, Y @ W
    return X, Y, theta, np.linalg.norm(Y - bmul(X) * theta, axis=0)


def reference_eigs_consistent(pen, nev, guard=None, degree=None, tol=TOL, max_iter=100, seed=0, mass_steps=None, locked=None):
    """dict(lam, U, residual, iterations, converged, max_degree, p, mass_steps): the steps of the device call in numpy float64.
    locked: (Q [n, m] B-orthonormal eigenvectors, lam [m]) of the m lowest pairs."""
    full = pen.n
    Q, lam_q = (None, None) if locked is None else locked
    m = 0 if Q is None else Q.shape[1]
    n = full - m
    lam_top = pen.lam_max_g
    p = ec.block_columns(n, nev, guard)
    degree = 20 if degree is None else degree
    k = default_mass_steps(pen.lo, pen.hi, tol) if mass_steps is None else mass_steps
    smul, bmul = pen.s_ell.mul, pen.b_ell.mul
    X = ec.normal_stream(seed, np.arange(full * p, dtype=np.uint64)).reshape(full, p)
    X, Y, theta, res = _rayleigh_ritz_b(smul, bmul, X, full, p, Q)
    its, max_degree = 0, 0
    while True:
        conv = 0
        while conv < nev and res[conv] <= tol * lam_top:
            conv += 1
        if conv == nev or its == max_iter:
            break
        if p < n:
            a, a0, b = theta[-1], theta[0], lam_top
            e, c = (b - a) / 2, (b + a) / 2
            sigma1 = e / (a0 - c)
            tau = 2 / sigma1
            mdeg = ec.degree_cap(theta, lam_top, degree) if m == 0 else _degree_cap_locked(theta, lam_q.min(), lam_top, degree)
            max_degree = max(max_degree, mdeg)
            amul = lambda V: mass_solve(bmul, smul(V), pen.lo, pen.hi, k)
            prev, cur = X, sigma1 / e * amul(X) - sigma1 * c / e * X
            sigma = sigma1
            for _ in range(1, mdeg):
                sn = 1 / (tau - sigma)
                prev, cur = cur, 2 * sn / e * amul(cur) - 2 * sn * c / e * cur - sigma * sn * prev
                sigma = sn
            X = cur
        its += 1
        out = _rayleigh_ritz_b(smul, bmul, X, full, p, Q)
        if out is None:
            return dict(converged=-1, iterations=its, p=p, mass_steps=k)
        X, Y, theta, res = out
    return dict(lam=theta[:nev], U=X[:, :nev], residual=res[:nev], iterations=its, converged=conv, max_degree=max_degree, p=p, mass_steps=k,
                worst=float(res[:nev].max() / lam_top))


def _degree_cap_locked(theta, lock_min, lam_max, degree):
    """ec.degree_cap with the smallest locked eigenvalue as one more point (section 27): a, a0 stay the block's."""
    a, a0, b = theta[-1], theta[0], lam_max
    e, c = (b - a) / 2, (b + a) / 2
    sigma1 = e / (a0 - c)
    tau, sigma = 2 / sigma1, sigma1
    pts = np.append(theta, lock_min)
    y0, y1 = np.ones_like(pts), sigma1 / e * (pts - c)
    best = 1
    for mm in range(1, degree + 1):
        if mm > 1:
            sn = 1 / (tau - sigma)
            y0, y1 = y1, 2 * sn / e * (pts - c) * y1 - sigma * sn * y0
            sigma = sn
        lo, hi = np.abs(y1).min(), np.abs(y1).max()
        if np.isfinite(hi) and hi < 2.0 ** 23 * lo:
            best = mm
    return best


def cluster_distance(Mmul, V_fix, V_span):
    """max over the columns of V_fix of the M-norm of what its M-projection onto span(V_span) leaves (V_span M-orthonormal)."""
    R = V_fix - V_span @ (V_span.T @ Mmul(V_fix))
    return float(np.sqrt(np.einsum("ij,ij->j", R, Mmul(R)).max()))


SPHERE_CLUSTERS = ((49, 64), (64, 81))          # the l = 7 and l = 8 clusters of the fixture's band


def cluster_bound(residual, lam_true, a, b):
    """2 ||R_cluster||_F / delta + 2e-11 for the columns a .. b - 1: delta is the distance from the cluster to the nearest eigenvalue
    outside it (the factor 2 is 1 / sqrt(lo): the residuals are 2-norms, the sin-theta theorem wants the B^-1 norm), 2e-11 the
    fixture's own accuracy (the reference allows itself 1.12e-11 per entry)."""
    delta = min(lam_true[a] - lam_true[a - 1], lam_true[b] - lam_true[b - 1])
    return 2 * float(np.linalg.norm(residual[a:b])) / delta + 2e-11
