"""Cases of conditioning the Chebyshev route on observations (bfhipChebCovCondCreate).  Builders only:
numpy and the host entries of the library (the fold of the mesh, the Chebyshev fit), no GPU.  tests/test_cheb_condition_cpu.py
asserts what the cases claim on the reference alone; tests/test_gpu_cheb_condition.py holds the device to them.

Reference.  The field is z = B w, B = D p(S).  Its observed rows, transposed, are X = p(S) D E_obs [n x k], formed by the
reference's forward recurrence (tests/cheb_cases.py: forward_recurrence on Ell(S)) in numpy.longdouble; nothing is n x n dense.
G = X^T X, noise, Cholesky, solves and Z = D p(S) (W + X alpha) follow in long double with the helpers of
tests/test_gpu_cov_condition.py; likelihood and variances come from the same matrices (LikReference).  `f64` is the same sequence
in plain float64 numpy: its error against the long-double results is the yardstick the device is held to (8 times that,
DESIGN.md section 22), floored at fwd_bound(n, k, cond(G + D)).

Cases.  mesh4099 (five chunks of BF_COND_CHUNK = 1024 rows, the last of three: the ears 4096, 4097, 4098, which every observed set
with k >= 3 contains), mesh63 (under one chunk) and n1 (k = 1); k in {1, 33, 130} (130: panels of 64 + 64 + 2, more than one Gram
tile and Cholesky block); orders {1, 2, 64} of matern_density(2, 2) on [0, Gershgorin]; noise 0.01 trace(G) / k (0.5 + u); 70
columns (passes of 64 + 6) and 70 queries, 8 of them observed.  On the large mesh the long-double Z is formed for the columns
ZCOLS only (first and last of both passes); alpha is checked in every column."""
import numpy as np

import cheb_cases as cc
from cond_cases import CHUNK, chunk_sensitivity, solve_f64
from test_cov_likelihood_cpu import PI_LD, LikReference, forward_ld
from test_gpu_cov_condition import LD, Reference, col_errs, fwd_bound, solve_ld

RHO = 0.01
KS = (1, 33, 130)
QS = (1, 17, 64, 70)
ORDERS = (1, 2, 64)
MAXQ, NQUERY = 70, 70
ZCOLS = (0, 16, 63, 64, 69)
TOL = 1e-12                         # the project's float64 tolerance: a chunk left out must move alpha by 1e3 of these
EARS = (4096, 4097, 4098)


def cases_of(name):
    """(k, order) pairs run on the matrix `name`."""
    ks = {"n1": (1,), "mesh63": (1, 33)}.get(name, KS)              # observed vertices are distinct: k <= n
    return [(k, order) for k in ks for order in ORDERS]


class Matrix:
    """One matrix of cheb_cases.catalogue(): the folded S in both precisions, the W block and the fitted coefficients."""
    def __init__(self, name, spec):
        self.name, self.spec = name, spec
        self.n = len(spec["rowptr"]) - 1
        self.val, self.d, self.gersh = cc.fold(spec["rowptr"], spec["colind"], spec["data"], spec["mass"])
        self.lam_max = self.gersh
        self.ell = {dt: cc.Ell(spec["rowptr"], spec["colind"], self.val, dt) for dt in (LD, np.float64)}
        self.W = np.random.default_rng(4000 + self.n).standard_normal((self.n, MAXQ))
        self.zcols = np.arange(MAXQ) if self.n <= 1000 else np.array(ZCOLS)
        self._coef, self._cases, self._cols = {}, {}, {}
        # the observed sets of the large mesh are nested and its queries share their unobserved part, so that the long-double
        # recurrence runs once per column and order (rows_t keeps the columns): the ears, then 127 of the grid's vertices
        rng = np.random.default_rng(5000 + self.n)
        if self.n > max(KS) + NQUERY:
            grid = rng.permutation(self.n - 3 if name == "mesh4099" else self.n)
            self.pool = np.concatenate([np.array(EARS), grid[:max(KS) - 3]]) if name == "mesh4099" else grid[:max(KS)]
            self.other_queries = grid[max(KS):max(KS) + NQUERY - 8]
        else:
            self.pool, self.other_queries = rng.permutation(self.n), None

    def coef(self, order):
        from butterfly_amd import cheb_fit, matern_density
        if order not in self._coef:
            self._coef[order] = cheb_fit(matern_density(2.0, 2.0), order, 0.0, self.lam_max)
        return self._coef[order]

    def poly(self, order, V, dt):
        """p(S) V in the float type dt."""
        return cc.forward_recurrence(self.ell[dt], self.lam_max, self.coef(order), np.asarray(V, dtype=dt))

    def rows_t(self, order, idx, dt):
        """X = p(S) D E_idx [n x len(idx)]: the rows of B = D p(S) at idx, transposed."""
        have = self._cols.setdefault((order, dt), {})
        new = np.array([v for v in idx if int(v) not in have], dtype=np.int64)
        if len(new):
            U = np.zeros((self.n, len(new)), dtype=dt)
            U[new, np.arange(len(new))] = self.d[new].astype(dt)
            for v, col in zip(new, self.poly(order, U, dt).T):
                have[int(v)] = col
        return np.stack([have[int(v)] for v in idx], axis=1)

    def field(self, order, Wp, dt):
        """Z = D p(S) W'."""
        return self.d.astype(dt)[:, None] * self.poly(order, Wp, dt)

    def observed(self, k):
        """k of the pool's vertices in an order of their own; on mesh4099 the three ears are among them from k = 3 on."""
        if self.name == "mesh4099" and k < 3:
            return np.array(EARS[1:1 + k])
        return np.random.default_rng(5000 + k).permutation(self.pool[:k])

    def queries(self, obs):
        """70 vertices (all of a smaller mesh), the first 8 of them observed."""
        if self.other_queries is not None:
            return np.concatenate([obs[:8], self.other_queries])[:NQUERY]
        rest = np.setdiff1d(np.arange(self.n), obs[:8])
        return np.concatenate([obs[:8], np.random.default_rng(6000 + len(obs)).permutation(rest)])[:NQUERY]

    def case(self, k, order, noise=True):
        key = (k, order, noise)
        if key not in self._cases:
            self._cases[key] = Case(self, k, order, noise)
        return self._cases[key]


class Case(Reference):
    """Everything of one (matrix, k, order) in long double (the Reference of tests/test_gpu_cov_condition.py with Bt = X and
    gamma = 1), and the same sequence in float64 (self.f64)."""
    def __init__(self, mat, k, order, noise=True):
        self.mat, self.order = mat, order
        n = mat.n
        rng = np.random.default_rng([n, k, order])
        obs = mat.observed(k)
        Reference.__init__(self, mat.rows_t(order, obs, LD), np.ones(n), obs, RHO, rng, phi=None)
        if not noise:
            self.noise = np.zeros(k)
            self.A = self.G.copy()
            ev = np.linalg.eigvalsh(self.A.astype(np.float64))
            self.kappa = float(ev[-1] / ev[0])
        self.lik = LikReference(self.Bt, self.noise, np.zeros(k))         # the one long-double factorization of the case
        self.L = self.lik.L
        self.y = np.asarray(self.Bt.T @ rng.standard_normal(n) + np.sqrt(self.noise) * rng.standard_normal(k), dtype=np.float64)
        self.E = np.sqrt(self.noise)[:, None] * rng.standard_normal((k, MAXQ))
        self.W = mat.W
        self.query = mat.queries(obs)
        self.bound = fwd_bound(n, k, self.kappa)
        self._out = None

    # ---- the long-double results and the float64 sequence's, computed once ----
    def _sequence(self, dt):
        mat, k, zc = self.mat, self.k, self.mat.zcols
        ld = dt is LD
        X = self.Bt if ld else mat.rows_t(self.order, self.obs, dt)
        A = self.A if ld else X.T @ X + np.diag(self.noise)
        L = self.L if ld else np.linalg.cholesky(A)
        solve = solve_ld if ld else solve_f64
        fwd = forward_ld if ld else (lambda l, r: np.linalg.solve(l, r))
        y = self.y.astype(dt)
        R = y[:, None] - X.T @ self.W.astype(dt) - self.E.astype(dt)
        alpha = solve(L, R)
        a_y = solve(L, y)
        out = dict(alpha=alpha, alpha_y=a_y)
        out["Z"] = mat.field(self.order, self.W[:, zc].astype(dt) + X @ alpha[:, zc], dt)
        out["mean"] = mat.field(self.order, (X @ a_y)[:, None], dt)[:, 0]
        quad, logdet = y @ a_y, 2 * np.log(np.diag(L)).sum()
        out["value"] = np.array([-quad / 2 - logdet / 2 - dt(k) / 2 * np.log(2 * (PI_LD if ld else np.pi)), quad, logdet], dtype=dt)
        out["grad_noise"] = (a_y ** 2 - (fwd(L, np.eye(k, dtype=dt)) ** 2).sum(axis=0)) / 2
        Xq = mat.rows_t(self.order, self.query, dt)
        out["prior"] = (Xq ** 2).sum(axis=0)
        out["post"] = out["prior"] - (fwd(L, X.T @ Xq) ** 2).sum(axis=0)
        return out

    def results(self):
        """(long double, float64): dicts of alpha [k x 70], alpha_y [k], Z [n x len(zcols)], mean [n], value [3], grad_noise [k],
        prior and post [numQuery]."""
        if self._out is None:
            self._out = self._sequence(LD), self._sequence(np.float64)
        return self._out

    def allowed(self, name):
        """The bound on the device's relative l2 error of `name`, per column (value: per entry): 8 times the float64 sequence's own,
        floored at fwd_bound(n, k, cond)."""
        ref, f64 = self.results()
        return np.maximum(8 * rel_errs(name, f64[name], ref[name]), self.bound)


def rel_errs(name, got, want):
    """Per-column relative l2 errors (vectors are one column); the three likelihood values are held entry by entry."""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    if name == "value":
        return (np.abs(got - want) / np.abs(want)).astype(np.float64)
    if got.ndim == 1:
        got, want = got[:, None], want[:, None]
    return col_errs(got, want)


def matrices(names=("mesh4099", "mesh63", "n1")):
    cat = cc.catalogue()
    return {name: Matrix(name, cat[name]) for name in names}


def every_chunk_matters(case, q=MAXQ):
    """The condition a kernel that drops or misplaces a chunk of n cannot pass, on the reference alone: {(chunk, "G" | "BtW"):
    the smallest relative change, over the columns, of alpha when that chunk's rows of X are left out of G, or out of X^T W}."""
    return chunk_sensitivity(case, case.W[:, :q], case.E[:, :q])


def num_chunks(n):
    return (n + CHUNK - 1) // CHUNK
