"""Cases of the likelihood's gradient in the density's parameters on the Chebyshev route (bfhipChebCovCondLogLikGradDevice;
DESIGN.md section 26).  Builders only: numpy and the host entries of the library (the fold of the mesh, the Chebyshev fit), no
GPU.  tests/test_cheb_gradient_cpu.py asserts what the cases claim on the reference alone; tests/test_gpu_cheb_gradient.py
holds the device to them.

Reference.  The cases are those of tests/chebcond_cases.py: mesh4099 (five chunks of 1024 rows, the last of 3), mesh63, n1;
k in {1, 33, 130} as cases_of allows; p of orders {1, 2, 64} of matern_density(2, 2).  For a parameter theta_t with derivative
polynomial q_t, X'_t = q_t(S) D E_obs by the forward recurrence on Ell(S), as Matrix.rows_t forms X; then in numpy.longdouble

    M = alpha alpha^T - K^-1,   grad_t = < X M, X'_t >_F,   t1 = (X alpha) . (X'_t alpha),   t2 = < X K^-1, X'_t >_F

(grad = t1 - t2), and the same sequence in plain float64 (its own X, Cholesky factor and solves).

Parameters.  ("kappa", o), ("nu", o): the Chebyshev fit of matern_density_grad(2, 2) at o points; ("scale", o): half the fit of
the density itself at o points -- at p's order that is p / 2, theta = the log of an amplitude on the covariance, whose gradient
has the closed form (quad - k) / 2 - sum_a noiseVar[a] gradNoise[a].  Parameter sets: "kappa" (kappa at p's order), "all"
(kappa, nu, scale at p's order), "mixed" (kappa at 64, nu at 1, scale at 2: orders other than p's).

Error measure.  |got - ref| / (|t1| + |t2|): a case near a stationary point needs no special handling.  The device is held to
max(8 x the float64 sequence's, fwd_bound(n, k, cond)), the project's yardstick and floor."""
import numpy as np

import cheb_cases as cc
import chebcond_cases as cq
from cond_cases import CHUNK, solve_f64
from test_gpu_cov_condition import LD, solve_ld

KAPPA, NU = 2.0, 2.0
PARAM_SETS = ("kappa", "all", "mixed")
MATRICES = ("mesh4099", "mesh63", "n1")
PANEL = 64


def param_set(pset, order):
    """[(name, order of the derivative polynomial)] of a parameter set for p of order `order`."""
    return {"kappa": [("kappa", order)], "all": [("kappa", order), ("nu", order), ("scale", order)],
            "mixed": [("kappa", 64), ("nu", 1), ("scale", 2)]}[pset]


def density_coef(lam_max, name, order, kappa=KAPPA, nu=NU):
    """The Chebyshev coefficients on [0, lam_max] of the derivative polynomial `name` at `order` points."""
    from butterfly_amd import cheb_fit, matern_density, matern_density_grad
    if name == "scale":
        return cheb_fit(matern_density(kappa, nu), order, 0.0, lam_max) / 2
    d_kappa, d_nu = matern_density_grad(kappa, nu)
    return cheb_fit(d_kappa if name == "kappa" else d_nu, order, 0.0, lam_max)


def coef_block(mat, params):
    """(coef [numParams x ld], orders) as the C entry takes them."""
    ld = max(o for _, o in params)
    coef = np.zeros((len(params), ld))
    for t, (name, o) in enumerate(params):
        coef[t, :o] = density_coef(mat.lam_max, name, o)
    return coef, [o for _, o in params]


def columns(mat, key, coef, idx, dt):
    """r(S) D E_idx [n x len(idx)] for the polynomial r of coefficients `coef`, cached per vertex under `key` like Matrix.rows_t."""
    have = mat._cols.setdefault(("grad", key, dt), {})
    new = np.array([v for v in idx if int(v) not in have], dtype=np.int64)
    if len(new):
        U = np.zeros((mat.n, len(new)), dtype=dt)
        U[new, np.arange(len(new))] = mat.d[new].astype(dt)
        for v, col in zip(new, cc.forward_recurrence(mat.ell[dt], mat.lam_max, coef, U).T):
            have[int(v)] = col
    return np.stack([have[int(v)] for v in idx], axis=1)


class GradCase:
    """The gradient's reference for one Case of tests/chebcond_cases.py: per derivative polynomial (name, order) the long-double
    (grad, t1, t2) and the float64 sequence's."""
    def __init__(self, case):
        self.case, self.mat, self.k, self.n = case, case.mat, case.k, case.mat.n
        self._base, self._out = {}, {}

    def xprime(self, name, order, dt):
        if name == "scale" and order == self.case.order:
            return self.x(dt) / dt(2)             # the recurrence is linear in the coefficients and halving is exact: p / 2 gives X / 2
        return columns(self.mat, (name, order), density_coef(self.mat.lam_max, name, order), self.case.obs, dt)

    def x(self, dt):
        return self.case.Bt if dt is LD else self.mat.rows_t(self.case.order, self.case.obs, dt)

    def base(self, dt):
        """(X, alpha, K^-1, X M) in dt."""
        if dt not in self._base:
            case, k = self.case, self.k
            X = self.x(dt)
            if dt is LD:
                L, solve = case.L, solve_ld
            else:
                L, solve = np.linalg.cholesky(X.T @ X + np.diag(case.noise)), solve_f64
            alpha = solve(L, case.y.astype(dt))
            Kinv = solve(L, np.eye(k, dtype=dt))
            M = np.outer(alpha, alpha) - Kinv
            self._base[dt] = (X, alpha, Kinv, M)
        return self._base[dt]

    def terms(self, name, order, dt):
        """(grad, t1, t2) in dt."""
        key = (name, order, dt)
        if key not in self._out:
            X, alpha, Kinv, M = self.base(dt)
            Xp = self.xprime(name, order, dt)
            grad = ((X @ M) * Xp).sum()
            t1 = (X @ alpha) @ (Xp @ alpha)
            t2 = ((X @ Kinv) * Xp).sum()
            self._out[key] = (grad, t1, t2)
        return self._out[key]

    def scale(self, name, order):
        """|t1| + |t2| of the long-double reference: what an error is measured against."""
        _, t1, t2 = self.terms(name, order, LD)
        return float(abs(t1) + abs(t2))

    def error(self, name, order, got):
        ref = self.terms(name, order, LD)[0]
        return float(abs(LD(got) - ref)) / self.scale(name, order)

    def f64_error(self, name, order):
        return self.error(name, order, self.terms(name, order, np.float64)[0])

    def allowed(self, name, order):
        return max(8 * self.f64_error(name, order), self.case.bound)

    def closed_form_scale(self, dt):
        """(quad - k) / 2 - sum_a noiseVar[a] gradNoise[a] from the results of the Case in dt."""
        res = self.case.results()[0 if dt is LD else 1]
        return (res["value"][1] - dt(self.k)) / 2 - (self.case.noise.astype(dt) * res["grad_noise"]).sum()

    # ---- what a kernel could leave out, on the long-double reference alone ----
    def omissions(self, name, order):
        """{what: |change of grad| / (|t1| + |t2|)} when one chunk of rows is left out of the dot, one live 16-column tile of Y, or
        (k mod 4 != 0) the last k-step of the contraction: the indices from 4 floor(k / 4) on."""
        X, _, _, M = self.base(LD)
        Xp = self.xprime(name, order, LD)
        Y = X @ M
        prod = Y * Xp
        s, out = self.scale(name, order), {}
        for c, r0 in enumerate(range(0, self.n, CHUNK)):
            out["chunk", c] = float(abs(prod[r0:r0 + CHUNK].sum())) / s
        for c0 in range(0, self.k, 16):
            out["tile", c0 // PANEL, (c0 % PANEL) // 16] = float(abs(prod[:, c0:c0 + 16].sum())) / s
        k4 = self.k // 4 * 4
        if k4 < self.k:
            out["kstep", k4] = float(abs(((X[:, k4:] @ M[k4:]) * Xp).sum())) / s
        return out


def likelihood_ld(mat, case, coef):
    """The long-double log marginal likelihood of the case's y, observed set and noise under the polynomial of coefficients `coef`."""
    from test_cov_likelihood_cpu import LikReference
    U = np.zeros((mat.n, case.k), dtype=LD)
    U[case.obs, np.arange(case.k)] = mat.d[case.obs].astype(LD)
    X = cc.forward_recurrence(mat.ell[LD], mat.lam_max, coef, U)
    return LikReference(X, case.noise, case.y).loglik


def matrices(names=MATRICES):
    return cq.matrices(names)


def cases(names=MATRICES):
    return [(name, k, order) for name in names for k, order in cq.cases_of(name)]
