/* bfhip_eigs.c -- the lowest eigenpairs of S = D L D of a BfhipChebCov by Chebyshev-filtered subspace iteration
 * (bfhipChebCovEigsDevice, include/bfhip.h; Zhou and Saad, "A Chebyshev-Davidson algorithm for large
 * symmetric eigenproblems", SIAM J. Matrix Anal. Appl. 29, 2007, and Zhou, Saad, Tiago, Chelikowsky, J. Comput. Phys. 219,
 * 2006, for the scaled filter).  Host side: the argument checks, the outer loop, the scalar recurrence that caps the
 * filter's degree, and the p x p dense work (Cholesky factor, triangular inverse, symmetric eigenproblem; p <= 256) in
 * double -- the loop needs the Ritz values and the residuals on the host in every iteration anyway.  The kernels are
 * bfhip_eigs.hip's.  bfEigsSolve is also the iteration of bfhipChebCovEigsBandDevice (bfhip_eigs_band.c):
 * with locked vectors the block is projected against them before every orthonormalisation and their lowest eigenvalue joins
 * the degree cap; with none it is section 25's call, launch for launch.  With BFHIP_EIGS_CONSISTENT_MASS the
 * same loop solves S u = theta B u: B^-1 S in the filter by a fixed number of Chebyshev semi-iterations, the B inner product in
 * Rayleigh-Ritz; the launches of bfhip_eigs_mass.hip are reached through the object's table (bfhip_eigs_mass.c), none is named here. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip_internal.h"
#include "../../include/bfhip.h"
#include "../../include/bfhip_abi.h"

/* ------------------------------------------------------------------------
 * small dense algebra (host)
 * ---------------------------------------------------------------------- */
/* Symmetric eigenproblem A = Q Theta Q^T: Householder tridiagonalisation and the implicit QL iteration with the
 * transformations accumulated (the EISPACK pair tred2 / tql2, Wilkinson and Reinsch, Handbook for Automatic Computation II,
 * 1971, contributions II/2 and II/4).  A [p x p, row-major, lda] is read in full (it is taken to be symmetric) and replaced
 * by Q, whose COLUMNS are the eigenvectors; theta ascending.  work: 2 p doubles. */
int bfEigsSymEig(size_t p, double *A, size_t lda, double *theta, double *work) {
  if (!p) return 0;
  size_t const n = p;
  double *d = theta, *e = work;
#define V(i, j) A[(i) * lda + (j)]
  for (size_t j = 0; j < n; ++j) d[j] = V(n - 1, j);
  for (size_t i = n - 1; i > 0; --i) {
    double scale = 0, h = 0;
    for (size_t k = 0; k < i; ++k) scale += fabs(d[k]);
    if (scale == 0) {
      e[i] = d[i - 1];
      for (size_t j = 0; j < i; ++j) { d[j] = V(i - 1, j); V(i, j) = 0; V(j, i) = 0; }
    } else {
      for (size_t k = 0; k < i; ++k) { d[k] /= scale; h += d[k] * d[k]; }
      double f = d[i - 1], g = sqrt(h);
      if (f > 0) g = -g;
      e[i] = scale * g; h -= f * g; d[i - 1] = f - g;
      for (size_t j = 0; j < i; ++j) e[j] = 0;
      for (size_t j = 0; j < i; ++j) {
        f = d[j]; V(j, i) = f; g = e[j] + V(j, j) * f;
        for (size_t k = j + 1; k < i; ++k) { g += V(k, j) * d[k]; e[k] += V(k, j) * f; }
        e[j] = g;
      }
      f = 0;
      for (size_t j = 0; j < i; ++j) { e[j] /= h; f += e[j] * d[j]; }
      double const hh = f / (h + h);
      for (size_t j = 0; j < i; ++j) e[j] -= hh * d[j];
      for (size_t j = 0; j < i; ++j) {
        f = d[j]; g = e[j];
        for (size_t k = j; k < i; ++k) V(k, j) -= f * e[k] + g * d[k];
        d[j] = V(i - 1, j); V(i, j) = 0;
      }
    }
    d[i] = h;
  }
  for (size_t i = 0; i + 1 < n; ++i) {
    V(n - 1, i) = V(i, i); V(i, i) = 1;
    double const h = d[i + 1];
    if (h != 0) {
      for (size_t k = 0; k <= i; ++k) d[k] = V(k, i + 1) / h;
      for (size_t j = 0; j <= i; ++j) {
        double g = 0;
        for (size_t k = 0; k <= i; ++k) g += V(k, i + 1) * V(k, j);
        for (size_t k = 0; k <= i; ++k) V(k, j) -= g * d[k];
      }
    }
    for (size_t k = 0; k <= i; ++k) V(k, i + 1) = 0;
  }
  for (size_t j = 0; j < n; ++j) { d[j] = V(n - 1, j); V(n - 1, j) = 0; }
  V(n - 1, n - 1) = 1; e[0] = 0;

  /* implicit QL */
  for (size_t i = 1; i < n; ++i) e[i - 1] = e[i];
  e[n - 1] = 0;
  double f = 0, tst1 = 0;
  double const eps = 0x1p-52;
  for (size_t l = 0; l < n; ++l) {
    double const t = fabs(d[l]) + fabs(e[l]);
    if (t > tst1) tst1 = t;
    size_t m = l;
    while (m + 1 < n && fabs(e[m]) > eps * tst1) ++m;
    if (m > l) {
      int iter = 0;
      do {
        if (++iter > 64) return 1;
        double g = d[l], pp = (d[l + 1] - g) / (2 * e[l]), r = hypot(pp, 1.0);
        if (pp < 0) r = -r;
        d[l] = e[l] / (pp + r); d[l + 1] = e[l] * (pp + r);
        double const dl1 = d[l + 1];
        double h = g - d[l];
        for (size_t i = l + 2; i < n; ++i) d[i] -= h;
        f += h;
        pp = d[m];
        double c = 1, c2 = 1, c3 = 1, s = 0, s2 = 0;
        double const el1 = e[l + 1];
        for (size_t i = m; i-- > l;) {
          c3 = c2; c2 = c; s2 = s;
          g = c * e[i]; h = c * pp; r = hypot(pp, e[i]);
          e[i + 1] = s * r; s = e[i] / r; c = pp / r; pp = c * d[i] - s * g;
          d[i + 1] = h + s * (c * g + s * d[i]);
          for (size_t k = 0; k < n; ++k) {
            h = V(k, i + 1);
            V(k, i + 1) = s * V(k, i) + c * h;
            V(k, i) = c * V(k, i) - s * h;
          }
        }
        pp = -s * s2 * c3 * el1 * e[l] / dl1;
        e[l] = s * pp; d[l] = c * pp;
      } while (fabs(e[l]) > eps * tst1);
    }
    d[l] += f; e[l] = 0;
  }
  /* ascending, by selection (stable enough: ties keep whatever order QL left) */
  for (size_t i = 0; i + 1 < n; ++i) {
    size_t k = i;
    for (size_t j = i + 1; j < n; ++j)
      if (d[j] < d[k]) k = j;
    if (k != i) {
      double t = d[k]; d[k] = d[i]; d[i] = t;
      for (size_t r = 0; r < n; ++r) { t = V(r, i); V(r, i) = V(r, k); V(r, k) = t; }
    }
  }
#undef V
  return 0;
}

/* G [p x p in ld] = L L^T in its lower triangle; 1 when a pivot is not a positive finite number */
static int eigsCholesky(size_t p, double *G, size_t ld) {
  for (size_t j = 0; j < p; ++j) {
    double s = G[j * ld + j];
    for (size_t k = 0; k < j; ++k) s -= G[j * ld + k] * G[j * ld + k];
    if (!(s > 0) || !isfinite(s)) return 1;
    double const l = sqrt(s);
    G[j * ld + j] = l;
    for (size_t i = j + 1; i < p; ++i) {
      double t = G[i * ld + j];
      for (size_t k = 0; k < j; ++k) t -= G[i * ld + k] * G[j * ld + k];
      G[i * ld + j] = t / l;
    }
  }
  return 0;
}

/* W [ld x ld, zero padded] = L^-T (upper triangular), L the lower triangle of G: X W = X R^-1 with R = L^T */
static void eigsInverseTransposed(size_t p, double const *G, size_t ld, double *W) {
  memset(W, 0, ld * ld * sizeof *W);
  /* column j of L^-1 by forward substitution, stored as row j of W */
  for (size_t j = 0; j < p; ++j) {
    W[j * ld + j] = 1 / G[j * ld + j];
    for (size_t i = j + 1; i < p; ++i) {
      double t = 0;
      for (size_t k = j; k < i; ++k) t -= G[i * ld + k] * W[j * ld + k];
      W[j * ld + i] = t / G[i * ld + i];
    }
  }
  /* so far W[j][i] = Linv[i][j], i >= j: that IS L^-T */
}

/* ------------------------------------------------------------------------
 * profile switch of tools/lbo_eigs_rate.py
 * ---------------------------------------------------------------------- */
static _Thread_local int eigsProfileOn;
static _Thread_local double eigsPhases[7];
enum { PH_FILTER, PH_SX, PH_GRAM, PH_ROTATE, PH_RESIDUAL, PH_HOST, PH_PROJECT };
void bfEigsProfile(int on) { eigsProfileOn = on; }
void bfEigsLastPhases(double out[6]) { memcpy(out, eigsPhases, 6 * sizeof(double)); }
double bfEigsLastProjectSeconds(void) { return eigsPhases[PH_PROJECT]; }
/* with the switch on, per Rayleigh-Ritz step of the last call (the first BF_EIGS_HISTORY of them): the largest residual of the
 * wanted pairs over lamMax, and the degree of the filter before it (0 for the start block) */
enum { BF_EIGS_HISTORY = 128 };
static _Thread_local uint32_t eigsHistoryCount, eigsHistoryDegree[BF_EIGS_HISTORY];
static _Thread_local double eigsHistoryResidual[BF_EIGS_HISTORY];
uint32_t bfEigsLastHistory(double *residual, uint32_t *degree, uint32_t cap) {
  uint32_t const k = eigsHistoryCount < cap ? eigsHistoryCount : cap;
  memcpy(residual, eigsHistoryResidual, k * sizeof *residual);
  memcpy(degree, eigsHistoryDegree, k * sizeof *degree);
  return k;
}
static void eigsRecord(double const *res, size_t nev, double lamMax, uint32_t degree) {
  if (!eigsProfileOn || eigsHistoryCount >= BF_EIGS_HISTORY) return;
  double worst = 0;
  for (size_t j = 0; j < nev; ++j)
    if (res[j] > worst) worst = res[j];
  eigsHistoryResidual[eigsHistoryCount] = worst / lamMax;
  eigsHistoryDegree[eigsHistoryCount++] = degree;
}

/* ------------------------------------------------------------------------
 * the iteration
 * ---------------------------------------------------------------------- */
typedef struct EigsRun {
  BfhipChebCov *c;
  uint64_t n;
  uint32_t p, ld, nev;
  double *B[3];                 /* the three blocks, device */
  uint32_t ix, iy, iz;          /* X, Y = S X, free */
  double *dPart, *dG, *dW, *dTheta, *dSumSq;
  double *G, *W, *theta, *res, *work;       /* host: ld x ld, ld x ld, ld, ld, 2 ld */
  uint64_t opColumns;
  void *stream;
  double t0;
  /* the locked block (section 27): m == 0 and project == NULL in bfhipChebCovEigsDevice */
  double const *dQ;
  uint64_t ldq, m;
  double lockMin;               /* the smallest locked eigenvalue */
  double *dC, *dPartC;          /* coefficients of one panel [<= 256 x ld] and their per-chunk partials */
  BfEigsProjectFn project;
  /* the consistent-mass pencil (section 28): ops == NULL in the lumped call, which then runs section 25's launches and no other */
  BfEigsMassOps const *ops;
  double *T, *Z2;               /* T = S Y_i of a filter step and B X of Rayleigh-Ritz; the mass solve's second block */
  uint32_t massSteps;
} EigsRun;

static void phaseBegin(EigsRun *r) {
  if (eigsProfileOn) { bfdevSync(r->stream); r->t0 = bfNowSeconds(); }
}
static void phaseEnd(EigsRun *r, int ph) {
  if (eigsProfileOn) { bfdevSync(r->stream); eigsPhases[ph] += bfNowSeconds() - r->t0; }
}

static int eigsStep(EigsRun *r, double const *b1, double const *b2, double *out, double alpha, double beta, double gamma) {
  BfhipChebCov const *c = r->c;
  BfEigsStep s = { c->dRowptr, c->dColind, c->dVal, r->n, r->p, r->ld, b1, b2, out, alpha, beta, gamma };
  r->opColumns += r->p;
  return bfdevEigsStep(&s, r->stream);
}

/* out = B X: one mass step without its other terms */
static int eigsMassMul(EigsRun *r, double const *X, double *out) {
  BfhipChebCov const *c = r->c;
  BfEigsMassStep s = { c->dRowptr, c->dColind, c->dMass, r->n, r->p, r->ld, X, NULL, NULL, out, 1.0, 0.0, 0.0, 0.0 };
  r->opColumns += r->p;
  return r->ops->step(&s, r->stream);
}

/* Z ~ B^-1 T into the free block; every step but the first applies B */
static int eigsMassSolve(EigsRun *r) {
  BfhipChebCov const *c = r->c;
  BfEigsMassSolve s = { c->dRowptr, c->dColind, c->dMass, r->n, r->p, r->ld, r->T, r->B[r->iz], r->Z2, c->massLo, c->massHi, r->massSteps, 0 };
  r->opColumns += (uint64_t)r->p * (r->massSteps - 1);
  return r->ops->solve(&s, r->stream);
}

static int eigsRotateX(EigsRun *r, double const *W) {
  int rc;
  phaseBegin(r);
  if ((rc = bfdevMemcpyH2DAsync(r->dW, W, (size_t)r->ld * r->ld * 8, r->stream)) ||
      (rc = bfdevEigsRotate(r->B[r->ix], r->dW, r->B[r->iz], r->n, r->ld, r->stream)) || (rc = bfdevSync(r->stream))) return rc;
  phaseEnd(r, PH_ROTATE);
  uint32_t const t = r->ix; r->ix = r->iz; r->iz = t;
  return 0;
}

static int eigsGramToHost(EigsRun *r, double const *X, double const *Y) {
  int rc;
  phaseBegin(r);
  if ((rc = bfdevEigsGram(X, Y, r->n, r->ld, r->dPart, r->dG, r->stream)) ||
      (rc = bfdevMemcpyD2HAsync(r->G, r->dG, (size_t)r->ld * r->ld * 8, r->stream)) || (rc = bfdevSync(r->stream))) return rc;
  phaseEnd(r, PH_GRAM);
  return 0;
}

/* With locked vectors Q first X <- X - Q (Q^T X), twice ("twice is enough"), the coefficients staying on the device.  Then
 * X <- X R^-1 twice (Cholesky QR applied twice); a failed pivot: that pass once more with G + s I, then two plain passes */
static int eigsOrthonormalise(EigsRun *r) {
  int rc, plain = 2, shifted = 0;
  size_t const p = r->p, ld = r->ld;
  if (r->m) {
    phaseBegin(r);
    for (int pass = 0; pass < 2; ++pass)
      if (r->ops) {
        if ((rc = eigsMassMul(r, r->B[r->ix], r->T)) ||
            (rc = r->ops->project(r->dQ, r->ldq, r->m, r->T, r->B[r->ix], r->n, r->ld, r->dPartC, r->dC, r->stream))) return rc;
      } else if ((rc = r->project(r->dQ, r->ldq, r->m, r->B[r->ix], r->n, r->ld, r->dPartC, r->dC, r->stream))) return rc;
    phaseEnd(r, PH_PROJECT);
  }
  while (plain > 0) {
    /* the Gram matrix of the inner product in force: X^T X, or X^T (B X) */
    if (r->ops) {
      phaseBegin(r);
      if ((rc = eigsMassMul(r, r->B[r->ix], r->T))) return rc;
      phaseEnd(r, PH_SX);
    }
    if ((rc = eigsGramToHost(r, r->B[r->ix], r->ops ? r->T : r->B[r->ix]))) return rc;
    double const th = bfNowSeconds();
    memcpy(r->W, r->G, ld * ld * sizeof(double));          /* the Gram matrix survives a failed factorisation in W */
    int bad = eigsCholesky(p, r->G, ld);
    if (bad) {
      if (shifted) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "eigensolver: the Gram matrix of the block is not positive definite, with the shift too");
      shifted = 1;
      double fro = 0;
      for (size_t i = 0; i < p; ++i)
        for (size_t j = 0; j < p; ++j) fro += r->W[i * ld + j] * r->W[i * ld + j];
      fro = sqrt(fro);
      if (!isfinite(fro)) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "eigensolver: the Gram matrix of the block is not finite");
      double const s = 11.0 * ((double)r->n * (double)p + (double)p * (double)(p + 1)) * 0x1p-53 * fro;
      memcpy(r->G, r->W, ld * ld * sizeof(double));
      for (size_t i = 0; i < p; ++i) r->G[i * ld + i] += s;
      if (eigsCholesky(p, r->G, ld)) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "eigensolver: the shifted Gram matrix of the block is not positive definite");
      plain = 2;
    } else {
      --plain;
    }
    eigsInverseTransposed(p, r->G, ld, r->W);
    if (eigsProfileOn) eigsPhases[PH_HOST] += bfNowSeconds() - th;
    if ((rc = eigsRotateX(r, r->W))) return rc;
  }
  return 0;
}

/* orthonormalise X, Y = S X, H = X^T Y = Q Theta Q^T, X <- X Q, Y <- Y Q, res_j = ||Y_j - theta_j X_j|| */
static int eigsRayleighRitz(EigsRun *r) {
  int rc;
  size_t const p = r->p, ld = r->ld;
  if ((rc = eigsOrthonormalise(r))) return rc;
  phaseBegin(r);
  if (r->ops) {
    /* Y = S X and T = B X from one gather of X's rows; T is rotated with X and Y below */
    BfhipChebCov const *c = r->c;
    r->opColumns += 2 * (uint64_t)r->p;
    if ((rc = r->ops->dual(c->dRowptr, c->dColind, c->dVal, c->dMass, r->n, r->p, r->ld, r->B[r->ix], r->B[r->iy], r->T, r->stream))) return rc;
  } else if ((rc = eigsStep(r, r->B[r->ix], NULL, r->B[r->iy], 1.0, 0.0, 0.0))) return rc;
  phaseEnd(r, PH_SX);
  if ((rc = eigsGramToHost(r, r->B[r->ix], r->B[r->iy]))) return rc;
  double const th = bfNowSeconds();
  for (size_t i = 0; i < p; ++i)
    for (size_t j = 0; j <= i; ++j) {
      double const h = 0.5 * (r->G[i * ld + j] + r->G[j * ld + i]);
      if (!isfinite(h)) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "eigensolver: the projected matrix is not finite");
      r->G[i * ld + j] = r->G[j * ld + i] = h;
    }
  memset(r->theta, 0, ld * sizeof(double));
  if (bfEigsSymEig(p, r->G, ld, r->theta, r->work)) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "eigensolver: the QL iteration of the projected problem did not converge");
  memset(r->W, 0, ld * ld * sizeof(double));
  for (size_t i = 0; i < p; ++i) memcpy(r->W + i * ld, r->G + i * ld, p * sizeof(double));
  if (eigsProfileOn) eigsPhases[PH_HOST] += bfNowSeconds() - th;
  /* X -> free block, then Y -> the old X block */
  uint32_t const oldX = r->ix, oldY = r->iy;
  if ((rc = eigsRotateX(r, r->W))) return rc;             /* ix = old free, iz = oldX */
  phaseBegin(r);
  if ((rc = bfdevEigsRotate(r->B[oldY], r->dW, r->B[oldX], r->n, r->ld, r->stream))) return rc;
  if (r->ops) {
    /* B X likewise, into the mass solve's second block, which is free between filters */
    if ((rc = bfdevEigsRotate(r->T, r->dW, r->Z2, r->n, r->ld, r->stream))) return rc;
    double *t = r->T; r->T = r->Z2; r->Z2 = t;
  }
  phaseEnd(r, PH_ROTATE);
  r->iy = oldX; r->iz = oldY;
  phaseBegin(r);
  /* with a mass the residual is Y - (B X) diag(theta): the kernel takes B X in the place of X */
  if ((rc = bfdevMemcpyH2DAsync(r->dTheta, r->theta, ld * 8, r->stream)) ||
      (rc = bfdevEigsResidual(r->ops ? r->T : r->B[r->ix], r->B[r->iy], r->dTheta, r->n, r->ld, r->dPart, r->dSumSq, r->stream)) ||
      (rc = bfdevMemcpyD2HAsync(r->res, r->dSumSq, ld * 8, r->stream)) || (rc = bfdevSync(r->stream))) return rc;
  phaseEnd(r, PH_RESIDUAL);
  for (size_t j = 0; j < p; ++j) {
    if (!isfinite(r->res[j])) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "eigensolver: residual %zu is not finite", j);
    r->res[j] = sqrt(r->res[j]);
  }
  return 0;
}

/* The scaled Chebyshev filter of degree m on [a, b] = [largest Ritz value, lamMax], normalised at a0 = the smallest:
 * e = (b - a) / 2, c = (b + a) / 2, sigma_1 = e / (a0 - c), tau = 2 / sigma_1,
 *   Y_1 = (sigma_1 / e) (S - c) X,   Y_{i+1} = (2 sigma_{i+1} / e) (S - c) Y_i - sigma_i sigma_{i+1} Y_{i-1},  sigma_{i+1} = 1 / (tau - sigma_i).
 * The degree is the largest m <= degree for which max_j |rho_m(theta_j)| / min_j |rho_m(theta_j)| < 2^23 over the block's Ritz
 * values, rho_m by the same recurrence in scalars: the filtered block's condition number then stays where Cholesky QR applied
 * twice still gives an orthonormal block (cond^2 2^-53 < 1 needs cond < 2^26; the factor 8 is margin).  With locked pairs
 * their smallest eigenvalue is one more point: the filter amplifies the locked directions most, and what rounding leaves of
 * them in the block (2^-53) must stay below 2^23 2^-53 of the least amplified Ritz direction before it is projected out. */
static uint32_t eigsDegreeCap(EigsRun const *r, uint32_t degree, double e, double cc, double sigma1) {
  size_t const p = r->p, q = r->m ? p + 1 : p;
  double *y0 = r->work, *y1 = r->work + q;            /* 2 (p + 1) doubles */
  if (r->m) r->theta[p] = r->lockMin;                 /* theta has ld + 1 entries; the slot is past every Ritz value */
  double const tau = 2 / sigma1;
  double sigma = sigma1;
  uint32_t best = 1;
  for (size_t j = 0; j < q; ++j) { y0[j] = 1; y1[j] = sigma1 / e * (r->theta[j] - cc); }
  for (uint32_t m = 1; m <= degree; ++m) {
    if (m > 1) {
      double const sn = 1 / (tau - sigma);
      for (size_t j = 0; j < q; ++j) {
        double const y = 2 * sn / e * (r->theta[j] - cc) * y1[j] - sigma * sn * y0[j];
        y0[j] = y1[j]; y1[j] = y;
      }
      sigma = sn;
    }
    double lo = INFINITY, hi = 0;
    for (size_t j = 0; j < q; ++j) {
      double const v = fabs(y1[j]);
      if (v < lo) lo = v;
      if (v > hi) hi = v;
    }
    if (isfinite(hi) && hi < 0x1p23 * lo) best = m;
  }
  return best;
}

static int eigsFilter(EigsRun *r, uint32_t degree, double lamMax, uint32_t *used) {
  size_t const p = r->p;
  double const a = r->theta[p - 1], a0 = r->theta[0], b = lamMax;
  if (!(a < b)) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "eigensolver: a Ritz value (%g) is not below lamMax (%g): lamMax is no upper bound of the spectrum", a, b);
  double const e = (b - a) / 2, cc = (b + a) / 2, sigma1 = e / (a0 - cc), tau = 2 / sigma1;
  uint32_t const m = eigsDegreeCap(r, degree, e, cc, sigma1);
  int rc;
  phaseBegin(r);
  /* Y_1 into the Y block; from there on the result is written over Y_{i-1} */
  double *prev = r->B[r->ix], *cur = r->B[r->iy];
  double sigma = sigma1;
  if (r->ops) {
    /* the same recurrence with A = B^-1 S: T = S Y_i, Z ~ B^-1 T in the free block, then the combination */
    if ((rc = eigsStep(r, prev, NULL, r->T, 1.0, 0.0, 0.0)) || (rc = eigsMassSolve(r)) ||
        (rc = r->ops->combine(r->B[r->iz], prev, NULL, cur, r->n, r->p, r->ld, sigma1 / e, -sigma1 * cc / e, 0.0, r->stream))) return rc;
    for (uint32_t i = 1; i < m; ++i) {
      double const sn = 1 / (tau - sigma);
      if ((rc = eigsStep(r, cur, NULL, r->T, 1.0, 0.0, 0.0)) || (rc = eigsMassSolve(r)) ||
          (rc = r->ops->combine(r->B[r->iz], cur, prev, prev, r->n, r->p, r->ld, 2 * sn / e, -2 * sn * cc / e, -sigma * sn, r->stream))) return rc;
      double *t = prev; prev = cur; cur = t;
      sigma = sn;
    }
  } else {
    if ((rc = eigsStep(r, prev, NULL, cur, sigma1 / e, -sigma1 * cc / e, 0.0))) return rc;
    for (uint32_t i = 1; i < m; ++i) {
      double const sn = 1 / (tau - sigma);
      if ((rc = eigsStep(r, cur, prev, prev, 2 * sn / e, -2 * sn * cc / e, -sigma * sn))) return rc;
      double *t = prev; prev = cur; cur = t;
      sigma = sn;
    }
  }
  phaseEnd(r, PH_FILTER);
  if (cur != r->B[r->ix]) { uint32_t const t = r->ix; r->ix = r->iy; r->iy = t; }
  *used = m;
  return 0;
}

int bfhipChebCovEigsDevice(BfhipChebCov *c, BfhipEigsOptions const *opt, size_t nev, double *lam, double *residual, double *dU, size_t ldu,
                           BfhipEigsInfo *info, void *stream) {
  return bfEigsSolve(c, opt, NULL, NULL, nev, lam, residual, dU, ldu, info, stream);
}

/* Both entries.  `full` is the object's n (rows of every block); n below is n - m, the dimension of the space that is left, which
 * takes n's place in every limit.  With m == 0 nothing here differs from section 25: the same launches in the same order. */
int bfEigsSolve(BfhipChebCov *c, BfhipEigsOptions const *opt, BfhipEigsLocked const *locked, BfEigsDeflation const *defl, size_t nev, double *lam,
                double *residual, double *dU, size_t ldu, BfhipEigsInfo *info, void *stream) {
  if (!c || !lam || !dU) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  uint64_t const full = c->n;
  uint64_t const m = locked && locked->structSize == sizeof *locked ? locked->count : 0;
  uint64_t const n = m < full ? full - m : 0;
  if (nev == 0 || nev > 255 || nev > n) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "nev out of range (1 .. min(n, 255))");
  if (ldu < nev) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "ldu is less than nev");
  if (opt && opt->structSize != sizeof *opt) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "structSize is not sizeof(BfhipEigsOptions)");
  if (info && info->structSize != sizeof *info) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "structSize is not sizeof(BfhipEigsInfo)");
  uint32_t const flags = opt ? opt->flags : 0;
  uint64_t const cap = n < 256 ? n : 256;
  uint64_t guard = opt ? opt->guard : 0;
  if (guard) {
    if (nev + guard > 256) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "nev + guard is more than 256");
    if (flags & BFHIP_EIGS_NO_GUARD) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "guard: both a count and BFHIP_EIGS_NO_GUARD");
    if (nev + guard > n) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "nev + guard is more than n");
  } else if (flags & BFHIP_EIGS_NO_GUARD) {
    if (nev != n) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "guard: without a guard column the last pair never converges (the filter's lower cut sits on it); only nev == n runs without");
  } else {
    guard = nev / 4 > 8 ? nev / 4 : 8;
    if (nev + guard > cap) guard = cap - nev;
  }
  uint32_t const degree = opt && opt->degree ? opt->degree : 20, maxIter = opt && opt->maxIter ? opt->maxIter : 100;
  if (degree == 1) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "degree is 1 (at least 2)");
  double tol = opt ? opt->tol : 0;
  if (!(tol >= 0) || !isfinite(tol)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "tol is negative or not finite");
  if (tol == 0) tol = 1e-10;
  /* with a mass set the flag moves the spectrum's upper bound -- the filter's upper end and the scale of the tolerance -- to
   * lamMax / lo (without one the flag is refused below, after every older refusal) */
  int const consistent = (flags & BFHIP_EIGS_CONSISTENT_MASS) != 0;
  double const lamTop = consistent && c->dMass ? c->lamMax / c->massLo : c->lamMax;
  double lockMin = 0;
  if (locked) {
    if (locked->structSize != sizeof *locked) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "structSize is not sizeof(BfhipEigsLocked)");
    if (m && (!locked->dVectors || !locked->lam)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "locked: count > 0 with NULL dVectors or lam");
    if (locked->ld < m) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "locked: ld is less than count");
    if (m >= full) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "locked: count is not below n");
    for (uint64_t k = 0; k < m; ++k) {
      if (!isfinite(locked->lam[k]) || locked->lam[k] > lamTop)
        return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "locked: eigenvalue %llu is not finite or lies above lamMax", (unsigned long long)k);
      if (!k || locked->lam[k] < lockMin) lockMin = locked->lam[k];
    }
    if (m && (flags & BFHIP_EIGS_MASS_NORMALISED))
      return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "locked: BFHIP_EIGS_MASS_NORMALISED with locked vectors (they must be U; bfhipChebCovEigsMassNormaliseDevice scales at the end)");
    if (m && !defl) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "locked: no projection");
  }
  uint32_t massSteps = 0;
  if (consistent) {
    if (!c->dMass || !c->massOps)
      return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BFHIP_EIGS_CONSISTENT_MASS on an object with no consistent mass: call bfhipChebCovSetConsistentMass first");
    if (opt->massSteps > 64) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "massSteps is more than 64");
    massSteps = opt->massSteps;
    if (!massSteps) {
      /* the smallest k with 2 rho^k <= tol: 22 at 1e-10 on P1 masses (rho = 1/3) */
      double const sk = sqrt(c->massHi / c->massLo), rho = (sk - 1) / (sk + 1);
      double bound = 2 * rho;
      for (massSteps = 1; massSteps < 64 && bound > tol; ++massSteps) bound *= rho;
    }
  }

  EigsRun r = { .c = c, .n = full, .p = (uint32_t)(nev + guard), .nev = (uint32_t)nev, .ix = 0, .iy = 1, .iz = 2, .stream = stream,
                .dQ = m ? locked->dVectors : NULL, .ldq = m ? locked->ld : 0, .m = m, .lockMin = lockMin, .project = m ? defl->project : NULL,
                .ops = consistent ? c->massOps : NULL, .massSteps = massSteps };
  r.ld = (r.p + 15) / 16 * 16;
  size_t const p = r.p, ld = r.ld;
  uint64_t const chunkRows = bfdevEigsChunkRows(full, r.ld), chunks = (full + chunkRows - 1) / chunkRows;
  uint64_t const blockElems = full * ld, partElems = chunks * ld * ld, smallElems = 2 * ld * ld + 2 * ld;
  /* one panel's coefficients and their per-chunk partials: a function of (n, ld, m) alone */
  uint64_t const m16 = m < 256 ? (m + 15) / 16 * 16 : 256;
  uint64_t const crossRows = m ? defl->chunkRows(full, r.ld) : 1, crossChunks = m ? (full + crossRows - 1) / crossRows : 0;
  uint64_t const coefElems = m16 * ld, crossElems = crossChunks * m16 * ld;
  uint64_t const blocks = consistent ? 5 : 3;          /* section 28: T and the mass solve's second block */
  uint64_t const bytes = (blocks * blockElems + partElems + smallElems + coefElems + crossElems) * 8;
  void *dAll = NULL;
  double *host = NULL;
  uint32_t iterations = 0, converged = 0, maxDegree = 0;
  int rc, stored = 0;
  BfDevScope ds = {0};
  if (eigsProfileOn) { memset(eigsPhases, 0, sizeof eigsPhases); eigsHistoryCount = 0; }
  if ((rc = bfDevEnter(&ds, c->device))) return rc;
  host = malloc((2 * ld * ld + 4 * ld + 3) * sizeof *host);
  if (!host) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory"); goto out; }
  r.G = host; r.W = host + ld * ld; r.theta = r.W + ld * ld; r.res = r.theta + ld + 1; r.work = r.res + ld;          /* theta: ld + 1, work: 2 ld + 2 */
  if ((rc = bfdevMalloc(&dAll, bytes))) goto out;
  for (int k = 0; k < 3; ++k) r.B[k] = (double *)dAll + (uint64_t)k * blockElems;
  if (consistent) { r.T = (double *)dAll + 3 * blockElems; r.Z2 = (double *)dAll + 4 * blockElems; }
  r.dPart = (double *)dAll + blocks * blockElems;
  r.dG = r.dPart + partElems; r.dW = r.dG + ld * ld; r.dTheta = r.dW + ld * ld; r.dSumSq = r.dTheta + ld;
  r.dC = r.dSumSq + ld; r.dPartC = r.dC + coefElems;

  /* ---- the start block: X[i][j] = N(seed, i p + j); the padding columns of all three blocks are zero from here on ---- */
  uint64_t const seed = opt ? opt->seed : 0;
  if (p == ld) {
    if ((rc = bfdevFillNormal(r.B[0], full * p, 0, BFHIP_F64, seed, stream)) || (rc = bfdevMemsetAsync(r.B[1], 0, (blocks - 1) * blockElems * 8, stream))) goto out;
  } else {
    if ((rc = bfdevMemsetAsync(r.B[0], 0, blockElems * 8, stream)) || (rc = bfdevFillNormal(r.B[1], full * p, 0, BFHIP_F64, seed, stream)) ||
        (rc = bfdevMemcpy2DAsync(r.B[0], ld * 8, r.B[1], p * 8, p * 8, full, stream)) ||
        (rc = bfdevMemsetAsync(r.B[1], 0, (blocks - 1) * blockElems * 8, stream))) goto out;
  }

  if ((rc = eigsRayleighRitz(&r))) goto out;
  eigsRecord(r.res, nev, lamTop, 0);
  for (;;) {
    converged = 0;
    while (converged < nev && r.res[converged] <= tol * lamTop) ++converged;
    if (converged == nev || iterations == maxIter) break;
    uint32_t used = 0;
    if (p < n) {
      if ((rc = eigsFilter(&r, degree, lamTop, &used))) goto out;
      if (used > maxDegree) maxDegree = used;
    }
    ++iterations;
    if ((rc = eigsRayleighRitz(&r))) goto out;
    eigsRecord(r.res, nev, lamTop, used);
  }

  /* ---- the outputs, converged or not ---- */
  if ((rc = bfdevEigsStore(r.B[r.ix], full, r.ld, r.nev, flags & BFHIP_EIGS_MASS_NORMALISED ? (double const *)c->dD : NULL, dU, ldu, stream)) ||
      (rc = bfdevSync(stream))) goto out;
  stored = 1;
  if (converged < nev)
    rc = bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "eigensolver: %u of %zu pairs converged to %g x lamMax in %u iterations (the outputs hold the best pairs found)",
                   converged, nev, tol, iterations);
out:
  if (stored) {
    double worst = 0;
    for (size_t j = 0; j < nev; ++j) {
      lam[j] = r.theta[j];
      if (residual) residual[j] = r.res[j];
      if (r.res[j] > worst) worst = r.res[j];
    }
    if (info) {
      uint32_t const ss = info->structSize;
      memset(info, 0, sizeof *info);
      info->structSize = ss; info->iterations = iterations; info->converged = converged; info->blockColumns = r.p;
      info->maxDegreeUsed = maxDegree; info->operatorColumns = r.opColumns; info->workspaceBytes = bytes;
      info->maxResidual = worst / lamTop; info->lamMax = lamTop;
    }
  }
  if (dAll) { bfdevSync(stream); bfdevFree(dAll); }
  free(host);
  bfDevLeave(&ds);
  return rc;
}
