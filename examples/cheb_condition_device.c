/* examples/cheb_condition_device.c -- from a triangle mesh and measurements at some of its vertices to the kriging mean and the
 * posterior variance, on the device, with no eigenpairs and no butterfly: bfhipChebCovCondCreate over the Chebyshev route of
 * examples/cheb_cov_device.c, in plain C against include/bfhip.h.  The driver
 *   1. generates a latitude-longitude mesh of the unit sphere, assembles its P1 stiffness matrix and lumped mass, uploads
 *      S and fits the Matern spectral density (as examples/cheb_cov_device.c does),
 *   2. draws ONE prior field (bfhipChebCovDrawDevice) and takes its exact values at numObs vertices spread over the sphere
 *      as the observations y, with a tiny noise variance d (1e-4 of the mean prior variance at those vertices),
 *   3. conditions on them (bfhipChebCovCondCreate) and checks
 *        a. the kriging mean reproduces y at the observed vertices: there mean = G alpha = y - d alpha exactly, so
 *           |mean[a] - (y[a] - d alpha[a])| is rounding, and d max |alpha| <= 1e-2 max |y| (the observations are not fitted
 *           away as noise),
 *        b. the posterior variance at every observed vertex is at most the noise variance d (and not negative beyond
 *           rounding), while the prior variance there is 1e4 times larger,
 *   4. prints the log marginal likelihood and a few posterior draws' spread at an unobserved vertex.
 * Exit 0 only if 3a and 3b hold.
 *
 *   gcc -O2 -std=gnu11 -Wall -Werror -Iinclude examples/cheb_condition_device.c -Lbutterfly_amd/csrc -lbfhip -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/butterfly_amd/csrc -Wl,-rpath,/opt/rocm/lib -o /tmp/cheb_condition_device
 *   /tmp/cheb_condition_device [numLat = 48] [numLon = 96] [order = 64] [numObs = 100]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip.h"

extern int hipMalloc(void **p, size_t bytes);
extern int hipFree(void *p);
extern int hipMemcpy(void *dst, void const *src, size_t bytes, int kind);   /* 1: H2D, 2: D2H */
extern int hipDeviceSynchronize(void);

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s failed: %s (%s)\n", #call, bfhipErrorString(rc_), bfhipLastErrorMessage()); return 2; } } while (0)
#define HIP(call) do { if (call) { fprintf(stderr, "%s failed\n", #call); return 3; } } while (0)

typedef struct { double kappa, nu; } Matern;
static double density(double lambda, void *ctx) {
  Matern const *m = ctx;
  return pow(fabs(1 + m->kappa * m->kappa * lambda), -m->nu / 4 - 0.5);
}

int main(int argc, char **argv) {
  uint64_t const numLat = argc > 1 ? strtoull(argv[1], NULL, 10) : 48, numLon = argc > 2 ? strtoull(argv[2], NULL, 10) : 96;
  size_t const order = argc > 3 ? strtoull(argv[3], NULL, 10) : 64;
  uint64_t const n = 2 + numLat * numLon, numFaces = 2 * numLon * numLat;
  size_t const k = argc > 4 ? strtoull(argv[4], NULL, 10) : 100;
  if (numLat < 2 || numLon < 3 || order < 1 || k < 1 || k > BFHIP_COND_MAX_OBS || k > n / 4) {
    fprintf(stderr, "usage: %s [numLat >= 2] [numLon >= 3] [order >= 1] [1 <= numObs <= min(%u, vertices / 4)]\n", argv[0], BFHIP_COND_MAX_OBS);
    return 1;
  }

  /* ---- 1. the mesh (two poles and numLat rings of numLon vertices), S and the polynomial ---- */
  double *verts = malloc(3 * n * sizeof *verts);
  uint64_t *faces = malloc(3 * numFaces * sizeof *faces);
  if (!verts || !faces) return 1;
  verts[0] = 0; verts[1] = 0; verts[2] = 1;
  verts[3 * (n - 1)] = 0; verts[3 * (n - 1) + 1] = 0; verts[3 * (n - 1) + 2] = -1;
  for (uint64_t r = 0; r < numLat; ++r)
    for (uint64_t j = 0; j < numLon; ++j) {
      double const th = M_PI * (double)(r + 1) / (double)(numLat + 1), ph = 2 * M_PI * (double)j / (double)numLon;
      double *v = verts + 3 * (1 + r * numLon + j);
      v[0] = sin(th) * cos(ph); v[1] = sin(th) * sin(ph); v[2] = cos(th);
    }
  uint64_t nf = 0;
  for (uint64_t j = 0; j < numLon; ++j) {
    uint64_t const jn = (j + 1) % numLon;
    faces[3 * nf] = 0; faces[3 * nf + 1] = 1 + j; faces[3 * nf + 2] = 1 + jn; ++nf;
    for (uint64_t r = 0; r + 1 < numLat; ++r) {
      uint64_t const a = 1 + r * numLon + j, b = 1 + (r + 1) * numLon + j, c = 1 + (r + 1) * numLon + jn, d = 1 + r * numLon + jn;
      faces[3 * nf] = a; faces[3 * nf + 1] = b; faces[3 * nf + 2] = c; ++nf;
      faces[3 * nf] = a; faces[3 * nf + 1] = c; faces[3 * nf + 2] = d; ++nf;
    }
    faces[3 * nf] = 1 + (numLat - 1) * numLon + j; faces[3 * nf + 1] = n - 1; faces[3 * nf + 2] = 1 + (numLat - 1) * numLon + jn; ++nf;
  }
  uint64_t nnz = 0;
  CHECK(bfhipTrimeshLboFemCount(n, nf, faces, &nnz));
  uint64_t *rowptr = malloc((n + 1) * sizeof *rowptr), *colind = malloc(nnz * sizeof *colind);
  double *L = malloc(nnz * sizeof *L), *mass = malloc(n * sizeof *mass);
  if (!rowptr || !colind || !L || !mass) return 1;
  CHECK(bfhipTrimeshLboFem(n, verts, nf, faces, rowptr, colind, L, mass));
  BfhipChebCov *cov = NULL;
  CHECK(bfhipChebCovCreate(-1, n, rowptr, colind, L, mass, 0.0, &cov));
  BfhipChebCovInfo info;
  memset(&info, 0, sizeof info);
  info.structSize = sizeof info;
  CHECK(bfhipChebCovGetInfo(cov, &info));
  Matern matern = { 0.5, 2.0 };
  double *coef = malloc(order * sizeof *coef);
  if (!coef) return 1;
  CHECK(bfhipChebFit(order, 0.0, info.lamMax, density, &matern, coef));
  CHECK(bfhipChebCovSetCoefficients(cov, coef, order));
  printf("sphere mesh: %llu vertices, %llu nonzeros; lamMax %.4f, order %zu\n", (unsigned long long)n, (unsigned long long)nnz, info.lamMax, order);

  /* ---- 2. one prior field and its values at k vertices, a stride apart ---- */
  uint64_t const q = 8;                                    /* posterior draws of step 4 */
  double *z = malloc(n * q * sizeof *z), *y = malloc(k * sizeof *y), *noise = malloc(k * sizeof *noise), *alpha = malloc(k * sizeof *alpha);
  double *prior = malloc(k * sizeof *prior), *post = malloc(k * sizeof *post);
  uint64_t *obs = malloc(k * sizeof *obs);
  if (!z || !y || !noise || !alpha || !prior || !post || !obs) return 1;
  void *dZ = NULL, *dY = NULL, *dAlpha = NULL, *dVar = NULL, *dValue = NULL;
  HIP(hipMalloc(&dZ, n * q * 8)); HIP(hipMalloc(&dY, k * 8)); HIP(hipMalloc(&dAlpha, k * 8)); HIP(hipMalloc(&dVar, 2 * k * 8)); HIP(hipMalloc(&dValue, 3 * 8));
  CHECK(bfhipChebCovDrawDevice(cov, 2025, 0, 1, dZ, NULL));
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(z, dZ, n * 8, 2));
  for (size_t a = 0; a < k; ++a) { obs[a] = 1 + a * ((n - 2) / k); y[a] = z[obs[a]]; }
  HIP(hipMemcpy(dY, y, k * 8, 1));

  /* the noise needs the prior variance's scale: a first object with unit noise gives it (the prior does not depend on the noise) */
  BfhipCovCond *cond = NULL;
  for (size_t a = 0; a < k; ++a) noise[a] = 1.0;
  CHECK(bfhipChebCovCondCreate(cov, obs, k, noise, &cond, NULL));
  CHECK(bfhipCovCondVarianceDevice(cond, obs, k, dVar, NULL, NULL));
  HIP(hipMemcpy(prior, dVar, k * 8, 2));
  bfhipCovCondFree(&cond);
  double meanPrior = 0;
  for (size_t a = 0; a < k; ++a) meanPrior += prior[a] / (double)k;
  double const d = 1e-4 * meanPrior;
  for (size_t a = 0; a < k; ++a) noise[a] = d;

  /* ---- 3. condition; the mean at the observed vertices, the variances there ---- */
  CHECK(bfhipChebCovCondCreate(cov, obs, k, noise, &cond, NULL));
  BfhipCovCondInfo ci;
  memset(&ci, 0, sizeof ci);
  ci.structSize = sizeof ci;
  CHECK(bfhipCovCondGetInfo(cond, &ci));
  printf("conditioned on %u vertices: %llu panels, rows %.3f s, Gram %.3f s, Cholesky %.3f s, %.2f MB; pivots in [%.3e, %.3e]\n", ci.numObs,
         (unsigned long long)ci.setupApplies, ci.rowsSeconds, ci.gramSeconds, ci.factorSeconds, (double)ci.factorBytes / 1e6, ci.minPivot, ci.maxPivot);
  CHECK(bfhipCovCondMeanDevice(cond, dY, dZ, dAlpha, NULL));
  CHECK(bfhipCovCondVarianceDevice(cond, obs, k, dVar, (double *)dVar + k, NULL));
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(z, dZ, n * 8, 2)); HIP(hipMemcpy(alpha, dAlpha, k * 8, 2));
  HIP(hipMemcpy(prior, dVar, k * 8, 2)); HIP(hipMemcpy(post, (double *)dVar + k, k * 8, 2));
  double ymax = 0, amax = 0, worstIdentity = 0, worstMisfit = 0, maxPost = -INFINITY, minPost = INFINITY, minPrior = INFINITY;
  for (size_t a = 0; a < k; ++a) {
    double const m = z[obs[a]];
    if (fabs(y[a]) > ymax) ymax = fabs(y[a]);
    if (fabs(alpha[a]) > amax) amax = fabs(alpha[a]);
    if (fabs(m - (y[a] - d * alpha[a])) > worstIdentity) worstIdentity = fabs(m - (y[a] - d * alpha[a]));
    if (fabs(m - y[a]) > worstMisfit) worstMisfit = fabs(m - y[a]);
    if (post[a] > maxPost) maxPost = post[a];
    if (post[a] < minPost) minPost = post[a];
    if (prior[a] < minPrior) minPrior = prior[a];
  }
  /* G alpha is a sum of k products of size max |G| max |alpha| <= max prior * max |alpha|; the solve adds its backward error, 1e-12 */
  double const rounding = 1e-10 * (ymax + meanPrior * amax * (double)k);
  printf("kriging mean at the observed vertices: max |mean - y| = %.3e (max |y| = %.3e), max |mean - (y - d alpha)| = %.3e (rounding allowance %.1e)\n",
         worstMisfit, ymax, worstIdentity, rounding);
  printf("posterior variance at the observed vertices: in [%.3e, %.3e], noise variance %.3e, prior variance >= %.3e\n", minPost, maxPost, d, minPrior);
  int const meanOk = worstIdentity <= rounding && d * amax <= 1e-2 * ymax && worstMisfit <= 1e-2 * ymax;
  int const varOk = maxPost <= d && minPost >= -1e-10 * meanPrior && minPrior > 100 * d;

  /* ---- 4. the likelihood and a few posterior draws ---- */
  double value[3];
  CHECK(bfhipCovCondLogLikelihoodDevice(cond, dY, dValue, NULL, NULL, NULL, NULL));
  CHECK(bfhipCovCondDrawDevice(cond, dY, 7, 8, 0, q, dZ, NULL));
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(value, dValue, 3 * 8, 2)); HIP(hipMemcpy(z, dZ, n * q * 8, 2));
  uint64_t const at = obs[0] + ((n - 2) / k + 1) / 2;       /* half a stride past an observed vertex */
  double lo = INFINITY, hi = -INFINITY;
  for (uint64_t s = 0; s < q; ++s) { double const v = z[at * q + s]; if (v < lo) lo = v; if (v > hi) hi = v; }
  printf("log marginal likelihood %.6f (quad %.4f, logDet %.4f); %llu posterior draws at vertex %llu lie in [%.4f, %.4f], at observed vertex %llu in [",
         value[0], value[1], value[2], (unsigned long long)q, (unsigned long long)at, lo, hi, (unsigned long long)obs[0]);
  lo = INFINITY; hi = -INFINITY;
  for (uint64_t s = 0; s < q; ++s) { double const v = z[obs[0] * q + s]; if (v < lo) lo = v; if (v > hi) hi = v; }
  printf("%.4f, %.4f] (y = %.4f)\n", lo, hi, y[0]);

  bfhipCovCondFree(&cond);                                 /* before the BfhipChebCov it references */
  hipFree(dZ); hipFree(dY); hipFree(dAlpha); hipFree(dVar); hipFree(dValue);
  bfhipChebCovFree(&cov);
  free(verts); free(faces); free(rowptr); free(colind); free(L); free(mass); free(coef); free(z); free(y); free(noise); free(alpha); free(prior); free(post); free(obs);
  if (!meanOk) { fprintf(stderr, "the kriging mean does not reproduce the observed values\n"); return 5; }
  if (!varOk) { fprintf(stderr, "the posterior variance at an observed vertex is above the noise variance (or negative)\n"); return 6; }
  return 0;
}
