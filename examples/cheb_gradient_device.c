/* examples/cheb_gradient_device.c -- the gradient of the log marginal likelihood in a parameter of the spectral density, on the
 * device, on the Chebyshev route: bfhipChebCovCondLogLikGradDevice in plain C against include/bfhip.h, checked against central
 * differences of the library's own likelihood value.  The driver
 *   1. generates the latitude-longitude mesh of the unit sphere of the other drivers (24 rings of 48: 1154 vertices), assembles
 *      its P1 stiffness matrix and lumped mass, uploads S and fits the Matern density (kappa = 0.5, nu = 2) at 64 points,
 *   2. draws one prior field and takes its values at 100 vertices as the observations y (noise variance 1e-2 of the mean prior
 *      variance there, held fixed from here on),
 *   3. fits d g / d kappa at the same 64 points -- the fit is linear, so these ARE the derivatives of p's coefficients -- and
 *      computes grad = d logLik / d kappa,
 *   4. computes the central differences FD(h) and FD(2h), h = 1e-3, of bfhipCovCondLogLikelihoodDevice's value over four more
 *      bfhipChebCovCondCreate (kappa -+ h, kappa -+ 2h).
 * FD(h) - grad = h^2 f''' / 6 + O(h^4) and FD(2h) - grad = 4 h^2 f''' / 6, so |FD(h) - FD(2h)| is three times the predicted
 * truncation error of FD(h); the rounding of a difference of two likelihood values, about 1e-13 |logLik| / h, is far below it.
 * Exit 0 only if |grad - FD(h)| <= |FD(h) - FD(2h)|: no tolerance is invented.
 *
 *   gcc -O2 -std=gnu11 -Wall -Werror -Iinclude examples/cheb_gradient_device.c -Lbutterfly_amd/csrc -lbfhip -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/butterfly_amd/csrc -Wl,-rpath,/opt/rocm/lib -o /tmp/cheb_gradient_device
 *   /tmp/cheb_gradient_device
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
static double densityDKappa(double lambda, void *ctx) {
  Matern const *m = ctx;
  double const e = -m->nu / 4 - 0.5;
  return e * pow(1 + m->kappa * m->kappa * lambda, e - 1) * 2 * m->kappa * lambda;
}

enum { ORDER = 64, NUM_OBS = 100 };

/* the likelihood value of y under the density at kappa: new coefficients, a new conditioning object */
static int likelihoodAt(BfhipChebCov *cov, double lamMax, double kappa, double nu, uint64_t const *obs, double const *noise, double const *dY, double *dValue,
                        double *logLik) {
  Matern m = { kappa, nu };
  double coef[ORDER], value[3];
  BfhipCovCond *cond = NULL;
  CHECK(bfhipChebFit(ORDER, 0.0, lamMax, density, &m, coef));
  CHECK(bfhipChebCovSetCoefficients(cov, coef, ORDER));
  CHECK(bfhipChebCovCondCreate(cov, obs, NUM_OBS, noise, &cond, NULL));
  CHECK(bfhipCovCondLogLikelihoodDevice(cond, dY, dValue, NULL, NULL, NULL, NULL));
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(value, dValue, sizeof value, 2));
  bfhipCovCondFree(&cond);
  *logLik = value[0];
  return 0;
}

int main(void) {
  uint64_t const numLat = 24, numLon = 48, n = 2 + numLat * numLon, numFaces = 2 * numLon * numLat;
  size_t const k = NUM_OBS;
  double const kappa = 0.5, nu = 2.0, h = 1e-3;

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
  Matern matern = { kappa, nu };
  double coef[ORDER], dcoef[ORDER];
  CHECK(bfhipChebFit(ORDER, 0.0, info.lamMax, density, &matern, coef));
  CHECK(bfhipChebFit(ORDER, 0.0, info.lamMax, densityDKappa, &matern, dcoef));
  CHECK(bfhipChebCovSetCoefficients(cov, coef, ORDER));
  printf("sphere mesh: %llu vertices, %llu nonzeros; lamMax %.4f, order %d, Matern(kappa = %.2f, nu = %.1f)\n", (unsigned long long)n,
         (unsigned long long)nnz, info.lamMax, (int)ORDER, kappa, nu);

  /* ---- 2. one prior field, its values at k vertices a stride apart, the noise ---- */
  double *z = malloc(n * sizeof *z), y[NUM_OBS], noise[NUM_OBS], prior[NUM_OBS];
  uint64_t obs[NUM_OBS];
  if (!z) return 1;
  void *dZ = NULL, *dY = NULL, *dVar = NULL, *dValue = NULL, *dGrad = NULL;
  HIP(hipMalloc(&dZ, n * 8)); HIP(hipMalloc(&dY, k * 8)); HIP(hipMalloc(&dVar, k * 8)); HIP(hipMalloc(&dValue, 3 * 8)); HIP(hipMalloc(&dGrad, 8));
  CHECK(bfhipChebCovDrawDevice(cov, 2025, 0, 1, dZ, NULL));
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(z, dZ, n * 8, 2));
  for (size_t a = 0; a < k; ++a) { obs[a] = 1 + a * ((n - 2) / k); y[a] = z[obs[a]]; noise[a] = 1.0; }
  HIP(hipMemcpy(dY, y, k * 8, 1));
  BfhipCovCond *cond = NULL;
  CHECK(bfhipChebCovCondCreate(cov, obs, k, noise, &cond, NULL));          /* the prior variance does not depend on the noise */
  CHECK(bfhipCovCondVarianceDevice(cond, obs, k, dVar, NULL, NULL));
  HIP(hipMemcpy(prior, dVar, k * 8, 2));
  bfhipCovCondFree(&cond);
  double meanPrior = 0;
  for (size_t a = 0; a < k; ++a) meanPrior += prior[a] / (double)k;
  for (size_t a = 0; a < k; ++a) noise[a] = 1e-2 * meanPrior;

  /* ---- 3. the gradient in kappa ---- */
  size_t const orders[1] = { ORDER };
  double grad = 0, value[3];
  CHECK(bfhipChebCovCondCreate(cov, obs, k, noise, &cond, NULL));
  CHECK(bfhipChebCovCondLogLikGradDevice(cond, dY, dcoef, orders, 1, ORDER, dGrad, dValue, NULL, NULL));
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(&grad, dGrad, 8, 2)); HIP(hipMemcpy(value, dValue, sizeof value, 2));
  bfhipCovCondFree(&cond);
  printf("log marginal likelihood %.9f (quad %.6f, logDet %.6f) of %zu observations, noise variance %.3e\n", value[0], value[1], value[2], k, noise[0]);

  /* ---- 4. central differences of the library's own value over four more Creates ---- */
  double lik[4];
  double const at[4] = { kappa + h, kappa - h, kappa + 2 * h, kappa - 2 * h };
  for (int i = 0; i < 4; ++i) {
    int const rc = likelihoodAt(cov, info.lamMax, at[i], nu, obs, noise, dY, dValue, &lik[i]);
    if (rc) return rc;
  }
  double const fd1 = (lik[0] - lik[1]) / (2 * h), fd2 = (lik[2] - lik[3]) / (4 * h);
  printf("d logLik / d kappa: grad = %.12e, FD(h) = %.12e, FD(2h) = %.12e, h = %.0e\n", grad, fd1, fd2, h);
  printf("|grad - FD(h)| = %.3e, |FD(h) - FD(2h)| = %.3e (three times the predicted truncation error of FD(h))\n", fabs(grad - fd1), fabs(fd1 - fd2));
  int const ok = fabs(grad - fd1) <= fabs(fd1 - fd2);

  hipFree(dZ); hipFree(dY); hipFree(dVar); hipFree(dValue); hipFree(dGrad);
  bfhipChebCovFree(&cov);
  free(verts); free(faces); free(rowptr); free(colind); free(L); free(mass); free(z);
  if (!ok) { fprintf(stderr, "the gradient is further from FD(h) than FD(h) is from FD(2h)\n"); return 5; }
  return 0;
}
