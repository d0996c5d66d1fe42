/* examples/cheb_cov_device.c -- from a triangle mesh to samples of a Matern field on the device, with no eigenpairs and no
 * butterfly: the route of the reference's examples/covariance/cheb_cov.c (a Chebyshev polynomial of S = M^-1/2 L M^-1/2 with
 * the lumped mass), in plain C against include/bfhip.h.  The driver
 *   1. generates a latitude-longitude mesh of the unit sphere and assembles its P1 stiffness matrix and lumped mass
 *      (bfhipTrimeshLboFem),
 *   2. uploads S (bfhipChebCovCreate; lamMax: the Gershgorin bound) and fits the Matern spectral density on [0, lamMax]
 *      (bfhipChebFit),
 *   3. checks p(S) on the null vector of S -- sqrt(mass), since L 1 = 0 -- against p(0) = bfhipChebEval(.., 0): the answer is
 *      known exactly,
 *   4. draws numSamples samples 64 at a time (bfhipChebCovDrawDevice) and prints their pointwise variance next to the
 *      diagonal entry of one covariance column (bfhipChebCovMatvecBlockDevice on a unit vector).
 *
 *   gcc -O2 -std=gnu11 -Wall -Werror -Iinclude examples/cheb_cov_device.c -Lbutterfly_amd/csrc -lbfhip -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/butterfly_amd/csrc -Wl,-rpath,/opt/rocm/lib -o /tmp/cheb_cov_device
 *   /tmp/cheb_cov_device [numLat = 48] [numLon = 96] [numSamples = 64] [order = 64]
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
/* the two densities of cheb_cov.c: squared exponential for nu == 0, else Matern normalised to 1 at lambda = 0 */
static double density(double lambda, void *ctx) {
  Matern const *m = ctx;
  if (m->nu == 0) return exp(-m->kappa * lambda * lambda);
  return pow(fabs(1 + m->kappa * m->kappa * lambda), -m->nu / 4 - 0.5);
}

int main(int argc, char **argv) {
  uint64_t const numLat = argc > 1 ? strtoull(argv[1], NULL, 10) : 48, numLon = argc > 2 ? strtoull(argv[2], NULL, 10) : 96;
  uint64_t const numSamples = argc > 3 ? strtoull(argv[3], NULL, 10) : 64;
  size_t const order = argc > 4 ? strtoull(argv[4], NULL, 10) : 64;
  if (numLat < 2 || numLon < 3 || numSamples < 1 || order < 1) { fprintf(stderr, "usage: %s [numLat >= 2] [numLon >= 3] [numSamples >= 1] [order >= 1]\n", argv[0]); return 1; }

  /* ---- 1. the mesh: two poles and numLat rings of numLon vertices ---- */
  uint64_t const n = 2 + numLat * numLon, numFaces = 2 * numLon * numLat;
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
  double area = 0;
  for (uint64_t i = 0; i < n; ++i) area += mass[i];
  printf("sphere mesh: %llu vertices, %llu faces, %llu nonzeros, area %.6f (4 pi = %.6f)\n", (unsigned long long)n, (unsigned long long)nf,
         (unsigned long long)nnz, area, 4 * M_PI);

  /* ---- 2. the operator and the polynomial ---- */
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
  CHECK(bfhipChebCovGetInfo(cov, &info));
  printf("S: lamMax (Gershgorin) %.4f, order %llu, error estimate %.2e, %.2f MB on the device\n", info.lamMax, (unsigned long long)info.order,
         info.errorEstimate, (double)info.deviceBytes / 1e6);

  /* ---- 3. p(S) on the null vector of S ---- */
  double *x = malloc(n * sizeof *x), *y = malloc(n * sizeof *y);
  if (!x || !y) return 1;
  for (uint64_t i = 0; i < n; ++i) x[i] = 3.0 * sqrt(mass[i]);
  void *dX = NULL, *dY = NULL, *dZ = NULL;
  uint64_t const q = numSamples < 64 ? numSamples : 64;
  HIP(hipMalloc(&dX, n * 8)); HIP(hipMalloc(&dY, n * 8)); HIP(hipMalloc(&dZ, n * q * 8));
  HIP(hipMemcpy(dX, x, n * 8, 1));
  CHECK(bfhipChebCovApplyBlockDevice(cov, dX, 1, dY, NULL));
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(y, dY, n * 8, 2));
  double const p0 = bfhipChebEval(order, 0.0, info.lamMax, coef, 0.0);
  double sumAbs = 0, worst = 0, xmax = 0;
  for (size_t k = 0; k < order; ++k) sumAbs += fabs(coef[k]);
  for (uint64_t i = 0; i < n; ++i) {
    double const e = fabs(y[i] - p0 * x[i]);
    if (e > worst) worst = e;
    if (fabs(x[i]) > xmax) xmax = fabs(x[i]);
  }
  /* S x = 0 holds to rounding only (the rows of L sum to a few ulp); every degree then adds a few ulp of sum |c_k| max |x| */
  double const tol = 64.0 * (double)order * 2.220446049250313e-16 * sumAbs * xmax;
  printf("p(S) on the null vector: p(0) = %.12f, worst |y - p(0) x| = %.2e (tolerance %.2e)\n", p0, worst, tol);

  /* ---- 4. samples and one covariance column ---- */
  double *z = malloc(n * q * sizeof *z), *var = calloc(n, sizeof *var);
  if (!z || !var) return 1;
  for (uint64_t s0 = 0; s0 < numSamples; s0 += q) {
    uint64_t const b = numSamples - s0 < q ? numSamples - s0 : q;
    CHECK(bfhipChebCovDrawDevice(cov, 2025, s0, b, dZ, NULL));
    HIP(hipDeviceSynchronize());
    HIP(hipMemcpy(z, dZ, n * b * 8, 2));
    for (uint64_t i = 0; i < n; ++i) for (uint64_t s = 0; s < b; ++s) var[i] += z[i * b + s] * z[i * b + s] / (double)numSamples;
  }
  uint64_t const at = 1 + (numLat / 2) * numLon;             /* a vertex near the equator */
  memset(x, 0, n * sizeof *x);
  x[at] = 1;
  HIP(hipMemcpy(dX, x, n * 8, 1));
  CHECK(bfhipChebCovMatvecBlockDevice(cov, dX, 1, dY, NULL));
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(y, dY, n * 8, 2));
  printf("covariance column %llu: C[at, at] = %.6e, C[at + 1, at] = %.6e, C[south pole, at] = %.6e\n", (unsigned long long)at, y[at], y[at + 1], y[n - 1]);
  printf("pointwise variance of %llu samples at that vertex: %.6e\n", (unsigned long long)numSamples, var[at]);
  int const finite = isfinite(y[at]) && y[at] > 0 && isfinite(var[at]) && var[at] > 0;

  hipFree(dX); hipFree(dY); hipFree(dZ);
  bfhipChebCovFree(&cov);
  free(verts); free(faces); free(rowptr); free(colind); free(L); free(mass); free(coef); free(x); free(y); free(z); free(var);
  if (!(worst <= tol)) { fprintf(stderr, "p(S) on the null vector of S is not p(0) times it\n"); return 5; }
  if (!finite) { fprintf(stderr, "the covariance column or the sample variance is not a positive finite number\n"); return 6; }
  return 0;
}
