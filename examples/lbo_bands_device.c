/* examples/lbo_bands_device.c -- more Laplace-Beltrami eigenpairs than one block holds, band after band: each call of
 * bfhipChebCovEigsBandDevice returns the pairs that follow the ones already found, deflating against them on the device, in
 * plain C against include/bfhip.h.  The driver
 *   1. generates the latitude-longitude sphere of examples/lbo_eigs_device.c (1154 vertices) and uploads S (bfhipChebCovCreate),
 *   2. computes 49 pairs in three bands of 16, 20 and 13 into ONE device array dAll [n x 49]: call k passes the columns
 *      found so far as the locked block and dAll + m as its output, so nothing is copied between the calls,
 *   3. checks on the host: eigenvalues ascending across the band boundaries, every residual at or below tol x lamMax,
 *      ||U^T U - I||_max over all 49 columns at or below 1e-12 (the bands are orthogonal to each other),
 *   4. mass-normalises in place (bfhipChebCovEigsMassNormaliseDevice), prints the values beside l(l+1), and exits 0.
 *
 *   gcc -O2 -std=gnu11 -Wall -Werror -Iinclude examples/lbo_bands_device.c -Lbutterfly_amd/csrc -lbfhip -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/butterfly_amd/csrc -Wl,-rpath,/opt/rocm/lib -o /tmp/lbo_bands_device
 *   /tmp/lbo_bands_device [numLat = 24] [numLon = 48]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip.h"

extern int hipMalloc(void **p, size_t bytes);
extern int hipFree(void *p);
extern int hipMemcpy(void *dst, void const *src, size_t bytes, int kind);   /* 1: H2D, 2: D2H */

#define CHECK(call) do { int rc_ = (call); if (rc_) { fprintf(stderr, "%s failed: %s (%s)\n", #call, bfhipErrorString(rc_), bfhipLastErrorMessage()); return 2; } } while (0)
#define HIP(call) do { if (call) { fprintf(stderr, "%s failed\n", #call); return 3; } } while (0)

enum { BANDS = 3, TOTAL = 49 };
static size_t const bandNev[BANDS] = { 16, 20, 13 };      /* the boundaries 16, 36, 49 are squares: between two l(l+1) */

int main(int argc, char **argv) {
  uint64_t const numLat = argc > 1 ? strtoull(argv[1], NULL, 10) : 24, numLon = argc > 2 ? strtoull(argv[2], NULL, 10) : 48;
  if (numLat < 4 || numLon < 8) { fprintf(stderr, "usage: %s [numLat >= 4] [numLon >= 8]\n", argv[0]); return 1; }

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
  printf("sphere mesh: %llu vertices, %llu faces, %llu nonzeros\n", (unsigned long long)n, (unsigned long long)nf, (unsigned long long)nnz);

  BfhipChebCov *cov = NULL;
  double lamMax = 0;
  CHECK(bfhipChebCovCreate(-1, n, rowptr, colind, L, mass, 0.0, &cov));

  /* ---- 2. three bands into one array ---- */
  double const tol = 1e-10;
  double lam[TOTAL], res[TOTAL];
  void *dAll = NULL;
  HIP(hipMalloc(&dAll, n * TOTAL * 8));
  size_t m = 0;
  for (int k = 0; k < BANDS; ++k) {
    BfhipEigsOptions opt;
    memset(&opt, 0, sizeof opt);
    opt.structSize = sizeof opt;
    opt.seed = 2025;
    opt.tol = tol;
    BfhipEigsInfo info;
    memset(&info, 0, sizeof info);
    info.structSize = sizeof info;
    BfhipEigsLocked locked;
    memset(&locked, 0, sizeof locked);
    locked.structSize = sizeof locked;
    locked.count = m; locked.dVectors = dAll; locked.ld = TOTAL; locked.lam = lam;
    CHECK(bfhipChebCovEigsBandDevice(cov, &opt, &locked, bandNev[k], lam + m, res + m, (double *)dAll + m, TOTAL, &info, NULL));
    printf("band %d: pairs %zu .. %zu, block of %u columns, %u outer iterations, largest degree %u, %llu columns of S applied, %.2f MB of workspace\n",
           k, m, m + bandNev[k] - 1, info.blockColumns, info.iterations, info.maxDegreeUsed, (unsigned long long)info.operatorColumns,
           (double)info.workspaceBytes / 1e6);
    lamMax = info.lamMax;
    m += bandNev[k];
  }

  /* ---- 3. the checks ---- */
  double *U = malloc(n * TOTAL * sizeof *U);
  if (!U) return 1;
  HIP(hipMemcpy(U, dAll, n * TOTAL * 8, 2));
  int ok = fabs(lam[0]) <= tol * lamMax;
  double orth = 0;
  for (int a = 0; a < TOTAL; ++a) {
    if (a && lam[a] < lam[a - 1]) { fprintf(stderr, "lambda_%d < lambda_%d\n", a, a - 1); ok = 0; }
    if (!(res[a] <= tol * lamMax)) { fprintf(stderr, "residual %d is %g x lamMax\n", a, res[a] / lamMax); ok = 0; }
    for (int b = 0; b <= a; ++b) {
      double s = 0;
      for (uint64_t i = 0; i < n; ++i) s += U[i * TOTAL + a] * U[i * TOTAL + b];
      orth = fmax(orth, fabs(s - (a == b)));
    }
  }
  printf("||U^T U - I||_max over all %d columns: %.3e\n", TOTAL, orth);
  if (!(orth <= 1e-12)) ok = 0;

  /* ---- 4. Phi = D U in place ---- */
  CHECK(bfhipChebCovEigsMassNormaliseDevice(cov, dAll, TOTAL, TOTAL, NULL));
  HIP(hipMemcpy(U, dAll, n * TOTAL * 8, 2));
  printf("  j   lambda_j          l(l+1)   difference   residual / lamMax   Phi_j^T M Phi_j\n");
  for (int j = 0; j < TOTAL; ++j) {
    int const l = (int)floor(sqrt((double)j));                 /* l(l+1) has multiplicity 2l + 1: indices l^2 .. l^2 + 2l */
    double mnorm = 0;
    for (uint64_t i = 0; i < n; ++i) mnorm += mass[i] * U[i * TOTAL + j] * U[i * TOTAL + j];
    if (j < 4 || j % 6 == 0 || j == TOTAL - 1)
      printf("%3d   %14.10f   %6d   %10.3e   %10.3e          %.12f\n", j, lam[j], l * (l + 1), lam[j] - l * (l + 1), res[j] / lamMax, mnorm);
    if (!(fabs(mnorm - 1) <= 1e-12)) ok = 0;
  }

  hipFree(dAll);
  bfhipChebCovFree(&cov);
  free(verts); free(faces); free(rowptr); free(colind); free(L); free(mass); free(U);
  if (!ok) { fprintf(stderr, "a check failed (tolerance %g x lamMax)\n", tol); return 5; }
  return 0;
}
