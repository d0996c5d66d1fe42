/* examples/lbo_consistent_device.c -- the lowest Laplace-Beltrami eigenpairs of a triangle mesh with the CONSISTENT P1 mass, the
 * pencil L phi = lambda M phi the reference solves with ARPACK and UMFPACK, on the device with no factorisation
 * (BFHIP_EIGS_CONSISTENT_MASS, include/bfhip.h), in plain C against include/bfhip.h.  The driver
 *   1. generates the latitude-longitude mesh of the unit sphere of examples/lbo_eigs_device.c (24 rings of 48: 1154 vertices)
 *      and assembles L, the lumped mass (bfhipTrimeshLboFem) and the consistent mass M on the same pattern (bfhipTrimeshLboFemMass),
 *   2. uploads S (bfhipChebCovCreate) and B = D M D (bfhipChebCovSetConsistentMass with the P1 bounds [1/4, 1]),
 *   3. computes the lowest 49 pairs (l = 0 .. 6) of the lumped and of the consistent pencil, mass-normalised, and prints them
 *      beside the sphere's l(l+1): the distances are the O(h^2) errors of the two P1 discretisations, printed and not judged,
 *   4. checks Phi^T M Phi = I with the consistent M on the host, and exits 0 when that holds to 1e-9, every residual of both
 *      calls is at or below tol x its lamMax and both lambda_0 are too.
 *
 *   gcc -O2 -std=gnu11 -Wall -Werror -Iinclude examples/lbo_consistent_device.c -Lbutterfly_amd/csrc -lbfhip -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/butterfly_amd/csrc -Wl,-rpath,/opt/rocm/lib -o /tmp/lbo_consistent_device
 *   /tmp/lbo_consistent_device [numLat = 24] [numLon = 48]
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

enum { NEV = 49 };

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
  double *M = malloc(nnz * sizeof *M);
  if (!M) return 1;
  CHECK(bfhipTrimeshLboFemMass(n, verts, nf, faces, rowptr, colind, M));
  printf("sphere mesh: %llu vertices, %llu faces, %llu nonzeros\n", (unsigned long long)n, (unsigned long long)nf, (unsigned long long)nnz);

  /* ---- 2. the operator and the consistent mass ---- */
  BfhipChebCov *cov = NULL;
  CHECK(bfhipChebCovCreate(-1, n, rowptr, colind, L, mass, 0.0, &cov));
  CHECK(bfhipChebCovSetConsistentMass(cov, M, 0.0, 0.0));

  /* ---- 3. the lowest 49 pairs of both pencils ---- */
  double const tol = 1e-10;                      /* the default, spelled out for the verdict below */
  double lam[2][NEV], res[2][NEV];
  BfhipEigsInfo info[2];
  void *dPhi = NULL;
  HIP(hipMalloc(&dPhi, n * NEV * 8));
  double *phi = malloc(n * NEV * sizeof *phi), *mphi = malloc(n * NEV * sizeof *mphi);
  if (!phi || !mphi) return 1;
  for (int pencil = 0; pencil < 2; ++pencil) {
    BfhipEigsOptions opt;
    memset(&opt, 0, sizeof opt);
    opt.structSize = sizeof opt;
    opt.seed = 2025;
    opt.tol = tol;
    opt.flags = BFHIP_EIGS_MASS_NORMALISED | (pencil ? BFHIP_EIGS_CONSISTENT_MASS : 0);
    memset(&info[pencil], 0, sizeof info[pencil]);
    info[pencil].structSize = sizeof info[pencil];
    CHECK(bfhipChebCovEigsDevice(cov, &opt, NEV, lam[pencil], res[pencil], dPhi, NEV, &info[pencil], NULL));
    printf("%s mass: lamMax %.4f; block of %u columns, %u outer iterations, largest degree %u, %llu columns of S and B applied, %.2f MB of workspace\n",
           pencil ? "consistent" : "lumped", info[pencil].lamMax, info[pencil].blockColumns, info[pencil].iterations, info[pencil].maxDegreeUsed,
           (unsigned long long)info[pencil].operatorColumns, (double)info[pencil].workspaceBytes / 1e6);
  }
  HIP(hipMemcpy(phi, dPhi, n * NEV * 8, 2));      /* the consistent pencil's Phi */

  printf("  j   l(l+1)   lumped lambda_j   consistent lambda_j   residual / lamMax (lumped, consistent)\n");
  int ok = fabs(lam[0][0]) <= tol * info[0].lamMax && fabs(lam[1][0]) <= tol * info[1].lamMax;
  for (int j = 0; j < NEV; ++j) {
    int const l = (int)floor(sqrt((double)j));                 /* l(l+1) has multiplicity 2l + 1: indices l^2 .. l^2 + 2l */
    printf("%3d   %6d   %15.10f   %19.10f   %10.3e   %10.3e\n", j, l * (l + 1), lam[0][j], lam[1][j], res[0][j] / info[0].lamMax, res[1][j] / info[1].lamMax);
    if (!(res[0][j] <= tol * info[0].lamMax) || !(res[1][j] <= tol * info[1].lamMax)) ok = 0;
  }

  /* ---- 4. Phi^T M Phi = I with the consistent M ---- */
  memset(mphi, 0, n * NEV * sizeof *mphi);
  for (uint64_t i = 0; i < n; ++i)
    for (uint64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
      for (int j = 0; j < NEV; ++j) mphi[i * NEV + j] += M[k] * phi[colind[k] * NEV + j];
  double worst = 0;
  for (int a = 0; a < NEV; ++a)
    for (int b = 0; b < NEV; ++b) {
      double g = 0;
      for (uint64_t i = 0; i < n; ++i) g += phi[i * NEV + a] * mphi[i * NEV + b];
      g = fabs(g - (a == b));
      if (g > worst) worst = g;
    }
  printf("||Phi^T M Phi - I||_max = %.3e with the consistent mass\n", worst);
  if (!(worst <= 1e-9)) ok = 0;

  hipFree(dPhi);
  bfhipChebCovFree(&cov);
  free(verts); free(faces); free(rowptr); free(colind); free(L); free(mass); free(M); free(phi); free(mphi);
  if (!ok) { fprintf(stderr, "a residual or lambda_0 is above %g x lamMax, or Phi^T M Phi is not I\n", tol); return 5; }
  return 0;
}
