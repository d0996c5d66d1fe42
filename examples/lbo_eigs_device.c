/* examples/lbo_eigs_device.c -- the lowest Laplace-Beltrami eigenpairs of a triangle mesh on the device, with no sparse
 * factorisation and no ARPACK: Chebyshev-filtered subspace iteration on S = M^-1/2 L M^-1/2 with the lumped mass
 * (bfhipChebCovEigsDevice), in plain C against include/bfhip.h.  The driver
 *   1. generates the latitude-longitude mesh of the unit sphere of examples/cheb_cov_device.c (24 rings of 48: 1154 vertices)
 *      and assembles its P1 stiffness matrix and lumped mass (bfhipTrimeshLboFem),
 *   2. uploads S (bfhipChebCovCreate; lamMax: the Gershgorin bound),
 *   3. computes the lowest 16 pairs, mass-normalised (Phi^T M Phi = I), and prints them beside the sphere's l(l+1), each
 *      2l + 1 times: the distance is the O(h^2) error of the P1 discretisation with lumped mass, printed and not judged,
 *   4. exits 0 when every residual is at or below tol x lamMax and lambda_0, the constant function's, is too.
 *
 *   gcc -O2 -std=gnu11 -Wall -Werror -Iinclude examples/lbo_eigs_device.c -Lbutterfly_amd/csrc -lbfhip -L/opt/rocm/lib -lamdhip64 -lm \
 *       -Wl,-rpath,$PWD/butterfly_amd/csrc -Wl,-rpath,/opt/rocm/lib -o /tmp/lbo_eigs_device
 *   /tmp/lbo_eigs_device [numLat = 24] [numLon = 48]
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

enum { NEV = 16 };

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

  /* ---- 2. the operator ---- */
  BfhipChebCov *cov = NULL;
  CHECK(bfhipChebCovCreate(-1, n, rowptr, colind, L, mass, 0.0, &cov));

  /* ---- 3. the lowest 16 pairs ---- */
  BfhipEigsOptions opt;
  memset(&opt, 0, sizeof opt);
  opt.structSize = sizeof opt;
  opt.seed = 2025;
  opt.flags = BFHIP_EIGS_MASS_NORMALISED;
  BfhipEigsInfo info;
  memset(&info, 0, sizeof info);
  info.structSize = sizeof info;
  double const tol = 1e-10;                      /* the default, spelled out for the verdict below */
  opt.tol = tol;
  double lam[NEV], res[NEV];
  void *dPhi = NULL;
  HIP(hipMalloc(&dPhi, n * NEV * 8));
  CHECK(bfhipChebCovEigsDevice(cov, &opt, NEV, lam, res, dPhi, NEV, &info, NULL));
  double *phi = malloc(n * NEV * sizeof *phi);
  if (!phi) return 1;
  HIP(hipMemcpy(phi, dPhi, n * NEV * 8, 2));
  printf("lamMax (Gershgorin) %.4f; block of %u columns, %u outer iterations, largest degree %u, %llu columns of S applied, %.2f MB of workspace\n",
         info.lamMax, info.blockColumns, info.iterations, info.maxDegreeUsed, (unsigned long long)info.operatorColumns, (double)info.workspaceBytes / 1e6);
  printf("  j   lambda_j          l(l+1)   difference   residual / lamMax   Phi_j^T M Phi_j\n");
  int ok = fabs(lam[0]) <= tol * info.lamMax;
  for (int j = 0; j < NEV; ++j) {
    int const l = (int)floor(sqrt((double)j));                 /* l(l+1) has multiplicity 2l + 1: indices l^2 .. l^2 + 2l */
    double mnorm = 0;
    for (uint64_t i = 0; i < n; ++i) mnorm += mass[i] * phi[i * NEV + j] * phi[i * NEV + j];
    printf("%3d   %14.10f   %6d   %10.3e   %10.3e          %.12f\n", j, lam[j], l * (l + 1), lam[j] - l * (l + 1), res[j] / info.lamMax, mnorm);
    if (!(res[j] <= tol * info.lamMax)) ok = 0;
  }

  hipFree(dPhi);
  bfhipChebCovFree(&cov);
  free(verts); free(faces); free(rowptr); free(colind); free(L); free(mass); free(phi);
  if (!ok) { fprintf(stderr, "a residual, or lambda_0, is above %g x lamMax\n", tol); return 5; }
  return 0;
}
