/* The host code of the consistent mass alone (butterfly_amd/csrc/bfhip_eigs_mass.c: bfhipTrimeshLboFemMass and bfEigsMassFold, the
 * checks and the fold of bfhipChebCovSetConsistentMass) on a jittered 6 x 7 grid mesh, every array allocated at its exact size.
 * Built by tests/test_consistent_eigs_cpu.py with -fsanitize=address,undefined together with bfhip_eigs_mass.c and bfhip_cheb.c
 * (for bfhipTrimeshLboFem, which makes the pattern) and run as a program of its own.  Checked: M is symmetric, its rows sum to
 * the lumped mass, its diagonal is half of it, its total is the area; the fold accepts the P1 bounds, returns [1/4, 1] and
 * B[i][i] = 1/2; every refusal refuses and leaves B untouched.  The device layer is never reached: stand-ins that abort. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int bfhipTrimeshLboFemCount(uint64_t numVerts, uint64_t numFaces, const uint64_t *faces, uint64_t *nnz);
int bfhipTrimeshLboFem(uint64_t numVerts, const double *verts, uint64_t numFaces, const uint64_t *faces, uint64_t *rowptr, uint64_t *colind,
                       double *Ldata, double *massLumped);
int bfhipTrimeshLboFemMass(uint64_t numVerts, const double *verts, uint64_t numFaces, const uint64_t *faces, const uint64_t *rowptr,
                           const uint64_t *colind, double *Mdata);
int bfEigsMassFold(uint64_t n, uint64_t const *rowptr, uint32_t const *colind, double const *d, double const *Mdata, double *lo, double *hi, double *B);

#define STUB(name) int name() { fprintf(stderr, "device layer reached: %s\n", #name); abort(); }
void bfdevFree(void *p) { if (p) abort(); }
int bfhipFail(int code, char const *fmt, ...) { (void)fmt; return code; }
STUB(bfdevChebStep) STUB(bfdevChebUnitPanel) STUB(bfdevCondPack) STUB(bfdevCondResidual) STUB(bfdevCondSolve) STUB(bfdevCovDrawFill)
STUB(bfdevCovMoments) STUB(bfdevEigsCombine) STUB(bfdevEigsDualProduct) STUB(bfdevEigsMassSolve) STUB(bfdevEigsMassStep) STUB(bfdevEigsProjectMass)
STUB(bfdevGetDevice)
STUB(bfdevLikGradContract) STUB(bfdevLikGradDot) STUB(bfdevLikGradM) STUB(bfdevLikGradSum) STUB(bfdevLikGradUnit) STUB(bfdevLikValue)
STUB(bfdevMalloc) STUB(bfdevMemcpyH2D) STUB(bfdevSetDevice) STUB(bfdevSync) STUB(condCheckObs) STUB(condLookupRange) STUB(condSetup)
void condRelease(void *c) { if (c) abort(); }

enum { NX = 6, NY = 7, NV = NX * NY, NF = 2 * (NX - 1) * (NY - 1) };

static int failures;
#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); ++failures; } } while (0)

int main(void) {
  double *verts = malloc(3 * NV * sizeof *verts);
  uint64_t *faces = malloc(3 * NF * sizeof *faces);
  uint64_t state = 12345;
  for (int i = 0; i < NX; ++i)
    for (int j = 0; j < NY; ++j) {
      double r[3];
      for (int k = 0; k < 3; ++k) { state = state * 6364136223846793005ull + 1442695040888963407ull; r[k] = (double)(state >> 11) * 0x1p-53 - 0.5; }
      double *v = verts + 3 * (i * NY + j);
      v[0] = i + 0.25 * r[0]; v[1] = j + 0.25 * r[1]; v[2] = 0.3 * sin(0.9 * i) * cos(0.7 * j) + 0.05 * r[2];
    }
  uint64_t nf = 0;
  for (uint64_t i = 0; i + 1 < NX; ++i)
    for (uint64_t j = 0; j + 1 < NY; ++j) {
      uint64_t const a = i * NY + j, b = (i + 1) * NY + j, c = (i + 1) * NY + j + 1, d = i * NY + j + 1;
      uint64_t const t[6] = { a, b, c, a, c, d };
      memcpy(faces + 3 * nf, t, sizeof t);
      nf += 2;
    }
  uint64_t nnz = 0;
  if (bfhipTrimeshLboFemCount(NV, NF, faces, &nnz)) { printf("count failed\n"); return 1; }
  uint64_t *rowptr = malloc((NV + 1) * sizeof *rowptr), *colind = malloc(nnz * sizeof *colind);
  uint32_t *col32 = malloc(nnz * sizeof *col32);
  double *L = malloc(nnz * sizeof *L), *M = malloc(nnz * sizeof *M), *B = malloc(nnz * sizeof *B), *lumped = malloc(NV * sizeof *lumped);
  double *d = malloc(NV * sizeof *d), *bad = malloc(nnz * sizeof *bad);
  if (bfhipTrimeshLboFem(NV, verts, NF, faces, rowptr, colind, L, lumped)) { printf("assembly failed\n"); return 1; }
  if (bfhipTrimeshLboFemMass(NV, verts, NF, faces, rowptr, colind, M)) { printf("mass assembly failed\n"); return 1; }
  double const u = 0x1p-53;
  double total = 0, area = 0;
  for (uint64_t i = 0; i < NV; ++i) {
    double sum = 0, diag = 0;
    for (uint64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      uint64_t const j = colind[k];
      col32[k] = (uint32_t)j;
      sum += M[k];
      if (j == i) diag = M[k];
      double mirror = NAN;
      for (uint64_t q = rowptr[j]; q < rowptr[j + 1]; ++q)
        if (colind[q] == i) mirror = M[q];
      CHECK(fabs(mirror - M[k]) <= 4 * u * fabs(M[k]), "M is not symmetric at (%llu, %llu)", (unsigned long long)i, (unsigned long long)j);
      CHECK(M[k] > 0, "M has a non-positive entry at (%llu, %llu)", (unsigned long long)i, (unsigned long long)j);
    }
    CHECK(fabs(sum - lumped[i]) <= 32 * u * lumped[i], "row %llu sums to %.17g, lumped %.17g", (unsigned long long)i, sum, lumped[i]);
    CHECK(fabs(diag - lumped[i] / 2) <= 32 * u * lumped[i], "diagonal %llu is %.17g, lumped / 2 %.17g", (unsigned long long)i, diag, lumped[i] / 2);
    total += sum; area += lumped[i];
    d[i] = 1 / sqrt(lumped[i]);
  }
  CHECK(fabs(total - area) <= 64 * u * area, "the total of M is %.17g, the area %.17g", total, area);

  /* the fold with the P1 bounds */
  double lo = 0, hi = 0;
  int rc = bfEigsMassFold(NV, rowptr, col32, d, M, &lo, &hi, B);
  CHECK(rc == 0 && lo == 0.25 && hi == 1.0, "the fold refused the P1 mass or gave other bounds: rc %d [%g, %g]", rc, lo, hi);
  for (uint64_t i = 0; i < NV; ++i)
    for (uint64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      double const want = (d[i] * M[k]) * d[colind[k]];
      CHECK(B[k] == want, "B[%llu] is not (d_i M) d_j", (unsigned long long)k);
      if (colind[k] == i) CHECK(fabs(B[k] - 0.5) <= 16 * u, "B[%llu][%llu] = %.17g, not 1/2", (unsigned long long)i, (unsigned long long)i, B[k]);
    }
  /* explicit bounds are taken as given */
  lo = 0.2; hi = 1.5;
  rc = bfEigsMassFold(NV, rowptr, col32, d, M, &lo, &hi, B);
  CHECK(rc == 0 && lo == 0.2 && hi == 1.5, "explicit bounds: rc %d [%g, %g]", rc, lo, hi);

  /* the refusals: B must stay as it is */
  for (uint64_t k = 0; k < nnz; ++k) B[k] = -77.0;
  struct { char const *what; int entry; double value, lo, hi; } const cases[] = {
    { "a NaN entry", 5, NAN, 0, 0 }, { "an infinite entry", (int)nnz - 1, INFINITY, 0.25, 1 }, { "lo == hi", -1, 0, 0.5, 0.5 }, { "lo > hi", -1, 0, 1, 0.25 },
    { "lo <= 0 with hi > 0", -1, 0, 0, 1 }, { "a NaN bound", -1, 0, NAN, 1 }, { "an infinite bound", -1, 0, 0.25, INFINITY },
    { "a row sum that is not the lumped mass", 3, 1.0, 0, 0 }, { "a negative diagonal", -2, 0, 0, 0 },
  };
  for (size_t t = 0; t < sizeof cases / sizeof *cases; ++t) {
    memcpy(bad, M, nnz * sizeof *bad);
    if (cases[t].entry >= 0) bad[cases[t].entry] = cases[t].value;
    if (cases[t].entry == -2) {
      /* row 0: the diagonal negated, the difference moved to a neighbour, so the row still sums to the lumped mass */
      uint64_t kd = rowptr[0], ko = rowptr[0];
      for (uint64_t k = rowptr[0]; k < rowptr[1]; ++k) { if (colind[k] == 0) kd = k; else ko = k; }
      bad[ko] += 2 * bad[kd]; bad[kd] = -bad[kd];
    }
    lo = cases[t].lo; hi = cases[t].hi;
    rc = bfEigsMassFold(NV, rowptr, col32, d, bad, &lo, &hi, B);
    CHECK(rc == 1, "%s was not refused (rc %d)", cases[t].what, rc);
    for (uint64_t k = 0; k < nnz; ++k)
      if (B[k] != -77.0) { CHECK(0, "%s: B was written", cases[t].what); break; }
  }
  lo = hi = 0;
  CHECK(bfEigsMassFold(NV, rowptr, col32, d, NULL, &lo, &hi, B) == 1 && bfEigsMassFold(NV, rowptr, col32, NULL, M, &lo, &hi, B) == 1, "NULL was not refused");
  /* the assembler on a pattern that is not this mesh's: a diagonal-only pattern */
  uint64_t *rp1 = malloc((NV + 1) * sizeof *rp1), *ci1 = malloc(NV * sizeof *ci1);
  double *m1 = malloc(NV * sizeof *m1);
  for (uint64_t i = 0; i <= NV; ++i) rp1[i] = i;
  for (uint64_t i = 0; i < NV; ++i) ci1[i] = i;
  CHECK(bfhipTrimeshLboFemMass(NV, verts, NF, faces, rp1, ci1, m1) == 1, "a foreign pattern was not refused");
  faces[4] = NV;
  CHECK(bfhipTrimeshLboFemMass(NV, verts, NF, faces, rowptr, colind, M) == 1, "a face index >= numVerts was not refused");
  CHECK(bfhipTrimeshLboFemMass(0, verts, NF, faces, rowptr, colind, M) == 1 && bfhipTrimeshLboFemMass(NV, NULL, NF, faces, rowptr, colind, M) == 1,
        "numVerts == 0 or NULL was not refused");

  free(verts); free(faces); free(rowptr); free(colind); free(col32); free(L); free(M); free(B); free(lumped); free(d); free(bad);
  free(rp1); free(ci1); free(m1);
  if (failures) { printf("FAILED\n"); return 1; }
  printf("ok\n");
  return 0;
}
