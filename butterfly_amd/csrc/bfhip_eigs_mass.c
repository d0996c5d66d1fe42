/* bfhip_eigs_mass.c -- the consistent mass of the device eigensolver (bfhipTrimeshLboFemMass, bfhipChebCovSetConsistentMass,
 * include/bfhip.h).  Host side: the P1 mass on the pattern of bfhipTrimeshLboFem, the checks and the fold
 * B = D M D (bfEigsMassFold, which tests/native/fem_mass_check.c runs alone), and the upload next to S's values.  The
 * iteration is bfhip_eigs.c's; it reaches the launches of bfhip_eigs_mass.hip through the table stored here. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip_internal.h"
#include "../../include/bfhip.h"
#include "../../include/bfhip_abi.h"

/* position of column j in the sorted row [beg, end) of colind, or end when it is not there */
static uint64_t massRowFind(uint64_t const *colind, uint64_t beg, uint64_t end, uint64_t j) {
  uint64_t lo = beg, hi = end;
  while (lo < hi) {
    uint64_t const mid = lo + (hi - lo) / 2;
    if (colind[mid] < j) lo = mid + 1; else hi = mid;
  }
  return lo < end && colind[lo] == j ? lo : end;
}

int bfhipTrimeshLboFemMass(uint64_t numVerts, double const *verts, uint64_t numFaces, uint64_t const *faces, uint64_t const *rowptr,
                           uint64_t const *colind, double *Mdata) {
  if (!verts || (!faces && numFaces) || !rowptr || !colind || !Mdata) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (numVerts == 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "numVerts is zero");
  for (uint64_t f = 0; f < 3 * numFaces; ++f)
    if (faces[f] >= numVerts) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "face %llu has a vertex index >= numVerts", (unsigned long long)(f / 3));
  for (uint64_t f = 0; f < numFaces; ++f)
    if (faces[3 * f] == faces[3 * f + 1] || faces[3 * f] == faces[3 * f + 2] || faces[3 * f + 1] == faces[3 * f + 2])
      return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "face %llu is degenerate (a repeated vertex)", (unsigned long long)f);
  if (rowptr[0] != 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "rowptr[0] is not zero");
  for (uint64_t i = 0; i < numVerts; ++i)
    if (rowptr[i + 1] < rowptr[i]) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "rowptr is not monotone at row %llu", (unsigned long long)i);
  uint64_t const nnz = rowptr[numVerts];
  memset(Mdata, 0, nnz * sizeof *Mdata);
  for (uint64_t f = 0; f < numFaces; ++f) {
    uint64_t const *v = faces + 3 * f;
    double e[2][3];
    for (int d = 0; d < 3; ++d) { e[0][d] = verts[3 * v[2] + d] - verts[3 * v[1] + d]; e[1][d] = verts[3 * v[0] + d] - verts[3 * v[2] + d]; }
    /* twice the area: |e0 x e1|, the edges of bfhipTrimeshLboFem */
    double const nx = e[0][1] * e[1][2] - e[0][2] * e[1][1], ny = e[0][2] * e[1][0] - e[0][0] * e[1][2], nz = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    double const area2 = sqrt(nx * nx + ny * ny + nz * nz);
    if (!(area2 > 0) || !isfinite(area2)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "face %llu is degenerate (zero area)", (unsigned long long)f);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        uint64_t const i = v[a], j = v[b], k = massRowFind(colind, rowptr[i], rowptr[i + 1], j);
        if (k == rowptr[i + 1])
          return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "face %llu: entry (%llu, %llu) is not in the pattern (it is not this mesh's)", (unsigned long long)f,
                           (unsigned long long)i, (unsigned long long)j);
        Mdata[k] += a == b ? area2 / 12 : area2 / 24;          /* A / 6 and A / 12 */
      }
  }
  return 0;
}

/* The checks that need no device, then B[k] = (d[i] M[k]) d[col[k]] in the order S was folded.  With the P1 bounds asked for
 * (lo <= 0 && hi <= 0): every row sum of M within (nnz_i + 2) 2^-52 of 1 / d[i]^2 (the sum's own rounding and that of d), and a
 * positive diagonal entry in every row. */
int bfEigsMassFold(uint64_t n, uint64_t const *rowptr, uint32_t const *colind, double const *d, double const *Mdata, double *lo, double *hi, double *B) {
  if (!rowptr || !colind || !d || !Mdata || !lo || !hi || !B) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  uint64_t const nnz = rowptr[n];
  for (uint64_t k = 0; k < nnz; ++k)
    if (!isfinite(Mdata[k])) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "consistent mass: entry %llu is not finite", (unsigned long long)k);
  if (isnan(*lo) || isnan(*hi) || isinf(*lo) || isinf(*hi)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "consistent mass: a bound of the spectrum is not finite");
  if (*lo <= 0 && *hi <= 0) {
    for (uint64_t i = 0; i < n; ++i) {
      double sum = 0, mag = 0, diag = 0;
      for (uint64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        sum += Mdata[k]; mag += fabs(Mdata[k]);
        if (colind[k] == i) diag += Mdata[k];
      }
      double const lumped = 1 / (d[i] * d[i]);
      if (!(fabs(sum - lumped) <= (double)(rowptr[i + 1] - rowptr[i] + 2) * 0x1p-52 * (mag + lumped)))
        return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "consistent mass: the P1 bounds [1/4, 1] were asked for, but row %llu sums to %.17g and the lumped mass is %.17g; give [lo, hi]",
                         (unsigned long long)i, sum, lumped);
      if (!(diag > 0))
        return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "consistent mass: the P1 bounds [1/4, 1] were asked for, but the diagonal entry of row %llu is not positive", (unsigned long long)i);
    }
    *lo = 0.25; *hi = 1.0;
  } else if (!(*lo > 0) || !(*lo < *hi)) {
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "consistent mass: the bounds must satisfy 0 < lo < hi (or both <= 0 for the P1 bounds)");
  }
  for (uint64_t i = 0; i < n; ++i)
    for (uint64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) B[k] = (d[i] * Mdata[k]) * d[colind[k]];
  return 0;
}

static BfEigsMassOps const massOps = { bfdevEigsMassStep, bfdevEigsMassSolve, bfdevEigsCombine, bfdevEigsProjectMass, bfdevEigsDualProduct };

int bfhipChebCovSetConsistentMass(BfhipChebCov *c, double const *Mdata, double lo, double hi) {
  if (!c || !Mdata) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (!c->hRowptr || !c->hColind || !c->hD) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "consistent mass: the object holds no pattern");
  double *B = malloc((c->nnz ? c->nnz : 1) * sizeof *B);
  if (!B) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory");
  int rc = bfEigsMassFold(c->n, c->hRowptr, c->hColind, c->hD, Mdata, &lo, &hi, B);
  if (rc) { free(B); return rc; }
  BfDevScope ds = {0};
  if ((rc = bfDevEnter(&ds, c->device))) { free(B); return rc; }
  void *dNew = NULL;
  /* a second call: work enqueued earlier may still read the old array */
  if (!(rc = bfdevSync(NULL)) && !(rc = bfdevMalloc(&dNew, (c->nnz ? c->nnz : 1) * 8)) && c->nnz) rc = bfdevMemcpyH2D(dNew, B, c->nnz * 8);
  if (rc) {
    bfdevFree(dNew);
  } else {
    bfdevFree(c->dMass);
    c->dMass = dNew; c->massLo = lo; c->massHi = hi; c->massOps = &massOps;
  }
  bfDevLeave(&ds);
  free(B);
  return rc;
}
