/* bfhip_cheb.c -- matrix-free Chebyshev covariance on a sparse FEM operator (include/bfhip.h, "matrix-free Chebyshev
 * covariance"): the second route of the reference's covariance examples (examples/covariance/cheb_cov.c), which needs no
 * eigenpairs and no butterfly.  Host side: the Chebyshev fit and evaluation, the P1 assembly of a triangle mesh, the
 * object (S = D L D in CSR on the device, folded here) and the drivers of Clenshaw's recurrence, one bfdevChebStep
 * (bfhip_cheb.hip) per degree.  The draw and the moments reuse the kernels of bfhip_cov.hip.  Then the Chebyshev backend
 * of conditioning on observations (bfhipChebCovCondCreate; the object is bfhip_cond.c's) and, last in
 * the file, the likelihood's gradient in the density's parameters on such an object (bfhipChebCovCondLogLikGradDevice;
 * kernels: bfhip_likgrad.hip). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip_internal.h"
#include "bfhip_cond.h"
#include "../../include/bfhip.h"
#include "../../include/bfhip_abi.h"

/* ------------------------------------------------------------------------
 * Chebyshev interpolation (host)
 * ---------------------------------------------------------------------- */
int bfhipChebFit(size_t order, double a, double b, double (*f)(double, void *), void *ctx, double *coef) {
  if (!f || !coef) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (order == 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "order is zero");
  if (!isfinite(a) || !isfinite(b) || a == b) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "the interval [a, b] must be finite and not empty");
  double *x = malloc(2 * order * sizeof *x);
  if (!x) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory");
  double *y = x + order;
  for (size_t j = 0; j < order; ++j) {
    x[j] = sin(M_PI * ((double)(2 * j + 1) - (double)order) / (2.0 * (double)order));
    y[j] = f((b - a) * (x[j] + 1) / 2 + a, ctx);
  }
  /* c_k = (2 / order) sum_j T_k(x_j) y_j, T_k(x_j) by the three-term recurrence per node (c_0 with 1 / order) */
  for (size_t k = 0; k < order; ++k) coef[k] = 0;
  for (size_t j = 0; j < order; ++j) {
    double t0 = 1, t1 = x[j];
    for (size_t k = 0; k < order; ++k) {
      coef[k] += t0 * y[j];
      double const t2 = 2 * x[j] * t1 - t0;
      t0 = t1; t1 = t2;
    }
  }
  coef[0] /= (double)order;
  for (size_t k = 1; k < order; ++k) coef[k] *= 2.0 / (double)order;
  free(x);
  return 0;
}

double bfhipChebEval(size_t order, double a, double b, double const *coef, double x) {
  if (!coef || order == 0) return NAN;
  double const t = (2 * x - a - b) / (b - a);
  double b1 = 0, b2 = 0;
  for (size_t k = order - 1; k >= 1; --k) {
    double const bk = coef[k] + 2 * t * b1 - b2;
    b2 = b1; b1 = bk;
  }
  return coef[0] + t * b1 - b2;
}

/* ------------------------------------------------------------------------
 * P1 assembly of a triangle mesh (host)
 * ---------------------------------------------------------------------- */
static int cmpU64(void const *a, void const *b) {
  uint64_t const x = *(uint64_t const *)a, y = *(uint64_t const *)b;
  return x < y ? -1 : x > y;
}

/* rowptr [numVerts + 1] and, with colind != NULL, the sorted rows (neighbours and the vertex itself).  A first pass counts
 * 1 + 2 x (faces at the vertex) slots per row, which holds every neighbour twice at most; the rows are then sorted,
 * made unique and compacted in place. */
static int trimeshRows(uint64_t numVerts, uint64_t numFaces, uint64_t const *faces, uint64_t *rowptr, uint64_t **colindOut) {
  for (uint64_t f = 0; f < 3 * numFaces; ++f)
    if (faces[f] >= numVerts) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "face %llu has a vertex index >= numVerts", (unsigned long long)(f / 3));
  for (uint64_t f = 0; f < numFaces; ++f)
    if (faces[3 * f] == faces[3 * f + 1] || faces[3 * f] == faces[3 * f + 2] || faces[3 * f + 1] == faces[3 * f + 2])
      return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "face %llu is degenerate (a repeated vertex)", (unsigned long long)f);
  uint64_t *start = calloc(numVerts + 1, sizeof *start);
  if (!start) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory");
  for (uint64_t i = 0; i < numVerts; ++i) start[i + 1] = 1;
  for (uint64_t f = 0; f < 3 * numFaces; ++f) start[faces[f] + 1] += 2;
  for (uint64_t i = 0; i < numVerts; ++i) start[i + 1] += start[i];
  uint64_t *slots = malloc((start[numVerts] ? start[numVerts] : 1) * sizeof *slots), *fill = malloc((numVerts ? numVerts : 1) * sizeof *fill);
  if (!slots || !fill) { free(start); free(slots); free(fill); return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory"); }
  for (uint64_t i = 0; i < numVerts; ++i) { slots[start[i]] = i; fill[i] = start[i] + 1; }
  for (uint64_t f = 0; f < numFaces; ++f)
    for (int k = 0; k < 3; ++k) {
      uint64_t const i = faces[3 * f + k];
      slots[fill[i]++] = faces[3 * f + (k + 1) % 3];
      slots[fill[i]++] = faces[3 * f + (k + 2) % 3];
    }
  uint64_t out = 0;
  rowptr[0] = 0;
  for (uint64_t i = 0; i < numVerts; ++i) {
    uint64_t const b = start[i], e = start[i + 1];
    qsort(slots + b, e - b, sizeof *slots, cmpU64);
    for (uint64_t k = b; k < e; ++k)
      if (k == b || slots[k] != slots[k - 1]) slots[out++] = slots[k];      /* out <= k: compaction in place */
    rowptr[i + 1] = out;
  }
  free(start); free(fill);
  if (colindOut) *colindOut = slots; else free(slots);
  return 0;
}

int bfhipTrimeshLboFemCount(uint64_t numVerts, uint64_t numFaces, uint64_t const *faces, uint64_t *nnz) {
  if (!nnz || (!faces && numFaces)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (numVerts == 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "numVerts is zero");
  uint64_t *rowptr = malloc((numVerts + 1) * sizeof *rowptr);
  if (!rowptr) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory");
  int const rc = trimeshRows(numVerts, numFaces, faces, rowptr, NULL);
  if (!rc) *nnz = rowptr[numVerts];
  free(rowptr);
  return rc;
}

/* position of column j in the sorted row [beg, end) of colind (it is there: the rows were made from the faces) */
static uint64_t rowFind(uint64_t const *colind, uint64_t beg, uint64_t end, uint64_t j) {
  while (end - beg > 1) {
    uint64_t const mid = beg + (end - beg) / 2;
    if (colind[mid] <= j) beg = mid; else end = mid;
  }
  return beg;
}

int bfhipTrimeshLboFem(uint64_t numVerts, double const *verts, uint64_t numFaces, uint64_t const *faces, uint64_t *rowptr, uint64_t *colind,
                       double *Ldata, double *massLumped) {
  if (!verts || (!faces && numFaces) || !rowptr || !colind || !Ldata) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (numVerts == 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "numVerts is zero");
  uint64_t *cols = NULL;
  int rc = trimeshRows(numVerts, numFaces, faces, rowptr, &cols);
  if (rc) return rc;
  uint64_t const nnz = rowptr[numVerts];
  memcpy(colind, cols, nnz * sizeof *colind);
  free(cols);
  memset(Ldata, 0, nnz * sizeof *Ldata);
  if (massLumped) memset(massLumped, 0, numVerts * sizeof *massLumped);
  for (uint64_t f = 0; f < numFaces; ++f) {
    uint64_t const *v = faces + 3 * f;
    double e[3][3];                    /* e[k] = the edge opposite corner k: from v[k + 1] to v[k + 2] */
    for (int k = 0; k < 3; ++k)
      for (int d = 0; d < 3; ++d) e[k][d] = verts[3 * v[(k + 2) % 3] + d] - verts[3 * v[(k + 1) % 3] + d];
    /* twice the area: |e0 x e1| */
    double const nx = e[0][1] * e[1][2] - e[0][2] * e[1][1], ny = e[0][2] * e[1][0] - e[0][0] * e[1][2], nz = e[0][0] * e[1][1] - e[0][1] * e[1][0];
    double const area2 = sqrt(nx * nx + ny * ny + nz * nz);
    if (!(area2 > 0) || !isfinite(area2)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "face %llu is degenerate (zero area)", (unsigned long long)f);
    for (int k = 0; k < 3; ++k) {
      /* the angle at corner k lies between -e[k + 1] and e[k + 2]; its cotangent weighs the opposite edge (v[k + 1], v[k + 2]) */
      double const *p = e[(k + 1) % 3], *r = e[(k + 2) % 3];
      double const w = -0.5 * (p[0] * r[0] + p[1] * r[1] + p[2] * r[2]) / area2;       /* cot / 2 */
      uint64_t const i = v[(k + 1) % 3], j = v[(k + 2) % 3];
      Ldata[rowFind(colind, rowptr[i], rowptr[i + 1], j)] -= w;
      Ldata[rowFind(colind, rowptr[j], rowptr[j + 1], i)] -= w;
      Ldata[rowFind(colind, rowptr[i], rowptr[i + 1], i)] += w;
      Ldata[rowFind(colind, rowptr[j], rowptr[j + 1], j)] += w;
      if (massLumped) massLumped[v[k]] += area2 / 6;
    }
  }
  return 0;
}

/* ------------------------------------------------------------------------
 * the object
 * ---------------------------------------------------------------------- */
/* struct BfhipChebCov: bfhip_internal.h (bfhip_eigs.c reads it too) */
void bfhipChebCovFree(BfhipChebCov **pc) {
  if (!pc || !*pc) return;
  BfhipChebCov *c = *pc;
  if (c->dRowptr || c->dWork) {
    BfDevScope ds;
    bfDevEnter(&ds, c->device);      /* a release cannot fail: errors are ignored on purpose */
    bfdevSync(NULL);
    bfdevFree(c->dRowptr); bfdevFree(c->dColind); bfdevFree(c->dVal); bfdevFree(c->dD); bfdevFree(c->dWork); bfdevFree(c->dMass);
    bfDevLeave(&ds);
  }
  free(c->hRowptr); free(c->hColind); free(c->hD);
  free(c->coef);
  free(c);
  *pc = NULL;
}

int bfhipChebCovCreate(int device, uint64_t n, uint64_t const *rowptr, uint64_t const *colind, double const *data, double const *massLumped,
                       double lamMax, BfhipChebCov **out) {
  if (!out) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  *out = NULL;
  if (!rowptr || !colind || !data) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (n == 0 || n >= (1ull << 32)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "n out of range (1 .. 2^32 - 1)");
  if (rowptr[0] != 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "rowptr[0] is not zero");
  for (uint64_t i = 0; i < n; ++i)
    if (rowptr[i + 1] < rowptr[i]) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "rowptr is not monotone at row %llu", (unsigned long long)i);
  uint64_t const nnz = rowptr[n];
  for (uint64_t k = 0; k < nnz; ++k)
    if (colind[k] >= n) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "column index %llu of entry %llu is >= n", (unsigned long long)colind[k], (unsigned long long)k);
  if (massLumped)
    for (uint64_t i = 0; i < n; ++i)
      if (!isfinite(massLumped[i]) || !(massLumped[i] > 0)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "massLumped[%llu] is not a positive finite number", (unsigned long long)i);
  if (!isfinite(lamMax)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "lamMax is not finite");

  int rc = 0;
  BfDevScope ds = {0};
  BfhipChebCov *c = calloc(1, sizeof *c);
  double *d = malloc(n * sizeof *d), *val = malloc((nnz ? nnz : 1) * sizeof *val);
  uint32_t *col32 = malloc((nnz ? nnz : 1) * sizeof *col32);
  uint64_t *rows = malloc((n + 1) * sizeof *rows);
  if (!c || !d || !val || !col32 || !rows) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory"); goto fail; }
  memcpy(rows, rowptr, (n + 1) * sizeof *rows);
  for (uint64_t i = 0; i < n; ++i) d[i] = massLumped ? 1 / sqrt(massLumped[i]) : 1.0;
  double gersh = 0;
  for (uint64_t i = 0; i < n; ++i) {
    double rowSum = 0;
    for (uint64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
      val[k] = (d[i] * data[k]) * d[colind[k]];
      col32[k] = (uint32_t)colind[k];
      rowSum += fabs(val[k]);
    }
    if (rowSum > gersh || rowSum != rowSum) gersh = rowSum;
  }
  if (lamMax <= 0) lamMax = gersh;
  if (!(lamMax > 0) || !isfinite(lamMax)) { rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "the Gershgorin bound of S is %g: no interval [0, lamMax]", lamMax); goto fail; }
  c->n = n; c->nnz = nnz; c->lamMax = lamMax;

  if ((rc = bfDevEnter(&ds, device))) goto fail;
  if (device < 0) bfdevGetDevice(&device);      /* -1: the object lives on the current device */
  c->device = device;
  if ((rc = bfdevMalloc(&c->dRowptr, (n + 1) * 8)) || (rc = bfdevMalloc(&c->dColind, (nnz ? nnz : 1) * 4)) ||
      (rc = bfdevMalloc(&c->dVal, (nnz ? nnz : 1) * 8)) || (rc = bfdevMalloc(&c->dD, n * 8))) goto fail;
  if ((rc = bfdevMemcpyH2D(c->dRowptr, rowptr, (n + 1) * 8)) || (nnz && (rc = bfdevMemcpyH2D(c->dColind, col32, nnz * 4))) ||
      (nnz && (rc = bfdevMemcpyH2D(c->dVal, val, nnz * 8))) || (rc = bfdevMemcpyH2D(c->dD, d, n * 8))) goto fail;
  c->deviceBytes = (n + 1) * 8 + nnz * 4 + nnz * 8 + n * 8;
  /* the pattern and d stay on the host for bfhipChebCovSetConsistentMass, whose checks and fold run before the device is touched */
  c->hRowptr = rows; c->hColind = col32; c->hD = d;
  rows = NULL; col32 = NULL; d = NULL;
  *out = c; c = NULL;
fail:
  free(d); free(val); free(col32); free(rows);
  if (c) bfhipChebCovFree(&c);             /* touches the device only for what was allocated there */
  bfDevLeave(&ds);
  return rc;
}

int bfhipChebCovSetCoefficients(BfhipChebCov *c, double const *coef, size_t order) {
  if (!c || !coef) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (order == 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "order is zero");
  for (size_t k = 0; k < order; ++k)
    if (!isfinite(coef[k])) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "coefficient %zu is not finite", k);
  double *copy = malloc(order * sizeof *copy);
  if (!copy) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory");
  memcpy(copy, coef, order * sizeof *copy);
  free(c->coef);
  c->coef = copy; c->order = order;
  ++c->generation;
  return 0;
}

int bfhipChebCovGetInfo(BfhipChebCov const *c, BfhipChebCovInfo *info) {
  if (!c || !info) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (info->structSize != sizeof *info) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "structSize is not sizeof(BfhipChebCovInfo)");
  info->reserved = 0;
  info->n = c->n; info->nnz = c->nnz; info->lamMax = c->lamMax; info->order = c->order;
  info->deviceBytes = c->deviceBytes; info->workspaceBytes = c->workBytes;
  info->errorEstimate = c->order ? fabs(c->coef[c->order - 1]) : 0;
  return 0;
}

/* ------------------------------------------------------------------------
 * the recurrence
 * ---------------------------------------------------------------------- */
/* `blocks` blocks of n x q doubles, packed at q columns: block k starts at k * n * q.  Growing is not stream-ordered (work
 * enqueued earlier may still read the old blocks): drain first, as the covariance scratch of the operators does */
static int chebWork(BfhipChebCov *c, uint32_t blocks, size_t q, void *stream) {
  uint64_t const need = (uint64_t)blocks * c->n * q * 8;
  if (c->dWork && c->workBytes >= need) return 0;
  int rc;
  if (c->dWork) {
    if ((rc = bfdevSync(stream))) return rc;
    bfdevFree(c->dWork); c->dWork = NULL; c->workBytes = 0;
  }
  if ((rc = bfdevMalloc(&c->dWork, need))) return rc;
  c->workBytes = need;
  return 0;
}
static double *chebBlock(BfhipChebCov const *c, uint32_t k, size_t q) { return (double *)c->dWork + (uint64_t)k * c->n * q; }

/* out = [outScale] r(S) ([wScale] w) by Clenshaw for the polynomial r with coefficients coef[0 .. order - 1] on [0, lamMax],
 * b_k written over b_{k+2} in blocks 0 and 1 of the workspace.  out == NULL: the result takes the place b_0 would (a workspace
 * block); *where receives it either way */
static int chebMulCoef(BfhipChebCov *c, double const *coef, size_t order, double const *w, int scaleIn, int scaleOut, size_t q, double *out,
                       double **where, void *stream) {
  BfChebStep s = { c->dRowptr, c->dColind, c->dVal, c->n, (uint32_t)q, w, scaleIn ? c->dD : NULL, NULL, NULL, NULL, NULL, 0, 0, 0 };
  double *P[2] = { chebBlock(c, 0, q), chebBlock(c, 1, q) };
  double *b1 = NULL, *b2 = NULL;
  int rc;
  for (size_t k = order; k-- > 0;) {
    double *dst = b2 ? b2 : b1 == P[0] ? P[1] : P[0];
    if (k == 0 && out) dst = out;
    s.b1 = b1; s.b2 = b2; s.out = dst; s.ck = coef[k];
    s.alpha = (k ? 4.0 : 2.0) / c->lamMax; s.beta = k ? -2.0 : -1.0;
    s.outScale = k == 0 && scaleOut ? c->dD : NULL;
    if ((rc = bfdevChebStep(&s, stream))) return rc;
    b2 = b1; b1 = dst;
  }
  if (where) *where = b1;
  return 0;
}

/* the object's own polynomial p */
static int chebMul(BfhipChebCov *c, double const *w, int scaleIn, int scaleOut, size_t q, double *out, double **where, void *stream) {
  return chebMulCoef(c, c->coef, c->order, w, scaleIn, scaleOut, q, out, where, stream);
}

static int chebBlockCheck(BfhipChebCov const *c, void const *in, void const *out, size_t q) {
  if (!c || !in || !out) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (q == 0 || q > 0xffffu) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "q out of range");
  if (in == out) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "in-place use: the input block is read at every step");
  if (!c->order) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "no coefficients: call bfhipChebCovSetCoefficients first");
  return 0;
}

static int chebProduct(BfhipChebCov *c, double const *in, int scaleIn, int scaleOut, size_t q, double *out, void *stream) {
  int rc;
  BfDevScope ds;
  if ((rc = bfDevEnter(&ds, c->device))) return rc;
  if (!(rc = chebWork(c, 2, q, stream))) rc = chebMul(c, in, scaleIn, scaleOut, q, out, NULL, stream);
  bfDevLeave(&ds);
  return rc;
}

int bfhipChebCovApplyBlockDevice(BfhipChebCov *c, double const *dW, size_t q, double *dX, void *stream) {
  int const rc = chebBlockCheck(c, dW, dX, q);
  return rc ? rc : chebProduct(c, dW, 0, 0, q, dX, stream);
}

int bfhipChebCovSampleBlockDevice(BfhipChebCov *c, double const *dW, size_t q, double *dZ, void *stream) {
  int const rc = chebBlockCheck(c, dW, dZ, q);
  return rc ? rc : chebProduct(c, dW, 0, 1, q, dZ, stream);
}

int bfhipChebCovMatvecBlockDevice(BfhipChebCov *c, double const *dV, size_t q, double *dZ, void *stream) {
  int rc;
  BfDevScope ds;
  if ((rc = chebBlockCheck(c, dV, dZ, q)) || (rc = bfDevEnter(&ds, c->device))) return rc;
  if ((rc = chebWork(c, 3, q, stream))) goto out;
  double *t = chebBlock(c, 2, q);
  if ((rc = chebMul(c, dV, 1, 0, q, t, NULL, stream))) goto out;          /* T = p(S) D V */
  rc = chebMul(c, t, 0, 1, q, dZ, NULL, stream);                          /* Z = D p(S) T */
out:
  bfDevLeave(&ds);
  return rc;
}

int bfhipChebCovDrawDevice(BfhipChebCov *c, uint64_t seed, uint64_t firstSample, size_t q, double *dZ, void *stream) {
  int rc;
  BfDevScope ds;
  if ((rc = chebBlockCheck(c, c, dZ, q)) || (rc = bfDevEnter(&ds, c->device))) return rc;
  if ((rc = chebWork(c, 3, q, stream))) goto out;
  double *w = chebBlock(c, 2, q);
  if ((rc = bfdevCovDrawFill(w, NULL, c->n, (uint32_t)q, BFHIP_F64, seed, firstSample, stream))) goto out;
  rc = chebMul(c, w, 0, 1, q, dZ, NULL, stream);
out:
  bfDevLeave(&ds);
  return rc;
}

int bfhipChebCovMomentsDevice(BfhipChebCov *c, uint64_t seed, uint64_t firstSample, uint64_t numSamples, uint32_t batch, double *dSum,
                              double *dSumSq, void *stream) {
  int rc;
  BfDevScope ds;
  if (!c) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (!dSum && !dSumSq) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "both moment outputs are NULL");
  if (batch > 64) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "batch out of range (at most 64)");
  if (numSamples == 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "numSamples is zero");
  if (!c->order) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "no coefficients: call bfhipChebCovSetCoefficients first");
  if (!batch) batch = 64;
  if (batch > numSamples) batch = (uint32_t)numSamples;
  if ((rc = bfDevEnter(&ds, c->device))) return rc;
  if ((rc = chebWork(c, 3, batch, stream))) goto out;
  for (uint64_t s0 = 0; s0 < numSamples; s0 += batch) {
    uint32_t const b = (uint32_t)(numSamples - s0 < batch ? numSamples - s0 : batch);
    /* a batch of b columns is packed at b columns; Z is never written: the last step leaves it in a workspace block */
    double *w = chebBlock(c, 2, b), *z = NULL;
    if ((rc = bfdevCovDrawFill(w, NULL, c->n, b, BFHIP_F64, seed, firstSample + s0, stream))) goto out;
    if ((rc = chebMul(c, w, 0, 1, b, NULL, &z, stream))) goto out;
    if ((rc = bfdevCovMoments(z, c->n, b, BFHIP_F64, NULL, dSum, dSumSq, stream))) goto out;
  }
out:
  bfDevLeave(&ds);
  return rc;
}

/* ------------------------------------------------------------------------
 * conditioning on observations: the backend of struct BfhipCovCond for B = D p(S)
 * ---------------------------------------------------------------------- */
/* The rows of B at the observed vertices, transposed, are X = p(S) D E_obs: unit columns scaled by d in the object's own block
 * (it is read at every step), one recurrence without the output scaling, the result packed into its columns of Bt. */
static int chebCondPanel(BfhipCovCond *c, uint64_t const *dRows, uint32_t p, double *Bt, uint32_t ld, uint32_t c0, void *stream) {
  BfhipChebCov *cheb = c->cheb;
  double *x = NULL;
  int rc;
  if ((rc = chebWork(cheb, 2, p, stream)) || (rc = bfdevChebUnitPanel(c->dWp, cheb->n, p, dRows, cheb->dD, stream)) ||
      (rc = chebMul(cheb, c->dWp, 0, 0, p, NULL, &x, stream))) return rc;
  return bfdevCondPack(Bt, cheb->n, ld, c0, x, p, NULL, BFHIP_F64, stream);
}

static void *chebCondWprime(BfhipCovCond *c) { return c->dWp; }

/* Z = D p(S) W': one polynomial application, as a prior batch costs; there is no permutation, so `scatter` changes nothing */
static int chebCondField(BfhipCovCond *c, uint32_t b, int scatter, void *dZ, void **packed, void *stream) {
  BfhipChebCov *cheb = c->cheb;
  double *z = NULL;
  int rc;
  (void)scatter;
  if ((rc = chebWork(cheb, 2, b, stream)) || (rc = chebMul(cheb, c->dWp, 0, 1, b, dZ, &z, stream))) return rc;
  if (packed) *packed = z;
  return 0;
}

static int chebCondLive(BfhipCovCond const *c) {
  if (c->cheb->generation == c->chebGeneration) return 0;
  return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "stale conditioning object: bfhipChebCovSetCoefficients was called after it was made (its rows hold the earlier polynomial); create a new one");
}

int bfhipChebCovCondCreate(BfhipChebCov *cheb, uint64_t const *obs, size_t numObs, double const *noiseVar, BfhipCovCond **out, void *stream) {
  if (out) *out = NULL;
  if (!cheb || !obs || !out) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (numObs == 0 || numObs > BFHIP_COND_MAX_OBS) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "numObs out of range (1 .. %u)", BFHIP_COND_MAX_OBS);
  uint32_t const k = (uint32_t)numObs;
  BfCondKey *keys = NULL;
  BfDevScope ds = {0};
  int rc = condCheckObs(obs, k, noiseVar, &keys);      /* nothing is read through cheb before the checks that need the arguments alone */
  if (rc) return rc;
  uint64_t const n = cheb->n;
  rc = condLookupRange(keys, k, "observed", n);
  if (!rc && !cheb->order) rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "no coefficients: call bfhipChebCovSetCoefficients first");
  if (!rc && !bfdevCondFits(n)) rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "conditioning: %llu vertices are more than the contractions' grids take (%llu)",
                                               (unsigned long long)n, (unsigned long long)BF_COND_MAX_COLS);
  if (rc) { free(keys); return rc; }

  BfhipCovCond *c = calloc(1, sizeof *c);
  if (!c) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory"); goto fail; }
  c->be = (BfCondBackend){ n, n, BFHIP_F64, sizeof(double), 0, chebCondPanel, chebCondWprime, chebCondField, chebCondLive };
  c->cheb = cheb; c->chebGeneration = cheb->generation; c->k = k; c->device = cheb->device;
  if (!(c->hObs = malloc(k * sizeof *c->hObs))) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory"); goto fail; }
  memcpy(c->hObs, obs, k * sizeof *c->hObs);         /* the gradient in the density's parameters makes the unit panels again */
  if ((rc = bfDevEnter(&ds, cheb->device))) goto fail;

  /* ---- the recurrence's two blocks at 64 columns in cheb's workspace, and the object's own W' block ---- */
  size_t const bytesWp = n * BF_COND_MAX_RHS * sizeof(double);
  if ((rc = bfdevSync(stream)) || (rc = chebWork(cheb, 2, BF_COND_MAX_RHS, stream)) || (rc = bfdevMalloc(&c->dWp, bytesWp))) goto fail;
  c->info.factorBytes = bytesWp;
  if ((rc = condSetup(c, keys, obs, noiseVar, stream))) goto fail;
  *out = c; c = NULL;
fail:
  condRelease(c);
  free(keys);
  bfDevLeave(&ds);
  return rc;
}

/* ------------------------------------------------------------------------
 * the likelihood's gradient in the density's parameters
 * ---------------------------------------------------------------------- */
/* profile switch of tools/cheb_gradient_rate.py: with it on, the phases of a call are separated by stream synchronisations */
enum { GPH_ALPHA, GPH_MPANEL, GPH_CONTRACT, GPH_RECURRENCE, GPH_DOT, GPH_COUNT };
static _Thread_local int gradProfileOn;
static _Thread_local double gradPhases[GPH_COUNT], gradT0;
void bfChebGradProfile(int on) { gradProfileOn = on; }
void bfChebGradLastPhases(double out[GPH_COUNT]) { memcpy(out, gradPhases, sizeof gradPhases); }
static void gradPhaseBegin(void *stream) {
  if (gradProfileOn) { bfdevSync(stream); gradT0 = bfNowSeconds(); }
}
static void gradPhaseEnd(void *stream, int ph) {
  if (gradProfileOn) { bfdevSync(stream); gradPhases[ph] += bfNowSeconds() - gradT0; }
}

/* the scratch of the gradient: allocated by the first call (which drains `stream`: allocating is not stream-ordered), kept until
 * the object is freed, not counted in factorBytes */
static int chebGradEnsure(BfhipCovCond *c, uint64_t chunks, void *stream) {
  if (c->dGradRows && c->dGradY && c->dGradM && c->dGradPart) return 0;
  uint64_t const n = c->be.n;
  uint32_t const k = c->k, Q = BF_COND_MAX_RHS;
  int rc;
  if ((rc = bfdevSync(stream))) return rc;
  if (!c->dGradRows) {
    if ((rc = bfdevMalloc((void **)&c->dGradRows, (size_t)k * 8))) return rc;
    if ((rc = bfdevMemcpyH2D(c->dGradRows, c->hObs, (size_t)k * 8))) { bfdevFree(c->dGradRows); c->dGradRows = NULL; return rc; }
  }
  if (!c->dGradY && (rc = bfdevMalloc((void **)&c->dGradY, n * Q * sizeof(double)))) return rc;
  if (!c->dGradM && (rc = bfdevMalloc((void **)&c->dGradM, 2 * (size_t)k * Q * sizeof(double)))) return rc;
  if (!c->dGradPart && (rc = bfdevMalloc((void **)&c->dGradPart, 64 * chunks * sizeof(double)))) return rc;
  return 0;
}

int bfhipChebCovCondLogLikGradDevice(BfhipCovCond *c, double const *dY, double const *dcoef, size_t const *orders, size_t numParams, size_t ldCoef,
                                     double *dGrad, double *dValue, BfhipCovCondLikOptions const *opt, void *stream) {
  if (!c || !dY || !dcoef || !orders || !dGrad) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (numParams == 0 || numParams > 64) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "numParams out of range (1 .. 64)");
  for (size_t t = 0; t < numParams; ++t)
    if (orders[t] == 0 || orders[t] > ldCoef)
      return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "orders[%zu] = %zu is zero or above ldCoef = %zu", t, orders[t], ldCoef);
  for (size_t t = 0; t < numParams; ++t)
    for (size_t j = 0; j < orders[t]; ++j)
      if (!isfinite(dcoef[t * ldCoef + j])) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "coefficient %zu of parameter %zu is not finite", j, t);
  if (opt && opt->structSize != sizeof *opt) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BfhipCovCondLikOptions.structSize is not the struct's");
  /* from here on the object is read */
  if (!c->cheb || !c->hObs) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "the object was not made by bfhipChebCovCondCreate: the gradient in the density's parameters is the Chebyshev route's");
  int rc;
  BfDevScope ds;
  if ((rc = chebCondLive(c)) || (rc = bfDevEnter(&ds, c->device))) return rc;
  BfhipChebCov *cheb = c->cheb;
  uint64_t const n = c->be.n, chunks = (n + BF_COND_CHUNK - 1) / BF_COND_CHUNK;
  uint32_t const k = c->k, Q = BF_COND_MAX_RHS, T = (uint32_t)numParams;
  if (gradProfileOn) memset(gradPhases, 0, sizeof gradPhases);
  if ((rc = chebGradEnsure(c, chunks, stream)) || (rc = chebWork(cheb, 2, Q, stream))) goto done;
  double *Kinv = c->dGradM, *Mp = c->dGradM + (size_t)k * Q;

  /* alpha = K^-1 y into c->dR and the value, launch for launch as bfhipCovCondLogLikelihoodDevice forms them */
  gradPhaseBegin(stream);
  if ((rc = bfdevCondResidual(c->dR, c->dPart, c->dBt, n, k, dY, NULL, 1, c->be.dtype, NULL, 1, 1, stream)) ||
      (rc = bfdevCondSolve(c->dL, k, c->dR, 1, stream)) || (dValue && (rc = bfdevLikValue(dValue, c->dL, k, dY, c->dR, stream)))) goto done;
  gradPhaseEnd(stream, GPH_ALPHA);

  for (uint32_t c0 = 0; c0 < k; c0 += Q) {
    uint32_t const pc = k - c0 < Q ? k - c0 : Q;
    /* M[:, panel] = alpha alpha[panel]^T - K^-1 E_panel: the two triangular solves of a sample pass on a k x pc block */
    gradPhaseBegin(stream);
    if ((rc = bfdevLikGradUnit(Kinv, k, c0, pc, stream)) || (rc = bfdevCondSolve(c->dL, k, Kinv, pc, stream)) ||
        (rc = bfdevLikGradM(Mp, c->dR, Kinv, k, c0, pc, stream))) goto done;
    gradPhaseEnd(stream, GPH_MPANEL);
    /* Y = X M[:, panel], once per panel */
    gradPhaseBegin(stream);
    if ((rc = bfdevLikGradContract(c->dGradY, c->dBt, n, k, Mp, pc, stream))) goto done;
    gradPhaseEnd(stream, GPH_CONTRACT);
    /* the panel of X'_t = q_t(S) D E_panel as Create makes X's: the unit panel (once), one recurrence per parameter, no output scaling */
    gradPhaseBegin(stream);
    if ((rc = bfdevChebUnitPanel(c->dWp, n, pc, c->dGradRows + c0, cheb->dD, stream))) goto done;
    gradPhaseEnd(stream, GPH_RECURRENCE);
    for (uint32_t t = 0; t < T; ++t) {
      double *xp = NULL;
      gradPhaseBegin(stream);
      if ((rc = chebMulCoef(cheb, dcoef + t * ldCoef, orders[t], c->dWp, 0, 0, pc, NULL, &xp, stream))) goto done;
      gradPhaseEnd(stream, GPH_RECURRENCE);
      gradPhaseBegin(stream);
      if ((rc = bfdevLikGradDot(c->dGradPart + t * chunks, c->dGradY, xp, n, pc, stream))) goto done;
      gradPhaseEnd(stream, GPH_DOT);
    }
    /* one owner per parameter: the panel's chunks in order, the panels in order */
    gradPhaseBegin(stream);
    if ((rc = bfdevLikGradSum(dGrad, c->dGradPart, chunks, T, c0 == 0, stream))) goto done;
    gradPhaseEnd(stream, GPH_DOT);
  }
done:
  bfDevLeave(&ds);
  return rc;
}
