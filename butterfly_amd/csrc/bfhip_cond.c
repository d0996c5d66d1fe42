/* bfhip_cond.c -- conditioning covariance samples on observations by a direct solve (include/bfhip.h, "conditioning on
 * observations").  Host side only: Create forms the observed rows of P A GammaLam with the adjoint
 * block apply, their Gram matrix and its Cholesky factor; a pass of <= 64 samples is then two contractions with the
 * stored n x k matrix, two triangular solves and ONE block sample (covSampleBlock of bfhip_cov.c, started from the
 * operator's covariance scratch).  The kernels are bfhip_cond.hip's.  A file of its own, like bfhip_cov.c, so that the
 * device-free sanitizer build of the host code keeps linking against its stubs unchanged.
 * What the object asks of the field it conditions goes through c->be (BfCondBackend, bfhip_cond.h): this file holds the
 * operator's backend, bfhip_cheb.c the Chebyshev route's; condSetup is the part of Create they share. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip_cond.h"
#include "../../include/bfhip_abi.h"

static int condKeyCmp(void const *a, void const *b) {
  uint64_t const x = ((BfCondKey const *)a)->idx, y = ((BfCondKey const *)b)->idx;
  return x < y ? -1 : x > y;
}

int condLookupSort(uint64_t const *idx, uint32_t count, char const *what, BfCondKey **keys) {
  BfCondKey *s = *keys = malloc(count * sizeof *s);
  if (!s) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory");
  for (uint32_t t = 0; t < count; ++t) { s[t].idx = idx[t]; s[t].slot = t; }
  qsort(s, count, sizeof *s, condKeyCmp);
  for (uint32_t t = 1; t < count; ++t)
    if (s[t].idx == s[t - 1].idx) {
      int const rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "%s index %llu is repeated", what, (unsigned long long)s[t].idx);
      free(s); *keys = NULL;
      return rc;
    }
  return 0;
}

int condLookupRange(BfCondKey const *keys, uint32_t count, char const *what, uint64_t numRows) {
  if (keys[count - 1].idx < numRows) return 0;
  return bfhipFail(BFABI_ERROR_OUT_OF_RANGE, "%s index %llu is outside the %llu rows", what, (unsigned long long)keys[count - 1].idx, (unsigned long long)numRows);
}

int condLookupRows(BfCondKey const *keys, uint64_t const *idx, uint32_t count, char const *what, uint64_t const *dRowPerm, uint64_t numRows, void *dRows,
                   void *stream) {
  if (!dRowPerm) return bfdevMemcpyH2D(dRows, idx, (size_t)count * 8);
  int rc;
  uint32_t flag = 0;
  uint64_t *hRows = malloc(count * sizeof *hRows), *hSorted = malloc(count * sizeof *hSorted);
  uint32_t *hSlot = malloc(count * sizeof *hSlot);
  void *dSorted = NULL, *dSlot = NULL, *dFlag = NULL;
  if (!hRows || !hSorted || !hSlot) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory"); goto out; }
  for (uint32_t t = 0; t < count; ++t) { hSorted[t] = keys[t].idx; hSlot[t] = keys[t].slot; hRows[t] = UINT64_MAX; }
  if ((rc = bfdevMalloc(&dSorted, (size_t)count * 8)) || (rc = bfdevMalloc(&dSlot, (size_t)count * 4)) || (rc = bfdevMalloc(&dFlag, 4)) ||
      (rc = bfdevMemcpyH2D(dSorted, hSorted, (size_t)count * 8)) || (rc = bfdevMemcpyH2D(dSlot, hSlot, (size_t)count * 4)) || (rc = bfdevMemcpyH2D(dFlag, &flag, 4)) ||
      (rc = bfdevMemcpyH2D(dRows, hRows, (size_t)count * 8))) goto out;
  if ((rc = bfdevCondInvertPerm(dRowPerm, numRows, dSorted, dSlot, count, dRows, dFlag, stream)) || (rc = bfdevSync(stream)) ||
      (rc = bfdevMemcpyD2H(hRows, dRows, (size_t)count * 8)) || (rc = bfdevMemcpyD2H(&flag, dFlag, 4))) goto out;
  for (uint32_t t = 0; t < count && !flag; ++t) if (hRows[t] >= numRows) flag = 1;
  if (flag) rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "dRowPerm does not hit every %s index exactly once", what);
out:
  bfdevFree(dSorted); bfdevFree(dSlot); bfdevFree(dFlag);
  free(hRows); free(hSorted); free(hSlot);
  return rc;
}

int condAdjointPanel(BfhipOperator *op, void const *dGammaLam, uint64_t const *dRows, uint32_t p, double *Bt, uint32_t k, uint32_t c0, void *stream) {
  uint64_t const m = op->plan.numRows, n = op->plan.numCols;
  uint32_t const dtype = op->plan.dtype;
  char *v, *t;                              /* the scratch's halves: unit panel, adjoint result */
  bfCovHalves(op, BF_COND_MAX_RHS, &v, &t);
  int rc;
  if ((rc = bfdevMemsetAsync(v, 0, m * p * op->plan.elemSize, stream)) || (rc = bfdevCondUnitPanel(v, m, p, dRows, dtype, stream)) ||
      (rc = bfhipApplyTransposeDevice(op, v, p, t, stream))) return rc;
  return bfdevCondPack(Bt, n, k, c0, t, p, dGammaLam, dtype, stream);
}

void condRelease(BfhipCovCond *c) {
  if (!c) return;
  bfdevFree(c->dBt); bfdevFree(c->dL); bfdevFree(c->dNoiseVar); bfdevFree(c->dNoiseSd); bfdevFree(c->dR); bfdevFree(c->dE); bfdevFree(c->dWn); bfdevFree(c->dPart);
  bfdevFree(c->dWp);
  condLikRelease(c);
  free(c->hObs);
  free(c);
}

int condCheckObs(uint64_t const *obs, uint32_t k, double const *noiseVar, BfCondKey **keys) {
  int rc = condLookupSort(obs, k, "observed", keys);
  if (rc) return rc;
  if (noiseVar) for (uint32_t a = 0; a < k && !rc; ++a)
    if (!(noiseVar[a] >= 0.0) || !isfinite(noiseVar[a])) rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "noiseVar[%u] is negative or not finite", a);
  if (rc) { free(*keys); *keys = NULL; }
  return rc;
}

int condSetup(BfhipCovCond *c, BfCondKey const *keys, uint64_t const *obs, double const *noiseVar, void *stream) {
  uint64_t const m = c->be.m, n = c->be.n;
  uint32_t const k = c->k, Q = BF_COND_MAX_RHS;
  uint64_t const chunks = (n + BF_COND_CHUNK - 1) / BF_COND_CHUNK;
  int rc;
  double *hSd = malloc(k * sizeof *hSd);
  void *dRows = NULL, *dStat = NULL;
  if (!hSd) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory");
  size_t const bytesBt = n * k * sizeof(double), bytesL = (size_t)k * k * sizeof(double), bytesR = (size_t)k * Q * sizeof(double);
  size_t const bytesW = n * Q * c->be.elemSize, bytesPart = chunks * bytesR;
  if ((rc = bfdevMalloc((void **)&c->dBt, bytesBt)) || (rc = bfdevMalloc((void **)&c->dL, bytesL)) || (rc = bfdevMalloc((void **)&c->dR, bytesR)) ||
      (rc = bfdevMalloc((void **)&c->dE, bytesR)) || (rc = bfdevMalloc(&c->dWn, bytesW)) || (rc = bfdevMalloc((void **)&c->dPart, bytesPart)) ||
      (rc = bfdevMalloc(&dRows, k * 8)) || (rc = bfdevMalloc(&dStat, sizeof(BfCondStat)))) goto out;
  c->info.structSize = sizeof c->info; c->info.numObs = k;
  c->info.factorBytes += bytesBt + bytesL + 2 * bytesR + bytesW + bytesPart;
  if (noiseVar) {
    for (uint32_t a = 0; a < k; ++a) hSd[a] = sqrt(noiseVar[a]);
    if ((rc = bfdevMalloc((void **)&c->dNoiseVar, k * 8)) || (rc = bfdevMalloc((void **)&c->dNoiseSd, k * 8)) ||
        (rc = bfdevMemcpyH2D(c->dNoiseVar, noiseVar, k * 8)) || (rc = bfdevMemcpyH2D(c->dNoiseSd, hSd, k * 8))) goto out;
    c->info.factorBytes += 2 * k * 8;
  }

  /* ---- phase 1: the rows i_a, then B^T by panels of <= 64 of them ---- */
  double t0 = bfNowSeconds();
  if ((rc = condLookupRows(keys, obs, k, "observed", c->dRowPerm, m, dRows, stream))) goto out;
  for (uint32_t c0 = 0; c0 < k; c0 += Q) {
    uint32_t const p = k - c0 < Q ? k - c0 : Q;
    if ((rc = c->be.panel(c, (uint64_t const *)dRows + c0, p, c->dBt, k, c0, stream))) goto out;
    ++c->info.setupApplies;
  }
  if ((rc = bfdevSync(stream))) goto out;
  double t1 = bfNowSeconds();
  c->info.rowsSeconds = t1 - t0;

  /* ---- phase 2: G + D (lower triangle; the rest stays zero) ---- */
  if ((rc = bfdevMemsetAsync(c->dL, 0, bytesL, stream)) || (rc = bfdevCondGram(c->dL, c->dBt, n, k, c->dNoiseVar, stream)) || (rc = bfdevSync(stream))) goto out;
  t0 = bfNowSeconds();
  c->info.gramSeconds = t0 - t1;

  /* ---- phase 3: Cholesky in place; the flag is read once, at the end ---- */
  BfCondStat st = {0xffffffffu, 0, INFINITY, -INFINITY};
  if ((rc = bfdevMemcpyH2D(dStat, &st, sizeof st)) || (rc = bfdevCondCholesky(c->dL, k, dStat, stream)) || (rc = bfdevSync(stream)) ||
      (rc = bfdevMemcpyD2H(&st, dStat, sizeof st))) goto out;
  c->info.factorSeconds = bfNowSeconds() - t0;
  if (st.failStep != 0xffffffffu) {
    rc = bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "Cholesky of G + D (%u observations): the pivot at step %u is <= 0 or not finite", k, st.failStep);
    goto out;
  }
  c->info.minPivot = st.minPivot; c->info.maxPivot = st.maxPivot;
out:
  bfdevFree(dRows); bfdevFree(dStat);
  free(hSd);
  return rc;
}

/* ---- the butterfly route's backend: B = P A GammaLam of an operator, W' in the first half of its covariance scratch ---- */
static int opPanel(BfhipCovCond *c, uint64_t const *dRows, uint32_t p, double *Bt, uint32_t ld, uint32_t c0, void *stream) {
  return condAdjointPanel(c->op, c->dGammaLam, dRows, p, Bt, ld, c0, stream);
}

static void *opWprime(BfhipCovCond *c) { return c->op->dCov; }

/* covSampleBlock scales the first half (bfCovHalves) in place, applies into the second and, with a permutation, scatters from there.
 * Into dZ directly; or packed into the half that sequence leaves free (without the scatter: where the apply left it) */
static int opField(BfhipCovCond *c, uint32_t b, int scatter, void *dZ, void **packed, void *stream) {
  BfhipOperator *op = c->op;
  uint64_t const *perm = scatter ? c->dRowPerm : NULL;
  if (dZ) return covSampleBlock(op, c->dGammaLam, perm, op->dCov, 0, b, dZ, stream);
  char *t0, *t1;
  bfCovHalves(op, b, &t0, &t1);
  *packed = perm ? t0 : t1;
  return covSampleBlock(op, c->dGammaLam, perm, t0, 0, b, *packed, stream);
}

int bfhipCovCondCreate(BfhipOperator *op, void const *dGammaLam, uint64_t const *dRowPerm, uint64_t const *obs, size_t numObs, double const *noiseVar,
                       BfhipCovCond **out, void *stream) {
  if (out) *out = NULL;
  if (!op || !obs || !out) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (numObs == 0 || numObs > BFHIP_COND_MAX_OBS) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "numObs out of range (1 .. %u)", BFHIP_COND_MAX_OBS);
  uint32_t const k = (uint32_t)numObs;
  BfCondKey *keys = NULL;
  BfDevScope ds = {0};
  int rc = condCheckObs(obs, k, noiseVar, &keys);
  if (rc) return rc;
  rc = condLookupRange(keys, k, "observed", op->plan.numRows);
  if (!rc) rc = bfCovCheckOperator(op, 1);
  /* the launch shapes of the per-pass kernels (bfhip_cond.hip): refused here, not in the first sample call after seconds of setup */
  if (!rc && !bfdevCondFits(op->plan.numCols)) rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "conditioning: %llu columns are more than the contractions' grids take (%llu)",
                                                              (unsigned long long)op->plan.numCols, (unsigned long long)BF_COND_MAX_COLS);
  if (rc) { free(keys); return rc; }

  BfhipCovCond *c = calloc(1, sizeof *c);
  if (!c) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "out of host memory"); goto fail; }
  c->be = (BfCondBackend){ op->plan.numCols, op->plan.numRows, op->plan.dtype, op->plan.elemSize, 1, opPanel, opWprime, opField, NULL };
  c->op = op; c->dGammaLam = dGammaLam; c->dRowPerm = dRowPerm; c->k = k; c->device = op->device;
  if ((rc = bfDevEnter(&ds, op->device))) goto fail;

  /* ---- everything a later call needs, for passes of 64 columns ---- */
  if ((rc = bfdevSync(stream))) goto fail;
  if ((rc = bfhipOperatorReserveRhs(op, BF_COND_MAX_RHS))) goto fail;
  if ((rc = covScratch(op, BF_COND_MAX_RHS, stream))) goto fail;
  if ((rc = condSetup(c, keys, obs, noiseVar, stream))) goto fail;
  *out = c; c = NULL;
fail:
  condRelease(c);
  free(keys);
  bfDevLeave(&ds);
  return rc;
}

/* Work enqueued on any stream may still read Bt, L and the per-pass blocks: the whole device is drained first.  Nothing is read
 * through c->op (the header asks for the object to go before its operator; the buffers are released correctly either way). */
void bfhipCovCondFree(BfhipCovCond **c) {
  if (!c || !*c) return;
  BfDevScope ds;
  bfDevEnter(&ds, (*c)->device);      /* a release cannot fail: errors are ignored on purpose */
  bfdevCondDeviceSync();
  condRelease(*c);
  *c = NULL;
  bfDevLeave(&ds);
}

int bfhipCovCondGetInfo(BfhipCovCond const *c, BfhipCovCondInfo *info) {
  if (!c || !info || info->structSize < sizeof *info) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument / BfhipCovCondInfo.structSize too small");
  *info = c->info;
  return 0;
}

/* the refusal of an object whose backend changed under it; every entry but Free and GetInfo asks */
static int condLive(BfhipCovCond const *c) { return c->be.live ? c->be.live(c) : 0; }

/* One pass of b <= 64 columns: alpha into c->dR, W' (not yet scaled by GammaLam) into the backend's packed block (the first b
 * columns' worth of the operator's covariance scratch, where a block sample of b columns starts; the object's own block on the
 * Chebyshev route).  W [n x .] and E [k x .] have leading dimensions ldw / lde (a pass of a wider block); NULL stands for zeros. */
static int condPass(BfhipCovCond *c, double const *dY, void const *W, uint64_t ldw, double const *E, uint64_t lde, uint32_t b, void *stream) {
  uint64_t const n = c->be.n;
  int rc;
  if ((rc = bfdevCondResidual(c->dR, c->dPart, c->dBt, n, c->k, dY, W, ldw, c->be.dtype, E, lde, b, stream))) return rc;
  if ((rc = bfdevCondSolve(c->dL, c->k, c->dR, b, stream))) return rc;
  return bfdevCondUpdate(c->be.wprime(c), c->dBt, n, c->k, c->dR, W, ldw, c->be.dtype, b, stream);
}

/* The rest of a pass: the field of the b columns of W' that condPass left, into columns s0 .. s0 + b - 1 of dZ [m x nrhs].  A whole
 * call (b == nrhs) writes dZ directly; a pass of a wider block lands packed in the backend's scratch and is copied into its columns. */
static int condFinish(BfhipCovCond *c, uint32_t b, size_t nrhs, size_t s0, void *dZ, void *stream) {
  size_t const es = c->be.elemSize;
  if (b == nrhs) return c->be.field(c, b, 1, dZ, NULL, stream);
  void *packed = NULL;
  int rc = c->be.field(c, b, 1, NULL, &packed, stream);
  if (!rc) rc = bfdevMemcpy2DAsync((char *)dZ + s0 * es, nrhs * es, packed, b * es, b * es, c->be.m, stream);
  return rc;
}

/* the passes of a block call: W / E NULL = zeros; dZ [m x nrhs], dAlpha [k x nrhs] or NULL */
static int condBlock(BfhipCovCond *c, double const *dY, void const *dW, double const *dEps, size_t nrhs, void *dZ, double *dAlpha, void *stream) {
  size_t const es = c->be.elemSize;
  int rc = 0;
  for (size_t s0 = 0; s0 < nrhs && !rc; s0 += BF_COND_MAX_RHS) {
    uint32_t const b = (uint32_t)(nrhs - s0 < BF_COND_MAX_RHS ? nrhs - s0 : BF_COND_MAX_RHS);
    if ((rc = condPass(c, dY, dW ? (char const *)dW + s0 * es : NULL, nrhs, dEps ? dEps + s0 : NULL, nrhs, b, stream))) break;
    if (dAlpha) {
      if (b == nrhs) rc = bfdevMemcpyD2DAsync(dAlpha, c->dR, (size_t)c->k * b * sizeof(double), stream);
      else rc = bfdevMemcpy2DAsync(dAlpha + s0, nrhs * sizeof(double), c->dR, b * sizeof(double), b * sizeof(double), c->k, stream);
      if (rc) break;
    }
    rc = condFinish(c, b, nrhs, s0, dZ, stream);
  }
  return rc;
}

int bfhipCovCondSampleBlockDevice(BfhipCovCond *c, double const *dY, void const *dW, double const *dEps, size_t nrhs, void *dZ, double *dAlpha, void *stream) {
  if (!c || !dY || !dW || !dZ) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (nrhs == 0 || nrhs > 0xffffu) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "nrhs out of range");
  int rc;
  BfDevScope ds;
  if ((rc = condLive(c)) || (rc = bfDevEnter(&ds, c->device))) return rc;
  rc = condBlock(c, dY, dW, dEps, nrhs, dZ, dAlpha, stream);
  bfDevLeave(&ds);
  return rc;
}

int bfhipCovCondMeanDevice(BfhipCovCond *c, double const *dY, void *dMean, double *dAlpha, void *stream) {
  if (!c || !dY || !dMean) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  int rc;
  BfDevScope ds;
  if ((rc = condLive(c)) || (rc = bfDevEnter(&ds, c->device))) return rc;
  rc = condBlock(c, dY, NULL, NULL, 1, dMean, dAlpha, stream);
  bfDevLeave(&ds);
  return rc;
}

/* the normals of samples first .. first + b - 1 into c->dWn [n x b] and c->dE [k x b] (the latter scaled, in double) */
static int condFill(BfhipCovCond *c, uint64_t seed, uint64_t noiseSeed, uint64_t first, uint32_t b, void *stream) {
  int rc = bfdevCovDrawFill(c->dWn, NULL, c->be.n, b, c->be.dtype, seed, first, stream);
  if (!rc && c->dNoiseSd) rc = bfdevCovDrawFill(c->dE, c->dNoiseSd, c->k, b, BFHIP_F64, noiseSeed, first, stream);
  return rc;
}

int bfhipCovCondDrawDevice(BfhipCovCond *c, double const *dY, uint64_t seed, uint64_t noiseSeed, uint64_t firstSample, size_t nrhs, void *dZ, void *stream) {
  if (!c || !dY || !dZ) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (nrhs == 0 || nrhs > 0xffffu) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "nrhs out of range");
  int rc;
  BfDevScope ds;
  if ((rc = condLive(c)) || (rc = bfDevEnter(&ds, c->device))) return rc;
  for (size_t s0 = 0; s0 < nrhs && !rc; s0 += BF_COND_MAX_RHS) {
    uint32_t const b = (uint32_t)(nrhs - s0 < BF_COND_MAX_RHS ? nrhs - s0 : BF_COND_MAX_RHS);
    if ((rc = condFill(c, seed, noiseSeed, firstSample + s0, b, stream))) break;
    if ((rc = condPass(c, dY, c->dWn, b, c->dNoiseSd ? c->dE : NULL, b, b, stream))) break;
    rc = condFinish(c, b, nrhs, s0, dZ, stream);
  }
  bfDevLeave(&ds);
  return rc;
}

int bfhipCovCondMomentsDevice(BfhipCovCond *c, double const *dY, uint64_t seed, uint64_t noiseSeed, uint64_t firstSample, uint64_t numSamples, uint32_t batch,
                              double *dSum, double *dSumSq, void *stream) {
  if (!c || !dY) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (!dSum && !dSumSq) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "both moment outputs are NULL");
  if (batch > BF_COND_MAX_RHS) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "batch out of range (at most 64)");
  if (numSamples == 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "numSamples is zero");
  if (!batch) batch = BF_COND_MAX_RHS;
  if (batch > numSamples) batch = (uint32_t)numSamples;
  int rc;
  BfDevScope ds;
  if ((rc = condLive(c)) || (rc = bfDevEnter(&ds, c->device))) return rc;
  for (uint64_t s0 = 0; s0 < numSamples && !rc; s0 += batch) {
    uint32_t const b = (uint32_t)(numSamples - s0 < batch ? numSamples - s0 : batch);
    void *z = NULL;
    if ((rc = condFill(c, seed, noiseSeed, firstSample + s0, b, stream))) break;
    if ((rc = condPass(c, dY, c->dWn, b, c->dNoiseSd ? c->dE : NULL, b, b, stream))) break;
    /* the field without its scatter, left in the backend's scratch: Z is never written, the un-permuted result goes straight into
     * the sums of its rows' places */
    if ((rc = c->be.field(c, b, 0, NULL, &z, stream))) break;
    rc = bfdevCovMoments(z, c->be.m, b, c->be.dtype, c->dRowPerm, dSum, dSumSq, stream);
  }
  bfDevLeave(&ds);
  return rc;
}
