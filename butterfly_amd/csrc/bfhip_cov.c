/* bfhip_cov.c -- batched covariance sampling: the covariance products of bfhip_api.c on blocks of right-hand sides, device
 * normals, the draw that needs no input vector and the streaming moments (include/bfhip.h, "batched covariance sampling").
 * Host side only: the operator is applied by bfhipApplyDevice / bfhipApplyTransposeDevice -- runPlan with nrhs columns, so
 * the operator's switches alone decide which stage kernels run -- and the blocks around the applies are prepared and
 * consumed by the kernels of bfhip_cov.hip.  The scratch is the single-vector entries' (covScratch, bfhip_api.c), grown. */
#include <stdint.h>
#include <stdlib.h>

#include "bfhip_operator.h"
#include "../../include/bfhip.h"
#include "../../include/bfhip_abi.h"

int bfhipFillNormalDevice(void *d, uint64_t count, uint64_t firstIdx, uint32_t dtype, uint64_t seed, void *stream) {
  if (!d) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (dtype != BFHIP_F64 && dtype != BFHIP_F32) return bfhipFail(BFABI_ERROR_TYPE_ERROR, "normals are real: dtype must be BFHIP_F64 or BFHIP_F32");
  return bfdevFillNormal(d, count, firstIdx, dtype, seed, stream);
}

/* the checks every block entry shares, in the order of the single-vector entries: arguments, element type, (adjoint,) device */
static int covBlockCheck(BfhipOperator const *op, void const *in, void const *out, size_t nrhs, int needAdjoint) {
  if (!op || !in || !out) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (nrhs == 0 || nrhs > 0xffffu) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "nrhs out of range");
  return bfCovCheckOperator(op, needAdjoint);
}

/* z = P A (GammaLam w) on blocks.  `scaled`: the input block is already in the scratch's first half, scaled (the draw) */
int covSampleBlock(BfhipOperator *op, void const *dGammaLam, uint64_t const *dRowPerm, void const *dW, int scaled, size_t nrhs, void *dZ, void *stream) {
  uint64_t const m = op->plan.numRows, n = op->plan.numCols;
  char *t0, *t1;
  bfCovHalves(op, nrhs, &t0, &t1);
  int rc;
  void const *xin = scaled ? t0 : dW;
  if (!scaled && dGammaLam) { if ((rc = bfdevCovScalePermute(t0, dW, dGammaLam, 1, NULL, n, (uint32_t)nrhs, op->plan.dtype, stream))) return rc; xin = t0; }
  if ((rc = bfhipApplyDevice(op, xin, nrhs, dRowPerm ? (void *)t1 : dZ, stream))) return rc;
  if (dRowPerm) rc = bfdevCovScalePermute(dZ, t1, NULL, 0, dRowPerm, m, (uint32_t)nrhs, op->plan.dtype, stream);
  return rc;
}

int bfhipCovSampleBlockDevice(BfhipOperator *op, void const *dGammaLam, uint64_t const *dRowPerm, void const *dW, size_t nrhs, void *dZ, void *stream) {
  int rc;
  BfDevScope ds;
  if ((rc = covBlockCheck(op, dW, dZ, nrhs, 0)) || (rc = bfDevEnter(&ds, op->device))) return rc;
  if (!(rc = covScratch(op, nrhs, stream))) rc = covSampleBlock(op, dGammaLam, dRowPerm, dW, 0, nrhs, dZ, stream);
  bfDevLeave(&ds);
  return rc;
}

int bfhipCovMatvecBlockDevice(BfhipOperator *op, void const *dGammaLam, uint64_t const *dRowPerm, uint64_t const *dRevRowPerm, void const *dV, size_t nrhs, void *dZ, void *stream) {
  int rc;
  BfDevScope ds;
  if ((rc = covBlockCheck(op, dV, dZ, nrhs, 1)) || (rc = bfDevEnter(&ds, op->device))) return rc;
  uint64_t const m = op->plan.numRows, n = op->plan.numCols;
  uint32_t const nr = (uint32_t)nrhs;
  if ((rc = covScratch(op, nrhs, stream))) goto out;
  char *t0, *t1;
  bfCovHalves(op, nrhs, &t0, &t1);
  void const *vin = dV;
  if (dRevRowPerm) { if ((rc = bfdevCovScalePermute(t0, dV, NULL, 0, dRevRowPerm, m, nr, op->plan.dtype, stream))) goto out; vin = t0; }
  if ((rc = bfhipApplyTransposeDevice(op, vin, nrhs, t1, stream))) goto out;                 /* tmp2 = Phi^T V */
  if (dGammaLam && (rc = bfdevCovScalePermute(t1, t1, dGammaLam, 2, NULL, n, nr, op->plan.dtype, stream))) goto out;   /* GammaLam twice, in place */
  if ((rc = bfhipApplyDevice(op, t1, nrhs, dRowPerm ? (void *)t0 : dZ, stream))) goto out;
  if (dRowPerm) rc = bfdevCovScalePermute(dZ, t0, NULL, 0, dRowPerm, m, nr, op->plan.dtype, stream);
out:
  bfDevLeave(&ds);
  return rc;
}

int bfhipCovDrawDevice(BfhipOperator *op, void const *dGammaLam, uint64_t const *dRowPerm, uint64_t seed, uint64_t firstSample, size_t nrhs, void *dZ, void *stream) {
  int rc;
  BfDevScope ds;
  if ((rc = covBlockCheck(op, dZ, dZ, nrhs, 0)) || (rc = bfDevEnter(&ds, op->device))) return rc;
  if ((rc = covScratch(op, nrhs, stream))) goto out;
  if ((rc = bfdevCovDrawFill(op->dCov, dGammaLam, op->plan.numCols, (uint32_t)nrhs, op->plan.dtype, seed, firstSample, stream))) goto out;
  rc = covSampleBlock(op, dGammaLam, dRowPerm, NULL, 1, nrhs, dZ, stream);
out:
  bfDevLeave(&ds);
  return rc;
}

int bfhipCovMomentsDevice(BfhipOperator *op, void const *dGammaLam, uint64_t const *dRowPerm, uint64_t seed, uint64_t firstSample, uint64_t numSamples,
                          uint32_t batch, double *dSum, double *dSumSq, void *stream) {
  int rc;
  BfDevScope ds;
  if (!op) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (!dSum && !dSumSq) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "both moment outputs are NULL");
  if (batch > 64) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "batch out of range (at most 64)");
  if (numSamples == 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "numSamples is zero");
  if ((rc = covBlockCheck(op, op, op, 1, 0))) return rc;
  if (!batch) batch = 64;
  if (batch > numSamples) batch = (uint32_t)numSamples;
  if ((rc = bfDevEnter(&ds, op->device))) return rc;
  uint64_t const m = op->plan.numRows, n = op->plan.numCols;
  if ((rc = covScratch(op, batch, stream))) goto out;
  for (uint64_t s0 = 0; s0 < numSamples; s0 += batch) {
    uint32_t const b = (uint32_t)(numSamples - s0 < batch ? numSamples - s0 : batch);
    /* a batch of b columns is packed at b columns: both halves start where they would for a call of nrhs = b */
    char *t0, *t1;
    bfCovHalves(op, b, &t0, &t1);
    if ((rc = bfdevCovDrawFill(t0, dGammaLam, n, b, op->plan.dtype, seed, firstSample + s0, stream))) goto out;
    if ((rc = bfhipApplyDevice(op, t0, b, t1, stream))) goto out;
    /* Z is never written: the un-permuted result goes straight into the sums of its rows' places */
    if ((rc = bfdevCovMoments(t1, m, b, op->plan.dtype, dRowPerm, dSum, dSumSq, stream))) goto out;
  }
out:
  bfDevLeave(&ds);
  return rc;
}
