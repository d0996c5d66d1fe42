/* bfhip_condlik.c -- the log marginal likelihood of the observations with its gradients, and exact kriging variances, of
 * a conditioned field (include/bfhip.h, "conditioning on observations").  Host side only; the object
 * and its matrices Bt, L are bfhip_cond.c's, the kernels bfhip_condlik.hip's.  Both entries come down to column sums of
 * squares of L^-1 S for a wide S that is never stored (bfdevLikStripSolve):
 *   gamma gradient   S = Bt^T (n columns)          u_j^2 - ||L^-1 b_j||^2
 *   noise gradient   S = I (k columns)             (alpha_a^2 - ||L^-1 e_a||^2) / 2
 *   variance         S = Bt^T r (<= 64 columns)    ||r||^2 - ||L^-1 Bt^T r||^2
 * A file of its own, like bfhip_cond.c, so that the device-free sanitizer build of the host code keeps linking against its
 * stubs unchanged. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip_cond.h"
#include "../../include/bfhip_abi.h"

#define LIK_DEFAULT_BYTES (256ull << 20)

void condLikRelease(BfhipCovCond *c) {
  bfdevFree(c->dStrips); bfdevFree(c->dLinv); bfdevFree(c->dColSq); bfdevFree(c->dVarBlk); bfdevFree(c->dVarPart);
  c->dStrips = c->dLinv = c->dColSq = c->dVarBlk = c->dVarPart = NULL;
  c->likSlots = 0;
  bfdevFree(c->dGradRows); bfdevFree(c->dGradY); bfdevFree(c->dGradM); bfdevFree(c->dGradPart);
  c->dGradRows = NULL; c->dGradY = c->dGradM = c->dGradPart = NULL;
}

static uint64_t stripBytes(BfhipCovCond const *c) { return (uint64_t)c->k * BF_LIK_STRIP * sizeof(double); }

/* at least `slots` strips of scratch, the inverses of the diagonal tiles of L (formed here, once) and, for the likelihood,
 * the vector of column sums; allocating is not stream-ordered and drains `stream` first */
static int likEnsure(BfhipCovCond *c, uint64_t slots, int colSq, void *stream) {
  int rc;
  if (c->likSlots >= slots && c->dLinv && (!colSq || c->dColSq)) return 0;
  if ((rc = bfdevSync(stream))) return rc;
  if (c->likSlots < slots) {
    bfdevFree(c->dStrips); c->dStrips = NULL; c->likSlots = 0;
    if ((rc = bfdevMalloc((void **)&c->dStrips, slots * stripBytes(c)))) return rc;
    c->likSlots = slots;
  }
  if (!c->dLinv) {
    size_t const tiles = (c->k + BF_LIK_NB - 1) / BF_LIK_NB;
    if ((rc = bfdevMalloc((void **)&c->dLinv, tiles * BF_LIK_NB * BF_LIK_NB * sizeof(double)))) return rc;
    if ((rc = bfdevLikInvDiag(c->dLinv, c->dL, c->k, stream))) { bfdevFree(c->dLinv); c->dLinv = NULL; return rc; }
  }
  if (colSq && !c->dColSq && (rc = bfdevMalloc((void **)&c->dColSq, (c->be.n + c->k) * sizeof(double)))) return rc;
  return 0;
}

int bfhipCovCondLogLikelihoodDevice(BfhipCovCond *c, double const *dY, double *dValue, double *dGradLogGamma, double *dGradNoise,
                                    BfhipCovCondLikOptions const *opt, void *stream) {
  if (!c || !dY || !dValue) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (opt && opt->structSize != sizeof *opt) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BfhipCovCondLikOptions.structSize is not the struct's");
  uint64_t const ws = opt ? opt->workspaceBytes : 0, strip = stripBytes(c);
  if (ws && ws < strip)
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "workspaceBytes %llu is below one strip (%llu bytes)", (unsigned long long)ws, (unsigned long long)strip);
  if (dGradLogGamma && !c->be.columnWeights)
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "dGradLogGamma: the field of this object has no per-column weights (Chebyshev route)");
  int rc;
  BfDevScope ds;
  if ((c->be.live && (rc = c->be.live(c))) || (rc = bfDevEnter(&ds, c->device))) return rc;
  uint64_t const n = c->be.n;
  uint32_t const k = c->k;
  /* no more slots than the wider of the two solves has strips */
  uint64_t const most = ((n > k ? n : k) + BF_LIK_STRIP - 1) / BF_LIK_STRIP;
  uint64_t slots = (ws ? ws : LIK_DEFAULT_BYTES) / strip;
  if (slots > most) slots = most;
  if (!slots) slots = 1;
  if ((dGradLogGamma || dGradNoise) && (rc = likEnsure(c, slots, 1, stream))) goto done;
  /* alpha = K^-1 y into c->dR: the first two steps of the mean's pass (W = 0, E = 0, one column) */
  if ((rc = bfdevCondResidual(c->dR, c->dPart, c->dBt, n, k, dY, NULL, 1, c->be.dtype, NULL, 1, 1, stream))) goto done;
  if ((rc = bfdevCondSolve(c->dL, k, c->dR, 1, stream))) goto done;
  if ((rc = bfdevLikValue(dValue, c->dL, k, dY, c->dR, stream))) goto done;
  if (dGradLogGamma) {
    if ((rc = bfdevLikStripSolve(c->dL, c->dLinv, k, BF_LIK_SRC_BT_ROWS, c->dBt, 0, n, c->dStrips, slots, c->dColSq, stream))) goto done;
    if ((rc = bfdevLikGradGamma(dGradLogGamma, c->dBt, n, k, c->dR, c->dColSq, stream))) goto done;
  }
  if (dGradNoise) {
    if ((rc = bfdevLikStripSolve(c->dL, c->dLinv, k, BF_LIK_SRC_IDENTITY, NULL, 0, k, c->dStrips, slots, c->dColSq + n, stream))) goto done;
    rc = bfdevLikGradNoise(dGradNoise, c->dR, c->dColSq + n, k, stream);
  }
done:
  bfDevLeave(&ds);
  return rc;
}

int bfhipCovCondVarianceDevice(BfhipCovCond *c, uint64_t const *query, size_t numQuery, double *dPrior, double *dPost, void *stream) {
  if (!c || !query) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (numQuery == 0 || numQuery > 0xffffffffu) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "numQuery out of range");
  if (!dPrior && !dPost) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "both variance outputs are NULL");
  uint32_t const nq = (uint32_t)numQuery;
  BfCondKey *keys = NULL;
  BfDevScope ds = {0};
  int rc = condLookupSort(query, nq, "query", &keys);
  if (rc) return rc;
  /* from here on the object is read; a bad index is refused before the device is touched */
  if ((rc = condLookupRange(keys, nq, "query", c->be.m)) || (c->be.live && (rc = c->be.live(c)))) { free(keys); return rc; }

  uint64_t const m = c->be.m, n = c->be.n;
  uint64_t const chunks = (n + BF_COND_CHUNK - 1) / BF_COND_CHUNK;
  uint32_t const k = c->k, Q = BF_COND_MAX_RHS;
  void *dRows = NULL;
  double *dSolved = NULL, *dZeros = NULL;
  if ((rc = bfDevEnter(&ds, c->device))) goto done;

  /* ---- workspace: one strip, the panel of rows and the small vectors ---- */
  if ((rc = likEnsure(c, 1, 0, stream))) goto done;
  if (!c->dVarBlk || !c->dVarPart) {
    if ((rc = bfdevSync(stream))) goto done;
    if (!c->dVarBlk && (rc = bfdevMalloc((void **)&c->dVarBlk, n * Q * sizeof(double)))) goto done;
    if (!c->dVarPart) {
      size_t const bytes = (chunks * BF_LIK_STRIP + BF_LIK_STRIP + k) * sizeof(double);
      if ((rc = bfdevMalloc((void **)&c->dVarPart, bytes)) || (rc = bfdevMemset(c->dVarPart, 0, bytes))) goto done;
    }
  }
  dSolved = c->dVarPart + chunks * BF_LIK_STRIP; dZeros = dSolved + BF_LIK_STRIP;       /* [64] sums of the solve, [k] zeros */

  /* ---- the rows i_t with dRowPerm[i_t] = query[t] ---- */
  if ((rc = bfdevMalloc(&dRows, (size_t)nq * 8)) || (rc = condLookupRows(keys, query, nq, "query", c->dRowPerm, m, dRows, stream))) goto done;

  /* ---- panels of <= 64 queries: r^T by the backend's panel (one adjoint apply), its squares, Bt^T r, the strip solve ---- */
  for (uint32_t t0 = 0; t0 < nq; t0 += Q) {
    uint32_t const p = nq - t0 < Q ? nq - t0 : Q;
    if ((rc = c->be.panel(c, (uint64_t const *)dRows + t0, p, c->dVarBlk, p, 0, stream)) ||
        (rc = bfdevVarPriorPart(c->dVarPart, c->dVarBlk, n, p, stream))) goto done;
    if (dPost) {
      /* R = 0 - Bt^T r (the sign does not reach the squares), then ||L^-1 R||^2 per column */
      if ((rc = bfdevCondResidual(c->dR, c->dPart, c->dBt, n, k, dZeros, c->dVarBlk, p, BFHIP_F64, NULL, 0, p, stream)) ||
          (rc = bfdevLikStripSolve(c->dL, c->dLinv, k, BF_LIK_SRC_BLOCK, c->dR, p, p, c->dStrips, 1, dSolved, stream))) goto done;
    }
    if ((rc = bfdevVarAssemble(dPrior ? dPrior + t0 : NULL, dPost ? dPost + t0 : NULL, c->dVarPart, chunks, dSolved, p, stream))) goto done;
  }
  rc = bfdevSync(stream);                                            /* the row buffer goes with the call */
done:
  bfdevFree(dRows);
  free(keys);
  bfDevLeave(&ds);
  return rc;
}
