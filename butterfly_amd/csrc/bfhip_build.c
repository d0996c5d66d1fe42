/* bfhip_build.c -- host side of the fac_helm2 value builder (include/bfhip_build.h).
 *
 * The reference builds one block at a time on the CPU (src/fac_helm2.c:42-509:
 * kernel matrix, SVD-based least squares, store the block).  Here the dense
 * leaves of the already laid-out operand are processed in batches that fit a
 * device workspace: every kernel matrix of a batch in one launch, every
 * least-squares problem of a batch in one Jacobi launch per size class, two
 * batched GEMM launches, then one launch that copies the batch's leaves into
 * the packed arena the apply kernels read.  Nothing but the recipes and the
 * point coordinates crosses PCIe.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"
#include "../../include/bfhip_build.h"

#define DEFAULT_WORKSPACE ((uint64_t)8 << 30)

static BfBuildPts toPts(BfhipPointSet const *p) {
  BfBuildPts q;
  q.kind = p->kind; q.count = p->count; q.first = p->first; q.cx = p->cx; q.cy = p->cy; q.r = p->r;
  return q;
}

static int checkPts(BfhipPointSet const *p, BfhipHelm2Problem const *prob, char const *what, uint64_t idx) {
  if (p->count == 0) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "recipe %llu: empty %s point set", (unsigned long long)idx, what);
  if (p->kind == BFHIP_PTS_TREE || p->kind == BFHIP_PTS_TREE_TGT) {
    if (p->kind == BFHIP_PTS_TREE_TGT && !prob->tgtPoints)
      return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "recipe %llu: %s points refer to a target tree but tgtPoints is NULL", (unsigned long long)idx, what);
    uint64_t const numPoints = p->kind == BFHIP_PTS_TREE ? prob->numPoints : prob->numTgtPoints;
    if (p->first + p->count > numPoints)
      return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "recipe %llu: %s points [%llu, %llu) exceed numPoints", (unsigned long long)idx, what,
                       (unsigned long long)p->first, (unsigned long long)(p->first + p->count));
  } else if (p->kind != BFHIP_PTS_CIRCLE) {
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "recipe %llu: unknown point-set kind %u", (unsigned long long)idx, p->kind);
  }
  return 0;
}

static uint32_t leafRows(BfhipHelm2Recipe const *r) { return r->kind == BFHIP_LEAF_KERNEL ? r->tgt.count : r->equiv.count; }

static int checkProblem(BfhipHelm2Problem const *prob) {
  if (!prob) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL problem");
  if (prob->structSize < sizeof(BfhipHelm2Problem)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BfhipHelm2Problem.structSize too small");
  if (prob->outDtype != BFHIP_C128 && prob->outDtype != BFHIP_C64)
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "outDtype must be 0 (BFHIP_C128) or BFHIP_C64, got %u", prob->outDtype);
  if (prob->layerPot != BFHIP_LAYER_POTENTIAL_SINGLE && prob->layerPot != BFHIP_LAYER_POTENTIAL_PV_NORMAL_DERIV_SINGLE &&
      prob->layerPot != BFHIP_LAYER_POTENTIAL_PV_DOUBLE && prob->layerPot != BFHIP_LAYER_POTENTIAL_COMBINED_FIELD)
    return bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "layer potential %u is not built on the device (S = 1, D = 2, S' = 3, combined = 5 are)",
                     prob->layerPot);                 /* as bfHelm2GetKernelMatrix, src/helm2.c:296-316 */
  if (prob->layerPot != BFHIP_LAYER_POTENTIAL_SINGLE && !prob->normals)
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "this layer potential needs the unit normals at the points");
  if (prob->krOrder != 0 && prob->krOrder != 2 && prob->krOrder != 6 && prob->krOrder != 10)
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "Kapur-Rokhlin order must be 0, 2, 6 or 10");    /* src/quadrature.c:106 */
  if (prob->krOrder && !prob->origIndex) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "the KR correction needs origIndex");
  if (prob->tgtPoints && (prob->krOrder || prob->selfValue[0] != 0 || prob->selfValue[1] != 0))
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "selfValue / KR correction apply to square operators (no separate target tree)");
  if (prob->krOrder && prob->numPoints < 2 * (uint64_t)prob->krOrder + 1)
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "too few points for the KR correction");          /* src/quadrature.c:115 */
  if (!prob->points || (!prob->recipes && prob->numRecipes)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL points / recipes");
  if (!(prob->wavenumber > 0)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "wavenumber must be positive");
  return 0;
}

static int checkRecipe(BfhipHelm2Problem const *prob, uint64_t i) {
  BfhipHelm2Recipe const *r = &prob->recipes[i];
  int rc;
  if ((rc = checkPts(&r->src, prob, "source", i))) return rc;
  if ((rc = checkPts(&r->tgt, prob, "target", i))) return rc;
  if (r->kind == BFHIP_LEAF_REEXP) {
    if ((rc = checkPts(&r->equiv, prob, "equivalent-source", i))) return rc;
    if (r->tgt.count < r->equiv.count)
      return bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "recipe %llu: fewer check points (%u) than equivalent sources (%u)",
                       (unsigned long long)i, r->tgt.count, r->equiv.count);
  } else if (r->kind != BFHIP_LEAF_KERNEL) {
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "recipe %llu: unknown kind %u", (unsigned long long)i, r->kind);
  } else if (prob->layerPot == BFHIP_LAYER_POTENTIAL_PV_NORMAL_DERIV_SINGLE &&
             (r->tgt.kind == BFHIP_PTS_CIRCLE || (r->tgt.kind == BFHIP_PTS_TREE_TGT && !prob->tgtNormals))) {
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "recipe %llu: an S' kernel leaf needs target normals, i.e. tree-point targets", (unsigned long long)i);
  }
  return 0;
}

/* potential codes of the device layer: what the operator's own leaves use, and what the two
 * matrices of a re-expansion use (BF_PROXY_LAYER_POT, include/bf/layer_pot.h:63-69) */
static uint32_t leafPotCode(uint32_t layerPot) {
  return layerPot == BFHIP_LAYER_POTENTIAL_PV_NORMAL_DERIV_SINGLE ? 1 : layerPot == BFHIP_LAYER_POTENTIAL_PV_DOUBLE ? 2
       : layerPot == BFHIP_LAYER_POTENTIAL_COMBINED_FIELD ? 3 : 0;
}
static uint32_t proxyPotCode(uint32_t layerPot) {
  return layerPot == BFHIP_LAYER_POTENTIAL_PV_DOUBLE ? 2 : layerPot == BFHIP_LAYER_POTENTIAL_COMBINED_FIELD ? 3 : 0;
}

/* device copies of what every kernel evaluation reads */
typedef struct DevEnv { BfEvalEnv env; void *dPoints, *dNormals, *dWeights, *dOrig, *dHits, *dTgtPoints, *dTgtNormals; } DevEnv;

static void envFree(DevEnv *e) {
  bfdevFree(e->dPoints); bfdevFree(e->dNormals); bfdevFree(e->dWeights); bfdevFree(e->dOrig); bfdevFree(e->dHits);
  bfdevFree(e->dTgtPoints); bfdevFree(e->dTgtNormals);
  memset(e, 0, sizeof *e);
}

static int envUpload(BfhipHelm2Problem const *prob, DevEnv *e) {
  memset(e, 0, sizeof *e);
  size_t const n = (size_t)(prob->numPoints ? prob->numPoints : 1);
  int rc = bfdevMalloc(&e->dPoints, n * 16);
  if (!rc) rc = bfdevMemcpyH2D(e->dPoints, prob->points, (size_t)prob->numPoints * 16);
  if (!rc && prob->normals) {
    rc = bfdevMalloc(&e->dNormals, n * 16);
    if (!rc) rc = bfdevMemcpyH2D(e->dNormals, prob->normals, (size_t)prob->numPoints * 16);
  }
  if (!rc && prob->colWeights) {
    rc = bfdevMalloc(&e->dWeights, n * 8);
    if (!rc) rc = bfdevMemcpyH2D(e->dWeights, prob->colWeights, (size_t)prob->numPoints * 8);
  }
  if (!rc && prob->tgtPoints) {
    size_t const m = (size_t)(prob->numTgtPoints ? prob->numTgtPoints : 1);
    rc = bfdevMalloc(&e->dTgtPoints, m * 16);
    if (!rc) rc = bfdevMemcpyH2D(e->dTgtPoints, prob->tgtPoints, (size_t)prob->numTgtPoints * 16);
    if (!rc && prob->tgtNormals) {
      rc = bfdevMalloc(&e->dTgtNormals, m * 16);
      if (!rc) rc = bfdevMemcpyH2D(e->dTgtNormals, prob->tgtNormals, (size_t)prob->numTgtPoints * 16);
    }
  }
  if (!rc && prob->krOrder) {
    rc = bfdevMalloc(&e->dOrig, n * 8);
    if (!rc) rc = bfdevMemcpyH2D(e->dOrig, prob->origIndex, (size_t)prob->numPoints * 8);
    if (!rc) rc = bfdevMalloc(&e->dHits, 8);
    if (!rc) rc = bfdevMemset(e->dHits, 0, 8);
  }
  if (rc) { envFree(e); return rc; }
  e->env.dOrigIndex = e->dOrig; e->env.numPoints = prob->numPoints; e->env.krOrder = prob->krOrder;
  e->env.dKrHits = (unsigned long long *)e->dHits;
  e->env.dTgtPoints = e->dTgtPoints; e->env.dTgtNormals = e->dTgtNormals;
  e->env.dPoints = e->dPoints; e->env.dNormals = e->dNormals; e->env.dColWeights = e->dWeights;
  e->env.wavenumber = prob->wavenumber; e->env.selfRe = prob->selfValue[0]; e->env.selfIm = prob->selfValue[1];
  e->env.alphaRe = prob->alpha[0]; e->env.alphaIm = prob->alpha[1]; e->env.betaRe = prob->beta[0]; e->env.betaIm = prob->beta[1];
  return 0;
}

/* workspace of one re-expansion problem, in complex elements */
typedef struct ReexpWs { uint64_t zeq, v, x, zor, t, scale, total; } ReexpWs;

/* Problems with at least this many equivalent sources go through the QR preconditioner (bfQrcpKernel) before the
 * Jacobi kernel: those are the ones whose stacked matrix does not stay in LDS.  BFHIP_JACOBI_QR_MIN overrides the
 * default (0: every problem, a test hook; a huge value: none); the route as a whole is bfLstSqRoute (bfhip_internal.h). */
static uint64_t qrMinCols(void) { return (uint64_t)bfLstSqResolve(NULL).qrMin; }
static int usesQr(BfhipHelm2Recipe const *r, uint64_t qrMin) {
  return r->equiv.count >= qrMin && bfQrcpLds(r->tgt.count, r->equiv.count) != 0;
}

static ReexpWs reexpWs(BfhipHelm2Recipe const *r, uint64_t qrMin) {
  uint64_t const mt = r->tgt.count, me = r->equiv.count, n = r->src.count;
  ReexpWs w;
  w.zeq = 0;
  w.v = w.zeq + mt * me;
  w.x = w.v + me * me;
  w.zor = w.x + (usesQr(r, qrMin) ? me * me : 0);
  w.t = w.zor + mt * n;
  w.scale = w.t + me * n;
  w.total = w.scale + (me + 1) / 2;
  return w;
}

static uint64_t recipeCost(BfhipHelm2Recipe const *r) {
  uint64_t c = (uint64_t)leafRows(r) * r->src.count;
  if (r->kind == BFHIP_LEAF_REEXP) c += reexpWs(r, qrMinCols()).total;
  return c;
}

/* Device buffers of the batches, kept from one batch to the next (allocating and freeing ~100 GB per batch costs seconds). */
typedef struct BatchBufs { void *store, *ws; uint64_t storeElems, wsElems; } BatchBufs;
static void batchBufsFree(BatchBufs *b) { bfdevFree(b->store); bfdevFree(b->ws); memset(b, 0, sizeof *b); }
static int batchBufsReserve(BatchBufs *b, uint64_t storeElems, uint64_t wsElems) {
  int rc = 0;
  if (storeElems > b->storeElems || !b->store) {
    bfdevFree(b->store); b->store = NULL; b->storeElems = 0;
    if ((rc = bfdevMalloc(&b->store, (size_t)(storeElems ? storeElems : 1) * 16))) return rc;
    b->storeElems = storeElems;
  }
  if (wsElems > b->wsElems) {
    bfdevFree(b->ws); b->ws = NULL; b->wsElems = 0;
    if ((rc = bfdevMalloc(&b->ws, (size_t)wsElems * 16))) return rc;
    b->wsElems = wsElems;
  }
  return 0;
}

/* leaf-store and workspace elements of a batch */
static void batchSizes(BfhipHelm2Problem const *prob, uint64_t const *idx, uint64_t count, uint64_t qrMin, uint64_t *storeElems, uint64_t *wsElems);

/* The truncated-SVD least-squares solve X = pinv_k(A) B of a batch of problems, on device workspace: A (mt x me) and B
 * (mt x n) are overwritten, V (me x me), Xq (me x me: QR route only), T (me x n), scale (me doubles), out = X (me x n,
 * ld me).  info (device [3] or NULL): sweeps, not converged, singular values kept.  One QR launch per LDS class, the Jacobi
 * launches, two batched GEMM launches:
 *   plain:  A V = W (orthogonal columns, norms sigma):  T = diag(1/sigma^2) W^H B,  X = V T;
 *   QR:     A P = Q R in place, B <- Q^H B, and the Jacobi kernel gets Xq = (R[0:r] P^T)^H (me x r) instead of A:
 *           Xq V1 = W  =>  X = W diag(1/sigma^2) V1^H (Q^H B)[0:r]  (bfhip_lstsq.hip).
 * qrOut (host [count] or NULL): the QR stage's rank of each problem (me when the problem skips it), with BF_QR_NONFINITE
 * when A was not finite; routes (host [count] or NULL): the route each problem took. */
typedef struct BfLsJob {
  void *a, *b, *v, *xq, *t, *out;
  double *scale;
  uint32_t *info;
  uint32_t mt, me, n, dim;
} BfLsJob;

static int lstsqSolve(BfLsJob const *jobs, uint64_t count, BfLstSqOpts const *opts, BfhipBuildStats *st, uint32_t *qrOut,
                      BfLstSqRoute *routes, int profile) {
  int rc = 0;
  BfLstSqOpts const o = bfLstSqResolve(opts);
  BfSvdProb *probs = malloc((count + 1) * sizeof *probs);
  BfGemmJob *g1 = malloc((count + 1) * sizeof *g1), *g2 = malloc((count + 1) * sizeof *g2);
  BfQrProb *qr = malloc((count + 1) * sizeof *qr);
  uint64_t *qrOf = malloc((count + 1) * sizeof *qrOf);          /* least-squares problem of the k-th QR problem */
  uint32_t *qrRank = malloc((count + 1) * sizeof *qrRank);
  uint64_t nq = 0;
  double tp = profile ? bfNowSeconds() : 0;
#define BF_PHASE(name) do { if (profile) { double const t = bfNowSeconds(); fprintf(stderr, "[build] %-12s %.3f s\n", name, t - tp); tp = t; } } while (0)
  if (!probs || !g1 || !g2 || !qr || !qrOf || !qrRank) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (least squares)"); goto done; }
  for (uint64_t i = 0; i < count; ++i) {
    BfLsJob const *J = &jobs[i];
    memset(&probs[i], 0, sizeof probs[i]);
    probs[i].a = J->a; probs[i].v = J->v; probs[i].scale = J->scale; probs[i].info = J->info;
    probs[i].mt = J->mt; probs[i].me = J->me; probs[i].dim = J->dim;
    if (qrOut) qrOut[i] = J->me;
    if (J->me >= o.qrMin && bfQrcpLds(J->mt, J->me)) {
      qr[nq].a = J->a; qr[nq].b = J->b; qr[nq].x = J->xq;
      qr[nq].mt = J->mt; qr[nq].me = J->me; qr[nq].n = J->n; qr[nq].dim = J->dim;
      qrOf[nq++] = i;
    }
    /* T = diag(1/sigma^2) (U Sigma)^H B */
    memset(&g1[i], 0, sizeof g1[i]);
    g1[i].a = J->a; g1[i].b = J->b; g1[i].c = J->t; g1[i].scale = J->scale;
    g1[i].M = J->me; g1[i].N = J->n; g1[i].K = J->mt; g1[i].lda = J->mt; g1[i].ldb = J->mt; g1[i].ldc = J->me; g1[i].transA = 1;
    /* X = V T */
    memset(&g2[i], 0, sizeof g2[i]);
    g2[i].a = J->v; g2[i].b = J->t; g2[i].c = J->out; g2[i].scale = NULL;
    g2[i].M = J->me; g2[i].N = J->n; g2[i].K = J->me; g2[i].lda = J->me; g2[i].ldb = J->me; g2[i].ldc = J->me; g2[i].transA = 0;
    if (routes) bfLstSqRoute(J->mt, J->me, J->me, &o, &routes[i]);
  }
  if ((rc = bfdevBuildQrcp(qr, nq, qrRank))) goto done;
  BF_PHASE("qr");
  for (uint64_t k = 0; k < nq; ++k) {
    uint64_t const q = qrOf[k];
    uint32_t const me = qr[k].me, nonFinite = qrRank[k] & BF_QR_NONFINITE, rk = nonFinite ? 0 : qrRank[k];
    probs[q].a = qr[k].x; probs[q].mt = me; probs[q].me = rk;                     /* V1: rk x rk in the v block */
    g1[q].a = probs[q].v; g1[q].M = rk; g1[q].K = rk; g1[q].lda = rk;             /* T[0:rk] = diag(1/sigma^2) V1^H (Q^H B)[0:rk] */
    g2[q].a = qr[k].x; g2[q].K = rk; g2[q].lda = me;                              /* X = W T[0:rk] */
    if (qrOut) qrOut[q] = qrRank[k];
    if (routes) bfLstSqRoute(jobs[q].mt, me, rk, &o, &routes[q]);
    st->qrProblems += 1; st->qrColumns += me; st->qrRank += rk;
    /* a matrix that is not finite has no answer: counted like an SVD that did not converge (the build then fails unless
     * BFHIP_ALLOW_UNCONVERGED_SVD=1); rank 0 of a finite matrix (zero, or below the threshold together) is the reference's
     * answer X = 0.  With K = 0 the second GEMM writes an exactly zero leaf instead of leaving what the reused store held. */
    if (nonFinite) st->notConverged += 1;
  }
  BfSvdStats ss = {st->maxSweeps, 0, 0, 0};
  if ((rc = bfdevBuildJacobi(probs, count, &o, &ss))) goto done;
  st->maxSweeps = ss.maxSweeps; st->notConverged += ss.notConverged; st->truncated += ss.truncated; st->sumSweeps += ss.sumSweeps;
  BF_PHASE("jacobi");
  if ((rc = bfdevBuildGemm(g1, count))) goto done;
  if ((rc = bfdevBuildGemm(g2, count))) goto done;
  BF_PHASE("gemm");
#undef BF_PHASE
done:
  free(probs); free(g1); free(g2); free(qr); free(qrOf); free(qrRank);
  return rc;
}

/* Compute recipes idx[0..count) on the current device.  *dStore receives a
 * device buffer holding the leaves column-major at storeOff[i] (elements). */
static int buildBatch(BfhipHelm2Problem const *prob, uint64_t const *idx, uint64_t count, BfEvalEnv const *env,
                      BatchBufs *bufs, void **dStore, uint64_t *storeOff, BfhipBuildStats *st) {
  int rc = 0;
  *dStore = NULL;
  void *dWs = NULL;
  uint64_t storeElems = 0, wsElems = 0, numReexp = 0;
  uint64_t *wsOff = malloc((count + 1) * sizeof *wsOff);
  BfEvalMat *mats = malloc(2 * count * sizeof *mats);
  uint64_t *prefix = malloc((2 * count + 1) * sizeof *prefix);
  BfLsJob *jobs = malloc((count + 1) * sizeof *jobs);
  uint64_t const qrMin = qrMinCols();
  if (!wsOff || !mats || !prefix || !jobs) {
    rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (builder batch)");
    goto done;
  }
  for (uint64_t i = 0; i < count; ++i) {
    BfhipHelm2Recipe const *r = &prob->recipes[idx[i]];
    storeOff[i] = storeElems;
    storeElems += (uint64_t)leafRows(r) * r->src.count;
    wsOff[i] = wsElems;
    if (r->kind == BFHIP_LEAF_REEXP) { wsElems += reexpWs(r, qrMin).total; ++numReexp; }
  }
  double const tAlloc = bfNowSeconds();
  if ((rc = batchBufsReserve(bufs, storeElems, wsElems))) goto done;
  *dStore = bufs->store; dWs = bufs->ws;
  char *store = (char *)*dStore, *ws = (char *)dWs;
  uint64_t nm = 0, np = 0;
  prefix[0] = 0;
  uint32_t const leafPot = leafPotCode(prob->layerPot), proxyPot = proxyPotCode(prob->layerPot);
  for (uint64_t i = 0; i < count; ++i) {
    BfhipHelm2Recipe const *r = &prob->recipes[idx[i]];
    if (r->kind == BFHIP_LEAF_KERNEL) {
      mats[nm].src = toPts(&r->src); mats[nm].tgt = toPts(&r->tgt); mats[nm].dst = store + storeOff[i] * 16;
      mats[nm].pot = leafPot; mats[nm].decorate = 1;
      prefix[nm + 1] = prefix[nm] + ((uint64_t)r->tgt.count * r->src.count + BF_EVAL_TILE - 1) / BF_EVAL_TILE;
      ++nm;
      st->kernelLeaves += 1;
      st->kernelEvals += (uint64_t)r->tgt.count * r->src.count;
      continue;
    }
    ReexpWs const w = reexpWs(r, qrMin);
    char *base = ws + wsOff[i] * 16;
    uint32_t const mt = r->tgt.count, me = r->equiv.count, n = r->src.count;
    /* re-expansions use the proxy potential; the column weights of the operator scale Z_orig */
    mats[nm].src = toPts(&r->equiv); mats[nm].tgt = toPts(&r->tgt); mats[nm].dst = base + w.zeq * 16;
    mats[nm].pot = proxyPot; mats[nm].decorate = 0;
    prefix[nm + 1] = prefix[nm] + ((uint64_t)mt * me + BF_EVAL_TILE - 1) / BF_EVAL_TILE;
    ++nm;
    mats[nm].src = toPts(&r->src); mats[nm].tgt = toPts(&r->tgt); mats[nm].dst = base + w.zor * 16;
    mats[nm].pot = proxyPot; mats[nm].decorate = 1;
    prefix[nm + 1] = prefix[nm] + ((uint64_t)mt * n + BF_EVAL_TILE - 1) / BF_EVAL_TILE;
    ++nm;
    BfLsJob *J = &jobs[np++];
    J->a = base + w.zeq * 16; J->b = base + w.zor * 16; J->v = base + w.v * 16; J->xq = base + w.x * 16; J->t = base + w.t * 16;
    J->out = store + storeOff[i] * 16; J->scale = (double *)(base + w.scale * 16); J->info = NULL;
    J->mt = mt; J->me = me; J->n = n; J->dim = mt > me ? mt : me;
    st->reexpLeaves += 1;
    st->kernelEvals += (uint64_t)mt * me + (uint64_t)mt * n;
  }
  char const *penv = getenv("BFHIP_JACOBI_PROFILE");
  int const profile = penv && penv[0] == '1';
  if (profile) fprintf(stderr, "[build] %-12s %.3f s\n", "alloc + lists", bfNowSeconds() - tAlloc);
  double const tEval = bfNowSeconds();
  if ((rc = bfdevBuildEval(mats, prefix, nm, env))) goto done;
  if (profile) fprintf(stderr, "[build] %-12s %.3f s\n", "kernel eval", bfNowSeconds() - tEval);
  if ((rc = lstsqSolve(jobs, np, NULL, st, NULL, NULL, profile))) goto done;
  st->numBatches += 1;
done:
  if (rc) *dStore = NULL;
  free(wsOff); free(mats); free(prefix); free(jobs);
  return rc;
}

static void batchSizes(BfhipHelm2Problem const *prob, uint64_t const *idx, uint64_t count, uint64_t qrMin, uint64_t *storeElems, uint64_t *wsElems) {
  uint64_t se = 0, we = 0;
  for (uint64_t i = 0; i < count; ++i) {
    BfhipHelm2Recipe const *r = &prob->recipes[idx[i]];
    se += (uint64_t)leafRows(r) * r->src.count;
    if (r->kind == BFHIP_LEAF_REEXP) we += reexpWs(r, qrMin).total;
  }
  *storeElems = se; *wsElems = we;
}

/* ---- arena fill: called by the compile step instead of packing host values ---- */
typedef struct PieceRec { uint64_t rec, dataOff; uint32_t row0, col0, mr, mrPad, ncols, rowMajor, ld; } PieceRec;

/* One arena the batches are packed into: a plan's pieces grouped by recipe (sorted[pieceBegin[i] .. pieceBegin[i + 1]) are
 * recipe i's), of either storage type.  bfhipBuildHelm2 has one, bfhipBuildHelm2Pair two filled from the same batches. */
typedef struct PackTarget {
  void *dArena;
  uint32_t dtype;            /* BFHIP_C128 or BFHIP_C64 */
  int whole;                 /* the plan is the whole square operator (the KR correction can be checked on it) */
  PieceRec *sorted;
  uint64_t *pieceBegin;      /* [numRecipes + 2] */
} PackTarget;

#define MAX_TARGETS 2
typedef struct BuildCtx {
  BfhipHelm2Problem const *prob;
  BfhipBuildStats *stats;
  PackTarget tgt[MAX_TARGETS];
  uint32_t numTargets, wanted;       /* collected so far; the values are built once `wanted` arenas are known */
} BuildCtx;

static void buildCtxFree(BuildCtx *ctx) {
  for (uint32_t t = 0; t < MAX_TARGETS; ++t) { free(ctx->tgt[t].sorted); free(ctx->tgt[t].pieceBegin); }
  memset(ctx->tgt, 0, sizeof ctx->tgt);
  ctx->numTargets = 0;
}

/* the plan's non-identity pieces, grouped by recipe; every recipe and its leaf checked on the way */
static int collectTarget(BfPlan const *pl, BfIr const *ir, void *dArena, BfhipHelm2Problem const *prob, PackTarget *T) {
  int rc = 0;
  if (pl->dtype != BFHIP_C128 && pl->dtype != BFHIP_C64) return bfhipFail(BFABI_ERROR_TYPE_ERROR, "the Helmholtz builder fills complex128 or complex64 operands");
  uint64_t const R = prob->numRecipes;
  int64_t *recOf = malloc((ir->numNodes + 1) * sizeof *recOf);
  uint64_t *pieceBegin = calloc(R + 2, sizeof *pieceBegin);
  PieceRec *pieces = NULL, *sorted = NULL;
  if (!recOf || !pieceBegin) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (builder)"); goto done; }
  for (uint64_t i = 0; i < ir->numNodes; ++i) recOf[i] = -1;
  for (uint64_t i = 0; i < R && !rc; ++i) {
    BfhipHelm2Recipe const *r = &prob->recipes[i];
    if (r->node >= ir->numNodes || ir->kind[r->node] != BFHIP_NODE_DENSE)
      rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "recipe %llu: node %llu is not a dense leaf", (unsigned long long)i, (unsigned long long)r->node);
    else if (recOf[r->node] >= 0)
      rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "recipe %llu: leaf %llu already has a recipe", (unsigned long long)i, (unsigned long long)r->node);
    else if ((rc = checkRecipe(prob, i)) == 0) {
      if (ir->rows[r->node] != leafRows(r) || ir->cols[r->node] != r->src.count)
        rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "recipe %llu: leaf %llu is %llu x %llu, recipe yields %u x %u", (unsigned long long)i,
                       (unsigned long long)r->node, (unsigned long long)ir->rows[r->node], (unsigned long long)ir->cols[r->node],
                       leafRows(r), r->src.count);
      recOf[r->node] = (int64_t)i;
    }
  }
  if (rc) goto done;

  /* the plan's pieces, grouped by recipe (counting sort) */
  uint64_t numPieces = 0;
  for (uint64_t s = 0; s < pl->numStages; ++s) numPieces += pl->stages[s].numPieces;
  pieces = malloc((numPieces + 1) * sizeof *pieces);
  sorted = malloc((numPieces + 1) * sizeof *sorted);
  if (!pieces || !sorted) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (builder pieces)"); goto done; }
  uint64_t np = 0;
  for (uint64_t s = 0; s < pl->numStages && !rc; ++s) {
    BfStage const *stg = &pl->stages[s];
    for (uint64_t i = 0; i < stg->numItems && !rc; ++i) {
      BfDevItem const *it = &stg->items[i];
      uint32_t const mr = it->mrFlags & 0xffffu;
      uint32_t const mrPad = (mr + pl->epl - 1) / pl->epl * pl->epl;
      for (uint32_t k = 0; k < it->numPieces; ++k) {
        BfDevPiece const *pc = &stg->pieces[it->pieceBegin + k];
        BfPieceSrc const *src = &stg->pieceSrc[it->pieceBegin + k];
        if (pc->flags & BF_PIECE_IDENTITY) continue;
        int64_t const rec = recOf[src->node];
        if (rec < 0) { rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "dense leaf %llu has no recipe", (unsigned long long)src->node); break; }
        PieceRec *p = &pieces[np++];
        p->rec = (uint64_t)rec; p->dataOff = pc->dataOff; p->row0 = src->row0; p->col0 = src->col0;
        p->mr = mr; p->mrPad = mrPad; p->ncols = pc->ncols;
        p->rowMajor = (pc->flags & BF_PIECE_ROWMAJOR) != 0; p->ld = pc->ld;
        pieceBegin[rec + 1] += 1;
      }
    }
  }
  if (rc) goto done;
  for (uint64_t i = 0; i < R; ++i) pieceBegin[i + 1] += pieceBegin[i];
  {
    uint64_t *cursor = malloc((R + 1) * sizeof *cursor);
    if (!cursor) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (builder)"); goto done; }
    memcpy(cursor, pieceBegin, (R + 1) * sizeof *cursor);
    for (uint64_t i = 0; i < np; ++i) sorted[cursor[pieces[i].rec]++] = pieces[i];
    free(cursor);
  }
  T->dArena = dArena; T->dtype = pl->dtype;
  T->whole = !prob->tgtPoints && pl->numRows == prob->numPoints && pl->numCols == prob->numPoints;
  T->sorted = sorted; T->pieceBegin = pieceBegin;
  sorted = NULL; pieceBegin = NULL;
done:
  free(recOf); free(pieceBegin); free(pieces); free(sorted);
  return rc;
}

/* does recipe i's leaf survive in any of the plans */
static int recipeKept(BuildCtx const *ctx, uint64_t i) {
  for (uint32_t t = 0; t < ctx->numTargets; ++t)
    if (ctx->tgt[t].pieceBegin[i + 1] != ctx->tgt[t].pieceBegin[i]) return 1;
  return 0;
}

/* every kept recipe computed once, batch by batch, and each batch packed into every arena its leaves survive in */
static int buildAndPack(BuildCtx *ctx) {
  BfhipHelm2Problem const *prob = ctx->prob;
  BfhipBuildStats *st = ctx->stats;
  uint64_t const R = prob->numRecipes;
  int rc = 0;
  uint64_t *batch = NULL, *storeOff = NULL;
  BfPackPiece *pack = NULL;
  DevEnv dev;
  memset(&dev, 0, sizeof dev);
  BatchBufs bufs;
  memset(&bufs, 0, sizeof bufs);

  char const *penv = getenv("BFHIP_JACOBI_PROFILE");
  int const profile = penv && penv[0] == '1';
  double tph = bfNowSeconds();
  if ((rc = envUpload(prob, &dev))) goto done;

  /* default workspace: half of what is free once the arena is allocated, at least 8 GiB asked for --
   * large batches keep all CUs busy through the tail of the biggest least-squares problems */
  uint64_t wsBytes = prob->workspaceBytes;
  if (!wsBytes) {
    uint64_t freeBytes = 0;
    if ((rc = bfdevMemFree(&freeBytes))) goto done;
    wsBytes = freeBytes / 2 > DEFAULT_WORKSPACE ? freeBytes / 2 : DEFAULT_WORKSPACE;
  }
  uint64_t const budget = wsBytes / 16;
  batch = malloc((R + 1) * sizeof *batch);
  storeOff = malloc((R + 1) * sizeof *storeOff);
  if (!batch || !storeOff) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (builder)"); goto done; }
  /* the largest batch sizes the buffers once */
  {
    uint64_t maxStore = 0, maxWs = 0;
    for (uint64_t j = 0; j < R;) {
      uint64_t nb = 0, cost = 0;
      for (; j < R; ++j) {
        if (!recipeKept(ctx, j)) continue;
        uint64_t const c = recipeCost(&prob->recipes[j]);
        if (nb && cost + c > budget) break;
        batch[nb++] = j; cost += c;
      }
      if (!nb) break;
      uint64_t se, we;
      batchSizes(prob, batch, nb, qrMinCols(), &se, &we);
      maxStore = se > maxStore ? se : maxStore; maxWs = we > maxWs ? we : maxWs;
    }
    if ((rc = batchBufsReserve(&bufs, maxStore, maxWs))) goto done;
  }
  uint64_t i = 0;
  while (i < R && !rc) {
    /* next batch: recipes whose leaves survive in one of the plans, until the workspace is full */
    uint64_t nb = 0, cost = 0;
    for (; i < R; ++i) {
      if (!recipeKept(ctx, i)) continue;                         /* sharded away */
      uint64_t const c = recipeCost(&prob->recipes[i]);
      if (nb && cost + c > budget) break;
      batch[nb++] = i; cost += c;
    }
    if (!nb) break;
    void *dStore = NULL;
    if (profile) { double const t = bfNowSeconds(); fprintf(stderr, "[build] host before batch %.3f s\n", t - tph); tph = t; }
    if ((rc = buildBatch(prob, batch, nb, &dev.env, &bufs, &dStore, storeOff, st))) break;
    if (profile) { double const t = bfNowSeconds(); fprintf(stderr, "[build] batch total %.3f s (%llu recipes)\n", t - tph, (unsigned long long)nb); tph = t; }
    for (uint32_t t = 0; t < ctx->numTargets && !rc; ++t) {
      PackTarget const *T = &ctx->tgt[t];
      uint64_t packCount = 0, q = 0;
      for (uint64_t b = 0; b < nb; ++b) packCount += T->pieceBegin[batch[b] + 1] - T->pieceBegin[batch[b]];
      pack = malloc((packCount + 1) * sizeof *pack);
      if (!pack) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (builder pack list)"); break; }
      for (uint64_t b = 0; b < nb; ++b) {
        uint64_t const rec = batch[b];
        uint32_t const ld = leafRows(&prob->recipes[rec]);
        for (uint64_t k = T->pieceBegin[rec]; k < T->pieceBegin[rec + 1]; ++k) {
          PieceRec const *p = &T->sorted[k];
          pack[q].dataOff = p->dataOff;
          pack[q].srcOff = storeOff[b] + (uint64_t)p->col0 * ld + p->row0;
          pack[q].srcLd = ld; pack[q].mr = p->mr; pack[q].mrPad = p->mrPad; pack[q].ncols = p->ncols;
          pack[q].rowMajor = p->rowMajor; pack[q].ld = p->ld;
          ++q;
        }
      }
      rc = bfdevBuildPack(T->dArena, T->dtype, dStore, pack, q);
      free(pack); pack = NULL;
    }
    if (profile) { double const t = bfNowSeconds(); fprintf(stderr, "[build] pack + free  %.3f s\n", t - tph); tph = t; }
  }
  /* every KR pair must have been met exactly once by a dense near-field leaf; a pair inside a
   * butterflied block cannot be corrected through the values */
  int whole = 0;
  for (uint32_t t = 0; t < ctx->numTargets; ++t) whole |= ctx->tgt[t].whole;
  if (!rc && prob->krOrder && whole) {
    unsigned long long hits = 0;
    rc = bfdevMemcpyD2H(&hits, dev.dHits, 8);
    if (!rc && hits != 2ull * prob->krOrder * prob->numPoints)
      rc = bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "KR correction: %llu of %llu near-diagonal entries lie in dense leaves",
                     hits, 2ull * prob->krOrder * prob->numPoints);
  }
done:
  batchBufsFree(&bufs);
  envFree(&dev);
  free(batch); free(storeOff);
  return rc;
}

/* The compile step's fill callback.  The host mirrors of a plan's pieces are gone once its compile returns, so each compile
 * collects its pieces here; the values are built when the last arena is known (the pair's first compile returns with its arena
 * still to be written, during the second compile's callback). */
static int fillArena(BfPlan const *pl, BfIr const *ir, void *dArena, void *vctx) {
  BuildCtx *ctx = vctx;
  if (ctx->numTargets >= ctx->wanted || ctx->wanted > MAX_TARGETS) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "builder: more arenas than asked for");
  int const rc = collectTarget(pl, ir, dArena, ctx->prob, &ctx->tgt[ctx->numTargets]);
  if (rc) return rc;
  ctx->numTargets += 1;
  return ctx->numTargets < ctx->wanted ? 0 : buildAndPack(ctx);
}

/* `opts` as the compile step reads them (fields a shorter struct lacks are 0), with the complex64 store asked for */
static int c64Options(BfhipOptions const *opts, BfhipOptions *o) {
  memset(o, 0, sizeof *o);
  o->device = -1;
  if (opts) {
    if (opts->structSize < BFHIP_OPTIONS_SIZE_V1) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BfhipOptions.structSize too small");
    memcpy(o, opts, opts->structSize < sizeof *o ? opts->structSize : sizeof *o);
  }
  o->structSize = sizeof *o;
  o->demoteToF32 = 1;
  return 0;
}

static int checkBuildOptions(BfhipOptions const *opts) {
  /* BfhipOptions.demoteToF32 stays refused on the builder entries: complex64 output is asked for through
   * BfhipHelm2Problem.outDtype (bfhipBuildHelm2) or bfhipBuildHelm2Pair */
  if (opts && opts->demoteToF32)
    return bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "the Helmholtz builder takes no demoteToF32: complex64 output is BfhipHelm2Problem.outDtype = BFHIP_C64");
  if (opts && (opts->flags & BFHIP_FLAG_PLAN_ONLY)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BFHIP_FLAG_PLAN_ONLY has no device to build on");
  return 0;
}

/* what both entries end with: the statistics handed out (also on failure: the counts say why), and an operator whose
 * least-squares leaves came from an SVD that hit the sweep cap refused -- it is silently wrong
 * (BFHIP_ALLOW_UNCONVERGED_SVD=1 in the environment keeps it, for diagnosis) */
static int finishBuild(int rc, BfhipBuildStats const *local, BfhipBuildStats *stats) {
  if (stats && stats->structSize >= sizeof *local) *stats = *local;
  if (!rc && stats && stats->structSize < sizeof *local) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BfhipBuildStats.structSize too small");
  if (!rc && local->notConverged && !getenv("BFHIP_ALLOW_UNCONVERGED_SVD"))
    return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "%llu Jacobi SVD problem(s) did not converge within the sweep cap; operator discarded",
                     (unsigned long long)local->notConverged);
  return rc;
}

int bfhipBuildHelm2(BfhipDesc const *desc, BfhipHelm2Problem const *prob, BfhipOptions const *opts, BfhipOperator **out,
                    BfhipBuildStats *stats) {
  if (!desc || !out) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  *out = NULL;
  int rc = checkProblem(prob);
  if (rc) return rc;
  if (desc->dtype != BFHIP_C128) return bfhipFail(BFABI_ERROR_TYPE_ERROR, "the Helmholtz builder fills complex128 operands");
  if ((rc = checkBuildOptions(opts))) return rc;
  /* complex64 output: the plan bfhipCompileDesc makes of this descriptor under demoteToF32 */
  BfhipOptions low;
  if (prob->outDtype == BFHIP_C64) {
    if ((rc = c64Options(opts, &low))) return rc;
    opts = &low;
  }
  BfhipBuildStats local;
  memset(&local, 0, sizeof local);
  local.structSize = sizeof local;
  BuildCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.prob = prob; ctx.stats = &local; ctx.wanted = 1;
  BfIr ir;
  if ((rc = bfIrFromDesc(desc, &ir))) return rc;
  double const t0 = bfNowSeconds();
  rc = bfhipCompileIrFill(&ir, opts, fillArena, &ctx, out);
  buildCtxFree(&ctx);
  local.seconds = bfNowSeconds() - t0;
  int const rc2 = finishBuild(rc, &local, stats);
  if (rc2 && !rc) bfhipFree(out);
  return rc2;
}

int bfhipBuildHelm2Pair(BfhipDesc const *desc, BfhipHelm2Problem const *prob, BfhipOptions const *opts, BfhipOptions const *optsLow,
                        BfhipOperator **out, BfhipOperator **outLow, BfhipBuildStats *stats) {
  if (!desc || !out || !outLow) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  *out = NULL; *outLow = NULL;
  int rc = checkProblem(prob);
  if (rc) return rc;
  if (prob->outDtype != BFHIP_C128)
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "bfhipBuildHelm2Pair makes both operators: outDtype must be 0 (BFHIP_C128)");
  if (desc->dtype != BFHIP_C128) return bfhipFail(BFABI_ERROR_TYPE_ERROR, "the Helmholtz builder fills complex128 operands");
  if (!optsLow) optsLow = opts;
  if ((rc = checkBuildOptions(opts)) || (rc = checkBuildOptions(optsLow))) return rc;
  if ((opts ? opts->device : -1) != (optsLow ? optsLow->device : -1))
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "bfhipBuildHelm2Pair: both operators live on one device");
  BfhipOptions low;
  if ((rc = c64Options(optsLow, &low))) return rc;
  BfhipBuildStats local;
  memset(&local, 0, sizeof local);
  local.structSize = sizeof local;
  BuildCtx ctx;
  memset(&ctx, 0, sizeof ctx);
  ctx.prob = prob; ctx.stats = &local; ctx.wanted = 2;
  double const t0 = bfNowSeconds();
  /* the first compile only collects its pieces (fillArena); its arena is written while the second one fills its own */
  BfIr ir;
  if (!(rc = bfIrFromDesc(desc, &ir))) rc = bfhipCompileIrFill(&ir, opts, fillArena, &ctx, out);
  if (!rc && !(rc = bfIrFromDesc(desc, &ir))) rc = bfhipCompileIrFill(&ir, &low, fillArena, &ctx, outLow);
  buildCtxFree(&ctx);
  local.seconds = bfNowSeconds() - t0;
  rc = finishBuild(rc, &local, stats);
  if (rc) { bfhipFree(out); bfhipFree(outLow); }      /* neither is returned: the first one's arena may be unwritten */
  return rc;
}

int bfhipHelm2BuildLeaf(BfhipHelm2Problem const *prob, uint64_t recipeIndex, int device, void *out) {
  int rc = checkProblem(prob);
  if (rc) return rc;
  if (!out || recipeIndex >= prob->numRecipes) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "bad recipe index / NULL output");
  if ((rc = checkRecipe(prob, recipeIndex))) return rc;
  BfDevScope ds;
  if ((rc = bfDevEnter(&ds, device))) return rc;
  BfhipHelm2Recipe const *r = &prob->recipes[recipeIndex];
  uint64_t const m = leafRows(r), n = r->src.count;
  void *dStore = NULL;
  DevEnv dev;
  memset(&dev, 0, sizeof dev);
  double *tmp = malloc((size_t)m * n * 16);
  BfhipBuildStats st;
  memset(&st, 0, sizeof st);
  uint64_t off = 0;
  if (!tmp) rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  if (!rc) rc = envUpload(prob, &dev);
  BatchBufs bufs;
  memset(&bufs, 0, sizeof bufs);
  if (!rc) rc = buildBatch(prob, &recipeIndex, 1, &dev.env, &bufs, &dStore, &off, &st);
  if (!rc) rc = bfdevMemcpyD2H(tmp, dStore, (size_t)m * n * 16);
  if (!rc) {
    double *o = out;                                   /* column-major store -> row-major result */
    for (uint64_t i = 0; i < m; ++i)
      for (uint64_t j = 0; j < n; ++j) { o[2 * (i * n + j)] = tmp[2 * (j * m + i)]; o[2 * (i * n + j) + 1] = tmp[2 * (j * m + i) + 1]; }
  }
  batchBufsFree(&bufs); envFree(&dev); free(tmp);
  bfDevLeave(&ds);
  return rc;
}

int bfhipHelm2DenseApplyDevice(BfhipHelm2Problem const *prob, int device, void const *dX, void *dY, void *stream) {
  int rc = checkProblem(prob);
  if (rc) return rc;
  if (!dX || !dY) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  BfDevScope ds;
  if ((rc = bfDevEnter(&ds, device))) return rc;
  DevEnv dev;
  rc = envUpload(prob, &dev);
  if (!rc && prob->tgtPoints && prob->layerPot == BFHIP_LAYER_POTENTIAL_PV_NORMAL_DERIV_SINGLE && !prob->tgtNormals)
    rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "S' on a separate target tree needs tgtNormals");
  if (!rc) rc = bfdevHelm2Dense(&dev.env, leafPotCode(prob->layerPot), prob->numPoints, prob->tgtPoints ? prob->numTgtPoints : 0, dX, dY, stream);
  envFree(&dev);
  bfDevLeave(&ds);
  return rc;
}

int bfhipHelm2DenseApply(BfhipHelm2Problem const *prob, int device, void const *X, void *Y) {
  int rc = checkProblem(prob);
  if (rc) return rc;
  if (!X || !Y) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  BfDevScope ds;
  if ((rc = bfDevEnter(&ds, device))) return rc;
  void *dX = NULL, *dY = NULL;
  uint64_t const m = prob->tgtPoints ? prob->numTgtPoints : prob->numPoints;
  rc = bfdevMalloc(&dX, (size_t)(prob->numPoints ? prob->numPoints : 1) * 16);
  if (!rc) rc = bfdevMalloc(&dY, (size_t)(m ? m : 1) * 16);
  if (!rc) rc = bfdevMemcpyH2D(dX, X, (size_t)prob->numPoints * 16);
  if (!rc) rc = bfhipHelm2DenseApplyDevice(prob, -1, dX, dY, NULL);
  if (!rc) rc = bfdevMemcpyD2H(Y, dY, (size_t)m * 16);
  bfdevFree(dX); bfdevFree(dY);
  bfDevLeave(&ds);
  return rc;
}

/* ---- the least-squares solve on caller matrices (include/bfhip_build.h) ---- */
static BfLstSqOpts lstsqOpts(BfhipLstSqOptions const *opts) {
  BfLstSqOpts o = {-1, -1, -1};
  if (opts) { o.qrMin = opts->qrMin; o.gramMin = opts->gramMin; o.forceGlobal = opts->forceGlobal; }
  return bfLstSqResolve(&o);
}

static void publicRoute(BfLstSqRoute const *r, BfhipLstSqRoute *p) {
  p->qr = r->qr; p->qrLdsClass = r->qrLdsClass; p->qrStreaming = r->qrStreaming; p->jacobi = r->jacobi;
  p->w = r->w; p->threads = r->threads; p->ldsClass = r->ldsClass; p->resident = r->resident;
}

static int checkLstSq(uint64_t count, uint32_t const *shapes, BfhipLstSqOptions const *opts) {
  if (count && !shapes) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL shapes");
  if (opts && opts->structSize < sizeof(BfhipLstSqOptions)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BfhipLstSqOptions.structSize too small");
  for (uint64_t i = 0; i < count; ++i)
    if (!shapes[3 * i] || !shapes[3 * i + 1] || !shapes[3 * i + 2])
      return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "least-squares problem %llu: empty shape %u x %u, %u right-hand sides", (unsigned long long)i,
                       shapes[3 * i], shapes[3 * i + 1], shapes[3 * i + 2]);
  return 0;
}

int bfhipLstSqRoutes(uint64_t count, uint32_t const *shapes, uint32_t const *ranks, BfhipLstSqOptions const *opts, BfhipLstSqRoute *routes) {
  int rc = checkLstSq(count, shapes, opts);
  if (rc) return rc;
  if (count && !routes) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL routes");
  BfLstSqOpts const o = lstsqOpts(opts);
  for (uint64_t i = 0; i < count; ++i) {
    uint32_t const mt = shapes[3 * i], me = shapes[3 * i + 1];
    BfLstSqRoute r;
    bfLstSqRoute(mt, me, ranks ? (ranks[i] < me ? ranks[i] : me) : me, &o, &r);
    publicRoute(&r, &routes[i]);
  }
  return 0;
}

static int allFinite(double const *v, uint64_t count) {
  for (uint64_t i = 0; i < count; ++i)
    if (!isfinite(v[i])) return 0;
  return 1;
}

static int cmpDescending(void const *pa, void const *pb) {
  double const a = *(double const *)pa, b = *(double const *)pb;
  return a > b ? -1 : a < b ? 1 : 0;
}

int bfhipLstSqTruncated(uint64_t count, uint32_t const *shapes, void const *A, void const *B, void *X, double *sigma, BfhipLstSqInfo *info,
                        BfhipLstSqOptions const *opts, int device) {
  int rc = checkLstSq(count, shapes, opts);
  if (rc) return rc;
  if (!count) return 0;
  if (!A || !B || !X) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL A / B / X");
  BfLstSqOpts const o = lstsqOpts(opts);
  /* element offsets of every problem's blocks (complex elements; scale and info in their own units) */
  uint64_t *off = calloc(8 * (count + 1), sizeof *off);
  BfLsJob *jobs = malloc(count * sizeof *jobs);
  uint32_t *qrOut = malloc(count * sizeof *qrOut);
  BfLstSqRoute *routes = malloc(count * sizeof *routes);
  uint32_t *hInfo = malloc(3 * count * sizeof *hInfo);
  if (!off || !jobs || !qrOut || !routes || !hInfo) {
    free(off); free(jobs); free(qrOut); free(routes); free(hInfo);
    return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (least squares)");
  }
  enum { OA, OB, OX, OV, OQ, OT, OS, OI };
  for (uint64_t i = 0; i < count; ++i) {
    uint64_t const mt = shapes[3 * i], me = shapes[3 * i + 1], n = shapes[3 * i + 2];
    uint64_t *c = off + 8 * i, *nx = off + 8 * (i + 1);
    nx[OA] = c[OA] + mt * me; nx[OB] = c[OB] + mt * n; nx[OX] = c[OX] + me * n; nx[OV] = c[OV] + me * me;
    nx[OQ] = c[OQ] + ((int64_t)me >= o.qrMin && bfQrcpLds((uint32_t)mt, (uint32_t)me) ? me * me : 0);
    nx[OT] = c[OT] + me * n; nx[OS] = c[OS] + me; nx[OI] = c[OI] + 3;
  }
  uint64_t const *tot = off + 8 * count;
  void *dA = NULL, *dB = NULL, *dX = NULL, *dV = NULL, *dQ = NULL, *dT = NULL, *dS = NULL, *dI = NULL;
  BfDevScope ds = {0};
  if ((rc = bfDevEnter(&ds, device))) goto done;
  if ((rc = bfdevMalloc(&dA, tot[OA] * 16)) || (rc = bfdevMalloc(&dB, tot[OB] * 16)) || (rc = bfdevMalloc(&dX, tot[OX] * 16)) ||
      (rc = bfdevMalloc(&dV, tot[OV] * 16)) || (rc = bfdevMalloc(&dQ, (tot[OQ] ? tot[OQ] : 1) * 16)) || (rc = bfdevMalloc(&dT, tot[OT] * 16)) ||
      (rc = bfdevMalloc(&dS, tot[OS] * 8)) || (rc = bfdevMalloc(&dI, tot[OI] * 4)))
    goto done;
  if ((rc = bfdevMemcpyH2D(dA, A, tot[OA] * 16)) || (rc = bfdevMemcpyH2D(dB, B, tot[OB] * 16)) || (rc = bfdevMemset(dI, 0, tot[OI] * 4)) ||
      (rc = bfdevMemset(dS, 0, tot[OS] * 8)))
    goto done;
  for (uint64_t i = 0; i < count; ++i) {
    uint64_t const *c = off + 8 * i;
    BfLsJob *J = &jobs[i];
    J->a = (char *)dA + c[OA] * 16; J->b = (char *)dB + c[OB] * 16; J->out = (char *)dX + c[OX] * 16; J->v = (char *)dV + c[OV] * 16;
    J->xq = (char *)dQ + c[OQ] * 16; J->t = (char *)dT + c[OT] * 16; J->scale = (double *)dS + c[OS]; J->info = (uint32_t *)dI + c[OI];
    J->mt = shapes[3 * i]; J->me = shapes[3 * i + 1]; J->n = shapes[3 * i + 2]; J->dim = J->mt > J->me ? J->mt : J->me;
  }
  BfhipBuildStats st;
  memset(&st, 0, sizeof st);
  if ((rc = lstsqSolve(jobs, count, &o, &st, qrOut, routes, 0))) goto done;
  if ((rc = bfdevMemcpyD2H(X, dX, tot[OX] * 16)) || (rc = bfdevMemcpyD2H(hInfo, dI, tot[OI] * 4))) goto done;
  if (sigma) {
    if ((rc = bfdevMemcpyD2H(sigma, dS, tot[OS] * 8))) goto done;
    /* scale[j] = 1 / sigma_j^2 for the kept ones, 0 else -> kept sigma, descending, zero padded */
    for (uint64_t i = 0; i < count; ++i) {
      double *sg = sigma + off[8 * i + OS];
      uint32_t const me = shapes[3 * i + 1];
      for (uint32_t j = 0; j < me; ++j) sg[j] = sg[j] > 0.0 ? sqrt(1.0 / sg[j]) : 0.0;
      qsort(sg, me, sizeof *sg, cmpDescending);
    }
  }
  if (info) {
    double const *b = B;
    for (uint64_t i = 0; i < count; ++i) {
      BfhipLstSqInfo *f = &info[i];
      uint32_t const *h = hInfo + 3 * i;
      publicRoute(&routes[i], &f->route);
      f->sweeps = h[0]; f->rank = h[2];
      f->qrRank = qrOut[i] & ~BF_QR_NONFINITE;
      /* B enters only the GEMMs: a NaN there reaches X unless the rank is 0, so it is looked for here */
      f->notConverged = h[1] || (qrOut[i] & BF_QR_NONFINITE) || !allFinite(b + 2 * off[8 * i + OB], 2 * (off[8 * (i + 1) + OB] - off[8 * i + OB]));
    }
  }
done:
  bfdevFree(dA); bfdevFree(dB); bfdevFree(dX); bfdevFree(dV); bfdevFree(dQ); bfdevFree(dT); bfdevFree(dS); bfdevFree(dI);
  bfDevLeave(&ds);
  free(off); free(jobs); free(qrOut); free(routes); free(hInfo);
  return rc;
}
