/* bfhip_api.c -- the C-ABI of include/bfhip.h: errors, operator lifetime, compile (IR -> plan -> HBM), profiling and
 * apply.  The other parts of the ABI that work on struct BfhipOperator (bfhip_operator.h) are bfhip_file.c (save / load),
 * bfhip_shim.c (the BfMat vtable shim) and bfhip_inspect.c (plan inspection, kernel names).
 */
#define _GNU_SOURCE
#include "bfhip_operator.h"
#include "../../include/bfhip_abi.h"
#include "../../include/bfhip_synth.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

/* ---- errors ----------------------------------------------------------------- */
static __thread char lastError[512];

int bfhipFail(int code, char const *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(lastError, sizeof lastError, fmt, ap);
  va_end(ap);
  return code;
}
char const *bfhipLastErrorMessage(void) { return lastError; }
char const *bfhipErrorString(int code) {
  static char const *const names[] = {"BF_ERROR_NONE", "BF_ERROR_INVALID_ARGUMENTS", "BF_ERROR_RUNTIME_ERROR",
                                      "BF_ERROR_NOT_IMPLEMENTED", "BF_ERROR_MEMORY_ERROR", "BF_ERROR_OUT_OF_RANGE",
                                      "BF_ERROR_FILE_ERROR", "BF_ERROR_TYPE_ERROR", "BF_ERROR_INCOMPATIBLE_SHAPES"};
  return (code >= 0 && code <= 8) ? names[code] : "BF_ERROR_UNKNOWN";
}

double bfhipSyntheticValue(uint64_t seed, uint64_t idx, int imag) { return bfhip_synth_value(seed, idx, imag); }

int bfhipSyntheticLeafBases(BfhipDesc const *desc, uint64_t *bases) {
  if (!desc || !bases) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  uint64_t acc = 0;
  for (uint64_t i = 0; i < desc->numNodes; ++i) {
    bases[i] = acc;
    if (desc->kind[i] == BFHIP_NODE_DENSE) acc += desc->rows[i] * desc->cols[i];
  }
  return 0;
}

/* ---- operator --------------------------------------------------------------- */
static void freeDevicePlanOf(BfPlan *plan) {
  for (uint64_t s = 0; s < plan->numStages && plan->stages; ++s) {
    BfStage *st = &plan->stages[s];
    bfdevFree(st->dItems); st->dItems = NULL;
    bfdevFree(st->dPieces); st->dPieces = NULL;
    bfdevFree(st->dTickets); st->dTickets = NULL;
    for (uint64_t r = 0; r < st->numReduce; ++r) {
      bfdevFree(st->reduce[r].dRowInterval); bfdevFree(st->reduce[r].dIvBegin); bfdevFree(st->reduce[r].dSrcBias);
      st->reduce[r].dRowInterval = st->reduce[r].dIvBegin = st->reduce[r].dSrcBias = NULL;
    }
  }
}
static void freeDevicePlan(BfhipOperator *op) {
  freeDevicePlanOf(&op->plan);
  freeDevicePlanOf(&op->tplan);
}

void bfhipFree(BfhipOperator **pop) {
  if (!pop || !*pop) return;
  BfhipOperator *op = *pop;
  BfDevScope ds;
  bfDevEnter(&ds, (op->flags & BFHIP_FLAG_PLAN_ONLY) ? -1 : op->device);      /* a plan-only operator never touched a device */
  if (op->extractRelease) op->extractRelease(op->extract);
  if (op->evStart && op->evStop) for (uint64_t s = 0; s < BF_EV_POOL * op->plan.numStages; ++s) { bfdevEventDestroy(op->evStart[s]); bfdevEventDestroy(op->evStop[s]); }
  free(op->evStart); free(op->evStop); free(op->stageMs); free(op->stageLaunches);
  freeDevicePlan(op);
  bfdevFree(op->dArena);
  bfdevFree(op->dArenaT);
  bfdevFree(op->dTemp);
  bfdevFree(op->dZero);
  bfdevFree(op->dFlowItems); bfdevFree(op->dFlowPieces); bfdevFree(op->dFlowItemOut); bfdevFree(op->dFlowWriters); bfdevFree(op->dFlowCounters);
  bfdevFree(op->dX);
  bfdevFree(op->dCov);
  bfdevFree(op->dY);
  bfdevHostFreePinned(op->hX);
  bfdevHostFreePinned(op->hY);
  for (int i = 0; i < 4; ++i) bfdevEventDestroy(op->evHost[i]);
  bfPlanFree(&op->plan);
  bfPlanFree(&op->tplan);
  if (op->ir) { bfIrFree(op->ir); free(op->ir); }
  if (op->irT) { bfIrFree(op->irT); free(op->irT); }
  free(op);
  *pop = NULL;
  bfDevLeave(&ds);
}

static int uploadArray(void **d, void const *h, size_t bytes, uint64_t *meta) {
  int rc = bfdevMalloc(d, bytes);
  if (rc) return rc;
  *meta += bytes;
  return bfdevMemcpyH2D(*d, h, bytes);
}

/* write one piece (mr x ncols sub-block of a leaf, column-major, rows padded
 * to mrPad) at dst */
static int packPiece(BfPlan const *pl, BfIr const *ir, BfDevPiece const *pc, BfPieceSrc const *src,
                      uint32_t mr, uint32_t mrPad, unsigned char *dst, uint64_t seed) {
  if (pl->dtype == BFHIP_C64) {
    /* complex64: the piece is packed in complex128 (decorations added in double), then each component is rounded once; the
     * device synthesizer (bfSynthKernel<BFHIP_C64>) rounds the same double values */
    size_t const elems = (pc->flags & BF_PIECE_ROWMAJOR) ? (size_t)mr * pc->ld : (size_t)mrPad * pc->ncols;
    double *wide = malloc(elems * 16 + 16);
    if (!wide) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (complex64 packing)");
    BfPlan wp = *pl;
    wp.dtype = BFHIP_C128;
    int const rc = packPiece(&wp, ir, pc, src, mr, mrPad, (unsigned char *)wide, seed);
    if (!rc) for (size_t k = 0; k < 2 * elems; ++k) ((float *)dst)[k] = (float)wide[k];
    free(wide);
    return rc;
  }
  uint64_t node = src->node;
  void const *data = ir->leafData[node];
  int const cplx = pl->dtype == BFHIP_C128;
  uint64_t ldr = ir->leafRowStride[node], ldc = ir->leafColStride[node];
  double const *A = (double const *)data;
  double scale = 0;
  /* synthetic leaves: element (i, j) of the ORIGINAL leaf is stream value base + i * n + j, n its column count; the leaves of a
   * transposed view (bfIrTransposed) hold element (j, i) of it */
  uint64_t vbase = ir->synthBase[node], n = ir->transposedView ? ir->rows[node] : ir->cols[node];
  uint64_t const sR = ir->transposedView ? 1 : n, sC = ir->transposedView ? n : 1;
  if (!data) scale = cplx ? sqrt(3.0 / (2.0 * (double)n)) : sqrt(3.0 / (double)n);
  int const rowMajor = (pc->flags & BF_PIECE_ROWMAJOR) != 0;      /* real dtypes only */
  uint32_t const rowsStored = rowMajor ? mr : mrPad;
  for (uint32_t c = 0; c < pc->ncols; ++c) {
    for (uint32_t r = 0; r < rowsStored; ++r) {
      double re = 0, im = 0;
      if (r < mr) {
        uint64_t i = src->row0 + r, j = src->col0 + c;
        if (data) {
          if (cplx && !(ir->leafReal[node] & BF_LEAF_REAL)) { double const *e = A + 2 * (i * ldr + j * ldc); re = e[0]; im = (ir->leafReal[node] & BF_LEAF_CONJ) ? -e[1] : e[1]; }
          else re = A[i * ldr + j * ldc];
        } else {
          re = bfhip_synth_value(seed, vbase + i * sR + j * sC, 0) * scale;
          if (cplx) im = bfhip_synth_value(seed, vbase + i * sR + j * sC, 1) * scale;
        }
      }
      uint64_t e = rowMajor ? (uint64_t)r * pc->ld + c : (uint64_t)c * mrPad + r;
      if (cplx) { ((double *)dst)[2 * e] = re; ((double *)dst)[2 * e + 1] = im; }
      else if (pl->dtype == BFHIP_F64) ((double *)dst)[e] = re;
      else ((float *)dst)[e] = (float)re;
    }
  }
  if (rowMajor)      /* the row ends are padded to the lane granule with zeros */
    for (uint32_t r = 0; r < mr; ++r)
      for (uint32_t c = pc->ncols; c < pc->ld; ++c) {
        uint64_t e = (uint64_t)r * pc->ld + c;
        if (cplx) ((double *)dst)[2 * e] = ((double *)dst)[2 * e + 1] = 0;
        else if (pl->dtype == BFHIP_F64) ((double *)dst)[e] = 0; else ((float *)dst)[e] = 0;
      }
  /* sparse decorations folded into this leaf (bfhip_ir.c: tryFold): patches are sorted by (leaf, row, col) */
  if (ir->numPatches && data) {
    uint64_t lo = 0, hi = ir->numPatches;
    while (lo < hi) { uint64_t mid = (lo + hi) / 2; if (ir->patches[mid].leaf < node || (ir->patches[mid].leaf == node && ir->patches[mid].row < src->row0)) lo = mid + 1; else hi = mid; }
    for (; lo < ir->numPatches && ir->patches[lo].leaf == node && ir->patches[lo].row < src->row0 + mr; ++lo) {
      BfIrPatch const *pt = &ir->patches[lo];
      if (pt->col < src->col0 || pt->col >= src->col0 + pc->ncols) continue;
      uint64_t e = rowMajor ? (uint64_t)(pt->row - src->row0) * pc->ld + (pt->col - src->col0) : (uint64_t)(pt->col - src->col0) * mrPad + (pt->row - src->row0);
      if (cplx) { ((double *)dst)[2 * e] += pt->re; ((double *)dst)[2 * e + 1] += pt->im; }
      else if (pl->dtype == BFHIP_F64) ((double *)dst)[e] += pt->re;
      else ((float *)dst)[e] = (float)((double)((float *)dst)[e] + pt->re);
    }
  }
  return 0;
}

/* pack leaves into the arena, stage by stage, in arena order.  hostDst != NULL:
 * write everything (synthetic leaves included) to host memory; else upload
 * host-valued leaves through a staging buffer and synthesize the rest on the
 * device. */
int packLeavesPlan(BfPlan const *pl, void *dArena, BfIr const *ir, uint64_t seed, void *hostDst) {
  size_t const es = pl->elemSize;
  int const cplx = bfDtypeComplex(pl->dtype);
  size_t const chunkBytes = (size_t)64 << 20;
  unsigned char *stage = NULL;
  BfSynthPiece *synth = NULL;
  uint64_t numSynth = 0, capSynth = 0;
  int rc = 0;
  uint64_t chunkBase = 0;    /* arena element offset of stage[0] */
  size_t fill = 0;           /* bytes used in stage */
  for (uint64_t s = 0; s < pl->numStages && !rc; ++s) {
    BfStage const *st = &pl->stages[s];
    for (uint64_t i = 0; i < st->numItems && !rc; ++i) {
      BfDevItem const *it = &st->items[i];
      uint32_t mr = it->mrFlags & 0xffffu;
      uint32_t mrPad = (mr + pl->epl - 1) / pl->epl * pl->epl;
      for (uint32_t k = 0; k < it->numPieces && !rc; ++k) {
        BfDevPiece const *pc = &st->pieces[it->pieceBegin + k];
        BfPieceSrc const *src = &st->pieceSrc[it->pieceBegin + k];
        if (pc->flags & BF_PIECE_IDENTITY) continue;
        uint64_t node = src->node;
        size_t bytes = ((pc->flags & BF_PIECE_ROWMAJOR) ? (size_t)mr * pc->ld : (size_t)mrPad * pc->ncols) * es;
        if (hostDst) {
          if ((rc = packPiece(pl, ir, pc, src, mr, mrPad, (unsigned char *)hostDst + pc->dataOff * es, seed))) break;
          continue;
        }
        if (!ir->leafData[node]) {
          if (numSynth == capSynth) {
            capSynth = capSynth ? capSynth * 2 : 4096;
            BfSynthPiece *p = realloc(synth, capSynth * sizeof *synth);
            if (!p) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (synth pieces)"); break; }
            synth = p;
          }
          BfSynthPiece *sp = &synth[numSynth++];
          sp->dataOff = pc->dataOff;
          sp->vbase = ir->synthBase[node];
          uint64_t const ncol = ir->transposedView ? ir->rows[node] : ir->cols[node];      /* columns of the leaf the stream was laid over */
          sp->strideR = ir->transposedView ? 1u : (uint32_t)ncol;
          sp->strideC = ir->transposedView ? (uint32_t)ncol : 1u;
          sp->row0 = src->row0; sp->col0 = src->col0;
          sp->mr = mr; sp->mrPad = mrPad; sp->ncols = pc->ncols;
          sp->rowMajor = (pc->flags & BF_PIECE_ROWMAJOR) != 0; sp->ldr = pc->ld;
          sp->scale = cplx ? sqrt(3.0 / (2.0 * (double)ncol)) : sqrt(3.0 / (double)ncol);
          continue;
        }
        if (!stage) {
          stage = malloc(chunkBytes);
          if (!stage) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (staging)"); break; }
          chunkBase = pc->dataOff; fill = 0;
        }
        /* pieces are consecutive in the arena except across synthetic ones */
        if (fill && (pc->dataOff != chunkBase + fill / es || fill + bytes > chunkBytes)) {
          rc = bfdevMemcpyH2D((char *)dArena + chunkBase * es, stage, fill);
          fill = 0;
          if (rc) break;
        }
        if (!fill) chunkBase = pc->dataOff;
        if (bytes > chunkBytes) { rc = bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "piece larger than staging chunk"); break; }
        if ((rc = packPiece(pl, ir, pc, src, mr, mrPad, stage + fill, seed))) break;
        fill += bytes;
      }
    }
  }
  if (!rc && fill) rc = bfdevMemcpyH2D((char *)dArena + chunkBase * es, stage, fill);
  free(stage);
  if (!rc && numSynth) rc = bfdevSynthFill(dArena, pl->dtype, synth, numSynth, seed);
  free(synth);
  return rc;
}

static int packLeaves(BfhipOperator const *op, BfIr const *ir, uint64_t seed, void *hostDst) {
  return packLeavesPlan(&op->plan, op->dArena, ir, seed, hostDst);
}

static int uploadPlanMeta(BfhipOperator *op, BfPlan *plan) {
  int rc = 0;
  for (uint64_t s = 0; s < plan->numStages && !rc; ++s) {
    BfStage *st = &plan->stages[s];
    rc = uploadArray(&st->dItems, st->items, st->numItems * sizeof(BfDevItem), &op->metaBytes);
    if (!rc) rc = uploadArray(&st->dPieces, st->pieces, st->numPieces * sizeof(BfDevPiece), &op->metaBytes);
    for (uint64_t r = 0; r < st->numReduce && !rc; ++r) {
      BfReduce *rd = &st->reduce[r];
      rc = uploadArray(&rd->dRowInterval, rd->rowInterval, rd->numRows * 4, &op->metaBytes);
      if (!rc) rc = uploadArray(&rd->dIvBegin, rd->ivBegin, (rd->numIntervals + 1) * 4, &op->metaBytes);
      if (!rc) rc = uploadArray(&rd->dSrcBias, rd->srcBias, rd->numSrc * 8, &op->metaBytes);
    }
  }
  return rc;
}

static void dropPlanMirrors(BfPlan *plan) {
  for (uint64_t s = 0; s < plan->numStages && plan->stages; ++s) {
    BfStage *st = &plan->stages[s];
    free(st->pieceSrc); st->pieceSrc = NULL;
    free(st->pieces); st->pieces = NULL;
    free(st->items); st->items = NULL;
    free(st->bundleBegin); st->bundleBegin = NULL;
    free(st->pieceBuf); st->pieceBuf = NULL;
    free(st->itemBuf); st->itemBuf = NULL;
    for (uint64_t r = 0; r < st->numReduce; ++r) {
      free(st->reduce[r].rowInterval); st->reduce[r].rowInterval = NULL;
      free(st->reduce[r].ivBegin); st->reduce[r].ivBegin = NULL;
      free(st->reduce[r].srcBias); st->reduce[r].srcBias = NULL;
    }
  }
}


#ifdef BFHIP_EXPERIMENTAL      /* the dependency-driven launch lives in `make experimental` builds only (bfhip_experimental.hip) */
/* Flat index tables for the dependency-driven launch (bfFlowKernelC128): all stages' items in stage order with global
 * piece indices, pieces carrying the id of the vector they read, per item the vector it writes, per vector its number
 * of writers, and the counters.  Needs the host mirrors of the plan. */
static int buildFlow(BfhipOperator *op, int hostOnly) {
  BfPlan const *pl = &op->plan;
  uint64_t ni = 0, np = 0;
  for (uint64_t s = 0; s < pl->numStages; ++s) { ni += pl->stages[s].numItems; np += pl->stages[s].numPieces; }
  if (!ni || ni >= 0x7fffffffu || np >= 0xffffffffu) return 0;       /* nothing to run / too large for 32-bit tickets: staged launches */
  BfDevItem *items = malloc(ni * sizeof *items);
  BfDevPiece *pieces = malloc((np ? np : 1) * sizeof *pieces);
  uint32_t *itemOut = malloc(ni * 4);
  int rc = 0;
  if (!items || !pieces || !itemOut) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (flow tables)"); goto done; }
  uint64_t i0 = 0, p0 = 0;
  for (uint64_t s = 0; s < pl->numStages; ++s) {
    BfStage const *st = &pl->stages[s];
    for (uint64_t i = 0; i < st->numItems; ++i) {
      items[i0 + i] = st->items[i];
      items[i0 + i].pieceBegin = (uint32_t)(p0 + st->items[i].pieceBegin);
      itemOut[i0 + i] = st->itemBuf[i];
    }
    for (uint64_t k = 0; k < st->numPieces; ++k) {
      pieces[p0 + k] = st->pieces[k];
      pieces[p0 + k].ld = st->pieceBuf[k];          /* column-major complex pieces do not use `ld` */
      if (st->pieceBuf[k]) {                        /* the number of writers of that vector rides above the flag bits */
        if (pl->bufWriters[st->pieceBuf[k]] >= (1u << 24)) { rc = 0; goto done; }      /* (never: a vector has one writer per <= 64 of its rows) -> staged launches */
        pieces[p0 + k].flags |= pl->bufWriters[st->pieceBuf[k]] << 8;
      }
    }
    i0 += st->numItems; p0 += st->numPieces;
  }
  uint32_t maxW = 1;
  for (uint64_t b = 0; b < pl->numBufs; ++b) if (pl->bufWriters[b] > maxW) maxW = pl->bufWriters[b];
  {
    /* The launch drains iff the list, walked in ticket order by ONE worker, never waits: every vector a piece reads has
     * been written completely by items earlier in the list.  Checked here, once, on the host. */
    uint32_t *seen = calloc(pl->numBufs + 1, 4);
    if (!seen) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (flow tables)"); goto done; }
    for (uint64_t i = 0; i < ni && !rc; ++i) {
      for (uint32_t k = 0; k < items[i].numPieces; ++k) {
        uint32_t const dep = pieces[items[i].pieceBegin + k].ld;
        if (dep >= pl->numBufs || (dep && (dep < 2 || !pl->bufWriters[dep] || seen[dep] != pl->bufWriters[dep]))) {
          rc = bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "internal: item %llu reads vector %u before it is complete (%u of %u writers)", (unsigned long long)i, dep,
                         dep < pl->numBufs ? seen[dep] : 0, dep < pl->numBufs ? pl->bufWriters[dep] : 0);
          break;
        }
      }
      if (itemOut[i] >= pl->numBufs || itemOut[i] == 1) rc = bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "internal: item %llu writes vector %u", (unsigned long long)i, itemOut[i]);
      else if (itemOut[i]) ++seen[itemOut[i]];
    }
    free(seen);
    if (rc) goto done;
  }
  uint64_t const nb = pl->numBufs < 2 ? 2 : pl->numBufs;
  if (hostOnly) { op->flow = 1; goto done; }        /* plan-only operators: the tables are built and checked, nothing is uploaded */
  if ((rc = uploadArray(&op->dFlowItems, items, ni * sizeof *items, &op->metaBytes))) goto done;
  if ((rc = uploadArray(&op->dFlowPieces, pieces, (np ? np : 1) * sizeof *pieces, &op->metaBytes))) goto done;
  if ((rc = uploadArray(&op->dFlowItemOut, itemOut, ni * 4, &op->metaBytes))) goto done;
  {
    uint32_t *w = calloc(nb, 4);
    if (!w) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (flow tables)"); goto done; }
    memcpy(w, pl->bufWriters, pl->numBufs * 4);
    rc = uploadArray(&op->dFlowWriters, w, nb * 4, &op->metaBytes);
    free(w);
    if (rc) goto done;
  }
  if ((rc = bfdevMalloc(&op->dFlowCounters, nb * 4))) goto done;
  if ((rc = bfdevMemset(op->dFlowCounters, 0, nb * 4))) goto done;
  if ((rc = bfdevFlowGrid(ni, &op->flowGrid))) goto done;
  op->flowNumItems = (uint32_t)ni; op->flowNumBufs = nb; op->flowMaxWriters = maxW;
  op->flowEpoch = 0; op->flowQueueBase = 0;
  op->flow = 1;
done:
  free(items); free(pieces); free(itemOut);
  return rc;
}
#endif

static int ensureTemp(BfhipOperator *op, uint32_t nrhs) {
  if (op->dTemp && op->tempRhs >= nrhs) return 0;
  bfdevFree(op->dTemp);
  op->dTemp = NULL;
  op->tempRhs = 0;
  uint64_t te = op->plan.tempElems > op->tplan.tempElems ? op->plan.tempElems : op->tplan.tempElems;
  int rc = bfdevMalloc(&op->dTemp, (size_t)te * nrhs * op->plan.elemSize);
  if (rc) return rc;
  op->tempRhs = nrhs;
  return 0;
}

/* what compile and load end with: the vector arena for maxRhs right-hand sides (0: one), the zero buffer and, under
 * BFHIP_FLAG_PROFILE, the per-stage timing arrays and the event pool */
int finishOperator(BfhipOperator *op, uint32_t maxRhs) {
  int rc;
  if ((rc = ensureTemp(op, maxRhs ? maxRhs : 1))) return rc;
  if ((rc = bfdevMalloc(&op->dZero, 4096))) return rc;
  if ((rc = bfdevMemset(op->dZero, 0, 4096))) return rc;
  if (op->flags & BFHIP_FLAG_PROFILE) {
    uint64_t S = op->plan.numStages;
    op->evStart = calloc(BF_EV_POOL * S, sizeof(void *));
    op->evStop = calloc(BF_EV_POOL * S, sizeof(void *));
    op->stageMs = calloc(S, sizeof(double));
    op->stageLaunches = calloc(S, sizeof(uint64_t));
    if (!op->evStart || !op->evStop || !op->stageMs || !op->stageLaunches) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
    for (uint64_t s = 0; s < BF_EV_POOL * S && !rc; ++s) {
      rc = bfdevEventCreate(&op->evStart[s]);
      if (!rc) rc = bfdevEventCreate(&op->evStop[s]);
    }
  }
  return rc;
}

/* The adjoint plan over the forward plan's packed leaves (BFHIP_FLAG_ADJOINT): index metadata only.  Needs the forward plan's
 * host mirrors.  Row-range / row-block shards: the transposed plan of the shard's own tasks (bfPlanBuild prunes the same way). */
static int buildSharedTplan(BfhipOperator *op, BfIr const *ir, BfPlanOptions const *po) {
  BfFwdPiece *fwd = NULL;
  uint64_t nf = 0;
  int rc = bfPlanFwdPieces(&op->plan, &fwd, &nf);
  if (rc) return rc;
  BfPlanOptions pt = *po;
  pt.itemsWanted = 0;
  pt.fwdPieces = fwd;
  pt.numFwdPieces = nf;
  pt.tCols = 0;      /* item width (16 or 64 columns of A) chosen stage by stage */
  rc = bfPlanBuild(ir, &pt, &op->tplan);
  free(fwd);
  if (!rc) { op->hasTplan = 1; op->packedT = 0; }
  return rc;
}

int bfhipCompileIrFill(BfIr *ir, BfhipOptions const *opts, BfFillFn fill, void *fillCtx, BfhipOperator **out) {
  BfhipOptions o;
  memset(&o, 0, sizeof o);
  o.device = -1;
  if (opts) {
    if (opts->structSize < BFHIP_OPTIONS_SIZE_V1) { bfIrFree(ir); return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BfhipOptions.structSize too small"); }
    memcpy(&o, opts, opts->structSize < sizeof o ? opts->structSize : sizeof o);      /* fields a shorter (older) struct lacks stay 0 */
  }
  BfhipOperator *op = calloc(1, sizeof *op);
  if (!op) { bfIrFree(ir); return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); }
  int rc = 0;
  BfDevScope ds = {0};
  int const planOnly = (o.flags & BFHIP_FLAG_PLAN_ONLY) != 0;
  BfIr irT;                      /* the transposed expression of a packed adjoint plan: released under `done` on every path */
  memset(&irT, 0, sizeof irT);
  op->flags = o.flags;
  op->seed = o.seed;
#ifndef BFHIP_EXPERIMENTAL
  if (o.flags & BFHIP_FLAG_FLOW) {
    rc = bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "BFHIP_FLAG_FLOW: this library was built without the experimental executors (make -C butterfly_amd/csrc experimental)");
    goto done;
  }
#endif
  if (!planOnly) {
    if ((rc = bfDevEnter(&ds, o.device))) goto done;
    if ((rc = bfdevGetDevice(&op->device))) goto done;      /* o.device may be -1: the operator lives on the current device */
  }
  op->srcDtype = ir->dtype;
  BfPlanOptions po;
  memset(&po, 0, sizeof po);
  po.storeDtype = ir->dtype;
  if (o.demoteToF32) po.storeDtype = ir->dtype == BFHIP_C128 ? BFHIP_C64 : BFHIP_F32;
  po.groupByInput = o.maxRhs >= 3;
#ifndef BF_MIN_CHUNK_ROWS
#define BF_MIN_CHUNK_ROWS 16     /* lower bound of the adaptive item height, in 16-byte row units (A/B builds: 8) */
#endif
  po.minChunkRows = o.maxRhs >= 3 ? 32 : BF_MIN_CHUNK_ROWS;   /* operators compiled for RHS blocks run on the matrix-core kernel */
  po.rowBlockBegin = o.rowBlockBegin;
  po.rowAlignBytes = 128;      /* rows of row-major pieces on 128-byte lines: the forward kernel gains 1 - 3 % on them, the transposed one 3 % */
  po.rowBlockEnd = o.rowBlockEnd;
  po.rowBegin = o.rowBegin;
  po.rowEnd = o.rowEnd;
  if ((rc = bfPlanBuild(ir, &po, &op->plan))) goto done;
  op->leafBytesAlgorithmic = op->plan.leafElems * op->plan.elemSize;
  /* The adjoint plan.  BFHIP_FLAG_ADJOINT_PACKED: a FORWARD plan of the transposed expression over its own packed copy of the
   * leaves (twice the leaf memory; A^T x then runs on the forward kernels at the forward rate).  Not with a caller-side
   * value builder (its values exist in the forward arena only) and not plan-only: those get the shared-leaf plan below. */
  /* (a row shard's adjoint is the shared-leaf plan as well: its input is the shard's rows of v, its transposed expression would have
   *  to be pruned by COLUMNS -- bfPlanBuild prunes the transposed task list instead, pruneToRowRangeT) */
  int packedT = (o.flags & BFHIP_FLAG_ADJOINT_PACKED) && !fill && !(po.rowEnd > 0 || po.rowBlockEnd > 0);
  if (packedT) {
    if ((rc = bfIrTransposed(ir, &irT))) goto done;
    BfPlanOptions pt = po;
    /* The block columns of a real (streamed) butterfly are long -- hundreds of leaves -- and the 1 MiB item cap leaves a stage of
     * the transposed expression with ~8000 items for 4096 wavefront slots: two uneven rounds.  Cutting them for >= 32768 items
     * per stage (N = 1M fp32: 8.66 -> 8.08 ms; 16384: 8.25, 65536: 8.15) costs nothing but a few more partial sums.  Complex
     * (fac_helm2) plans keep 4096: their stages are 10 GB, the cap binds either way and more items measured 1-2 % slower, as did
     * more items in the FORWARD plan of either operand (DESIGN_EXPERIMENTS.md section 10). */
    if (!bfDtypeC128Layout(op->plan.dtype)) pt.itemsWanted = 32768;
    if ((rc = bfPlanBuild(&irT, &pt, &op->tplan))) goto done;
    op->hasTplan = 1;
    op->packedT = 1;
    if (planOnly) {          /* kept for bfhipPlanPackArenaT */
      op->irT = malloc(sizeof *op->irT);
      if (!op->irT) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); goto done; }
      *op->irT = irT;
      memset(&irT, 0, sizeof irT);
    }
  } else if (o.flags & (BFHIP_FLAG_ADJOINT | BFHIP_FLAG_ADJOINT_PACKED)) {
    if ((rc = buildSharedTplan(op, ir, &po))) goto done;
  }
  if (planOnly) {
#ifdef BFHIP_EXPERIMENTAL
    if (op->plan.dtype == BFHIP_C128 && op->plan.flowOk && (o.flags & BFHIP_FLAG_FLOW) && (rc = buildFlow(op, 1))) goto done;
#endif
    /* keep the IR (with its borrowed leaf pointers) for bfhipPlanPackArena */
    op->ir = malloc(sizeof *op->ir);
    if (!op->ir) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); goto done; }
    *op->ir = *ir;
    memset(ir, 0, sizeof *ir);
    *out = op;
    return 0;
  }

  /* + 256 B of slack: no kernel reads past the last piece by construction, the slack keeps a
   * future mistake there off the end of the mapping */
  if ((rc = bfdevMalloc(&op->dArena, (size_t)op->plan.arenaElems * op->plan.elemSize + BF_ARENA_SLACK))) goto done;
  if ((rc = uploadPlanMeta(op, &op->plan))) goto done;
  if (op->hasTplan && (rc = uploadPlanMeta(op, &op->tplan))) goto done;
  /* leaf values: computed on the device by the caller's builder, or packed / synthesized from the IR */
  if ((rc = fill ? fill(&op->plan, ir, op->dArena, fillCtx) : packLeaves(op, ir, o.seed, NULL))) goto done;
  if (packedT) {
    rc = bfdevMalloc(&op->dArenaT, (size_t)op->tplan.arenaElems * op->tplan.elemSize + BF_ARENA_SLACK);
    if (rc == BFABI_ERROR_MEMORY_ERROR) {
      /* no room for a second copy of the leaves (the flag doubles the leaf memory): the adjoint degrades to the shared-leaf plan
       * on the transposed kernels instead of failing the compile */
      op->dArenaT = NULL;
      freeDevicePlanOf(&op->tplan);
      bfPlanFree(&op->tplan);
      op->hasTplan = 0; op->packedT = 0; packedT = 0;
      if ((rc = buildSharedTplan(op, ir, &po))) goto done;
      if ((rc = uploadPlanMeta(op, &op->tplan))) goto done;
    } else {
      if (!rc) rc = packLeavesPlan(&op->tplan, op->dArenaT, &irT, o.seed, NULL);
      if (rc) goto done;
    }
  }
#ifdef BFHIP_EXPERIMENTAL
  {
    char const *envFlow = getenv("BFHIP_FLOW");         /* A/B switch for whole programs; BFHIP_FLAG_FLOW is the per-operator one */
    if (op->plan.dtype == BFHIP_C128 && op->plan.flowOk && ((o.flags & BFHIP_FLAG_FLOW) || (envFlow && envFlow[0] == '1')) && (rc = buildFlow(op, 0))) goto done;
  }
  /* the persistent ticket launch (BFHIP_PERSISTENT=1): every stage's counters exist before the first apply, so that an
   * apply never allocates or synchronises (a sharded step must not fail on ONE rank after its peers entered the collective) */
  if (op->plan.dtype == BFHIP_C128 && bfdevPersistentGrid()) {
    for (uint64_t s_ = 0; s_ < op->plan.numStages; ++s_) {
      BfStage *st_ = &op->plan.stages[s_];
      if ((rc = bfdevMalloc(&st_->dTickets, BF_TICKET_POOLS * BF_TICKET_STRIDE * 4))) goto done;
      if ((rc = bfdevMemset(st_->dTickets, 0, BF_TICKET_POOLS * BF_TICKET_STRIDE * 4))) goto done;
    }
    if ((rc = bfdevSync(NULL))) goto done;
  }
#endif
  /* host mirrors of the bulky per-piece arrays are no longer needed */
  dropPlanMirrors(&op->plan);
  dropPlanMirrors(&op->tplan);
  if ((rc = finishOperator(op, o.maxRhs))) goto done;
done:
  bfIrFree(ir);
  bfIrFree(&irT);
  if (rc) bfhipFree(&op);
  bfDevLeave(&ds);
  if (rc) return rc;
  *out = op;
  return 0;
}

int bfhipCompile(void const *bfMat, BfhipOptions const *opts, BfhipOperator **out) {
  if (!bfMat || !out) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  *out = NULL;
  BfIr ir;
  int rc = bfIrFromBfMat(bfMat, &ir);
  if (rc) return rc;
  return bfhipCompileIrFill(&ir, opts, NULL, NULL, out);
}

int bfhipCompileDesc(BfhipDesc const *desc, BfhipOptions const *opts, BfhipOperator **out) {
  if (!desc || !out) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  *out = NULL;
  BfIr ir;
  int rc = bfIrFromDesc(desc, &ir);
  if (rc) return rc;
  return bfhipCompileIrFill(&ir, opts, NULL, NULL, out);
}

/* out[v] = leaf elements (sum of rows x cols over the dense leaves) under node v, for every node */
int bfhipDescSubtreeLeafElems(BfhipDesc const *desc, uint64_t *out) {
  if (!desc || !out || !desc->kind || !desc->rows || !desc->cols || !desc->childBegin) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  uint64_t const n = desc->numNodes;
  int ordered = 1;       /* children before parents (what the native layouts emit): one pass */
  for (uint64_t v = 0; v < n && ordered; ++v)
    for (uint64_t c = desc->childBegin[v]; c < desc->childBegin[v + 1]; ++c) if (desc->childNode[c] >= v) { ordered = 0; break; }
  if (ordered) {
    for (uint64_t v = 0; v < n; ++v) {
      uint64_t t = desc->kind[v] == BFHIP_NODE_DENSE ? desc->rows[v] * desc->cols[v] : 0;
      for (uint64_t c = desc->childBegin[v]; c < desc->childBegin[v + 1]; ++c) t += out[desc->childNode[c]];
      out[v] = t;
    }
    return 0;
  }
  /* any order: memoised depth-first walk with an explicit stack (node, next child) */
  uint8_t *done = calloc(n ? n : 1, 1);
  uint64_t *stack = malloc((2 * n + 2) * 8);
  if (!done || !stack) { free(done); free(stack); return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); }
  int rc = 0;
  for (uint64_t r = 0; r < n && !rc; ++r) {
    if (done[r]) continue;
    uint64_t sp = 0;
    stack[sp++] = r; stack[sp++] = desc->childBegin[r];
    out[r] = desc->kind[r] == BFHIP_NODE_DENSE ? desc->rows[r] * desc->cols[r] : 0;
    while (sp) {
      uint64_t const v = stack[sp - 2], c = stack[sp - 1];
      if (c == desc->childBegin[v + 1]) { done[v] = 1; sp -= 2; if (sp) out[stack[sp - 2]] += out[v]; continue; }
      stack[sp - 1] = c + 1;
      uint64_t const ch = desc->childNode[c];
      if (ch >= n) { rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "child index out of range"); break; }
      if (done[ch]) { out[v] += out[ch]; continue; }
      if (sp >= 2 * n) { rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "descriptor is not a tree (cycle)"); break; }
      out[ch] = desc->kind[ch] == BFHIP_NODE_DENSE ? desc->rows[ch] * desc->cols[ch] : 0;
      stack[sp++] = ch; stack[sp++] = desc->childBegin[ch];
    }
  }
  free(done); free(stack);
  return rc;
}

int bfhipRowPartition(BfhipDesc const *desc, uint32_t world, uint64_t *cuts, uint64_t *leafElems) {
  if (!desc || !cuts) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  BfIr ir;
  int rc = bfIrFromDesc(desc, &ir);
  if (rc) return rc;
  rc = bfPlanRowPartition(&ir, world, cuts, leafElems);
  bfIrFree(&ir);
  return rc;
}
int bfhipRowPartitionMat(void const *bfMat, uint32_t world, uint64_t *cuts, uint64_t *leafElems) {
  if (!bfMat || !cuts) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  BfIr ir;
  int rc = bfIrFromBfMat(bfMat, &ir);
  if (rc) return rc;
  rc = bfPlanRowPartition(&ir, world, cuts, leafElems);
  bfIrFree(&ir);
  return rc;
}

/* ---- profiling helpers ------------------------------------------------------ */
/* read back the events of applies [evHarvested, upTo): synchronizes on each (they complete in order) */
static int harvestEvents(BfhipOperator *op, uint64_t upTo) {
  uint64_t const S = op->plan.numStages;
  for (; op->evHarvested < upTo; ++op->evHarvested) {
    uint64_t const slot = op->evHarvested % BF_EV_POOL;
    for (uint64_t s = 0; s < (op->evFlow[slot] ? 1 : S); ++s) {
      float ms = 0;
      int rc = bfdevEventElapsed(op->evStart[slot * S + s], op->evStop[slot * S + s], &ms);
      if (rc) return rc;
      op->stageMs[s] += ms;
      op->stageLaunches[s] += 1;
    }
  }
  return 0;
}

static uint64_t stageBytes(BfhipOperator const *op, uint64_t s, uint32_t nrhs) {
  BfStage const *st = &op->plan.stages[s];
  return st->leafElems * op->plan.elemSize + (st->vecIn + st->vecOut) * (uint64_t)nrhs * op->plan.elemSize;
}

int bfhipGetStageProfile(BfhipOperator *op, double *ms, uint64_t *launches, uint64_t *bytes, int reset) {
  if (!op) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator");
  if (!(op->flags & BFHIP_FLAG_PROFILE)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "operator was not compiled with BFHIP_FLAG_PROFILE");
  int rc = harvestEvents(op, op->evIssued);
  if (rc) return rc;
  uint32_t const nr = op->lastNrhs ? op->lastNrhs : 1;
  int const oneLaunch = op->flow && nr < 2;        /* the whole apply is one launch: its time and bytes are reported under stage 0 */
  for (uint64_t s = 0; s < op->plan.numStages; ++s) {
    if (ms) ms[s] = op->stageMs[s];
    if (launches) launches[s] = op->stageLaunches[s];
    if (bytes) bytes[s] = oneLaunch ? 0 : stageBytes(op, s, nr);
    if (bytes && oneLaunch) bytes[0] += stageBytes(op, s, nr);
    if (reset) { op->stageMs[s] = 0; op->stageLaunches[s] = 0; }
  }
  return 0;
}

int bfhipSetProfileSampling(BfhipOperator *op, uint32_t every) {
  if (!op) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator");
  if (!(op->flags & BFHIP_FLAG_PROFILE)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "operator was not compiled with BFHIP_FLAG_PROFILE");
  op->profEvery = every;
  op->applyCount = 0;
  return 0;
}

/* ---- apply ------------------------------------------------------------------ */
/* what bfdevLaunchStage gets for stage `st` of `plan` (x and y left NULL) */
void stageLaunchArgs(BfhipOperator const *op, BfPlan const *plan, BfStage const *st, uint32_t nrhs, BfLaunchArgs *a) {
  a->arena = (plan == &op->tplan && op->dArenaT) ? op->dArenaT : op->dArena; a->items = st->dItems; a->pieces = st->dPieces; a->numItems = st->numItems; a->firstSmall = st->firstSmall; a->numCoop = st->numCoop; a->numNarrow = st->numNarrow; a->numCoopNarrow = st->numCoopNarrow; a->maxRowsRest = st->maxRowsRest;
  a->x = NULL; a->y = NULL; a->temp = op->dTemp; a->zero = op->dZero; a->nrhs = nrhs; a->dtype = plan->dtype; a->maxRows = st->maxRows;
  a->transposed = plan->transposed;
  a->tickets = NULL;
  a->exactComplex = (op->flags & BFHIP_FLAG_EXACT_COMPLEX) != 0; a->rhsBlocks = plan == &op->plan ? op->rhsBlocks : op->adjointRhsBlocks;      /* the adjoint's plans (shared or packed) have a switch of their own */
}

/* the reduce passes of a stage, BF_REDUCE_BATCH to a launch; `allIntoY`: every destination is y (the one-launch flow path) */
static int launchReduces(BfhipOperator *op, BfPlan const *plan, BfStage const *st, uint32_t nrhs, void *dY, int allIntoY, void *stream) {
  for (uint64_t r0 = 0; r0 < st->numReduce; r0 += BF_REDUCE_BATCH) {
    BfReduceArgs ra[BF_REDUCE_BATCH];
    uint32_t const cnt = (uint32_t)(st->numReduce - r0 < BF_REDUCE_BATCH ? st->numReduce - r0 : BF_REDUCE_BATCH);
    for (uint32_t r = 0; r < cnt; ++r) {
      BfReduce *rd = &st->reduce[r0 + r];
      ra[r].rowInterval = rd->dRowInterval; ra[r].ivBegin = rd->dIvBegin; ra[r].srcBias = rd->dSrcBias;
      ra[r].numRows = rd->numRows; ra[r].temp = op->dTemp; ra[r].nrhs = nrhs; ra[r].dtype = plan->dtype;
      ra[r].longLists = rd->maxSrc >= 64; ra[r].pad = 0;
      ra[r].dest = allIntoY || rd->destSpace == BF_SPACE_Y ? dY : (void *)((char *)op->dTemp + rd->destOff * nrhs * plan->elemSize);
    }
    int const rc = bfdevLaunchReduce(ra, cnt, stream);
    if (rc) return rc;
  }
  return 0;
}

static int runPlan(BfhipOperator *op, BfPlan *plan, void const *dX, size_t nrhs, void *dY, void *stream) {
  if (!op || !dX || !dY) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (nrhs == 0 || nrhs > 0xffffu) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "nrhs out of range");
  if (op->flags & BFHIP_FLAG_PLAN_ONLY) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "operator was compiled with BFHIP_FLAG_PLAN_ONLY: no device operator exists");
  int rc;
  BfDevScope ds;
  if ((rc = bfDevEnter(&ds, op->device))) return rc;
  if (op->tempRhs < nrhs) {
    /* growing the vector arena is not stream-ordered: drain first */
    if ((rc = bfdevSync(stream))) goto out;
    if ((rc = ensureTemp(op, (uint32_t)nrhs))) goto out;
  }
  int const prof = (op->flags & BFHIP_FLAG_PROFILE) != 0 && plan == &op->plan && (op->profEvery <= 1 || op->applyCount % op->profEvery == 0);
  if (plan == &op->plan) ++op->applyCount;
  /* timing never makes an apply wait for the previous one: only when all BF_EV_POOL event sets are in flight is the oldest read back */
  if (prof && op->evIssued - op->evHarvested >= BF_EV_POOL && (rc = harvestEvents(op, op->evIssued - BF_EV_POOL + 1))) goto out;
  uint64_t const evBase = prof ? (op->evIssued % BF_EV_POOL) * plan->numStages : 0;
  if (prof) op->evFlow[op->evIssued % BF_EV_POOL] = 0;
#ifdef BFHIP_EXPERIMENTAL
  if (op->flow && plan == &op->plan && nrhs < 2) {            /* (two and more right-hand sides: the matrix-core kernel, staged) */
    /* the whole plan as ONE dependency-driven launch (bfFlowKernelC128), then the reduce passes into y */
    uint32_t const perApply = op->flowNumItems + op->flowGrid * 4u;      /* tickets an apply consumes: every wavefront draws one past the end */
    if (op->flowEpoch >= 0x7fffffffu / op->flowMaxWriters - 1 || op->flowQueueBase >= 0xffffffffu - 2u * perApply) {
      if ((rc = bfdevMemsetAsync(op->dFlowCounters, 0, op->flowNumBufs * 4, stream))) goto out;      /* long before 32 bits wrap */
      op->flowEpoch = 0; op->flowQueueBase = 0;
    }
    BfFlowArgs fa;
    fa.arena = op->dArena; fa.items = op->dFlowItems; fa.pieces = op->dFlowPieces; fa.itemOut = op->dFlowItemOut; fa.writers = op->dFlowWriters;
    fa.counters = op->dFlowCounters; fa.numItems = op->flowNumItems; fa.nrhs = (uint32_t)nrhs; fa.epoch = ++op->flowEpoch;
    fa.queueBase = op->flowQueueBase; fa.gridWorkgroups = op->flowGrid; fa.x = dX; fa.y = dY; fa.temp = op->dTemp;
    op->flowQueueBase += perApply;
    if (prof) { op->evFlow[op->evIssued % BF_EV_POOL] = 1; if ((rc = bfdevEventRecord(op->evStart[evBase], stream))) goto out; }
    if ((rc = bfdevLaunchFlow(&fa, stream))) goto out;
    if (prof && (rc = bfdevEventRecord(op->evStop[evBase], stream))) goto out;
    {
      static int dbg = -1;
      if (dbg < 0) { char const *e = getenv("BFHIP_FLOW_DEBUG"); dbg = e && e[0] == '1'; }
      if (dbg) {      /* diagnostic: after the launch every vector's counter must stand at writers x epoch */
        if ((rc = bfdevSync(stream))) goto out;
        uint32_t *c = malloc(op->flowNumBufs * 4), *w = malloc(op->flowNumBufs * 4);
        if (c && w && !bfdevMemcpyD2H(c, op->dFlowCounters, op->flowNumBufs * 4) && !bfdevMemcpyD2H(w, op->dFlowWriters, op->flowNumBufs * 4)) {
          uint64_t bad = 0;
          for (uint64_t b = 2; b < op->flowNumBufs; ++b) if (c[b] != w[b] * op->flowEpoch) { if (bad++ < 8) fprintf(stderr, "bfhip flow: vector %llu counter %u, expected %u x %u\n", (unsigned long long)b, c[b], w[b], op->flowEpoch); }
          fprintf(stderr, "bfhip flow: epoch %u queue %u (base %u + %u items + %u waves) error %u, %llu of %llu counters off\n", op->flowEpoch, c[0], fa.queueBase, op->flowNumItems,
                  op->flowGrid * 4u, c[1], (unsigned long long)bad, (unsigned long long)op->flowNumBufs);
        }
        free(c); free(w);
      }
    }
    for (uint64_t s = 0; s < plan->numStages; ++s)
      if ((rc = launchReduces(op, plan, &plan->stages[s], (uint32_t)nrhs, dY, 1, stream))) goto out;      /* flowOk: every reduce sums into y */
    if (prof) { ++op->evIssued; op->lastNrhs = (uint32_t)nrhs; }
    goto out;
  }
#endif
  for (uint64_t s = 0; s < plan->numStages; ++s) {
    BfStage *st = &plan->stages[s];
    BfLaunchArgs a;
    stageLaunchArgs(op, plan, st, (uint32_t)nrhs, &a);
    a.x = dX; a.y = dY;
    if (plan->dtype == BFHIP_C128 && !plan->transposed && nrhs < 2) a.tickets = st->dTickets;      /* NULL unless this is an EXPERIMENTAL build run with BFHIP_PERSISTENT=1 (allocated at compile time) */
    if (prof && (rc = bfdevEventRecord(op->evStart[evBase + s], stream))) goto out;
    if ((rc = bfdevLaunchStage(&a, stream))) goto out;
    if (prof && (rc = bfdevEventRecord(op->evStop[evBase + s], stream))) goto out;
    if ((rc = launchReduces(op, plan, st, (uint32_t)nrhs, dY, 0, stream))) goto out;
  }
  if (prof) { ++op->evIssued; op->lastNrhs = (uint32_t)nrhs; }
out:
  bfDevLeave(&ds);      /* every path hands the caller's device back */
  return rc;
}

/* grow the vector arena for `nrhs` right-hand sides now (not stream-ordered: synchronizes the device's default
 * stream), so that later applies of up to that many cannot fail on an allocation */
int bfhipOperatorReserveRhs(BfhipOperator *op, uint32_t nrhs) {
  if (!op || !nrhs) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator / zero nrhs");
  if (op->flags & BFHIP_FLAG_PLAN_ONLY) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "operator was compiled with BFHIP_FLAG_PLAN_ONLY: no device operator exists");
  if (op->tempRhs >= nrhs) return 0;
  int rc;
  BfDevScope ds;
  if ((rc = bfDevEnter(&ds, op->device))) return rc;
  rc = bfdevSync(NULL);
  if (!rc) rc = ensureTemp(op, nrhs);
  bfDevLeave(&ds);
  return rc;
}

/* Is the forward plan applied as ONE dependency-driven launch (one right-hand side), and has any of its waits ever
 * given up?  (They cannot, by construction; the flag exists so that a broken invariant shows up as an error instead
 * of a hung GPU.)  Synchronizes the device's default stream when the flag is read. */
int bfhipFlowStatus(BfhipOperator *op, uint32_t *enabled, uint32_t *waitGaveUp) {
  if (!op) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator");
  if (enabled) *enabled = (uint32_t)op->flow;
  if (waitGaveUp) {
    *waitGaveUp = 0;
    if (op->flow && !(op->flags & BFHIP_FLAG_PLAN_ONLY)) {
      uint32_t two[2] = {0, 0};
      int rc;
      BfDevScope ds;
      if ((rc = bfDevEnter(&ds, op->device))) return rc;
      rc = bfdevMemcpyD2H(two, op->dFlowCounters, sizeof two);       /* [0] ticket queue, [1] error flag */
      bfDevLeave(&ds);
      if (rc) return rc;
      *waitGaveUp = two[1];
    }
  }
  return 0;
}

int bfhipApplyDevice(BfhipOperator *op, void const *dX, size_t nrhs, void *dY, void *stream) {
  if (!op) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator");
  return runPlan(op, &op->plan, dX, nrhs, dY, stream);
}

int bfhipApplyTransposeDevice(BfhipOperator *op, void const *dX, size_t nrhs, void *dY, void *stream) {
  if (!op) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator");
  if (!op->hasTplan) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "operator was not compiled with BFHIP_FLAG_ADJOINT");
  return runPlan(op, &op->tplan, dX, nrhs, dY, stream);
}

/* ---- covariance products (the caller of the real path) ------------------------ */
int covScratch(BfhipOperator *op, size_t nrhs, void *stream) {
  if (op->dCov && op->covRhs >= nrhs) return 0;
  /* two blocks of the longer side: [permuted input | A^T result] resp. [scaled input | A result].  Growing is not
   * stream-ordered (work enqueued earlier may still read the old blocks): drain first, as runPlan does for the vector arena */
  uint64_t const big = op->plan.numRows > op->plan.numCols ? op->plan.numRows : op->plan.numCols;
  int rc;
  if (op->dCov) {
    if ((rc = bfdevSync(stream))) return rc;
    bfdevFree(op->dCov); op->dCov = NULL; op->covRhs = 0;
  }
  if ((rc = bfdevMalloc(&op->dCov, 2 * big * nrhs * op->plan.elemSize + 32))) return rc;
  op->covRhs = (uint32_t)nrhs;
  return 0;
}

int bfhipCovSampleDevice(BfhipOperator *op, void const *dGammaLam, uint64_t const *dRowPerm, void const *dW, void *dZ, void *stream) {
  if (!op || !dW || !dZ) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  int rc;
  BfDevScope ds;
  if ((rc = bfCovCheckOperator(op, 0)) || (rc = bfDevEnter(&ds, op->device))) return rc;
  uint64_t const m = op->plan.numRows, n = op->plan.numCols;
  if ((rc = covScratch(op, 1, stream))) goto out;
  char *t0, *t1;
  bfCovHalves(op, 1, &t0, &t1);
  void const *xin = dW;
  if (dGammaLam) { if ((rc = bfdevScalePermute(t0, dW, dGammaLam, 1, NULL, n, op->plan.dtype, stream))) goto out; xin = t0; }
  if ((rc = runPlan(op, &op->plan, xin, 1, dRowPerm ? (void *)t1 : dZ, stream))) goto out;
  if (dRowPerm) rc = bfdevScalePermute(dZ, t1, NULL, 0, dRowPerm, m, op->plan.dtype, stream);
out:
  bfDevLeave(&ds);
  return rc;
}

int bfhipCovMatvecDevice(BfhipOperator *op, void const *dGammaLam, uint64_t const *dRowPerm, uint64_t const *dRevRowPerm, void const *dV, void *dZ, void *stream) {
  if (!op || !dV || !dZ) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  int rc;
  BfDevScope ds;
  if ((rc = bfCovCheckOperator(op, 1)) || (rc = bfDevEnter(&ds, op->device))) return rc;
  uint64_t const m = op->plan.numRows, n = op->plan.numCols;
  if ((rc = covScratch(op, 1, stream))) goto out;
  char *t0, *t1;
  bfCovHalves(op, 1, &t0, &t1);
  void const *vin = dV;
  if (dRevRowPerm) { if ((rc = bfdevScalePermute(t0, dV, NULL, 0, dRevRowPerm, m, op->plan.dtype, stream))) goto out; vin = t0; }
  if ((rc = runPlan(op, &op->tplan, vin, 1, t1, stream))) goto out;                 /* tmp2 = Phi^T v */
  if (dGammaLam && (rc = bfdevScalePermute(t1, t1, dGammaLam, 2, NULL, n, op->plan.dtype, stream))) goto out;   /* GammaLam twice */
  if ((rc = runPlan(op, &op->plan, t1, 1, dRowPerm ? (void *)t0 : dZ, stream))) goto out;
  if (dRowPerm) rc = bfdevScalePermute(dZ, t0, NULL, 0, dRowPerm, m, op->plan.dtype, stream);
out:
  bfDevLeave(&ds);
  return rc;
}

/* (the batched entries -- block products, device normals, draw, streaming moments -- are in bfhip_cov.c) */
double bfhipNormalValue(uint64_t seed, uint64_t idx) { return bfhip_normal_value(seed, idx); }

/* The host-vector apply behind bfhipApply and every slot of the vtable shim (the path an unmodified reference caller takes:
 * bfSolveGMRES calls bfMatMul once per iteration, src/linalg.c:125,155).  What each of X and Y is decides what it costs:
 *   device memory of the operator's GPU, densely packed   used in place: no copy at all (the call is then bfhipApplyDevice + a wait);
 *   pinned / registered host memory, densely packed       DMA straight from / to the caller's buffer (hipHostMalloc'd, or registered with
 *                                                         bfhipHostRegister by a caller who knows its lifetime: a Krylov basis, say);
 *   anything else (pageable memory, ld != nrhs, fp32)     packed through the operator's own pinned staging buffer, then DMA.
 * The wait is on the apply's own stream, not on the device.  The library never registers a caller's buffer by itself: a cached
 * registration of memory the caller has since freed (glibc hands 4 MB vectors back to the kernel) would leave the GPU with a stale
 * mapping. */
/* One piece of it: all `nrhs` columns (<= 0xffff) in one apply, with the staging buffers and the vector arena sized for them.
 * The operator's device is current. */
static int applyHostPiece(BfhipOperator *op, int transpose, void const *X, size_t ldx, size_t nrhs, void *Y, size_t ldy) {
  int rc;
  size_t es = op->plan.elemSize;
  size_t hostEs = op->srcDtype == BFHIP_C128 ? 16 : 8;      /* host side is always double precision */
  size_t const nc = bfDtypeComplex(op->plan.dtype) ? 2 : 1;  /* scalars per element (the fp32 / complex64 conversions below) */
  uint64_t n = transpose ? op->plan.numRows : op->plan.numCols, m = transpose ? op->plan.numCols : op->plan.numRows;
  uint64_t big = n > m ? n : m;
  int const same = es == hostEs;
  int const kx = same && ldx == nrhs ? bfdevPointerKind(X) : 0, ky = same && ldy == nrhs ? bfdevPointerKind(Y) : 0;
  void *hx = NULL, *hy = NULL;
  if (op->xyRhs < nrhs && (kx != 1 || ky != 1)) {
    bfdevFree(op->dX); bfdevFree(op->dY); op->dX = op->dY = NULL; op->xyRhs = 0;
    bfdevHostFreePinned(op->hX); bfdevHostFreePinned(op->hY); op->hX = op->hY = NULL;
    if ((rc = bfdevMalloc(&op->dX, big * nrhs * es))) goto out;
    if ((rc = bfdevMalloc(&op->dY, big * nrhs * es))) goto out;
    /* pinned staging: the copies run at PCIe rate instead of through the runtime's pageable bounce buffers */
    if ((rc = bfdevHostAllocPinned(&op->hX, (big * nrhs * es) != 0 ? big * nrhs * es : 16))) goto out;
    if ((rc = bfdevHostAllocPinned(&op->hY, (big * nrhs * es) != 0 ? big * nrhs * es : 16))) goto out;
    op->xyRhs = (uint32_t)nrhs;
  }
  hx = op->hX; hy = op->hY;
  void const *dXuse = op->dX;
  void *dYuse = ky == 1 ? Y : op->dY;
  if (kx == 1) dXuse = X;
  else if (kx == 2 || kx == 3) { if ((rc = bfdevMemcpyAnyAsync(op->dX, X, n * nrhs * es, NULL))) goto out; }
  else {
    /* pack to ld == nrhs (and demote if the operator computes in fp32) into the pinned buffer, in pieces: the DMA of a piece runs
     * while the CPU packs the next one (a 4 MB vector: ~0.1 ms of the ~0.25 ms its copy costs) */
    uint64_t const rowsPer = n > 4 * BF_HOST_PIECE_ROWS ? (n + 3) / 4 : n;
    for (uint64_t r0 = 0; r0 < n; r0 += rowsPer) {
      uint64_t const r1 = r0 + rowsPer < n ? r0 + rowsPer : n;
      if (same) {
        if (ldx == nrhs) memcpy((char *)hx + r0 * nrhs * es, (char const *)X + r0 * nrhs * es, (r1 - r0) * nrhs * es);
        else for (uint64_t i = r0; i < r1; ++i) memcpy((char *)hx + i * nrhs * es, (char const *)X + i * ldx * es, nrhs * es);
      } else {
        for (uint64_t i = r0; i < r1; ++i) for (size_t q = 0; q < nrhs * nc; ++q) ((float *)hx)[i * nrhs * nc + q] = (float)((double const *)X)[i * ldx * nc + q];
      }
      if ((rc = bfdevMemcpyH2DAsync((char *)op->dX + r0 * nrhs * es, (char *)hx + r0 * nrhs * es, (r1 - r0) * nrhs * es, NULL))) goto out;
    }
  }
  if ((rc = runPlan(op, transpose ? &op->tplan : &op->plan, dXuse, nrhs, dYuse, NULL))) goto out;
  if (ky == 2 || ky == 3) { if ((rc = bfdevMemcpyAnyAsync(Y, op->dY, m * nrhs * es, NULL))) goto out; }
  if (ky != 0) { if ((rc = bfdevSync(NULL))) goto out; }
  else {
    /* the result comes back in pieces too: the CPU unpacks a piece while the DMA of the next is in flight (an event per piece) */
    uint64_t const rowsPer = m > 4 * BF_HOST_PIECE_ROWS ? (m + 3) / 4 : m;
    uint32_t np = 0;
    for (uint64_t r0 = 0; r0 < m; r0 += rowsPer, ++np) {
      uint64_t const r1 = r0 + rowsPer < m ? r0 + rowsPer : m;
      if ((rc = bfdevMemcpyD2HAsync((char *)hy + r0 * nrhs * es, (char *)op->dY + r0 * nrhs * es, (r1 - r0) * nrhs * es, NULL))) goto out;
      if (!op->evHost[np] && (rc = bfdevEventCreate(&op->evHost[np]))) goto out;
      if ((rc = bfdevEventRecord(op->evHost[np], NULL))) goto out;
    }
    np = 0;
    for (uint64_t r0 = 0; r0 < m; r0 += rowsPer, ++np) {
      uint64_t const r1 = r0 + rowsPer < m ? r0 + rowsPer : m;
      if ((rc = bfdevEventSync(op->evHost[np]))) goto out;
      if (same) {
        if (ldy == nrhs) memcpy((char *)Y + r0 * nrhs * es, (char *)hy + r0 * nrhs * es, (r1 - r0) * nrhs * es);
        else for (uint64_t i = r0; i < r1; ++i) memcpy((char *)Y + i * ldy * es, (char *)hy + i * nrhs * es, nrhs * es);
      } else {
        for (uint64_t i = r0; i < r1; ++i) for (size_t q = 0; q < nrhs * nc; ++q) ((double *)Y)[i * ldy * nc + q] = ((float *)hy)[i * nrhs * nc + q];
      }
    }
    if (m == 0 && (rc = bfdevSync(NULL))) goto out;
  }
out:
  return rc;
}

int bfhipHostApplyPanelWidth(uint64_t nrhs, uint64_t perColBytes, uint64_t budget, uint64_t *width) {
  if (!width || !nrhs) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL width / zero nrhs");
  uint64_t const fit = perColBytes ? budget / perColBytes : UINT64_MAX;      /* columns the budget holds */
  if (nrhs <= 0xffffu && nrhs <= fit) { *width = nrhs; return 0; }
  uint64_t w = (fit < 0xffffu ? fit : 0xffffu) / 64 * 64;
  if (w > nrhs) w = nrhs;
  if (w < 64) {
    *width = 0;
    return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host apply: %llu device bytes per column, budget %llu bytes: %llu columns fit, a panel needs %llu",
                     (unsigned long long)perColBytes, (unsigned long long)budget, (unsigned long long)fit, (unsigned long long)(nrhs < 64 ? nrhs : 64));
  }
  *width = w;
  return 0;
}

/* Columns per piece of a host-vector apply.  The call runs in one piece -- today's path, bit for bit -- unless it cannot:
 * more than 0xffff columns (what one apply takes), or a working set (two staging vectors of the longer side + the vector
 * arena, per column) larger than the budget.  The budget is bfhipSetHostApplyBudget's, or, when that is 0, the free device
 * memory plus what the operator already holds for vectors, less BF_HOST_BUDGET_MARGIN; the automatic budget is only consulted
 * when the call would grow the buffers and has more than 64 columns.  Pieces are the widest multiple of 64 columns that fits;
 * they are packed through the staging buffers, so vectors in device memory cannot be panelled (refused past 0xffff
 * columns, run in one piece otherwise). */
static int hostApplyWidth(BfhipOperator *op, int transpose, void const *X, void const *Y, size_t nrhs, uint64_t *width) {
  *width = nrhs;
  uint64_t const es = op->plan.elemSize;
  uint64_t const n = transpose ? op->plan.numRows : op->plan.numCols, m = transpose ? op->plan.numCols : op->plan.numRows;
  uint64_t const big = n > m ? n : m;
  uint64_t const te = op->plan.tempElems > op->tplan.tempElems ? op->plan.tempElems : op->tplan.tempElems;
  uint64_t const perCol = (2 * big + te) * es;
  uint64_t budget = op->hostApplyBudget;
  int rc;
  if (!budget) {
    if (nrhs <= 0xffffu && (nrhs <= 64 || (op->xyRhs >= nrhs && op->tempRhs >= nrhs))) return 0;     /* nothing grows */
    uint64_t freeBytes = 0;
    if ((rc = bfdevMemFree(&freeBytes))) return rc;
    uint64_t const held = (uint64_t)op->xyRhs * 2 * big * es + (uint64_t)op->tempRhs * te * es;
    budget = freeBytes + held > BF_HOST_BUDGET_MARGIN ? freeBytes + held - BF_HOST_BUDGET_MARGIN : 1;
  }
  if ((rc = bfhipHostApplyPanelWidth(nrhs, perCol, budget, width))) return rc;
  if (*width < nrhs) {
    int const kx = bfdevPointerKind(X), ky = bfdevPointerKind(Y);
    if (kx == 1 || kx == 3 || ky == 1 || ky == 3) {
      if (nrhs > 0xffffu) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "host apply of %llu > 65535 columns needs host vectors (device memory cannot be panelled)", (unsigned long long)nrhs);
      *width = nrhs;
    }
  }
  return 0;
}

int applyHost(BfhipOperator *op, int transpose, void const *X, size_t ldx, size_t nrhs, void *Y, size_t ldy) {
  if (!op || !X || !Y) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (transpose && !op->hasTplan) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "operator was not compiled with BFHIP_FLAG_ADJOINT");
  if (nrhs == 0 || ldx < nrhs || ldy < nrhs) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "bad nrhs / leading dimension");
  if (op->flags & BFHIP_FLAG_PLAN_ONLY) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "operator was compiled with BFHIP_FLAG_PLAN_ONLY: no device operator exists");
  int rc;
  BfDevScope ds;
  if ((rc = bfDevEnter(&ds, op->device))) return rc;
  uint64_t width = nrhs;
  if ((rc = hostApplyWidth(op, transpose, X, Y, nrhs, &width))) goto out;
  if (width >= nrhs) rc = applyHostPiece(op, transpose, X, ldx, nrhs, Y, ldy);
  else {
    /* column panels: each is packed into the staging buffers (ld != width), applied and unpacked like a call of its own */
    size_t const hostEs = op->srcDtype == BFHIP_C128 ? 16 : 8;
    for (uint64_t c0 = 0; c0 < nrhs && !rc; c0 += width) {
      uint64_t const w = nrhs - c0 < width ? nrhs - c0 : width;
      rc = applyHostPiece(op, transpose, (char const *)X + c0 * hostEs, ldx, w, (char *)Y + c0 * hostEs, ldy);
    }
  }
out:
  bfDevLeave(&ds);
  return rc;
}

int bfhipSetHostApplyBudget(BfhipOperator *op, uint64_t bytes) {
  if (!op) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator");
  op->hostApplyBudget = bytes;
  return 0;
}

/* The three switches of the right-hand-side block kernels.  Host-only: the setting travels to the stage selection in every BfLaunchArgs
 * (stageLaunchArgs), nothing else reads it.  Their common checks, in the order all three make them: the operator, the element type
 * (`dtypes` = a bit per element type the switch serves, `wrongType` = the refusal's text for the others), the value. */
static int rhsBlocksCheck(BfhipOperator const *op, uint32_t minRhs, uint32_t dtypes, char const *wrongType) {
  if (!op) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator");
  if (!(dtypes >> op->plan.dtype & 1u)) return bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "%s", wrongType);
  if (minRhs == 1) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "minRhs must be 0 (off) or at least 2");
  return 0;
}

int bfhipSetRhsBlocks(BfhipOperator *op, uint32_t minRhs) {
  int const rc = rhsBlocksCheck(op, minRhs, 1u << BFHIP_C64,
                                "right-hand-side block kernels are a complex64 switch: complex128 operators already run block kernels "
                                "(bfStageKernelC128Mfma*) at nrhs >= 2, and the real element types (F64, F32) are not covered");
  if (!rc) op->rhsBlocks = minRhs;
  return rc;
}

/* The same switch for the real element types, in the same field (an operator has one element type). */
int bfhipSetRealRhsBlocks(BfhipOperator *op, uint32_t minRhs) {
  int const rc = rhsBlocksCheck(op, minRhs, 1u << BFHIP_F64 | 1u << BFHIP_F32,
                                "bfhipSetRealRhsBlocks is the switch of the real element types (F64, F32): complex64 operators take "
                                "bfhipSetRhsBlocks, complex128 operators already run block kernels (bfStageKernelC128Mfma*) at nrhs >= 2");
  if (!rc) op->rhsBlocks = minRhs;
  return rc;
}

/* The adjoint plan's switch, a field of its own: stageLaunchArgs hands it to the launches of op->tplan, shared-leaf or packed. */
int bfhipSetAdjointRhsBlocks(BfhipOperator *op, uint32_t minRhs) {
  int const rc = rhsBlocksCheck(op, minRhs, ~0u, NULL);
  if (rc) return rc;
  if (!op->hasTplan) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "operator has no adjoint plan (compile with BFHIP_FLAG_ADJOINT or BFHIP_FLAG_ADJOINT_PACKED)");
  op->adjointRhsBlocks = minRhs;
  return 0;
}

/* A caller who knows the lifetime of its vectors (the Krylov basis of a solver, a right-hand side applied many times) registers
 * them once: bfhipApply / the shim's Mul then DMA straight from / to them instead of packing through the staging buffer. */
int bfhipHostRegister(void *p, size_t bytes) {
  if (!p || !bytes) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL pointer / zero bytes");
  return bfdevHostRegister(p, bytes);
}
int bfhipHostUnregister(void *p) {
  if (!p) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL pointer");
  return bfdevHostUnregister(p);
}

int bfhipApply(BfhipOperator *op, void const *X, size_t ldx, size_t nrhs, void *Y, size_t ldy) {
  return applyHost(op, 0, X, ldx, nrhs, Y, ldy);
}
int bfhipApplyTranspose(BfhipOperator *op, void const *X, size_t ldx, size_t nrhs, void *Y, size_t ldy) {
  return applyHost(op, 1, X, ldx, nrhs, Y, ldy);
}

/* ---- introspection ---------------------------------------------------------- */
void **bfhipOperatorExtractSlot(BfhipOperator *op, void (*release)(void *)) { op->extractRelease = release; return &op->extract; }
uint64_t bfhipOperatorTempElems(BfhipOperator const *op) { return op->plan.tempElems > op->tplan.tempElems ? op->plan.tempElems : op->tplan.tempElems; }
uint32_t bfhipOperatorElemSize(BfhipOperator const *op) { return op ? op->plan.elemSize : 0; }
int bfhipOperatorHasAdjoint(BfhipOperator const *op) { return op ? op->hasTplan : 0; }
uint32_t bfhipOperatorSrcDtype(BfhipOperator const *op) { return op ? op->srcDtype : BFHIP_C128; }
int bfhipOperatorDevice(BfhipOperator const *op) { return (!op || (op->flags & BFHIP_FLAG_PLAN_ONLY)) ? -1 : op->device; }
BfPlan const *bfhipOperatorPlan(BfhipOperator const *op) { return op ? &op->plan : NULL; }
void const *bfhipOperatorArena(BfhipOperator const *op) { return op ? op->dArena : NULL; }
size_t bfhipGetNumRows(BfhipOperator const *op) { return op ? op->plan.numRows : 0; }
size_t bfhipGetNumCols(BfhipOperator const *op) { return op ? op->plan.numCols : 0; }
size_t bfhipNumBytes(BfhipOperator const *op) { return op ? op->plan.leafElems * (op->srcDtype == BFHIP_C128 ? 16 : 8) : 0; }
