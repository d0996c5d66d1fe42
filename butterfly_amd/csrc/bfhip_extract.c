/* bfhip_extract.c -- dense extraction A[I, J] in bounded memory (include/bfhip.h, "dense extraction"), and the shim's ToType.
 *
 * Per panel of <= 64 columns: the unit panel (ones at the panel's indices: bfdevExtractUnit clears the previous panel's ones and
 * sets the new ones, O(p)), one apply through the public entry (bfhipApplyDevice, or bfhipApplyTransposeDevice on the adjoint
 * route) and one gather of the wanted rows of the result (bfdevExtractGather, or the LDS-tiled bfdevExtractGatherT that writes
 * the transposed block).  A 64-column panel is the shape the 64-RHS matrix-core kernel runs at its best rate.
 *
 * The workspace lives on the operator (bfhipOperatorExtractSlot), grown to the largest call and released by bfhipFree: the input
 * and result panels, the index copies and, for the host entry, two gathered blocks on the device, two pinned staging blocks, a
 * copy stream and an event per buffer.  The host entry runs the panels on the default stream and the copies on the copy stream:
 * the DMA of panel t overlaps the apply of panel t + 1, and the CPU unpacks panel t - 1 while both run.
 *
 * This file is not part of the host sanitizer harness (tests/test_host_asan.py): it is where the new device launchers are called
 * from.  bfhip_shim.c reaches it only through the weakly referenced shim slot, bfhip_api.c through the release pointer stored on the operator. */
#define _GNU_SOURCE
#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"

#include <dlfcn.h>
#include <stdlib.h>
#include <string.h>

#define BF_EXTRACT_PANEL_MAX 64u

typedef struct BfExtractWork {
  void *dIn, *dRes, *dIdx, *dGath[2];
  uint64_t inBytes, resBytes, idxBytes, gathBytes[2];
  void *hStage[2];
  uint64_t stageBytes;
  void *copyStream;
  void *evGath[2], *evCopy[2];
} BfExtractWork;

static void workRelease(void *p) {
  BfExtractWork *w = p;
  if (!w) return;
  bfdevFree(w->dIn); bfdevFree(w->dRes); bfdevFree(w->dIdx);
  bfdevFree(w->dGath[0]); bfdevFree(w->dGath[1]);
  bfdevHostFreePinned(w->hStage[0]); bfdevHostFreePinned(w->hStage[1]);
  for (int i = 0; i < 2; ++i) { bfdevEventDestroy(w->evGath[i]); bfdevEventDestroy(w->evCopy[i]); }
  bfdevStreamDestroy(w->copyStream);
  free(w);
}

/* a device buffer of at least `bytes` (grown, old contents dropped); callers drain the streams that used it first */
static int growDevice(void **d, uint64_t *have, uint64_t bytes) {
  if (*have >= bytes && *d) return 0;
  bfdevFree(*d); *d = NULL; *have = 0;
  int rc = bfdevMalloc(d, bytes ? bytes : 16);
  if (!rc) *have = bytes;
  return rc;
}

typedef struct BfExtractCall {
  int adjointPlan;           /* the operator whose entries are taken: A (0) or A^T (1, the shim's transposed ToType) */
  int viaOther;              /* panels over the row set through the other plan, transposed gather */
  uint32_t p, es, dtype;
  uint64_t opRows, opCols;   /* of the operator whose entries are taken */
} BfExtractCall;

/* everything that can be refused without a device */
static int validate(BfhipOperator const *op, uint64_t const *rows, size_t numRows, uint64_t const *cols, size_t numCols, size_t ldOut,
                    BfhipExtractOptions const *opt, int adjointPlan, BfExtractCall *c) {
  if (!op) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator");
  uint32_t const flags = opt ? opt->flags : 0, panel = opt ? opt->panel : 0;
  if (flags & ~BFHIP_EXTRACT_VIA_ADJOINT) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "unknown extraction flags 0x%x", flags);
  if (panel > BF_EXTRACT_PANEL_MAX) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "panel %u: at most %u columns", panel, BF_EXTRACT_PANEL_MAX);
  int const hasT = bfhipOperatorHasAdjoint(op);
  if ((flags & BFHIP_EXTRACT_VIA_ADJOINT) && !hasT) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BFHIP_EXTRACT_VIA_ADJOINT needs an operator compiled with BFHIP_FLAG_ADJOINT");
  if (adjointPlan && !hasT) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "operator was not compiled with BFHIP_FLAG_ADJOINT");
  BfhipStats st;
  memset(&st, 0, sizeof st);
  st.structSize = sizeof st;
  int rc = bfhipGetStats(op, &st);
  if (rc) return rc;
  c->adjointPlan = adjointPlan;
  c->viaOther = (flags & BFHIP_EXTRACT_VIA_ADJOINT) != 0;
  c->p = panel ? panel : BF_EXTRACT_PANEL_MAX;
  c->es = bfhipOperatorElemSize(op);
  c->dtype = st.dtype;
  c->opRows = adjointPlan ? st.numCols : st.numRows;
  c->opCols = adjointPlan ? st.numRows : st.numCols;
  if (!rows && numRows != c->opRows)
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "rows == NULL stands for all %llu rows, numRows is %llu", (unsigned long long)c->opRows, (unsigned long long)numRows);
  if (!cols && numCols != c->opCols)
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "cols == NULL stands for all %llu columns, numCols is %llu", (unsigned long long)c->opCols, (unsigned long long)numCols);
  if (ldOut < numCols) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "ldOut %llu < numCols %llu", (unsigned long long)ldOut, (unsigned long long)numCols);
  if (rows) for (size_t i = 0; i < numRows; ++i)
    if (rows[i] >= c->opRows) return bfhipFail(BFABI_ERROR_OUT_OF_RANGE, "rows[%llu] = %llu >= %llu rows", (unsigned long long)i, (unsigned long long)rows[i], (unsigned long long)c->opRows);
  if (cols) for (size_t j = 0; j < numCols; ++j)
    if (cols[j] >= c->opCols) return bfhipFail(BFABI_ERROR_OUT_OF_RANGE, "cols[%llu] = %llu >= %llu columns", (unsigned long long)j, (unsigned long long)cols[j], (unsigned long long)c->opCols);
  return 0;
}

int bfhipExtractWorkspaceBytes(BfhipOperator const *op, size_t numRows, size_t numCols, BfhipExtractOptions const *opt, uint64_t *bytes) {
  if (!bytes) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL bytes");
  if (!op) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator");
  uint32_t const panel = opt ? opt->panel : 0;
  if (panel > BF_EXTRACT_PANEL_MAX) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "panel %u: at most %u columns", panel, BF_EXTRACT_PANEL_MAX);
  uint64_t const p = panel ? panel : BF_EXTRACT_PANEL_MAX, es = bfhipOperatorElemSize(op);
  uint64_t const g = (opt && (opt->flags & BFHIP_EXTRACT_VIA_ADJOINT)) ? numCols : numRows;
  *bytes = (bfhipGetNumRows(op) + bfhipGetNumCols(op)) * p * es + ((uint64_t)numRows + numCols) * 8 + bfhipOperatorTempElems(op) * p * es + 2 * g * p * es;
  return 0;
}

/* the panel loop.  Device entry: dOut != NULL, host == NULL, blocks go straight into dOut on `stream`.  Host entry: host != NULL,
 * blocks are gathered into the two device blocks and copied out (direct: DMA into `host` itself, which is of the device element
 * size; else through pinned staging, unpacked and promoted into `host` of hostEs bytes per element). */
static int runExtract(BfhipOperator *op, BfExtractCall const *c, uint64_t const *rows, size_t numRows, uint64_t const *cols, size_t numCols,
                      void *dOut, void *host, size_t ldOut, int direct, void *stream) {
  int rc;
  BfDevScope ds;
  if ((rc = bfDevEnter(&ds, bfhipOperatorDevice(op)))) return rc;
  void **slot = bfhipOperatorExtractSlot(op, workRelease);
  if (!*slot && !(*slot = calloc(1, sizeof(BfExtractWork)))) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); goto out; }
  BfExtractWork *w = *slot;
  uint32_t const p = c->p, es = c->es;
  /* the panels run over the column set (forward) or over the row set (through the other plan) */
  uint64_t const unitExt = c->viaOther ? c->opRows : c->opCols, resExt = c->viaOther ? c->opCols : c->opRows;
  uint64_t const numUnit = c->viaOther ? numRows : numCols, numGath = c->viaOther ? numCols : numRows;
  int const applyT = c->adjointPlan != c->viaOther;       /* which plan the panels go through */
  size_t const hostEs = bfDtypeComplex(c->dtype) ? 16 : 8, nc = bfDtypeComplex(c->dtype) ? 2 : 1;
  int const same = hostEs == es;
  /* setup (synchronising): the operator's streams drained, buffers grown, indices uploaded */
  if ((rc = bfdevSync(stream))) goto out;
  if (host && (rc = bfdevSync(NULL))) goto out;
  if ((rc = bfhipOperatorReserveRhs(op, p))) goto out;
  if ((rc = growDevice(&w->dIn, &w->inBytes, unitExt * p * es))) goto out;
  if ((rc = growDevice(&w->dRes, &w->resBytes, resExt * p * es))) goto out;
  uint64_t const nIdxR = rows ? numRows : 0, nIdxC = cols ? numCols : 0;
  if ((rc = growDevice(&w->dIdx, &w->idxBytes, (nIdxR + nIdxC) * 8))) goto out;
  uint64_t *dRows = rows ? (uint64_t *)w->dIdx : NULL, *dCols = cols ? (uint64_t *)w->dIdx + nIdxR : NULL;
  if (rows && (rc = bfdevMemcpyH2D(dRows, rows, nIdxR * 8))) goto out;
  if (cols && (rc = bfdevMemcpyH2D(dCols, cols, nIdxC * 8))) goto out;
  uint64_t const *dUnit = c->viaOther ? dRows : dCols, *dGath = c->viaOther ? dCols : dRows;
  uint64_t const blockBytes = numGath * p * es;       /* one gathered panel, densely packed */
  if (host) {
    if ((rc = growDevice(&w->dGath[0], &w->gathBytes[0], blockBytes))) goto out;
    if ((rc = growDevice(&w->dGath[1], &w->gathBytes[1], blockBytes))) goto out;
    if (!direct && w->stageBytes < blockBytes) {
      bfdevHostFreePinned(w->hStage[0]); bfdevHostFreePinned(w->hStage[1]); w->hStage[0] = w->hStage[1] = NULL; w->stageBytes = 0;
      if ((rc = bfdevHostAllocPinned(&w->hStage[0], blockBytes))) goto out;
      if ((rc = bfdevHostAllocPinned(&w->hStage[1], blockBytes))) goto out;
      w->stageBytes = blockBytes;
    }
    if (!w->copyStream && (rc = bfdevStreamCreateNonBlocking(&w->copyStream))) goto out;
    for (int i = 0; i < 2; ++i) {
      if (!w->evGath[i] && (rc = bfdevEventCreate(&w->evGath[i]))) goto out;
      if (!w->evCopy[i] && (rc = bfdevEventCreate(&w->evCopy[i]))) goto out;
    }
  }
  if ((rc = bfdevMemsetAsync(w->dIn, 0, unitExt * p * es, stream))) goto out;
  uint64_t const numPanels = (numUnit + p - 1) / p;
  uint32_t prevCount = 0, prevLd = p;
  uint64_t prevBase = 0;
  for (uint64_t t = 0; t <= numPanels; ++t) {
    if (t < numPanels) {
      uint64_t const u0 = t * p;
      uint32_t const pw = (uint32_t)(numUnit - u0 < p ? numUnit - u0 : p);
      if ((rc = bfdevExtractUnit(w->dIn, c->dtype, unitExt, dUnit, prevBase, prevCount, prevLd, dUnit, u0, pw, pw, stream))) goto out;
      prevBase = u0; prevCount = pw; prevLd = pw;
      rc = applyT ? bfhipApplyTransposeDevice(op, w->dIn, pw, w->dRes, stream) : bfhipApplyDevice(op, w->dIn, pw, w->dRes, stream);
      if (rc) goto out;
      /* where this panel's block goes, and its leading dimension */
      void *dst;
      uint64_t ld;
      uint32_t const b = (uint32_t)(t & 1);
      if (host) {
        if (t >= 2 && (rc = bfdevStreamWaitEvent(stream, w->evCopy[b]))) goto out;     /* the copy out of this block two panels ago */
        dst = w->dGath[b];
        ld = c->viaOther ? numGath : pw;
      } else {
        dst = c->viaOther ? (char *)dOut + u0 * ldOut * es : (char *)dOut + u0 * es;
        ld = ldOut;
      }
      rc = c->viaOther ? bfdevExtractGatherT(dst, ld, w->dRes, resExt, pw, dGath, 0, numGath, es, stream)
                       : bfdevExtractGather(dst, ld, w->dRes, resExt, pw, dGath, 0, numGath, es, stream);
      if (rc) goto out;
      if (host) {
        if ((rc = bfdevEventRecord(w->evGath[b], stream))) goto out;
        if ((rc = bfdevStreamWaitEvent(w->copyStream, w->evGath[b]))) goto out;
        if (direct) {
          /* forward: numGath rows of pw elements at column u0; adjoint: pw rows of numGath elements at row u0 */
          rc = c->viaOther ? bfdevMemcpy2DAsync((char *)host + u0 * ldOut * es, ldOut * es, dst, numGath * es, numGath * es, pw, w->copyStream)
                           : bfdevMemcpy2DAsync((char *)host + u0 * es, ldOut * es, dst, (size_t)pw * es, (size_t)pw * es, numGath, w->copyStream);
        } else {
          rc = bfdevMemcpyD2HAsync(w->hStage[b], dst, numGath * pw * es, w->copyStream);
        }
        if (rc) goto out;
        if ((rc = bfdevEventRecord(w->evCopy[b], w->copyStream))) goto out;
      }
    }
    /* the CPU unpacks the previous panel while this one runs */
    if (host && !direct && t >= 1) {
      uint64_t const q = t - 1, u0 = q * p;
      uint32_t const b = (uint32_t)(q & 1);
      uint32_t const pw = (uint32_t)(numUnit - u0 < p ? numUnit - u0 : p);
      if ((rc = bfdevEventSync(w->evCopy[b]))) goto out;
      char const *src = w->hStage[b];
      /* block rows: forward numGath rows of pw elements into columns u0.., adjoint pw rows of numGath elements into rows u0.. */
      uint64_t const nRowsBlk = c->viaOther ? pw : numGath, rowLen = c->viaOther ? numGath : pw;
      for (uint64_t i = 0; i < nRowsBlk; ++i) {
        char *d = c->viaOther ? (char *)host + (u0 + i) * ldOut * hostEs : (char *)host + (i * ldOut + u0) * hostEs;
        char const *s = src + i * rowLen * es;
        if (same) memcpy(d, s, rowLen * es);
        else for (uint64_t q2 = 0; q2 < rowLen * nc; ++q2) ((double *)d)[q2] = ((float const *)s)[q2];
      }
    }
  }
  if (host && direct && (rc = bfdevSync(w->copyStream))) goto out;
  if (host && (rc = bfdevSync(stream))) goto out;
out:
  if (rc && host && *slot) { bfdevSync(stream); bfdevSync(((BfExtractWork *)*slot)->copyStream); }   /* nothing in flight touches `host` */
  bfDevLeave(&ds);
  return rc;
}

int bfhipExtractDevice(BfhipOperator *op, uint64_t const *rows, size_t numRows, uint64_t const *cols, size_t numCols, void *dOut, size_t ldOut,
                       BfhipExtractOptions const *opt, void *stream) {
  BfExtractCall c;
  int rc = validate(op, rows, numRows, cols, numCols, ldOut, opt, 0, &c);
  if (rc) return rc;
  if (!numRows || !numCols) return 0;
  if (bfhipOperatorDevice(op) < 0) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "operator was compiled with BFHIP_FLAG_PLAN_ONLY: no device operator exists");
  if (!dOut) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL output");
  return runExtract(op, &c, rows, numRows, cols, numCols, dOut, NULL, ldOut, 0, stream);
}

static int extractHost(BfhipOperator *op, int adjointPlan, uint64_t const *rows, size_t numRows, uint64_t const *cols, size_t numCols, void *Out,
                       size_t ldOut, BfhipExtractOptions const *opt) {
  BfExtractCall c;
  int rc = validate(op, rows, numRows, cols, numCols, ldOut, opt, adjointPlan, &c);
  if (rc) return rc;
  if (!numRows || !numCols) return 0;
  if (bfhipOperatorDevice(op) < 0) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "operator was compiled with BFHIP_FLAG_PLAN_ONLY: no device operator exists");
  if (!Out) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL output");
  size_t const hostEs = bfDtypeComplex(c.dtype) ? 16 : 8;
  BfDevScope ds;
  if ((rc = bfDevEnter(&ds, bfhipOperatorDevice(op)))) return rc;
  int const kind = hostEs == c.es ? bfdevPointerKind(Out) : 0;      /* pinned / registered / device memory: the DMA's own target */
  bfDevLeave(&ds);
  return runExtract(op, &c, rows, numRows, cols, numCols, NULL, Out, ldOut, kind != 0, NULL);
}

int bfhipExtract(BfhipOperator *op, uint64_t const *rows, size_t numRows, uint64_t const *cols, size_t numCols, void *Out, size_t ldOut,
                 BfhipExtractOptions const *opt) {
  return extractHost(op, 0, rows, numRows, cols, numCols, Out, ldOut, opt);
}

/* ---- the shim's ToType (slot 54) ------------------------------------------------------------------------------------------------ */
/* bfMatToType(A_hip, BF_TYPE_MAT_DENSE_COMPLEX): the dense matrix the object stands for, in a BfMatDenseComplex the reference owns
 * (allocated by its own bfMatDenseComplexZeros, looked up in the host process like bfSetError), filled by the host extraction of
 * every row and column.  After bfMatTranspose the object stands for A^H (its Mul multiplies by A^H): the entries of A^T are taken
 * through the adjoint plan and conjugated.  Any other type, a real operator, a missing constructor and a sharded object raise
 * NOT_IMPLEMENTED and return NULL. */
BfAbiMat *bfhipShimToType(BfAbiMat const *m, int type) {
  BfhipOperator *op = NULL;
  int transposed = 0, sharded = 0;
  int rc = bfhipShimGet(m, &op, &transposed, &sharded);
  if (rc) { bfhipShimRaise(rc); return NULL; }
  if (type != BFABI_TYPE_MAT_DENSE_COMPLEX) { bfhipShimRaise(bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "ToType: only BF_TYPE_MAT_DENSE_COMPLEX (type %d)", type)); return NULL; }
  if (sharded) { bfhipShimRaise(bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "ToType: sharded operators are not supported")); return NULL; }
  if (bfhipOperatorSrcDtype(op) != BFHIP_C128) { bfhipShimRaise(bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "ToType: BF_TYPE_MAT_DENSE_COMPLEX of a real operator")); return NULL; }
  BfAbiMatDenseComplex *(*zeros)(size_t, size_t) = (BfAbiMatDenseComplex * (*)(size_t, size_t))dlsym(RTLD_DEFAULT, "bfMatDenseComplexZeros");
  if (!zeros) { bfhipShimRaise(bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "ToType: the host process has no bfMatDenseComplexZeros")); return NULL; }
  size_t const rows = transposed ? bfhipGetNumCols(op) : bfhipGetNumRows(op), cols = transposed ? bfhipGetNumRows(op) : bfhipGetNumCols(op);
  BfAbiMatDenseComplex *d = zeros(rows, cols);
  if (!d) { bfhipShimRaise(bfhipFail(BFABI_ERROR_MEMORY_ERROR, "ToType: bfMatDenseComplexZeros(%zu, %zu) failed", rows, cols)); return NULL; }
  if (d->colStride != 1 || d->rowStride < cols) rc = bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "ToType: the dense result is not row-major with unit column stride");
  else rc = extractHost(op, transposed, NULL, rows, NULL, cols, d->data, d->rowStride, NULL);
  if (!rc && transposed)
    for (size_t i = 0; i < rows; ++i)
      for (size_t j = 0; j < cols; ++j) d->data[2 * (i * d->rowStride + j) + 1] *= -1.0;
  if (rc) {
    BfAbiDeleteFn del = (BfAbiDeleteFn)d->super.vtbl->slot[BFABI_SLOT_Delete];
    BfAbiMat *dm = &d->super;
    if (del) del(&dm);
    bfhipShimRaise(rc);
    return NULL;
  }
  return &d->super;
}
