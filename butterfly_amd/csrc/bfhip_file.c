/* bfhip_file.c -- the on-disk form of a compiled operator: bfhipSave, bfhipLoad and the validation of everything a file
 * makes the kernels dereference.
 */
#include "bfhip_operator.h"
#include "../../include/bfhip_abi.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* =============================================================================
 * Serialization: the flattened device layout is the
 * natural on-disk form of a compiled operator.  The reference's bfMatDump is
 * write-only and lacks a complex dense payload (src/mat.c:67-73,
 * src/mat_dense_complex.c:173-222); here Save / Load round-trip the operator
 * exactly (bit-identical applies) without the BfMat graph or a rebuild.
 * File: "BFHIPOP1" | header | per plan: per stage {counts, items, pieces,
 * reduces} | leaf arena bytes.  Little-endian, same-architecture format.
 * ============================================================================= */
#define BFHIP_FILE_MAGIC "BFHIPOP1"

typedef struct FileHeader {
  char magic[8];
  uint32_t version, dtype, srcDtype, elemSize, epl, xcap, hasTplan, reserved;
  uint64_t numRows, numCols, arenaElems, leafElems, numLeaves, leafBytesAlgorithmic;
} FileHeader;

typedef struct FilePlanHeader { uint64_t numStages, tempElems, numRows, numCols; uint32_t maxItemRows, transposed; } FilePlanHeader;
typedef struct FileStageHeader { uint64_t numItems, numPieces, leafElems, vecIn, vecOut, numReduce; uint32_t maxRows, reserved; } FileStageHeader;
typedef struct FileReduceHeader { uint64_t destOff, numRows, numIntervals, numSrc; uint32_t destSpace, reserved; } FileReduceHeader;

static int writeAll(FILE *fp, void const *p, size_t n) { return n == 0 || fwrite(p, 1, n, fp) == n ? 0 : bfhipFail(BFABI_ERROR_FILE_ERROR, "short write"); }
static int readAll(FILE *fp, void *p, size_t n) { return n == 0 || fread(p, 1, n, fp) == n ? 0 : bfhipFail(BFABI_ERROR_FILE_ERROR, "short read / truncated file"); }

static int writeDeviceArray(FILE *fp, void const *d, size_t bytes) {
  if (!bytes) return 0;
  size_t const chunk = (size_t)64 << 20;
  void *h = malloc(bytes < chunk ? bytes : chunk);
  if (!h) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  int rc = 0;
  for (size_t off = 0; off < bytes && !rc; off += chunk) {
    size_t n = bytes - off < chunk ? bytes - off : chunk;
    rc = bfdevMemcpyD2H(h, (char const *)d + off, n);
    if (!rc) rc = writeAll(fp, h, n);
  }
  free(h);
  return rc;
}
static int readDeviceArray(FILE *fp, void **d, size_t bytes, uint64_t *meta) {
  int rc = bfdevMalloc(d, bytes + BF_ARENA_SLACK);
  if (rc || !bytes) return rc;
  if (meta) *meta += bytes;
  size_t const chunk = (size_t)64 << 20;
  void *h = malloc(bytes < chunk ? bytes : chunk);
  if (!h) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  for (size_t off = 0; off < bytes && !rc; off += chunk) {
    size_t n = bytes - off < chunk ? bytes - off : chunk;
    rc = readAll(fp, h, n);
    if (!rc) rc = bfdevMemcpyH2D((char *)*d + off, h, n);
  }
  free(h);
  return rc;
}

static int savePlan(FILE *fp, BfPlan const *pl) {
  FilePlanHeader ph = {pl->numStages, pl->tempElems, pl->numRows, pl->numCols, pl->maxItemRows, (uint32_t)pl->transposed};
  int rc = writeAll(fp, &ph, sizeof ph);
  for (uint64_t s = 0; s < pl->numStages && !rc; ++s) {
    BfStage const *st = &pl->stages[s];
    FileStageHeader sh = {st->numItems, st->numPieces, st->leafElems, st->vecIn, st->vecOut, st->numReduce, st->maxRows, 0};
    rc = writeAll(fp, &sh, sizeof sh);
    if (!rc) rc = writeDeviceArray(fp, st->dItems, st->numItems * sizeof(BfDevItem));
    if (!rc) rc = writeDeviceArray(fp, st->dPieces, st->numPieces * sizeof(BfDevPiece));
    for (uint64_t r = 0; r < st->numReduce && !rc; ++r) {
      BfReduce const *rd = &st->reduce[r];
      FileReduceHeader rh = {rd->destOff, rd->numRows, rd->numIntervals, rd->numSrc, rd->destSpace, 0};
      rc = writeAll(fp, &rh, sizeof rh);
      if (!rc) rc = writeDeviceArray(fp, rd->dRowInterval, rd->numRows * 4);
      if (!rc) rc = writeDeviceArray(fp, rd->dIvBegin, (rd->numIntervals + 1) * 4);
      if (!rc) rc = writeDeviceArray(fp, rd->dSrcBias, rd->numSrc * 8);
    }
  }
  return rc;
}

/* index tables are small (0.03 % of the operand): read whole, validate on the host, then upload */
static int readMetaArray(FILE *fp, void **d, void **h, size_t bytes, uint64_t *meta) {
  *h = NULL;
  int rc = bfdevMalloc(d, bytes);
  if (rc || !bytes) return rc;
  if (meta) *meta += bytes;
  *h = malloc(bytes);
  if (!*h) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  if ((rc = readAll(fp, *h, bytes))) return rc;
  return bfdevMemcpyH2D(*d, *h, bytes);
}

/* A file is untrusted input: every offset the kernels will dereference is checked against the
 * sizes in the header before the operator is accepted (a truncated or corrupt file must not turn
 * into device out-of-bounds accesses). */
/* offset + extent <= len without wrapping: offsets and extents come straight from the file as 64-bit values,
 * and `off + ext > len` accepts off = 2^64 - 16 (the sum wraps to a small value) */
static int fitsIn(uint64_t off, uint64_t ext, uint64_t len) { return off <= len && ext <= len - off; }
/* a * b + c, saturating at UINT64_MAX */
static uint64_t mulAddSat(uint64_t a, uint64_t b, uint64_t c) {
  uint64_t r;
  if (__builtin_mul_overflow(a, b, &r) || __builtin_add_overflow(r, c, &r)) return UINT64_MAX;
  return r;
}

static int validateStage(BfPlan const *pl, uint64_t arenaElems, BfStage const *st, BfDevItem const *items, BfDevPiece const *pieces) {
  uint64_t const inX = pl->numCols, outY = pl->numRows, temp = pl->tempElems;
  for (uint64_t i = 0; i < st->numItems; ++i) {
    BfDevItem const *it = &items[i];
    uint32_t const mr = it->mrFlags & 0xffffu;
    uint64_t const outLen = (it->mrFlags & BF_ITEM_OUT_Y) ? outY : temp;
    if (!mr || mr > pl->maxItemRows || mr > st->maxRows || (it->mrFlags & ~(0xffffu | BF_ITEM_OUT_Y | BF_ITEM_ROWMAJOR | BF_ITEM_MERGED | BF_ITEM_SMALL | BF_ITEM_TNARROW)) ||
        ((it->mrFlags & BF_ITEM_TNARROW) != 0) != (i < st->numNarrow) || ((it->mrFlags & BF_ITEM_TNARROW) && (!pl->transposed || mr > 16)) ||
        ((it->mrFlags & BF_ITEM_SMALL) != 0) != (i >= st->firstSmall) ||
        ((it->mrFlags & BF_ITEM_ROWMAJOR) && (pl->transposed || bfDtypeC128Layout(pl->dtype) || mr > 2 * pl->epl)) ||
        (pl->transposed && mr > 64) ||       /* bfStageKernelT: at most 64 columns of A per item */
        !fitsIn(it->outOff, mr, outLen) || !fitsIn(it->pieceBegin, it->numPieces, st->numPieces))
      return bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt operator file: item %llu out of bounds", (unsigned long long)i);
    uint32_t const mrPad = (mr + pl->epl - 1) / pl->epl * pl->epl;
    if (it->mrFlags & (BF_ITEM_MERGED | BF_ITEM_SMALL)) {     /* the kernel reads the dense pieces as one block from the first one's offset */
      int const sm = (it->mrFlags & BF_ITEM_SMALL) != 0;
      uint64_t next = 0, dense = 0;
      int const smRm = sm && (it->mrFlags & BF_ITEM_ROWMAJOR);      /* small items: row-major pieces, no contiguity promise */
      int badm = pl->transposed || bfDtypeC128Layout(pl->dtype) || (!sm && (it->mrFlags & BF_ITEM_ROWMAJOR)) || it->numPieces > (sm ? BF_SMALL_PIECES : 64u) ||
                 (sm && (mr > 2 * pl->epl || !(it->mrFlags & BF_ITEM_ROWMAJOR)));
      for (uint32_t k = 0; k < it->numPieces && !badm; ++k) {
        BfDevPiece const *pc = &pieces[it->pieceBegin + k];
        if (pc->flags & BF_PIECE_IDENTITY) continue;
        if (!smRm && dense && pc->dataOff != next) badm = 1;
        next = mulAddSat(mrPad, pc->ncols, pc->dataOff); dense += pc->ncols;
      }
      if (badm || (!dense && !sm) || dense > (sm ? BF_SMALL_COLS : BF_MERGE_COLS))
        return bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt operator file: merged item %llu is not one block", (unsigned long long)i);
    }
    for (uint32_t k = 0; k < it->numPieces; ++k) {
      BfDevPiece const *pc = &pieces[it->pieceBegin + k];
      uint64_t const inLen = (pc->flags & BF_PIECE_IN_X) ? inX : temp;
      int bad = (pc->flags & ~(BF_PIECE_IN_X | BF_PIECE_IDENTITY | BF_PIECE_ROWMAJOR)) != 0;
      int const rm = (pc->flags & BF_PIECE_ROWMAJOR) != 0;
      if (!(pc->flags & BF_PIECE_IDENTITY) && !pl->transposed && rm != ((it->mrFlags & BF_ITEM_ROWMAJOR) != 0)) bad = 1;
      if (pc->flags & BF_PIECE_IDENTITY) bad |= !fitsIn(pc->inOff, mr, inLen);
      else if (pl->transposed && rm)      /* rows of a row-major forward piece: ncols rows, mr columns from dataOff */
        bad |= !pc->ld || pc->ld % pl->epl || pc->dataOff % pl->epl || bfDtypeC128Layout(pl->dtype) || !pc->ncols ||
               !fitsIn(pc->dataOff, mulAddSat(pc->ncols - 1, pc->ld, (mr + pl->epl - 1) / pl->epl * pl->epl), arenaElems) ||
               !fitsIn(pc->inOff, pc->ncols, inLen);
      else if (rm)
        bad |= !pc->ncols || pc->ld % pl->epl || pc->ld < pc->ncols || pc->dataOff % pl->epl ||   /* x is read from global memory: no xcap */
               !fitsIn(pc->dataOff, mulAddSat(mr, pc->ld, 0), arenaElems) || !fitsIn(pc->inOff, pc->ncols, inLen);
      else if (pl->transposed)
        bad |= !pc->ld || pc->ld % pl->epl || pc->ncols > pc->ld || pc->dataOff % pl->epl ||
               !fitsIn(pc->dataOff, mulAddSat(mr - 1, pc->ld, (pc->ncols + pl->epl - 1) / pl->epl * pl->epl), arenaElems) ||
               !fitsIn(pc->inOff, pc->ncols, inLen);
      else
        bad |= !pc->ncols || pc->ncols > pl->xcap || pc->dataOff % pl->epl ||
               !fitsIn(pc->dataOff, mulAddSat(mrPad, pc->ncols, 0), arenaElems) || !fitsIn(pc->inOff, pc->ncols, inLen);
      if (bad) return bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt operator file: piece %u of item %llu out of bounds", k, (unsigned long long)i);
    }
  }
  return 0;
}

static int validateReduce(BfPlan const *pl, BfReduce const *rd, uint32_t const *rowInterval, uint32_t const *ivBegin, int64_t const *srcBias) {
  uint64_t const destLen = rd->destSpace == BF_SPACE_Y ? pl->numRows : pl->tempElems;
  if ((rd->destSpace != BF_SPACE_Y && rd->destSpace != BF_SPACE_TEMP) || !fitsIn(rd->destOff, rd->numRows, destLen) || rd->numIntervals > rd->numRows + 1)
    return bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt operator file: reduce destination out of bounds");
  if (ivBegin[0] != 0 || ivBegin[rd->numIntervals] > rd->numSrc) return bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt operator file: reduce interval table");
  for (uint64_t i = 0; i < rd->numIntervals; ++i)
    if (ivBegin[i + 1] < ivBegin[i]) return bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt operator file: reduce interval table not monotone");
  for (uint64_t r = 0; r < rd->numRows; ++r) {
    uint32_t const iv = rowInterval[r];
    if (iv == BF_REDUCE_SKIP) continue;
    if (iv >= rd->numIntervals) return bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt operator file: reduce row %llu", (unsigned long long)r);
    for (uint32_t k = ivBegin[iv]; k < ivBegin[iv + 1]; ++k) {
      int64_t src;
      if (__builtin_add_overflow(srcBias[k], (int64_t)r, &src) || src < 0 || (uint64_t)src >= pl->tempElems) return bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt operator file: reduce source out of bounds");
    }
  }
  return 0;
}

static int loadPlan(FILE *fp, BfhipOperator *op, BfPlan *pl, FileHeader const *fh, uint64_t arenaElems) {
  FilePlanHeader ph;
  int rc = readAll(fp, &ph, sizeof ph);
  if (rc) return rc;
  if (ph.numStages > (1u << 20) || ph.tempElems >= 0xffffffffu) return bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt plan header");
  pl->dtype = fh->dtype; pl->elemSize = fh->elemSize; pl->epl = fh->epl; pl->xcap = fh->xcap;
  pl->maxItemRows = ph.maxItemRows; pl->transposed = (int)ph.transposed;
  pl->numRows = ph.numRows; pl->numCols = ph.numCols; pl->numStages = ph.numStages; pl->tempElems = ph.tempElems;
  pl->arenaElems = pl->transposed ? 0 : arenaElems;
  pl->leafElems = fh->leafElems; pl->numLeaves = fh->numLeaves;
  if (pl->epl != 16 / pl->elemSize || pl->xcap != 256 || pl->maxItemRows > 64 * pl->epl || (pl->transposed && pl->maxItemRows > 128))
    return bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt plan header (lane granule / piece width / item height)");
  pl->stages = calloc(ph.numStages ? ph.numStages : 1, sizeof(BfStage));
  if (!pl->stages) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  for (uint64_t s = 0; s < pl->numStages && !rc; ++s) {
    BfStage *st = &pl->stages[s];
    FileStageHeader sh;
    if ((rc = readAll(fp, &sh, sizeof sh))) break;
    if (sh.numItems > 0xffffffffu || sh.numPieces > 0xffffffffu || sh.numReduce > (1u << 20)) { rc = bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt stage header"); break; }
    st->numItems = sh.numItems; st->numPieces = sh.numPieces; st->leafElems = sh.leafElems; st->vecIn = sh.vecIn; st->vecOut = sh.vecOut;
    st->maxRows = sh.maxRows;
    void *hItems = NULL, *hPieces = NULL;
    rc = readMetaArray(fp, &st->dItems, &hItems, st->numItems * sizeof(BfDevItem), &op->metaBytes);
    if (!rc) rc = readMetaArray(fp, &st->dPieces, &hPieces, st->numPieces * sizeof(BfDevPiece), &op->metaBytes);
    if (!rc) {       /* small items are the tail of the list (validateStage checks that they are nowhere else) */
      st->firstSmall = st->numItems;
      while (st->firstSmall && (((BfDevItem const *)hItems)[st->firstSmall - 1].mrFlags & BF_ITEM_SMALL)) --st->firstSmall;
      st->numNarrow = 0;
      while (st->numNarrow < st->numItems && (((BfDevItem const *)hItems)[st->numNarrow].mrFlags & BF_ITEM_TNARROW)) ++st->numNarrow;
      rc = validateStage(pl, arenaElems, st, hItems, hPieces);
      if (!rc && pl->transposed) {
        st->maxRowsRest = 0;
        for (uint64_t i = st->numNarrow; i < st->numItems; ++i) {
          uint32_t const mr = ((BfDevItem const *)hItems)[i].mrFlags & 0xffffu;
          if (mr > st->maxRowsRest) st->maxRowsRest = mr;
        }
        st->numCoopNarrow = bfPlanCountCoop(hItems, hPieces, st->numNarrow, pl->elemSize);
        st->numCoop = bfPlanCountCoop((BfDevItem const *)hItems + st->numNarrow, hPieces, st->numItems - st->numNarrow, pl->elemSize);
      }
    }
    free(hItems); free(hPieces);
    if (!rc && sh.numReduce) {
      st->reduce = calloc(sh.numReduce, sizeof(BfReduce));
      if (!st->reduce) rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
    }
    for (uint64_t r = 0; r < sh.numReduce && !rc; ++r) {
      BfReduce *rd = &st->reduce[r];
      FileReduceHeader rh;
      if ((rc = readAll(fp, &rh, sizeof rh))) break;
      st->numReduce = r + 1;
      rd->destOff = rh.destOff; rd->numRows = rh.numRows; rd->numIntervals = rh.numIntervals; rd->numSrc = rh.numSrc; rd->destSpace = rh.destSpace;
      if (rd->numRows >= 0xffffffffu || rd->numIntervals >= 0xffffffffu || rd->numSrc >= 0xffffffffu) { rc = bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt reduce header"); break; }
      void *hRow = NULL, *hIv = NULL, *hBias = NULL;
      rc = readMetaArray(fp, &rd->dRowInterval, &hRow, rd->numRows * 4, &op->metaBytes);
      if (!rc) rc = readMetaArray(fp, &rd->dIvBegin, &hIv, (rd->numIntervals + 1) * 4, &op->metaBytes);
      if (!rc) rc = readMetaArray(fp, &rd->dSrcBias, &hBias, rd->numSrc * 8, &op->metaBytes);
      if (!rc) rc = validateReduce(pl, rd, hRow, hIv, hBias);
      if (!rc) {
        uint32_t const *iv = hIv;
        rd->maxSrc = 0;
        for (uint64_t i = 0; i < rd->numIntervals; ++i) if (iv[i + 1] - iv[i] > rd->maxSrc) rd->maxSrc = iv[i + 1] - iv[i];
      }
      free(hRow); free(hIv); free(hBias);
    }
  }
  return rc;
}

int bfhipSave(BfhipOperator *op, char const *path) {
  if (!op || !path) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  if (op->flags & BFHIP_FLAG_PLAN_ONLY) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "a plan-only operator has no device data to save");
  BfDevScope ds;
  int rc = bfDevEnter(&ds, op->device);
  if (rc) return rc;
  if ((rc = bfdevSync(NULL))) goto out;
  FILE *fp = fopen(path, "wb");
  if (!fp) { rc = bfhipFail(BFABI_ERROR_FILE_ERROR, "cannot open %s for writing", path); goto out; }
  FileHeader fh;
  memset(&fh, 0, sizeof fh);
  memcpy(fh.magic, BFHIP_FILE_MAGIC, 8);
  fh.version = 1; fh.dtype = op->plan.dtype; fh.srcDtype = op->srcDtype; fh.elemSize = op->plan.elemSize; fh.epl = op->plan.epl;
  fh.xcap = op->plan.xcap; fh.hasTplan = (uint32_t)op->hasTplan;
  fh.reserved = op->dArenaT ? 1u : 0u;        /* bit 0: the adjoint plan is a forward plan of the transposed expression over a second arena (BFHIP_FLAG_ADJOINT_PACKED) */
  fh.numRows = op->plan.numRows; fh.numCols = op->plan.numCols; fh.arenaElems = op->plan.arenaElems;
  fh.leafElems = op->plan.leafElems; fh.numLeaves = op->plan.numLeaves; fh.leafBytesAlgorithmic = op->leafBytesAlgorithmic;
  rc = writeAll(fp, &fh, sizeof fh);
  uint64_t const arenaElemsT = op->dArenaT ? op->tplan.arenaElems : 0;
  if (!rc && op->dArenaT) rc = writeAll(fp, &arenaElemsT, sizeof arenaElemsT);
  if (!rc) rc = savePlan(fp, &op->plan);
  if (!rc && op->hasTplan) rc = savePlan(fp, &op->tplan);
  if (!rc) rc = writeDeviceArray(fp, op->dArena, (size_t)op->plan.arenaElems * op->plan.elemSize);
  if (!rc && op->dArenaT) rc = writeDeviceArray(fp, op->dArenaT, (size_t)arenaElemsT * op->plan.elemSize);
  if (fclose(fp) != 0 && !rc) rc = bfhipFail(BFABI_ERROR_FILE_ERROR, "error closing %s", path);
out:
  bfDevLeave(&ds);
  return rc;
}

int bfhipLoad(char const *path, BfhipOptions const *opts, BfhipOperator **out) {
  if (!path || !out) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL argument");
  *out = NULL;
  BfhipOptions o;
  memset(&o, 0, sizeof o);
  o.device = -1;
  if (opts) {
    if (opts->structSize < BFHIP_OPTIONS_SIZE_V1) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BfhipOptions.structSize too small");
    memcpy(&o, opts, opts->structSize < sizeof o ? opts->structSize : sizeof o);
  }
  if (o.flags & BFHIP_FLAG_PLAN_ONLY) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "cannot load as plan-only");
  FILE *fp = fopen(path, "rb");
  if (!fp) return bfhipFail(BFABI_ERROR_FILE_ERROR, "cannot open %s", path);
  FileHeader fh;
  int rc = readAll(fp, &fh, sizeof fh);
  if (!rc && (memcmp(fh.magic, BFHIP_FILE_MAGIC, 8) != 0 || fh.version != 1 || fh.dtype > BFHIP_C64 ||
              fh.elemSize != bfDtypeElemSize(fh.dtype) || (fh.dtype == BFHIP_C64 && fh.srcDtype != BFHIP_C128)))
    rc = bfhipFail(BFABI_ERROR_FILE_ERROR, "%s is not a bfhip operator file (bad magic / version / dtype)", path);
  if (rc) { fclose(fp); return rc; }
  BfhipOperator *op = calloc(1, sizeof *op);
  if (!op) { fclose(fp); return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); }
  BfDevScope ds = {0};
  op->flags = o.flags & ~(uint32_t)(BFHIP_FLAG_ADJOINT | BFHIP_FLAG_ADJOINT_PACKED);
  op->srcDtype = fh.srcDtype;
  op->leafBytesAlgorithmic = fh.leafBytesAlgorithmic;
  if ((rc = bfDevEnter(&ds, o.device))) goto done;
  if ((rc = bfdevGetDevice(&op->device))) goto done;      /* o.device may be -1: the operator lives on the current device */
  uint64_t arenaElemsT = 0;
  int const packedT = (fh.reserved & 1u) != 0;
  if (fh.reserved & ~1u) { rc = bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt operator file (header flags)"); goto done; }
  if (packedT && (!fh.hasTplan || (rc = readAll(fp, &arenaElemsT, sizeof arenaElemsT)))) { if (!rc) rc = bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt operator file (packed adjoint without a plan)"); goto done; }
  if ((rc = loadPlan(fp, op, &op->plan, &fh, fh.arenaElems))) goto done;
  if (fh.hasTplan) {
    if ((rc = loadPlan(fp, op, &op->tplan, &fh, packedT ? arenaElemsT : fh.arenaElems))) goto done;
    /* a packed adjoint plan is a FORWARD plan over its own arena, a shared one a transposed plan over the forward arena */
    if ((op->tplan.transposed != 0) == packedT) { rc = bfhipFail(BFABI_ERROR_FILE_ERROR, "corrupt operator file (adjoint plan kind)"); goto done; }
    op->hasTplan = 1;
    op->packedT = packedT;
    op->flags |= packedT ? BFHIP_FLAG_ADJOINT_PACKED : BFHIP_FLAG_ADJOINT;
  }
  if ((rc = readDeviceArray(fp, &op->dArena, (size_t)fh.arenaElems * fh.elemSize, NULL))) goto done;
  if (packedT && (rc = readDeviceArray(fp, &op->dArenaT, (size_t)arenaElemsT * fh.elemSize, NULL))) goto done;
  if ((rc = finishOperator(op, o.maxRhs))) goto done;
done:
  fclose(fp);
  if (rc) bfhipFree(&op);
  bfDevLeave(&ds);
  if (rc) return rc;
  *out = op;
  return 0;
}
