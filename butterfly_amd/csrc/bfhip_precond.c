/* bfhip_precond.c -- block-Jacobi preconditioners built on the device from a compiled operator (include/bfhip.h,
 * "block-Jacobi preconditioner").
 *
 * The direct part of the operator is read from its FORWARD plan: a piece that reads x (BF_PIECE_IN_X) contributes to y when
 * its item writes y (BF_ITEM_OUT_Y), or writes vector-arena rows that a reduce of the same stage sums into y (destSpace Y:
 * y[r] += temp[srcBias + r] for every source of r's interval).  The plan tables are the host mirrors on a plan-only
 * operator and are downloaded from the device otherwise (the mirrors are dropped after compile), so compile, the device
 * builders and bfhipLoad need nothing new.
 *
 * From the direct pieces: (1) the automatic cuts -- the row and column ranges of every dense direct piece that meets the
 * diagonal, merged into connected intervals (identity pieces cover their diagonal entries only); (2) per block the list of
 * sub-rectangles of direct pieces that fall inside D_b x D_b, in a fixed order (stage, item, piece).  Three kernels
 * (bfhip_precond.hip) gather the blocks into a workspace in double precision, invert them and write the result's arena;
 * the result is compiled as a BlockDiag of dense leaves through bfhipCompileIrFill.
 *
 * This file is not part of the host sanitizer harness (tests/test_host_asan.py): it calls the new device launchers.
 * Neither bfhip_api.c nor bfhip_file.c, bfhip_shim.c or bfhip_inspect.c references it. */
#define _GNU_SOURCE
#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#define BJ_DEFAULT_MAX_BLOCK 128u

/* one direct contribution: item rows [pr0, pr0 + nr) of a piece, landing on y rows [y0, y0 + nr) */
typedef struct BjDirect {
  uint64_t dataOff;
  uint64_t y0;
  uint32_t pr0, nr;
  uint32_t inOff, ncols;
  uint32_t mrPad, ld;        /* column-major row stride of the piece / row-major row stride */
  uint32_t identity, rowMajor;
} BjDirect;

typedef struct BjDirectList { BjDirect *d; uint64_t n, cap; } BjDirectList;

static int pushDirect(BjDirectList *L, BjDirect const *e) {
  if (L->n == L->cap) {
    uint64_t const cap = L->cap ? 2 * L->cap : 4096;
    BjDirect *p = realloc(L->d, cap * sizeof *p);
    if (!p) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (direct pieces)");
    L->d = p; L->cap = cap;
  }
  L->d[L->n++] = *e;
  return 0;
}

/* a plan table: the host mirror, or a downloaded copy (owned) */
static int table(void const *host, void const *dev, size_t bytes, int planOnly, void **out, int *owned) {
  *owned = 0;
  if (planOnly || !bytes) { *out = (void *)host; return 0; }
  void *h = malloc(bytes);
  if (!h) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (plan tables)");
  int rc = bfdevMemcpyD2H(h, dev, bytes);
  if (rc) { free(h); return rc; }
  *out = h; *owned = 1;
  return 0;
}

/* every direct contribution of the forward plan, in (stage, item, piece) order.  The caller's device is the operator's. */
static int collectDirect(BfhipOperator const *op, BjDirectList *L) {
  BfPlan const *pl = bfhipOperatorPlan(op);
  int const planOnly = bfhipOperatorDevice(op) < 0;
  uint64_t const T = pl->tempElems;
  int64_t *tmap = malloc((T ? T : 1) * sizeof *tmap);     /* vector-arena row -> the y row a reduce of this stage sums it into */
  if (!tmap) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (reduce map)");
  int rc = 0;
  for (uint64_t s = 0; s < pl->numStages && !rc; ++s) {
    BfStage const *st = &pl->stages[s];
    BfDevItem *items = NULL;
    BfDevPiece *pieces = NULL;
    int ownI = 0, ownP = 0;
    if ((rc = table(st->items, st->dItems, st->numItems * sizeof(BfDevItem), planOnly, (void **)&items, &ownI))) break;
    if ((rc = table(st->pieces, st->dPieces, st->numPieces * sizeof(BfDevPiece), planOnly, (void **)&pieces, &ownP))) { if (ownI) free(items); break; }
    for (uint64_t t = 0; t < T; ++t) tmap[t] = -1;
    for (uint64_t r = 0; r < st->numReduce && !rc; ++r) {
      BfReduce const *rd = &st->reduce[r];
      if (rd->destSpace != BF_SPACE_Y || !rd->numRows) continue;
      uint32_t *ri = NULL, *ib = NULL;
      int64_t *sb = NULL;
      int o1 = 0, o2 = 0, o3 = 0;
      rc = table(rd->rowInterval, rd->dRowInterval, rd->numRows * 4, planOnly, (void **)&ri, &o1);
      if (!rc) rc = table(rd->ivBegin, rd->dIvBegin, (rd->numIntervals + 1) * 4, planOnly, (void **)&ib, &o2);
      if (!rc) rc = table(rd->srcBias, rd->dSrcBias, rd->numSrc * 8, planOnly, (void **)&sb, &o3);
      for (uint64_t row = 0; row < rd->numRows && !rc; ++row) {
        uint32_t const iv = ri[row];
        if (iv == BF_REDUCE_SKIP || iv >= rd->numIntervals) continue;
        for (uint32_t k = ib[iv]; k < ib[iv + 1] && k < rd->numSrc; ++k) {
          int64_t const t = sb[k] + (int64_t)row;       /* y rows of a y-reduce are its own rows (runPlan: dest = y) */
          if (t >= 0 && (uint64_t)t < T) tmap[t] = (int64_t)row;
        }
      }
      if (o1) free(ri);
      if (o2) free(ib);
      if (o3) free(sb);
    }
    for (uint64_t i = 0; i < st->numItems && !rc; ++i) {
      BfDevItem const *it = &items[i];
      uint32_t const mr = it->mrFlags & 0xffffu;
      uint32_t const mrPad = (mr + pl->epl - 1) / pl->epl * pl->epl;
      int const outY = (it->mrFlags & BF_ITEM_OUT_Y) != 0;
      for (uint32_t k = 0; k < it->numPieces && !rc; ++k) {
        BfDevPiece const *pc = &pieces[it->pieceBegin + k];
        if (!(pc->flags & BF_PIECE_IN_X)) continue;
        BjDirect e;
        memset(&e, 0, sizeof e);
        e.dataOff = pc->dataOff; e.inOff = pc->inOff; e.ncols = pc->ncols; e.mrPad = mrPad; e.ld = pc->ld;
        e.identity = (pc->flags & BF_PIECE_IDENTITY) != 0;
        e.rowMajor = (pc->flags & BF_PIECE_ROWMAJOR) != 0;
        if (outY) {
          e.y0 = it->outOff; e.pr0 = 0; e.nr = mr;
          rc = pushDirect(L, &e);
          continue;
        }
        /* vector-arena rows: the runs of rows a y-reduce maps to consecutive y rows */
        uint32_t r = 0;
        while (r < mr && !rc) {
          uint64_t const t = (uint64_t)it->outOff + r;
          if (t >= T || tmap[t] < 0) { ++r; continue; }
          uint32_t q = r + 1;
          while (q < mr && (uint64_t)it->outOff + q < T && tmap[it->outOff + q] == tmap[t] + (int64_t)(q - r)) ++q;
          e.y0 = (uint64_t)tmap[t]; e.pr0 = r; e.nr = q - r;
          rc = pushDirect(L, &e);
          r = q;
        }
      }
    }
    if (ownI) free(items);
    if (ownP) free(pieces);
  }
  free(tmap);
  return rc;
}

/* reach[lo] = the largest end of a connected interval starting at lo (-1: none) from the direct pieces that meet the
 * diagonal; then *covered* rows are those inside an interval */
static int diagonalIntervals(BjDirectList const *L, uint64_t n, int64_t *reach) {
  for (uint64_t i = 0; i < n; ++i) reach[i] = -1;
  for (uint64_t k = 0; k < L->n; ++k) {
    BjDirect const *e = &L->d[k];
    uint64_t const r0 = e->y0, r1 = e->y0 + e->nr;
    if (e->identity) {
      /* item row pr0 + t reads input row inOff + pr0 + t: on the diagonal iff y0 == inOff + pr0 */
      if (r0 != (uint64_t)e->inOff + e->pr0) continue;
      for (uint64_t y = r0; y < r1 && y < n; ++y) if (reach[y] < (int64_t)y + 1) reach[y] = (int64_t)y + 1;
      continue;
    }
    uint64_t const c0 = e->inOff, c1 = (uint64_t)e->inOff + e->ncols;
    uint64_t const lo = r0 > c0 ? r0 : c0, hi = r1 < c1 ? r1 : c1;
    if (lo >= hi) continue;                 /* the rectangle misses the diagonal */
    uint64_t const a = r0 < c0 ? r0 : c0, b = r1 > c1 ? r1 : c1;
    if (b > n) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "direct piece reaches past the operator's %llu rows", (unsigned long long)n);
    if (reach[a] < (int64_t)b) reach[a] = (int64_t)b;
  }
  return 0;
}

/* automatic partition: cuts[0..numBlocks] (at most `cap` written; cuts == NULL: count only), the uncovered rows, the longest
block, and the covered mask (may be NULL) */
static void autoPartition(int64_t const *reach, uint64_t n, uint64_t *cuts, uint64_t cap, uint64_t *numBlocks, uint64_t *uncovered,
                          uint64_t *longest, uint8_t *covered) {
  uint64_t nb = 0, unc = 0, lng = 0, i = 0;
  if (cuts && cap) cuts[0] = 0;
  while (i < n) {
    uint64_t end;
    if (reach[i] < 0) {
      end = i + 1; ++unc;
      if (covered) covered[i] = 0;
    } else {
      end = (uint64_t)reach[i];
      for (uint64_t j = i + 1; j < end; ++j) if (reach[j] > (int64_t)end) end = (uint64_t)reach[j];
      if (covered) memset(covered + i, 1, end - i);
    }
    if (end - i > lng) lng = end - i;
    ++nb;
    if (cuts && nb < cap) cuts[nb] = end;
    i = end;
  }
  *numBlocks = nb; *uncovered = unc; *longest = lng;
}

typedef struct BjTaskList { BfBjTask *t; uint64_t *block; uint64_t n, cap; } BjTaskList;

static int pushTask(BjTaskList *L, BfBjTask const *t, uint64_t block) {
  if (L->n == L->cap) {
    uint64_t const cap = L->cap ? 2 * L->cap : 4096;
    BfBjTask *p = realloc(L->t, cap * sizeof *p);
    if (!p) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (block pieces)");
    L->t = p;
    uint64_t *q = realloc(L->block, cap * sizeof *q);
    if (!q) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (block pieces)");
    L->block = q; L->cap = cap;
  }
  L->t[L->n] = *t; L->block[L->n] = block; ++L->n;
  return 0;
}

static int checkSquare(BfhipOperator const *op) {
  if (!op) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator");
  BfPlan const *pl = bfhipOperatorPlan(op);
  if (pl->numRows != pl->numCols)
    return bfhipFail(BFABI_ERROR_INCOMPATIBLE_SHAPES, "block-Jacobi needs a square operator (%llu x %llu)", (unsigned long long)pl->numRows,
                     (unsigned long long)pl->numCols);
  if (pl->numRows > 0xffffffffull) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "operator too large");
  return 0;
}

int bfhipBlockJacobiPartition(BfhipOperator const *op, uint32_t maxBlock, uint64_t *cuts, uint64_t cap, uint64_t *numBlocks) {
  int rc = checkSquare(op);
  if (rc) return rc;
  if (!numBlocks || (cap && !cuts)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL numBlocks / cuts");
  if (maxBlock > BFHIP_BJ_MAX_BLOCK) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "maxBlock %u > %u", maxBlock, BFHIP_BJ_MAX_BLOCK);
  if (!maxBlock) maxBlock = BJ_DEFAULT_MAX_BLOCK;
  uint64_t const n = bfhipOperatorPlan(op)->numRows;
  BjDirectList L = {0};
  int64_t *reach = malloc((n ? n : 1) * sizeof *reach);
  BfDevScope ds = {0};
  if (!reach) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); goto out; }
  if ((rc = bfDevEnter(&ds, bfhipOperatorDevice(op)))) goto out;      /* -1 (plan-only): no device is touched */
  if ((rc = collectDirect(op, &L))) goto out;
  if ((rc = diagonalIntervals(&L, n, reach))) goto out;
  uint64_t nb = 0, unc = 0, lng = 0;
  autoPartition(reach, n, cuts, cap, &nb, &unc, &lng, NULL);
  if (lng > maxBlock) {
    rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "an automatic diagonal block has %llu rows > maxBlock %u: pass cuts", (unsigned long long)lng, maxBlock);
    goto out;
  }
  *numBlocks = nb;
out:
  bfDevLeave(&ds);
  free(reach);
  free(L.d);
  return rc;
}

/* ---- the result's arena: one fill launch over the result plan's pieces ---- */
typedef struct BjFillCtx {
  void const *ws;            /* workspace on the operator's device */
  int wsDevice;
  uint64_t wsBytes;
  BfBjBlock const *blocks;   /* host */
  uint64_t numBlocks;
} BjFillCtx;

static int fillResult(BfPlan const *pl, BfIr const *ir, void *dArena, void *vctx) {
  BjFillCtx const *ctx = vctx;
  uint64_t np = 0;
  for (uint64_t s = 0; s < pl->numStages; ++s) np += pl->stages[s].numPieces;
  BfBjFillPiece *fp = malloc((np ? np : 1) * sizeof *fp);
  if (!fp) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM (fill pieces)");
  uint64_t k = 0;
  int rc = 0;
  for (uint64_t s = 0; s < pl->numStages && !rc; ++s) {
    BfStage const *st = &pl->stages[s];
    for (uint64_t i = 0; i < st->numItems && !rc; ++i) {
      BfDevItem const *it = &st->items[i];
      uint32_t const mr = it->mrFlags & 0xffffu;
      for (uint32_t q = 0; q < it->numPieces; ++q) {
        BfDevPiece const *pc = &st->pieces[it->pieceBegin + q];
        BfPieceSrc const *src = &st->pieceSrc[it->pieceBegin + q];
        if (pc->flags & BF_PIECE_IDENTITY) continue;
        if (src->node >= ctx->numBlocks || ir->kind[src->node] != BFHIP_NODE_DENSE) { rc = bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "unexpected leaf %llu", (unsigned long long)src->node); break; }
        BfBjFillPiece *f = &fp[k++];
        f->dataOff = pc->dataOff; f->wsOff = ctx->blocks[src->node].wsOff; f->m = ctx->blocks[src->node].m;
        f->row0 = src->row0; f->col0 = src->col0; f->mr = mr; f->mrPad = (mr + pl->epl - 1) / pl->epl * pl->epl;
        f->ncols = pc->ncols; f->rowMajor = (pc->flags & BF_PIECE_ROWMAJOR) != 0; f->ld = pc->ld;
      }
    }
  }
  void *dFp = NULL, *wsHere = NULL;
  void const *ws = ctx->ws;
  int dev = -1;
  if (!rc) rc = bfdevGetDevice(&dev);
  if (!rc && dev != ctx->wsDevice) {
    /* the result lives on another device: a copy of the workspace there */
    if (!(rc = bfdevMalloc(&wsHere, ctx->wsBytes ? ctx->wsBytes : 16))) rc = bfdevMemcpyAnyAsync(wsHere, ctx->ws, ctx->wsBytes, NULL);
    if (!rc) rc = bfdevSync(NULL);
    ws = wsHere;
  }
  if (!rc && k) rc = bfdevMalloc(&dFp, k * sizeof *fp);
  if (!rc && k) rc = bfdevMemcpyH2D(dFp, fp, k * sizeof *fp);
  if (!rc && k) rc = bfdevBjFill(dArena, pl->dtype, ws, dFp, k, NULL);
  if (!rc) rc = bfdevSync(NULL);
  bfdevFree(dFp);
  bfdevFree(wsHere);
  free(fp);
  return rc;
}

static int demotable(uint32_t from, uint32_t to) {
  if (from == to) return 1;
  return (from == BFHIP_C128 && to == BFHIP_C64) || (from == BFHIP_F64 && to == BFHIP_F32);
}

int bfhipBlockJacobi(BfhipOperator *op, BfhipBlockJacobiOptions const *opt, BfhipOperator **pre, BfhipBlockJacobiInfo *info) {
  if (!pre) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL result pointer");
  *pre = NULL;
  int rc = checkSquare(op);
  if (rc) return rc;
  BfhipBlockJacobiOptions o;
  memset(&o, 0, sizeof o);
  o.device = -1;
  if (opt) {
    if (opt->structSize < sizeof o) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BfhipBlockJacobiOptions.structSize too small");
    o = *opt;
  }
  if (info && info->structSize < sizeof *info) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "BfhipBlockJacobiInfo.structSize too small");
  if (o.flags & ~BFHIP_BJ_NO_INVERT) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "unknown block-Jacobi flags 0x%x", o.flags);
  if (o.maxBlock > BFHIP_BJ_MAX_BLOCK) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "maxBlock %u > %u", o.maxBlock, BFHIP_BJ_MAX_BLOCK);
  uint32_t const maxBlock = o.maxBlock ? o.maxBlock : BJ_DEFAULT_MAX_BLOCK;
  BfPlan const *pl = bfhipOperatorPlan(op);
  uint32_t const srcDt = pl->dtype;
  uint32_t const outDt = o.outDtype ? o.outDtype : srcDt;
  if (!bfDtypeKnown(outDt) || !demotable(srcDt, outDt))
    return bfhipFail(BFABI_ERROR_TYPE_ERROR, "outDtype %u: a dtype-%u operator can only give its own dtype or its demotion", outDt, srcDt);
  uint64_t const n = pl->numRows;
  if (o.cuts) {
    if (!o.numBlocks || o.cuts[0] != 0 || o.cuts[o.numBlocks] != n)
      return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "cuts must run from 0 to %llu", (unsigned long long)n);
    for (uint64_t b = 0; b < o.numBlocks; ++b) {
      if (o.cuts[b + 1] <= o.cuts[b]) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "cuts are not strictly increasing at %llu", (unsigned long long)b);
      if (o.cuts[b + 1] - o.cuts[b] > maxBlock)
        return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "block %llu has %llu rows > maxBlock %u", (unsigned long long)b,
                         (unsigned long long)(o.cuts[b + 1] - o.cuts[b]), maxBlock);
    }
  } else if (o.numBlocks) {
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "numBlocks without cuts");
  }
  int const planOnly = bfhipOperatorDevice(op) < 0;
  int const cplx = bfDtypeComplex(srcDt);
  size_t const wes = cplx ? 16 : 8;
  double const t0 = bfNowSeconds();
  double t1 = t0, t2 = t0;

  BjDirectList L = {0};
  int64_t *reach = NULL;
  uint8_t *covered = NULL;
  uint64_t *cuts = NULL, *blockOf = NULL;
  BjTaskList TL = {0};
  BfBjTask *sorted = NULL;
  BfBjBlock *blocks = NULL;
  BfBjResult *res = NULL;
  uint64_t *cnt = NULL;
  uint64_t nb = 0, unc = 0, lng = 0;
  void *dWs = NULL, *dBlocks = NULL, *dTasks = NULL, *dRes = NULL;
  uint64_t *descArrays = NULL;
  uint8_t *kinds = NULL;
  BfDevScope ds = {0};
  int64_t firstSingular = -1;
  double minPivotRel = NAN;
  uint64_t wsElems = 0;

  reach = malloc((n ? n : 1) * sizeof *reach);
  covered = malloc(n ? n : 1);
  if (!reach || !covered) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); goto out; }
  if ((rc = bfDevEnter(&ds, bfhipOperatorDevice(op)))) goto out;      /* -1 (plan-only): no device is touched */
  if ((rc = collectDirect(op, &L))) goto out;
  if ((rc = diagonalIntervals(&L, n, reach))) goto out;
  autoPartition(reach, n, NULL, 0, &nb, &unc, &lng, covered);
  if (o.cuts) {
    nb = o.numBlocks;
    cuts = malloc((nb + 1) * sizeof *cuts);
    if (!cuts) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); goto out; }
    memcpy(cuts, o.cuts, (nb + 1) * sizeof *cuts);
  } else {
    if (lng > maxBlock) {
      rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "an automatic diagonal block has %llu rows > maxBlock %u: pass cuts", (unsigned long long)lng, maxBlock);
      goto out;
    }
    cuts = malloc((nb + 1) * sizeof *cuts);
    if (!cuts) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); goto out; }
    autoPartition(reach, n, cuts, nb + 1, &nb, &unc, &lng, NULL);
  }
  if (planOnly) { rc = bfhipFail(BFABI_ERROR_NOT_IMPLEMENTED, "bfhipBlockJacobi needs a device operator (this one was compiled with BFHIP_FLAG_PLAN_ONLY)"); goto out; }

  /* blocks and the workspace layout */
  blocks = calloc(nb ? nb : 1, sizeof *blocks);
  blockOf = malloc((n ? n : 1) * sizeof *blockOf);
  if (!blocks || !blockOf) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); goto out; }
  uint64_t maxRows = 0;
  for (uint64_t b = 0; b < nb; ++b) {
    uint64_t const m = cuts[b + 1] - cuts[b];
    blocks[b].wsOff = wsElems; blocks[b].m = (uint32_t)m;
    wsElems += m * m;
    if (m > maxRows) maxRows = m;
    for (uint64_t r = cuts[b]; r < cuts[b + 1]; ++r) blockOf[r] = b;
  }
  /* tasks: sub-rectangles of the direct pieces inside the diagonal blocks, then the 1s of uncovered rows */
  for (uint64_t k = 0; k < L.n; ++k) {
    BjDirect const *e = &L.d[k];
    uint64_t y = e->y0;
    uint64_t const yEnd = e->y0 + e->nr;
    if (yEnd > n) { rc = bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "direct piece reaches past row %llu", (unsigned long long)n); goto out; }
    while (y < yEnd) {
      uint64_t const b = blockOf[y];
      uint64_t const cb0 = cuts[b], cb1 = cuts[b + 1];
      uint64_t const ya = y, yb = yEnd < cb1 ? yEnd : cb1;
      BfBjTask t;
      memset(&t, 0, sizeof t);
      if (e->identity) {
        /* entries (y, y + delta) for y in [ya, yb) */
        int64_t const delta = (int64_t)e->inOff + e->pr0 - (int64_t)e->y0;
        int64_t lo = (int64_t)ya, hi = (int64_t)yb;
        if (lo < (int64_t)cb0 - delta) lo = (int64_t)cb0 - delta;
        if (hi > (int64_t)cb1 - delta) hi = (int64_t)cb1 - delta;
        if (lo < hi) {
          t.br = (uint32_t)((uint64_t)lo - cb0); t.bc = (uint32_t)((uint64_t)(lo + delta) - cb0);
          t.nr = t.nc = (uint32_t)(hi - lo);
          if ((rc = pushTask(&TL, &t, b))) goto out;
        }
      } else {
        uint64_t const c0 = e->inOff, c1 = (uint64_t)e->inOff + e->ncols;
        uint64_t const ca = c0 > cb0 ? c0 : cb0, cc = c1 < cb1 ? c1 : cb1;
        if (ca < cc) {
          uint64_t const pr = e->pr0 + (ya - e->y0), pcol = ca - c0;
          t.br = (uint32_t)(ya - cb0); t.bc = (uint32_t)(ca - cb0);
          t.nr = (uint32_t)(yb - ya); t.nc = (uint32_t)(cc - ca);
          if (e->rowMajor) { t.ldr = e->ld; t.ldc = 1; }
          else { t.ldr = 1; t.ldc = e->mrPad; }
          t.dataOff = e->dataOff + pr * t.ldr + pcol * t.ldc;
          if ((rc = pushTask(&TL, &t, b))) goto out;
        }
      }
      y = yb;
    }
  }
  for (uint64_t r = 0; r < n;) {
    if (covered[r]) { ++r; continue; }
    uint64_t const b = blockOf[r];
    uint64_t q = r + 1;
    while (q < n && !covered[q] && blockOf[q] == b) ++q;
    BfBjTask t;
    memset(&t, 0, sizeof t);
    t.br = t.bc = (uint32_t)(r - cuts[b]); t.nr = t.nc = (uint32_t)(q - r);
    if ((rc = pushTask(&TL, &t, b))) goto out;
    r = q;
  }
  if (TL.n > 0xffffffffull) { rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "too many block pieces"); goto out; }
  /* grouped by block, in their order inside each (counting sort) */
  cnt = calloc(nb + 1, sizeof *cnt);
  sorted = malloc((TL.n ? TL.n : 1) * sizeof *sorted);
  if (!cnt || !sorted) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); goto out; }
  for (uint64_t k = 0; k < TL.n; ++k) cnt[TL.block[k] + 1] += 1;
  for (uint64_t b = 0; b < nb; ++b) cnt[b + 1] += cnt[b];
  for (uint64_t b = 0; b < nb; ++b) { blocks[b].taskBegin = (uint32_t)cnt[b]; blocks[b].taskEnd = (uint32_t)cnt[b + 1]; }
  for (uint64_t k = 0; k < TL.n; ++k) sorted[cnt[TL.block[k]]++] = TL.t[k];
  uint64_t const numTasks = TL.n;

  /* gather */
  if ((rc = bfdevMalloc(&dWs, wsElems * wes + 16))) goto out;
  if ((rc = bfdevMalloc(&dBlocks, nb * sizeof *blocks + 16))) goto out;
  if ((rc = bfdevMalloc(&dTasks, numTasks * sizeof *sorted + 16))) goto out;
  if ((rc = bfdevMemcpyH2D(dBlocks, blocks, nb * sizeof *blocks))) goto out;
  if ((rc = bfdevMemcpyH2D(dTasks, sorted, numTasks * sizeof *sorted))) goto out;
  if ((rc = bfdevBjGather(dWs, bfhipOperatorArena(op), pl->arenaElems, srcDt, dBlocks, dTasks, nb, NULL))) goto out;
  if ((rc = bfdevSync(NULL))) goto out;
  t1 = bfNowSeconds();

  /* inversion */
  if (!(o.flags & BFHIP_BJ_NO_INVERT)) {
    res = malloc((nb ? nb : 1) * sizeof *res);
    if (!res) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); goto out; }
    if ((rc = bfdevMalloc(&dRes, nb * sizeof *res + 16))) goto out;
    if ((rc = bfdevBjInvert(dWs, cplx, dBlocks, dRes, nb, NULL))) goto out;
    if ((rc = bfdevMemcpyD2H(res, dRes, nb * sizeof *res))) goto out;
    double mpr = INFINITY;
    for (uint64_t b = 0; b < nb; ++b) {
      if (res[b].status && firstSingular < 0) firstSingular = (int64_t)b;
      double const r = res[b].maxAbs > 0 ? res[b].minPivot / res[b].maxAbs : 0.0;
      if (!(r >= mpr)) mpr = r;
    }
    minPivotRel = nb ? mpr : NAN;
    if (firstSingular >= 0) {
      rc = bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "diagonal block %lld (rows %llu..%llu) has a zero or non-finite pivot, pivot reciprocal or scaled pivot row at step %u", (long long)firstSingular,
                     (unsigned long long)cuts[firstSingular], (unsigned long long)cuts[firstSingular + 1], res[firstSingular].step);
      goto out;
    }
  }
  t2 = bfNowSeconds();

  /* the result: a BlockDiag of dense leaves 0..nb-1, root nb */
  {
    uint64_t const nn = nb + 1;
    descArrays = malloc((5 * nn + 2 + 3 * nb) * sizeof *descArrays);
    kinds = malloc(nn);
    if (!descArrays || !kinds) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); goto out; }
    uint64_t *rows = descArrays, *cols = rows + nn, *cb = cols + nn, *chN = cb + nn + 1, *chR = chN + nb, *chC = chR + nb;
    for (uint64_t b = 0; b < nb; ++b) {
      kinds[b] = BFHIP_NODE_DENSE;
      rows[b] = cols[b] = blocks[b].m;
      cb[b] = 0;
      chN[b] = b; chR[b] = chC[b] = cuts[b];
    }
    kinds[nb] = BFHIP_NODE_BLOCK;
    rows[nb] = cols[nb] = n;
    cb[nb] = 0; cb[nb + 1] = nb;
    BfhipDesc d;
    memset(&d, 0, sizeof d);
    d.structSize = sizeof d;
    d.dtype = cplx ? BFHIP_C128 : BFHIP_F64;
    d.numNodes = nn; d.root = nb;
    d.kind = kinds; d.rows = rows; d.cols = cols; d.childBegin = cb; d.childNode = chN; d.childRow0 = chR; d.childCol0 = chC;
    BfIr ir;
    if ((rc = bfIrFromDesc(&d, &ir))) goto out;
    BfhipOptions co;
    memset(&co, 0, sizeof co);
    co.structSize = sizeof co;
    co.device = o.device >= 0 ? o.device : bfhipOperatorDevice(op);
    co.maxRhs = o.maxRhs;
    co.demoteToF32 = outDt != (cplx ? BFHIP_C128 : BFHIP_F64);
    BjFillCtx fc = {dWs, bfhipOperatorDevice(op), wsElems * wes, blocks, nb};
    rc = bfhipCompileIrFill(&ir, &co, fillResult, &fc, pre);      /* consumes ir */
    if (rc) { *pre = NULL; goto out; }
  }

out:
  {
    double const t3 = bfNowSeconds();
    if (info) {
      info->numBlocks = nb; info->maxBlockRows = 0; info->uncoveredRows = unc;
      if (cuts) for (uint64_t b = 0; b < nb; ++b) if (cuts[b + 1] - cuts[b] > info->maxBlockRows) info->maxBlockRows = cuts[b + 1] - cuts[b];
      info->firstSingularBlock = firstSingular;
      info->minPivotRel = minPivotRel;
      info->gatherSeconds = t1 > t0 ? t1 - t0 : 0;
      info->invertSeconds = (o.flags & BFHIP_BJ_NO_INVERT) || t2 < t1 ? 0 : t2 - t1;
      info->compileSeconds = rc || t3 < t2 ? 0 : t3 - t2;
    }
  }
  bfdevFree(dWs); bfdevFree(dBlocks); bfdevFree(dTasks); bfdevFree(dRes);
  bfDevLeave(&ds);
  free(L.d); free(reach); free(covered); free(cuts); free(blockOf); free(TL.t); free(TL.block); free(sorted); free(blocks); free(res); free(cnt);
  free(descArrays); free(kinds);
  return rc;
}
