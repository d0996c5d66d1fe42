/* The planner (bfPlanBuild, bfhip_plan.c) alone, on the CPU, under AddressSanitizer / UBSan / LeakSanitizer, with malloc,
 * calloc and realloc wrapped (-Wl,--wrap=...): built and run by tests/test_plan_oom_cpu.py; the device layer is
 * tests/native/device_stubs.c.
 *
 * For every build of every operand below:
 *   digest  one line "digest <name> <16 hex digits>": a 64-bit FNV-1a hash over every host field of the BfPlan -- what the
 *           inspection C-ABI shows and what it does not (pieceSrc, pieceBuf, itemBuf, bufWriters, flowOk).  The test compares
 *           the lines with tests/golden/plan_fingerprints.json.
 *   sweep   the build's allocations are counted; then it is repeated once per allocation with that allocation failing.  Each
 *           must return BFABI_ERROR_MEMORY_ERROR and leave the BfPlan zeroed; the sanitizers see the rest (leaks, double frees).
 * "flags <name> ..." lines count the item kinds, so that a reader can see which branches an operand drives. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bfhip_internal.h"
#include "bfhip_build.h"
#include "bfhip_abi.h"

/* ---- allocation counting and failure injection ------------------------------------------------------------------ */
void *__real_malloc(size_t);
void *__real_calloc(size_t, size_t);
void *__real_realloc(void *, size_t);
static int armed;                       /* count (and fail) only inside the bfPlanBuild under test */
static long allocCount, failAt = -1;
static int failNow(void) { return armed && allocCount++ == failAt; }
void *__wrap_malloc(size_t n) { return failNow() ? NULL : __real_malloc(n); }
void *__wrap_calloc(size_t n, size_t m) { return failNow() ? NULL : __real_calloc(n, m); }
void *__wrap_realloc(void *p, size_t n) { return failNow() ? NULL : __real_realloc(p, n); }

/* ---- digest ------------------------------------------------------------------------------------------------------ */
static uint64_t fnv(uint64_t h, void const *p, size_t n) {
  unsigned char const *b = p;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
static uint64_t fnvU(uint64_t h, uint64_t v) { return fnv(h, &v, 8); }

static uint64_t planDigest(BfPlan const *p) {
  uint64_t h = 1469598103934665603ull;
  uint64_t const ps[] = { p->dtype, p->elemSize, p->epl, p->maxItemRows, p->xcap, p->numRows, p->numCols, p->numStages, p->arenaElems,
                          p->tempElems, p->numLeaves, p->leafElems, (uint64_t)p->transposed, p->numBufs, (uint64_t)p->flowOk };
  h = fnv(h, ps, sizeof ps);
  h = fnv(h, p->bufWriters, p->numBufs * 4);
  for (uint64_t s = 0; s < p->numStages; ++s) {
    BfStage const *st = &p->stages[s];
    uint64_t const ss[] = { st->numItems, st->numPieces, st->maxRows, st->firstSmall, st->numNarrow, st->maxRowsRest, st->padRest,
                            st->numCoopNarrow, st->numCoop, st->leafElems, st->vecIn, st->vecOut, st->numReduce, st->numBundles,
                            st->bundleBegin != NULL };
    h = fnv(h, ss, sizeof ss);
    h = fnv(h, st->items, st->numItems * sizeof(BfDevItem));           /* (neither record has padding) */
    h = fnv(h, st->pieces, st->numPieces * sizeof(BfDevPiece));
    h = fnv(h, st->pieceSrc, st->numPieces * sizeof(BfPieceSrc));
    h = fnv(h, st->pieceBuf, st->numPieces * 4);
    h = fnv(h, st->itemBuf, st->numItems * 4);
    if (st->bundleBegin) h = fnv(h, st->bundleBegin, (st->numBundles + 1) * 4);
    for (uint64_t r = 0; r < st->numReduce; ++r) {
      BfReduce const *rd = &st->reduce[r];
      uint64_t const rs[] = { rd->destSpace, rd->destOff, rd->numRows, rd->numIntervals, rd->numSrc, rd->maxSrc };
      h = fnv(h, rs, sizeof rs);
      h = fnv(h, rd->rowInterval, rd->numRows * 4);
      h = fnv(h, rd->ivBegin, (rd->numIntervals + 1) * 4);
      h = fnv(h, rd->srcBias, rd->numSrc * 8);
    }
    h = fnvU(h, s);
  }
  return h;
}

static void printFlags(char const *name, BfPlan const *p) {
  uint64_t items = 0, rowMajor = 0, merged = 0, small = 0, narrow = 0, zero = 0, reduces = 0, skipRows = 0, bundles = 0;
  for (uint64_t s = 0; s < p->numStages; ++s) {
    BfStage const *st = &p->stages[s];
    items += st->numItems; bundles += st->numBundles; reduces += st->numReduce;
    for (uint64_t i = 0; i < st->numItems; ++i) {
      uint32_t const f = st->items[i].mrFlags;
      rowMajor += (f & BF_ITEM_ROWMAJOR) != 0; merged += (f & BF_ITEM_MERGED) != 0; small += (f & BF_ITEM_SMALL) != 0;
      narrow += (f & BF_ITEM_TNARROW) != 0; zero += st->items[i].numPieces == 0;
    }
    for (uint64_t r = 0; r < st->numReduce; ++r)
      for (uint64_t i = 0; i < st->reduce[r].numRows; ++i) skipRows += st->reduce[r].rowInterval[i] == BF_REDUCE_SKIP;
  }
  printf("flags %s stages=%llu items=%llu rowmajor=%llu merged=%llu small=%llu narrow=%llu zerofill=%llu bundles=%llu reduces=%llu skiprows=%llu\n",
         name, (unsigned long long)p->numStages, (unsigned long long)items, (unsigned long long)rowMajor, (unsigned long long)merged,
         (unsigned long long)small, (unsigned long long)narrow, (unsigned long long)zero, (unsigned long long)bundles,
         (unsigned long long)reduces, (unsigned long long)skipRows);
}

/* ---- one build: digest, then the sweep ------------------------------------------------------------------------- */
static int checkBuild(char const *operand, char const *build, BfIr const *ir, BfPlanOptions const *po) {
  char name[96];
  snprintf(name, sizeof name, "%s/%s", operand, build);
  BfPlan plan, zero;
  memset(&zero, 0, sizeof zero);
  allocCount = 0; failAt = -1; armed = 1;
  int rc = bfPlanBuild(ir, po, &plan);
  armed = 0;
  long const count = allocCount;
  if (rc == BFABI_ERROR_MEMORY_ERROR) { fprintf(stderr, "%s: bfPlanBuild -> %d (%s)\n", name, rc, bfhipLastErrorMessage()); return 1; }
  if (rc) {
    /* a build the planner refuses is recorded as such, and the allocations it made before refusing are swept like any other's */
    printf("digest %s refused:%d\n", name, rc);
    if (memcmp(&plan, &zero, sizeof plan)) { fprintf(stderr, "%s: refused, but the BfPlan is not zeroed\n", name); return 1; }
  } else {
    printf("digest %s %016llx\n", name, (unsigned long long)planDigest(&plan));
    printFlags(name, &plan);
    bfPlanFree(&plan);
  }
  for (long k = 0; k < count; ++k) {
    memset(&plan, 0xa5, sizeof plan);
    allocCount = 0; failAt = k; armed = 1;
    rc = bfPlanBuild(ir, po, &plan);
    armed = 0;
    if (rc != BFABI_ERROR_MEMORY_ERROR) { fprintf(stderr, "%s: allocation %ld of %ld failing -> %d, not MEMORY_ERROR\n", name, k, count, rc); if (!rc) bfPlanFree(&plan); return 1; }
    if (memcmp(&plan, &zero, sizeof plan)) { fprintf(stderr, "%s: allocation %ld of %ld failing: the BfPlan is not zeroed\n", name, k, count); return 1; }
  }
  printf("sweep %s allocations=%ld\n", name, count);
  return 0;
}

/* the options bfhipCompileIrFill sets (bfhip_api.c) */
static BfPlanOptions compileOptions(uint32_t storeDtype, unsigned maxRhs) {
  BfPlanOptions po;
  memset(&po, 0, sizeof po);
  po.storeDtype = storeDtype;
  po.groupByInput = maxRhs >= 3;
  po.minChunkRows = maxRhs >= 3 ? 32 : 16;
  po.rowAlignBytes = 128;
  return po;
}

/* the shared-leaf adjoint plan over the forward plan of `po` (buildSharedTplan, bfhip_api.c) */
static int checkShared(char const *operand, char const *build, BfIr const *ir, BfPlanOptions const *po) {
  BfPlan fwdPlan;
  int rc = bfPlanBuild(ir, po, &fwdPlan);
  if (rc) { fprintf(stderr, "%s/%s: forward plan -> %d (%s)\n", operand, build, rc, bfhipLastErrorMessage()); return 1; }
  BfFwdPiece *fwd = NULL;
  uint64_t nf = 0;
  if ((rc = bfPlanFwdPieces(&fwdPlan, &fwd, &nf))) { bfPlanFree(&fwdPlan); return 1; }
  BfPlanOptions pt = *po;
  pt.itemsWanted = 0; pt.fwdPieces = fwd; pt.numFwdPieces = nf; pt.tCols = 0;
  rc = checkBuild(operand, build, ir, &pt);
  free(fwd);
  bfPlanFree(&fwdPlan);
  return rc;
}

static int checkOperand(char const *operand, BfhipDesc const *d, uint32_t storeDtype) {
  BfIr ir, irT;
  if (bfIrFromDesc(d, &ir)) { fprintf(stderr, "%s: bfIrFromDesc: %s\n", operand, bfhipLastErrorMessage()); return 1; }
  uint64_t const n = ir.rows[ir.root];
  BfPlanOptions const po1 = compileOptions(storeDtype, 1), po64 = compileOptions(storeDtype, 64);
  BfPlanOptions range = po1;
  range.rowBegin = n / 6 + 3; range.rowEnd = n * 2 / 3 + 100;      /* neither end on a leaf boundary */
  int rc = checkBuild(operand, "forward_rhs1", &ir, &po1);
  if (!rc) rc = checkBuild(operand, "forward_rhs64", &ir, &po64);
  if (!rc) rc = checkBuild(operand, "row_range", &ir, &range);
  if (!rc) rc = checkShared(operand, "shared_adjoint", &ir, &po1);
  if (!rc) rc = checkShared(operand, "shared_adjoint_row_range", &ir, &range);
  if (!rc && !bfDtypeC128Layout(storeDtype)) {
    /* Real element types: the planner refuses the shared adjoint of the range above ("transposed piece not on a lane boundary",
     * a runtime error: the trimmed leaf starts at an odd row).  That refusal is recorded; the same range started one row later,
     * on a multiple of every lane granule, gives the trimmed transposed plan a digest. */
    range.rowBegin = n / 6 + 4;
    rc = checkBuild(operand, "row_range_lane", &ir, &range);
    if (!rc) rc = checkShared(operand, "shared_adjoint_row_range_lane", &ir, &range);
  }
  if (!rc) {
    /* the packed adjoint: a forward plan of the transposed expression (bfhipCompileIrFill) */
    if (bfIrTransposed(&ir, &irT)) { bfIrFree(&ir); return 1; }
    BfPlanOptions pt = po1;
    if (!bfDtypeC128Layout(storeDtype)) pt.itemsWanted = 32768;
    rc = checkBuild(operand, "packed_adjoint", &irT, &pt);
    bfIrFree(&irT);
  }
  bfIrFree(&ir);
  return rc;
}

int main(void) {
  int rc = 0;
  {
    /* the helm2 layout of tests/native/asan_host.c: 6000 points on an ellipse, k = 150, complex128 */
    enum { N = 6000 };
    double *pts = malloc(N * 16);
    for (int i = 0; i < N; ++i) { double const t = 2 * M_PI * i / N; pts[2 * i] = cos(t); pts[2 * i + 1] = 0.4 * sin(t); }
    BfhipHelm2Layout *lay = NULL;
    if (bfhipHelm2LayoutCreate2(pts, N, NULL, 0, 150.0, &lay)) { fprintf(stderr, "helm2 layout: %s\n", bfhipLastErrorMessage()); return 1; }
    rc = checkOperand("helm2_c128", bfhipHelm2LayoutGetDesc(lay), BFHIP_C128);
    bfhipHelm2LayoutFree(&lay);
    free(pts);
  }
  if (!rc) {
    /* its streamer layout: 3000 points on the Fibonacci sphere, eight bands, maxCols 300; stored as F64 and as F32 */
    enum { N = 3000 };
    double *pts = malloc(3 * N * sizeof *pts);
    for (int i = 0; i < N; ++i) {
      double const x = 1 - 2.0 * (i + 0.5) / N, r = sqrt(1 - x * x), th = 3.141592653589793 * (sqrt(5.0) - 1) * i;
      pts[3 * i] = x; pts[3 * i + 1] = r * cos(th); pts[3 * i + 2] = r * sin(th);
    }
    uint64_t bands[8] = {30, 64, 90, 110, 12, 140, 160, 182};
    BfhipStreamerSpec spec;
    memset(&spec, 0, sizeof spec);
    spec.structSize = sizeof spec; spec.colDepth = 3; spec.wmax = 28.0; spec.bandColumns = bands; spec.maxCols = 300;
    BfhipStreamerLayout *lay = NULL;
    if (bfhipStreamerLayoutCreate(pts, N, &spec, &lay)) { fprintf(stderr, "streamer layout: %s\n", bfhipLastErrorMessage()); return 1; }
    rc = checkOperand("streamer_f64", bfhipStreamerLayoutGetDesc(lay), BFHIP_F64);
    if (!rc) rc = checkOperand("streamer_f32", bfhipStreamerLayoutGetDesc(lay), BFHIP_F32);
    bfhipStreamerLayoutFree(&lay);
    free(pts);
  }
  printf(rc ? "FAILED\n" : "planner clean\n");
  return rc;
}
