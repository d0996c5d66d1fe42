/* bfhip_inspect.c -- what a compiled operator reports about itself: statistics, the plan views of BFHIP_FLAG_PLAN_ONLY
 * operators (stages, reduces, packed arenas) and the stage kernels a launch would run, by id and by name.
 */
#include "bfhip_operator.h"
#include "../../include/bfhip_abi.h"

#include <stddef.h>

int bfhipGetStats(BfhipOperator const *op, BfhipStats *st) {
  if (!op || !st || st->structSize < sizeof(BfhipStats)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "bad stats struct");
  BfPlan const *pl = &op->plan;
  st->dtype = pl->dtype;
  st->numRows = pl->numRows; st->numCols = pl->numCols; st->numStages = pl->numStages;
  st->numLeaves = pl->numLeaves;
  st->numItems = 0; st->numPieces = 0; st->vecElemsRead = 0; st->vecElemsWritten = 0;
  for (uint64_t s = 0; s < pl->numStages; ++s) {
    st->numItems += pl->stages[s].numItems;
    st->numPieces += pl->stages[s].numPieces;
    st->vecElemsRead += pl->stages[s].vecIn;
    st->vecElemsWritten += pl->stages[s].vecOut;
  }
  st->leafElems = pl->leafElems;
  st->leafBytes = pl->leafElems * pl->elemSize;
  st->arenaBytes = pl->arenaElems * pl->elemSize + (op->dArenaT ? op->tplan.arenaElems * op->tplan.elemSize : 0);      /* both packed copies with BFHIP_FLAG_ADJOINT_PACKED */
  st->tempElems = pl->tempElems;
  st->metaBytes = op->metaBytes;
  return 0;
}

/* ---- plan inspection (BFHIP_FLAG_PLAN_ONLY) --------------------------------- */
static int needPlanOnly(BfhipOperator const *op) {
  if (!op) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL operator");
  if (!(op->flags & BFHIP_FLAG_PLAN_ONLY)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "plan inspection needs BFHIP_FLAG_PLAN_ONLY");
  return 0;
}
int bfhipPlanGetInfo(BfhipOperator const *op, BfhipPlanInfo *info) {
  int rc = needPlanOnly(op);
  if (rc) return rc;
  if (!info || info->structSize < sizeof *info) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "bad info struct");
  BfPlan const *pl = &op->plan;
  info->dtype = pl->dtype; info->elemSize = pl->elemSize; info->epl = pl->epl; info->xcap = pl->xcap;
  info->numRows = pl->numRows; info->numCols = pl->numCols; info->numStages = pl->numStages;
  info->arenaElems = pl->arenaElems; info->tempElems = pl->tempElems;
  info->numStagesT = op->hasTplan ? op->tplan.numStages : 0;
  info->tempElemsT = op->hasTplan ? op->tplan.tempElems : 0;
  info->reserved = op->packedT ? 1u : 0u;                     /* 1: the adjoint plan is a forward plan over its own arena ... */
  info->arenaElemsT = op->packedT ? op->tplan.arenaElems : 0;      /* ... of this many elements */
  return 0;
}
int bfhipPlanGetStage(BfhipOperator const *op, uint64_t stage, BfhipStageView *v) {
  int rc = needPlanOnly(op);
  if (rc) return rc;
  BfPlan const *pl = &op->plan;
  if (stage >= pl->numStages && op->hasTplan) { stage -= pl->numStages; pl = &op->tplan; }
  if (!v || v->structSize < offsetof(BfhipStageView, numBundles) || stage >= pl->numStages) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "bad stage view request");
  BfStage const *st = &pl->stages[stage];
  v->numItems = st->numItems; v->numPieces = st->numPieces; v->numReduce = st->numReduce;
  v->items = st->items; v->pieces = st->pieces;
  if (v->structSize >= sizeof *v) { v->numBundles = st->numBundles; v->bundleBegin = st->bundleBegin; }
  return 0;
}
/* indexed by BfhipKernelId: an id without an entry reads as NULL (tests/test_kernel_coverage_cpu.py walks every id) */
static char const *const kernelNames[] = {
  [BFHIP_KERNEL_C128] = "bfStageKernelC128",
  [BFHIP_KERNEL_C128_MFMA1] = "bfStageKernelC128Mfma1",
  [BFHIP_KERNEL_C128_MFMA2] = "bfStageKernelC128Mfma2",
  [BFHIP_KERNEL_C128_MFMA4] = "bfStageKernelC128Mfma",
  [BFHIP_KERNEL_C128_MFMA1_EXACT] = "bfStageKernelC128Mfma1Exact",
  [BFHIP_KERNEL_C128_MFMA2_EXACT] = "bfStageKernelC128Mfma2Exact",
  [BFHIP_KERNEL_C128_MFMA4_EXACT] = "bfStageKernelC128MfmaExact",
  [BFHIP_KERNEL_REAL_F64] = "bfStageKernelReal<F64>",
  [BFHIP_KERNEL_REAL_F32] = "bfStageKernelReal<F32>",
  [BFHIP_KERNEL_REAL_C64] = "bfStageKernelReal<C64>",
  [BFHIP_KERNEL_REALBOTH_F64] = "bfStageKernelRealBoth<F64>",
  [BFHIP_KERNEL_REALBOTH_F32] = "bfStageKernelRealBoth<F32>",
  [BFHIP_KERNEL_REALBOTH_C64] = "bfStageKernelRealBoth<C64>",
  [BFHIP_KERNEL_SMALL_F64] = "bfStageKernelSmall<F64>",
  [BFHIP_KERNEL_SMALL_F32] = "bfStageKernelSmall<F32>",
  [BFHIP_KERNEL_SMALL_C64] = "bfStageKernelSmall<C64>",
#define BF_T_NAMES(ID, DT) \
  [ID##_NARROW_N] = "bfStageKernelT<" DT ", narrow, nrhs>1>", [ID##_NARROW_ONE] = "bfStageKernelT<" DT ", narrow, nrhs=1>", \
  [ID##_NARROW_COOP_N] = "bfStageKernelT<" DT ", narrow, coop, nrhs>1>", [ID##_NARROW_COOP_ONE] = "bfStageKernelT<" DT ", narrow, coop, nrhs=1>", \
  [ID##_WIDE_N] = "bfStageKernelT<" DT ", wide, nrhs>1>", [ID##_WIDE_ONE] = "bfStageKernelT<" DT ", wide, nrhs=1>", \
  [ID##_WIDE_COOP_N] = "bfStageKernelT<" DT ", wide, coop, nrhs>1>", [ID##_WIDE_COOP_ONE] = "bfStageKernelT<" DT ", wide, coop, nrhs=1>"
  BF_T_NAMES(BFHIP_KERNEL_T_C128, "C128"), BF_T_NAMES(BFHIP_KERNEL_T_F64, "F64"),
  BF_T_NAMES(BFHIP_KERNEL_T_F32, "F32"), BF_T_NAMES(BFHIP_KERNEL_T_C64, "C64"),
#undef BF_T_NAMES
  [BFHIP_KERNEL_TBOTH_F64_N] = "bfStageKernelTBoth<F64, nrhs>1>",
  [BFHIP_KERNEL_TBOTH_F64_ONE] = "bfStageKernelTBoth<F64, nrhs=1>",
  [BFHIP_KERNEL_TBOTH_F32_N] = "bfStageKernelTBoth<F32, nrhs>1>",
  [BFHIP_KERNEL_TBOTH_F32_ONE] = "bfStageKernelTBoth<F32, nrhs=1>",
  [BFHIP_KERNEL_TBOTH_C64_N] = "bfStageKernelTBoth<C64, nrhs>1>",
  [BFHIP_KERNEL_TBOTH_C64_ONE] = "bfStageKernelTBoth<C64, nrhs=1>",
  [BFHIP_KERNEL_REDUCE_C128] = "bfReduceKernel<C128>",
  [BFHIP_KERNEL_REDUCE_F64] = "bfReduceKernel<F64>",
  [BFHIP_KERNEL_REDUCE_F64_LONG] = "bfReduceKernel<F64, long>",
  [BFHIP_KERNEL_REDUCE_F32] = "bfReduceKernel<F32>",
  [BFHIP_KERNEL_REDUCE_F32_LONG] = "bfReduceKernel<F32, long>",
  [BFHIP_KERNEL_REDUCE_C64] = "bfReduceKernel<C64>",
  [BFHIP_KERNEL_REDUCE_C64_LONG] = "bfReduceKernel<C64, long>",
};
static char const *const kernelNamesExt[] = {
  [BFHIP_KERNEL_C64_MFMA1 - BFHIP_KERNEL_EXT_BASE] = "bfStageKernelC64Mfma<1 tile>",
  [BFHIP_KERNEL_C64_MFMA2 - BFHIP_KERNEL_EXT_BASE] = "bfStageKernelC64Mfma<2 tiles>",
  [BFHIP_KERNEL_C64_MFMA4 - BFHIP_KERNEL_EXT_BASE] = "bfStageKernelC64Mfma<4 tiles>",
};
static char const *const kernelNamesRealExt[] = {
  [BFHIP_KERNEL_F64_MFMA1 - BFHIP_KERNEL_REAL_EXT_BASE] = "bfStageKernelRealMfma<F64, 1 tile>",
  [BFHIP_KERNEL_F64_MFMA2 - BFHIP_KERNEL_REAL_EXT_BASE] = "bfStageKernelRealMfma<F64, 2 tiles>",
  [BFHIP_KERNEL_F64_MFMA4 - BFHIP_KERNEL_REAL_EXT_BASE] = "bfStageKernelRealMfma<F64, 4 tiles>",
  [BFHIP_KERNEL_F32_MFMA1 - BFHIP_KERNEL_REAL_EXT_BASE] = "bfStageKernelRealMfma<F32, 1 tile>",
  [BFHIP_KERNEL_F32_MFMA2 - BFHIP_KERNEL_REAL_EXT_BASE] = "bfStageKernelRealMfma<F32, 2 tiles>",
  [BFHIP_KERNEL_F32_MFMA4 - BFHIP_KERNEL_REAL_EXT_BASE] = "bfStageKernelRealMfma<F32, 4 tiles>",
};
static char const *const kernelNamesTExt[] = {
#define BF_TM_NAMES(ID, DT) \
  [ID##_MFMA1 - BFHIP_KERNEL_T_EXT_BASE] = "bfStageKernelTMfma<" DT ", 1 tile>", [ID##_MFMA2 - BFHIP_KERNEL_T_EXT_BASE] = "bfStageKernelTMfma<" DT ", 2 tiles>", \
  [ID##_MFMA4 - BFHIP_KERNEL_T_EXT_BASE] = "bfStageKernelTMfma<" DT ", 4 tiles>"
  BF_TM_NAMES(BFHIP_KERNEL_T_C128, "C128"), BF_TM_NAMES(BFHIP_KERNEL_T_F64, "F64"), BF_TM_NAMES(BFHIP_KERNEL_T_F32, "F32"), BF_TM_NAMES(BFHIP_KERNEL_T_C64, "C64"),
#undef BF_TM_NAMES
};
_Static_assert(sizeof kernelNamesTExt / sizeof kernelNamesTExt[0] == BFHIP_KERNEL_T_EXT_END - BFHIP_KERNEL_T_EXT_BASE, "kernelNamesTExt: one entry per id of the third extension range");
_Static_assert(sizeof kernelNamesRealExt / sizeof kernelNamesRealExt[0] == BFHIP_KERNEL_REAL_EXT_END - BFHIP_KERNEL_REAL_EXT_BASE, "kernelNamesRealExt: one entry per id of the second extension range");
_Static_assert(sizeof kernelNames / sizeof kernelNames[0] == BFHIP_KERNEL_COUNT, "kernelNames: one entry per BfhipKernelId");
_Static_assert(sizeof kernelNamesExt / sizeof kernelNamesExt[0] == BFHIP_KERNEL_EXT_END - BFHIP_KERNEL_EXT_BASE, "kernelNamesExt: one entry per id of the extension range");
char const *bfhipKernelName(uint32_t id) {
  if (id >= BFHIP_KERNEL_EXT_BASE && id < BFHIP_KERNEL_EXT_END) return kernelNamesExt[id - BFHIP_KERNEL_EXT_BASE];
  if (id >= BFHIP_KERNEL_REAL_EXT_BASE && id < BFHIP_KERNEL_REAL_EXT_END) return kernelNamesRealExt[id - BFHIP_KERNEL_REAL_EXT_BASE];
  if (id >= BFHIP_KERNEL_T_EXT_BASE && id < BFHIP_KERNEL_T_EXT_END) return kernelNamesTExt[id - BFHIP_KERNEL_T_EXT_BASE];
  return id < BFHIP_KERNEL_COUNT ? kernelNames[id] : NULL;
}

int bfhipPlanStageKernels(BfhipOperator const *op, uint64_t stage, uint32_t nrhs, uint32_t *ids, uint32_t cap, uint32_t *count) {
  if (!op || !count || (cap && !ids) || !nrhs) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "bad stage kernel request");
  BfPlan const *pl = &op->plan;
  if (stage >= pl->numStages && op->hasTplan) { stage -= pl->numStages; pl = &op->tplan; }
  if (stage >= pl->numStages) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "bad stage kernel request");
  BfStage const *st = &pl->stages[stage];
  BfLaunchArgs a;
  stageLaunchArgs(op, pl, st, nrhs, &a);
  BfKernelLaunch L[2];
  uint32_t const nl = bfSelectStageKernels(&a, L);
  uint32_t n = 0;
  for (uint32_t i = 0; i < nl; ++i, ++n) if (n < cap) ids[n] = L[i].kernel;
  /* the reduce launches of runPlan: groups of 16, each split by bfdevLaunchReduce into batches of BF_REDUCE_BATCH; a batch
   * of no rows launches nothing */
  for (uint64_t r0 = 0; r0 < st->numReduce; r0 += 16) {
    uint64_t const cnt = st->numReduce - r0 < 16 ? st->numReduce - r0 : 16;
    for (uint64_t base = 0; base < cnt; base += BF_REDUCE_BATCH) {
      uint64_t const bc = cnt - base < BF_REDUCE_BATCH ? cnt - base : BF_REDUCE_BATCH;
      int longLists = 0, rows = 0;
      for (uint64_t k = 0; k < bc; ++k) {
        BfReduce const *rd = &st->reduce[r0 + base + k];
        longLists = longLists || rd->maxSrc >= 64;
        rows = rows || rd->numRows;
      }
      if (!rows) continue;
      if (n < cap) ids[n] = bfSelectReduceKernel(pl->dtype, longLists);
      ++n;
    }
  }
  *count = n;
  return 0;
}
int bfhipPlanGetReduce(BfhipOperator const *op, uint64_t stage, uint64_t index, BfhipReduceView *v) {
  int rc = needPlanOnly(op);
  if (rc) return rc;
  BfPlan const *pl = &op->plan;
  if (stage >= pl->numStages && op->hasTplan) { stage -= pl->numStages; pl = &op->tplan; }
  if (!v || v->structSize < sizeof *v || stage >= pl->numStages || index >= pl->stages[stage].numReduce)
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "bad reduce view request");
  BfReduce const *rd = &pl->stages[stage].reduce[index];
  v->destIsY = rd->destSpace == BF_SPACE_Y; v->destOff = rd->destOff; v->numRows = rd->numRows;
  v->numIntervals = rd->numIntervals; v->numSrc = rd->numSrc;
  v->rowInterval = rd->rowInterval; v->ivBegin = rd->ivBegin; v->srcBias = rd->srcBias;
  return 0;
}
int bfhipPlanPackArena(BfhipOperator const *op, void *dst) {
  int rc = needPlanOnly(op);
  if (rc) return rc;
  if (!dst) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL destination");
  return packLeavesPlan(&op->plan, op->dArena, op->ir, op->seed, dst);
}
/* the second arena of a BFHIP_FLAG_ADJOINT_PACKED plan (arenaElemsT elements): the leaves of the transposed expression */
int bfhipPlanPackArenaT(BfhipOperator const *op, void *dst) {
  int rc = needPlanOnly(op);
  if (rc) return rc;
  if (!dst) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "NULL destination");
  if (!op->packedT || !op->irT) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "operator was not compiled with BFHIP_FLAG_ADJOINT_PACKED");
  return packLeavesPlan(&op->tplan, NULL, op->irT, op->seed, dst);
}
