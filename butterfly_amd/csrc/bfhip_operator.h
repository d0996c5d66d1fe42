/* bfhip_operator.h -- struct BfhipOperator and the few helpers shared by the files that implement it: bfhip_api.c
 * (lifetime, compile, apply), bfhip_file.c (save / load), bfhip_shim.c (BfMat vtable), bfhip_inspect.c (plan inspection),
 * bfhip_cov.c (batched covariance sampling) and bfhip_cond.c / bfhip_condlik.c (conditioning on observations; their object is bfhip_cond.h's).  Private to those seven: every other file reads an operator through the bfhipOperator* accessors of bfhip_internal.h.
 */
#ifndef BFHIP_OPERATOR_H
#define BFHIP_OPERATOR_H

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"

struct BfhipOperator {
  BfPlan plan;
  BfPlan tplan;               /* plan of A^T over the same leaf arena (BFHIP_FLAG_ADJOINT) */
  int hasTplan;
  uint32_t srcDtype;          /* dtype of the operand as given (C128 / F64) */
  int device;
  uint32_t flags;
  void *dArena;               /* leaf data */
  void *dArenaT;              /* BFHIP_FLAG_ADJOINT_PACKED: the leaves of A^T packed for tplan, a FORWARD plan of the transposed expression */
  void *dTemp;                /* vector arena: intermediates + partial slots, tempElems * maxRhs */
  void *dZero;                /* 4 KiB of zeros */
  uint32_t tempRhs;
  uint64_t metaBytes;
  uint64_t leafBytesAlgorithmic;
  /* staging for the host-pointer apply */
  void *dX, *dY;
  void *hX, *hY;              /* pinned host mirrors of dX / dY */
  void *evHost[4];            /* "piece i of the result is in hY" (created on first use) */
  uint32_t xyRhs;
  /* profiling */
  void **evStart, **evStop;   /* [BF_EV_POOL][numStages]: one set per apply in flight, so timing an apply never waits for the one before */
  double *stageMs;
  uint64_t *stageLaunches;
  uint32_t lastNrhs;
  uint64_t evIssued, evHarvested;   /* applies whose events were recorded / read back */
  uint64_t applyCount;              /* forward applies so far */
  void *dCov;                       /* scratch of the covariance products (2 blocks of the longer side x covRhs columns) */
  uint32_t covRhs;                  /* columns dCov holds (0: none yet; the single-vector entries ask for 1, the block entries grow it) */
  uint32_t profEvery;               /* events around one apply in profEvery (0, 1: every apply) */
  /* BFHIP_FLAG_PLAN_ONLY: the IR is kept (borrowed leaf pointers!) for bfhipPlanPackArena; irT: its transposed view when the
   * adjoint plan has an arena of its own (BFHIP_FLAG_ADJOINT_PACKED), for bfhipPlanPackArenaT */
  BfIr *ir, *irT;
  int packedT;
  uint64_t seed;
  /* dependency-driven launch of the forward plan (complex128, one right-hand side): flat copies of the index tables */
  int flow;
  void *dFlowItems, *dFlowPieces, *dFlowItemOut, *dFlowWriters, *dFlowCounters;
  uint32_t flowNumItems, flowGrid, flowEpoch, flowQueueBase, flowMaxWriters;
  uint64_t flowNumBufs;
  uint8_t evFlow[64];               /* per event set: that apply ran as ONE launch (its time is recorded under stage 0) */
  uint32_t rhsBlocks;               /* bfhipSetRhsBlocks / bfhipSetRealRhsBlocks: 0 = off, else the smallest nrhs whose forward stages run the element type's block kernels */
  uint32_t adjointRhsBlocks;        /* bfhipSetAdjointRhsBlocks: the same for the stages of the adjoint plan (shared-leaf: bfStageKernelTMfma; packed: the forward block kernels); independent of rhsBlocks */
  uint64_t hostApplyBudget;         /* device bytes the host-vector apply may use for vectors; 0 = free memory - BF_HOST_BUDGET_MARGIN */
  void *extract;                    /* workspace of the dense extraction (bfhip_extract.c), released by extractRelease */
  void (*extractRelease)(void *);
};

/* The scratch convention of the covariance products, in one place: op->dCov (covScratch) is two blocks of the longer side, and a
 * block of `nrhs` columns packs both at nrhs columns -- t0 = the permuted / scaled input, t1 = where the apply's result starts. */
static inline void bfCovHalves(BfhipOperator const *op, size_t nrhs, char **t0, char **t1) {
  uint64_t const big = op->plan.numRows > op->plan.numCols ? op->plan.numRows : op->plan.numCols;
  *t0 = (char *)op->dCov;
  *t1 = (char *)op->dCov + big * nrhs * op->plan.elemSize;
}

/* what every covariance entry refuses about its operator, in this order: element type, (adjoint,) device */
static inline int bfCovCheckOperator(BfhipOperator const *op, int needAdjoint) {
  if (bfDtypeComplex(op->plan.dtype)) return bfhipFail(BFABI_ERROR_TYPE_ERROR, "covariance products are defined for real operators (not complex128 / complex64)");
  if (needAdjoint && !op->hasTplan) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "operator was not compiled with BFHIP_FLAG_ADJOINT");
  if (op->flags & BFHIP_FLAG_PLAN_ONLY) return bfhipFail(BFABI_ERROR_RUNTIME_ERROR, "operator was compiled with BFHIP_FLAG_PLAN_ONLY: no device operator exists");
  return 0;
}

#define BF_ARENA_SLACK 256u
#define BF_HOST_PIECE_ROWS 8192u    /* host vectors of more than 4 x this many rows cross PCIe in 4 pieces, copy and DMA overlapped */
#define BF_EV_POOL 64u
#define BF_HOST_BUDGET_MARGIN (512ull << 20)   /* automatic host-apply budget: what the device has free, less this */

/* defined in bfhip_api.c; not exported from the library */
#define BF_HIDDEN __attribute__((visibility("hidden")))
BF_HIDDEN int packLeavesPlan(BfPlan const *pl, void *dArena, BfIr const *ir, uint64_t seed, void *hostDst);
BF_HIDDEN int finishOperator(BfhipOperator *op, uint32_t maxRhs);
BF_HIDDEN void stageLaunchArgs(BfhipOperator const *op, BfPlan const *plan, BfStage const *st, uint32_t nrhs, BfLaunchArgs *a);
/* the covariance entries' scratch holds at least `nrhs` columns after this (bfhip_api.c; the batched entries of bfhip_cov.c share it) */
BF_HIDDEN int covScratch(BfhipOperator *op, size_t nrhs, void *stream);
BF_HIDDEN int applyHost(BfhipOperator *op, int transpose, void const *X, size_t ldx, size_t nrhs, void *Y, size_t ldy);
/* z = P A (GammaLam w) on a block (bfhip_cov.c); `scaled`: the input is already in the scratch's first half, scaled.  With scaled = 0, dW may
 * BE the scratch's first half (it is scaled in place): the conditioned entries of bfhip_cond.c start from there */
BF_HIDDEN int covSampleBlock(BfhipOperator *op, void const *dGammaLam, uint64_t const *dRowPerm, void const *dW, int scaled, size_t nrhs, void *dZ, void *stream);

/* ---- conditioning on observations: the device entry points of bfhip_cond.c, defined in bfhip_cond.hip ---- */
#define BF_COND_CHUNK 1024u          /* rows of Bt per partial sum of the two contractions over n */
#define BF_COND_MAX_RHS 64u          /* columns a pass */
/* numCols the per-pass kernels take: one grid z per chunk of the first contraction (<= 65535; the second's 2^31 - 1 tiles of 32 rows is the wider limit) */
#define BF_COND_MAX_COLS (65535ull * BF_COND_CHUNK)
static inline int bfdevCondFits(uint64_t numCols) { return numCols <= BF_COND_MAX_COLS; }
typedef struct { uint32_t failStep, pad; double minPivot, maxPivot; } BfCondStat;   /* failStep 0xffffffff: none */
#ifdef __cplusplus
extern "C" {
#endif
int bfdevCondInvertPerm(uint64_t const *dPerm, uint64_t m, uint64_t const *dObsSorted, uint32_t const *dObsSlot, uint32_t k, uint64_t *dRows, uint32_t *dFlag, void *stream);
int bfdevCondUnitPanel(void *V, uint64_t m, uint32_t p, uint64_t const *dRows, uint32_t dtype, void *stream);
int bfdevCondPack(double *Bt, uint64_t n, uint32_t k, uint32_t c0, void const *T, uint32_t p, void const *gamma, uint32_t dtype, void *stream);
int bfdevCondGram(double *G, double const *Bt, uint64_t n, uint32_t k, double const *dNoiseVar, void *stream);
int bfdevCondCholesky(double *G, uint32_t k, BfCondStat *dStat, void *stream);
int bfdevCondResidual(double *R, double *part, double const *Bt, uint64_t n, uint32_t k, double const *dY, void const *W, uint64_t ldw, uint32_t dtype,
                      double const *E, uint64_t lde, uint32_t b, void *stream);
int bfdevCondSolve(double const *L, uint32_t k, double *R, uint32_t b, void *stream);
int bfdevCondDeviceSync(void);       /* drains every stream of the current device */
int bfdevCondUpdate(void *Wout, double const *Bt, uint64_t n, uint32_t k, double const *alpha, void const *W, uint64_t ldw, uint32_t dtype, uint32_t b, void *stream);
#ifdef __cplusplus
}
#endif

#endif
