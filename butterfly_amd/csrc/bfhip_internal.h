/* bfhip_internal.h -- shared between the C host (ir / plan / api) and the HIP
 * device layer (bfhip_device.hip).  The host side is plain C11; it reaches HIP
 * only through the `bfdev*` functions declared at the bottom (the "thin
 * C-ABI" between host C and device code). */
#ifndef BFHIP_INTERNAL_H
#define BFHIP_INTERNAL_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <time.h>
#include "../../include/bfhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a function the C host and a kernel both call (bfJacobiTile) */
#ifdef __HIPCC__
#define BF_HOST_DEVICE __host__ __device__
#else
#define BF_HOST_DEVICE
#endif

/* ------------------------------------------------------------------------
 * error plumbing
 * ---------------------------------------------------------------------- */
int bfhipFail(int code, char const *fmt, ...);   /* records message, returns code */
static inline double bfNowSeconds(void) {       /* monotonic wall clock, for the phase timings the info structs report */
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* element types: complex (C128, C64) vs real; the complex128 layout (one element per 16-byte lane load, its own kernels and
 * plan shapes) vs the real family's (C64 is 8 bytes like F64 and gets exactly the F64 plan) */
static inline int bfDtypeComplex(uint32_t dt) { return dt == BFHIP_C128 || dt == BFHIP_C64; }
static inline int bfDtypeC128Layout(uint32_t dt) { return dt == BFHIP_C128; }
static inline uint32_t bfDtypeElemSize(uint32_t dt) { return dt == BFHIP_C128 ? 16u : (dt == BFHIP_F64 || dt == BFHIP_C64) ? 8u : 4u; }

/* ------------------------------------------------------------------------
 * IR: owned copy of a BfhipDesc (or of a walked BfMat graph)
 * ---------------------------------------------------------------------- */
#define BF_REDUCE_SKIP 0xffffffffu
#define BF_LEAF_REAL 1u
#define BF_LEAF_CONJ 2u
typedef struct BfIr {
  uint32_t dtype;
  uint64_t numNodes, numChildren, root;
  uint8_t *kind;
  uint64_t *rows, *cols;
  uint64_t *childBegin;        /* numNodes+1 */
  uint64_t *childNode, *childRow0, *childCol0;
  void const **leafData;       /* borrowed host pointers (valid during compile only) */
  uint64_t *leafRowStride;
  uint64_t *leafColStride;     /* element stride between columns (BfMat graphs may have colStride != 1) */
  uint8_t *leafReal;           /* bit 0 (BF_LEAF_REAL): host values of this leaf are real doubles even in a complex operand (BfMatDiagReal
                                * terms); bit 1 (BF_LEAF_CONJ): the leaf is the CONJUGATE of the host values it points at (a dense complex
                                * leaf the reference flagged TRANS | CONJ: its strides are swapped as well) */
  uint64_t *synthBase;         /* per node: base index in the synthetic stream */
  int transposedView;          /* this IR is the transpose of the one the operator was compiled from (bfIrTransposed): synthetic leaf
                                * values are stream(base + col * rows + row), i.e. the ORIGINAL leaf's row-major index */
  uint64_t *topRowBlock;       /* per child of root, or NULL */
  uint32_t *depth;             /* stages needed by the subtree */
  /* sparse decorations folded into host-valued dense leaves: value added to leaf element (row, col) when the
   * arena is packed (sorted by leaf, row, col once finalized) */
  struct BfIrPatch *patches;
  uint64_t numPatches, capPatches;
  /* growable capacity (walker) */
  uint64_t capNodes, capChildren;
} BfIr;

typedef struct BfIrPatch { uint64_t leaf; uint32_t row, col; double re, im; } BfIrPatch;
void bfIrFree(BfIr *ir);
int bfIrFromDesc(BfhipDesc const *desc, BfIr *ir);
int bfIrFromBfMat(void const *bfMat, BfIr *ir);
int bfIrFinalize(BfIr *ir);   /* validation, depth, synthetic bases */
int bfIrTransposed(BfIr const *src, BfIr *dst);   /* dst = the expression of src^T over the same (borrowed) leaf values; src finalized */

/* ------------------------------------------------------------------------
 * Plan: the flattened per-stage layout (host mirror of what lives in HBM)
 * ---------------------------------------------------------------------- */

/* Where a vector segment lives.  All intermediates and partial-result slots
 * are sub-ranges of one device "vector arena" (element offsets, per RHS);
 * X and Y are the caller's buffers. */
enum { BF_SPACE_TEMP = 0, BF_SPACE_X = 1, BF_SPACE_Y = 2 };

/* device records (layouts shared with the kernels) */
typedef struct BfDevItem {
  uint32_t pieceBegin;
  uint32_t numPieces;
  uint32_t outOff;     /* element offset of row 0 of this item in its output space */
  uint32_t mrFlags;    /* bits 0..15: rows; bit 16: output space is Y (else vector arena) */
} BfDevItem;

typedef struct BfDevPiece {
  uint64_t dataOff;    /* element offset into the leaf arena (column-major mr_pad x ncols) */
  uint32_t inOff;      /* element offset of column 0 in the input space */
  uint32_t ncols;
  uint32_t flags;      /* bit 0: input space is X (else vector arena); bit 1: identity piece */
  uint32_t ld;         /* transposed plans: element stride between the lanes' columns (forward mrPad); row-major pieces: row stride; else 0 */
} BfDevPiece;

#define BF_ITEM_OUT_Y (1u << 16)
#define BF_COOP_BYTES (32u << 10)     /* transposed items at least this large are shared by the 4 wavefronts of a workgroup if they average BF_COOP_PIECES pieces */
#define BF_COOP_PIECES 8u
uint64_t bfPlanCountCoop(BfDevItem const *items, BfDevPiece const *pieces, uint64_t numItems, uint32_t elemSize);
#define BF_ITEM_TNARROW (1u << 20)    /* transposed plans: an item of <= 16 columns of a tall leaf (16-row-lane kernel); such items are the START of the list */
#define BF_ITEM_SMALL (1u << 19)      /* real, forward: <= 2 lane granules of rows, <= 16 pieces, <= BF_SMALL_COLS dense columns (one block);
                                        * small items are the END of a stage's item list and run four to a wavefront */
#define BF_SMALL_COLS 384u            /* (128 until round 4: the 8 KB row-major items of 130 - 380 columns of a streamed butterfly's stage 5 ran one per
                                        * wavefront at 5.56 TB/s; four to a wavefront 6.38) */
#define BF_SMALL_PIECES 16u
#define BF_ITEM_MERGED (1u << 18)     /* real, column-major: <= 64 pieces whose dense parts are ONE contiguous mrPad x n block, n <= BF_MERGE_COLS */
#define BF_MERGE_COLS 256u
#define BF_ITEM_ROWMAJOR (1u << 17)   /* all dense pieces of the item are stored row-major (few-row leaves of real operands) */
#define BF_PIECE_IN_X 1u
#define BF_PIECE_IDENTITY 2u
#define BF_PIECE_ROWMAJOR 4u          /* element (r, c) at dataOff + r * ld + c, ld = columns padded to the lane granule */

/* host-only: where each piece's values come from (for packing / synthesis) */
typedef struct BfPieceSrc {
  uint64_t node;       /* IR leaf */
  uint32_t row0, col0; /* sub-block origin inside the leaf */
} BfPieceSrc;

/* deterministic reduction of overlapping row groups (final accumulate into
 * Y, or any buffer several differently-shaped contributions land in) */
typedef struct BfReduce {
  uint32_t destSpace;       /* BF_SPACE_Y or BF_SPACE_TEMP */
  uint64_t destOff;         /* element offset in dest space */
  uint64_t numRows;
  uint64_t numIntervals;
  uint32_t *rowInterval;    /* [numRows] interval id of each row; BF_REDUCE_SKIP: the row is written directly by the one group that owns it */
  uint32_t *ivBegin;        /* [numIntervals+1] CSR into srcBias */
  int64_t *srcBias;         /* per source: (slot offset in arena) - (first row of the group) */
  uint64_t numSrc;
  uint32_t maxSrc;          /* longest source list of an interval (not stored in files: recomputed on load) */
  /* device copies */
  void *dRowInterval, *dIvBegin, *dSrcBias;
} BfReduce;

typedef struct BfStage {
  uint64_t numItems, numPieces;
  BfDevItem *items;
  BfDevPiece *pieces;
  BfPieceSrc *pieceSrc;
  uint32_t maxRows;          /* largest item row count */
  uint64_t firstSmall;       /* items [firstSmall, numItems) carry BF_ITEM_SMALL */
  uint64_t numNarrow;        /* transposed plans: items [0, numNarrow) carry BF_ITEM_TNARROW (<= 16 columns of A: their own launch) */
  uint32_t maxRowsRest, padRest;   /* largest item of the rest */
  uint64_t numCoopNarrow, numCoop;   /* the first items of either range that get a whole workgroup each (a scheduling hint) */
  uint64_t leafElems;        /* algorithmic: sum m*n over this stage's leaves */
  uint64_t vecIn, vecOut;    /* algorithmic vector elements read / written */
  uint64_t numReduce;
  BfReduce *reduce;
  /* dependency-driven launch (forward plans): which vector each piece reads / each item writes -- buffer ids of the
   * planner: 0 = x (pieces) or "nothing a later item waits for" (items: y, private slots), >= 2 an intermediate */
  uint32_t *pieceBuf;        /* [numPieces] */
  uint32_t *itemBuf;         /* [numItems] */
  /* forward complex128 plans: bundles of list neighbours that read the same input rows (bfPlanBundles): what bfhipPlanGetStage
   * reports of the list's X sharing; no kernel reads it.  bundleBegin[numBundles + 1]; host only, dropped with the other mirrors;
   * a loaded operator has none (numBundles = 0) */
  uint32_t *bundleBegin;
  uint64_t numBundles;
  /* device copies */
  void *dItems, *dPieces;
  /* persistent launches of a stage with more items than wavefront slots (bfStageKernelC128P): BF_TICKET_POOLS ticket
   * counters, zero between launches (the wavefront that draws a pool's last ticket of a launch puts it back to zero) */
  void *dTickets;
} BfStage;

typedef struct BfPlan {
  uint32_t dtype;            /* storage/compute type: BFHIP_C128 / F64 / F32 / C64 */
  uint32_t elemSize;         /* bytes per element */
  uint32_t epl;              /* elements per 16-byte lane load */
  uint32_t maxItemRows;      /* 64 * epl */
  uint32_t xcap;             /* max columns per piece (LDS staging capacity) */
  uint64_t numRows, numCols;
  uint64_t numStages;
  BfStage *stages;
  uint64_t arenaElems;       /* leaf arena size in elements */
  uint64_t tempElems;        /* vector arena elements per RHS */
  uint64_t numLeaves, leafElems;
  int transposed;            /* plan of A^T over the forward plan's arena */
  /* dependency-driven launch: number of vectors (buffer ids < numBufs), how many items write each, and whether the plan
   * qualifies (forward; every reduce pass sums into y, i.e. runs after all items) */
  uint64_t numBufs;
  uint32_t *bufWriters;      /* [numBufs] */
  int flowOk;
} BfPlan;

/* where the forward plan put each (leaf, row chunk, column range): the
 * transposed plan reads the same packed data with the roles of rows and
 * columns exchanged */
typedef struct BfFwdPiece {
  uint64_t node;
  uint64_t dataOff;
  uint32_t row0, mr, mrPad, col0, ncols;
  uint32_t rowMajor, ldr;      /* row-major forward piece and its row stride */
} BfFwdPiece;

typedef struct BfPlanOptions {
  uint32_t storeDtype;
  uint32_t itemRows;         /* rows per item cap (<= 64*epl); 0 -> default */
  uint32_t xcap;
  uint32_t groupByInput;     /* forward plans: order a stage's items by cost bucket, then by the input rows they read (RHS-block kernel: neighbours share an L2) */
  uint32_t itemsWanted;      /* a stage's groups are cut so that it has about this many items at least (0 -> 4096); never above 1 MiB per item */
  uint32_t minChunkRows;     /* lower bound of the adaptive item height, in 16-byte row units (0 -> 16): 32 keeps the RHS-block kernel's two-slab passes full */
  uint64_t rowBlockBegin, rowBlockEnd;
  uint64_t rowBegin, rowEnd;   /* row-range shard: keep what output rows [rowBegin, rowEnd) depend on; rowEnd == 0 -> all */
  /* transposed plan (A^T x): pieces are located in the forward plan's arena */
  BfFwdPiece const *fwdPieces;   /* sorted by (node, col0, row0); NULL -> forward plan */
  uint64_t numFwdPieces;
  uint32_t tCols;            /* transposed plan: columns of A per item, 16 (default) or 64 */
  uint32_t rowAlignBytes;    /* forward plan: start the rows of row-major pieces on this boundary (bfhipCompile: 128; 0 -> lane granule) */
} BfPlanOptions;

int bfPlanBuild(BfIr const *ir, BfPlanOptions const *po, BfPlan *plan);
#ifndef BF_BUNDLE_ITEMS
#define BF_BUNDLE_ITEMS 4u      /* list neighbours of a bundle (A/B builds: 1 = no bundles) */
#endif
#define BF_BUNDLE_MIXED 0x80000000u   /* bundleBegin[] bit: four unrelated items, not one shared X panel */
int bfPlanBundles(BfDevItem const *items, BfDevPiece const *pieces, uint64_t numItems, uint32_t **out, uint64_t *numBundles);
/* balanced contiguous row ranges for `world` ranks: cuts[world + 1], loads[world] (leaf elements each range keeps) or NULL */
int bfPlanRowPartition(BfIr const *ir, uint32_t world, uint64_t *cuts, uint64_t *loads);
/* table of the forward plan's pieces (needs its host mirrors); caller frees */
int bfPlanFwdPieces(BfPlan const *plan, BfFwdPiece **out, uint64_t *count);
void bfPlanFree(BfPlan *plan);

/* compile step with a caller-supplied arena fill (bfhip_build.c): `fill` runs
 * with the operator's device current, the plan's host mirrors still present
 * and the arena allocated; it must write every non-identity piece.  Consumes
 * `ir` like the plain compile. */
typedef int (*BfFillFn)(BfPlan const *plan, BfIr const *ir, void *dArena, void *ctx);
struct BfhipOptions;
struct BfhipOperator;
int bfhipCompileIrFill(BfIr *ir, struct BfhipOptions const *opts, BfFillFn fill, void *fillCtx, struct BfhipOperator **out);
/* HIP ordinal the operator lives on; -1 for a plan-only operator */
int bfhipOperatorDevice(struct BfhipOperator const *op);
/* vector arena for `nrhs` right-hand sides allocated now, so that applies of up to that many cannot fail on it */
int bfhipOperatorReserveRhs(struct BfhipOperator *op, uint32_t nrhs);

/* has the operator a plan of A^T (BFHIP_FLAG_ADJOINT / _PACKED); element type of the operand as given (BFHIP_C128 / BFHIP_F64) */
int bfhipOperatorHasAdjoint(struct BfhipOperator const *op);
uint32_t bfhipOperatorSrcDtype(struct BfhipOperator const *op);

/* GMRES around any device matvec (bfhip_gmres.c): `apply(ctx, dX, nrhs, dY, stream)` enqueues Y = A X on `stream`; n = order of A;
 * `device` = the HIP ordinal everything lives on.  bfhipSolveGMRESOptsDevice and bfhipShardedSolveGMRESDevice are this. */
typedef int (*BfGmresApplyFn)(void *ctx, void const *dX, size_t nrhs, void *dY, void *stream);
struct BfhipGmresOptions;
int bfGmresSolve(BfGmresApplyFn apply, void *ctx, uint64_t n, int device, struct BfhipGmresOptions const *opt, void const *dB, size_t nrhs,
                 void const *dX0, size_t *numIter, double *residual, void *dX, void *stream);
/* BFHIP_GMRES_ORTH_DEFAULT resolved (the environment decides: BFHIP_GMRES_MGS=1 -> MGS, else CGS2); -1 for an unknown value */
int bfGmresResolveOrth(uint32_t orthogonalization);
/* The workspace of one solver configuration (order n, at most m Krylov vectors, nrhs columns, orthogonalisation, with or without a
 * left preconditioner and x0): Krylov basis, partials, pinned Hessenberg slots, host Givens state.  Allocated once and reused by
 * any number of bfGmresRun calls (the refinement solver of bfhip_refine.c runs one per outer step); on the current device. */
typedef struct BfGmresWork {
  uint64_t n;
  size_t m, nrhs;
  uint32_t nb;
  int useMgs, hasPrecond, hasX0;
  void *dV, *dW, *dPartA, *dPartB, *dH, *dY, *dAX0, *dPartAll, *dH1, *dH2, *dPre, *dExp, *hHpinned;
  void *evCol[2];
  void *H, *S, *Jc, *Js, *y;   /* double _Complex host arrays */
  double *rnorm, *expo;        /* per column: ||r_p|| 2^-e_p and e_p (the residual's power-of-two scale) */
  size_t *len;                 /* per column: Krylov vectors its solution uses once it has stopped (SIZE_MAX while it runs) */
} BfGmresWork;
int bfGmresWorkInit(BfGmresWork *w, uint64_t n, size_t m, size_t nrhs, int orth, int hasPrecond, int hasX0);
void bfGmresWorkRelease(BfGmresWork *w);   /* idempotent; a zeroed struct is released as a no-op */
/* One GMRES solve on the workspace: `precond` (may be NULL when the workspace has none) applies M^{-1} like `apply` applies A.
 * dX0 may be non-NULL only if the workspace was made with hasX0.  Synchronous on return (the stream is drained on every path). */
int bfGmresRun(BfGmresWork *w, BfGmresApplyFn apply, void *ctx, BfGmresApplyFn precond, void *pctx, void const *dB, void const *dX0,
               double tol, size_t *numIter, double *residual, void *dX, void *stream);

/* the sharded step on host vectors (bfhip_shard.hip): staging buffers of the sharded object; used by the vtable shim */
struct BfhipSharded;
int bfhipShardedApplyHost(struct BfhipSharded *sh, int transpose, void const *X, size_t ldx, size_t nrhs, void *Y, size_t ldy);
struct BfhipOperator *bfhipShardedOperator(struct BfhipSharded const *sh);

/* ------------------------------------------------------------------------
 * Device layer (implemented in bfhip_device.hip; the GMRES / refinement kernels at the end of the section in bfhip_gmres.hip)
 * ---------------------------------------------------------------------- */
int bfdevSetDevice(int device);                 /* -1: keep current; returns BfError */
int bfdevGetDevice(int *device);
/* Run on `device`, give the caller's device back.  bfDevEnter: device < 0 keeps the current one (no call at all); otherwise the device
 * is set only when the query failed or named another one, and a failed set returns its code with the scope left inert (nothing was
 * changed).  bfDevLeave restores only after a switch whose query had succeeded; it is idempotent and a no-op on a zeroed scope, so a
 * function declares `BfDevScope ds = {0}` up front and reaches one bfDevLeave from every exit. */
typedef struct BfDevScope { int prev; int switched; } BfDevScope;
static inline int bfDevEnter(BfDevScope *s, int device) {
  s->prev = -1; s->switched = 0;
  if (device < 0) return 0;
  int const known = !bfdevGetDevice(&s->prev) && s->prev >= 0;
  if (known && s->prev == device) return 0;
  int const rc = bfdevSetDevice(device);
  if (!rc) s->switched = known;
  return rc;
}
static inline void bfDevLeave(BfDevScope *s) {
  if (s->switched) bfdevSetDevice(s->prev);
  s->switched = 0;
}
int bfdevMalloc(void **p, size_t bytes);
void bfdevFree(void *p);
int bfdevMemcpyH2D(void *dst, void const *src, size_t bytes);
int bfdevMemcpyD2H(void *dst, void const *src, size_t bytes);
int bfdevMemset(void *dst, int value, size_t bytes);
int bfdevSync(void *stream);
int bfdevPointerKind(void const *p);            /* 0 pageable host, 1 this device, 2 pinned / registered host, 3 another device */
int bfdevHostRegister(void *p, size_t bytes);
int bfdevHostUnregister(void *p);
int bfdevMemcpyAnyAsync(void *dst, void const *src, size_t bytes, void *stream);
int bfdevHostAllocPinned(void **p, size_t bytes);
void bfdevHostFreePinned(void *p);

/* fill pieces [p0, p1) of a stage with the synthetic stream, directly in HBM */
typedef struct BfSynthPiece {
  uint64_t dataOff;     /* element offset in arena */
  uint64_t vbase;       /* synthetic index of leaf element (0,0) */
  uint32_t strideR, strideC;   /* virtual index of leaf element (i, j) = vbase + i * strideR + j * strideC (n, 1 -- or 1, rows of the leaf
                                * as stored, for the leaves of a transposed view) */
  uint32_t row0, col0;
  uint32_t mr, mrPad, ncols;
  uint32_t rowMajor, ldr;      /* row-major piece: element (r, c) at dataOff + r * ldr + c */
  double scale;
} BfSynthPiece;
int bfdevSynthFill(void *arena, uint32_t dtype, BfSynthPiece const *hostPieces, uint64_t count, uint64_t seed);

typedef struct BfLaunchArgs {
  void const *arena;
  void const *items;
  void const *pieces;
  uint64_t numItems;
  uint64_t firstSmall;   /* == numItems when the stage has no small items */
  uint64_t numNarrow, numCoopNarrow, numCoop;      /* transposed: see BfStage */
  uint32_t maxRowsRest;
  void const *x;
  void *y;
  void *temp;
  void const *zero;      /* device buffer of >= 64 zero bytes */
  uint32_t nrhs;
  uint32_t dtype;
  uint32_t maxRows;
  int transposed;        /* pieces carry `ld`: lanes own columns of the forward pieces */
  void *tickets;         /* NULL, or BF_TICKET_POOLS x BF_TICKET_STRIDE uint32 owned by this stage, zero between launches (see BfStage.dTickets) */
  uint32_t exactComplex; /* BFHIP_FLAG_EXACT_COMPLEX: the matrix-core kernels form complex products with four real multiplications */
  uint32_t rhsBlocks;    /* forward plan: bfhipSetRhsBlocks (complex64) / bfhipSetRealRhsBlocks (F64, F32); adjoint plan (shared or packed):
                          * bfhipSetAdjointRhsBlocks: stages of nrhs >= rhsBlocks run the block kernels; 0 = off */
} BfLaunchArgs;
#define BF_TICKET_POOLS 64u
#define BF_TICKET_STRIDE 64u      /* uint32 between two pools' counters: a 256-byte block each -- counters that share a cache line share its atomic unit (measured: 64 packed counters behaved like one) */
int bfdevLaunchStage(BfLaunchArgs const *a, void *stream);

/* Which stage kernels bfdevLaunchStage runs (host-only: bfhipPlanStageKernels reports the same choice without a device).
 * A launch covers one or two item ranges [first, first + count); the leading `coop` items of a transposed range get a
 * workgroup each.  Two-range launches (REALBOTH: ordinary then small items; TBOTH: narrow then wide) are one kernel. */
#ifndef BF_MFMA_MIN_RHS
#define BF_MFMA_MIN_RHS 2
#endif
typedef struct BfKernelLaunch {
  uint32_t kernel;                 /* BfhipKernelId */
  uint32_t numRanges;
  uint64_t first[2], count[2], coop[2];
} BfKernelLaunch;
static inline uint32_t bfDtypeRealIndex(uint32_t dt) { return dt == BFHIP_F64 ? 0u : dt == BFHIP_F32 ? 1u : 2u; }   /* F64, F32, C64 */
static inline uint32_t bfDtypeKnown(uint32_t dt) { return dt == BFHIP_C128 || dt == BFHIP_F64 || dt == BFHIP_F32 || dt == BFHIP_C64; }
/* the matrix-core kernels come in three widths: passes of 1, 2 or 4 tiles of 16 right-hand sides (ids ..._MFMA1, _MFMA2, _MFMA4 in a row) */
static inline uint32_t bfRhsTileIndex(uint32_t nrhs) { return nrhs <= 16 ? 0u : nrhs <= 32 ? 1u : 2u; }
/* first id of the opt-in block kernels of a plan (bfhip_stage_mfma_blocks.h); 0: none (complex128 forward runs bfStageKernelC128Mfma* whatever the switch) */
static inline uint32_t bfRhsBlockKernelBase(int transposed, uint32_t dt) {
  if (transposed) return BFHIP_KERNEL_T_EXT_BASE + 3u * (dt == BFHIP_C128 ? 0u : 1u + bfDtypeRealIndex(dt));      /* C128, F64, F32, C64 */
  return dt == BFHIP_C64 ? BFHIP_KERNEL_C64_MFMA1 : dt == BFHIP_F64 ? BFHIP_KERNEL_F64_MFMA1 : dt == BFHIP_F32 ? BFHIP_KERNEL_F32_MFMA1 : 0u;
}
/* returns the number of launches (0 - 2) written to out[]; an unknown dtype gives 0 */
static inline uint32_t bfSelectStageKernels(BfLaunchArgs const *a, BfKernelLaunch out[2]) {
  if (!a->numItems || !bfDtypeKnown(a->dtype)) return 0;
  uint32_t const one = a->nrhs == 1;
  /* the plan's block kernels switched on (forward plan: bfhipSetRhsBlocks / bfhipSetRealRhsBlocks; adjoint plan, shared-leaf or packed:
   * bfhipSetAdjointRhsBlocks): one launch over all items -- ordinary and small, or narrow, wide and shared alike */
  uint32_t const blockBase = bfRhsBlockKernelBase(a->transposed, a->dtype);
  if (blockBase && a->rhsBlocks && a->nrhs >= a->rhsBlocks) {
    out[0].numRanges = 1; out[0].first[0] = 0; out[0].count[0] = a->numItems; out[0].coop[0] = 0;
    out[0].kernel = blockBase + bfRhsTileIndex(a->nrhs);
    return 1;
  }
  if (a->transposed) {
    uint64_t const numNarrow = a->numNarrow < a->numItems ? a->numNarrow : a->numItems;
    if (a->dtype != BFHIP_C128 && numNarrow && numNarrow < a->numItems && a->maxRowsRest > 16) {
      uint64_t const cntW = a->numItems - numNarrow;
      out[0].kernel = BFHIP_KERNEL_TBOTH_F64_N + 2u * bfDtypeRealIndex(a->dtype) + one;
      out[0].numRanges = 2;
      out[0].first[0] = 0; out[0].count[0] = numNarrow; out[0].coop[0] = a->numCoopNarrow < numNarrow ? a->numCoopNarrow : numNarrow;
      out[0].first[1] = numNarrow; out[0].count[1] = cntW; out[0].coop[1] = a->numCoop < cntW ? a->numCoop : cntW;
      return 1;
    }
    uint32_t n = 0;
    /* dtype-major blocks of 8 in BfhipKernelId: C128, F64, F32, C64 */
    uint32_t const dtBase = BFHIP_KERNEL_T_C128_NARROW_N + 8u * (a->dtype == BFHIP_C128 ? 0u : 1u + bfDtypeRealIndex(a->dtype));
    for (int range = 0; range < 2; ++range) {
      uint64_t const first = range ? numNarrow : 0, count = range ? a->numItems - numNarrow : numNarrow;
      if (!count) continue;
      uint32_t const wide = range == 1 && a->maxRowsRest > 16;
      uint64_t nc = range ? a->numCoop : a->numCoopNarrow;
      if (nc > count) nc = count;
      /* complex128 16-column kernel: no shared items (98 VGPRs with the shared-item code: 4 wavefronts per SIMD instead of 5) */
      if (a->dtype == BFHIP_C128 && !wide) nc = 0;
      out[n].kernel = dtBase + 4u * wide + 2u * (nc != 0) + one;
      out[n].numRanges = 1;
      out[n].first[0] = first; out[n].count[0] = count; out[n].coop[0] = nc;
      ++n;
    }
    return n;
  }
  if (a->dtype == BFHIP_C128) {
    out[0].numRanges = 1; out[0].first[0] = 0; out[0].count[0] = a->numItems; out[0].coop[0] = 0;
    if (a->nrhs < BF_MFMA_MIN_RHS) out[0].kernel = BFHIP_KERNEL_C128;
    else out[0].kernel = (a->exactComplex ? BFHIP_KERNEL_C128_MFMA1_EXACT : BFHIP_KERNEL_C128_MFMA1) + bfRhsTileIndex(a->nrhs);
    return 1;
  }
  /* the real family: items [firstSmall, numItems) are small (four to a wavefront) */
  uint32_t const r = bfDtypeRealIndex(a->dtype);
  uint64_t const firstSmall = a->firstSmall < a->numItems ? a->firstSmall : a->numItems;
  uint64_t const numSmall = a->numItems - firstSmall;
  uint32_t n = 0;
  if (firstSmall && numSmall) {
    out[0].kernel = BFHIP_KERNEL_REALBOTH_F64 + r;
    out[0].numRanges = 2;
    out[0].first[0] = 0; out[0].count[0] = firstSmall; out[0].coop[0] = 0;
    out[0].first[1] = firstSmall; out[0].count[1] = numSmall; out[0].coop[1] = 0;
    return 1;
  }
  if (firstSmall) {
    out[n].kernel = BFHIP_KERNEL_REAL_F64 + r; out[n].numRanges = 1;
    out[n].first[0] = 0; out[n].count[0] = firstSmall; out[n].coop[0] = 0; ++n;
  }
  if (numSmall) {
    out[n].kernel = BFHIP_KERNEL_SMALL_F64 + r; out[n].numRanges = 1;
    out[n].first[0] = firstSmall; out[n].count[0] = numSmall; out[n].coop[0] = 0; ++n;
  }
  return n;
}
/* bfReduceKernel of one batch: `longLists` = some reduce of the batch has a row of >= 64 partial sums (complex128 has no
 * long instantiation); BFHIP_KERNEL_COUNT for an unknown dtype */
static inline uint32_t bfSelectReduceKernel(uint32_t dtype, int longLists) {
  if (dtype == BFHIP_C128) return BFHIP_KERNEL_REDUCE_C128;
  if (dtype == BFHIP_C64) return longLists ? BFHIP_KERNEL_REDUCE_C64_LONG : BFHIP_KERNEL_REDUCE_C64;
  if (dtype == BFHIP_F64) return longLists ? BFHIP_KERNEL_REDUCE_F64_LONG : BFHIP_KERNEL_REDUCE_F64;
  if (dtype == BFHIP_F32) return longLists ? BFHIP_KERNEL_REDUCE_F32_LONG : BFHIP_KERNEL_REDUCE_F32;
  return BFHIP_KERNEL_COUNT;
}
#define BF_REDUCE_BATCH 16        /* reduces per bfReduceKernel launch (their descriptors travel in the kernel arguments) */
/* bfhip_persist.hip (experimental persistent launch of the complex128 stage kernel) */
uint32_t bfdevPersistentGrid(void);
int bfdevLaunchPersistC128(void const *stageParams, uint32_t grid, void *tickets, void *timeline, void *stream);

/* dependency-driven launch of a whole forward complex128 plan (bfFlowKernelC128): see bfhip_experimental.hip */
typedef struct BfFlowArgs {
  void const *arena;
  void const *items, *pieces, *itemOut, *writers;   /* flat over all stages; pieces' `ld` holds the vector id they read */
  void *counters;        /* uint32[numBufs]: [0] the ticket queue, [1] the error flag, [id >= 2] writes seen by vector id */
  uint32_t numItems, nrhs, epoch, queueBase, gridWorkgroups;
  void const *x;
  void *y, *temp;
} BfFlowArgs;
int bfdevLaunchFlow(BfFlowArgs const *a, void *stream);
/* EXPERIMENTAL builds: timeline / persistent launch of a complex128 stage (bfhip_experimental.hip); *handled = 0 -> the caller launches it */
int bfdevLaunchStageExperimental(BfLaunchArgs const *a, void const *stageParams, uint32_t grid, void *stream, int *handled);
int bfdevFlowGrid(uint64_t numItems, uint32_t *grid);
int bfdevMemsetAsync(void *dst, int value, size_t bytes, void *stream);

typedef struct BfReduceArgs {
  void const *rowInterval, *ivBegin, *srcBias;
  uint64_t numRows;
  void const *temp;
  void *dest;            /* already offset to destOff*nrhs */
  uint32_t nrhs;
  uint32_t dtype;
  uint32_t longLists;    /* some row has >= 64 partial sums: the launch uses the kernel that loads them 32 at a time */
  uint32_t pad;
} BfReduceArgs;
/* all `count` reduces (one stage; same temp / nrhs / dtype) in as few launches as possible */
int bfdevLaunchReduce(BfReduceArgs const *a, uint32_t count, void *stream);
int bfdevScalePermute(void *dst, void const *src, void const *scale, int power, uint64_t const *perm, uint64_t n, uint32_t dtype, void *stream);

/* the batched covariance entries' plumbing (bfhip_cov.hip): blocks are row-major rows x nrhs, densely packed, F64 / F32 */
/* dst[perm ? perm[i] : i, :] = src[i, :] * (scale ? scale[i]^power : 1); src == dst is legal when perm == NULL */
int bfdevCovScalePermute(void *dst, void const *src, void const *scale, int power, uint64_t const *perm, uint64_t rows, uint32_t nrhs, uint32_t dtype, void *stream);
/* d[i] = N(seed, firstIdx + i) (bfhip_normal_value) */
int bfdevFillNormal(void *d, uint64_t count, uint64_t firstIdx, uint32_t dtype, uint64_t seed, void *stream);
/* w[j, s] = N(seed, (firstSample + s) * cols + j) * (gamma ? gamma[j] : 1), w is cols x nrhs */
int bfdevCovDrawFill(void *w, void const *gamma, uint64_t cols, uint32_t nrhs, uint32_t dtype, uint64_t seed, uint64_t firstSample, void *stream);
/* sum[perm ? perm[i] : i] += sum_q t[i, q], sumSq[...] += sum_q t[i, q]^2 over the b columns of t (rows x b); either output may be NULL */
int bfdevCovMoments(void const *t, uint64_t rows, uint32_t b, uint32_t dtype, uint64_t const *perm, double *sum, double *sumSq, void *stream);

/* one Clenshaw step of the Chebyshev covariance (bfhip_cheb.hip; driven by bfhip_cheb.c): on blocks of n x q doubles
 *   out[i, :] = ck * (wScale ? wScale[i] : 1) * w[i, :] + alpha * sum_j S[i][j] * b1[col_j, :] + beta * b1[i, :] - b2[i, :]
 * and then out[i, :] *= outScale[i] when outScale is given.  b1 == NULL drops the two b1 terms, b2 == NULL the last one;
 * out may be b2 (a row's owner is the only reader of its b2 row) and nothing else it reads.  S is CSR on the device:
 * rowptr uint64 [n + 1], colind uint32, values double */
typedef struct BfChebStep {
  uint64_t const *rowptr;
  uint32_t const *colind;
  double const *val;
  uint64_t n;
  uint32_t q;
  double const *w, *wScale, *b1, *b2, *outScale;
  double *out;
  double ck, alpha, beta;
} BfChebStep;
int bfdevChebStep(BfChebStep const *s, void *stream);
/* U [n x p] = D E: U[j, c] = d[j] where j == rows[c], else 0 (the whole block is written; rows [p] on the device, p <= 64) */
int bfdevChebUnitPanel(double *U, uint64_t n, uint32_t p, uint64_t const *dRows, double const *d, void *stream);

/* the object of the Chebyshev covariance (bfhip_cheb.c makes and frees it; bfhip_eigs.c reads S, D and lamMax from it) */
struct BfhipChebCov {
  int device;
  uint64_t n, nnz;
  double lamMax;
  void *dRowptr, *dColind, *dVal, *dD;
  uint64_t deviceBytes;
  double *coef;
  size_t order;
  uint64_t generation;          /* bumped by every SetCoefficients: a conditioning object made before it is stale */
  void *dWork;
  uint64_t workBytes;
  /* the consistent mass of the eigensolver (bfhipChebCovSetConsistentMass, bfhip_eigs_mass.c): host copies of
   * the pattern and of d, which the fold and its checks read before the device is touched; B = D M D on S's pattern (NULL: none
   * set), an interval that encloses its spectrum, and the launches of bfhip_eigs_mass.hip */
  uint64_t *hRowptr;
  uint32_t *hColind;
  double *hD;
  void *dMass;
  double massLo, massHi;
  struct BfEigsMassOps const *massOps;
};

/* filtered subspace iteration on S (bfhip_eigs.hip; driven by bfhip_eigs.c).  Blocks are row-major n x ld doubles, ld = p
 * rounded up to a multiple of 16, the padding columns zero and never written.
 *   step:     out = alpha (S b1) + beta b1 + gamma b2 on the first p columns; b2 may be NULL, out may be b2
 *   gram:     G [ld x ld] = X^T Y, partials per chunk of bfdevEigsChunkRows rows in `part` (chunks x ld x ld), summed in chunk order
 *   rotate:   out = X W, W [ld x ld] on the device with zero padding; out is another block
 *   residual: sumSq[c] = sum_r (Y[r][c] - theta[c] X[r][c])^2, partials in `part` (chunks x ld)
 *   store:    dst[i * ldu + j] = (d ? d[i] : 1) X[i][j], j < nev */
typedef struct BfEigsStep {
  uint64_t const *rowptr;
  uint32_t const *colind;
  double const *val;
  uint64_t n;
  uint32_t p, ld;
  double const *b1, *b2;
  double *out;
  double alpha, beta, gamma;
} BfEigsStep;
uint64_t bfdevEigsChunkRows(uint64_t n, uint32_t ld);
int bfdevEigsStep(BfEigsStep const *s, void *stream);
int bfdevEigsGram(double const *X, double const *Y, uint64_t n, uint32_t ld, double *part, double *G, void *stream);
int bfdevEigsRotate(double const *X, double const *W, double *out, uint64_t n, uint32_t ld, void *stream);
int bfdevEigsResidual(double const *X, double const *Y, double const *theta, uint64_t n, uint32_t ld, double *part, double *sumSq, void *stream);
int bfdevEigsStore(double const *X, uint64_t n, uint32_t ld, uint32_t nev, double const *d, double *dst, uint64_t ldu, void *stream);
/* deflation against locked eigenvectors.  dQ [n x >= m0 + mq, row-major, leading dimension ldq] lies in the
 * caller's layout: no alignment beyond 8 bytes of dQ, ldq or m0; a panel is the mq <= 256 columns from m0.  mq16 = mq rounded up to 16.
 *   crossGram: C [mq16 x ld] = Q[:, m0 .. m0 + mq)^T X, rows from mq on exact +0; partials per chunk of bfdevEigsCrossChunkRows rows in
 *              `part` (chunks x mq16 x ld), summed in chunk order
 *   deflate:   X <- X - Q[:, m0 .. m0 + mq) C in place (C as crossGram leaves it)
 *   project:   one pass over all m locked columns, panel by panel: crossGram, then deflate; part: chunks x min(m16, 256) x ld, C: min(m16, 256) x ld */
uint64_t bfdevEigsCrossChunkRows(uint64_t n, uint32_t ld);
int bfdevEigsCrossGram(double const *dQ, uint64_t ldq, uint64_t m0, uint32_t mq, double const *X, uint64_t n, uint32_t ld, double *part, double *C,
                       void *stream);
int bfdevEigsDeflate(double const *dQ, uint64_t ldq, uint64_t m0, uint32_t mq, double const *C, double *X, uint64_t n, uint32_t ld, void *stream);
int bfdevEigsProject(double const *dQ, uint64_t ldq, uint64_t m, double *X, uint64_t n, uint32_t ld, double *part, double *C, void *stream);
/* the consistent-mass pencil S u = theta B u (bfhip_eigs_mass.hip).  B lies on S's pattern (rowptr, colind) with
 * values of its own.
 *   massStep: out = alpha (B b1) + beta b1 + gamma b2 + delta w on the first p columns.  b1 == NULL drops its two terms (no gather),
 *             b2 == NULL and w == NULL theirs; out may be b2 and nothing else the launch reads
 *   massSolve: z ~ B^-1 t by `steps` >= 1 steps of the three-term Chebyshev semi-iteration on [lo, hi] from z = 0, one massStep each
 *             (the first has no product: z_1 = 2 / (hi + lo) t); `work` is a second block; the result is in z, work holds z_{steps-1}
 *   combine:  out = a z + b y1 + g y2 on the first p columns, y2 == NULL drops its term, out may be y2
 *   projectMass: X <- X - Q (Q^T BX) over all m locked columns with BX given: per panel of <= 256 crossGram(Q, BX), deflate(Q, C, X)
 *   dualProduct: outS = S b1 and outB = B b1 from one gather of b1's rows, each bit-equal to its single launch (Rayleigh-Ritz needs both
 *             of the same X; 0.64 of the two launches' time at n = 2^20, p = 64) */
typedef struct BfEigsMassStep {
  uint64_t const *rowptr;
  uint32_t const *colind;
  double const *val;
  uint64_t n;
  uint32_t p, ld;
  double const *b1, *b2, *w;
  double *out;
  double alpha, beta, gamma, delta;
} BfEigsMassStep;
typedef struct BfEigsMassSolve {
  uint64_t const *rowptr;
  uint32_t const *colind;
  double const *val;
  uint64_t n;
  uint32_t p, ld;
  double const *t;
  double *z, *work;
  double lo, hi;
  uint32_t steps, reserved;
} BfEigsMassSolve;
int bfdevEigsMassStep(BfEigsMassStep const *s, void *stream);
int bfdevEigsMassSolve(BfEigsMassSolve const *s, void *stream);
int bfdevEigsCombine(double const *z, double const *y1, double const *y2, double *out, uint64_t n, uint32_t p, uint32_t ld, double a, double b,
                     double g, void *stream);
int bfdevEigsDualProduct(uint64_t const *rowptr, uint32_t const *colind, double const *valS, double const *valB, uint64_t n, uint32_t p, uint32_t ld,
                         double const *b1, double *outS, double *outB, void *stream);
int bfdevEigsProjectMass(double const *dQ, uint64_t ldq, uint64_t m, double const *BX, double *X, uint64_t n, uint32_t ld, double *part, double *C,
                         void *stream);
/* what bfhip_eigs.c calls through the object (bfhipChebCovSetConsistentMass stores the table: bfhip_eigs.c names none of these launches) */
typedef struct BfEigsMassOps {
  int (*step)(BfEigsMassStep const *s, void *stream);
  int (*solve)(BfEigsMassSolve const *s, void *stream);
  int (*combine)(double const *z, double const *y1, double const *y2, double *out, uint64_t n, uint32_t p, uint32_t ld, double a, double b, double g,
                 void *stream);
  int (*project)(double const *dQ, uint64_t ldq, uint64_t m, double const *BX, double *X, uint64_t n, uint32_t ld, double *part, double *C,
                 void *stream);
  int (*dual)(uint64_t const *rowptr, uint32_t const *colind, double const *valS, double const *valB, uint64_t n, uint32_t p, uint32_t ld,
              double const *b1, double *outS, double *outB, void *stream);
} BfEigsMassOps;
/* host, bfhip_eigs_mass.c: the checks of bfhipChebCovSetConsistentMass that need no device and the fold B[k] = (d[i] M[k]) d[col[k]];
 * outside the public header so that tests/native/fem_mass_check.c can call it alone.  lo <= 0 && hi <= 0: the P1 bounds, after
 * the row sums and the diagonal were checked; *lo and *hi return the interval in force */
int bfEigsMassFold(uint64_t n, uint64_t const *rowptr, uint32_t const *colind, double const *d, double const *Mdata, double *lo, double *hi, double *B);
/* host, bfhip_eigs.c: the eigenpairs of a symmetric p x p matrix (row-major, lda), ascending, Q's columns the vectors; outside the
 * public header so that tests/native/eigs_symeig_check.c can call it alone.  work: 2 p doubles.  Returns 0, or 1 when QL did not converge */
int bfEigsSymEig(size_t p, double *A, size_t lda, double *theta, double *work);
/* host, bfhip_eigs.c: the iteration behind bfhipChebCovEigsDevice (locked NULL, defl NULL) and bfhipChebCovEigsBandDevice
 * (bfhip_eigs_band.c, which passes { bfdevEigsProject, bfdevEigsCrossChunkRows }: bfhip_eigs.c itself names no launch newer than
 * section 25's, so that tests/native/eigs_symeig_check.c still links it against its fixed list of stand-ins).  project runs one
 * projection pass; chunkRows sizes the partials it needs. */
typedef int (*BfEigsProjectFn)(double const *dQ, uint64_t ldq, uint64_t m, double *X, uint64_t n, uint32_t ld, double *part, double *C, void *stream);
typedef struct BfEigsDeflation { BfEigsProjectFn project; uint64_t (*chunkRows)(uint64_t n, uint32_t ld); } BfEigsDeflation;
/* the last profiled call of this thread (bfEigsProfile; tools/lbo_bands_rate.py): seconds spent projecting, and per Rayleigh-Ritz
 * step (at most 128 are kept) the largest residual of the wanted pairs over lamMax and the degree of the filter before it */
double bfEigsLastProjectSeconds(void);
uint32_t bfEigsLastHistory(double *residual, uint32_t *degree, uint32_t cap);
int bfEigsSolve(BfhipChebCov *c, BfhipEigsOptions const *opt, BfhipEigsLocked const *locked, BfEigsDeflation const *defl, size_t nev, double *lam,
                double *residual, double *dU, size_t ldu, BfhipEigsInfo *info, void *stream);
/* phase seconds of the last bfhipChebCovEigsDevice of this thread when bfEigsProfile(1) was called before (tools/lbo_eigs_rate.py):
 * filter, S X, Gram, rotate, residual, host dense, summed over the call; the phases are then separated by stream synchronisations */
void bfEigsProfile(int on);
void bfEigsLastPhases(double out[6]);
/* the same switch for bfhipChebCovCondLogLikGradDevice (bfhip_cheb.c; tools/cheb_gradient_rate.py): phase seconds of this thread's
 * last call, summed over its panels: alpha and value, the M panels, the contraction, the recurrences, the dot and the owner's sum */
void bfChebGradProfile(int on);
void bfChebGradLastPhases(double out[5]);

/* device-resident GMRES building blocks (bfhip_gmres.hip; complex128; bfhip_gmres.c drives them).
 * Vectors are n x nrhs row-major; reductions are per RHS column, two-stage and
 * in fixed order (per-block partials, then a tree over the partials), so a
 * solve is bit-reproducible.  `nb` = number of row blocks = partials per RHS. */
/* W = B - AX0 (AX0 may be NULL); partialOut = per-block (|W|^2, largest |component|).  With expOut (nrhs doubles) it then scales
 * each column: e = binary exponent of its largest component (0 for a zero column), W *= 2^-e exactly, expOut[q] = e, and
 * partialScaled = per-block |W|^2 of the scaled column */
int bfdevGmresResidual(void const *B, void const *AX0, void *W, void *partialOut, uint64_t n, uint32_t nrhs, uint32_t nb, void *expOut,
                       void *partialScaled, void *stream);
int bfdevGmresDot(void const *Vi, void const *W, void *partialOut, uint64_t n, uint32_t nrhs, uint32_t nb, void *stream);
/* h = sum(partialIn); hOut[q] = h; W -= h * Vi; then partialOut = conj(Vnext).W (Vnext != NULL) or |W|^2 */
int bfdevGmresMgsStep(void const *Vi, void const *Vnext, void *W, void const *partialIn, void *partialOut, void *hOut,
                      uint64_t n, uint32_t nrhs, uint32_t nb, void *stream);
/* batched Gram-Schmidt pass over V_0..V_{numVec-1} (vectors n*nrhs apart): partial[(q*numVec + i)*nb + b] */
int bfdevGmresDots(void const *V, void const *W, void *partial, uint64_t n, uint32_t nrhs, uint32_t nb, uint32_t numVec, void *stream);
/* h[i*nrhs + q] = sum_b partial; hSum = h + hPrev (hSum / hPrev may be NULL) */
int bfdevGmresDotsFinish(void const *partial, void const *hPrev, void *h, void *hSum, uint32_t nrhs, uint32_t nb, uint32_t numVec, void *stream);
/* W -= sum_i h_i V_i; partialOut (may be NULL) = per-block |W|^2 */
int bfdevGmresProject(void const *V, void *W, void const *h, void *partialOut, uint64_t n, uint32_t nrhs, uint32_t nb, uint32_t numVec, void *stream);
/* nrm = sqrt(sum(partialIn)); hOut[q] = nrm; Vout = W / nrm, or 0 where nrm is 0 */
int bfdevGmresFinish(void const *W, void const *partialIn, void *Vout, void *hOut, uint64_t n, uint32_t nrhs, uint32_t nb, void *stream);
/* X = X0 + sum_{i<j} V_i * y[i] ; V = (j) vectors of n*nrhs, y = [j][nrhs]; a zero y[i] adds nothing (not even +0) */
int bfdevGmresUpdate(void const *X0, void const *V, void const *y, uint32_t j, void *X, uint64_t n, uint32_t nrhs, void *stream);
/* mixed-precision refinement (bfhip_refine.c drives them; streaming kernels, not stage kernels: no BfhipKernelId).
 * count = complex elements.  Demote rounds each component to nearest. */
int bfdevRefineDemote(void const *src128, void *dst64, uint64_t count, void *stream);
int bfdevRefinePromote(void const *src64, void *dst128, uint64_t count, void *stream);
/* R, partialIn, expIn: the scaled column, its |R|^2 partials and its exponent e as bfdevGmresResidual leaves them (W, partialScaled,
 * expOut).  Per column q: s = sqrt(sum of the nb partials); s > 0: Rhat = R / s, scale[q] = 2^e s (the norm of the unscaled column);
 * s == 0: Rhat = 1/sqrt(n) (a unit right-hand side), scale[q] = 0.  scale: nrhs doubles on the device */
int bfdevRefineScale(void const *R, void const *partialIn, double const *expIn, void *Rhat, double *scale, uint64_t n, uint32_t nrhs, uint32_t nb,
                     void *stream);
/* Xout = Xin + scale[q] * D per column (Xin NULL = zeros); a column with scale 0 is Xin exactly, whatever D holds */
int bfdevRefineUpdate(void const *Xin, void const *D, double const *scale, void *Xout, uint64_t n, uint32_t nrhs, void *stream);
int bfdevMemcpyD2HAsync(void *dst, void const *src, size_t bytes, void *stream);

/* ------------------------------------------------------------------------
 * Builder device layer (bfhip_build.hip: kernel evaluation, pack, dense check; bfhip_lstsq.hip: the truncated
 * least squares -- QR, Jacobi SVD, GEMM; driven by bfhip_build.c).  All
 * matrices are complex128, column-major; offsets are in complex elements
 * relative to the base pointer named per call.
 * ---------------------------------------------------------------------- */
typedef struct BfBuildPts {        /* = BfhipPointSet (include/bfhip_build.h) */
  uint32_t kind, count;
  uint64_t first;
  double cx, cy, r;
} BfBuildPts;

/* one kernel matrix to evaluate: dst[i + j*tgt.count] = G(tgt_i, src_j) */
typedef struct BfEvalMat {
  BfBuildPts src, tgt;
  void *dst;
  uint32_t pot;          /* 0: S, 1: S' (target normals; tree targets), 2: D (source normals), 3: alpha S + beta D */
  uint32_t decorate;     /* 1: apply column weights / self value (leaves of the operator, not Z_equiv) */
} BfEvalMat;
/* what every kernel evaluation needs besides the two points */
typedef struct BfEvalEnv {
  void const *dPoints, *dNormals, *dColWeights;   /* device; normals / weights may be NULL */
  void const *dTgtPoints, *dTgtNormals;           /* separate target tree (BFHIP_PTS_TREE_TGT) or NULL */
  void const *dOrigIndex;                         /* device uint64[numPoints] or NULL */
  double wavenumber, selfRe, selfIm;
  double alphaRe, alphaIm, betaRe, betaIm;
  uint64_t numPoints;
  uint32_t krOrder;                               /* 0, 2, 6, 10 */
  unsigned long long *dKrHits;                    /* device counter of corrected entries (consistency check) or NULL */
} BfEvalEnv;
/* tilePrefix[numMats+1]: prefix sums of ceil(rows*cols / BF_EVAL_TILE) */
#define BF_EVAL_TILE 1024u
int bfdevBuildEval(BfEvalMat const *hostMats, uint64_t const *hostTilePrefix, uint64_t numMats, BfEvalEnv const *env);

/* one-sided Jacobi SVD of A (mt x me, mt >= me), in place: on return the
 * columns of A are U*Sigma, V (me x me) holds the right singular vectors and
 * scale[j] = 1/sigma_j^2 (0 for truncated sigma_j < max(mt,me) eps sigma_max + eps) */
typedef struct BfSvdProb {
  void *a, *v;
  double *scale;         /* [me] */
  uint32_t mt, me;
  uint32_t dim, pad;     /* the max(rows, cols) of the truncation rule (src/mat_dense_complex.c:1800-1812): that of the ORIGINAL
                            matrix when (a) is the QR-preconditioned one */
  uint32_t *info;        /* device [3] or NULL: sweeps, not converged (0/1), singular values kept */
  void *pad2;
} BfSvdProb;
typedef struct BfSvdStats { unsigned long long maxSweeps, notConverged, truncated, sumSweeps; } BfSvdStats;

/* ---- routing of a least-squares problem (host-only; bfhipLstSqRoutes reports it without a device) ----
 * Sizes the Jacobi kernels are built for: columns of the plain kernel's live list, columns of the block (Gram) form, the
 * largest LDS tile, and the tiles of the four LDS classes. */
#define BF_JACOBI_MAX_COLS 2304          /* 2 (rows + cols) 16 B <= the LDS tile  =>  cols <= 2300 */
#define BF_GRAM_MAX_COLS 4096
#define BF_JACOBI_LDS_MAX (144u << 10)
#define BF_QR_LDS_CLASSES 6
enum { BF_JACOBI_PLAIN = 0, BF_JACOBI_GRAM = 1, BF_JACOBI_GLOBAL = 2 };
/* the route's switches: < 0 takes the default (the BFHIP_JACOBI_QR_MIN / _GRAM_MIN / _GLOBAL environment hooks, else 65 /
 * 512 / 0); qrMin: problems with at least this many columns get the QR preconditioner (0: all); gramMin: problems with
 * rows + columns >= gramMin go to the Gram form; forceGlobal: 1 sends every Jacobi problem to the global-memory kernel */
typedef struct BfLstSqOpts { int64_t qrMin, gramMin, forceGlobal; } BfLstSqOpts;
typedef struct BfLstSqRoute {
  uint32_t qr;           /* 1: bfQrcpKernel first */
  uint32_t qrLdsClass;   /* 0..5: 8, 16, 32, 64, 128, 150 KiB */
  uint32_t qrStreaming;  /* 1: columns longer than 1024 rows, streamed (else held in registers) */
  uint32_t jacobi;       /* BF_JACOBI_* */
  uint32_t w, threads;   /* plain kernel: lane-group width and workgroup size */
  uint32_t ldsClass;     /* plain kernel: 0..3, 16, 32, 64, 144 KiB */
  uint32_t resident;     /* plain kernel: the whole stacked matrix stays in LDS (else block sweeps) */
} BfLstSqRoute;
static inline int64_t bfLstSqEnvInt(char const *name, int64_t dflt) {
  char const *e = getenv(name);
  return e && e[0] ? (int64_t)strtoull(e, NULL, 10) : dflt;
}
static inline BfLstSqOpts bfLstSqResolve(BfLstSqOpts const *o) {
  BfLstSqOpts r;
  r.qrMin = o && o->qrMin >= 0 ? o->qrMin : bfLstSqEnvInt("BFHIP_JACOBI_QR_MIN", 65);
  r.gramMin = o && o->gramMin >= 0 ? o->gramMin : bfLstSqEnvInt("BFHIP_JACOBI_GRAM_MIN", 512);
  if (o && o->forceGlobal >= 0) r.forceGlobal = o->forceGlobal != 0;
  else { char const *e = getenv("BFHIP_JACOBI_GLOBAL"); r.forceGlobal = e && e[0] == '1'; }
  return r;
}
/* LDS the QR kernel needs for an mt x me problem (0: does not fit), and its class */
static inline uint32_t bfQrcpLds(uint32_t mt, uint32_t me) {
  uint64_t const need = (uint64_t)mt * 16 + (uint64_t)me * 12 + 64;
  return need <= (150u << 10) ? (uint32_t)need : 0;
}
static inline uint32_t bfQrcpLdsCap(uint32_t cls) {
  static uint32_t const cap[BF_QR_LDS_CLASSES] = {8u << 10, 16u << 10, 32u << 10, 64u << 10, 128u << 10, 150u << 10};
  return cap[cls];
}
static inline uint32_t bfQrcpLdsClass(uint32_t need) {
  uint32_t c = 0;
  while (c + 1 < BF_QR_LDS_CLASSES && bfQrcpLdsCap(c) < need) ++c;
  return c;
}
/* LDS tile of the four classes of the plain Jacobi kernel: the router picks the class, the launcher asks for its bytes */
#define BF_JACOBI_LDS_CLASSES 4
static inline uint32_t bfJacobiLdsCap(uint32_t cls) {
  static uint32_t const cap[BF_JACOBI_LDS_CLASSES] = {16u << 10, 32u << 10, 64u << 10, BF_JACOBI_LDS_MAX};
  return cap[cls];
}
/* Geometry of the plain Jacobi kernel's tile of ldsBytes for an mt x me problem, the one copy the router and
 * bfJacobiKernel share.  A stacked column [a_j; v_j] has mt + me rows; Rp, its stride in 16-byte units, is odd so that
 * the lane groups of a wavefront spread over the banks.  The tile holds an even number C >= 2 of them: blocks of
 * b = min(C / 2, ceil(me / 2)) columns, a pair of blocks at a time.  resident: at most two blocks, so everything is
 * loaded once and slot = column.  (me = 0 gives b = 0 and counts as resident; the kernel returns before it asks.) */
typedef struct BfJacobiTile { uint32_t Rp, b, resident; } BfJacobiTile;
BF_HOST_DEVICE static inline BfJacobiTile bfJacobiTile(uint32_t ldsBytes, uint32_t mt, uint32_t me) {
  BfJacobiTile t;
  t.Rp = (mt + me) | 1u;
  uint32_t C = (ldsBytes / 16u) / t.Rp;
  C = C < 2 ? 2 : C & ~1u;
  t.b = C / 2 < (me + 1) / 2 ? C / 2 : (me + 1) / 2;
  t.resident = t.b ? (me + t.b - 1) / t.b <= 2 : 1;
  return t;
}
/* the Jacobi stage of an mt x me problem (after the QR stage: me x rank) */
static inline void bfJacobiRoute(uint32_t mt, uint32_t me, BfLstSqOpts const *o, BfLstSqRoute *r) {
  uint64_t const R = (uint64_t)mt + me, Rp = R | 1u;       /* 64 bits: `fits` is asked of every shape */
  r->w = 64; r->threads = 1024; r->ldsClass = 0; r->resident = 0;
  int const fits = !(2 * Rp * 16 > BF_JACOBI_LDS_MAX || me > BF_JACOBI_MAX_COLS);
  if (!o->forceGlobal && me <= BF_GRAM_MAX_COLS && (!fits || R >= (uint64_t)o->gramMin)) { r->jacobi = BF_JACOBI_GRAM; r->threads = 512; return; }
  if (!fits || o->forceGlobal) { r->jacobi = BF_JACOBI_GLOBAL; return; }
  r->jacobi = BF_JACOBI_PLAIN;
  uint64_t const meEven = me + (me & 1u);
  uint32_t lc = BF_JACOBI_LDS_CLASSES - 1;
  for (uint32_t c = 0; c + 1 < BF_JACOBI_LDS_CLASSES; ++c)
    if (meEven * Rp * 16 <= bfJacobiLdsCap(c)) { lc = c; break; }
  BfJacobiTile const t = bfJacobiTile(bfJacobiLdsCap(lc), mt, me);
  r->ldsClass = lc;
  r->threads = me > 64 ? 1024 : 256;
  uint32_t w = 64;
  while (w > 4 && (r->threads / w < t.b || w / 2 >= mt)) w >>= 1;
  r->w = w;
  r->resident = t.resident;
}
/* the whole route of an mt x me least-squares problem; `rank`: what the QR stage leaves for the Jacobi stage (if it runs) */
static inline void bfLstSqRoute(uint32_t mt, uint32_t me, uint32_t rank, BfLstSqOpts const *o, BfLstSqRoute *r) {
  uint32_t const need = bfQrcpLds(mt, me);
  r->qr = me >= o->qrMin && need != 0;
  r->qrLdsClass = r->qr ? bfQrcpLdsClass(need) : 0;
  r->qrStreaming = r->qr && mt > 1024;
  if (r->qr) bfJacobiRoute(me, rank, o, r);
  else bfJacobiRoute(mt, me, o, r);
}
int bfdevBuildJacobi(BfSvdProb const *hostProbs, uint64_t numProbs, BfLstSqOpts const *opts, BfSvdStats *stats);

/* QR with column pivoting ahead of the Jacobi SVD (bfQrcpKernel): a (mt x me, ld mt) is overwritten (R in its upper
 * triangle), b (mt x n, ld mt) becomes Q^H b, x (me x me workspace) receives the me x rank matrix the Jacobi kernel
 * then works on (ld me); hostRanks[i] = the number of steps taken before the trailing columns' total squared norm fell
 * below (dim * eps)^2 x the largest squared column of a, with BF_QR_NONFINITE set when a holds a NaN or an infinity. */
#define BF_QR_NONFINITE 0x80000000u
typedef struct BfQrProb {
  void *a, *b, *x;
  uint32_t mt, me, n, dim;
} BfQrProb;
int bfdevQrcpFits(uint32_t mt, uint32_t me);
int bfdevBuildQrcp(BfQrProb const *hostProbs, uint64_t numProbs, uint32_t *hostRanks);

/* C (M x N) = op(A) * B with optional row scaling C[i,:] *= scale[i];
 * transA: op(A)[i,k] = conj(A[k + i*lda]) (A stored K x M), else A[i + k*lda] */
typedef struct BfGemmJob {
  void const *a, *b;
  void *c;
  double const *scale;   /* NULL: none */
  uint32_t M, N, K, lda, ldb, ldc, transA, pad;
} BfGemmJob;
int bfdevBuildGemm(BfGemmJob const *hostJobs, uint64_t numJobs);

/* column-major: arena[dataOff + c*mrPad + r] = r < mr ? store[srcOff + c*srcLd + r] : 0,      r < mrPad, c < ncols
 * row-major:    arena[dataOff + r*ld + c]    = c < ncols ? store[srcOff + c*srcLd + r] : 0,   r < mr,    c < ld
 * The store is complex128; the arena holds outDtype (BFHIP_C128: copied; BFHIP_C64: each component rounded to float once). */
typedef struct BfPackPiece {
  uint64_t dataOff, srcOff;
  uint32_t srcLd, mr, mrPad, ncols;
  uint32_t rowMajor, ld;     /* BF_PIECE_ROWMAJOR pieces (real-family plans) and their row stride */
} BfPackPiece;
int bfdevBuildPack(void *arena, uint32_t outDtype, void const *store, BfPackPiece const *hostPieces, uint64_t count);

int bfdevMemFree(uint64_t *freeBytes);    /* free device memory right now */

/* y = G x, N x N single-layer kernel evaluated on the fly; scratch is allocated inside */
/* numTgt == 0: square (targets = the points); else targets = env->dTgtPoints */
int bfdevHelm2Dense(BfEvalEnv const *env, uint32_t pot, uint64_t n, uint64_t numTgt, void const *dX, void *dY, void *stream);
int bfdevMemcpyH2DAsync(void *dst, void const *src, size_t bytes, void *stream);
int bfdevMemcpyD2DAsync(void *dst, void const *src, size_t bytes, void *stream);

/* events for BFHIP_FLAG_PROFILE */
int bfdevEventCreate(void **ev);
void bfdevEventDestroy(void *ev);
int bfdevEventRecord(void *ev, void *stream);
int bfdevEventElapsed(void *start, void *stop, float *ms);
int bfdevEventSync(void *ev);

/* dense extraction A[I, J] (bfhip_extract.hip; driven by bfhip_extract.c only -- no file of the host sanitizer harness calls
 * these).  Index lists are (idx, base): entry k is idx[base + k], or base + k when idx == NULL (all rows / columns).
 * Unit panel: X[prev(k) * prevLd + k] = 0 for k < prevCount, then X[new(k) * ld + k] = 1 for k < count (<= 64 each).
 * Gather: Out[i * ldOut + k] = Y[rows(i) * p + k].  Transposed gather: Out[k * ldOut + j] = P[cols(j) * p + k] (p <= 64).
 * An index >= ext is skipped (unit) or reads as zero (gathers). */
int bfdevExtractUnit(void *X, uint32_t dtype, uint64_t ext, uint64_t const *prevIdx, uint64_t prevBase, uint32_t prevCount, uint32_t prevLd,
                     uint64_t const *idx, uint64_t base, uint32_t count, uint32_t ld, void *stream);
int bfdevExtractGather(void *Out, uint64_t ldOut, void const *Y, uint64_t ext, uint32_t p, uint64_t const *rows, uint64_t rowBase, uint64_t numRows,
                       uint32_t elemSize, void *stream);
int bfdevExtractGatherT(void *Out, uint64_t ldOut, void const *P, uint64_t ext, uint32_t p, uint64_t const *cols, uint64_t colBase, uint64_t numCols,
                        uint32_t elemSize, void *stream);
int bfdevStreamCreateNonBlocking(void **stream);
void bfdevStreamDestroy(void *stream);
int bfdevStreamWaitEvent(void *stream, void *ev);
int bfdevMemcpy2DAsync(void *dst, size_t dpitch, void const *src, size_t spitch, size_t width, size_t height, void *stream);

/* host side of the extraction (the operator of bfhip_operator.h keeps the state, bfhip_api.c releases it; bfhip_extract.c owns what it means) */
/* the operator's extraction workspace slot; `release` is stored and called on it by bfhipFree */
void **bfhipOperatorExtractSlot(struct BfhipOperator *op, void (*release)(void *));
/* largest vector-arena elements per right-hand side of the operator's plans (what bfhipOperatorReserveRhs allocates per RHS) */
uint64_t bfhipOperatorTempElems(struct BfhipOperator const *op);
/* element size of the operator on the device; 0 for NULL */
uint32_t bfhipOperatorElemSize(struct BfhipOperator const *op);
/* the vtable shim object behind a BfMat of bfhipMatNew / bfhipShardedMatNew: its operator, whether it is transposed and whether
 * it is sharded.  INVALID_ARGUMENTS if `mat` is not a shim object. */
int bfhipShimGet(void const *mat, struct BfhipOperator **op, int *transposed, int *sharded);
void bfhipShimRaise(int code);     /* the reference's bfSetError(code), when forwarding is on and the host process has it */
/* Panel width of a host-vector apply of `nrhs` columns, `perColBytes` device bytes per column, under `budget` bytes:
 * *width = nrhs when the call runs in one piece (nrhs <= 0xffff and nrhs * perColBytes <= budget), else the widest multiple
 * of 64 (<= 0xffff, <= nrhs) that fits; MEMORY_ERROR when not even min(64, nrhs) columns fit.  Host-only. */
int bfhipHostApplyPanelWidth(uint64_t nrhs, uint64_t perColBytes, uint64_t budget, uint64_t *width);

/* block-Jacobi preconditioner (bfhip_precond.c reads the operator through these; none of bfhip_api.c, bfhip_file.c, bfhip_shim.c, bfhip_inspect.c calls it) */
/* the forward plan: host mirrors on a plan-only operator, device tables (dItems, dPieces, reduce d*) otherwise */
BfPlan const *bfhipOperatorPlan(struct BfhipOperator const *op);
void const *bfhipOperatorArena(struct BfhipOperator const *op);    /* leaf arena on the device; NULL for a plan-only operator */

/* bfhip_precond.hip (driven by bfhip_precond.c only -- no file of the host sanitizer harness calls these).
 * Workspace: per block b a row-major m_b x m_b matrix at element wsOff[b] (complex double for complex operands, double for
 * real ones).  Task t of block b (tasks [taskBegin[b], taskBegin[b + 1]), walked in order, one workgroup per block):
 * ws[b](br + r, bc + c) += arena[dataOff + r * ldr + c * ldc] for r < nr, c < nc; an identity task (ldr == ldc == 0) adds 1 at
 * (br + r, bc + r) for r < nr. */
typedef struct BfBjTask {
  uint64_t dataOff;
  uint32_t br, bc, nr, nc;
  uint32_t ldr, ldc;
} BfBjTask;
typedef struct BfBjBlock {
  uint64_t wsOff;
  uint32_t m, taskBegin, taskEnd, pad;
} BfBjBlock;
/* per block of the inversion: status 0 = inverted, 1 = zero or non-finite pivot (the block is left as it is); the smallest
 * |pivot| seen and the largest |B_b(i, j)| */
typedef struct BfBjResult {
  double minPivot, maxAbs;
  uint32_t status, step;
} BfBjResult;
/* srcDtype = the operator's storage dtype; the workspace is complex iff it is complex */
int bfdevBjGather(void *ws, void const *arena, uint64_t arenaElems, uint32_t srcDtype, BfBjBlock const *dBlocks, BfBjTask const *dTasks, uint64_t numBlocks,
                  void *stream);
int bfdevBjInvert(void *ws, int cplx, BfBjBlock const *dBlocks, BfBjResult *dResults, uint64_t numBlocks, void *stream);
/* arena[dataOff + e] of a result piece = ws element (row0 + r, col0 + c) of its block, converted to outDtype (padding: 0) */
typedef struct BfBjFillPiece {
  uint64_t dataOff, wsOff;
  uint32_t m, row0, col0, mr, mrPad, ncols, rowMajor, ld;
} BfBjFillPiece;
int bfdevBjFill(void *arena, uint32_t outDtype, void const *ws, BfBjFillPiece const *dPieces, uint64_t numPieces, void *stream);

#ifdef __cplusplus
}
#endif
#endif
