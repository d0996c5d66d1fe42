/* bfhip.h -- C-ABI of the MI355X butterfly-apply engine (libbfhip.so).
 *
 * One hot path of sampotter/butterfly is replaced: applying an already-built
 * factorization, i.e. `bfMatMul(A, X)` / `bfMatMulVec(A, x)` where A is a
 * `BfMatProduct` / `BfMatBlock{Dense,Diag,Coo}` hierarchy over dense leaves
 * (reference src/mat.c:183-189 dispatching to src/mat_product.c:211-280,
 * src/mat_block_dense.c:512-638, src/mat_block_diag.c:370-456,
 * src/mat_block_coo.c:382-474, src/mat_dense_complex.c:1024-1051,
 * src/mat_dense_real.c:1373-1407, src/mat_identity.c:149-181).
 *
 * Usage mirrors what a cgo/ctypes/C caller of the reference would bind:
 *
 *   BfhipOperator *op;
 *   bfhipCompile(A, NULL, &op);          // walk the BfMat graph once, upload
 *   BfMat *A_hip = bfhipMatNew(op);      // drop-in BfMat: bfMatMul(A_hip, X)
 *   ... or bfhipApply(op, X, ldx, nrhs, Y, ldy) on raw host buffers,
 *   ... or bfhipApplyDevice(op, dX, nrhs, dY, stream) on resident vectors.
 *   bfhipFree(&op);
 *
 * Every function returns 0 (BF_ERROR_NONE) or a reference `enum BfError`
 * value (include/bf/error.h:3-16); nothing in this library aborts.  All
 * pointers are plain C; no torch / HIP types appear in signatures (streams
 * are passed as `void *` = hipStream_t).
 *
 * Thread-safety: as the reference (single host thread per operator).
 */
#ifndef BFHIP_H
#define BFHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct BfhipOperator BfhipOperator;

/* element type of leaves and vectors */
enum {
  BFHIP_C128 = 0,  /* double _Complex: fac_helm2 operands (BfMatDenseComplex) */
  BFHIP_F64 = 1,   /* double: fac_streamer operands (BfMatDenseReal)          */
  BFHIP_F32 = 2,   /* float: build extension -- real leaves demoted on upload */
  BFHIP_C64 = 3    /* float _Complex: build extension -- complex leaves demoted on upload (the real family's plan, complex MACs in double) */
};

/* node kinds of the flat expression descriptor */
enum {
  BFHIP_NODE_DENSE = 0,     /* leaf: rows x cols row-major values          */
  BFHIP_NODE_IDENTITY = 1,  /* leaf: square identity (mat_identity.c:149)   */
  BFHIP_NODE_BLOCK = 2,     /* sum of children placed at (row0, col0)      */
  BFHIP_NODE_PRODUCT = 3    /* F0 * F1 * ... * F_{L-1}, applied right-to-left */
};

enum {
  BFHIP_FLAG_NONE = 0,
  BFHIP_FLAG_PROFILE = 1u << 0,  /* record hipEvents around every stage launch */
  BFHIP_FLAG_PLAN_ONLY = 1u << 1,/* build the host-side plan only: no device is touched, apply is refused;
                                    for inspecting the flattened layout (bfhipPlan* below) */
  BFHIP_FLAG_ADJOINT = 1u << 2,  /* also build the plan of A^T (bfhipApplyTranspose*, RmulVec of the shim):
                                    index metadata only, the packed leaf data is shared */
  BFHIP_FLAG_ADJOINT_PACKED = 1u << 4,  /* as BFHIP_FLAG_ADJOINT, but A^T gets a packed copy of the leaves of its own: the adjoint
                                    plan is then a FORWARD plan of the transposed expression (factors reversed, every leaf
                                    transposed -- what bfMatProductTranspose leaves behind, src/mat_product.c:409-420) and
                                    A^T x runs on the forward kernels at the forward rate, for twice the leaf memory.
                                    Falls back to the shared-leaf plan (BFHIP_FLAG_ADJOINT) with a device value builder (bfhipBuildHelm2: its
                                    values exist in the forward arena only), on a row shard (rowBegin / rowBlockBegin: the shard's adjoint is the
                                    pruned transposed task list) and when the second arena does not fit the device's memory; a plan-only operator
                                    keeps the packed plan (bfhipPlanPackArenaT packs its arena).  bfhipSave / bfhipLoad carry both arenas */
  BFHIP_FLAG_EXACT_COMPLEX = 1u << 5,  /* complex128 operators applied to blocks of right-hand sides (nrhs >= 2, the matrix-core kernels): form
                                    every complex product with its FOUR real multiplications, as cblas_zgemm's recurrence does
                                    (src/mat_dense_complex.c:1704-1765), instead of Gauss's three.  The default is normwise as accurate
                                    (same 1e-12 tolerance against the oracle) but its imaginary part carries a rounding error of
                                    eps * sum (|Ar| + |Ai|)(|Xr| + |Xi|) whatever its own size; with this flag each part's error is
                                    bounded by eps times ITS OWN sum of absolute products (e.g. nearly real data keep a relatively
                                    accurate small imaginary part).  Costs a third more matrix-pipe work (nrhs = 64: ~25 % slower).
                                    One right-hand side (the GEMV kernel) always uses the four-product form */
  BFHIP_FLAG_FLOW = 1u << 3      /* EXPERIMENTAL BUILDS ONLY (libbfhip_exp.so, `make -C butterfly_amd/csrc experimental`): complex128
                                    operators applied to ONE right-hand side run the whole plan as ONE dependency-driven
                                    persistent launch (items wait for the intermediate vectors they read, not for the previous
                                    stage; bit-identical results).  Measured slower than the staged launches on MI355X
                                    (DESIGN_EXPERIMENTS.md section 15).  The product library (libbfhip.so) does not contain that executor
                                    and refuses the flag with BF_ERROR_NOT_IMPLEMENTED */
};
/* Environment variables.  The product library reads six, all test / diagnosis hooks:
 *   BFHIP_JACOBI_GLOBAL=1   builder: every SVD problem through the global-memory fallback kernel (test hook)
 *   BFHIP_JACOBI_QR_MIN=n   builder: least-squares problems of >= n equivalent sources are QR-factored with column pivoting
 *                           before the Jacobi SVD (default 65; 0: every problem, a test hook; a huge value: none)
 *   BFHIP_JACOBI_GRAM_MIN=n builder: least-squares problems of rows + columns >= n run the block form of the Jacobi SVD on Gram matrices
 *                           (default 512; 0: every problem, a test hook; a huge value: none)
 *   BFHIP_JACOBI_PROFILE=1  builder: prints the time of every phase and of every SVD size class to stderr (synchronises per class)
 *   BFHIP_ALLOW_UNCONVERGED_SVD=1   builder: keep an operator whose Jacobi SVDs hit the sweep limit (diagnosis)
 *   BFHIP_GMRES_MGS=1       GMRES: the reference's modified Gram-Schmidt order instead of batched CGS2 (as the per-call option)
 * The experimental build (libbfhip_exp.so) additionally reads, once per process:
 *   BFHIP_FLOW=1            as BFHIP_FLAG_FLOW for every operator compiled in the process
 *   BFHIP_PERSISTENT=1      complex128 stages with more items than wavefront slots run as a persistent grid that draws
 *                           pooled tickets (bfhip_persist.hip; bit-identical results, measured equal to slower)
 *   BFHIP_TIMELINE_FILE=p   every complex128 stage launch (one right-hand side) becomes a synchronous diagnostic launch
 *                           that appends each item's start / end stamps to file p (tools/timeline.py; same results)
 *   BFHIP_FLOW_SPIN, BFHIP_FLOW_DEBUG, BFHIP_FLOW_DEBUGMODE   diagnostics of the one-launch executor */

typedef struct BfhipOptions {
  uint32_t structSize;      /* = sizeof(BfhipOptions) */
  int32_t device;           /* HIP ordinal; -1 = current device */
  uint32_t flags;           /* BFHIP_FLAG_* */
  uint32_t maxRhs;          /* intermediates preallocated for this many RHS (0 -> 1); grows on demand */
  uint32_t demoteToF32;     /* 1: store/compute BFHIP_F64 operands in fp32 and BFHIP_C128 operands in complex64 (BFHIP_C64; config 5
                             * extension).  A complex64 operator's bfhipApplyDevice / bfhipApplyTransposeDevice take complex64 device
                             * vectors (interleaved float re / im); its host entries (bfhipApply, the vtable shim) keep taking complex128.
                             * GMRES and covariance products refuse complex64 (NOT_IMPLEMENTED / TYPE_ERROR); the Helmholtz builders
                             * refuse this field (NOT_IMPLEMENTED) and make complex64 operators through BfhipHelm2Problem.outDtype
                             * or bfhipBuildHelm2Pair (bfhip_build.h); bfhipSolveGMRESRefine[Device] takes one as its inner operator. */
  uint32_t reserved0;
  uint64_t seed;            /* value seed for synthetic (data == NULL) leaves */
  /* row sharding: keep only block rows
   * [rowBlockBegin, rowBlockEnd) of a BLOCK root; rowBlockEnd == 0 -> all.
   * The operator then maps the full x to the concatenation of those rows. */
  uint64_t rowBlockBegin;
  uint64_t rowBlockEnd;
  /* row-range sharding: keep exactly what output rows [rowBegin, rowEnd) depend on (any operand, not only a BLOCK
   * root): leaves no kept row needs are dropped, source-side factors several ranges need are replicated, and the
   * rows produced are bit for bit those of the whole operator when no leaf straddles the range ends (the cuts
   * bfhipRowPartition returns).  rowEnd == 0 -> all rows.  Exclusive with rowBlockBegin/End.  (Fields added in
   * round 3: a caller passing the shorter round-2 struct through structSize gets "all rows".) */
  uint64_t rowBegin;
  uint64_t rowEnd;
} BfhipOptions;
#define BFHIP_OPTIONS_SIZE_V1 48u   /* sizeof(BfhipOptions) before rowBegin / rowEnd */

/* Flat description of an operand: the same expression tree as a BfMat graph,
 * as arrays.  Used (a) internally by bfhipCompile after walking a BfMat graph
 * and (b) directly by callers that synthesize structure-exact operands
 * without ever materializing host values (leafData[i] == NULL: values are
 * generated on the device from `seed`, see bfhipSyntheticValue). */
typedef struct BfhipDesc {
  uint32_t structSize;      /* = sizeof(BfhipDesc) */
  uint32_t dtype;           /* BFHIP_C128 or BFHIP_F64 */
  uint64_t numNodes;
  uint64_t root;
  const uint8_t *kind;          /* [numNodes] BFHIP_NODE_* */
  const uint64_t *rows;         /* [numNodes] element rows */
  const uint64_t *cols;         /* [numNodes] element cols */
  const uint64_t *childBegin;   /* [numNodes+1] CSR into child arrays */
  const uint64_t *childNode;    /* [numChildren] */
  const uint64_t *childRow0;    /* [numChildren] row offset inside parent (BLOCK) */
  const uint64_t *childCol0;    /* [numChildren] col offset inside parent (BLOCK) */
  const void *const *leafData;  /* [numNodes] or NULL; row-major host values */
  const uint64_t *leafRowStride;/* [numNodes] or NULL (-> cols), in elements */
  const uint64_t *topRowBlock;  /* [numChildren of root] or NULL: block-row id of each root child (for sharding) */
  const uint8_t *blockKind;     /* [numNodes] or NULL: reference BfType of BLOCK nodes (15 coo, 16 dense, 17 diag); informative only */
} BfhipDesc;

typedef struct BfhipStats {
  uint32_t structSize;
  uint32_t dtype;
  uint64_t numRows, numCols;
  uint64_t numStages;
  uint64_t numLeaves;        /* dense leaves kept (after sharding) */
  uint64_t numItems;         /* kernel work items over all stages */
  uint64_t numPieces;
  uint64_t leafElems;        /* sum over leaves of m*n */
  uint64_t leafBytes;        /* leafElems * sizeof(element) = algorithmic operand bytes */
  uint64_t vecElemsRead;     /* sum over stages of input elements read once per distinct segment */
  uint64_t vecElemsWritten;  /* sum over stages of output elements */
  uint64_t arenaBytes;       /* device bytes actually held for leaves (incl. padding) */
  uint64_t tempElems;        /* intermediate-vector elements per RHS */
  uint64_t metaBytes;        /* device bytes of index metadata */
} BfhipStats;

/* ---- compile ------------------------------------------------------------- */

/* Walk a reference object graph (read-only; nothing of A is retained) and
 * build the device operator.  `bfMat` is a `BfMat const *` of the reference
 * (layouts: bfhip_abi.h).  Replaces the recursive dispatch the reference does
 * on every bfMatMul call (src/mat.c:183 and callees listed above).
 * Errors: TYPE_ERROR (unknown node type / mixed real+complex),
 * NOT_IMPLEMENTED (a dense leaf flagged CONJ without TRANS; a leaf flagged TRANS is read as the reference multiplies by
 * it: a complex one as its conjugate transpose, mat_dense_complex.c:27-35, 503-511, a real one as its transpose),
 * INVALID_ARGUMENTS (NULL vtable, non-monotone offsets, shape mismatch),
 * MEMORY_ERROR (host or device OOM), RUNTIME_ERROR (HIP failure). */
int bfhipCompile(const void *bfMat, const BfhipOptions *opts, BfhipOperator **out);

/* Same, from a flat descriptor. */
int bfhipCompileDesc(const BfhipDesc *desc, const BfhipOptions *opts, BfhipOperator **out);

/* Balanced contiguous row ranges for `world` ranks: cuts[0] = 0 < ... < cuts[world] = rows, rank r owning rows
 * [cuts[r], cuts[r + 1]) (BfhipOptions.rowBegin/rowEnd).  Cuts fall only where no leaf that writes y straddles them
 * (quadtree node boundaries of a fac_helm2 operand: the level-3 and deeper row blocks inside each level-2 BlockDense,
 * reference src/fac_helm2.c:814-858), and the largest per-rank load -- leaf elements kept, replicated source-side
 * factors included -- is minimised.  `leafElems` [world] may be NULL.  INVALID_ARGUMENTS if the operand offers fewer
 * than `world` ranges.  No device is touched. */
int bfhipRowPartition(const BfhipDesc *desc, uint32_t world, uint64_t *cuts, uint64_t *leafElems);
int bfhipRowPartitionMat(const void *bfMat, uint32_t world, uint64_t *cuts, uint64_t *leafElems);

/* leafElems[v] = sum of rows x cols over the dense leaves under node v, for every node of the descriptor (what
 * bfMatNumBytes / 16 resp. / 8 of that subtree's leaves is): balancing ranks, sampling sub-operators. */
int bfhipDescSubtreeLeafElems(const BfhipDesc *desc, uint64_t *leafElems);

/* ---- apply --------------------------------------------------------------- */

/* Y[numRows x nrhs] = A * X[numCols x nrhs]; host buffers, row-major with
 * leading dimensions ldx/ldy in elements (the layout of BfMatDenseComplex
 * with colStride == 1, mat_dense_complex.h:69-81).  Synchronous. */
int bfhipApply(BfhipOperator *op, const void *X, size_t ldx, size_t nrhs, void *Y, size_t ldy);

/* What bfhipApply (and every slot of the vtable shim) does with X and Y depends on what they are (hipPointerGetAttributes):
 * densely packed (ld == nrhs) double-precision vectors in DEVICE memory of the operator's GPU are used in place, in PINNED or
 * REGISTERED host memory they are the source / target of the DMA itself, anything else is packed through the operator's pinned
 * staging buffer (one more pass over the vector on the CPU, each way).  The library never registers a caller's buffer on its own
 * (it cannot know when the caller frees it); a caller that reuses its vectors -- the Krylov basis of bfSolveGMRES, say --
 * registers them once (hipHostRegister underneath; undo before freeing the memory). */
int bfhipHostRegister(void *p, size_t bytes);
int bfhipHostUnregister(void *p);

/* Same on device-resident, densely packed (ld == nrhs) vectors; enqueued on
 * `stream` (hipStream_t, NULL = default stream) and asynchronous. */
int bfhipApplyDevice(BfhipOperator *op, const void *dX, size_t nrhs, void *dY, void *stream);

/* Y[numCols x nrhs] = A^T X[numRows x nrhs] (plain transpose, no conjugation): what the reference's
 * bfMatRmulVec computes on a BfVecReal (x^T A as a vector: src/mat_product.c:314-345,
 * src/mat_block_diag.c:458-505, src/mat_block_coo.c:476-520, src/mat_block_dense.c:696-758,
 * src/mat_dense_real.c:1508-1542) and what `cov_matvec` needs for Phi^T v
 * (examples/covariance/lbo_cov.c:48-60).  Needs BFHIP_FLAG_ADJOINT at compile. */
int bfhipApplyTranspose(BfhipOperator *op, const void *X, size_t ldx, size_t nrhs, void *Y, size_t ldy);
int bfhipApplyTransposeDevice(BfhipOperator *op, const void *dX, size_t nrhs, void *dY, void *stream);

/* Device bytes bfhipApply / bfhipApplyTranspose / the vtable shim may use for vectors (two staging vectors of the longer side and
 * the vector arena, per right-hand side).  A call that needs more, or has more than 65535 right-hand sides, runs in column panels
 * of the widest multiple of 64 that fits, each packed through the staging buffers (MEMORY_ERROR if not even 64 columns fit).
 * 0 (the default) = automatic: the device's free memory plus what the operator holds for vectors, less 512 MiB, consulted only
 * when a call of more than 64 right-hand sides would grow those buffers.  A call that fits runs in one piece as before. */
int bfhipSetHostApplyBudget(BfhipOperator *op, uint64_t bytes);

/* complex64 operators: forward stages of applies with nrhs >= minRhs run on the block kernels
 * (bfStageKernelC64Mfma*): one launch over all items of the stage, every leaf element loaded once per pass of up to 64
 * right-hand sides (the default kernels load it once per right-hand side), widened exactly to double, contracted on the
 * FP64 matrix cores and rounded to complex64 once at the store -- the element type's contract and error bound are unchanged.
 * 0 = off (the default: every apply runs exactly the kernels it runs today); otherwise minRhs >= 2 (2 is the recommended
 * value: the block path reads the operand once where the default path reads it nrhs times).  Plan, arena, saved file and
 * applies of nrhs < minRhs are untouched; transposed stages and reduces are unchanged.  Results of the block path are
 * deterministic and may differ from the default path's in the last float bit (another summation order).
 * Works on any complex64 operator (compiled, loaded, a complex64 block-Jacobi result, a row shard) and under
 * BFHIP_FLAG_PLAN_ONLY.  Errors: INVALID_ARGUMENTS (NULL operator, minRhs == 1); NOT_IMPLEMENTED for any other element type
 * (complex128 already has block kernels; the real types are not covered by THIS entry: they have bfhipSetRealRhsBlocks). */
int bfhipSetRhsBlocks(BfhipOperator *op, uint32_t minRhs);

/* The same switch for F64 / F32 operators (bfStageKernelRealMfma*), with the same contract: 0 = off (the default), otherwise
 * minRhs >= 2; host-only, works under BFHIP_FLAG_PLAN_ONLY and on compiled, loaded, block-Jacobi-result and row-shard operators.
 * Forward stages of applies with nrhs >= minRhs run one launch over all items: every leaf element is loaded once per pass of up to
 * 64 right-hand sides and contracted on the FP64 matrix cores.  F64: products and sums in double as before, in another order.
 * F32: elements are widened exactly, item sums are accumulated in DOUBLE and rounded to float once at the store (the default F32
 * kernels accumulate in float), so the block path's results meet a tighter bound and differ from the default path's within float
 * rounding.  Transposed stages, reduces, plan, arena and saved file are untouched; results are deterministic.
 * Errors: INVALID_ARGUMENTS (NULL operator, minRhs == 1); NOT_IMPLEMENTED for the complex element types (complex64 has
 * bfhipSetRhsBlocks; complex128 runs block kernels by default). */
int bfhipSetRealRhsBlocks(BfhipOperator *op, uint32_t minRhs);

/* The adjoint's switch, for all four element types and independent of the two forward switches: 0 = off (the default: every
 * apply runs exactly the kernels it runs today), otherwise minRhs >= 2; host-only, works under BFHIP_FLAG_PLAN_ONLY and on
 * compiled, loaded, block-Jacobi-result and row-shard operators.  The stages of the ADJOINT plan of applies with nrhs >= minRhs
 * (bfhipApplyTranspose[Device], the shim's Rmul, bfhipExtract* with BFHIP_EXTRACT_VIA_ADJOINT, bfhipShardedApplyTransposeDevice):
 *   - shared-leaf plan (BFHIP_FLAG_ADJOINT): one launch of bfStageKernelTMfma over all items of the stage, narrow, wide and
 *     shared alike: every leaf element is loaded once per pass of up to 64 right-hand sides (the default kernels walk the item
 *     once per right-hand side) and contracted on the FP64 matrix cores.  F32 / complex64 fragments are widened exactly,
 *     everything accumulates in double and is rounded once at the store; complex products are four real products
 *     (BFHIP_FLAG_EXACT_COMPLEX changes nothing);
 *   - packed plan (BFHIP_FLAG_ADJOINT_PACKED, a forward plan): complex64 / F64 / F32 stages run the forward block kernels
 *     (bfStageKernelC64Mfma*, bfStageKernelRealMfma*); complex128 already does.
 * Plan, arenas, saved file, forward stages and every reduce are untouched; results are deterministic (one owner per output,
 * no atomics) and differ from the default path's within the element type's rounding (another summation order).
 * Errors: INVALID_ARGUMENTS (NULL operator, minRhs == 1, an operator without an adjoint plan). */
int bfhipSetAdjointRhsBlocks(BfhipOperator *op, uint32_t minRhs);

/* ---- dense extraction ------------------------------------------------------ */
/* Entries of the operator, Out[i * ldOut + j] = A[rows[i], cols[j]]: a block A[I, J] (a near-field block, a check against the
 * dense kernel) or, with rows = cols = NULL, the whole matrix (what the reference's bfMatToType densifies, src/mat_product.c:377-407).
 * The operator is applied to panels of `panel` (<= 64) unit vectors and the wanted rows of each result are gathered: the cost is
 * ceil(numCols / panel) applies of `panel` right-hand sides, and the memory is bounded by bfhipExtractWorkspaceBytes whatever the
 * block's size.  With BFHIP_EXTRACT_VIA_ADJOINT the panels run over the ROW set through the adjoint plan (A^T applied to unit
 * vectors; plain transpose, no conjugation: A[I, J] = (A^T)[J, I]), the cheaper route when numRows < numCols.
 *   rows / cols: HOST arrays of uint64 indices (any order, repeats allowed); NULL = all rows (numRows must then equal the
 *                operator's rows), likewise cols.  numRows or numCols == 0: nothing is done.
 * Every argument is checked on the host before anything is enqueued -- INVALID_ARGUMENTS (NULL operator / output, ldOut <
 * numCols, panel > 64, unknown flags, VIA_ADJOINT without BFHIP_FLAG_ADJOINT, a NULL set with the wrong count), OUT_OF_RANGE (an
 * index) -- also on a BFHIP_FLAG_PLAN_ONLY operator, which is then refused (RUNTIME_ERROR).  Sharded operators are not supported. */
typedef struct BfhipExtractOptions {
  uint32_t flags;        /* BFHIP_EXTRACT_VIA_ADJOINT: panels run over the row set through the adjoint plan */
  uint32_t panel;        /* columns per panel, 1..64; 0 = 64 */
} BfhipExtractOptions;
#define BFHIP_EXTRACT_VIA_ADJOINT 1u
/* dOut: DEVICE memory of the operator's GPU, in the operator's compute element type (complex64 / f32 for a demoted operator),
 * numRows rows of ldOut elements.  Setup may synchronise (uploading the indices, growing the workspace and the vector arena);
 * every launch after it goes on `stream`, and the call returns without waiting for them.  Not graph-capturable (unlike
 * bfhipApplyDevice).  `opt` may be NULL (forward route, panels of 64). */
int bfhipExtractDevice(BfhipOperator *op, const uint64_t *rows, size_t numRows, const uint64_t *cols, size_t numCols,
                       void *dOut, size_t ldOut, const BfhipExtractOptions *opt, void *stream);
/* Out: HOST memory, double precision (complex128 or f64, a demoted operator's results promoted as bfhipApply does); synchronous.
 * The copy of one panel's gathered block overlaps the apply of the next; a pinned or registered Out (bfhipHostRegister) of the
 * operator's own element size is the target of the DMA itself, anything else is unpacked from pinned staging on the CPU. */
int bfhipExtract(BfhipOperator *op, const uint64_t *rows, size_t numRows, const uint64_t *cols, size_t numCols,
                 void *Out, size_t ldOut, const BfhipExtractOptions *opt);
/* Device bytes the two entries may hold beyond the operator, with p = the panel width and es = the device element size:
 *   (numRows_A + numCols_A) * p * es        input and result panel
 * + (numRows + numCols) * 8                 index copies
 * + tempElems * p * es                      vector arena at p right-hand sides (BfhipStats.tempElems, both plans)
 * + 2 * g * p * es                          the host entry's two gathered blocks, g = numRows (forward) or numCols (VIA_ADJOINT).
 * Host-only: works on a BFHIP_FLAG_PLAN_ONLY operator.  The workspace is kept on the operator (grown, never shrunk) until bfhipFree. */
int bfhipExtractWorkspaceBytes(const BfhipOperator *op, size_t numRows, size_t numCols, const BfhipExtractOptions *opt, uint64_t *bytes);

/* ---- GMRES (the production caller of the apply path) --------------------- */

/* Solve A X = B with the operator as A, mirroring the reference's
 * bfSolveGMRES(A, B, X0, tol, maxNumIter, &numIter, M = NULL)
 * (src/linalg.c:47-317): unrestarted GMRES, modified Gram-Schmidt, Givens
 * rotations, convergence when max_p |s_{j+1,p}| / max_p ||r_p|| < tol.  The
 * Krylov basis, the work vector, x0 and b stay on the device; only the new
 * Hessenberg column crosses PCIe per iteration.  X0 may be NULL (zeros).
 * `numIter` receives the number of Arnoldi steps, which is the number of
 * basis vectors the solution is built from: j + 1 when the test passes at
 * iteration j (the reference stops one vector short and reports j), maxNumIter
 * when it never does.  `residual` receives the last relative residual; either
 * may be NULL.  Each residual column is scaled by a power of two before its
 * norm is taken, so right-hand sides of any magnitude are solved (b scaled by
 * 2^k gives X scaled by 2^k exactly); a column with a zero residual returns
 * its x0, and a column whose Krylov space is exhausted stops there.  Complex square operators only; the left preconditioner
 * (the reference's M) is the *Precond* entry below.  Host-pointer form: B, X0, X are
 * row-major n x nrhs with leading dimensions in elements. */
int bfhipSolveGMRES(BfhipOperator *op, const void *B, size_t ldb, size_t nrhs, const void *X0, size_t ldx0,
                    double tol, size_t maxNumIter, size_t *numIter, double *residual, void *X, size_t ldx);
/* Device-resident form (densely packed n x nrhs buffers on the operator's
 * GPU, which must be the current device); synchronous on return. */
int bfhipSolveGMRESDevice(BfhipOperator *op, const void *dB, size_t nrhs, const void *dX0, double tol,
                          size_t maxNumIter, size_t *numIter, double *residual, void *dX, void *stream);

/* ---- multi-GPU: one process per GPU, one RCCL collective per apply -------- */
/* The top-level block rows of a factorization are independent (bfMatBlockDenseMul computes each from the
 * full x, src/mat_block_dense.c:534-566), so they shard across the GPUs of a node with no data-path
 * exchange except the closing collective on y.  Each rank compiles the operator of
 * ITS share (BfhipOptions.rowBlockBegin/End, or a descriptor restricted to its blocks) and then:
 *
 *   char id[128]; if (rank == 0) bfhipCommGetUniqueId(id);  ... ship `id` to every rank (MPI, a file, ...)
 *   bfhipCommInitRank(id, nranks, rank, device, &comm);      // ncclCommInitRank
 *   bfhipShardedCreate(op, comm, &spec, maxRhs, &sh);
 *   bfhipShardedApplyDevice(sh, dX, nrhs, dY, stream);       // every rank: x replicated in, FULL y out
 *
 * BFHIP_SHARD_ROWS:   this rank's operator yields the rows of the segments it owns, in global order,
 *                     compacted; the step ends with ONE in-place ncclAllGather (xGMI) and a small kernel
 *                     that puts the segments into global row order in dY.
 * BFHIP_SHARD_BLOCKS: this rank's operator yields a full-length partial y (its (row, col) blocks at
 *                     their original offsets, zeros elsewhere); the step ends with ONE ncclAllReduce.  The
 *                     summation order is RCCL's: equal to one GPU to rounding, not bit for bit (ROWS is).
 * Everything is enqueued on `stream` behind the stage kernels; nothing synchronizes the host.  RCCL is
 * looked up at run time (the copy already in the process, else librccl.so.1); without it these entry
 * points return RUNTIME_ERROR and the rest of the library works.
 * The environment variable BFHIP_RCCL_LIBRARY, read at the first bfhipComm* call of the process, names the collective
 * library by path (a host whose RCCL is not on the default path; a stand-in that exports the same seven nccl* symbols):
 * it is then the ONLY library tried (dlopen RTLD_NOW | RTLD_LOCAL), and a path that cannot be loaded is a RUNTIME_ERROR
 * naming it, as is one that loads but lacks a symbol -- no fallback to librccl.  Unset or empty: the lookup above.
 * Threads: a BfhipSharded / BfhipComm belongs to one thread at a time; different threads may drive DIFFERENT sharded
 * operators (each over its own operator and communicator) concurrently.  The library lookup itself is serialised: the
 * first bfhipComm* calls of a process may come from several threads at once. */
typedef struct BfhipComm BfhipComm;
typedef struct BfhipSharded BfhipSharded;
enum { BFHIP_SHARD_ROWS = 0, BFHIP_SHARD_BLOCKS = 1 };
typedef struct BfhipShardSpec {
  uint32_t structSize;      /* = sizeof(BfhipShardSpec) */
  uint32_t mode;            /* BFHIP_SHARD_* */
  uint64_t numRowsGlobal;   /* rows of the whole operator = length of y */
  uint32_t numSegments;     /* ROWS: row segments of y (top-level block rows, row ranges) */
  uint32_t reserved;
  const uint64_t *segRows;  /* [numSegments] rows of each segment */
  const uint32_t *segOwner; /* [numSegments] rank that computes it */
  /* ROWS, optional (round 3; NULL or a struct of the shorter round-2 size: segments are consecutive in global order,
   * each row computed by exactly one rank).  [numSegments] first global row of each segment.  Several segments may then
   * cover the SAME rows (identical ranges only): ranks that share a block row by columns each send a partial result
   * for it, and after the one all-gather every rank adds the partials of a range in LIST order -- a fixed order, so the
   * result is the same on every rank and from run to run (to rounding the one-GPU result, not bit for bit: that is the
   * price of splitting a row's sum).  A rank's operator yields its segments in list order, compacted. */
  const uint64_t *segGlobalOff;
} BfhipShardSpec;
#define BFHIP_SHARDSPEC_SIZE_V1 40u   /* sizeof(BfhipShardSpec) before segGlobalOff */
int bfhipCommGetUniqueId(void *id128);                                       /* ncclGetUniqueId: 128 bytes */
int bfhipCommInitRank(const void *id128, int nranks, int rank, int device, BfhipComm **out);
void bfhipCommDestroy(BfhipComm **comm);
int bfhipShardedCreate(BfhipOperator *op, BfhipComm *comm, const BfhipShardSpec *spec, uint32_t maxRhs, BfhipSharded **out);
int bfhipShardedApplyDevice(BfhipSharded *sh, const void *dX, size_t nrhs, void *dY, void *stream);
/* hipEvent times of the most recent apply: stage kernels, and collective (+ reordering).  Synchronizes. */
int bfhipShardedLastTimes(BfhipSharded *sh, double *localMs, double *collectiveMs);
/* The three events behind bfhipShardedLastTimes cost ~17 us of stream time per apply (they are what keeps the stage
 * kernels, the collective and the next apply apart): on by default, turn them off for production loops. */
int bfhipShardedSetTiming(BfhipSharded *sh, int enabled);
/* The adjoint of the same step: dZ[numCols x nrhs] = A^T dV[numRowsGlobal x nrhs] on every rank (v replicated in, the FULL z
 * out), what bfMatRmulVec / cov_matvec need at sizes that only fit sharded (reference src/mat_product.c:312-345,
 * src/mat_block_dense.c:696-758).  Rank r holds A_r -- a set of rows (ROWS) or of blocks (BLOCKS) of A -- so it applies A_r^T
 * to ITS entries of v (its segments, gathered into the order its operator produces them) and gets a full-length partial
 * z_r; the partials add up: ONE in-place ncclAllReduce on dZ.  The local operator needs BFHIP_FLAG_ADJOINT (a row-range
 * shard's adjoint plan is the transposed task list pruned by reachability from its rows; BFHIP_FLAG_ADJOINT_PACKED falls
 * back to that shared-leaf plan on a shard).  Sum order is RCCL's: equal to the one-GPU A^T v to rounding. */
int bfhipShardedApplyTransposeDevice(BfhipSharded *sh, const void *dV, size_t nrhs, void *dZ, void *stream);
/* cov_matvec (examples/covariance/lbo_cov.c:48-60) over a sharded real operator, one call: z = P A G G A^T P' v with the
 * sharded adjoint (all-reduce) and the sharded forward step (all-gather) above; arguments as bfhipCovMatvecDevice, every
 * vector replicated on every rank.  Scratch is allocated in bfhipShardedCreate (real operators with an adjoint plan). */
int bfhipShardedCovMatvecDevice(BfhipSharded *sh, const void *dGammaLam, const uint64_t *dRowPerm, const uint64_t *dRevRowPerm,
                                const void *dV, void *dZ, void *stream);
/* bfSolveGMRES (src/linalg.c:47-317) with the sharded step as the matvec: SURVEY 8(f) row 1, "with multi-GPU the allgathered
 * iterate is already replicated".  Every rank calls it with the same (replicated) dB / dX0 and receives the same dX: the
 * Krylov recurrences of bfhipSolveGMRESOptsDevice run redundantly on every GPU, the only communication of an iteration is
 * the step's one collective, and every rank takes the same decisions (they are computed from identical data).  `opt` as
 * for bfhipSolveGMRESOptsDevice; a preconditioner, if any, is a whole (unsharded) operator on this rank's GPU.  Complex
 * square operators. */
struct BfhipGmresOptions;
int bfhipShardedSolveGMRESDevice(BfhipSharded *sh, const struct BfhipGmresOptions *opt, const void *dB, size_t nrhs, const void *dX0,
                                 size_t *numIter, double *residual, void *dX, void *stream);
size_t bfhipShardedGetNumRows(const BfhipSharded *sh);      /* rows of the whole operator */
size_t bfhipShardedGetNumCols(const BfhipSharded *sh);
/* The vtable shim of bfhipMatNew over a SHARDED operator: every rank's host calls bfMatMul / bfMatMulVec / bfMatRmulVec /
 * bfMatTranspose on its copy with the same (replicated) right-hand side and gets the full result (host vectors are staged
 * through device buffers allocated in bfhipShardedCreate).  Delete releases the shim and, if `ownsSharded`, the sharded
 * object (never the operator or the communicator). */
void *bfhipShardedMatNew(BfhipSharded *sh, int ownsSharded);
/* Neither the operator nor the communicator is released.  Order: free the sharded objects of a communicator before
 * bfhipCommDestroy (a sharded object keeps a pointer to it for its steps; freeing itself does not touch it). */
void bfhipShardedFree(BfhipSharded **sh);
/* Failure semantics of a step: arguments are checked and every allocation is made in bfhipShardedCreate (the vector
 * arena for maxRhs included), so a step cannot fail on one rank for a reason the others do not share.  If a launch
 * still fails locally with more than one rank, the communicator is aborted (ncclCommAbort: the peers' collective
 * returns an error instead of hanging), the step returns non-zero and later steps on that communicator are refused. */

/* Left-preconditioned form: the reference's M argument (src/linalg.c:47-49,90-97,131,159).  `solveM` is a device
 * operator that applies what bfMatSolve(M, .) computes, i.e. the action of M^{-1} (n x n, same device and dtype
 * as `op`); NULL = no preconditioner.  As in the reference the residual is then the preconditioned one. */
int bfhipSolveGMRESPrecondDevice(BfhipOperator *op, BfhipOperator *solveM, const void *dB, size_t nrhs, const void *dX0, double tol,
                                 size_t maxNumIter, size_t *numIter, double *residual, void *dX, void *stream);

/* The same solver with its choices per call.  Orthogonalisation: the reference runs modified Gram-Schmidt one basis
 * vector at a time (src/linalg.c:174-184); CGS2 (classical Gram-Schmidt, two batched passes: 7 launches per iteration
 * whatever j is) is equally stable, 20 % faster on the device and may differ from the reference by one iteration;
 * MGS reproduces the reference's H and iteration count.  DEFAULT = CGS2 unless the environment variable
 * BFHIP_GMRES_MGS=1 asks for MGS (an override for hosts that cannot pass options; an explicit choice here wins). */
enum { BFHIP_GMRES_ORTH_DEFAULT = 0, BFHIP_GMRES_ORTH_CGS2 = 1, BFHIP_GMRES_ORTH_MGS = 2 };
typedef struct BfhipGmresOptions {
  uint32_t structSize;          /* = sizeof(BfhipGmresOptions) */
  uint32_t orthogonalization;   /* BFHIP_GMRES_ORTH_* */
  double tol;
  size_t maxNumIter;
  BfhipOperator *solveM;        /* left preconditioner (action of M^{-1}; complex128, n x n, same device) or NULL */
} BfhipGmresOptions;
int bfhipSolveGMRESOptsDevice(BfhipOperator *op, const BfhipGmresOptions *opt, const void *dB, size_t nrhs, const void *dX0,
                              size_t *numIter, double *residual, void *dX, void *stream);

/* Mixed-precision GMRES refinement: complex128 accuracy from mostly complex64 work.  The outer loop computes TRUE residuals
 * r = b - A x with `op` (complex128); each correction A d = r is solved by an inner GMRES (unrestarted, `maxInner` Krylov
 * vectors, from zero, to `innerTol`) that applies only `opLow` (complex64), and x += d.  Each column's correction is solved
 * on r_p / ||r_p||, so every column gains the full inner reduction.  `opLow` may be any complex64 approximation of `op` (the
 * demoteToF32 compile of the same operand is the intended one); it is not checked against `op`, and a worse approximation
 * only converges more slowly.  Stops when max_p ||b_p - A x_p|| / ||b_p|| <= tol (a column with b_p = 0: ||A x_p||), after
 * maxOuter steps, or on stagnation: a step that does not bring that residual below 0.5 x the previous one.  Stagnation and
 * the step cap return 0 with the residual as it is, like bfhipSolveGMRES when it does not converge.  dX receives the iterate
 * of the smallest residual seen (x0 itself if no step improved on it).  A column whose residual is exactly zero keeps its
 * x_p bit for bit.  Every norm is taken of the column scaled by a power of two: b may hold columns of any magnitude
 * whose entries, A x and x are normal finite numbers (2^-600 next to 2^+600 is tested), and b -> 2^k b scales x by 2^k
 * bit for bit.  A NaN in b or x0 gives residual = NaN, no step and rc 0.  Outputs (each may be NULL): numOuter =
 * refinement steps taken, numInner = inner iterations summed over the steps, residual = the true relative residual of
 * dX, history = maxOuter + 1 doubles: the residual of x0, then of each step's iterate (entries past numOuter: NaN).
 * Types: `op` complex128 and `opLow` complex64 (TYPE_ERROR otherwise), both n x n on one device; dB, dX0 (NULL =
 * zeros) and dX complex128 row-major n x nrhs as for bfhipSolveGMRESDevice.  Every argument is checked before the
 * operator's device is (plan-only operators reach each refusal).  `opLow` may also come from the
 * Helmholtz builder (outDtype = BFHIP_C64); bfhipBuildHelm2Pair makes `op` and `opLow` from one value build. */
typedef struct BfhipGmresRefineOptions {
  uint32_t structSize;          /* = sizeof(BfhipGmresRefineOptions) */
  uint32_t orthogonalization;   /* inner GMRES: BFHIP_GMRES_ORTH_* (as BfhipGmresOptions) */
  double tol;                   /* outer: max_p ||b_p - A x_p|| / ||b_p|| <= tol, A = `op`; > 0 */
  double innerTol;              /* relative tolerance of each correction solve; 0 = 1e-6 */
  size_t maxOuter;              /* refinement steps, > 0 */
  size_t maxInner;              /* Krylov vectors per correction solve, > 0 */
  BfhipOperator *solveM;        /* inner left preconditioner (action of M^{-1}, n x n, complex64 or complex128) or NULL */
} BfhipGmresRefineOptions;
int bfhipSolveGMRESRefineDevice(BfhipOperator *op, BfhipOperator *opLow, const BfhipGmresRefineOptions *opt, const void *dB, size_t nrhs,
                                const void *dX0, size_t *numOuter, size_t *numInner, double *residual, double *history, void *dX,
                                void *stream);
/* Host-array form (row-major with leading dimensions in elements, like bfhipSolveGMRES); runs on the default stream. */
int bfhipSolveGMRESRefine(BfhipOperator *op, BfhipOperator *opLow, const BfhipGmresRefineOptions *opt, const void *B, size_t ldb, size_t nrhs,
                          const void *X0, size_t ldx0, size_t *numOuter, size_t *numInner, double *residual, double *history, void *X,
                          size_t ldx);

/* ---- block-Jacobi preconditioner ------------------------------------------ */
/* A preconditioner made on the device from the operator itself, for `solveM` of the GMRES entries above (the reference's
 * production caller assembles the same kind: examples/multiple_scattering/multiple_scattering_context.c:544-606).
 *
 * The direct part A_dir of a SQUARE operator is the sum of the terms that map x to y within one stage of its compiled plan:
 * pieces that read x and either write y or write a vector-arena slot that a reduce of the same stage sums into y.  Identity
 * leaves count as identity entries.  The factors of a product never qualify (its first factor writes an intermediate, its
 * last reads one), so product contributions inside a diagonal block are LEFT OUT: this is a near-field preconditioner.  On a
 * fac_helm2 operand with leaf-aligned blocks nothing is left out (products couple only well-separated boxes), and the
 * gathered block B_b = A_dir[D_b, D_b] equals A[D_b, D_b], the folded decorations (self value, KR correction, column
 * weights) included.  The values are read from the operator's device plan tables and leaf arena, so operators from
 * bfhipCompile, bfhipCompileDesc, the device builders and bfhipLoad all work, with no host values and no applies.
 *
 * Blocks D_b = [cuts[b], cuts[b + 1]) partition [0, n).  Automatic cuts: the direct pieces whose rectangle meets the diagonal
 * are merged, row range with column range, into connected intervals (identity pieces cover only their diagonal entries);
 * on a fac_helm2 operand these are exactly the leaf boxes of the quadtree.  A row no such piece covers is its own 1 x 1
 * block (its direct diagonal entry is zero; it is taken as 1, so M = 1 there) and is counted in `uncoveredRows`; an uncovered
 * row inside a caller's block gets the same 1 on its diagonal.  An interval longer than maxBlock is refused
 * (INVALID_ARGUMENTS: pass cuts), never split.
 *
 * The result M = blockdiag(B_b^{-1}) (or blockdiag(B_b) with BFHIP_BJ_NO_INVERT) is an ordinary operator: a BlockDiag of dense
 * leaves, applied, saved, loaded and described like any other.  The inverses are EXPLICIT (batched Gauss-Jordan with partial
 * pivoting in double / complex double, ties to the smaller row), unlike the reference's LU solves (bfLuSolve): the
 * preconditioner runs on the stage kernels, and its rounding differs from an LU solve's.  Repeated builds are bit-identical.
 *
 * Errors: INCOMPATIBLE_SHAPES (a non-square operator, a row shard included), INVALID_ARGUMENTS (NULL pointers, unknown
 * flags, maxBlock > 256, cuts that are not strictly increasing from 0 to n or have a block over maxBlock, an automatic
 * interval over maxBlock), TYPE_ERROR (an outDtype the operator's dtype cannot be demoted to), NOT_IMPLEMENTED
 * (bfhipBlockJacobi on a BFHIP_FLAG_PLAN_ONLY operator, after every check above), RUNTIME_ERROR (a block with a zero or
 * non-finite pivot, with a pivot whose reciprocal is not finite -- a subnormal pivot such as 2^-1074 -- or with a non-finite
 * entry in a scaled pivot row; the inversion kernel tests each at the step it occurs and the message names block and step:
 * info.firstSingularBlock is set and no operator is made), MEMORY_ERROR.  Sharded operators are not supported; blocks are
 * contiguous and at most 256 rows. */
#define BFHIP_BJ_NO_INVERT 1u
#define BFHIP_BJ_MAX_BLOCK 256u
typedef struct BfhipBlockJacobiOptions {
  uint32_t structSize;     /* = sizeof(BfhipBlockJacobiOptions) */
  uint32_t flags;          /* BFHIP_BJ_NO_INVERT: M = blockdiag(B_b) itself */
  uint32_t maxBlock;       /* 0 -> 128; <= 256 */
  uint32_t outDtype;       /* 0 -> op's dtype; BFHIP_C64 from a complex128 op (inner preconditioner of the refinement), BFHIP_F32 from f64 */
  const uint64_t *cuts;    /* [numBlocks + 1] or NULL = automatic */
  uint64_t numBlocks;
  int32_t device;          /* of the result; -1 = op's */
  uint32_t maxRhs;         /* of the result, as BfhipOptions */
} BfhipBlockJacobiOptions;
typedef struct BfhipBlockJacobiInfo {
  uint32_t structSize, reserved;   /* structSize = sizeof(BfhipBlockJacobiInfo) */
  uint64_t numBlocks, maxBlockRows, uncoveredRows;
  int64_t firstSingularBlock;      /* -1 if none */
  double minPivotRel;              /* min over blocks of |pivot| / max |B_b| */
  double gatherSeconds;            /* plan tables downloaded, block lists built, blocks gathered */
  double invertSeconds;            /* the batched inversion (0 with BFHIP_BJ_NO_INVERT) */
  double compileSeconds;           /* the result compiled and filled */
} BfhipBlockJacobiInfo;
/* The automatic cuts: cuts[0..numBlocks] (at most `cap` entries are written; *numBlocks is set whenever the partition
 * exists).  maxBlock 0 -> 128.  Host-only on a BFHIP_FLAG_PLAN_ONLY operator (its plan's host mirrors); a device operator's
 * plan tables are downloaded. */
int bfhipBlockJacobiPartition(const BfhipOperator *op, uint32_t maxBlock, uint64_t *cuts, uint64_t cap, uint64_t *numBlocks);
/* *pre = the preconditioner (freed with bfhipFree); `opt` may be NULL (automatic cuts, inverses, op's dtype and device);
 * `info` may be NULL.  Synchronous; the workspace (sum of m_b^2 elements in double precision) is released before returning. */
int bfhipBlockJacobi(BfhipOperator *op, const BfhipBlockJacobiOptions *opt, BfhipOperator **pre, BfhipBlockJacobiInfo *info);

/* ---- introspection ------------------------------------------------------- */
int bfhipGetStats(const BfhipOperator *op, BfhipStats *stats);
size_t bfhipGetNumRows(const BfhipOperator *op);
size_t bfhipGetNumCols(const BfhipOperator *op);
/* same meaning as bfMatNumBytes on the original graph: leaf payload bytes
 * (mat_block_coo.c:238-258, mat_dense_complex.c:452-455). */
size_t bfhipNumBytes(const BfhipOperator *op);

/* Whether applies of one right-hand side run as one dependency-driven launch (see BFHIP_FLAG_FLOW), and whether
 * one of its waits ever gave up (0 by construction; checked by the test-suite after every flow test). */
int bfhipFlowStatus(BfhipOperator *op, uint32_t *enabled, uint32_t *waitGaveUp);

/* With BFHIP_FLAG_PROFILE: per-stage accumulated kernel time (ms) and launch
 * count since the last reset, measured with hipEvents on the apply stream.
 * `ms`/`launches`/`bytes` are [numStages] arrays (any may be NULL); `bytes`
 * receives the algorithmic bytes one launch of that stage moves for the nrhs
 * of the last apply.  Synchronizes the stream.  An operator whose applies run as ONE launch (bfhipFlowStatus)
 * reports that launch under stage 0 -- time, launch count and the bytes of all stages -- and zeros elsewhere. */
int bfhipGetStageProfile(BfhipOperator *op, double *ms, uint64_t *launches, uint64_t *bytes, int reset);
/* Bracket only one apply in `every` with events (default 1: all of them).  An event pair per launch costs ~4 us of
 * stream time on this hardware (launch gaps of 10 us instead of 6, measured with rocprofv3 --kernel-trace): 2.5 % of
 * an N = 65536 apply, 0.3 % of the headline one.  The sampled launches are timed exactly as before. */
int bfhipSetProfileSampling(BfhipOperator *op, uint32_t every);

/* ---- covariance products: the caller of the real path ------------------------ */
/* examples/covariance/lbo_cov.c:36-60 wraps the streamed butterfly Phi (N x J) in two products, both called in loops:
 *   sample_z:    z = P Phi GammaLam w                         (MulVec, MulVec, bfVecPermute)
 *   cov_matvec:  z = P Phi GammaLam GammaLam Phi^T P' v       (bfVecPermute, RmulVec, MulVec x3, bfVecPermute)
 * with GammaLam a BfMatDiagReal (its J diagonal entries are passed here) and P, P' = bfVecRealPermute with rowPerm /
 * revRowPerm, which SCATTERS: out[perm[i]] = in[i] (src/vec_real.c:312-329).  Through the vtable shim every step is a
 * host vector (two PCIe round trips per product); these entries keep everything on the device, on `stream`:
 * permute, A^T, scale, A, permute.  dGammaLam [numCols] in the operator's element type (NULL: identity), perms
 * uint64 [numRows] (= BfPerm.index; NULL: identity), dW [numCols], dV and dZ [numRows].  Real operators only
 * (TYPE_ERROR otherwise); bfhipCovMatvecDevice needs BFHIP_FLAG_ADJOINT. */
int bfhipCovSampleDevice(BfhipOperator *op, const void *dGammaLam, const uint64_t *dRowPerm, const void *dW, void *dZ, void *stream);
int bfhipCovMatvecDevice(BfhipOperator *op, const void *dGammaLam, const uint64_t *dRowPerm, const uint64_t *dRevRowPerm,
                         const void *dV, void *dZ, void *stream);

/* ---- batched covariance sampling ------------------------------------------------ */
/* lbo_cov.c:219-225 draws numSamples samples one after another, each from a fresh bfVecRealNewRandn, then evaluates covariance
 * columns with cov_matvec.  These entries are that loop in blocks, resident on the device.  All vectors are row-major
 * rows x nrhs, densely packed (the layout of bfhipApplyDevice); P and P' scatter whole rows: out[perm[i], :] = in[i, :].
 *
 * Block products: column q of the result is what the single-vector entry computes for column q of the input -- the same
 * sequence with nrhs right-hand sides through every step (sample: scale, A, scatter; matvec: scatter, A^T, scale twice, A,
 * scatter).  Which stage kernels run is decided by the operator's switches (bfhipSetRealRhsBlocks, bfhipSetAdjointRhsBlocks)
 * and nothing else: off (the default), a column equals the single-vector result to rounding (bit for bit at nrhs = 1); on,
 * the leaves are read once per pass of 64 columns.  dW [numCols x nrhs], dV and dZ [numRows x nrhs]; 1 <= nrhs <= 65535.
 * The scratch (2 x the longer side x nrhs elements) grows on demand; growing is not stream-ordered and drains `stream`
 * first (as growing the vector arena does).  A call that grows nothing only enqueues work and can be captured in a graph. */
int bfhipCovSampleBlockDevice(BfhipOperator *op, const void *dGammaLam, const uint64_t *dRowPerm, const void *dW, size_t nrhs, void *dZ,
                              void *stream);
int bfhipCovMatvecBlockDevice(BfhipOperator *op, const void *dGammaLam, const uint64_t *dRowPerm, const uint64_t *dRevRowPerm,
                              const void *dV, size_t nrhs, void *dZ, void *stream);

/* Standard normals without a host: value `idx` of the normal stream for `seed` (= bfhip_normal_value, include/bfhip_synth.h:
 * Box-Muller over two counters of the synthetic stream; one normal per index, independent of every other index).  The device
 * evaluates the same formula in double and rounds once for F32; host and device agree to the accuracy of log / cos (within
 * 8 ulp of double), not bit for bit.  bfhipFillNormalDevice: d[i] = N(seed, firstIdx + i), i < count, on the current device;
 * dtype BFHIP_F64 or BFHIP_F32 (TYPE_ERROR otherwise). */
double bfhipNormalValue(uint64_t seed, uint64_t idx);
int bfhipFillNormalDevice(void *d, uint64_t count, uint64_t firstIdx, uint32_t dtype, uint64_t seed, void *stream);

/* Draw: dZ[:, s] = P A GammaLam w_s for s < nrhs with w_s[j] = N(seed, (firstSample + s) * numCols + j), generated on the
 * device (already scaled) in one kernel; the rest is bfhipCovSampleBlockDevice.  The normals of a sample depend on
 * (seed, firstSample + s) alone: calls with (firstSample, nrhs) = (0, a) and (a, b) use bit for bit the W of one call (0, a + b).
 *
 * Moments: samples firstSample .. firstSample + numSamples - 1, `batch` at a time (0 -> 64, at most 64; the last batch may
 * be shorter), WITHOUT storing them: per row i of each batch's un-permuted result T the sums over its columns of T[i, q] and
 * of T[i, q]^2 are formed in double (F32 values widened exactly) and ADDED to dSum[perm[i]] / dSumSq[perm[i]] (double
 * [numRows] each; either may be NULL, not both; the caller zeroes them before the first call): mean = sum / K and
 * var = sumSq / K - mean^2 after K samples.  One thread owns each output row, the order of every sum is fixed, no atomics:
 * results are identical from run to run.  dRowPerm must be a permutation (an index >= numRows is dropped; a repeated one
 * would lose updates).
 *
 * Errors of the six entries, all raised before the device is touched: INVALID_ARGUMENTS (a NULL operator, input or output;
 * nrhs == 0 or > 65535; batch > 64; numSamples == 0; both moment outputs NULL; matvec on an operator without
 * BFHIP_FLAG_ADJOINT), TYPE_ERROR (a complex operator; a fill dtype that is not real), then RUNTIME_ERROR for a
 * BFHIP_FLAG_PLAN_ONLY operator. */
int bfhipCovDrawDevice(BfhipOperator *op, const void *dGammaLam, const uint64_t *dRowPerm, uint64_t seed, uint64_t firstSample,
                       size_t nrhs, void *dZ, void *stream);
int bfhipCovMomentsDevice(BfhipOperator *op, const void *dGammaLam, const uint64_t *dRowPerm, uint64_t seed, uint64_t firstSample,
                          uint64_t numSamples, uint32_t batch, double *dSum, double *dSumSq, void *stream);

/* ---- conditioning on observations ------------------------------------------------ */
/* Kriging means and posterior samples of the field z = P A GammaLam w given k <= BFHIP_COND_MAX_OBS noisy point values
 * y_a = z[obs[a]] + e_a, e_a ~ N(0, noiseVar[a]), by a direct solve (Matheron's rule in coefficient space).  With
 *   B [k x n]   the observed rows of P A GammaLam:  B[a, j] = A[i_a, j] * gamma[j],  dRowPerm[i_a] = obs[a]  (no perm: i_a = obs[a])
 *   G = B B^T,  D = diag(noiseVar),  L L^T = G + D  (Cholesky, double)
 * a block of q samples is
 *   R  = y 1^T - B W - E            [k x q], double; y is shared by the columns
 *   alpha = (G + D)^-1 R            two triangular solves with L
 *   W' = W + B^T alpha              [n x q]: summed in double, rounded once to the operator's element type
 *   Z  = P A GammaLam W'            bfhipCovSampleBlockDevice's sequence: one apply a pass
 * Z[:, s] is a posterior sample when W[:, s] is standard normal and E[a, s] = sqrt(noiseVar[a]) N(0, 1); W = 0, E = 0 gives
 * the posterior mean.
 *
 * Create: real operators with BFHIP_FLAG_ADJOINT.  `op`, dGammaLam (operator dtype, [numCols], NULL: ones) and dRowPerm
 * (NULL: identity) are referenced, not copied: the caller keeps them alive and unchanged, as for every covariance entry.
 * obs [numObs] (host) index the output z, distinct, < numRows; noiseVar [numObs] (host, >= 0, finite; NULL: zeros).  B^T is
 * formed by bfhipApplyTransposeDevice on panels of <= 64 unit columns (the adjoint switch of the operator decides the
 * kernels), widened exactly, multiplied by gamma in double and kept as an n x k double matrix, also for F32 operators.
 * dRowPerm is inverted on the device and must hit every observed index exactly once (INVALID_ARGUMENTS otherwise).
 * Everything a later call needs is allocated here for passes of 64 columns (the operator's covariance scratch and vector
 * arena are grown to 64 columns too): a later call only enqueues work on `stream`.  Create is synchronous: it returns after
 * the factorization.  A Cholesky pivot (the value under the root) that is <= 0 or not finite gives RUNTIME_ERROR naming
 * the step (the index of the pivot); *out stays NULL and everything is released.
 * Free: drains the whole device first (work enqueued on any stream may still read the object's matrices), then releases what
 * the object holds.  Free it BEFORE its operator: every other entry reads the operator through the object, and an object whose
 * operator is gone may only be freed.
 *
 * SampleBlock: dY [k] double, dW [n x nrhs] operator dtype, dEps [k x nrhs] double (NULL: zeros), dZ [m x nrhs] operator
 * dtype, dAlpha [k x nrhs] double (NULL: not wanted); all device, row-major, densely packed.  nrhs > 64 runs in passes of 64
 * columns.  Mean: the same with W = 0, E = 0, one column, bit for bit.
 * Draw: W[j, s] = N(seed, (firstSample + s) n + j) (not scaled: the block sample applies GammaLam) and
 * E[a, s] = sqrt(noiseVar[a]) N(noiseSeed, (firstSample + s) k + a), the product formed in double: bit for bit SampleBlock
 * on the blocks bfhipFillNormalDevice makes with those indices.  The normals of a sample do not depend on the call or batch
 * it is drawn in.
 * Moments: bfhipCovMomentsDevice's loop over conditioned draws (batch 0 -> 64, at most 64), added to dSum / dSumSq.
 *
 * Errors, raised before the device is touched, in this order: INVALID_ARGUMENTS (NULL operator / object, output or dY;
 * numObs == 0 or > BFHIP_COND_MAX_OBS; a repeated observed index; a noiseVar entry negative or not finite; nrhs == 0 or
 * > 65535; both moment outputs NULL; batch > 64; numSamples == 0), OUT_OF_RANGE (an observed index >= numRows), TYPE_ERROR
 * (a complex operator), INVALID_ARGUMENTS (no BFHIP_FLAG_ADJOINT; more than 65535 x 1024 columns, the per-pass kernels' grid),
 * RUNTIME_ERROR (a BFHIP_FLAG_PLAN_ONLY operator).  The
 * entries that take a BfhipCovCond read nothing through it before their own arguments are checked.  Sharded operators are
 * not supported. */
typedef struct BfhipCovCond BfhipCovCond;
#define BFHIP_COND_MAX_OBS 2048u
typedef struct BfhipCovCondInfo {
  uint32_t structSize;            /* in: sizeof(BfhipCovCondInfo) */
  uint32_t numObs;
  double minPivot, maxPivot;      /* smallest and largest Cholesky pivot: the values under the roots */
  uint64_t setupApplies;          /* adjoint panel applies of Create */
  uint64_t factorBytes;           /* device bytes the object holds: B^T, L and the per-pass blocks */
  double rowsSeconds, gramSeconds, factorSeconds;   /* setup phases: rows of B (inverse permutation, panels, pack), Gram, Cholesky */
} BfhipCovCondInfo;

int bfhipCovCondCreate(BfhipOperator *op, const void *dGammaLam, const uint64_t *dRowPerm, const uint64_t *obs, size_t numObs,
                       const double *noiseVar, BfhipCovCond **out, void *stream);
void bfhipCovCondFree(BfhipCovCond **c);
int bfhipCovCondGetInfo(const BfhipCovCond *c, BfhipCovCondInfo *info);
int bfhipCovCondSampleBlockDevice(BfhipCovCond *c, const double *dY, const void *dW, const double *dEps, size_t nrhs, void *dZ,
                                  double *dAlpha, void *stream);
int bfhipCovCondMeanDevice(BfhipCovCond *c, const double *dY, void *dMean, double *dAlpha, void *stream);
int bfhipCovCondDrawDevice(BfhipCovCond *c, const double *dY, uint64_t seed, uint64_t noiseSeed, uint64_t firstSample, size_t nrhs,
                           void *dZ, void *stream);
int bfhipCovCondMomentsDevice(BfhipCovCond *c, const double *dY, uint64_t seed, uint64_t noiseSeed, uint64_t firstSample,
                              uint64_t numSamples, uint32_t batch, double *dSum, double *dSumSq, void *stream);

/* Log marginal likelihood of the observations with its gradients, and exact kriging variances.  Both come from what the
 * object already holds (B^T and L) and from one kernel: the column sums of squares of L^-1 S for a wide S that is never
 * stored, a workgroup running the whole forward substitution for a strip of 64 columns in a k x 64 strip of scratch of its
 * own.  Everything is double, for F32 operators too (rows widened exactly and multiplied by gamma in double, as in Create).
 * One owner per output, every sum in a fixed order that depends on (n, k) alone, no atomics: a second call gives the same
 * bits, whatever the workspace.
 *
 * LogLikelihood: y ~ N(0, K), K = G + D.  dValue[3] = { logLik, quad, logDet }.  The gradients are with respect to the
 * log of every spectral weight and to every noise variance, at fixed observed rows: a caller with a parametric
 * gamma(lambda; theta) finishes by the chain rule.  A zero weight gives exactly +0.  workspaceBytes (0: as many strips as
 * S = B^T has, at most 256 MiB) sets how many workgroups run at once: workspaceBytes / (numObs * 64 * 8).  The first call
 * and a call with a larger workspace allocate; that is not stream-ordered and drains `stream` first; a later call with the
 * same or a smaller workspace only enqueues work.
 * Variance: of the latent field at the output indices query[] (the noise of a new measurement is not added), in panels of
 * <= 64 indices: bfhipApplyTransposeDevice on unit columns (the operator's adjoint switch decides the kernels, as in
 * Create), the pack into double, B r and the strip solve.  The call uploads the indices, inverts dRowPerm for them on the
 * device (a permutation that does not hit every query index exactly once: INVALID_ARGUMENTS) and returns after its work on
 * `stream` is done.
 * A re-fit at new weights means a new bfhipCovCondCreate: the stored rows are pre-scaled.
 *
 * Errors, raised before the device is touched, in this order: INVALID_ARGUMENTS (NULL object, dY or dValue; NULL query,
 * numQuery == 0, both variance outputs NULL, a repeated query index; a structSize that is not the struct's; a non-zero
 * workspaceBytes below one strip, numObs * 64 * 8), OUT_OF_RANGE (a query index >= numRows).  Nothing is read through the
 * object before the checks that need only the arguments (all but the last two).  bfhipCovCondFree releases the workspaces;
 * BfhipCovCondInfo.factorBytes keeps reporting what Create allocated. */
typedef struct BfhipCovCondLikOptions {
  uint32_t structSize;      /* = sizeof(BfhipCovCondLikOptions) */
  uint32_t reserved;
  uint64_t workspaceBytes;  /* strip scratch of the wide solve; 0 -> default */
} BfhipCovCondLikOptions;

/* dValue[3] (device, double) = { logLik, quad = y^T K^-1 y, logDet = 2 sum_a log L[a,a] },
 * logLik = -quad/2 - logDet/2 - (k/2) log(2 pi).
 * dGradLogGamma [numCols] (device, double, may be NULL): d logLik / d log gamma_j = u_j^2 - ||L^-1 b_j||^2,
 *   u = Bt alpha, alpha = K^-1 y, b_j = row j of Bt (= gamma_j * Phi[obs rows, j]).
 * dGradNoise [numObs] (device, double, may be NULL): d logLik / d noiseVar[a] = (alpha_a^2 - ||L^-1 e_a||^2) / 2. */
int bfhipCovCondLogLikelihoodDevice(BfhipCovCond *c, const double *dY, double *dValue, double *dGradLogGamma,
                                    double *dGradNoise, const BfhipCovCondLikOptions *opt, void *stream);

/* query [numQuery] (HOST): indices of the output z, distinct, < numRows, any order.
 * dPrior / dPost [numQuery] (device, double, either may be NULL, not both):
 *   dPrior[t] = ||r||^2, dPost[t] = ||r||^2 - ||L^-1 (Bt^T r)||^2,  r = row of P A GammaLam at query[t]
 * (latent field: the noise of a new measurement is not added). */
int bfhipCovCondVarianceDevice(BfhipCovCond *c, const uint64_t *query, size_t numQuery, double *dPrior, double *dPost,
                               void *stream);

/* ---- matrix-free Chebyshev covariance on a sparse operator ------------------------ */
/* examples/covariance/cheb_cov.c reaches the covariance of the butterfly route without eigenpairs: with the P1 stiffness
 * matrix L of a triangle mesh and its lumped mass, S = D L D, D = diag(massLumped)^-1/2, and a Chebyshev interpolant p of
 * the spectral density on [0, lamMax],
 *   chebmul:     x = p(S) w
 *   sample_z:    z = D p(S) w
 *   cov_matvec:  z = D p(S) p(S) D v
 * These entries keep S (CSR, folded once on the host) and everything else on one device and work on blocks: vectors are
 * row-major n x q, densely packed, double; the output is in mesh order (no permutation).  Real double precision only.
 *
 * The device evaluates p(S) W by Clenshaw's recurrence, one launch of one kernel per degree (bfChebStepKernel):
 *   b_k = c_k W + (4 / lamMax) S b_{k+1} - 2 b_{k+1} - b_{k+2},  k = order - 1 .. 1,  b_order = b_{order+1} = 0
 *   x   = c_0 W + (2 / lamMax) S b_1 - b_1 - b_2
 * with b_k written over b_{k+2}; D on either side is fused into the first / last step.  A row's sum runs over its
 * nonzeros in CSR order by fma and every output row has one owner: column j of a result does not depend on q, and a
 * second call gives the same bits.  Workspace: two blocks of n x q doubles (apply, sample), three (matvec, draw,
 * moments); it grows on demand, which is not stream-ordered and drains `stream` first; a call that grows nothing only
 * enqueues work and can be captured in a graph.
 *
 * Create (host CSR arrays of the symmetric positive semidefinite L; massLumped [n] positive, NULL: ones): the scaling is
 * folded as S[i][j] = (d[i] * L[i][j]) * d[j], d[i] = 1 / sqrt(massLumped[i]).  lamMax must be an UPPER BOUND of the
 * spectrum of S (an underestimate makes the recurrence diverge); lamMax <= 0 asks for the Gershgorin bound
 * max_i sum_j |S[i][j]|, summed in row order.  Empty rows are legal.  Raised before the device is touched, all
 * INVALID_ARGUMENTS: a NULL pointer, n == 0 or n >= 2^32, rowptr[0] != 0, rowptr not monotone, a column index >= n, a
 * massLumped entry that is not finite or <= 0, lamMax NaN or infinite (and a bound that is not positive: S == 0).
 * SetCoefficients: coef[0 .. order - 1] of p in the Chebyshev basis of [0, lamMax] (bfhipChebFit with a = 0, b = lamMax),
 * copied; order >= 1, every coefficient finite.  GetInfo: errorEstimate = |coef[order - 1]| (bfChebStdGetErrorEstimate).
 * Free drains the device, then releases everything. */
typedef struct BfhipChebCov BfhipChebCov;
typedef struct BfhipChebCovInfo {
  uint32_t structSize;            /* in: sizeof(BfhipChebCovInfo) */
  uint32_t reserved;
  uint64_t n, nnz;
  double lamMax;                  /* as given, or the Gershgorin bound */
  uint64_t order;                 /* 0 before bfhipChebCovSetCoefficients */
  uint64_t deviceBytes;           /* rowptr, colind, values of S and d */
  uint64_t workspaceBytes;        /* the blocks of the recurrence, as grown so far */
  double errorEstimate;           /* |coef[order - 1]|; 0 before bfhipChebCovSetCoefficients */
} BfhipChebCovInfo;

int bfhipChebCovCreate(int device, uint64_t n, const uint64_t *rowptr, const uint64_t *colind, const double *data,
                       const double *massLumped, double lamMax, BfhipChebCov **out);
int bfhipChebCovSetCoefficients(BfhipChebCov *c, const double *coef, size_t order);
void bfhipChebCovFree(BfhipChebCov **c);
int bfhipChebCovGetInfo(const BfhipChebCov *c, BfhipChebCovInfo *info);

/* Chebyshev interpolation on [a, b], host only: coef[0 .. order - 1] of the interpolant of f at the `order` points
 * t_i = (b - a) (x_i + 1) / 2 + a, x_i = sin(pi (2 i + 1 - order) / (2 order)):  c_0 = (1 / order) sum_j y_j,
 * c_k = (2 / order) sum_j T_k(x_j) y_j.  Eval: Clenshaw at (2 x - a - b) / (b - a); NaN for order == 0 or NULL coef.
 * INVALID_ARGUMENTS: order == 0, NULL f or coef, a or b not finite, a == b. */
int bfhipChebFit(size_t order, double a, double b, double (*f)(double, void *), void *ctx, double *coef);
double bfhipChebEval(size_t order, double a, double b, const double *coef, double x);

/* The P1 (cotangent) stiffness matrix of a triangle mesh in CSR and its lumped mass, host only.  verts [numVerts x 3],
 * faces [numFaces x 3] vertex indices.  A row holds the vertex's neighbours in increasing order with the vertex itself
 * inserted at its place (the layout of bfTrimeshGetLboFemDiscretization): nnz = numVerts + 2 x (number of edges), which
 * Count reports.  L[i][j] = -(cot a + cot b) / 2 over the angles opposite edge (i, j), L[i][i] = -sum_j L[i][j];
 * massLumped[i] = a third of the area of the triangles at i.  rowptr [numVerts + 1], colind and Ldata [nnz], massLumped
 * [numVerts] (may be NULL).  INVALID_ARGUMENTS: a NULL pointer, numVerts == 0, a face index >= numVerts, a face with a
 * repeated vertex or zero area. */
int bfhipTrimeshLboFemCount(uint64_t numVerts, uint64_t numFaces, const uint64_t *faces, uint64_t *nnz);
int bfhipTrimeshLboFem(uint64_t numVerts, const double *verts, uint64_t numFaces, const uint64_t *faces, uint64_t *rowptr,
                       uint64_t *colind, double *Ldata, double *massLumped);
/* The P1 consistent mass on the pattern bfhipTrimeshLboFem produced (rowptr, colind: inputs), host only: per triangle of area A
 * M[i][i] += A / 6 and M[i][j] += A / 12 (the M of bfTrimeshGetLboFemDiscretization), so every row sums to massLumped[i].  Mdata
 * [nnz].  Arguments are checked as bfhipTrimeshLboFem checks them, with the same codes. */
int bfhipTrimeshLboFemMass(uint64_t numVerts, const double *verts, uint64_t numFaces, const uint64_t *faces, const uint64_t *rowptr,
                           const uint64_t *colind, double *Mdata);

/* The products, on blocks of 1 <= q <= 65535 columns; device pointers on the object's GPU; dW, dV, dX, dZ are n x q
 * doubles.  In-place use (output == input) is refused: the input is read at every step.
 *   Apply:   X = p(S) W                    Sample: Z = D p(S) W                    Matvec: Z = D p(S) p(S) D V
 *   Draw:    the sample of W[j, s] = N(seed, (firstSample + s) n + j), the normal stream of bfhipCovDrawDevice
 *   Moments: samples firstSample .. firstSample + numSamples - 1, `batch` at a time (0 -> 64, at most 64), never stored:
 *            their sums and sums of squares per point are ADDED to dSum / dSumSq (double [n], either may be NULL, not both)
 *            as bfhipCovMomentsDevice does.
 * Errors, raised before the device is touched: INVALID_ARGUMENTS (a NULL object, input or output; q == 0 or > 65535;
 * output == input; batch > 64; numSamples == 0; both moment outputs NULL; no coefficients set). */
int bfhipChebCovApplyBlockDevice(BfhipChebCov *c, const double *dW, size_t q, double *dX, void *stream);
int bfhipChebCovSampleBlockDevice(BfhipChebCov *c, const double *dW, size_t q, double *dZ, void *stream);
int bfhipChebCovMatvecBlockDevice(BfhipChebCov *c, const double *dV, size_t q, double *dZ, void *stream);
int bfhipChebCovDrawDevice(BfhipChebCov *c, uint64_t seed, uint64_t firstSample, size_t q, double *dZ, void *stream);
int bfhipChebCovMomentsDevice(BfhipChebCov *c, uint64_t seed, uint64_t firstSample, uint64_t numSamples, uint32_t batch,
                              double *dSum, double *dSumSq, void *stream);

/* Conditioning the Chebyshev route on observations: a BfhipCovCond (above, "conditioning on observations") for the field
 * z = B w, B = D p(S), given noisy values at the mesh vertices obs[] (host, distinct, < n, mesh order: there is no
 * permutation).  The observed rows of B, transposed, are X = p(S) D E_obs [n x k]: panels of <= 64 unit columns scaled by d
 * (one small kernel), one recurrence each without the output scaling, packed into the stored n x k double matrix; then
 * G = X^T X + D, its Cholesky factor and every entry of the object are the butterfly route's, kernel for kernel.  The
 * correction W' = W + X alpha happens in w space, so a batch of posterior samples costs ONE polynomial application, as a
 * prior batch does.  BfhipCovCondInfo: setupApplies = the number of panels; factorBytes counts everything Create allocates,
 * the object's own W' block [n x 64] included (X alone is n * numObs doubles: a failed allocation is MEMORY_ERROR and
 * leaks nothing).
 *
 * Every block is float64: dW, dZ [n x nrhs], moments [n].  Draw: w_s[j] = N(seed, (firstSample + s) n + j), the stream of
 * bfhipChebCovDrawDevice; the noise as on the butterfly route.  Variance: queries are vertex indices,
 * prior = ||p(S) D e_i||^2, post = prior - ||L^-1 X^T x_i||^2.  LogLikelihood: value and dGradNoise; dGradLogGamma != NULL is
 * refused (INVALID_ARGUMENTS): this route has no per-column weights.
 *
 * `cheb` is referenced: it must outlive the object (bfhipCovCondFree reads nothing through it), and the recurrence runs in
 * cheb's workspace, which Create grows to two blocks of 64 columns.  X holds the polynomial in force at Create:
 * bfhipChebCovSetCoefficients on `cheb` afterwards makes the object STALE -- sample, mean, draw, moments, likelihood and
 * variance then refuse with INVALID_ARGUMENTS and a message that says so; Free and GetInfo still work.  Create a new one.
 *
 * Errors, raised before the device is touched, in bfhipCovCondCreate's order: INVALID_ARGUMENTS (NULL cheb, obs or out;
 * numObs == 0 or > BFHIP_COND_MAX_OBS; a repeated observed index; a noiseVar entry negative or not finite), OUT_OF_RANGE (an
 * observed index >= n), INVALID_ARGUMENTS (no coefficients set; n beyond 65535 x 1024).  A Cholesky pivot <= 0 or not
 * finite: RUNTIME_ERROR, as there. */
int bfhipChebCovCondCreate(BfhipChebCov *cheb, const uint64_t *obs, size_t numObs, const double *noiseVar, BfhipCovCond **out,
                           void *stream);

/* The gradient of the log marginal likelihood in the parameters of the spectral density, on an object made by
 * bfhipChebCovCondCreate.  With X = p(S) D E_obs [n x k] (the object's rows), K = X^T X + N,
 * alpha = K^-1 y and, for a parameter theta_t, the polynomial q_t = d p / d theta_t,
 *   d logLik / d theta_t = < X M, X'_t >_F,   M = alpha alpha^T - K^-1 [k x k],   X'_t = q_t(S) D E_obs.
 * q_t is given by its Chebyshev coefficients on [0, lamMax]: row t of dcoef (HOST, numParams rows of ldCoef doubles, of which
 * the first orders[t] are read).  The fit is linear, so the interpolant of d g / d theta at the order of p IS d coef / d theta:
 * with those coefficients the result is the exact derivative of the value bfhipCovCondLogLikelihoodDevice returns.  An order
 * other than p's is legal.  X'_t is never stored: it is made 64 observed columns at a time as Create makes X (the unit panel,
 * one recurrence with q_t's coefficients, no output scaling), so a call costs numParams x ceil(k / 64) polynomial applications.
 *
 * Per panel of <= 64 observed columns: M[:, panel] from the two triangular solves of a sample pass on the panel's columns of
 * the identity; Y = X M[:, panel] on the FP64 matrix cores (v_mfma_f64_16x16x4_f64), once per panel; per parameter the
 * recurrence and the partial sums of Y o X'_t per 1024 rows; one owner adds the partials in chunk, then panel order.  No
 * atomics: every sum order depends on (n, k, panel) alone, two calls give equal bits, and dGrad[t] depends neither on numParams
 * nor on t's place among the parameters.
 *
 * dGrad [numParams] (device, double).  dValue [3] (device, double) or NULL: { logLik, quad, logDet }, the bits of
 * bfhipCovCondLogLikelihoodDevice.  opt may be NULL; workspaceBytes is not used.  The recurrence runs in cheb's workspace and
 * the unit panels in the object's W' block, as in Create; the scratch of the gradient (Y [n x 64], two k x 64 blocks, the
 * partial sums, the observed indices) is allocated by the first call, which drains `stream`, and kept until bfhipCovCondFree
 * (not counted in factorBytes); a later call only enqueues work.  dcoef and orders are read before the call returns.
 *
 * Errors, raised before the device is touched, in this order: INVALID_ARGUMENTS (a NULL c, dY, dcoef, orders or dGrad;
 * numParams outside 1 .. 64; an order of 0 or above ldCoef; a coefficient that is not finite; a structSize that is not the
 * struct's) -- nothing is read through c up to here --, INVALID_ARGUMENTS (an object not made by bfhipChebCovCondCreate), and
 * the refusal of a stale object (bfhipChebCovSetCoefficients was called after it was made). */
int bfhipChebCovCondLogLikGradDevice(BfhipCovCond *c, const double *dY, const double *dcoef, const size_t *orders,
                                     size_t numParams, size_t ldCoef, double *dGrad, double *dValue,
                                     const BfhipCovCondLikOptions *opt, void *stream);

/* Lowest eigenpairs of the lumped-mass pencil L phi = lambda M phi, on the device, from a BfhipChebCov: the nev lowest
 * pairs (theta, u) of S = D L D by Chebyshev-filtered subspace iteration (Zhou and Saad) on a block of p = nev + guard
 * columns -- what the reference takes from ARPACK and UMFPACK (bfGetShiftedEigs, src/linalg.c) for the lowest band, with
 * no factorisation.  lam[j] = theta_j ascending; dU [n x nev, row-major, leading dimension ldu] = the orthonormal
 * eigenvectors U of S (U^T U = I), or with BFHIP_EIGS_MASS_NORMALISED Phi = D U (Phi^T M Phi = I), the eigenfunctions of
 * the pencil.  The lumped mass unless BFHIP_EIGS_CONSISTENT_MASS asks for the reference's consistent-mass pencil, which has other
 * numbers (bfhipChebCovSetConsistentMass, further down).  Lowest pairs only, p <= 256 per
 * call; bfhipChebCovEigsBandDevice below continues where a call stopped.
 *
 * Per outer iteration: a degree-m Chebyshev filter that damps [largest Ritz value, lamMax] (m <= degree, lowered so that
 * the filtered block's condition number stays below 2^23), Cholesky QR twice, Rayleigh-Ritz, residuals
 * r_j = ||S u_j - theta_j u_j||_2; converged when the first nev are <= tol * lamMax.  The p x p factorisations and the
 * p x p symmetric eigenproblem run on the host, so the call is SYNCHRONOUS (it drains `stream` in every iteration).  It
 * needs no coefficients, leaves the generation counter alone, allocates its own workspace (three blocks of n x p16
 * doubles, p16 = p rounded up to 16, and the partial sums) and frees it before it returns: the object's Clenshaw workspace,
 * which live BfhipCovCond objects share, is not touched.  Two calls with the same arguments give the same bits.
 *
 * Errors, in this order and before the device is touched: INVALID_ARGUMENTS for a NULL c, lam or dU; nev == 0 or
 * nev > min(n, 255); ldu < nev; a wrong structSize; nev + guard > 256, an explicit request for no guard column
 * (BFHIP_EIGS_NO_GUARD, refused unless nev == n) or nev + guard > n with a guard given; degree == 1; tol negative or not
 * finite.  Not converged within maxIter: RUNTIME_ERROR, the outputs hold the best pairs found and the message says how
 * many converged.  A Cholesky pivot that is not positive: one retry of the pass with a shifted Gram matrix, then
 * RUNTIME_ERROR; the caller's buffers are not written in that case. */
#define BFHIP_EIGS_MASS_NORMALISED 1u
#define BFHIP_EIGS_NO_GUARD 2u             /* flags: ask for guard == 0 explicitly (the field's 0 means "default") */
#define BFHIP_EIGS_CONSISTENT_MASS 4u      /* flags: the pencil S u = theta B u of bfhipChebCovSetConsistentMass (below) */
typedef struct BfhipEigsOptions {
  uint32_t structSize;   /* in: sizeof(BfhipEigsOptions) */
  uint32_t guard;        /* extra block columns; 0 = default max(8, nev / 4), clipped so that nev + guard <= min(n, 256) */
  uint32_t degree;       /* filter degree per outer iteration; 0 = default 20; >= 2 */
  uint32_t maxIter;      /* 0 = default 100 */
  double tol;            /* a pair is converged when ||S u - theta u||_2 <= tol * lamMax; 0 = default 1e-10 */
  uint64_t seed;         /* start block X[i][j] = N(seed, i * p + j), the normal stream of bfhipFillNormalDevice */
  uint32_t flags;        /* BFHIP_EIGS_MASS_NORMALISED | BFHIP_EIGS_NO_GUARD | BFHIP_EIGS_CONSISTENT_MASS */
  uint32_t massSteps;    /* BFHIP_EIGS_CONSISTENT_MASS: steps k of every mass solve; 0 = the smallest k with 2 rho^k <= tol; <= 64 */
} BfhipEigsOptions;

typedef struct BfhipEigsInfo {
  uint32_t structSize;   /* in: sizeof(BfhipEigsInfo) */
  uint32_t iterations;   /* outer iterations (filters) run */
  uint32_t converged;    /* leading pairs at or below the tolerance, at most nev */
  uint32_t blockColumns; /* p */
  uint32_t maxDegreeUsed;
  uint32_t reserved;
  uint64_t operatorColumns;   /* columns of S applied in total */
  uint64_t workspaceBytes;
  double maxResidual;         /* over the nev returned pairs, divided by lamMax */
  double lamMax;
} BfhipEigsInfo;

int bfhipChebCovEigsDevice(BfhipChebCov *c, const BfhipEigsOptions *opt /* NULL = defaults */, size_t nev,
                           double *lam /* host, nev, ascending */, double *residual /* host, nev, or NULL */,
                           double *dU /* device, n x nev row-major */, size_t ldu, BfhipEigsInfo *info /* or NULL */, void *stream);

/* The next band: the nev pairs of S that follow m locked ones (the m lowest, found by earlier calls), ascending, with the
 * conventions of bfhipChebCovEigsDevice -- so any number of pairs, a band of nev <= 255 at a time.  The algorithm is the same
 * with the block kept orthogonal to the locked vectors Q: before every orthonormalisation (of the start block and of each
 * filtered block) X <- X - Q (Q^T X) is applied twice, on the device, Q in panels of at most 256 columns one after the other;
 * the filter's degree is lowered further so that the locked directions, which it amplifies most, stay below 2^23 times the
 * block's least amplified Ritz direction (min(locked.lam) is one more point of the cap).  Limits: nev <= min(n - m, 255),
 * p = nev + guard <= min(n - m, 256); with p == n - m the first Rayleigh-Ritz step is exact and no filter runs;
 * BFHIP_EIGS_NO_GUARD is legal only for nev == n - m; the default guard is clipped to n - m - nev.
 *
 * Intended use: one wide array dAll [n x total]; call k passes locked = {m, dAll, total, lamAll}, dU = dAll + m, ldu = total.
 * The call writes columns m .. m + nev - 1 and nothing beside them, and only reads the locked columns.  The locked block must
 * be U (orthonormal), so BFHIP_EIGS_MASS_NORMALISED is refused with count > 0: keep U across the bands and call
 * bfhipChebCovEigsMassNormaliseDevice once at the end.  With locked NULL or count 0 the call is bfhipChebCovEigsDevice.
 *
 * Errors before the device is touched: those of bfhipChebCovEigsDevice in its order, with n - m in place of n; then
 * INVALID_ARGUMENTS for a wrong locked->structSize; count > 0 with NULL dVectors or lam; ld < count; count >= n; a locked
 * eigenvalue that is not finite or lies above lamMax; BFHIP_EIGS_MASS_NORMALISED together with count > 0. */
typedef struct BfhipEigsLocked {
  uint32_t structSize;     /* in: sizeof(BfhipEigsLocked) */
  uint32_t reserved;
  uint64_t count;          /* m >= 0 locked pairs: the m lowest of S */
  const double *dVectors;  /* device, n x count row-major, orthonormal eigenvectors U of S (not mass-normalised) */
  uint64_t ld;             /* >= count; no alignment beyond 8 bytes is required of dVectors or ld */
  const double *lam;       /* host, count eigenvalues of the locked pairs */
} BfhipEigsLocked;

int bfhipChebCovEigsBandDevice(BfhipChebCov *c, const BfhipEigsOptions *opt, const BfhipEigsLocked *locked /* NULL or count 0: none */,
                               size_t nev, double *lam, double *residual, double *dU, size_t ldu, BfhipEigsInfo *info, void *stream);
/* dU[i][j] <- d[i] dU[i][j], j < count, in place (U -> Phi = D U): one multiplication per element.  INVALID_ARGUMENTS for a
 * NULL c or dU (with count > 0) and for ldu < count. */
int bfhipChebCovEigsMassNormaliseDevice(BfhipChebCov *c, double *dU, size_t ldu, size_t count, void *stream);

/* The consistent-mass pencil L phi = lambda M phi (the reference's: bfTrimeshGetLboFemDiscretization, bfGetShiftedEigs,
 * bfGetEigenband), M on the object's CSR pattern.  bfhipChebCovSetConsistentMass folds
 * B[i][j] = (d[i] M[i][j]) d[j], d = massLumped^-1/2 as the object holds it, on the host and uploads one more value array next to
 * S's.  [lo, hi] must enclose the spectrum of B.  lo <= 0 && hi <= 0 asks for the P1 bounds [1/4, 1], which hold for the mass of
 * bfhipTrimeshLboFemMass on any triangle mesh (element by element M_e has the eigenvalues A/12 {4, 1, 1} and the lumped element
 * matrix is A/3 I); they are accepted only when every row sum of Mdata equals massLumped[i] within rounding and every diagonal
 * entry is positive.  Otherwise 0 < lo < hi, both finite.  INVALID_ARGUMENTS, before the device is touched: a NULL argument, an
 * entry of Mdata or a bound that is not finite, lo >= hi or lo <= 0 with bounds given, and the two P1 conditions.  A second call
 * replaces the array after draining the device.  Neither the coefficients nor the generation counter nor any other entry is
 * affected; bfhipChebCovFree releases the array.
 *
 * With BFHIP_EIGS_CONSISTENT_MASS both eigensolver entries solve S u = theta B u: the operator is A = B^-1 S, self-adjoint in the
 * B inner product, with the upper bound lamMaxG = lamMax / lo (BfhipEigsInfo.lamMax reports it).  A filter step is T = S Y_i,
 * Z ~ B^-1 T by massSteps steps of the Chebyshev semi-iteration on [lo, hi] (error <= 2 rho^k, rho = (sqrt(hi / lo) - 1) /
 * (sqrt(hi / lo) + 1): 1/3 for P1), then the three-term combination; Rayleigh-Ritz runs in the B inner product (G = X^T (B X),
 * H = X^T (S X)); the residual is r_j = ||S u_j - theta_j B u_j||_2 with u_j^T B u_j = 1, converged at <= tol * lamMaxG.  Outputs: U
 * with U^T B U = I, or with BFHIP_EIGS_MASS_NORMALISED Phi = D U, Phi^T M Phi = I, the reference's normalisation.  Locked vectors
 * are B-orthonormal eigenvectors of the pencil (U, not Phi); the projection is X <- X - Q (Q^T B X), twice; a locked eigenvalue
 * above lamMaxG is refused.  operatorColumns counts the columns of B applied too.  The call allocates five blocks of n x p16
 * doubles.  massSteps limits the accuracy: the filter's invariant subspace differs from the pencil's by about rho^k, so a k
 * much below the default stagnates above tol.  Refused after every refusal of the lumped call, in this order: the flag on an
 * object with no consistent mass set; massSteps > 64.  Without the flag nothing changes, with a mass set or not. */
int bfhipChebCovSetConsistentMass(BfhipChebCov *c, const double *Mdata /* host, nnz values on the object's pattern */, double lo, double hi);

/* ---- truncated SVD of a real f64 matrix on the device ---------------------- */
/* What the streamer's one numerical step needs (the reference's bfGetTruncatedSvd, src/linalg.c:1002-1082, cut by
 * bfTruncSpecGetNumTerms, src/linalg.c:26-35): A [m x n, row-major, leading dimension lda, device, left unchanged] ~ U_k W,
 * W = S_k V_k^T.  dSigma receives all min(m, n) singular values, descending; k is the number of leading s_j with
 * s_j >= tol * s_0; dU [m x ldu] gets its first k columns (orthonormal), dW [k x n in ldw] its first k rows; nothing else of
 * either is written.  dU / dW may be NULL (a values-only call); capU / capW say how many columns / rows fit: with k above one
 * of them the call returns OUT_OF_RANGE with dSigma and info->k set and U, W untouched, so a caller can size from a first call.
 * An all-zero A returns k = 0 (the reference's rule, 0 >= tol * 0, would keep every term of it).
 *
 * One-sided block Jacobi on the taller orientation (B = A or A^T, M x N with M >= N, columns in tiles of 16 padded with zero
 * columns to an even number of tiles): sweeps of N_tiles - 1 round-robin steps; per step every disjoint tile pair's 32 x 32
 * Gram matrix on the FP64 matrix cores, its eigenvectors Q by cyclic Jacobi in LDS (larger eigenvalue first), the panel times Q
 * on the matrix cores in place.  An entry g_ij is converged at |g_ij| <= max(32, sqrt(M)) eps sqrt(g_ii g_jj), or when one of
 * its columns is below (32 + N) eps times the largest column norm of B as loaded; the call stops after a sweep that rotated nothing.  No V is
 * accumulated: the columns of B end as s_j u_j.  Tall: U = B_k / s, W = U^T A; wide: W = B_k^T, U = A B_k / s^2.
 * SYNCHRONOUS (one drain of `stream` per sweep); allocates its own workspace (the M x N block, the partial Gram matrices, and
 * for U / W a block of M x k and the partials of one contraction) and frees it before it returns.  Every sum has one fixed
 * order that depends on (m, n) alone: two calls give the same bits.
 *
 * Errors, in this order and before the device is touched: INVALID_ARGUMENTS for a NULL dA, opt or dSigma; a wrong structSize;
 * tol <= 0 or tol >= 1 (or NaN); flags or reserved not 0; min(m, n) == 0; min(m, n) > 16384; max(m, n) > 2^32; lda < n;
 * ldu < capU (with dU); ldw < n (with dW).  Not converged within maxSweeps: RUNTIME_ERROR with dSigma (the column norms as they
 * stand) and info filled in, U and W not written. */
typedef struct BfhipTruncSvdOptions {
  uint32_t structSize;   /* in: sizeof(BfhipTruncSvdOptions) */
  uint32_t maxSweeps;    /* 0 = default 30 */
  double tol;            /* relative truncation tolerance, 0 < tol < 1 */
  uint32_t flags;        /* 0 */
  uint32_t reserved;     /* 0 */
} BfhipTruncSvdOptions;

typedef struct BfhipTruncSvdInfo {
  uint32_t structSize;   /* in: sizeof(BfhipTruncSvdInfo) */
  uint32_t sweeps;       /* sweeps run, the last one (which rotated nothing) included */
  uint64_t k;            /* terms kept by the count rule */
  uint64_t numSingular;  /* min(m, n) */
  uint32_t transposed;   /* 1: the call worked on A^T (m < n) */
  uint32_t reserved;
  double offNorm;        /* the largest |g_ij| / sqrt(g_ii g_jj) the last sweep saw, noise columns left out */
  double seconds;        /* wall clock of the call */
  uint64_t workspaceBytes;
} BfhipTruncSvdInfo;

int bfhipTruncSvdDevice(int device /* < 0: the current one */, const double *dA, size_t m, size_t n, size_t lda, const BfhipTruncSvdOptions *opt,
                        double *dSigma, double *dU /* or NULL */, size_t ldu, size_t capU, double *dW /* or NULL */, size_t ldw, size_t capW,
                        BfhipTruncSvdInfo *info /* or NULL */, void *stream);

/* ---- many truncated SVDs in one call ---------------------------------------- */
/* The independent SVDs of one frontier of the streamer (all row nodes of one depth of a feed, or of a merge) in one call: every
 * kernel launch covers all problems, and the host waits once per sweep of the batch instead of once per sweep of every problem.
 * Each problem gets exactly what bfhipTruncSvdDevice gives it -- orientation, padding, thresholds, its own noise level, its own
 * number of sweeps, the sort, the count rule, U and W -- and BIT FOR BIT so: the kernels run the single call's device code on
 * the problem's own parameters, and no sum's order depends on the other problems, on their number, on their order or on the
 * grouping below.  A problem that has converged is skipped on the device from then on.
 *
 * problems: host array of `count` (<= 2^20) problems, device pointers inside, each with the meaning of the single call's
 * arguments; the problems must not overlap in what they write.  infos[i] (or NULL) is filled as the single call fills it, apart
 * from seconds and workspaceBytes, which are 0: they belong to the batch.  status[i] (or NULL) is the code the single call would
 * return for problem i: 0; INVALID_ARGUMENTS for a non-finite column (nothing of the problem written, infos[i] untouched);
 * RUNTIME_ERROR when maxSweeps sweeps did not converge (dSigma holds the column norms, U and W untouched); OUT_OF_RANGE for
 * k > capU or k > capW (dSigma and infos[i].k set, U and W untouched).  A failed problem does not stop the others.  The call
 * returns the status of the lowest-index failed problem, its message (prefixed "problem i: ") in bfhipLastErrorMessage, or 0.
 *
 * Refused before a device is touched, nothing run, in this order: INVALID_ARGUMENTS for a NULL opt or (with count > 0) NULL
 * problems; a wrong structSize of opt or batch; count > 2^20; then, problem by problem, every refusal of bfhipTruncSvdDevice in
 * its order (infos[i].structSize included), the message being the single call's prefixed "problem i: ".  count == 0 returns 0.
 *
 * Workspace: the problems are processed in consecutive groups whose summed device workspace (per problem: what the single call
 * allocates for the sweeps, plus its recovery stage at k = min(m, n) when dU or dW is given) fits workspaceLimitBytes; 0 means
 * 1 GiB.  A problem above the limit is a group of its own.  One allocation per group for the sweeps and one for the recovery.
 * SYNCHRONOUS.  batch->synchronisations is, exactly, the sum over the groups of (the largest sweep count in the group + 3): one
 * wait for the sums of squares of the blocks as loaded, one per sweep, one for the final column norms, one at the end; with one
 * group that is batch->maxSweeps + 3.  batch->launches counts kernel launches: per group 3 for the load and its sums, per sweep
 * 3 (max tiles of a still active problem - 1) + 1, then 2 + 1 and at most 6 for the recovery. */
typedef struct BfhipTruncSvdProblem {
  const double *dA; uint64_t m, n, lda;
  double *dSigma;                          /* min(m, n) */
  double *dU; uint64_t ldu, capU;          /* dU may be NULL */
  double *dW; uint64_t ldw, capW;          /* dW may be NULL */
} BfhipTruncSvdProblem;

typedef struct BfhipTruncSvdBatchInfo {
  uint32_t structSize, groups;             /* in: sizeof(BfhipTruncSvdBatchInfo); groups: consecutive sub-batches the workspace limit forced */
  uint32_t maxSweeps, failed;              /* largest sweep count of a problem; problems whose status != 0 */
  uint64_t launches, synchronisations;     /* kernel launches and stream synchronisations of the whole call */
  uint64_t workspaceBytes;                 /* peak over the groups */
  double seconds;                          /* wall clock of the call */
} BfhipTruncSvdBatchInfo;

int bfhipTruncSvdBatchDevice(int device /* < 0: the current one */, const BfhipTruncSvdProblem *problems, size_t count, const BfhipTruncSvdOptions *opt,
                             uint64_t workspaceLimitBytes /* 0: 1 GiB */, BfhipTruncSvdInfo *infos /* [count] or NULL */,
                             int32_t *status /* [count] or NULL */, BfhipTruncSvdBatchInfo *batch /* or NULL */, void *stream);

/* ---- plan inspection (no device needed) ---------------------------------- */
/* The flattened per-stage layout, as the kernels see it.  Valid only for an
 * operator compiled with BFHIP_FLAG_PLAN_ONLY (the host mirrors are dropped
 * after upload otherwise); pointers stay owned by the operator.  Record
 * layouts: BfDevItem = {u32 pieceBegin, numPieces, outOff, mrFlags},
 * BfDevPiece = {u64 dataOff; u32 inOff, ncols, flags, ld}; in the transposed
 * plan a piece is a forward piece read with lanes on its columns: element
 * (step s, lane j) = arena[dataOff + j*ld + s], ncols = number of steps.
 * mrFlags = rows | flags: 1<<16 the item writes y (else the vector arena);
 * 1<<17 ROWMAJOR (real operands, <= 2 lane granules of rows: the item's dense
 * pieces are stored row by row, element (r, c) = arena[dataOff + r*ld + c],
 * row ends zero-padded: ld is a multiple of the granule, and of 128 bytes for
 * pieces of >= 128 columns, whose rows start on 128-byte lines; one piece per
 * <= 1024-column task);
 * 1<<18 MERGED (column-major dense pieces are one contiguous block of <= 256
 * columns, contracted in one go); 1<<19 SMALL (<= 2 granules of rows, <= 16
 * pieces, < 128 columns: such items are the END of a stage's list and run
 * four to a wavefront in their own launch; their pieces are row-major too);
 * 1<<20 TNARROW (transposed plans: <= 16 columns of a tall leaf; such items
 * are the START of a stage's list and run on the 16-row-lane kernel).  Piece flags: 1 reads x (else the
 * vector arena), 2 identity (no data: adds the input rows), 4 row-major. */
typedef struct BfhipPlanInfo {
  uint32_t structSize, dtype, elemSize, epl, xcap;
  uint32_t reserved;                 /* 1: the adjoint plan is a forward plan of the transposed expression over an arena of its own
                                        (BFHIP_FLAG_ADJOINT_PACKED): its stages are run like forward stages, on bfhipPlanPackArenaT's data */
  uint64_t numRows, numCols, numStages, arenaElems, tempElems;
  uint64_t numStagesT, tempElemsT;   /* transposed plan (0 without BFHIP_FLAG_ADJOINT) */
  uint64_t arenaElemsT;              /* elements of the packed adjoint's own arena (0 otherwise) */
} BfhipPlanInfo;
typedef struct BfhipStageView {
  uint32_t structSize, reserved;
  uint64_t numItems, numPieces, numReduce;
  const void *items;      /* BfDevItem[numItems]  (16 bytes each) */
  const void *pieces;     /* BfDevPiece[numPieces] (24 bytes each) */
  /* filled when structSize covers them: forward complex128 stages -- runs of up to 4 list neighbours that read the same input rows
   * (bit 31 of an entry: unrelated neighbours); bundleBegin[numBundles + 1].  A description of the list's X sharing: no kernel reads
   * it.  Operators without the planner's host tables (bfhipLoad) report numBundles = 0 and a NULL table */
  uint64_t numBundles;
  const uint32_t *bundleBegin;
} BfhipStageView;
typedef struct BfhipReduceView {
  uint32_t structSize, destIsY;
  uint64_t destOff, numRows, numIntervals, numSrc;
  const uint32_t *rowInterval;   /* [numRows] */
  const uint32_t *ivBegin;       /* [numIntervals+1] */
  const int64_t *srcBias;        /* [numSrc] */
} BfhipReduceView;
/* `stage` indices >= numStages address the transposed plan (BFHIP_FLAG_ADJOINT): stage - numStages */
int bfhipPlanGetInfo(const BfhipOperator *op, BfhipPlanInfo *info);
int bfhipPlanGetStage(const BfhipOperator *op, uint64_t stage, BfhipStageView *view);
int bfhipPlanGetReduce(const BfhipOperator *op, uint64_t stage, uint64_t index, BfhipReduceView *view);
/* Which kernels an apply runs: one value per instantiation of the apply path's stage and reduce kernels (the experimental
 * library's executors are not listed).  T = transposed (shared-leaf adjoint); NARROW / WIDE = the 16- and 4-row-lane tilings
 * of bfStageKernelT, COOP = its workgroup-shared leading items; ONE = the nrhs == 1 instantiation, N = the others. */
typedef enum BfhipKernelId {
  BFHIP_KERNEL_C128 = 0,                                  /* forward complex128, nrhs < 2: bfStageKernelC128 */
  BFHIP_KERNEL_C128_MFMA1, BFHIP_KERNEL_C128_MFMA2, BFHIP_KERNEL_C128_MFMA4,                     /* nrhs <= 16, <= 32, more */
  BFHIP_KERNEL_C128_MFMA1_EXACT, BFHIP_KERNEL_C128_MFMA2_EXACT, BFHIP_KERNEL_C128_MFMA4_EXACT,   /* BFHIP_FLAG_EXACT_COMPLEX */
  BFHIP_KERNEL_REAL_F64, BFHIP_KERNEL_REAL_F32, BFHIP_KERNEL_REAL_C64,                           /* bfStageKernelReal */
  BFHIP_KERNEL_REALBOTH_F64, BFHIP_KERNEL_REALBOTH_F32, BFHIP_KERNEL_REALBOTH_C64,               /* ordinary + small items */
  BFHIP_KERNEL_SMALL_F64, BFHIP_KERNEL_SMALL_F32, BFHIP_KERNEL_SMALL_C64,                        /* small items alone */
  /* transposed: 8 per dtype, dtype-major in BFHIP_C128, F64, F32, C64 order */
  BFHIP_KERNEL_T_C128_NARROW_N, BFHIP_KERNEL_T_C128_NARROW_ONE, BFHIP_KERNEL_T_C128_NARROW_COOP_N, BFHIP_KERNEL_T_C128_NARROW_COOP_ONE,
  BFHIP_KERNEL_T_C128_WIDE_N, BFHIP_KERNEL_T_C128_WIDE_ONE, BFHIP_KERNEL_T_C128_WIDE_COOP_N, BFHIP_KERNEL_T_C128_WIDE_COOP_ONE,
  BFHIP_KERNEL_T_F64_NARROW_N, BFHIP_KERNEL_T_F64_NARROW_ONE, BFHIP_KERNEL_T_F64_NARROW_COOP_N, BFHIP_KERNEL_T_F64_NARROW_COOP_ONE,
  BFHIP_KERNEL_T_F64_WIDE_N, BFHIP_KERNEL_T_F64_WIDE_ONE, BFHIP_KERNEL_T_F64_WIDE_COOP_N, BFHIP_KERNEL_T_F64_WIDE_COOP_ONE,
  BFHIP_KERNEL_T_F32_NARROW_N, BFHIP_KERNEL_T_F32_NARROW_ONE, BFHIP_KERNEL_T_F32_NARROW_COOP_N, BFHIP_KERNEL_T_F32_NARROW_COOP_ONE,
  BFHIP_KERNEL_T_F32_WIDE_N, BFHIP_KERNEL_T_F32_WIDE_ONE, BFHIP_KERNEL_T_F32_WIDE_COOP_N, BFHIP_KERNEL_T_F32_WIDE_COOP_ONE,
  BFHIP_KERNEL_T_C64_NARROW_N, BFHIP_KERNEL_T_C64_NARROW_ONE, BFHIP_KERNEL_T_C64_NARROW_COOP_N, BFHIP_KERNEL_T_C64_NARROW_COOP_ONE,
  BFHIP_KERNEL_T_C64_WIDE_N, BFHIP_KERNEL_T_C64_WIDE_ONE, BFHIP_KERNEL_T_C64_WIDE_COOP_N, BFHIP_KERNEL_T_C64_WIDE_COOP_ONE,
  /* transposed real-family stages with both item ranges in one launch (bfStageKernelTBoth) */
  BFHIP_KERNEL_TBOTH_F64_N, BFHIP_KERNEL_TBOTH_F64_ONE, BFHIP_KERNEL_TBOTH_F32_N, BFHIP_KERNEL_TBOTH_F32_ONE,
  BFHIP_KERNEL_TBOTH_C64_N, BFHIP_KERNEL_TBOTH_C64_ONE,
  /* bfReduceKernel; LONG: some row of the batch has >= 64 partial sums */
  BFHIP_KERNEL_REDUCE_C128, BFHIP_KERNEL_REDUCE_F64, BFHIP_KERNEL_REDUCE_F64_LONG, BFHIP_KERNEL_REDUCE_F32,
  BFHIP_KERNEL_REDUCE_F32_LONG, BFHIP_KERNEL_REDUCE_C64, BFHIP_KERNEL_REDUCE_C64_LONG,
  BFHIP_KERNEL_COUNT
} BfhipKernelId;
/* Extension range: kernels that only an opted-in operator runs (bfhipSetRhsBlocks).  The ids above never move; ids
 * [BFHIP_KERNEL_COUNT, BFHIP_KERNEL_EXT_BASE) are unused. */
#define BFHIP_KERNEL_EXT_BASE 64u
enum { BFHIP_KERNEL_C64_MFMA1 = 64, BFHIP_KERNEL_C64_MFMA2 = 65, BFHIP_KERNEL_C64_MFMA4 = 66, BFHIP_KERNEL_EXT_END = 67 };   /* forward complex64 block kernels: nrhs <= 16, <= 32, more */
/* Second extension range: the forward block kernels of the real element types (bfhipSetRealRhsBlocks); per type nrhs <= 16,
 * <= 32, more.  Ids [BFHIP_KERNEL_EXT_END, BFHIP_KERNEL_REAL_EXT_BASE) are unused. */
#define BFHIP_KERNEL_REAL_EXT_BASE 72u
enum { BFHIP_KERNEL_F64_MFMA1 = 72, BFHIP_KERNEL_F64_MFMA2 = 73, BFHIP_KERNEL_F64_MFMA4 = 74,
       BFHIP_KERNEL_F32_MFMA1 = 75, BFHIP_KERNEL_F32_MFMA2 = 76, BFHIP_KERNEL_F32_MFMA4 = 77, BFHIP_KERNEL_REAL_EXT_END = 78 };
/* Third extension range: the block kernels of the shared-leaf adjoint (bfhipSetAdjointRhsBlocks), bfStageKernelTMfma: per element
 * type (in the order of the transposed ids above: C128, F64, F32, C64) nrhs <= 16, <= 32, more.  Ids [BFHIP_KERNEL_REAL_EXT_END,
 * BFHIP_KERNEL_T_EXT_BASE) are unused. */
#define BFHIP_KERNEL_T_EXT_BASE 80u
enum { BFHIP_KERNEL_T_C128_MFMA1 = 80, BFHIP_KERNEL_T_C128_MFMA2 = 81, BFHIP_KERNEL_T_C128_MFMA4 = 82,
       BFHIP_KERNEL_T_F64_MFMA1 = 83, BFHIP_KERNEL_T_F64_MFMA2 = 84, BFHIP_KERNEL_T_F64_MFMA4 = 85,
       BFHIP_KERNEL_T_F32_MFMA1 = 86, BFHIP_KERNEL_T_F32_MFMA2 = 87, BFHIP_KERNEL_T_F32_MFMA4 = 88,
       BFHIP_KERNEL_T_C64_MFMA1 = 89, BFHIP_KERNEL_T_C64_MFMA2 = 90, BFHIP_KERNEL_T_C64_MFMA4 = 91, BFHIP_KERNEL_T_EXT_END = 92 };
/* "bfStageKernelT<F64, wide, coop, nrhs=1>"-style name of a kernel id; NULL for an id that is neither below BFHIP_KERNEL_COUNT
 * nor in one of the three extension ranges */
const char *bfhipKernelName(uint32_t id);
/* The kernels, in launch order, that applying stage `stage` (numbering as bfhipPlanGetStage) to `nrhs` right-hand sides
 * launches: the stage's own kernels, then one reduce kernel per reduce launch.  Works under BFHIP_FLAG_PLAN_ONLY (no device).
 * *count = the number of launches; at most `cap` ids are written. */
int bfhipPlanStageKernels(const BfhipOperator *op, uint64_t stage, uint32_t nrhs, uint32_t *ids, uint32_t cap, uint32_t *count);
/* Write the packed leaf arena (arenaElems elements) to host memory; the
 * descriptor's / graph's leaf values must still be alive.  Synthetic leaves
 * are generated with the host copy of the value stream. */
int bfhipPlanPackArena(const BfhipOperator *op, void *dst);
/* the second arena of a BFHIP_FLAG_ADJOINT_PACKED plan (BfhipPlanInfo.arenaElemsT elements) */
int bfhipPlanPackArenaT(const BfhipOperator *op, void *dst);

/* ---- serialization ------------------------------------------------------- */
/* Write / read a compiled operator (packed leaf arena + per-stage index
 * metadata, both plans if BFHIP_FLAG_ADJOINT) -- the loader the reference's
 * write-only bfMatDump never had (src/mat.c:67-73).  A loaded operator applies
 * bit-identically to the saved one.  Errors: FILE_ERROR (cannot open, bad
 * magic, truncated), MEMORY_ERROR, RUNTIME_ERROR.  `opts` of Load: device,
 * maxRhs, BFHIP_FLAG_PROFILE are honoured. */
int bfhipSave(BfhipOperator *op, const char *path);
int bfhipLoad(const char *path, const BfhipOptions *opts, BfhipOperator **out);

/* ---- lifetime ------------------------------------------------------------ */
void bfhipFree(BfhipOperator **op);

/* ---- reference-vtable shim ----------------------------------------------- */

/* A `BfMat *` whose vtable implements Mul, Rmul, MulVec, RmulVec, Transpose, GetView, GetNumRows,
 * GetNumCols, GetType (-> BF_TYPE_MAT_FUNC), NumBytes and Delete on top of
 * `op`, so that unmodified reference code (bfSolveGMRES src/linalg.c:125,155;
 * cov_matvec examples/covariance/lbo_cov.c:48-60; an enclosing BfMatBlockDense,
 * src/mat_block_dense.c:541-563) can call bfMatMul / bfMatMulVec / bfMatRmulVec
 * on it.  Mul results are allocated through the RHS's own vtable (`EmptyLike`,
 * slot 8) so that the reference's bfMatDelete frees them
 * (mat_dense_complex.c:2164-2187); Rmul (slot 44: bfMatRmul(A, X) = X A for a
 * BfMatDenseComplex X, src/mat.c:195-197, src/mat_product.c:282-310,
 * src/mat_dense_complex.c:1075-1133) applies the adjoint plan to the rows of X
 * (BFHIP_FLAG_ADJOINT) and allocates X A the same way; MulVec / RmulVec results are malloc'd
 * BfVecReal of the operator's row / column count carrying the argument's
 * vtable (rectangular operators are fine).  Transpose (slot 63, bfMatTranspose,
 * src/mat.c:271-273) works in place like bfMatProductTranspose
 * (src/mat_product.c:409-420): the object switches between the forward and the
 * adjoint plan of `op` (BFHIP_FLAG_ADJOINT; without it the slot raises
 * BF_ERROR_NOT_IMPLEMENTED and changes nothing), GetNumRows / GetNumCols answer
 * for A^T, MulVec multiplies by A^T and RmulVec by A (real operators); Mul on a
 * complex operator multiplies by A^H afterwards, as in the reference, whose dense
 * complex leaves transpose by bfMatConjTrans and multiply through CblasConjTrans
 * (src/mat_dense_complex.c:1475-1478, 27-35); twice is the identity.
 * Delete releases the shim and, if `ownsOperator`, the operator; a GetView copy
 * never owns it (and is transposed if its source was). */
void *bfhipMatNew(BfhipOperator *op, int ownsOperator);

/* Failures of the shim's Mul / MulVec / RmulVec / GetView return NULL and, by default, also raise
 * the reference's global error state: `bfSetError(code)` (src/error.c:20-24) is looked up in the
 * host process at run time (libbfhip does not link the reference).  bfSetError asserts on a
 * non-zero code, so in a reference build with assertions this is as fatal as the reference's own
 * BF_DIE() paths; pass 0 to keep failures to NULL + bfhipLastErrorMessage(). */
void bfhipSetErrorForwarding(int on);

/* `MatMulFunc` for the reference's own callback operator
 * (include/bf/mat_func.h:5): bfMatFuncInit(f, m, n, bfhipMatMulFunc, op). */
void *bfhipMatMulFunc(const void *rhsBfMat, void *op);

/* ---- errors -------------------------------------------------------------- */
const char *bfhipErrorString(int code);
/* message of the most recent failure on this thread ("" if none) */
const char *bfhipLastErrorMessage(void);

/* Value of element `idx` of the synthetic value stream for `seed`: uniform in
 * [-1, 1).  Identical on host and device (exact IEEE operations), so a CPU
 * restatement can rebuild the very operand the device synthesized.  A leaf
 * with node id L and m x n row-major elements uses
 *   idx = leafBase(L) + i*n + j  (re) and the same idx with stream bit set (im),
 * scaled by sqrt(3/(2n)) (complex) or sqrt(3/n) (real). */
double bfhipSyntheticValue(uint64_t seed, uint64_t idx, int imag);   /* = bfhip_synth_value, include/bfhip_synth.h */
/* virtual base index of leaf `node` (prefix sum of rows*cols over dense nodes
 * in node order), for a given descriptor */
int bfhipSyntheticLeafBases(const BfhipDesc *desc, uint64_t *bases);

#ifdef __cplusplus
}
#endif
#endif /* BFHIP_H */
