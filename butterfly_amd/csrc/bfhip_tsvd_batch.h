/* bfhip_tsvd_batch.h -- what the host side (bfhip_tsvd_batch.c) and the batched kernels (second half of bfhip_tsvd.hip) of
 * bfhipTruncSvdBatchDevice share: the device tables, the flat pair index and the launches.  The algorithm, the geometry and the
 * kernel bodies are the single call's (bfhip_tsvd.h, bfhip_tsvd.hip).  Plain C, no HIP type: tests/native/tsvd_batch_host_check.c
 * compiles the host side against stand-ins of the launches.  DESIGN.md section 30. */
#ifndef BFHIP_TSVD_BATCH_H
#define BFHIP_TSVD_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "bfhip_tsvd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One problem of a group as the sweep kernels see it: constant for the group's lifetime, uploaded once.  B, part and Q are the
 * problem's slices of the group's workspace in the single call's layout (bfTsvdWorkspaceElems); sumSq is its slice of ONE
 * packed array of the group (so that all sums come back in one copy), flag its slice of the flag array. */
typedef struct BfTsvdBatchItem {
  double const *A;                 /* as given: m x n in lda */
  uint64_t m, n, lda;
  double *B, *part, *Q, *sumSq;
  uint32_t *flag;
  uint64_t M, chunkRows;           /* rows of B; rows per chunk of the partials (bfTsvdChunkRows) */
  uint32_t ld, nt, chunks, transposed;
  uint32_t pairBase, reserved;     /* the flat index of the problem's pair 0 */
  double thr;                      /* bfTsvdThreshold(M) */
} BfTsvdBatchItem;

/* What changes while a group runs, one per problem, beside the item table: written by the host once (after the noise levels are
 * known), updated by the pair solves (state) and by the end-of-sweep kernel (active, sweeps; state cleared for the problems that
 * go on), read back whole in one copy per sweep.  A problem retires (active = 0) after a sweep that rotated nothing or at
 * maxSweeps; its state keeps the last sweep's figures. */
typedef struct BfTsvdBatchWords {
  BfTsvdSweepState state;
  double noiseAbs;                 /* noise * noise * gmax, computed by the host from the sums of squares of the block as loaded */
  uint32_t active, sweeps;
} BfTsvdBatchWords;

/* The recovery of one problem: written by the host after the sort, uploaded once with the packed sigma / scale / perm arrays */
enum { BF_TSVD_FIN_SIGMA = 1, BF_TSVD_FIN_GATHER = 2, BF_TSVD_FIN_GATHERT = 4, BF_TSVD_FIN_COPY = 8, BF_TSVD_FIN_RELOAD = 16, BF_TSVD_FIN_CONTRACT = 32 };
typedef struct BfTsvdBatchFin {
  double *dSigma, *dU, *dW;        /* the caller's */
  uint64_t ldu, ldw;
  double const *sigma, *scale;     /* device, the problem's slices of the packed arrays: N values, k scales */
  uint32_t const *perm;            /* k column indices */
  double *Bs, *cpart;              /* the gathered block M x kld; the contraction's partials */
  uint64_t k, N, crows, cchunks;   /* crows: bfTsvdContractChunkRows(M, ld) */
  uint32_t kld, ops;               /* ops: BF_TSVD_FIN_* */
} BfTsvdBatchFin;

/* the flat pair index of a group: problem i owns the pairs [first[i], first[i] + nt_i / 2); owner[flat] = i.  first has count + 1
 * entries; returns the total, or 0 when it would pass 2^31 - 1 (the group is then too large for one grid dimension) */
static inline uint64_t bfTsvdBatchPairTable(uint32_t const *nts, size_t count, uint32_t *first, uint32_t *owner) {
  uint64_t total = 0;
  for (size_t i = 0; i < count; ++i) {
    first[i] = (uint32_t)total;
    uint32_t const pairs = nts[i] / 2;
    if (total + pairs > 0x7fffffffull) return 0;
    if (owner)
      for (uint32_t p = 0; p < pairs; ++p) owner[total + p] = (uint32_t)i;
    total += pairs;
  }
  first[count] = (uint32_t)total;
  return total;
}

/* the work of flat pair `flat` in round-robin step `step`: 1 with the two tiles, or 0 when its problem (of nt tiles, first pair
 * `pairBase`) has no such step: step >= nt - 1.  One function for the host's checks and the kernels. */
static inline BF_TSVD_BOTH int bfTsvdBatchPair(uint32_t nt, uint32_t pairBase, uint32_t flat, uint32_t step, uint32_t *pair, uint32_t *ti, uint32_t *tj) {
  if (step + 1 >= nt) return 0;
  *pair = flat - pairBase;
  bfTsvdPair(nt, step, *pair, ti, tj);
  return 1;
}

/* bytes of device memory one problem takes in a group: the sweep stage (what the single call allocates) and the upper bound
 * (k = N) of its share of the recovery stage when U or W is asked for.  The grouping under a workspace limit sums these. */
uint64_t bfTsvdBatchProblemBytes(uint64_t m, uint64_t n, int wantUW);
#define BF_TSVD_BATCH_DEFAULT_LIMIT (1ull << 30)

/* ---- launches (bfhip_tsvd.hip), each over all `count` problems of a group; every one is ONE kernel launch but step (three) and
 * sumSq (two).  A workgroup beyond its problem's extent exits after reading the item.
 *   load:       B = A or A^T for every problem (fin == NULL), or for those with BF_TSVD_FIN_RELOAD (the wide case's U)
 *   step:       one round-robin step over the totalPairs pairs of all problems: Gram partials, pair solves, rotations; a pair
 *               whose problem is not active, or has fewer than step + 2 tiles, is skipped on the device
 *   endSweep:   per problem still active: ++sweeps; retire it if the sweep rotated nothing or sweeps == maxSweeps, else clear
 *               its counters
 *   sumSq:      the column sums of squares of every problem into its sumSq slice
 *   finish*:    the recovery's kernels over the problems whose `ops` ask for them: sigma (dSigma <- packed values), gather,
 *               gatherT, copyCols, contract + store */
int bfdevTsvdBatchLoad(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream);
int bfdevTsvdBatchStep(BfTsvdBatchItem const *items, BfTsvdBatchWords *words, uint32_t const *owner, uint32_t totalPairs, uint32_t step,
                       uint32_t maxChunks, uint64_t maxRows, void *stream);
int bfdevTsvdBatchEndSweep(BfTsvdBatchWords *words, uint32_t count, uint32_t maxSweeps, void *stream);
int bfdevTsvdBatchSumSq(BfTsvdBatchItem const *items, uint32_t count, uint32_t maxChunks, uint32_t maxLd, void *stream);
int bfdevTsvdBatchSigma(BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxN, void *stream);
int bfdevTsvdBatchGather(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream);
int bfdevTsvdBatchGatherT(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream);
int bfdevTsvdBatchCopyCols(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream);
int bfdevTsvdBatchContract(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint32_t maxChunks, uint64_t maxTileWork, void *stream);
int bfdevTsvdBatchContractStore(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream);

#ifdef __cplusplus
}
#endif
#endif
