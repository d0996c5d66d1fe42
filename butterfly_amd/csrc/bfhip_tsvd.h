/* bfhip_tsvd.h -- what the host side (bfhip_tsvd.c) and the kernels (bfhip_tsvd.hip) of bfhipTruncSvdDevice share: the tile
 * geometry, the round-robin schedule of the tile pairs, the thresholds, the chunking of the partial sums and the launches.
 * Plain C, no HIP type: tests/native/tsvd_host_check.c compiles the host side against stand-ins of the launches.
 * DESIGN.md section 29. */
#ifndef BFHIP_TSVD_H
#define BFHIP_TSVD_H

#include <math.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the schedule is one function for the host and the kernels */
#ifdef __HIPCC__
#define BF_TSVD_BOTH __host__ __device__
#else
#define BF_TSVD_BOTH
#endif

#define BF_TSVD_TILE 16u            /* columns of a tile */
#define BF_TSVD_PAIR 32u            /* columns of a tile pair: the order of the pair's Gram matrix */
#define BF_TSVD_MAX_DIM 16384u      /* min(m, n) at most */
#define BF_TSVD_INNER_SWEEPS 12u    /* cyclic Jacobi sweeps of one pair solve at most */
#define BF_TSVD_EPS 0x1p-52

/* the leading dimension of the working block: N columns rounded up to an EVEN number of 16-column tiles */
static inline uint32_t bfTsvdLd(uint64_t N) { return (uint32_t)((N + BF_TSVD_PAIR - 1) / BF_TSVD_PAIR * BF_TSVD_PAIR); }

/* Pair p (< nt / 2) of step `step` (< nt - 1) of the round robin over nt (even, >= 2) tiles: tile nt - 1 stays, the others
 * turn.  Over the nt - 1 steps of a sweep every two tiles meet exactly once; within a step the pairs are disjoint.  The
 * smaller index comes first, so the columns with the larger norms (sorted first by the pair solve) drift to the low tiles. */
static inline BF_TSVD_BOTH void bfTsvdPair(uint32_t nt, uint32_t step, uint32_t p, uint32_t *ti, uint32_t *tj) {
  uint32_t const r = nt - 1;
  uint32_t a, b;
  if (p == 0) { a = r; b = step % r; }
  else { a = (step + p) % r; b = (step + r - p) % r; }
  if (a < b) { *ti = a; *tj = b; } else { *ti = b; *tj = a; }
}

/* an entry g_ij of a pair's Gram matrix is converged at or below this times sqrt(g_ii g_jj): the rounding of an M-term sum */
static inline double bfTsvdThreshold(uint64_t M) {
  double const s = sqrt((double)M);
  return (s > 32.0 ? s : 32.0) * BF_TSVD_EPS;
}
/* a column whose norm is at or below this times the largest column norm of the block as it was loaded takes no part in a
 * rotation: what the updates' own rounding leaves in a column that is zero in exact arithmetic.  The level is global on
 * purpose: measured against its own pair's largest column, a ladder of ever smaller noise columns stays live wherever no large
 * column sits beside it, and converges only linearly */
static inline double bfTsvdNoise(uint64_t N) { return (32.0 + (double)N) * BF_TSVD_EPS; }

/* rows per chunk of the pair-Gram partials (chunks x pairs x 32 x 32 doubles, within 2^24 doubles) and of the column sums of
 * squares: a multiple of 16, 128 at least, at most 256 chunks.  A function of (M, ld) alone. */
static inline uint64_t bfTsvdChunkRows(uint64_t M, uint32_t ld) {
  uint64_t const pairs = ld / BF_TSVD_PAIR;
  uint64_t maxChunks = (1ull << 14) / pairs;
  if (maxChunks > 256) maxChunks = 256;
  if (maxChunks < 1) maxChunks = 1;
  uint64_t rows = (M + maxChunks - 1) / maxChunks;
  rows = (rows + 15) / 16 * 16;
  return rows < 128 ? 128 : rows;
}
/* rows per chunk of the final contraction X^T Y (chunks x ld x ld doubles at most, within 2^25 doubles); (M, ld) alone */
static inline uint64_t bfTsvdContractChunkRows(uint64_t M, uint32_t ld) {
  uint64_t maxChunks = (1ull << 25) / ((uint64_t)ld * ld);
  if (maxChunks > 64) maxChunks = 64;
  if (maxChunks < 1) maxChunks = 1;
  uint64_t rows = (M + maxChunks - 1) / maxChunks;
  rows = (rows + 15) / 16 * 16;
  return rows < 256 ? 256 : rows;
}

/* the sweep's counters, device: [0] pairs rotated in the sweep, [1] the bits of the largest relative off-diagonal entry seen */
typedef struct BfTsvdSweepState { unsigned long long rotated, offBits; } BfTsvdSweepState;

/* ---- the host side's own pieces (bfhip_tsvd.c), shared with the batched driver (bfhip_tsvd_batch.c) -------------------------
 *   tsvdColCmp:            qsort comparator of the column norms: descending, ties by the lower index
 *   bfTsvdCount:           the count rule: leading sigma_j >= tol * sigma_0; 0 for an all-zero matrix
 *   bfTsvdCheckArguments:  the entry's refusals, in the header's order; 0 or the recorded failure (declared by its users: its types are bfhip.h's)
 *   bfTsvdWorkspaceElems:  doubles of the sweep workspace (block, partials, Q, sums of squares) and the offsets in it */
typedef struct TsvdCol { double norm; uint32_t index; } TsvdCol;
int tsvdColCmp(void const *a, void const *b);
uint64_t bfTsvdCount(double const *sigma, uint64_t count, double tol);
uint64_t bfTsvdWorkspaceElems(uint64_t M, uint32_t ld, uint64_t *offPart, uint64_t *offQ, uint64_t *offSumSq);

/* ---- launches (bfhip_tsvd.hip); every block is row-major ------------------------------------------------------------------
 *   load:      B [M x ld] = A (m x n in lda) or A^T, padding columns zero
 *   step:      one round-robin step of one sweep over all nt / 2 pairs: partial Gram matrices per chunk, the pair solves (Q
 *              [pairs x 32 x 32] and flag [pairs]; the counters of `state` updated), the rotations of the flagged pairs in place;
 *              noiseAbs: the SQUARED column norm at or below which a column is left alone
 *   sumSq:     out[c] = sum over rows of B[r][c]^2, c < ld, partials per chunk summed in chunk order
 *   gather:    out [M x kld] column j < k = scale[j] * B[:, perm[j]], the columns from k to kld zero
 *   gatherT:   out[j][c] = B[c][perm[j]], j < k, c < M (the wide case's W)
 *   contract:  out [nx x ny in ldo] = X[:, :nx]^T Y[:, :ny] over M rows, partials per chunk summed in chunk order
 *   copyCols:  out[i][j] = X[i][j], j < k (U out of the gathered block) */
int bfdevTsvdLoad(double const *dA, uint64_t m, uint64_t n, uint64_t lda, int transpose, double *B, uint32_t ld, void *stream);
int bfdevTsvdStep(double *B, uint64_t M, uint32_t ld, uint32_t step, double thr, double noiseAbs, double *part, double *Q, uint32_t *flag,
                  BfTsvdSweepState *state, void *stream);
int bfdevTsvdSumSq(double const *B, uint64_t M, uint32_t ld, double *part, double *out, void *stream);
int bfdevTsvdGather(double const *B, uint64_t M, uint32_t ld, uint32_t const *perm, double const *scale, uint64_t k, double *out, uint32_t kld,
                    void *stream);
int bfdevTsvdGatherT(double const *B, uint64_t M, uint32_t ld, uint32_t const *perm, uint64_t k, double *out, uint64_t ldo, void *stream);
int bfdevTsvdContract(double const *X, uint64_t ldx, uint64_t nx, double const *Y, uint64_t ldy, uint64_t ny, uint64_t M, uint64_t chunkRows,
                      double *part, double *out, uint64_t ldo, void *stream);
int bfdevTsvdCopyCols(double const *X, uint64_t M, uint32_t ldx, uint64_t k, double *out, uint64_t ldo, void *stream);

#ifdef __cplusplus
}
#endif
#endif
