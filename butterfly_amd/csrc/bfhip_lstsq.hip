// bfhip_lstsq.hip -- gfx950 device layer of the fac_helm2 value builder: the batched truncated least squares
// (bfhipLstSqTruncated; include/bfhip_build.h).
//
// What runs here replaces, for every re-expansion matrix of a Helmholtz butterfly,
//   * bfHelm2GetReexpansionMatrix                   src/helm2.c:321-365
//     = bfMatDenseComplexDenseComplexLstSq          src/mat_dense_complex.c:1767-1849
//       (LAPACK zgesvd + truncation + two zgemm)
//       -> bfJacobiKernel: one-sided (Hestenes) Jacobi SVD, one workgroup per
//          problem, column pairs of a round-robin step spread over lane groups;
//          bfQrcpKernel ahead of it for the problems that do not stay in LDS
//          (Householder QR with column pivoting; Jacobi then works on R^H);
//          bfGemmKernel: T = diag(1/sigma^2) (U Sigma)^H Z_orig, X = V T.
// Not on the apply path: compute-bound FP64 VALU work (rotations), written for clarity
// first: fixed summation orders, no atomics in any result.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"
#include "../../include/bfhip_build.h"

// ---------------------------------------------------------------------------
// one-sided (Hestenes) Jacobi SVD, block form.  One workgroup per problem.
//
// The stacked matrix S = [A; V] (mt + me rows) carries the right singular
// vectors along: a rotation J = [[c, s], [-s e^{-i phi}, c e^{-i phi}]] of columns
// (p, q) -- phi = arg(a_p^H a_q), tan(theta) the small root of t^2 + 2 zeta t - 1,
// zeta = (|a_q|^2 - |a_p|^2) / (2 |a_p^H a_q|) -- is applied to all of S, the inner
// products use the A rows only.
//
// Traffic is what bounds this kernel: a plain sweep streams every column pair
// from memory (~80 m^3 bytes per sweep, ~30 sweeps).  So the columns are cut in
// blocks of b; a pair of blocks (2b stacked columns) is staged in LDS, swept
// completely there (round-robin over the 2b columns: b disjoint pairs per step
// on the workgroup's lane groups), and written back; block pairs follow the same
// round-robin ordering.  Memory traffic per sweep drops by ~2.5 b, and when all
// columns fit (me <= 2b, the bulk of the problems) the matrix is loaded once
// and never leaves LDS until it has converged.
//
// The three kernels share everything but the way a sweep visits its column pairs:
// bfJacobiBegin (thresholds, V = I), bfJacobiSweeps (the loop: norms, freeze,
// convergence, bfJacobiFinish) and the arithmetic of a pair (bfColNorm2,
// bfPairDots, bfJacobiAngle, bfJacobiRotate).
// ---------------------------------------------------------------------------
#define BF_JACOBI_MAX_SWEEPS 40

// what a workgroup of any of the three kernels shares besides its columns
struct BfJacobiShared {
  double sigMax;                     // bfJacobiFinish
  double angleDead2;                 // bfJacobiFreeze -> bfJacobiAngle
  unsigned long long maxNormBits;    // bfJacobiMaxNorm2
  uint32_t numLive;                  // columns the sweep rotates
  int rotated;                       // the sweep rotated a pair
};

template <int W> __device__ __forceinline__ double bfGroupSum(double v) {
#pragma unroll
  for (int m = 1; m < W; m <<= 1) v += __shfl_xor(v, m, W);
  return v;
}

// squared norm of col[0..mt) by one group of W lanes (l: the lane's place in it); every lane gets it
template <int W> __device__ __forceinline__ double bfColNorm2(double2 const *col, uint32_t mt, uint32_t l) {
  double s2 = 0;
  for (uint32_t r = l; r < mt; r += W) { double2 const a = col[r]; s2 = fma(a.x, a.x, fma(a.y, a.y, s2)); }
  return bfGroupSum<W>(s2);
}

// the inner products of a column pair by one group of W lanes: alpha = |x|^2, beta = |y|^2, gr + i gi = x^H y
template <int W>
__device__ __forceinline__ void bfPairDots(double2 const *xc, double2 const *yc, uint32_t mt, uint32_t l, double &alpha, double &beta,
                                           double &gr, double &gi) {
  alpha = 0; beta = 0; gr = 0; gi = 0;
  for (uint32_t r = l; r < mt; r += W) {
    double2 const x = xc[r], y = yc[r];
    alpha = fma(x.x, x.x, fma(x.y, x.y, alpha));
    beta = fma(y.x, y.x, fma(y.y, y.y, beta));
    gr = fma(x.x, y.x, fma(x.y, y.y, gr));     // conj(x) * y
    gi = fma(x.x, y.y, fma(-x.y, y.x, gi));
  }
  alpha = bfGroupSum<W>(alpha); beta = bfGroupSum<W>(beta);
  gr = bfGroupSum<W>(gr); gi = bfGroupSum<W>(gi);
}

// pair kk of step s of a round-robin tournament over M (even) players
__device__ __forceinline__ void bfRoundRobin(uint32_t M, uint32_t s, uint32_t kk, uint32_t &p, uint32_t &q) {
  p = kk == 0 ? M - 1 : (s + kk) % (M - 1);
  q = kk == 0 ? s : (s + (M - 1) - kk) % (M - 1);
  if (p > q) { uint32_t const t = p; p = q; q = t; }
}

// singular values, the reference's truncation rule (src/mat_dense_complex.c:1800-1812) and the
// statistics, once the columns of A are orthogonal; col(j): where column j of A is now
template <int W, typename Col>
__device__ void bfJacobiFinish(BfSvdProb const &P, BfSvdStats *stats, int sweep, bool converged, double *sigMaxShared, Col col) {
  uint32_t const mt = P.mt, me = P.me;
  uint32_t const nthreads = blockDim.x, tid = threadIdx.x;
  uint32_t const groups = nthreads / W, g = tid / W, l = tid % W;
  for (uint32_t j = g; j < me; j += groups) {
    double const s2 = bfColNorm2<W>(col(j), mt, l);
    if (l == 0) P.scale[j] = s2;
  }
  __syncthreads();
  // a NaN or an infinity anywhere in A ends in a column norm that is not finite (a rotation carries it along, a frozen
  // column keeps it): such a problem has no answer and counts as not converged, whatever the sweeps said
  if (tid == 0) {
    double mx = 0;
    bool finite = true;
    for (uint32_t j = 0; j < me; ++j) { mx = fmax(mx, P.scale[j]); finite = finite && isfinite(P.scale[j]); }
    *sigMaxShared = finite ? sqrt(mx) : -1.0;
  }
  __syncthreads();
  if (*sigMaxShared < 0.0) converged = false;
  double const eps = 2.220446049250313e-16;
  double const tol = (double)P.dim * eps * *sigMaxShared + eps;
  unsigned long long dropped = 0;
  for (uint32_t j = tid; j < me; j += nthreads) {
    double const s2 = P.scale[j];
    bool const keep = sqrt(s2) >= tol;
    P.scale[j] = keep ? 1.0 / s2 : 0.0;
    dropped += keep ? 0 : 1;
  }
  // statistics only (not part of any result)
  if (dropped) atomicAdd(&stats->truncated, dropped);
  if (tid == 0) {
    atomicMax(&stats->maxSweeps, (unsigned long long)(sweep + (converged ? 1 : 0)));
    atomicAdd(&stats->sumSweeps, (unsigned long long)(sweep + (converged ? 1 : 0)));
    if (!converged) atomicAdd(&stats->notConverged, 1ull);
  }
  if (P.info) {
    __syncthreads();
    if (tid == 0) {
      uint32_t kept = 0;
      for (uint32_t j = 0; j < me; ++j) kept += P.scale[j] != 0.0;
      P.info[0] = (uint32_t)(sweep + (converged ? 1 : 0)); P.info[1] = converged ? 0u : 1u; P.info[2] = kept;
    }
  }
}

// The columns a sweep leaves alone.  A column below the threshold (dead2, squared) is noise, but many of them together can
// carry a singular value well above it: only a set whose squared norms SUM to less than dead2 may be frozen -- the
// Frobenius norm of what is then dropped bounds its 2-norm.  Every column below the threshold when their sum allows it
// (rotations of a pair one of whose columns fell below it during the sweep are then skipped as well: *angleDead2 = dead2);
// else, in column order, those that still fit under the sum, and no pair of live columns is skipped for its norms
// (*angleDead2 = 0).  frozen(j) is written for every j < me.  Thread 0 only.
template <typename F>
__device__ void bfJacobiFreeze(double const *s2, uint32_t me, double dead2, double *angleDead2, F frozen) {
  double small = 0;
  for (uint32_t j = 0; j < me; ++j)
    if (s2[j] < dead2) small += s2[j];
  if (small < dead2) {
    *angleDead2 = dead2;
    for (uint32_t j = 0; j < me; ++j) frozen(j, !(s2[j] >= dead2));
    return;
  }
  *angleDead2 = 0.0;
  double acc = 0;
  for (uint32_t j = 0; j < me; ++j) {
    bool const f = s2[j] < dead2 && acc + s2[j] < dead2;
    if (f) acc += s2[j];
    frozen(j, f);
  }
}

// largest squared column norm of A (a lower bound of sigma_max^2), order-independent
template <int W>
__device__ double bfJacobiMaxNorm2(BfSvdProb const &P, unsigned long long *maxBitsShared) {
  uint32_t const mt = P.mt, me = P.me;
  double2 const *A = (double2 const *)P.a;
  uint32_t const nthreads = blockDim.x, tid = threadIdx.x;
  uint32_t const groups = nthreads / W, g = tid / W, l = tid % W;
  if (tid == 0) *maxBitsShared = 0;
  __syncthreads();
  for (uint32_t j = g; j < me; j += groups) {
    double const s2 = bfColNorm2<W>(A + (uint64_t)j * mt, mt, l);
    if (l == 0) atomicMax(maxBitsShared, (unsigned long long)__double_as_longlong(s2));
  }
  __syncthreads();
  return __longlong_as_double((long long)*maxBitsShared);
}

// rotation of a column pair from its inner products (alpha, beta, gamma); false: below the threshold
__device__ __forceinline__ bool bfJacobiAngle(double alpha, double beta, double gr, double gi, double tol2, double dead2,
                                               double &c, double &sn, double &er, double &ei) {
  double const g2 = gr * gr + gi * gi;
  if (alpha < dead2 || beta < dead2) return false;
  if (!(g2 > tol2 * alpha * beta) || g2 == 0.0) return false;
  double const gabs = sqrt(g2);
  double const zeta = (beta - alpha) / (2.0 * gabs);
  double const t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  c = 1.0 / sqrt(1.0 + t * t); sn = c * t;
  er = gr / gabs; ei = -gi / gabs;                // e^{-i phi}
  return true;
}

// one row of a rotated pair: yt = e y, x' = c x - s yt, y' = s x + c yt with e = er + i ei = e^{-i phi} (columns), or its
// conjugate where the caller passes -ei (rows of a Gram matrix)
__device__ __forceinline__ void bfJacobiRotate(double2 *xp, double2 *yp, double c, double sn, double er, double ei) {
  double2 const x = *xp, y = *yp;
  double2 const yt = make_double2(er * y.x - ei * y.y, er * y.y + ei * y.x);
  *xp = make_double2(c * x.x - sn * yt.x, c * x.y - sn * yt.y);
  *yp = make_double2(sn * x.x + c * yt.x, sn * x.y + c * yt.y);
}

// The thresholds of a problem, and V = I in memory when asked (the resident plain kernel builds it in its tile).
// tol2: a pair is rotated while |a_p^H a_q|^2 > tol2 |a_p|^2 |a_q|^2 (xGESVJ: sqrt(mt) eps).
// dead2: columns below the truncation threshold (relative to the largest column norm, a lower bound of sigma_max) are
// never rotated: they will be dropped, and what they carry is below the rounding error of the matrix.  Left alone they
// would keep the sweeps busy orthogonalising noise.  A column that is never rotated never changes, so it stays below:
// every sweep starts by finding the columns still above the threshold (bfJacobiFreeze) and visits the pairs of those
// only (with half of the columns frozen, a quarter of the pairs).
template <int W>
__device__ __forceinline__ void bfJacobiBegin(BfSvdProb const &P, BfJacobiShared &sh, bool initV, double &tol2, double &dead2) {
  uint32_t const me = P.me;
  tol2 = (double)P.mt * 2.220446049250313e-16 * 2.220446049250313e-16;
  double const deadRel = (double)P.dim * 2.220446049250313e-16;
  dead2 = deadRel * deadRel * bfJacobiMaxNorm2<W>(P, &sh.maxNormBits);
  if (!initV) return;
  double2 *V = (double2 *)P.v;
  for (uint64_t e = threadIdx.x; e < (uint64_t)me * me; e += blockDim.x) V[e] = make_double2((e % me == e / me) ? 1.0 : 0.0, 0.0);
}

// The iteration of all three kernels: up to BF_JACOBI_MAX_SWEEPS sweeps, then bfJacobiFinish.  A sweep: the squared column
// norms into P.scale (free until the end), bfJacobiFreeze on them by thread 0, the kernel's visit of the pairs; a visit
// that rotated nothing ends the iteration.  The kernel supplies
//   col(j)           where column j of A is (its tile slot for the resident plain kernel, memory otherwise);
//   record(j, f, n)  column j is frozen (f) or the n-th live one: a live list, or a mark in P.scale -- the pair order of a
//                    sweep, and so every result, depends on which;
//   visit(nLive)     the rotations of one sweep: sets sh.rotated if there was one, ends on a barrier.
// LIVE_LIST: the visit runs over the live columns only, and fewer than two of them end the iteration.  The global-memory
// kernel visits all pairs, skips by the marks and has no such exit.  me == 0: the plain and the Gram kernel return before
// they touch anything; the global-memory kernel gets here, and bfJacobiFinish counts one sweep and writes P.info.
template <int W, bool LIVE_LIST, typename Col, typename Record, typename Visit>
__device__ __forceinline__ void bfJacobiSweeps(BfSvdProb const &P, BfSvdStats *stats, BfJacobiShared &sh, double dead2, Col col, Record record,
                                               Visit visit) {
  uint32_t const mt = P.mt, me = P.me;
  uint32_t const tid = threadIdx.x, groups = blockDim.x / W, g = tid / W, l = tid % W;
  int sweep = 0;
  bool converged = false;
  __syncthreads();
  for (; sweep < BF_JACOBI_MAX_SWEEPS; ++sweep) {
    for (uint32_t j = g; j < me; j += groups) {
      double const s2 = bfColNorm2<W>(col(j), mt, l);
      if (l == 0) P.scale[j] = s2;
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t n = 0;
      bfJacobiFreeze(P.scale, me, dead2, &sh.angleDead2, [&](uint32_t j, bool f) { record(j, f, n); n += f ? 0 : 1; });
      sh.numLive = n;
      sh.rotated = 0;
    }
    __syncthreads();
    uint32_t const nLive = sh.numLive;
    if (LIVE_LIST && nLive < 2) { converged = true; break; }
    visit(nLive);
    converged = sh.rotated == 0;
    __syncthreads();
    if (converged) break;
  }
  bfJacobiFinish<W>(P, stats, sweep, converged, &sh.sigMax, col);
}

template <int W>
__global__ __launch_bounds__(1024) void bfJacobiKernel(BfSvdProb const *probs, uint32_t const *list, BfSvdStats *stats, uint32_t ldsBytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bfJacobiLds[];
  double2 *tile = (double2 *)bfJacobiLds;
  __shared__ BfJacobiShared sh;
  __shared__ uint16_t live[BF_JACOBI_MAX_COLS];     // the columns a sweep rotates (bfJacobiFreeze), in column order
  BfSvdProb const P = probs[list[blockIdx.x]];
  uint32_t const mt = P.mt, me = P.me;
  if (me == 0) return;                              // rank 0 after the QR preconditioner: nothing to orthogonalise
  double2 *A = (double2 *)P.a, *V = (double2 *)P.v;
  uint32_t const nthreads = blockDim.x, tid = threadIdx.x;
  uint32_t const groups = nthreads / W, g = tid / W, l = tid % W;
  BfJacobiTile const T = bfJacobiTile(ldsBytes, mt, me);
  uint32_t const R = mt + me, Rp = T.Rp, b = T.b;
  bool const resident = T.resident;                 // everything fits: loaded once, slot = column
  double tol2, dead2;
  bfJacobiBegin<W>(P, sh, !resident, tol2, dead2);

  // one column pair held in the tile at slots (p, q): inner products over the A rows, rotation of all R rows
  auto rotatePair = [&](uint32_t p, uint32_t q) {
    double2 *sp = tile + p * Rp, *sq = tile + q * Rp;
    double alpha, beta, gr, gi, c, sn, er, ei;
    bfPairDots<W>(sp, sq, mt, l, alpha, beta, gr, gi);
    if (!bfJacobiAngle(alpha, beta, gr, gi, tol2, sh.angleDead2, c, sn, er, ei)) return;
    for (uint32_t r = l; r < R; r += W) bfJacobiRotate(sp + r, sq + r, c, sn, er, ei);
    if (l == 0) sh.rotated = 1;
  };
  // resident: round robin over the live columns, in place
  auto sweepResident = [&](uint32_t nLive) {
    uint32_t const M = nLive + (nLive & 1u);
    for (uint32_t s = 0; s + 1 < M; ++s) {
      for (uint32_t kk = g; kk < M / 2; kk += groups) {
        uint32_t p, q;
        bfRoundRobin(M, s, kk, p, q);
        if (q >= nLive) continue;                  // the dummy player of an odd count
        rotatePair(live[p], live[q]);
      }
      __syncthreads();
    }
  };
  // else: round robin over the blocks of b live columns, a pair of blocks staged in the tile at a time
  auto sweepBlocks = [&](uint32_t nLive) {
    uint32_t nb = (nLive + b - 1) / b;
    nb = nb < 2 ? 2 : nb;
    uint32_t const NB = nb + (nb & 1u);
    for (uint32_t S = 0; S + 1 < NB; ++S) {
      for (uint32_t KK = 0; KK < NB / 2; ++KK) {
        uint32_t I, J;
        bfRoundRobin(NB, S, KK, I, J);
        if (J >= nb) continue;                       // the dummy block of an odd block count
        // slot of the staged block pair (I, J) of the live list -> global column; none: 0xffffffff
        auto slotCol = [&](uint32_t slot) -> uint32_t {
          uint32_t const blk = slot < b ? I : J, off = slot < b ? slot : slot - b;
          uint32_t const a = blk * b + off;
          return a < nLive ? (uint32_t)live[a] : 0xffffffffu;
        };
        for (uint32_t e = tid; e < 2 * b * R; e += nthreads) {
          uint32_t const slot = e / R, r = e - slot * R;
          uint32_t const c = slotCol(slot);
          if (c == 0xffffffffu) continue;
          tile[slot * Rp + r] = r < mt ? A[(uint64_t)c * mt + r] : V[(uint64_t)c * me + (r - mt)];
        }
        __syncthreads();
        // one complete sweep over the 2b staged columns
        for (uint32_t s = 0; s + 1 < 2 * b; ++s) {
          for (uint32_t kk = g; kk < b; kk += groups) {
            uint32_t p, q;
            bfRoundRobin(2 * b, s, kk, p, q);
            if (slotCol(p) == 0xffffffffu || slotCol(q) == 0xffffffffu) continue;
            rotatePair(p, q);
          }
          __syncthreads();
        }
        for (uint32_t e = tid; e < 2 * b * R; e += nthreads) {
          uint32_t const slot = e / R, r = e - slot * R;
          uint32_t const c = slotCol(slot);
          if (c == 0xffffffffu) continue;
          double2 const v = tile[slot * Rp + r];
          if (r < mt) A[(uint64_t)c * mt + r] = v; else V[(uint64_t)c * me + (r - mt)] = v;
        }
        __syncthreads();
      }
    }
  };

  // resident: [A; I] into the tile before the iteration, [U Sigma; V] out of it after
  if (resident) {
    for (uint32_t e = tid; e < me * R; e += nthreads) {
      uint32_t const c = e / R, r = e - c * R;
      tile[c * Rp + r] = r < mt ? A[(uint64_t)c * mt + r] : make_double2(r - mt == c ? 1.0 : 0.0, 0.0);
    }
  }
  bfJacobiSweeps<W, true>(
      P, stats, sh, dead2, [=](uint32_t j) -> double2 const * { return resident ? tile + j * Rp : A + (uint64_t)j * mt; },
      [&](uint32_t j, bool f, uint32_t n) { if (!f) live[n] = (uint16_t)j; },
      [&](uint32_t nLive) { if (resident) sweepResident(nLive); else sweepBlocks(nLive); });
  if (resident) {
    for (uint32_t e = tid; e < me * R; e += nthreads) {
      uint32_t const c = e / R, r = e - c * R;
      double2 const v = tile[c * Rp + r];
      if (r < mt) A[(uint64_t)c * mt + r] = v; else V[(uint64_t)c * me + (r - mt)] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// Block form for the problems whose stacked columns are long for the LDS tile (rows + columns >= 512: only 2 - 8
// stacked columns of a block fit, an inner step keeps 2 - 5 of 16 wavefronts busy and every block pair is a round trip
// of its columns for a handful of rotations).  Here a block is 16 columns whatever their length.  For a pair of blocks
// (32 columns Xp):
//   A. G = Xp^H Xp, 32 x 32, one pass over the rows (32-row chunks staged in LDS, 4 x 4 register blocks, 8 row slices;
//      accumulating only the upper triangle -- 36 blocks x 14 slices -- measured no faster);
//   B. two-sided Jacobi on G in LDS (16 disjoint rotations per round-robin step, four to a wavefront on each of the four
//      SIMDs, 16 lanes each; the same rotation formula and the same thresholds as the scalar kernel -- the inner products it would
//      compute are the entries of G), one sweep, the rotations accumulated in Q (32 x 32);
//   C. [Xp; Vp] <- [Xp; Vp] Q, one thread per row, the row's 32 values in registers, Q broadcast from LDS.
// The next outer sweep forms every G afresh from the columns, so what an inner solve leaves undone (its later rotations
// use updated, not recomputed, inner products) is met again; a sweep in which no fresh G holds a pair above the
// threshold ends the iteration, exactly the scalar kernel's criterion.  (CPU prototype on re-expansion matrices of
// 160 - 300 columns: 6 - 9 outer sweeps against 9 scalar ones, V orthogonal to 1e-13.)  Traffic per sweep falls by
// the block size over the tile's 2 - 5 columns, and the arithmetic is two GEMM-shaped passes all wavefronts share.
// ---------------------------------------------------------------------------
#define BF_GRAM_NB 16
#define BF_GRAM_P 32
#define BF_GRAM_THREADS 512
#define BF_GRAM_RC 32
#define BF_GRAM_LD 33
#define BF_GRAM_NONE 0xffffu
#define BF_GRAM_INNER 1                  /* sweeps of the inner solve per visit of a block pair (2: 10.2 instead of 10.5 outer sweeps on
                                          * average, but the solve -- then by one wavefront -- was half of a visit's time: 4.66 against 3.76 s per batch) */


__global__ __launch_bounds__(BF_GRAM_THREADS) void bfJacobiGramKernel(BfSvdProb const *probs, uint32_t const *list, BfSvdStats *stats) {
  constexpr int W = 64;
  __shared__ __attribute__((aligned(16))) double2 G[BF_GRAM_P * BF_GRAM_LD];
  __shared__ __attribute__((aligned(16))) double2 Q[BF_GRAM_P * BF_GRAM_LD];
  __shared__ __attribute__((aligned(16))) double2 tile[BF_GRAM_P * BF_GRAM_LD];      // [column][row of the chunk]
  __shared__ uint16_t live[BF_GRAM_MAX_COLS];
  __shared__ uint16_t pcol[BF_GRAM_P];
  __shared__ BfJacobiShared sh;
  __shared__ int pairRot;
  BfSvdProb const P = probs[list[blockIdx.x]];
  uint32_t const mt = P.mt, me = P.me;
  if (me == 0) return;
  double2 *A = (double2 *)P.a, *V = (double2 *)P.v;
  uint32_t const nthreads = blockDim.x, tid = threadIdx.x;
  double tol2, dead2;
  bfJacobiBegin<W>(P, sh, true, tol2, dead2);
  // round robin over the blocks of 16 live columns
  auto sweepBlocks = [&](uint32_t nLive) {
    uint32_t nb = (nLive + BF_GRAM_NB - 1) / BF_GRAM_NB;
    nb = nb < 2 ? 2 : nb;
    uint32_t const NBk = nb + (nb & 1u);
    for (uint32_t S = 0; S + 1 < NBk; ++S) {
      for (uint32_t KK = 0; KK < NBk / 2; ++KK) {
        uint32_t I, J;
        bfRoundRobin(NBk, S, KK, I, J);
        if (J >= nb) continue;
        if (tid < BF_GRAM_P) {
          uint32_t const a = (tid < BF_GRAM_NB ? I : J) * BF_GRAM_NB + (tid % BF_GRAM_NB);
          pcol[tid] = a < nLive ? live[a] : (uint16_t)BF_GRAM_NONE;
        }
        for (uint32_t e = tid; e < BF_GRAM_P * BF_GRAM_LD; e += nthreads) {
          G[e] = make_double2(0.0, 0.0);
          uint32_t const i = e / BF_GRAM_LD, j = e - i * BF_GRAM_LD;
          Q[e] = make_double2(i == j ? 1.0 : 0.0, 0.0);
        }
        if (tid == 0) pairRot = 0;
        __syncthreads();
        // ---- A: the Gram matrix of the pair's columns
        {
          uint32_t const slice = tid / 64, w = tid % 64, bp = w / 8, bq = w % 8;
          double ar[4][4], ai[4][4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) { ar[i][j] = 0; ai[i][j] = 0; }
          for (uint32_t r0 = 0; r0 < mt; r0 += BF_GRAM_RC) {
#pragma unroll
            for (int k = 0; k < (BF_GRAM_P * BF_GRAM_RC) / BF_GRAM_THREADS; ++k) {
              uint32_t const e = tid + BF_GRAM_THREADS * k, c = e / BF_GRAM_RC, r = e % BF_GRAM_RC;
              uint32_t const col = pcol[c];
              double2 v = make_double2(0.0, 0.0);
              if (col != BF_GRAM_NONE && r0 + r < mt) v = A[(uint64_t)col * mt + r0 + r];
              tile[c * BF_GRAM_LD + r] = v;
            }
            __syncthreads();
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              uint32_t const r = slice * 4 + rr;
              double2 a[4], b[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) { a[i] = tile[(4 * bp + i) * BF_GRAM_LD + r]; b[i] = tile[(4 * bq + i) * BF_GRAM_LD + r]; }
#pragma unroll
              for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {            // conj(a) * b
                  ar[i][j] = fma(a[i].x, b[j].x, fma(a[i].y, b[j].y, ar[i][j]));
                  ai[i][j] = fma(a[i].x, b[j].y, fma(-a[i].y, b[j].x, ai[i][j]));
                }
            }
            __syncthreads();
          }
          for (uint32_t sl = 0; sl < BF_GRAM_THREADS / 64; ++sl) {      // the row slices added in a fixed order
            if (slice == sl) {
#pragma unroll
              for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                  double2 &gg = G[(4 * bp + i) * BF_GRAM_LD + 4 * bq + j];
                  gg = make_double2(gg.x + ar[i][j], gg.y + ai[i][j]);
                }
            }
            __syncthreads();
          }
        }
        // ---- B: two-sided Jacobi on G; Q accumulates the rotations.  Wavefronts 0 - 3 (one per SIMD) take four of the 16
        // disjoint rotations of a round-robin step each, 16 lanes per rotation; the others only keep the barriers.
        {
          bool const worker = tid < 256;
          uint32_t const kk = tid / 16, sub = tid % 16;
          for (int inner = 0; inner < BF_GRAM_INNER; ++inner) {
            for (uint32_t s = 0; s + 1 < BF_GRAM_P; ++s) {
              uint32_t p = 0, q = 1;
              double c = 1, sn = 0, er = 1, ei = 0;
              bool rot = false;
              if (worker) {
                bfRoundRobin(BF_GRAM_P, s, kk, p, q);
                double2 const gpq = G[p * BF_GRAM_LD + q];
                rot = bfJacobiAngle(G[p * BF_GRAM_LD + p].x, G[q * BF_GRAM_LD + q].x, gpq.x, gpq.y, tol2, sh.angleDead2, c, sn, er, ei);
              }
              __syncthreads();                                       // every rotation of the step has read its inputs
              if (rot) {
                if (inner == 0 && sub == 0) { pairRot = 1; sh.rotated = 1; }
#pragma unroll
                for (int t = 0; t < BF_GRAM_P / 16; ++t) {                // columns p, q of G and of Q
                  uint32_t const i = sub + 16 * t;
                  bfJacobiRotate(&G[i * BF_GRAM_LD + p], &G[i * BF_GRAM_LD + q], c, sn, er, ei);
                  bfJacobiRotate(&Q[i * BF_GRAM_LD + p], &Q[i * BF_GRAM_LD + q], c, sn, er, ei);
                }
              }
              __syncthreads();
              if (rot) {
#pragma unroll
                for (int t = 0; t < BF_GRAM_P / 16; ++t) {                // rows p, q of G: J^H G, conj(e) on row q
                  uint32_t const j = sub + 16 * t;
                  bfJacobiRotate(&G[p * BF_GRAM_LD + j], &G[q * BF_GRAM_LD + j], c, sn, er, -ei);
                }
              }
              __syncthreads();
            }
          }
        }
        __syncthreads();
        // ---- C: the pair's columns of [X; V] times Q
        if (pairRot) {
          uint32_t const R = mt + me;
          for (uint32_t row0 = 0; row0 < R; row0 += nthreads) {
            uint32_t const row = row0 + tid;
            if (row < R) {
              double2 *base = row < mt ? A + row : V + (row - mt);
              uint64_t const ld = row < mt ? mt : me;
              double2 x[BF_GRAM_P];
#pragma unroll
              for (int k = 0; k < BF_GRAM_P; ++k) {
                uint32_t const col = pcol[k];
                x[k] = col != BF_GRAM_NONE ? base[(uint64_t)col * ld] : make_double2(0.0, 0.0);
              }
#pragma unroll 4
              for (int c = 0; c < BF_GRAM_P; ++c) {
                uint32_t const col = pcol[c];
                if (col == BF_GRAM_NONE) continue;
                double yr = 0, yi = 0;
#pragma unroll
                for (int k = 0; k < BF_GRAM_P; ++k) {
                  double2 const qk = Q[k * BF_GRAM_LD + c];
                  yr = fma(x[k].x, qk.x, fma(-x[k].y, qk.y, yr));
                  yi = fma(x[k].x, qk.y, fma(x[k].y, qk.x, yi));
                }
                base[(uint64_t)col * ld] = make_double2(yr, yi);
              }
            }
          }
        }
        __syncthreads();
      }
    }
  };
  bfJacobiSweeps<W, true>(
      P, stats, sh, dead2, [=](uint32_t j) -> double2 const * { return A + (uint64_t)j * mt; },
      [&](uint32_t j, bool f, uint32_t n) { if (!f) live[n] = (uint16_t)j; }, sweepBlocks);
}

// Fallback for problems whose stacked column pair does not fit the LDS tile (check points +
// equivalent sources > ~4600): the same sweeps straight out of global memory, one column pair per
// 64-lane group of a 1024-thread workgroup.  Slow (every rotation streams its columns), but total.
// There is no bound on the columns, so no live list in LDS: the frozen columns of a sweep are marked
// P.scale[j] < 0 (scratch until bfJacobiFinish) and the round robin runs over all me columns.
__global__ __launch_bounds__(1024) void bfJacobiGlobalKernel(BfSvdProb const *probs, uint32_t const *list, BfSvdStats *stats) {
  constexpr int W = 64;
  __shared__ BfJacobiShared sh;
  BfSvdProb const P = probs[list[blockIdx.x]];
  uint32_t const mt = P.mt, me = P.me;
  double2 *A = (double2 *)P.a, *V = (double2 *)P.v;
  uint32_t const groups = blockDim.x / W, g = threadIdx.x / W, l = threadIdx.x % W;
  double tol2, dead2;
  bfJacobiBegin<W>(P, sh, true, tol2, dead2);
  uint32_t const M = me + (me & 1u);
  auto sweepAll = [&](uint32_t) {
    for (uint32_t s = 0; s + 1 < M; ++s) {
      for (uint32_t kk = g; kk < M / 2; kk += groups) {
        uint32_t p, q;
        bfRoundRobin(M, s, kk, p, q);
        if (q >= me) continue;                       // the dummy column of an odd me
        if (P.scale[p] < 0.0 || P.scale[q] < 0.0) continue;
        double2 *ap = A + (uint64_t)p * mt, *aq = A + (uint64_t)q * mt;
        double alpha, beta, gr, gi, c, sn, er, ei;
        bfPairDots<W>(ap, aq, mt, l, alpha, beta, gr, gi);
        if (!bfJacobiAngle(alpha, beta, gr, gi, tol2, sh.angleDead2, c, sn, er, ei)) continue;
        double2 *vp = V + (uint64_t)p * me, *vq = V + (uint64_t)q * me;
        for (uint32_t r = l; r < mt + me; r += W)
          bfJacobiRotate(r < mt ? ap + r : vp + (r - mt), r < mt ? aq + r : vq + (r - mt), c, sn, er, ei);
        if (l == 0) sh.rotated = 1;
      }
      __syncthreads();
    }
  };
  bfJacobiSweeps<W, false>(
      P, stats, sh, dead2, [=](uint32_t j) -> double2 const * { return A + (uint64_t)j * mt; },
      [&](uint32_t j, bool f, uint32_t) { if (f) P.scale[j] = -1.0; }, sweepAll);
}

// ---------------------------------------------------------------------------
// Preconditioner of the Jacobi SVD for the problems that do not fit LDS (Drmac & Veselic's
// scheme, first stage): Householder QR with column pivoting  A P = Q R,  stopped at the first step
// whose trailing columns together (their squared norms summed) are below the threshold under which the Jacobi
// kernel freezes columns (r steps): the Frobenius norm of the trailing block bounds the 2-norm of what is dropped.  The right-hand side B rides along as extra, never pivoted
// columns and leaves as Q^H B.  What the Jacobi kernel then orthogonalises is
//   X = (R[0:r, :] P^T)^H      (me x r, rows in the ORIGINAL column order of A),
// whose columns are already graded and few: X V1 = W (orthogonal columns, norms sigma)  gives
//   A ~ (Q[:, 0:r] V1) (W^H)  and  pinv(A) B = W diag(1/sigma^2) V1^H (Q^H B)[0:r, :].
// One workgroup per problem; a column of the trailing matrix per 64-lane group (its segment in
// registers between the dot product and the update when it has <= 1024 rows); the squared norm
// of every updated column is accumulated from the updated values themselves, so the pivot
// choice never sees a downdated norm.  The reflector lives in LDS.  All orders are fixed.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(512) void bfQrcpKernel(BfQrProb const *probs, uint32_t *ranks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bfQrLds[];
  constexpr int W = 64;
  BfQrProb const P = probs[blockIdx.x];
  uint32_t const mt = P.mt, me = P.me, n = P.n;
  double2 *A = (double2 *)P.a, *B = (double2 *)P.b, *X = (double2 *)P.x;
  double2 *u = (double2 *)bfQrLds;                       // [mt]
  double *cn = (double *)(u + mt);                       // [me] squared norms of rows j.. of the columns
  uint32_t *perm = (uint32_t *)(cn + me);                // [me]
  __shared__ double redVal[16], redSum[16];
  __shared__ uint32_t redIdx[16];
  __shared__ double sCoef, sDead2, sTotal;
  __shared__ int sNonFinite;
  __shared__ uint32_t sPivot;
  uint32_t const nthreads = blockDim.x, tid = threadIdx.x;
  uint32_t const groups = nthreads / W, g = tid / W, l = tid % W;

  // largest cn[c], c >= from (lowest index among equals) -> sPivot; every thread gets the value.  The sum of those cn[c]
  // -> sTotal (fixed order: lane strides, a butterfly, the groups in turn)
  auto argmax = [&](uint32_t from) -> double {
    double bv = -1.0, sum = 0.0; uint32_t bi = 0xffffffffu;
    for (uint32_t c = from + tid; c < me; c += nthreads) { double const v = cn[c]; sum += v; if (v > bv) { bv = v; bi = c; } }
#pragma unroll
    for (int m = 1; m < W; m <<= 1) {
      double const ov = __shfl_xor(bv, m, W); uint32_t const oi = __shfl_xor(bi, m, W);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    sum = bfGroupSum<W>(sum);
    if (l == 0) { redVal[g] = bv; redIdx[g] = bi; redSum[g] = sum; }
    __syncthreads();
    if (tid == 0) {
      for (uint32_t k = 1; k < groups; ++k) {
        if (redVal[k] > bv || (redVal[k] == bv && redIdx[k] < bi)) { bv = redVal[k]; bi = redIdx[k]; }
        sum += redSum[k];
      }
      redVal[0] = bv; sPivot = bi; sTotal = sum;
    }
    __syncthreads();
    return redVal[0];
  };

  if (tid == 0) sNonFinite = 0;
  __syncthreads();
  for (uint32_t c = g; c < me; c += groups) {
    double const s2 = bfColNorm2<W>(A + (uint64_t)c * mt, mt, l);
    if (l == 0) { cn[c] = s2; perm[c] = c; if (!isfinite(s2)) sNonFinite = 1; }
  }
  __syncthreads();
  {
    double const mx = argmax(0);
    double const deadRel = (double)P.dim * 2.220446049250313e-16;
    if (tid == 0) sDead2 = deadRel * deadRel * mx;
    __syncthreads();
  }
  uint32_t const steps = sNonFinite ? 0 : mt < me ? mt : me;      // not finite: nothing to factor, the problem is flagged
  uint32_t j = 0;
  for (; j < steps; ++j) {
    double const best = argmax(j);
    if (!(sTotal >= sDead2) || best <= 0.0) break;     // what is left is below the threshold together
    uint32_t const p = sPivot;
    if (p != j) {
      double2 *aj = A + (uint64_t)j * mt, *ap = A + (uint64_t)p * mt;
      for (uint32_t r = tid; r < mt; r += nthreads) { double2 const t = aj[r]; aj[r] = ap[r]; ap[r] = t; }
      if (tid == 0) { double const t = cn[j]; cn[j] = cn[p]; cn[p] = t; uint32_t const q = perm[j]; perm[j] = perm[p]; perm[p] = q; }
    }
    __syncthreads();
    // reflector H = I - coef u u^H with u = x + e^{i arg x0} |x| e_1:  H x = -e^{i arg x0} |x| e_1
    uint32_t const L = mt - j;
    double2 *aj = A + (uint64_t)j * mt + j;
    for (uint32_t i = tid; i < L; i += nthreads) u[i] = aj[i];
    __syncthreads();
    if (tid == 0) {
      double2 const x0 = u[0];
      double const nx = sqrt(best), a0 = hypot(x0.x, x0.y);
      double const pr = a0 > 0.0 ? x0.x / a0 : 1.0, pi = a0 > 0.0 ? x0.y / a0 : 0.0;
      u[0] = make_double2(x0.x + pr * nx, x0.y + pi * nx);
      sCoef = 1.0 / (nx * (nx + a0));                  // 2 / (u^H u)
      aj[0] = make_double2(-pr * nx, -pi * nx);          // R[j][j]
    }
    __syncthreads();
    double const coef = sCoef;
    uint32_t const trailing = me - j - 1, cols = trailing + n;
    for (uint32_t c = g; c < cols; c += groups) {
      double2 *col = c < trailing ? A + (uint64_t)(j + 1 + c) * mt + j : B + (uint64_t)(c - trailing) * mt + j;
      double sr = 0, si = 0, nn = 0;
      if (L <= 16 * W) {
        double2 v[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          uint32_t const i = l + W * t;
          v[t] = i < L ? col[i] : make_double2(0.0, 0.0);
          double2 const ui = i < L ? u[i] : make_double2(0.0, 0.0);
          sr = fma(ui.x, v[t].x, fma(ui.y, v[t].y, sr));     // conj(u) * v
          si = fma(ui.x, v[t].y, fma(-ui.y, v[t].x, si));
        }
        sr = bfGroupSum<W>(sr) * coef; si = bfGroupSum<W>(si) * coef;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          uint32_t const i = l + W * t;
          if (i < L) {
            double2 const ui = u[i];
            double2 const w = make_double2(v[t].x - (sr * ui.x - si * ui.y), v[t].y - (sr * ui.y + si * ui.x));
            col[i] = w;
            if (i) nn = fma(w.x, w.x, fma(w.y, w.y, nn));
          }
        }
      } else {
        for (uint32_t i = l; i < L; i += W) {
          double2 const ui = u[i], x = col[i];
          sr = fma(ui.x, x.x, fma(ui.y, x.y, sr));
          si = fma(ui.x, x.y, fma(-ui.y, x.x, si));
        }
        sr = bfGroupSum<W>(sr) * coef; si = bfGroupSum<W>(si) * coef;
        for (uint32_t i = l; i < L; i += W) {
          double2 const ui = u[i], x = col[i];
          double2 const w = make_double2(x.x - (sr * ui.x - si * ui.y), x.y - (sr * ui.y + si * ui.x));
          col[i] = w;
          if (i) nn = fma(w.x, w.x, fma(w.y, w.y, nn));
        }
      }
      nn = bfGroupSum<W>(nn);
      if (l == 0 && c < trailing) cn[j + 1 + c] = nn;
    }
    __syncthreads();
  }
  uint32_t const r = j;
  if (tid == 0) ranks[blockIdx.x] = r | (sNonFinite ? BF_QR_NONFINITE : 0u);
  // X[perm[c] + i me] = conj(R[i][c]), i <= c; zero below the diagonal of R
  for (uint32_t c = g; c < me; c += groups) {
    double2 const *rc = A + (uint64_t)c * mt;
    uint32_t const row = perm[c];
    for (uint32_t i = l; i < r; i += W) {
      double2 v = make_double2(0.0, 0.0);
      if (i <= c) { v = rc[i]; v.y = -v.y; }
      X[(uint64_t)i * me + row] = v;
    }
  }
}

int bfdevQrcpFits(uint32_t mt, uint32_t me) { return bfQrcpLds(mt, me) != 0; }

typedef struct QrOrder { double cost; uint32_t idx; int cls; } QrOrder;
static int qrOrderCmp(void const *pa, void const *pb) {
  QrOrder const *a = (QrOrder const *)pa, *b = (QrOrder const *)pb;
  if (a->cls != b->cls) return a->cls < b->cls ? -1 : 1;
  if (a->cost != b->cost) return a->cost > b->cost ? -1 : 1;
  return a->idx < b->idx ? -1 : 1;
}

// one launch per LDS class (several small problems then share a CU)
int bfdevBuildQrcp(BfQrProb const *hostProbs, uint64_t numProbs, uint32_t *hostRanks) {
  if (!numProbs) return 0;
  enum { NC = BF_QR_LDS_CLASSES };                       /* <= 8, 16, 32, 64, 128, 150 KiB (bfLstSqRoute) */
  uint32_t *order = (uint32_t *)malloc(numProbs * sizeof(uint32_t));
  BfQrProb *sorted = (BfQrProb *)malloc(numProbs * sizeof(BfQrProb));
  uint32_t *ranks = (uint32_t *)malloc(numProbs * sizeof(uint32_t));
  uint64_t count[NC + 1] = {0};
  int rc = order && sorted && ranks ? 0 : bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  QrOrder *ord = (QrOrder *)malloc(numProbs * sizeof(QrOrder));
  if (!rc && !ord) rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  for (uint64_t i = 0; i < numProbs && !rc; ++i) {
    uint32_t const need = bfQrcpLds(hostProbs[i].mt, hostProbs[i].me);
    if (!need) { rc = bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "QR preconditioner: problem %llu does not fit LDS", (unsigned long long)i); break; }
    int const c = (int)bfQrcpLdsClass(need);
    ord[i].cls = c; ord[i].idx = (uint32_t)i;
    ord[i].cost = (double)hostProbs[i].mt * hostProbs[i].me * (hostProbs[i].me + hostProbs[i].n);
    count[c + 1] += 1;
  }
  for (int c = 0; c < NC; ++c) count[c + 1] += count[c];
  if (!rc) {
    // by LDS class, the longest first within a class (dispatch order: the tail of a launch is made of cheap problems)
    qsort(ord, numProbs, sizeof(QrOrder), qrOrderCmp);
    for (uint64_t at = 0; at < numProbs; ++at) { sorted[at] = hostProbs[ord[at].idx]; order[ord[at].idx] = (uint32_t)at; }
  }
  free(ord);
  BfQrProb *dP = NULL;
  uint32_t *dR = NULL;
  if (!rc) rc = uploadArrayB(&dP, sorted, numProbs, "qr problems");
  if (!rc) rc = bfHipFail(hipMalloc((void **)&dR, numProbs * sizeof(uint32_t)), "qr ranks");
  if (!rc) rc = bfHipFail(hipFuncSetAttribute((void const *)bfQrcpKernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bfQrcpLdsCap(NC - 1)), "hipFuncSetAttribute(QR LDS)");
  for (int c = NC - 1; c >= 0 && !rc; --c) {              /* the big ones first */
    uint64_t const nc = count[c + 1] - count[c];
    if (!nc) continue;
    uint32_t const threads = c >= 2 ? 512 : 256;          /* LDS class ~ rows: short columns need few lane groups */
    hipLaunchKernelGGL(bfQrcpKernel, dim3((uint32_t)nc), dim3(threads), bfQrcpLdsCap(c), 0, dP + count[c], dR + count[c]);
    rc = bfHipFail(hipGetLastError(), "QR preconditioner launch");
  }
  if (!rc) rc = bfHipFail(hipDeviceSynchronize(), "QR preconditioner");
  if (!rc) rc = bfHipFail(hipMemcpy(ranks, dR, numProbs * sizeof(uint32_t), hipMemcpyDeviceToHost), "qr ranks");
  for (uint64_t i = 0; i < numProbs && !rc; ++i) hostRanks[i] = ranks[order[i]];
  (void)hipFree(dP); (void)hipFree(dR);
  free(order); free(sorted); free(ranks);
  return rc;
}

// Launch classes (bfJacobiRoute, bfhip_internal.h).  Workgroup: 256 threads for <= 64 columns, 1024 above.  LDS: the
// smallest of 16/32/64/144 KiB that holds the whole stacked matrix (several small problems then share a CU), else 144 KiB
// and block sweeps.  Lane-group width W: the largest power of two that still gives each of the b column pairs of an inner
// step its own group, at most the column length.
template <int W> static int jacobiLaunch(uint32_t count, uint32_t threads, uint32_t lds, BfSvdProb const *dP, uint32_t const *dL, BfSvdStats *dS) {
  int rc = bfHipFail(hipFuncSetAttribute((void const *)bfJacobiKernel<W>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BF_JACOBI_LDS_MAX),
                    "hipFuncSetAttribute(Jacobi LDS)");
  if (rc) return rc;
  hipLaunchKernelGGL(bfJacobiKernel<W>, dim3(count), dim3(threads), lds, 0, dP, dL, dS, lds);
  return bfHipFail(hipGetLastError(), "Jacobi SVD launch");
}

typedef struct JacobiOrder { double cost; uint32_t idx; } JacobiOrder;
static int jacobiCostDescending(void const *pa, void const *pb) {
  JacobiOrder const *a = (JacobiOrder const *)pa, *b = (JacobiOrder const *)pb;
  if (a->cost != b->cost) return a->cost > b->cost ? -1 : 1;
  return a->idx < b->idx ? -1 : 1;
}
static double jacobiCost(BfSvdProb const *q) { return (double)q->me * q->me * (q->mt + q->me); }

// BFHIP_JACOBI_PROFILE=1: what lies between Begin and End is timed on its own, a synchronisation on either side
typedef struct JacobiProfile { int on; BfSvdStats const *dS; BfSvdStats before; double t0; } JacobiProfile;
static void jacobiProfileBegin(JacobiProfile *p) {
  if (!p->on) return;
  (void)hipDeviceSynchronize();
  (void)hipMemcpy(&p->before, p->dS, sizeof p->before, hipMemcpyDeviceToHost);
  p->t0 = bfNowSeconds();
}
// the seconds since Begin; *sweeps: what the launches in between added to the sweep statistics
static double jacobiProfileEnd(JacobiProfile const *p, unsigned long long *sweeps) {
  (void)hipDeviceSynchronize();
  double const dt = bfNowSeconds() - p->t0;
  BfSvdStats after;
  (void)hipMemcpy(&after, p->dS, sizeof after, hipMemcpyDeviceToHost);
  *sweeps = after.sumSweeps - p->before.sumSweeps;
  return dt;
}

int bfdevBuildJacobi(BfSvdProb const *hostProbs, uint64_t numProbs, BfLstSqOpts const *opts, BfSvdStats *stats) {
  if (!numProbs) return 0;
  enum { NW = 5, NL = BF_JACOBI_LDS_CLASSES, NCLS = 2 * NW * NL };
  uint32_t *lists[NCLS] = {0};
  uint64_t counts[NCLS] = {0};
  uint8_t *cls = (uint8_t *)malloc(numProbs);
  int rc = cls ? 0 : bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  // the route of every problem (bfJacobiRoute): the block form on Gram matrices (bfJacobiGramKernel) for rows + columns >=
  // gramMin (512 by default: fewer than nine stacked columns of a block would fit the LDS tile; N = 262144 build with the
  // limit at 384 / 512 / 768 / 1024: 21.5 / 22.0 / 22.0 - 23.6 / 27.5 s) and for those too long for the tile at all when they
  // have <= 4096 columns; the global-memory fallback beyond that (or for every problem: forceGlobal, a test hook for a path
  // that otherwise needs problems of > 2300 columns); else one launch class per (W, threads, LDS tile)
  BfLstSqOpts const o = bfLstSqResolve(opts);
  uint32_t *globalList = (uint32_t *)malloc(numProbs * sizeof(uint32_t));
  uint64_t numGlobal = 0;
  if (!globalList) rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  JacobiOrder *gramList = (JacobiOrder *)malloc((numProbs ? numProbs : 1) * sizeof(JacobiOrder));
  uint64_t numGram = 0;
  if (!gramList) rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  for (uint64_t i = 0; i < numProbs && !rc; ++i) {
    BfLstSqRoute r;
    bfJacobiRoute(hostProbs[i].mt, hostProbs[i].me, &o, &r);
    if (r.jacobi == BF_JACOBI_GRAM) {
      cls[i] = 0xff;
      gramList[numGram].idx = (uint32_t)i;
      gramList[numGram++].cost = jacobiCost(&hostProbs[i]);
      continue;
    }
    if (r.jacobi == BF_JACOBI_GLOBAL) { cls[i] = 0xff; globalList[numGlobal++] = (uint32_t)i; continue; }
    int wlog = 0;
    while ((4u << wlog) < r.w) ++wlog;                   // W = 4 << wlog, wlog = 0..4
    cls[i] = (uint8_t)((wlog * 2 + (r.threads == 1024)) * NL + (int)r.ldsClass);
    counts[cls[i]] += 1;
  }
  for (int c = 0; c < NCLS && !rc; ++c) {
    if (!counts[c]) continue;
    lists[c] = (uint32_t *)malloc(counts[c] * sizeof(uint32_t));
    if (!lists[c]) rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
    counts[c] = 0;
  }
  for (uint64_t i = 0; i < numProbs && !rc; ++i)
    if (cls[i] != 0xff) lists[cls[i]][counts[cls[i]]++] = (uint32_t)i;
  // longest first within a class (workgroups are dispatched in list order): the tail of a launch is then made of
  // the cheap problems, not of one 890-column problem started last
  for (int c = 0; c < NCLS && !rc; ++c) {
    if (counts[c] < 2) continue;
    JacobiOrder *ord = (JacobiOrder *)malloc(counts[c] * sizeof(JacobiOrder));
    if (!ord) { rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM"); break; }
    for (uint64_t i = 0; i < counts[c]; ++i) { ord[i].cost = jacobiCost(&hostProbs[lists[c][i]]); ord[i].idx = lists[c][i]; }
    qsort(ord, counts[c], sizeof(JacobiOrder), jacobiCostDescending);
    for (uint64_t i = 0; i < counts[c]; ++i) lists[c][i] = ord[i].idx;
    free(ord);
  }
  BfSvdProb *dP = NULL;
  BfSvdStats *dS = NULL;
  if (!rc) rc = uploadArrayB(&dP, hostProbs, numProbs, "svd problems");
  BfSvdStats zero = {0, 0, 0, 0};
  if (!rc) rc = uploadArrayB(&dS, &zero, 1, "svd stats");
  uint32_t *dL[NCLS] = {0};
  // BFHIP_JACOBI_PROFILE=1: time every class launch on its own (a synchronisation per class) and print it
  char const *penv = getenv("BFHIP_JACOBI_PROFILE");
  JacobiProfile prof = {penv && penv[0] == '1', dS, {0, 0, 0, 0}, 0.0};
  unsigned long long sweeps;
  // the block-form problems go first, on a stream of their own: they are the longest, and the class launches below (null
  // stream; a non-blocking stream does not order with it) fill the CUs their tail leaves idle
  uint32_t *dGram = NULL;
  hipStream_t sGram = NULL;
  if (!rc && numGram) rc = bfHipFail(hipStreamCreateWithFlags(&sGram, hipStreamNonBlocking), "hipStreamCreate");
  if (!rc && numGram) {
    qsort(gramList, numGram, sizeof(JacobiOrder), jacobiCostDescending);
    uint32_t *ids = (uint32_t *)malloc(numGram * sizeof(uint32_t));
    if (!ids) rc = bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
    for (uint64_t i = 0; i < numGram && !rc; ++i) ids[i] = gramList[i].idx;
    if (!rc) rc = uploadArrayB(&dGram, ids, numGram, "svd block-form list");
    free(ids);
    if (!rc) {
      jacobiProfileBegin(&prof);
      hipLaunchKernelGGL(bfJacobiGramKernel, dim3((uint32_t)numGram), dim3(BF_GRAM_THREADS), 0, sGram, dP, dGram, dS);
      rc = bfHipFail(hipGetLastError(), "Jacobi SVD (block form) launch");
    }
    if (prof.on && !rc) {
      double const dt = jacobiProfileEnd(&prof, &sweeps);
      fprintf(stderr, "[jacobi] block form (Gram) problems=%llu sweeps=%.1f  %.3f s\n", (unsigned long long)numGram, (double)sweeps / (double)numGram, dt);
    }
  }
  // classes are launched back to back (largest tiles first: they run longest) and synchronised once
  for (int lc = NL - 1; lc >= 0 && !rc; --lc)
    for (int wb = 0; wb < 2 * NW && !rc; ++wb) {
      int const c = wb * NL + lc;
      if (!counts[c]) continue;
      rc = uploadArrayB(&dL[c], lists[c], counts[c], "svd class list");
      if (rc) break;
      uint32_t const threads = wb & 1 ? 1024 : 256, lds = bfJacobiLdsCap((uint32_t)lc), n = (uint32_t)counts[c];
      jacobiProfileBegin(&prof);
      switch (wb >> 1) {
        case 0: rc = jacobiLaunch<4>(n, threads, lds, dP, dL[c], dS); break;
        case 1: rc = jacobiLaunch<8>(n, threads, lds, dP, dL[c], dS); break;
        case 2: rc = jacobiLaunch<16>(n, threads, lds, dP, dL[c], dS); break;
        case 3: rc = jacobiLaunch<32>(n, threads, lds, dP, dL[c], dS); break;
        default: rc = jacobiLaunch<64>(n, threads, lds, dP, dL[c], dS); break;
      }
      if (prof.on && !rc) {
        double const dt = jacobiProfileEnd(&prof, &sweeps);
        uint32_t lo = 0xffffffffu, hi = 0;
        double cube = 0;
        for (uint64_t i = 0; i < counts[c]; ++i) {
          BfSvdProb const *q = &hostProbs[lists[c][i]];
          lo = q->me < lo ? q->me : lo; hi = q->me > hi ? q->me : hi;
          cube += jacobiCost(q);
        }
        fprintf(stderr, "[jacobi] W=%d threads=%u lds=%uK problems=%u me=%u..%u sum(me^2 (mt+me))=%.3g sweeps=%.1f  %.3f s\n", 4 << (wb >> 1), threads,
                lds >> 10, n, lo, hi, cube, (double)sweeps / n, dt);
      }
    }
  uint32_t *dG = NULL;
  if (!rc && numGlobal) {
    rc = uploadArrayB(&dG, globalList, numGlobal, "svd fallback list");
    if (!rc) {
      hipLaunchKernelGGL(bfJacobiGlobalKernel, dim3((uint32_t)numGlobal), dim3(1024), 0, 0, dP, dG, dS);
      rc = bfHipFail(hipGetLastError(), "Jacobi SVD (global-memory fallback) launch");
    }
  }
  if (!rc) rc = bfHipFail(hipDeviceSynchronize(), "Jacobi SVD");
  (void)hipFree(dG); (void)hipFree(dGram);
  if (sGram) (void)hipStreamDestroy(sGram);
  free(globalList); free(gramList);
  for (int c = 0; c < NCLS; ++c) (void)hipFree(dL[c]);
  if (!rc && stats) {
    BfSvdStats got;
    rc = bfHipFail(hipMemcpy(&got, dS, sizeof got, hipMemcpyDeviceToHost), "svd stats");
    if (!rc) {
      if (got.maxSweeps > stats->maxSweeps) stats->maxSweeps = got.maxSweeps;
      stats->notConverged += got.notConverged;
      stats->truncated += got.truncated;
      stats->sumSweeps += got.sumSweeps;
    }
  }
  (void)hipFree(dP);
  (void)hipFree(dS);
  for (int c = 0; c < NCLS; ++c) free(lists[c]);
  free(cls);
  return rc;
}

// ---------------------------------------------------------------------------
// batched small complex GEMM, 32 x 32 output tile per workgroup, K in steps of
// 16 through LDS, 2 x 2 outputs per thread (fixed k order: deterministic)
// ---------------------------------------------------------------------------
#define BF_GT 32
#define BF_GK 16

__global__ __launch_bounds__(256) void bfGemmKernel(BfGemmJob const *jobs, uint64_t const *prefix, uint32_t numJobs, uint64_t tileBase) {
  __shared__ double2 As[BF_GK][BF_GT + 1];
  __shared__ double2 Bs[BF_GK][BF_GT + 1];
  uint64_t const tile = tileBase + blockIdx.x;
  uint32_t lo = 0, hi = numJobs;
  while (hi - lo > 1) {
    uint32_t const mid = (lo + hi) >> 1;
    if (prefix[mid] <= tile) lo = mid; else hi = mid;
  }
  BfGemmJob const J = jobs[lo];
  uint32_t const tilesM = (J.M + BF_GT - 1) / BF_GT;
  uint32_t const tl = (uint32_t)(tile - prefix[lo]);
  uint32_t const i0 = (tl % tilesM) * BF_GT, j0 = (tl / tilesM) * BF_GT;
  double2 const *A = (double2 const *)J.a, *B = (double2 const *)J.b;
  uint32_t const tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  double cr[2][2] = {{0, 0}, {0, 0}}, ci[2][2] = {{0, 0}, {0, 0}};
  for (uint32_t k0 = 0; k0 < J.K; k0 += BF_GK) {
    // stage op(A)[i0.., k0..] and B[k0.., j0..]
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      double2 a = make_double2(0.0, 0.0);
      if (J.transA) {
        uint32_t const kk = tid & 15, ii = (tid >> 4) + 16 * h;
        if (k0 + kk < J.K && i0 + ii < J.M) { a = A[(uint64_t)(i0 + ii) * J.lda + k0 + kk]; a.y = -a.y; }
        As[kk][ii] = a;
      } else {
        uint32_t const ii = tid & 31, kk = (tid >> 5) + 8 * h;
        if (k0 + kk < J.K && i0 + ii < J.M) a = A[(uint64_t)(k0 + kk) * J.lda + i0 + ii];
        As[kk][ii] = a;
      }
      uint32_t const kb = tid & 15, jj = (tid >> 4) + 16 * h;
      double2 b = make_double2(0.0, 0.0);
      if (k0 + kb < J.K && j0 + jj < J.N) b = B[(uint64_t)(j0 + jj) * J.ldb + k0 + kb];
      Bs[kb][jj] = b;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BF_GK; ++kk) {
      double2 const a0 = As[kk][ty], a1 = As[kk][ty + 16], b0 = Bs[kk][tx], b1 = Bs[kk][tx + 16];
      double2 const av[2] = {a0, a1}, bv[2] = {b0, b1};
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          cr[u][v] = fma(av[u].x, bv[v].x, cr[u][v]); cr[u][v] = fma(-av[u].y, bv[v].y, cr[u][v]);
          ci[u][v] = fma(av[u].x, bv[v].y, ci[u][v]); ci[u][v] = fma(av[u].y, bv[v].x, ci[u][v]);
        }
    }
    __syncthreads();
  }
  double2 *C = (double2 *)J.c;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    uint32_t const i = i0 + ty + 16 * u;
    if (i >= J.M) continue;
    double const sc = J.scale ? J.scale[i] : 1.0;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      uint32_t const j = j0 + tx + 16 * v;
      if (j < J.N) C[(uint64_t)j * J.ldc + i] = make_double2(cr[u][v] * sc, ci[u][v] * sc);
    }
  }
}

int bfdevBuildGemm(BfGemmJob const *hostJobs, uint64_t numJobs) {
  if (!numJobs) return 0;
  uint64_t *prefix = (uint64_t *)malloc((numJobs + 1) * sizeof(uint64_t));
  if (!prefix) return bfhipFail(BFABI_ERROR_MEMORY_ERROR, "host OOM");
  prefix[0] = 0;
  for (uint64_t i = 0; i < numJobs; ++i)
    prefix[i + 1] = prefix[i] + (uint64_t)((hostJobs[i].M + BF_GT - 1) / BF_GT) * ((hostJobs[i].N + BF_GT - 1) / BF_GT);
  BfGemmJob *dJ = NULL;
  uint64_t *dP = NULL;
  int rc = uploadArrayB(&dJ, hostJobs, numJobs, "gemm jobs");
  if (!rc) rc = uploadArrayB(&dP, prefix, numJobs + 1, "gemm tile prefix");
  uint64_t const tiles = prefix[numJobs];
  for (uint64_t done = 0; done < tiles && !rc;) {
    uint32_t const n = (uint32_t)(tiles - done > (1u << 30) ? (1u << 30) : tiles - done);
    hipLaunchKernelGGL(bfGemmKernel, dim3(n), dim3(256), 0, 0, dJ, dP, (uint32_t)numJobs, done);
    rc = bfHipFail(hipGetLastError(), "builder gemm launch");
    done += n;
  }
  if (!rc) rc = bfHipFail(hipDeviceSynchronize(), "builder gemm");
  (void)hipFree(dJ);
  (void)hipFree(dP);
  free(prefix);
  return rc;
}

