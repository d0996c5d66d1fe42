// bfhip_condlik.hip -- the kernels of the log-likelihood, its gradients and the kriging variances of a conditioned field
// (bfhipCovCondLogLikelihoodDevice, bfhipCovCondVarianceDevice, include/bfhip.h; host side: bfhip_condlik.c; DESIGN.md
// section 21).  Nothing here is a stage kernel.  Everything is double; every index into a matrix is 64 bits; no atomics:
// each output element has one owner and every sum a fixed order that depends on the shapes alone.
//
// Matrices (row-major, as in bfhip_cond.hip): Bt [n x k], L [k x k] lower triangular, alpha [k].
//
// The hot path is bfLikStripKernel: the column sums of squares of X = L^-1 S for a wide S [k x s] that is never stored.
// Columns of a triangular solve are independent: a workgroup of 256 threads owns a strip of 64 columns and runs the whole
// forward substitution for it, block row by block row of 64 (BF_LIK_NB):
//   T   = S_p - L[p, < p] X_<p    left-looking: a 64 x 64 tile contracted over all earlier rows, slabs of 32 staged through
//                                 LDS (25 KiB), thread (ty, tx) of 16 x 16 owning rows 4 ty .. + 3 and columns tx, tx + 16,
//                                 tx + 32, tx + 48: per step of the contraction 8 LDS reads feed 16 FMAs; the next slab's
//                                 global loads are in flight during the FMAs
//   X_p = L[p, p]^-1 T            two more slabs of the same routine: the inverse of the diagonal tile (formed once per object
//                                 by bfLikInvDiagKernel) and T meet in LDS, so all 256 threads work and the owner of an
//                                 element of the tile stays its owner; the tiles are 64 x 64 blocks of a Cholesky factor,
//                                 cond(L[p, p]) <= sqrt(cond(K)): the product loses sqrt(cond(K)) ulps at most, far below
//                                 what the factorization itself loses
//   sum[s] += X_p[i, s]^2         per owner in increasing row order; the 16 owners of a column added in the order of their rows
// X lives in the workgroup's own k x 64 strip of scratch, which nobody else touches; the kernel writes that strip and the
// 64 sums.  The result of a column does not depend on the number of workgroups.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bfhip_cond.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"

#define BF_LIK_TP 32u            // slab of the contracted index
#define BF_LIK_TS BF_LIK_STRIP   // 64 columns

// ---------------------------------------------------------------------------
// the strip solve
// ---------------------------------------------------------------------------
template <int KIND>
__device__ __forceinline__ double bfLikSource(double const *src, uint64_t ld, uint32_t k, uint64_t a, uint64_t col) {
  if (KIND == BF_LIK_SRC_BT_ROWS) return src[col * k + a];
  if (KIND == BF_LIK_SRC_IDENTITY) return a == col ? 1.0 : 0.0;
  return src[a * ld + col];
}

// acc[u][v] += sum_pl sa[pl][4 ty + u] sb[pl][tx + 16 v]: the a's are broadcasts, the b's 16 consecutive doubles a read
__device__ __forceinline__ void bfLikSlab(double (&acc)[4][4], double (*sa)[BF_LIK_NB + 1], double (*sb)[BF_LIK_TS + 1], uint32_t ty, uint32_t tx) {
#pragma unroll 4
  for (uint32_t pl = 0; pl < BF_LIK_TP; ++pl) {
    double a[4], b[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) a[u] = sa[pl][4 * ty + u];
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v) b[v] = sb[pl][tx + 16 * v];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u)
#pragma unroll
      for (uint32_t v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
  }
}

template <int KIND>
__global__ __launch_bounds__(256) void bfLikStripKernel(double const *L, double const *Linv, uint32_t k, double const *src, uint64_t ld, uint64_t numCols,
                                                        uint64_t numStrips, double *strips, double *out) {
  __shared__ double sa[BF_LIK_TP][BF_LIK_NB + 1];     // L[block row, slab], then half the inverse of the diagonal tile: sa[pl][il]
  __shared__ double sb[BF_LIK_TP][BF_LIK_TS + 1];     // X[slab, 64 columns], then half of T
  uint32_t const t = threadIdx.x, ty = t >> 4, tx = t & 15;
  double *X = strips + (uint64_t)blockIdx.x * k * BF_LIK_TS;
  for (uint64_t strip = blockIdx.x; strip < numStrips; strip += gridDim.x) {
    uint64_t const c0 = strip * BF_LIK_TS;
    // identity: column c0 + s is zero above row c0 + s, so is X: the rows before c0 (a multiple of 64) are neither formed nor read
    uint32_t const kstart = KIND == BF_LIK_SRC_IDENTITY ? (uint32_t)c0 : 0u;
    double ss[4] = {0, 0, 0, 0};
    for (uint32_t r0 = kstart; r0 < k; r0 += BF_LIK_NB) {
      uint32_t const nb = k - r0 < BF_LIK_NB ? k - r0 : BF_LIK_NB;
      double acc[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
      if (r0 > kstart) {
        double ra[8], rb[8];
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) {
          uint32_t const e = t + 256 * r;
          ra[r] = (e >> 5) < nb ? L[(uint64_t)(r0 + (e >> 5)) * k + kstart + (e & 31)] : 0.0;
          rb[r] = X[(uint64_t)(kstart + (e >> 6)) * BF_LIK_TS + (e & 63)];
        }
        for (uint32_t pp = kstart; pp < r0; pp += BF_LIK_TP) {
#pragma unroll
          for (uint32_t r = 0; r < 8; ++r) {
            uint32_t const e = t + 256 * r;
            sa[e & 31][e >> 5] = ra[r];
            sb[e >> 6][e & 63] = rb[r];
          }
          __syncthreads();
          uint32_t const pn = pp + BF_LIK_TP;
          if (pn < r0) {                                // the next slab, in flight during this one's FMAs
#pragma unroll
            for (uint32_t r = 0; r < 8; ++r) {
              uint32_t const e = t + 256 * r;
              ra[r] = (e >> 5) < nb ? L[(uint64_t)(r0 + (e >> 5)) * k + pn + (e & 31)] : 0.0;
              rb[r] = X[(uint64_t)(pn + (e >> 6)) * BF_LIK_TS + (e & 63)];
            }
          }
          bfLikSlab(acc, sa, sb, ty, tx);
          __syncthreads();
        }
      }
      // T = S_p - acc (zero beyond the last row), kept by its owners
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u)
#pragma unroll
        for (uint32_t v = 0; v < 4; ++v) {
          uint32_t const i = 4 * ty + u;
          uint64_t const col = c0 + tx + 16 * v;
          double const sv = (i < nb && col < numCols) ? bfLikSource<KIND>(src, ld, k, (uint64_t)r0 + i, col) : 0.0;
          acc[u][v] = sv - acc[u][v];
        }
      // X_p = Linv T: two more slabs, the rows 0 .. 31 of T with the columns 0 .. 31 of the inverse, then the other halves
      double const *tile = Linv + (uint64_t)(r0 / BF_LIK_NB) * BF_LIK_NB * BF_LIK_NB;
      double x[4][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
      for (uint32_t half = 0; half < 2; ++half) {
        if ((ty >> 3) == half) {
#pragma unroll
          for (uint32_t u = 0; u < 4; ++u)
#pragma unroll
            for (uint32_t v = 0; v < 4; ++v) sb[4 * (ty & 7) + u][tx + 16 * v] = acc[u][v];
        }
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) { uint32_t const e = t + 256 * r; sa[e & 31][e >> 5] = tile[(e >> 5) * BF_LIK_NB + BF_LIK_TP * half + (e & 31)]; }
        __syncthreads();
        bfLikSlab(x, sa, sb, ty, tx);
        if (half == 0) __syncthreads();
      }
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u)
        if (4 * ty + u < nb) {
#pragma unroll
          for (uint32_t v = 0; v < 4; ++v) {
            X[(uint64_t)(r0 + 4 * ty + u) * BF_LIK_TS + tx + 16 * v] = x[u][v];
            ss[v] = fma(x[u][v], x[u][v], ss[v]);
          }
        }
      __syncthreads();                                  // X_p is visible to the workgroup; the LDS tiles are free again
    }
    // the 16 owners of a column, added in the order of their rows
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v) sb[ty][tx + 16 * v] = ss[v];
    __syncthreads();
    if (t < BF_LIK_TS && c0 + t < numCols) {
      double sum = 0.0;
      for (uint32_t g = 0; g < 16; ++g) sum += sb[g][t];
      out[c0 + t] = sum;
    }
    __syncthreads();
  }
}

// Linv [ceil(k / 64)][64][64]: the inverses of the diagonal tiles of L (identity beyond the last row), formed once per object.
// Thread s owns column s of the identity; its unknowns live in a column of LDS of its own, eliminated right-looking
// (unknown d loses its products in increasing c); the entries of L are read by the whole wavefront at once.
__global__ __launch_bounds__(64) void bfLikInvDiagKernel(double *Linv, double const *L, uint32_t k) {
  __shared__ double xs[BF_LIK_NB][BF_LIK_NB + 1];
  uint32_t const s = threadIdx.x, r0 = blockIdx.x * BF_LIK_NB, nb = k - r0 < BF_LIK_NB ? k - r0 : BF_LIK_NB;
  double *tile = Linv + (uint64_t)blockIdx.x * BF_LIK_NB * BF_LIK_NB;
  for (uint32_t c = 0; c < BF_LIK_NB; ++c) xs[c][s] = c == s ? 1.0 : 0.0;
  for (uint32_t c = 0; c < BF_LIK_NB; ++c) {
    double const xc = c < nb ? xs[c][s] / L[(uint64_t)(r0 + c) * k + r0 + c] : xs[c][s];
    tile[c * BF_LIK_NB + s] = xc;
    for (uint32_t d = c + 1; d < nb; ++d) xs[d][s] = fma(-L[(uint64_t)(r0 + d) * k + r0 + c], xc, xs[d][s]);
  }
}

int bfdevLikInvDiag(double *Linv, double const *L, uint32_t k, void *stream) {
  if (!k) return 0;
  hipLaunchKernelGGL(bfLikInvDiagKernel, dim3((k + BF_LIK_NB - 1) / BF_LIK_NB), dim3(64), 0, (hipStream_t)stream, Linv, L, k);
  return bfHipFail(hipGetLastError(), "diagonal tile inverse launch");
}

int bfdevLikStripSolve(double const *L, double const *Linv, uint32_t k, int kind, double const *src, uint64_t ld, uint64_t numCols, double *strips, uint64_t slots, double *out,
                       void *stream) {
  if (!k || !numCols) return 0;
  if (!slots) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "strip solve: no workspace");
  uint64_t const numStrips = (numCols + BF_LIK_TS - 1) / BF_LIK_TS;
  uint64_t const g = slots < numStrips ? slots : numStrips;
  dim3 const grid((uint32_t)(g < 0x7fffffffu ? g : 0x7fffffffu)), block(256);
  hipStream_t const s = (hipStream_t)stream;
  if (kind == BF_LIK_SRC_BT_ROWS) hipLaunchKernelGGL(bfLikStripKernel<BF_LIK_SRC_BT_ROWS>, grid, block, 0, s, L, Linv, k, src, ld, numCols, numStrips, strips, out);
  else if (kind == BF_LIK_SRC_IDENTITY) {
    if (numCols != k) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "strip solve: the identity has k columns");
    hipLaunchKernelGGL(bfLikStripKernel<BF_LIK_SRC_IDENTITY>, grid, block, 0, s, L, Linv, k, src, ld, numCols, numStrips, strips, out);
  } else if (kind == BF_LIK_SRC_BLOCK) hipLaunchKernelGGL(bfLikStripKernel<BF_LIK_SRC_BLOCK>, grid, block, 0, s, L, Linv, k, src, ld, numCols, numStrips, strips, out);
  else return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "strip solve: unknown source");
  return bfHipFail(hipGetLastError(), "strip solve launch");
}

// ---------------------------------------------------------------------------
// the value: quad = y^T alpha, logDet = 2 sum log L[a, a]
// ---------------------------------------------------------------------------
// One workgroup: thread t sums its entries a = t, t + 256, ... in that order, then a binary tree over the 256 partials.
__global__ __launch_bounds__(256) void bfLikValueKernel(double *value, double const *L, uint32_t k, double const *y, double const *alpha) {
  __shared__ double sq[256], sl[256];
  uint32_t const t = threadIdx.x;
  double q = 0.0, l = 0.0;
  for (uint32_t a = t; a < k; a += 256) {
    q = fma(y[a], alpha[a], q);
    l += log(L[(uint64_t)a * k + a]);
  }
  sq[t] = q; sl[t] = l;
  __syncthreads();
  for (uint32_t w = 128; w; w >>= 1) {
    if (t < w) { sq[t] += sq[t + w]; sl[t] += sl[t + w]; }
    __syncthreads();
  }
  if (t == 0) {
    double const quad = sq[0], logDet = 2.0 * sl[0];
    value[0] = -0.5 * quad - 0.5 * logDet - 0.5 * (double)k * 1.8378770664093454835606594728112;   // log(2 pi)
    value[1] = quad;
    value[2] = logDet;
  }
}

int bfdevLikValue(double *value, double const *L, uint32_t k, double const *y, double const *alpha, void *stream) {
  hipLaunchKernelGGL(bfLikValueKernel, dim3(1), dim3(256), 0, (hipStream_t)stream, value, L, k, y, alpha);
  return bfHipFail(hipGetLastError(), "likelihood value launch");
}

// ---------------------------------------------------------------------------
// gradients
// ---------------------------------------------------------------------------
// u_j = sum_a Bt[j, a] alpha[a] in double (bfCondUpdateKernel rounds to the operator's type): a wavefront owns row j, lane l
// sums a = l, l + 64, ... in that order, then the butterfly over the 64 lanes; grad[j] = u_j^2 - colSq[j].  A zero row of Bt
// gives u_j = 0 and, with colSq[j] = +0, exactly +0.
__global__ __launch_bounds__(256) void bfLikGradGammaKernel(double *grad, double const *Bt, uint64_t n, uint32_t k, double const *alpha, double const *colSq) {
  uint32_t const lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint64_t j = (uint64_t)blockIdx.x * 4 + w; j < n; j += (uint64_t)gridDim.x * 4) {
    double const *row = Bt + j * k;
    double u = 0.0;
    for (uint32_t a = lane; a < k; a += 64) u = fma(row[a], alpha[a], u);
    for (int off = 32; off; off >>= 1) u += __shfl_xor(u, off, 64);
    if (lane == 0) grad[j] = u * u - colSq[j];
  }
}

int bfdevLikGradGamma(double *grad, double const *Bt, uint64_t n, uint32_t k, double const *alpha, double const *colSq, void *stream) {
  if (!n) return 0;
  uint64_t const need = (n + 3) / 4;
  hipLaunchKernelGGL(bfLikGradGammaKernel, dim3((uint32_t)(need < 65536 ? need : 65536)), dim3(256), 0, (hipStream_t)stream, grad, Bt, n, k, alpha, colSq);
  return bfHipFail(hipGetLastError(), "gamma gradient launch");
}

__global__ __launch_bounds__(256) void bfLikGradNoiseKernel(double *grad, double const *alpha, double const *colSq, uint32_t k) {
  uint32_t const a = blockIdx.x * 256 + threadIdx.x;
  if (a < k) grad[a] = 0.5 * (alpha[a] * alpha[a] - colSq[a]);
}

int bfdevLikGradNoise(double *grad, double const *alpha, double const *colSq, uint32_t k, void *stream) {
  hipLaunchKernelGGL(bfLikGradNoiseKernel, dim3((k + 255) / 256), dim3(256), 0, (hipStream_t)stream, grad, alpha, colSq, k);
  return bfHipFail(hipGetLastError(), "noise gradient launch");
}

// ---------------------------------------------------------------------------
// the prior variance: column sums of squares over n, chunked like the Gram kernel
// ---------------------------------------------------------------------------
// A workgroup owns a chunk of BF_COND_CHUNK rows: thread (g, s) of 4 x 64 sums the rows j0 + g, j0 + g + 4, ... of column s
// from zero, the four are added in the order of g; part [chunks x 64].
__global__ __launch_bounds__(256) void bfVarPriorPartKernel(double *part, double const *blk, uint64_t n, uint32_t p) {
  __shared__ double red[4][BF_LIK_TS];
  uint32_t const s = threadIdx.x & 63, g = threadIdx.x >> 6;
  uint64_t const j0 = (uint64_t)blockIdx.x * BF_COND_CHUNK, j1 = j0 + BF_COND_CHUNK < n ? j0 + BF_COND_CHUNK : n;
  double sum = 0.0;
  if (s < p)
    for (uint64_t j = j0 + g; j < j1; j += 4) { double const v = blk[j * p + s]; sum = fma(v, v, sum); }
  red[g][s] = sum;
  __syncthreads();
  if (g == 0) part[(uint64_t)blockIdx.x * BF_LIK_TS + s] = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
}

int bfdevVarPriorPart(double *part, double const *blk, uint64_t n, uint32_t p, void *stream) {
  if (!p || p > BF_LIK_TS) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "prior variance: 1 .. 64 columns a panel");
  uint64_t const chunks = (n + BF_COND_CHUNK - 1) / BF_COND_CHUNK;
  if (!chunks || chunks > 65535) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "prior variance: 1 .. 65535 chunks of %u columns", BF_COND_CHUNK);
  hipLaunchKernelGGL(bfVarPriorPartKernel, dim3((uint32_t)chunks), dim3(256), 0, (hipStream_t)stream, part, blk, n, p);
  return bfHipFail(hipGetLastError(), "prior variance launch");
}

__global__ __launch_bounds__(64) void bfVarAssembleKernel(double *prior, double *post, double const *part, uint64_t chunks, double const *solved, uint32_t p) {
  uint32_t const s = threadIdx.x;
  if (s >= p) return;
  double sum = 0.0;
  for (uint64_t c = 0; c < chunks; ++c) sum += part[c * BF_LIK_TS + s];
  if (prior) prior[s] = sum;
  if (post) post[s] = sum - solved[s];
}

int bfdevVarAssemble(double *prior, double *post, double const *part, uint64_t chunks, double const *solved, uint32_t p, void *stream) {
  if (!p || p > BF_LIK_TS) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "variance: 1 .. 64 columns a panel");
  hipLaunchKernelGGL(bfVarAssembleKernel, dim3(1), dim3(64), 0, (hipStream_t)stream, prior, post, part, chunks, solved, p);
  return bfHipFail(hipGetLastError(), "variance assembly launch");
}
