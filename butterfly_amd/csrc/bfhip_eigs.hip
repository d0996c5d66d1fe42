// bfhip_eigs.hip -- the kernels of the filtered subspace iteration (bfhipChebCovEigsDevice, include/bfhip.h; host side:
// bfhip_eigs.c).  The operator is the CSR matrix S of a BfhipChebCov; the blocks are row-major
// n x ld doubles of which the first p columns are in use, ld = p rounded up to a multiple of 16.  The padding columns are
// zero when the workspace is made and no kernel here ever writes anything else into them (the step kernel writes columns
// below p only, the rotation multiplies by a matrix whose padding is zero), so the dense kernels see whole 16 x 16 tiles
// and need no column guard; rows are guarded wherever a tile or a chunk can pass n.
//
//   bfEigsStepKernel      out = alpha (S b1) + beta b1 + gamma b2        every filter step and Y = S X
//   bfEigsGramKernel      partial X^T Y per chunk of rows               v_mfma_f64_16x16x4_f64
//   bfEigsReduceKernel    the partials summed in chunk order            (no floating-point atomics anywhere)
//   bfEigsRotateKernel    out = X W for a p x p matrix W                v_mfma_f64_16x16x4_f64, out of place
//   bfEigsResidualKernel  partial column sums of squares of Y - X diag(theta) per chunk
//   bfEigsStoreKernel     the first nev columns, scaled by d when asked, into the caller's block
//   bfEigsCrossGramKernel partial Q[:, m0 .. m0 + mq)^T X per chunk of rows, Q in the caller's layout   (section 27)
//   bfEigsDeflateKernel   X <- X - Q[:, m0 .. m0 + mq) C, in place                                      (section 27)
//
// Every sum has one fixed order that depends on (n, p) alone (the two deflation kernels: on (n, ld, m) and the panel): two calls
// give the same bits.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"
#include "bfhip_cheb_gather.h"

#define BF_EIGS_MAX_GRID (1u << 20)
typedef double bf_d4 __attribute__((ext_vector_type(4)));      // the C/D fragment of v_mfma_f64_16x16x4_f64, as in bfhip_stage_mfma.h

// The lane layout, the gather groups and the row sum of bfChebStepKernel (bfhip_cheb_gather.h), one block stream fewer:
// there is no w.  Per element: r = alpha * sum; r = fma(beta, b1, r); r = fma(gamma, b2, r) -- the same sequence for every
// p, so column j of a p-column block equals the one-column result bit for bit.  out may be b2 (an element's owner is the
// only reader of its b2 element) and nothing else the kernel reads.
__global__ __launch_bounds__(256) void bfEigsStepKernel(BfEigsStep a, uint32_t lanesLog2) {
  uint32_t const lanes = 1u << lanesLog2, lane = threadIdx.x & (lanes - 1), rowsPerWg = 256u >> lanesLog2;
  uint64_t const p = a.p, ld = a.ld;
  for (uint64_t i = (uint64_t)blockIdx.x * rowsPerWg + (threadIdx.x >> lanesLog2); i < a.n; i += (uint64_t)gridDim.x * rowsPerWg) {
    uint64_t const beg = a.rowptr[i], end = a.rowptr[i + 1];
    for (uint64_t c0 = 0; c0 < p; c0 += lanes) {
      uint64_t const c = c0 + lane;
      bool const live = c < p;
      double own = 0, old = 0;
      if (live) {
        own = a.b1[i * ld + c];
        if (a.b2) old = a.b2[i * ld + c];
      }
      double const acc = bfChebRowGather(a.colind, a.val, beg, end, a.b1, ld, c, lane, lanes, live);
      double r = a.alpha * acc;
      r = fma(a.beta, own, r);
      if (a.b2) r = fma(a.gamma, old, r);
      if (live) a.out[i * ld + c] = r;
    }
  }
}

// G = X^T Y on the FP64 matrix cores, one partial per chunk of rows.  One wavefront per workgroup: chunk blockIdx.x, tile
// row ti = blockIdx.y (16 columns of X) and up to four tile columns from 4 * blockIdx.z (64 columns of Y).  A k-step is
// four rows of the blocks: the tile of X^T is the A operand as it lies in memory (lane l loads X[r + (l >> 4)][16 ti + (l & 15)],
// 128 contiguous bytes per row), the tile of Y the B operand in the same way.  C/D: col = lane & 15, row = (lane >> 4) + 4 reg.
// Four k-steps are requested before the first is used.  Rows at or past the chunk's end load zero.
template <int NT> static __device__ __forceinline__ void bfEigsGramTiles(double const *X, double const *Y, uint64_t ld, uint64_t r0, uint64_t r1,
                                                                         uint32_t ti, uint32_t tj0, double *part) {
  constexpr int UNR = 4;
  uint32_t const lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  bf_d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = bf_d4{0, 0, 0, 0};
  for (uint64_t r = r0; r < r1; r += 4 * UNR) {
    double a[UNR], b[UNR][NT];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      uint64_t const row = r + 4 * u + kq;
      bool const ok = row < r1;
      a[u] = ok ? X[row * ld + 16 * ti + col] : 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t) b[u][t] = ok ? Y[row * ld + 16 * (tj0 + t) + col] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u][t], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) part[(uint64_t)(16 * ti + kq + 4 * g) * ld + 16 * (tj0 + t) + col] = acc[t][g];
}

__global__ __launch_bounds__(64) void bfEigsGramKernel(double const *X, double const *Y, uint64_t n, uint32_t ld, uint64_t chunkRows, double *part) {
  uint32_t const tiles = ld / 16, ti = blockIdx.y, tj0 = 4 * blockIdx.z, nt = tiles - tj0 < 4 ? tiles - tj0 : 4;
  uint64_t const r0 = (uint64_t)blockIdx.x * chunkRows, r1 = r0 + chunkRows < n ? r0 + chunkRows : n;
  double *dst = part + (uint64_t)blockIdx.x * ld * ld;
  switch (nt) {
    case 4: bfEigsGramTiles<4>(X, Y, ld, r0, r1, ti, tj0, dst); break;
    case 3: bfEigsGramTiles<3>(X, Y, ld, r0, r1, ti, tj0, dst); break;
    case 2: bfEigsGramTiles<2>(X, Y, ld, r0, r1, ti, tj0, dst); break;
    default: bfEigsGramTiles<1>(X, Y, ld, r0, r1, ti, tj0, dst); break;
  }
}

// out[e] = part[0][e] + part[1][e] + ... in chunk order, e < count; chunk c starts at c * count
__global__ __launch_bounds__(256) void bfEigsReduceKernel(double const *part, uint64_t chunks, uint64_t count, double *out) {
  uint64_t const e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  double s = 0;
  for (uint64_t c = 0; c < chunks; ++c) s += part[c * count + e];
  out[e] = s;
}

// out = X W, W [ld x ld] row-major with zero padding.  One wavefront per workgroup: 16 rows (blockIdx.x) and up to four tile
// columns from 4 * blockIdx.y.  The contraction index is walked in blocks of 16: lane (m = l & 15, kq = l >> 4) loads the four
// neighbours X[r0 + m][k16 + 4 kq + e], e < 4, as one 32-byte request (the four lanes of a row cover 128 contiguous bytes),
// and MFMA e of the block contracts over the slots kq with B slot kq = W[k16 + 4 kq + e][.]: every index of the block is
// used exactly once, in an order that is fixed.  Out of place: a workgroup's rows are read by the other tile-column groups.
template <int NT> static __device__ __forceinline__ void bfEigsRotateTiles(double const *X, double const *W, double *out, uint64_t n, uint64_t ld,
                                                                           uint64_t r0, uint32_t tj0) {
  uint32_t const lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  uint64_t const rowA = r0 + col;
  bool const okA = rowA < n;
  bf_d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = bf_d4{0, 0, 0, 0};
  for (uint64_t k16 = 0; k16 < ld; k16 += 16) {
    bf_d4 const a = okA ? *(bf_d4 const *)(X + rowA * ld + k16 + 4 * kq) : bf_d4{0, 0, 0, 0};
    double b[4][NT];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < NT; ++t) b[e][t] = W[(k16 + 4 * kq + e) * ld + 16 * (tj0 + t) + col];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], b[e][t], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint64_t const row = r0 + kq + 4 * g;
      if (row < n) out[row * ld + 16 * (tj0 + t) + col] = acc[t][g];
    }
}

__global__ __launch_bounds__(64) void bfEigsRotateKernel(double const *X, double const *W, double *out, uint64_t n, uint32_t ld) {
  uint32_t const tiles = ld / 16, tj0 = 4 * blockIdx.y, nt = tiles - tj0 < 4 ? tiles - tj0 : 4;
  for (uint64_t r0 = (uint64_t)blockIdx.x * 16; r0 < n; r0 += (uint64_t)gridDim.x * 16)
    switch (nt) {
      case 4: bfEigsRotateTiles<4>(X, W, out, n, ld, r0, tj0); break;
      case 3: bfEigsRotateTiles<3>(X, W, out, n, ld, r0, tj0); break;
      case 2: bfEigsRotateTiles<2>(X, W, out, n, ld, r0, tj0); break;
      default: bfEigsRotateTiles<1>(X, W, out, n, ld, r0, tj0); break;
    }
}

// part[chunk][c] = sum over the chunk's rows of (Y[r][c] - theta[c] X[r][c])^2.  Thread (cl = t & 63, rl = t >> 6) walks the
// rows r0 + rl, r0 + rl + 4, ... of column cl of every panel of 64 columns; the four row lanes are summed through LDS in
// the order rl = 0, 1, 2, 3.
__global__ __launch_bounds__(256) void bfEigsResidualKernel(double const *X, double const *Y, double const *theta, uint64_t n, uint32_t ld,
                                                            uint64_t chunkRows, double *part) {
  __shared__ double sh[4][64];
  uint32_t const cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  uint64_t const r0 = (uint64_t)blockIdx.x * chunkRows, r1 = r0 + chunkRows < n ? r0 + chunkRows : n;
  for (uint32_t c0 = 0; c0 < ld; c0 += 64) {
    uint32_t const c = c0 + cl;
    double s = 0;
    if (c < ld) {
      double const th = theta[c];
      for (uint64_t r = r0 + rl; r < r1; r += 4) {
        double const d = fma(-th, X[r * ld + c], Y[r * ld + c]);
        s = fma(d, d, s);
      }
    }
    sh[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < ld) part[(uint64_t)blockIdx.x * ld + c] = ((sh[0][cl] + sh[1][cl]) + sh[2][cl]) + sh[3][cl];
    __syncthreads();
  }
}

// dst[i * ldu + j] = (d ? d[i] : 1) * X[i * ld + j], j < nev: the columns the caller asked for and nothing beside them
__global__ __launch_bounds__(256) void bfEigsStoreKernel(double const *X, uint64_t n, uint32_t ld, uint32_t nev, double const *d, double *dst, uint64_t ldu) {
  uint64_t const total = n * nev;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
    uint64_t const i = e / nev;
    uint32_t const j = (uint32_t)(e - i * nev);
    double const x = X[i * ld + j];
    dst[i * ldu + j] = d ? d[i] * x : x;
  }
}

// ---- deflation against locked vectors (bfhipChebCovEigsBandDevice) ---------------------------------
// Q is the caller's block of locked eigenvectors: row-major, leading dimension ldq (any), the panel's columns m0 .. m0 + mq - 1,
// mq <= 256; no alignment beyond a double's.  C is [mq16 x ld], mq16 = mq rounded up to 16, rows from mq on exact +0.
//
// C = Q^T X, one partial per chunk of rows: bfEigsGramTiles with the A operand taken from Q as it lies in memory (lane l loads
// Q[r + (l >> 4)][m0 + 16 ti + (l & 15)], one double at stride ldq; a column at or past mq and a row at or past the chunk's end
// load exact zero), the B operand the X tile, four k-steps requested before the first is used.
template <int NT> static __device__ __forceinline__ void bfEigsCrossGramTiles(double const *Q, uint64_t ldq, uint32_t mq, double const *X, uint64_t ld,
                                                                              uint64_t r0, uint64_t r1, uint32_t ti, uint32_t tj0, double *part) {
  constexpr int UNR = 4;
  uint32_t const lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  bool const okCol = 16 * ti + col < mq;
  bf_d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = bf_d4{0, 0, 0, 0};
  for (uint64_t r = r0; r < r1; r += 4 * UNR) {
    double a[UNR], b[UNR][NT];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      uint64_t const row = r + 4 * u + kq;
      bool const ok = row < r1;
      a[u] = ok && okCol ? Q[row * ldq + 16 * ti + col] : 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t) b[u][t] = ok ? X[row * ld + 16 * (tj0 + t) + col] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u][t], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) part[(uint64_t)(16 * ti + kq + 4 * g) * ld + 16 * (tj0 + t) + col] = acc[t][g];
}

// grid: (chunks, mq16 / 16, tile-column groups of X); Q points at column m0 already
__global__ __launch_bounds__(64) void bfEigsCrossGramKernel(double const *Q, uint64_t ldq, uint32_t mq, double const *X, uint64_t n, uint32_t ld,
                                                            uint64_t chunkRows, double *part) {
  uint32_t const tiles = ld / 16, ti = blockIdx.y, tj0 = 4 * blockIdx.z, nt = tiles - tj0 < 4 ? tiles - tj0 : 4;
  uint64_t const r0 = (uint64_t)blockIdx.x * chunkRows, r1 = r0 + chunkRows < n ? r0 + chunkRows : n;
  double *dst = part + (uint64_t)blockIdx.x * (16 * gridDim.y) * ld;
  switch (nt) {
    case 4: bfEigsCrossGramTiles<4>(Q, ldq, mq, X, ld, r0, r1, ti, tj0, dst); break;
    case 3: bfEigsCrossGramTiles<3>(Q, ldq, mq, X, ld, r0, r1, ti, tj0, dst); break;
    case 2: bfEigsCrossGramTiles<2>(Q, ldq, mq, X, ld, r0, r1, ti, tj0, dst); break;
    default: bfEigsCrossGramTiles<1>(Q, ldq, mq, X, ld, r0, r1, ti, tj0, dst); break;
  }
}

// X[r][:] <- X[r][:] - sum_k Q[r][k] C[k][:], k < mq.  bfEigsRotateTiles with A = Q and B = C: lane (m = l & 15, kq = l >> 4)
// holds the four neighbours Q[r0 + m][k16 + 4 kq + e], e < 4 -- one 32-byte request when VEC (Q 32-byte aligned, ldq % 4 == 0)
// and the four lie below mq, four guarded doubles otherwise; an index at or past mq contributes zero.  The sum runs from zero
// over the blocks of 16 in order, then one subtraction from the loaded X.  In place: a workgroup's 16 rows x <= 4 tile columns
// of X are read by nobody else.
template <int NT, bool VEC> static __device__ __forceinline__ void bfEigsDeflateTiles(double const *Q, uint64_t ldq, uint32_t mq, double const *C, double *X,
                                                                                      uint64_t n, uint64_t ld, uint64_t r0, uint32_t tj0) {
  uint32_t const lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  uint64_t const rowA = r0 + col;
  bool const okA = rowA < n;
  double const *qrow = Q + rowA * ldq;
  bf_d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = bf_d4{0, 0, 0, 0};
  for (uint32_t k16 = 0; k16 < mq; k16 += 16) {
    uint32_t const k = k16 + 4 * kq;
    bf_d4 a = bf_d4{0, 0, 0, 0};
    if (okA) {
      if (VEC && k + 4 <= mq) {
        a = *(bf_d4 const *)(qrow + k);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k + e < mq) a[e] = qrow[k + e];
      }
    }
    double b[4][NT];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < NT; ++t) b[e][t] = C[(uint64_t)(k + e) * ld + 16 * (tj0 + t) + col];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], b[e][t], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint64_t const row = r0 + kq + 4 * g;
      if (row < n) {
        double *x = X + row * ld + 16 * (tj0 + t) + col;
        *x = *x - acc[t][g];
      }
    }
}

template <bool VEC> __global__ __launch_bounds__(64) void bfEigsDeflateKernel(double const *Q, uint64_t ldq, uint32_t mq, double const *C, double *X,
                                                                              uint64_t n, uint32_t ld) {
  uint32_t const tiles = ld / 16, tj0 = 4 * blockIdx.y, nt = tiles - tj0 < 4 ? tiles - tj0 : 4;
  for (uint64_t r0 = (uint64_t)blockIdx.x * 16; r0 < n; r0 += (uint64_t)gridDim.x * 16)
    switch (nt) {
      case 4: bfEigsDeflateTiles<4, VEC>(Q, ldq, mq, C, X, n, ld, r0, tj0); break;
      case 3: bfEigsDeflateTiles<3, VEC>(Q, ldq, mq, C, X, n, ld, r0, tj0); break;
      case 2: bfEigsDeflateTiles<2, VEC>(Q, ldq, mq, C, X, n, ld, r0, tj0); break;
      default: bfEigsDeflateTiles<1, VEC>(Q, ldq, mq, C, X, n, ld, r0, tj0); break;
    }
}

// ---- launches ------------------------------------------------------------------------------------------------------------
// rows per chunk of the Gram and residual partials: 1024 at least, more when that keeps the partials of a Gram matrix
// (chunks x ld x ld doubles) within 2^23 doubles; a multiple of 16 (four k-steps).  A function of (n, ld) alone.
uint64_t bfdevEigsChunkRows(uint64_t n, uint32_t ld) {
  uint64_t maxChunks = (1ull << 23) / ((uint64_t)ld * ld);
  if (maxChunks > 1024) maxChunks = 1024;
  if (maxChunks < 64) maxChunks = 64;
  uint64_t rows = (n + maxChunks - 1) / maxChunks;
  rows = (rows + 15) / 16 * 16;
  return rows < 1024 ? 1024 : rows;
}

int bfdevEigsStep(BfEigsStep const *s, void *stream) {
  if (!s->n || !s->p) return 0;
  uint32_t lg = 0;
  while ((1u << lg) < s->p && lg < 6) ++lg;
  uint64_t const perWg = 256u >> lg, need = (s->n + perWg - 1) / perWg;
  dim3 const grid((uint32_t)(need < BF_EIGS_MAX_GRID ? need : BF_EIGS_MAX_GRID)), block(256);
  hipLaunchKernelGGL(bfEigsStepKernel, grid, block, 0, (hipStream_t)stream, *s, lg);
  return bfHipFail(hipGetLastError(), "eigensolver step launch");
}

static int eigsReduce(double const *part, uint64_t chunks, uint64_t count, double *out, void *stream) {
  dim3 const grid((uint32_t)((count + 255) / 256)), block(256);
  hipLaunchKernelGGL(bfEigsReduceKernel, grid, block, 0, (hipStream_t)stream, part, chunks, count, out);
  return bfHipFail(hipGetLastError(), "eigensolver reduce launch");
}

int bfdevEigsGram(double const *X, double const *Y, uint64_t n, uint32_t ld, double *part, double *G, void *stream) {
  uint64_t const rows = bfdevEigsChunkRows(n, ld), chunks = (n + rows - 1) / rows;
  uint32_t const tiles = ld / 16;
  dim3 const grid((uint32_t)chunks, tiles, (tiles + 3) / 4), block(64);
  hipLaunchKernelGGL(bfEigsGramKernel, grid, block, 0, (hipStream_t)stream, X, Y, n, ld, rows, part);
  int const rc = bfHipFail(hipGetLastError(), "eigensolver Gram launch");
  return rc ? rc : eigsReduce(part, chunks, (uint64_t)ld * ld, G, stream);
}

int bfdevEigsRotate(double const *X, double const *W, double *out, uint64_t n, uint32_t ld, void *stream) {
  uint64_t const need = (n + 15) / 16;
  dim3 const grid((uint32_t)(need < BF_EIGS_MAX_GRID ? need : BF_EIGS_MAX_GRID), (ld / 16 + 3) / 4), block(64);
  hipLaunchKernelGGL(bfEigsRotateKernel, grid, block, 0, (hipStream_t)stream, X, W, out, n, ld);
  return bfHipFail(hipGetLastError(), "eigensolver rotate launch");
}

int bfdevEigsResidual(double const *X, double const *Y, double const *theta, uint64_t n, uint32_t ld, double *part, double *sumSq, void *stream) {
  uint64_t const rows = bfdevEigsChunkRows(n, ld), chunks = (n + rows - 1) / rows;
  dim3 const grid((uint32_t)chunks), block(256);
  hipLaunchKernelGGL(bfEigsResidualKernel, grid, block, 0, (hipStream_t)stream, X, Y, theta, n, ld, rows, part);
  int const rc = bfHipFail(hipGetLastError(), "eigensolver residual launch");
  return rc ? rc : eigsReduce(part, chunks, ld, sumSq, stream);
}

int bfdevEigsStore(double const *X, uint64_t n, uint32_t ld, uint32_t nev, double const *d, double *dst, uint64_t ldu, void *stream) {
  uint64_t const need = (n * nev + 255) / 256;
  dim3 const grid((uint32_t)(need < 65536 ? need : 65536)), block(256);
  hipLaunchKernelGGL(bfEigsStoreKernel, grid, block, 0, (hipStream_t)stream, X, n, ld, nev, d, dst, ldu);
  return bfHipFail(hipGetLastError(), "eigensolver store launch");
}

// rows per chunk of the cross-Gram partials (chunks x mq16 x ld doubles, mq16 <= 256): bfdevEigsChunkRows with 256 x ld in
// place of ld x ld, so a panel's partials stay within 2^23 doubles too.  A function of (n, ld) alone.
uint64_t bfdevEigsCrossChunkRows(uint64_t n, uint32_t ld) {
  uint64_t maxChunks = (1ull << 23) / (256ull * ld);
  if (maxChunks > 1024) maxChunks = 1024;
  if (maxChunks < 64) maxChunks = 64;
  uint64_t rows = (n + maxChunks - 1) / maxChunks;
  rows = (rows + 15) / 16 * 16;
  return rows < 1024 ? 1024 : rows;
}

int bfdevEigsCrossGram(double const *dQ, uint64_t ldq, uint64_t m0, uint32_t mq, double const *X, uint64_t n, uint32_t ld, double *part, double *C,
                       void *stream) {
  if (!mq || mq > 256 || !n) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "eigensolver cross-Gram: a panel of 1 .. 256 columns and n >= 1");
  uint64_t const rows = bfdevEigsCrossChunkRows(n, ld), chunks = (n + rows - 1) / rows;
  uint32_t const tiles = ld / 16, mq16 = (mq + 15) / 16 * 16;
  dim3 const grid((uint32_t)chunks, mq16 / 16, (tiles + 3) / 4), block(64);
  hipLaunchKernelGGL(bfEigsCrossGramKernel, grid, block, 0, (hipStream_t)stream, dQ + m0, ldq, mq, X, n, ld, rows, part);
  int const rc = bfHipFail(hipGetLastError(), "eigensolver cross-Gram launch");
  return rc ? rc : eigsReduce(part, chunks, (uint64_t)mq16 * ld, C, stream);
}

int bfdevEigsDeflate(double const *dQ, uint64_t ldq, uint64_t m0, uint32_t mq, double const *C, double *X, uint64_t n, uint32_t ld, void *stream) {
  if (!mq || mq > 256 || !n) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "eigensolver deflation: a panel of 1 .. 256 columns and n >= 1");
  uint64_t const need = (n + 15) / 16;
  dim3 const grid((uint32_t)(need < BF_EIGS_MAX_GRID ? need : BF_EIGS_MAX_GRID), (ld / 16 + 3) / 4), block(64);
  double const *Q = dQ + m0;
  if ((uintptr_t)Q % 32 == 0 && ldq % 4 == 0)
    hipLaunchKernelGGL(bfEigsDeflateKernel<true>, grid, block, 0, (hipStream_t)stream, Q, ldq, mq, C, X, n, ld);
  else
    hipLaunchKernelGGL(bfEigsDeflateKernel<false>, grid, block, 0, (hipStream_t)stream, Q, ldq, mq, C, X, n, ld);
  return bfHipFail(hipGetLastError(), "eigensolver deflation launch");
}

// one projection pass X <- X - Q (Q^T X) over all m locked columns: panels of at most 256, one after the other, coefficients
// then update (block modified Gram-Schmidt over panels); C never leaves the device
int bfdevEigsProject(double const *dQ, uint64_t ldq, uint64_t m, double *X, uint64_t n, uint32_t ld, double *part, double *C, void *stream) {
  for (uint64_t m0 = 0; m0 < m; m0 += 256) {
    uint32_t const mq = (uint32_t)(m - m0 < 256 ? m - m0 : 256);
    int rc;
    if ((rc = bfdevEigsCrossGram(dQ, ldq, m0, mq, X, n, ld, part, C, stream)) || (rc = bfdevEigsDeflate(dQ, ldq, m0, mq, C, X, n, ld, stream))) return rc;
  }
  return 0;
}
