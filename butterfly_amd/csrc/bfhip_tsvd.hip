// bfhip_tsvd.hip -- the kernels of the truncated SVD of a real f64 matrix (bfhipTruncSvdDevice, include/bfhip.h; host side:
// bfhip_tsvd.c; shared geometry: bfhip_tsvd.h): one-sided block Jacobi on the taller orientation.  The
// working block B is row-major M x ld, M >= N, ld = N rounded up to an even number of 16-column tiles; the padding columns are
// zero when the block is loaded and stay zero (a pair solve never rotates a zero column: the noise rule), so the dense kernels
// see whole tiles and need no column guard on B; rows are guarded wherever a tile or a chunk can pass M.
//
//   bfTsvdLoadKernel          B = A or A^T, padding zero
//   bfTsvdPairGramKernel      partial 32 x 32 Gram matrices of a step's tile pairs, per chunk of rows   v_mfma_f64_16x16x4_f64
//   bfTsvdPairSolveKernel     partials summed in chunk order; cyclic Jacobi in LDS; Q, sorted; flag    one workgroup per pair
//   bfTsvdPairRotateKernel    [B_I B_J] <- [B_I B_J] Q in place, flagged pairs only                    v_mfma_f64_16x16x4_f64
//   bfTsvdSumSqKernel         partial column sums of squares per chunk
//   bfTsvdReduceKernel        partials summed in chunk order
//   bfTsvdGatherKernel        the k kept columns, sorted and scaled, into a block of their own
//   bfTsvdGatherTKernel       the same columns transposed (W of the wide case)
//   bfTsvdContractKernel      partial X^T Y per chunk of rows, any leading dimensions, columns guarded  v_mfma_f64_16x16x4_f64
//   bfTsvdContractStoreKernel partials summed in chunk order into the caller's block
//   bfTsvdCopyColsKernel      the first k columns of a block into the caller's
//
// Every kernel's body is a __device__ function of one problem's parameters and of the workgroup's place in that problem's own
// grid (bfTsvd...Body).  The __global__ kernels above are thin wrappers with the grids they always had; the batched kernels of
// bfhipTruncSvdBatchDevice (the second half of this file) look their problem up in a device table and
// call the same bodies, so a problem meets the same instructions in the same order in a batch as alone.
//
// No floating-point atomic anywhere: every sum has one fixed order that depends on (m, n) alone, so two calls give the same
// bits.  The two integer atomics of the pair solve (a count, and a maximum over the bits of non-negative doubles) commute.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"
#include "bfhip_tsvd.h"

#define BF_TSVD_MAX_GRID (1u << 16)
typedef double bf_d4 __attribute__((ext_vector_type(4)));      // the C/D fragment of v_mfma_f64_16x16x4_f64, as in bfhip_eigs.hip

// (wg, wgs): the workgroup's index and count in the problem's own grid, as in every body below
static __device__ __forceinline__ void bfTsvdLoadBody(double const *A, uint64_t m, uint64_t n, uint64_t lda, int transpose, double *B, uint64_t M, uint32_t ld,
                                                      uint32_t wg, uint32_t wgs) {
  uint64_t const total = M * ld, N = transpose ? m : n;
  for (uint64_t e = (uint64_t)wg * 256 + threadIdx.x; e < total; e += (uint64_t)wgs * 256) {
    uint64_t const i = e / ld, j = e - i * ld;
    double v = 0;
    if (j < N) v = transpose ? A[j * lda + i] : A[i * lda + j];
    B[e] = v;
  }
}

__global__ __launch_bounds__(256) void bfTsvdLoadKernel(double const *A, uint64_t m, uint64_t n, uint64_t lda, int transpose, double *B, uint64_t M,
                                                        uint32_t ld) {
  bfTsvdLoadBody(A, m, n, lda, transpose, B, M, ld, blockIdx.x, gridDim.x);
}

// The Gram matrix of the 32 columns [B_I B_J] of pair `pair` (of `pairs`), rows of chunk `chunk`.  One wavefront; a k-step is four
// rows: lane l loads B[r + (l >> 4)][16 t + (l & 15)] of both tiles (128 contiguous bytes per row and tile), and the value is
// the A operand (a tile of P^T as it lies in memory) and the B operand alike.  II, IJ and JJ are accumulated; JI is IJ
// mirrored by the solve.  C/D: col = lane & 15, row = (lane >> 4) + 4 reg.  Four k-steps are requested before the first is
// used.  Rows at or past the chunk's end load zero.
static __device__ __forceinline__ void bfTsvdPairGramBody(double const *B, uint64_t M, uint32_t ld, uint32_t step, uint64_t chunkRows, double *part,
                                                          uint32_t chunk, uint32_t pair, uint32_t pairs) {
  constexpr int UNR = 4;
  uint32_t const lane = threadIdx.x, col = lane & 15, kq = lane >> 4, nt = ld / BF_TSVD_TILE;
  uint32_t ti, tj;
  bfTsvdPair(nt, step, pair, &ti, &tj);
  uint64_t const r0 = (uint64_t)chunk * chunkRows, r1 = r0 + chunkRows < M ? r0 + chunkRows : M;
  bf_d4 gii = bf_d4{0, 0, 0, 0}, gij = gii, gjj = gii;
  for (uint64_t r = r0; r < r1; r += 4 * UNR) {
    double a[UNR], b[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      uint64_t const row = r + 4 * u + kq;
      bool const ok = row < r1;
      a[u] = ok ? B[row * ld + 16 * ti + col] : 0.0;
      b[u] = ok ? B[row * ld + 16 * tj + col] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      gii = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], a[u], gii, 0, 0, 0);
      gij = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], gij, 0, 0, 0);
      gjj = __builtin_amdgcn_mfma_f64_16x16x4f64(b[u], b[u], gjj, 0, 0, 0);
    }
  }
  double *dst = part + ((uint64_t)chunk * pairs + pair) * (BF_TSVD_PAIR * BF_TSVD_PAIR);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    uint32_t const row = kq + 4 * g;
    dst[row * 32 + col] = gii[g];
    dst[row * 32 + 16 + col] = gij[g];
    dst[(16 + row) * 32 + 16 + col] = gjj[g];
  }
}

__global__ __launch_bounds__(64) void bfTsvdPairGramKernel(double const *B, uint64_t M, uint32_t ld, uint32_t step, uint64_t chunkRows, double *part) {
  bfTsvdPairGramBody(B, M, ld, step, chunkRows, part, blockIdx.x, blockIdx.y, gridDim.y);
}

// One workgroup of 256 per pair.  G = the partials summed in chunk order (upper triangle, mirrored).  The pair needs a
// rotation when some |g_ij| > thr sqrt(g_ii g_jj) with both columns above the noise level (g_ii, g_jj > noiseAbs, the same
// for every pair of the call); otherwise flag = 0 and nothing else is written.  The solve: cyclic Jacobi on G in the round-robin order of 32 indices
// (31 steps of 16 disjoint rotations: the 16 angles by 16 lanes, then the rows, then the columns of G and of V by all), an
// entry rotated while it is above 2 eps relative and both columns are above the noise level, at most BF_TSVD_INNER_SWEEPS
// sweeps; then Q = V with its columns in the order of descending eigenvalue (ties: the lower index first).
static __device__ __forceinline__ void bfTsvdPairSolveBody(double const *part, uint32_t chunks, double thr, double noiseAbs, double *Q, uint32_t *flag,
                                                           BfTsvdSweepState *state, uint32_t pair, uint32_t pairs) {
  __shared__ double G[32][33], V[32][33], cs[16], sn[16];
  __shared__ uint32_t pp[16], qq[16], order[32];
  __shared__ unsigned long long offBits;
  __shared__ int rot;
  uint32_t const tid = threadIdx.x;
  if (tid == 0) offBits = 0;
  for (uint32_t e = tid; e < 1024; e += 256) {
    uint32_t const i = e >> 5, j = e & 31;
    if (i <= j) {
      double s = 0;
      for (uint32_t c = 0; c < chunks; ++c) s += part[((uint64_t)c * pairs + pair) * 1024 + e];
      G[i][j] = s;
      G[j][i] = s;
    }
    V[i][j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  double worst = 0;
  for (uint32_t e = tid; e < 1024; e += 256) {
    uint32_t const i = e >> 5, j = e & 31;
    if (i < j) {
      double const di = G[i][i], dj = G[j][j];
      if (fmin(di, dj) > noiseAbs) worst = fmax(worst, fabs(G[i][j]) / sqrt(di * dj));
    }
  }
  if (worst > 0) atomicMax(&offBits, (unsigned long long)__double_as_longlong(worst));
  int const need = __syncthreads_or(worst > thr);
  if (tid == 0) atomicMax(&state->offBits, offBits);
  if (!need) {
    if (tid == 0) flag[pair] = 0;
    return;
  }
  for (uint32_t sw = 0; sw < BF_TSVD_INNER_SWEEPS; ++sw) {
    if (tid == 0) rot = 0;
    __syncthreads();
    for (uint32_t st = 0; st < 31; ++st) {
      if (tid < 16) {
        uint32_t p, q;
        bfTsvdPair(32, st, tid, &p, &q);
        double const a = G[p][p], d = G[q][q], b = G[p][q];
        double c = 1, s = 0;
        if (fmin(a, d) > noiseAbs && fabs(b) > 2 * BF_TSVD_EPS * sqrt(a * d)) {
          double const tau = (d - a) / (2 * b);
          double const t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1 + tau * tau));
          c = 1 / sqrt(1 + t * t);
          s = t * c;
          rot = 1;
        }
        pp[tid] = p; qq[tid] = q; cs[tid] = c; sn[tid] = s;
      }
      __syncthreads();
      for (uint32_t it = tid; it < 512; it += 256) {          // rows: G <- J^T G
        uint32_t const r = it >> 5, k = it & 31, p = pp[r], q = qq[r];
        double const c = cs[r], s = sn[r];
        if (s != 0) {
          double const gp = G[p][k], gq = G[q][k];
          G[p][k] = c * gp - s * gq;
          G[q][k] = s * gp + c * gq;
        }
      }
      __syncthreads();
      for (uint32_t it = tid; it < 512; it += 256) {          // columns: G <- G J, V <- V J
        uint32_t const r = it >> 5, k = it & 31, p = pp[r], q = qq[r];
        double const c = cs[r], s = sn[r];
        if (s != 0) {
          double const gp = G[k][p], gq = G[k][q];
          G[k][p] = c * gp - s * gq;
          G[k][q] = s * gp + c * gq;
          double const vp = V[k][p], vq = V[k][q];
          V[k][p] = c * vp - s * vq;
          V[k][q] = s * vp + c * vq;
        }
      }
      __syncthreads();
    }
    int const again = rot;
    __syncthreads();
    if (!again) break;
  }
  if (tid < 32) {
    double const d = G[tid][tid];
    uint32_t rank = 0;
    for (uint32_t i = 0; i < 32; ++i) {
      double const di = G[i][i];
      rank += (di > d || (di == d && i < tid)) ? 1u : 0u;
    }
    order[rank] = tid;
  }
  __syncthreads();
  double *dst = Q + (uint64_t)pair * 1024;
  for (uint32_t e = tid; e < 1024; e += 256) dst[e] = V[e >> 5][order[e & 31]];
  if (tid == 0) {
    flag[pair] = 1;
    atomicAdd(&state->rotated, 1ull);
  }
}

__global__ __launch_bounds__(256) void bfTsvdPairSolveKernel(double const *part, uint32_t chunks, double thr, double noiseAbs, double *Q, uint32_t *flag,
                                                             BfTsvdSweepState *state) {
  bfTsvdPairSolveBody(part, chunks, thr, noiseAbs, Q, flag, state, blockIdx.x, gridDim.x);
}

// [B_I B_J] <- [B_I B_J] Q for the flagged pairs, in place.  One wavefront per 16 rows (wg, stride wgs) and pair.  Lane (m = l & 15, kq = l >> 4) loads the four neighbours B[r0 + m][16 t + 4 kq + e], e < 4, of both tiles as one
// 32-byte request each; MFMA e of a tile contracts over the slots kq with B slot kq = Q[16 t' + 4 kq + e][.]: every index of
// the 32 is used exactly once, in an order that is fixed.  The wavefront is the only reader of the 16 x 32 panel it overwrites,
// and every load of it feeds the accumulators that the stores write.
static __device__ __forceinline__ void bfTsvdPairRotateBody(double *B, uint64_t M, uint32_t ld, uint32_t step, double const *Q, uint32_t const *flag,
                                                            uint32_t pair, uint32_t wg, uint32_t wgs) {
  if (!flag[pair]) return;
  uint32_t const lane = threadIdx.x, col = lane & 15, kq = lane >> 4, nt = ld / BF_TSVD_TILE;
  uint32_t ti, tj;
  bfTsvdPair(nt, step, pair, &ti, &tj);
  double const *Qp = Q + (uint64_t)pair * 1024;
  double q[2][4][2];            // [source tile][e][destination tile]
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 2; ++t) q[s][e][t] = Qp[(16 * s + 4 * kq + e) * 32 + 16 * t + col];
  for (uint64_t r0 = (uint64_t)wg * 16; r0 < M; r0 += (uint64_t)wgs * 16) {
    uint64_t const rowA = r0 + col;
    bool const okA = rowA < M;
    bf_d4 const zero = bf_d4{0, 0, 0, 0};
    bf_d4 const a0 = okA ? *(bf_d4 const *)(B + rowA * ld + 16 * ti + 4 * kq) : zero;
    bf_d4 const a1 = okA ? *(bf_d4 const *)(B + rowA * ld + 16 * tj + 4 * kq) : zero;
    bf_d4 acc[2] = {zero, zero};
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[e], q[0][e][t], acc[t], 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[e], q[1][e][t], acc[t], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint64_t const row = r0 + kq + 4 * g;
      if (row < M) {
        B[row * ld + 16 * ti + col] = acc[0][g];
        B[row * ld + 16 * tj + col] = acc[1][g];
      }
    }
  }
}

__global__ __launch_bounds__(64) void bfTsvdPairRotateKernel(double *B, uint64_t M, uint32_t ld, uint32_t step, double const *Q, uint32_t const *flag) {
  bfTsvdPairRotateBody(B, M, ld, step, Q, flag, blockIdx.y, blockIdx.x, gridDim.x);
}

// part[chunk][c] = sum over the chunk's rows of B[r][c]^2.  Thread (cl = t & 63, rl = t >> 6) walks the rows r0 + rl, r0 + rl + 4,
// ... of column cl of every panel of 64 columns; the four row lanes are summed through LDS in the order rl = 0, 1, 2, 3.
static __device__ __forceinline__ void bfTsvdSumSqBody(double const *B, uint64_t M, uint32_t ld, uint64_t chunkRows, double *part, uint32_t chunk) {
  __shared__ double sh[4][64];
  uint32_t const cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  uint64_t const r0 = (uint64_t)chunk * chunkRows, r1 = r0 + chunkRows < M ? r0 + chunkRows : M;
  for (uint32_t c0 = 0; c0 < ld; c0 += 64) {
    uint32_t const c = c0 + cl;
    double s = 0;
    if (c < ld)
      for (uint64_t r = r0 + rl; r < r1; r += 4) {
        double const v = B[r * ld + c];
        s = fma(v, v, s);
      }
    sh[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < ld) part[(uint64_t)chunk * ld + c] = ((sh[0][cl] + sh[1][cl]) + sh[2][cl]) + sh[3][cl];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void bfTsvdSumSqKernel(double const *B, uint64_t M, uint32_t ld, uint64_t chunkRows, double *part) {
  bfTsvdSumSqBody(B, M, ld, chunkRows, part, blockIdx.x);
}

// out[e] = part[0][e] + part[1][e] + ... in chunk order, e < count; chunk c starts at c * count
static __device__ __forceinline__ void bfTsvdReduceBody(double const *part, uint64_t chunks, uint64_t count, double *out, uint32_t wg) {
  uint64_t const e = (uint64_t)wg * 256 + threadIdx.x;
  if (e >= count) return;
  double s = 0;
  for (uint64_t c = 0; c < chunks; ++c) s += part[c * count + e];
  out[e] = s;
}

__global__ __launch_bounds__(256) void bfTsvdReduceKernel(double const *part, uint64_t chunks, uint64_t count, double *out) {
  bfTsvdReduceBody(part, chunks, count, out, blockIdx.x);
}

// out[i][j] = scale[j] * B[i][perm[j]] for j < k and exact zero for k <= j < kld
static __device__ __forceinline__ void bfTsvdGatherBody(double const *B, uint64_t M, uint32_t ld, uint32_t const *perm, double const *scale, uint64_t k,
                                                        double *out, uint32_t kld, uint32_t wg, uint32_t wgs) {
  uint64_t const total = M * kld;
  for (uint64_t e = (uint64_t)wg * 256 + threadIdx.x; e < total; e += (uint64_t)wgs * 256) {
    uint64_t const i = e / kld, j = e - i * kld;
    out[e] = j < k ? scale[j] * B[i * ld + perm[j]] : 0.0;
  }
}

__global__ __launch_bounds__(256) void bfTsvdGatherKernel(double const *B, uint64_t M, uint32_t ld, uint32_t const *perm, double const *scale, uint64_t k,
                                                          double *out, uint32_t kld) {
  bfTsvdGatherBody(B, M, ld, perm, scale, k, out, kld, blockIdx.x, gridDim.x);
}

// out[j][c] = B[c][perm[j]], j < k, c < M
static __device__ __forceinline__ void bfTsvdGatherTBody(double const *B, uint64_t M, uint32_t ld, uint32_t const *perm, uint64_t k, double *out,
                                                         uint64_t ldo, uint32_t wg, uint32_t wgs) {
  uint64_t const total = M * k;
  for (uint64_t e = (uint64_t)wg * 256 + threadIdx.x; e < total; e += (uint64_t)wgs * 256) {
    uint64_t const c = e / k, j = e - c * k;          // neighbours in j read one row of B
    out[j * ldo + c] = B[c * ld + perm[j]];
  }
}

__global__ __launch_bounds__(256) void bfTsvdGatherTKernel(double const *B, uint64_t M, uint32_t ld, uint32_t const *perm, uint64_t k, double *out,
                                                           uint64_t ldo) {
  bfTsvdGatherTBody(B, M, ld, perm, k, out, ldo, blockIdx.x, gridDim.x);
}

// C = X[:, :nx]^T Y[:, :ny] on the FP64 matrix cores, one partial per chunk of rows, as bfEigsGramTiles with both operands in
// their own leading dimension and their columns guarded (a column at or past nx / ny and a row at or past the chunk's end
// load exact zero).  part: [chunk][px][py], px = 16 gridDim.y, py = the tile columns of Y times 16.
template <int NT> static __device__ __forceinline__ void bfTsvdContractTiles(double const *X, uint64_t ldx, uint64_t nx, double const *Y, uint64_t ldy,
                                                                             uint64_t ny, uint64_t r0, uint64_t r1, uint32_t ti, uint32_t tj0, double *part,
                                                                             uint64_t py) {
  constexpr int UNR = 4;
  uint32_t const lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  bool const okX = 16 * (uint64_t)ti + col < nx;
  bool okY[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) okY[t] = 16 * (uint64_t)(tj0 + t) + col < ny;
  bf_d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = bf_d4{0, 0, 0, 0};
  for (uint64_t r = r0; r < r1; r += 4 * UNR) {
    double a[UNR], b[UNR][NT];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      uint64_t const row = r + 4 * u + kq;
      bool const ok = row < r1;
      a[u] = ok && okX ? X[row * ldx + 16 * ti + col] : 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t) b[u][t] = ok && okY[t] ? Y[row * ldy + 16 * (tj0 + t) + col] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u][t], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) part[(uint64_t)(16 * ti + kq + 4 * g) * py + 16 * (tj0 + t) + col] = acc[t][g];
}

// one workgroup of the grid (chunks, tile rows of X, groups of four tile columns of Y): (chunk, ti, group)
static __device__ __forceinline__ void bfTsvdContractBody(double const *X, uint64_t ldx, uint64_t nx, double const *Y, uint64_t ldy, uint64_t ny, uint64_t M,
                                                          uint64_t chunkRows, uint32_t tilesY, double *part, uint32_t chunk, uint32_t ti, uint32_t tilesX,
                                                          uint32_t group) {
  uint32_t const tj0 = 4 * group, nt = tilesY - tj0 < 4 ? tilesY - tj0 : 4;
  uint64_t const r0 = (uint64_t)chunk * chunkRows, r1 = r0 + chunkRows < M ? r0 + chunkRows : M;
  uint64_t const py = 16 * (uint64_t)tilesY;
  double *dst = part + (uint64_t)chunk * (16 * (uint64_t)tilesX) * py;
  switch (nt) {
    case 4: bfTsvdContractTiles<4>(X, ldx, nx, Y, ldy, ny, r0, r1, ti, tj0, dst, py); break;
    case 3: bfTsvdContractTiles<3>(X, ldx, nx, Y, ldy, ny, r0, r1, ti, tj0, dst, py); break;
    case 2: bfTsvdContractTiles<2>(X, ldx, nx, Y, ldy, ny, r0, r1, ti, tj0, dst, py); break;
    default: bfTsvdContractTiles<1>(X, ldx, nx, Y, ldy, ny, r0, r1, ti, tj0, dst, py); break;
  }
}

// grid: (chunks, tile rows of X, groups of four tile columns of Y)
__global__ __launch_bounds__(64) void bfTsvdContractKernel(double const *X, uint64_t ldx, uint64_t nx, double const *Y, uint64_t ldy, uint64_t ny, uint64_t M,
                                                           uint64_t chunkRows, uint32_t tilesY, double *part) {
  bfTsvdContractBody(X, ldx, nx, Y, ldy, ny, M, chunkRows, tilesY, part, blockIdx.x, blockIdx.y, gridDim.y, blockIdx.z);
}

// out[r][c] = part[0][r][c] + part[1][r][c] + ... in chunk order, r < nx, c < ny; a chunk is px x py
static __device__ __forceinline__ void bfTsvdContractStoreBody(double const *part, uint64_t chunks, uint64_t px, uint64_t py, uint64_t nx, uint64_t ny,
                                                               double *out, uint64_t ldo, uint32_t wg, uint32_t wgs) {
  uint64_t const total = nx * ny;
  for (uint64_t e = (uint64_t)wg * 256 + threadIdx.x; e < total; e += (uint64_t)wgs * 256) {
    uint64_t const r = e / ny, c = e - r * ny;
    double s = 0;
    for (uint64_t ch = 0; ch < chunks; ++ch) s += part[(ch * px + r) * py + c];
    out[r * ldo + c] = s;
  }
}

__global__ __launch_bounds__(256) void bfTsvdContractStoreKernel(double const *part, uint64_t chunks, uint64_t px, uint64_t py, uint64_t nx, uint64_t ny,
                                                                 double *out, uint64_t ldo) {
  bfTsvdContractStoreBody(part, chunks, px, py, nx, ny, out, ldo, blockIdx.x, gridDim.x);
}

static __device__ __forceinline__ void bfTsvdCopyColsBody(double const *X, uint64_t M, uint32_t ldx, uint64_t k, double *out, uint64_t ldo, uint32_t wg,
                                                          uint32_t wgs) {
  uint64_t const total = M * k;
  for (uint64_t e = (uint64_t)wg * 256 + threadIdx.x; e < total; e += (uint64_t)wgs * 256) {
    uint64_t const i = e / k, j = e - i * k;
    out[i * ldo + j] = X[i * ldx + j];
  }
}

__global__ __launch_bounds__(256) void bfTsvdCopyColsKernel(double const *X, uint64_t M, uint32_t ldx, uint64_t k, double *out, uint64_t ldo) {
  bfTsvdCopyColsBody(X, M, ldx, k, out, ldo, blockIdx.x, gridDim.x);
}

// ---- launches ------------------------------------------------------------------------------------------------------------
static inline uint32_t tsvdGrid(uint64_t items) {
  uint64_t const need = (items + 255) / 256;
  return (uint32_t)(need < BF_TSVD_MAX_GRID ? (need ? need : 1) : BF_TSVD_MAX_GRID);
}

int bfdevTsvdLoad(double const *dA, uint64_t m, uint64_t n, uint64_t lda, int transpose, double *B, uint32_t ld, void *stream) {
  uint64_t const M = transpose ? n : m;
  hipLaunchKernelGGL(bfTsvdLoadKernel, dim3(tsvdGrid(M * ld)), dim3(256), 0, (hipStream_t)stream, dA, m, n, lda, transpose, B, M, ld);
  return bfHipFail(hipGetLastError(), "truncated SVD load launch");
}

int bfdevTsvdStep(double *B, uint64_t M, uint32_t ld, uint32_t step, double thr, double noiseAbs, double *part, double *Q, uint32_t *flag,
                  BfTsvdSweepState *state, void *stream) {
  uint32_t const pairs = ld / BF_TSVD_PAIR;
  uint64_t const rows = bfTsvdChunkRows(M, ld), chunks = (M + rows - 1) / rows;
  int rc;
  hipLaunchKernelGGL(bfTsvdPairGramKernel, dim3((uint32_t)chunks, pairs), dim3(64), 0, (hipStream_t)stream, B, M, ld, step, rows, part);
  if ((rc = bfHipFail(hipGetLastError(), "truncated SVD pair Gram launch"))) return rc;
  hipLaunchKernelGGL(bfTsvdPairSolveKernel, dim3(pairs), dim3(256), 0, (hipStream_t)stream, part, (uint32_t)chunks, thr, noiseAbs, Q, flag, state);
  if ((rc = bfHipFail(hipGetLastError(), "truncated SVD pair solve launch"))) return rc;
  uint64_t const rowBlocks = (M + 15) / 16;
  hipLaunchKernelGGL(bfTsvdPairRotateKernel, dim3((uint32_t)(rowBlocks < 4096 ? rowBlocks : 4096), pairs), dim3(64), 0, (hipStream_t)stream, B, M, ld, step,
                     Q, flag);
  return bfHipFail(hipGetLastError(), "truncated SVD pair rotate launch");
}

int bfdevTsvdSumSq(double const *B, uint64_t M, uint32_t ld, double *part, double *out, void *stream) {
  uint64_t const rows = bfTsvdChunkRows(M, ld), chunks = (M + rows - 1) / rows;
  hipLaunchKernelGGL(bfTsvdSumSqKernel, dim3((uint32_t)chunks), dim3(256), 0, (hipStream_t)stream, B, M, ld, rows, part);
  int const rc = bfHipFail(hipGetLastError(), "truncated SVD column norms launch");
  if (rc) return rc;
  hipLaunchKernelGGL(bfTsvdReduceKernel, dim3((ld + 255) / 256), dim3(256), 0, (hipStream_t)stream, part, chunks, (uint64_t)ld, out);
  return bfHipFail(hipGetLastError(), "truncated SVD reduce launch");
}

int bfdevTsvdGather(double const *B, uint64_t M, uint32_t ld, uint32_t const *perm, double const *scale, uint64_t k, double *out, uint32_t kld,
                    void *stream) {
  hipLaunchKernelGGL(bfTsvdGatherKernel, dim3(tsvdGrid(M * kld)), dim3(256), 0, (hipStream_t)stream, B, M, ld, perm, scale, k, out, kld);
  return bfHipFail(hipGetLastError(), "truncated SVD gather launch");
}

int bfdevTsvdGatherT(double const *B, uint64_t M, uint32_t ld, uint32_t const *perm, uint64_t k, double *out, uint64_t ldo, void *stream) {
  hipLaunchKernelGGL(bfTsvdGatherTKernel, dim3(tsvdGrid(M * k)), dim3(256), 0, (hipStream_t)stream, B, M, ld, perm, k, out, ldo);
  return bfHipFail(hipGetLastError(), "truncated SVD transposed gather launch");
}

int bfdevTsvdContract(double const *X, uint64_t ldx, uint64_t nx, double const *Y, uint64_t ldy, uint64_t ny, uint64_t M, uint64_t chunkRows,
                      double *part, double *out, uint64_t ldo, void *stream) {
  uint64_t const chunks = (M + chunkRows - 1) / chunkRows, tilesX = (nx + 15) / 16, tilesY = (ny + 15) / 16;
  hipLaunchKernelGGL(bfTsvdContractKernel, dim3((uint32_t)chunks, (uint32_t)tilesX, (uint32_t)((tilesY + 3) / 4)), dim3(64), 0, (hipStream_t)stream, X, ldx, nx,
                     Y, ldy, ny, M, chunkRows, (uint32_t)tilesY, part);
  int const rc = bfHipFail(hipGetLastError(), "truncated SVD contraction launch");
  if (rc) return rc;
  hipLaunchKernelGGL(bfTsvdContractStoreKernel, dim3(tsvdGrid(nx * ny)), dim3(256), 0, (hipStream_t)stream, part, chunks, 16 * tilesX, 16 * tilesY, nx, ny, out,
                     ldo);
  return bfHipFail(hipGetLastError(), "truncated SVD contraction store launch");
}

int bfdevTsvdCopyCols(double const *X, uint64_t M, uint32_t ldx, uint64_t k, double *out, uint64_t ldo, void *stream) {
  hipLaunchKernelGGL(bfTsvdCopyColsKernel, dim3(tsvdGrid(M * k)), dim3(256), 0, (hipStream_t)stream, X, M, ldx, k, out, ldo);
  return bfHipFail(hipGetLastError(), "truncated SVD copy launch");
}

// ---- the batched kernels (bfhipTruncSvdBatchDevice; tables and launches: bfhip_tsvd_batch.h) -----------
// blockIdx.x is the problem (or the flat pair, whose problem `owner` names); blockIdx.y is the workgroup's place in that
// problem's own grid, sized by the largest problem of the group.  A workgroup reads its item, leaves if the problem is not
// active, has no such step or is smaller than the workgroup's place, and otherwise runs the single call's body on the problem's
// parameters: nothing in a body depends on the other problems, so a problem's bits are those of a call of its own.
#include "bfhip_tsvd_batch.h"

#define BF_TSVD_BATCH_WGS 1024u          // workgroups per problem of the grid-stride kernels, at most

__global__ __launch_bounds__(256) void bfTsvdBatchLoadKernel(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin) {
  uint32_t const p = blockIdx.x;
  if (fin && !(fin[p].ops & BF_TSVD_FIN_RELOAD)) return;
  BfTsvdBatchItem const *it = items + p;
  if ((uint64_t)blockIdx.y * 256 >= it->M * it->ld) return;
  bfTsvdLoadBody(it->A, it->m, it->n, it->lda, (int)it->transposed, it->B, it->M, it->ld, blockIdx.y, gridDim.y);
}

__global__ __launch_bounds__(64) void bfTsvdBatchPairGramKernel(BfTsvdBatchItem const *items, BfTsvdBatchWords const *words, uint32_t const *owner,
                                                                uint32_t step) {
  uint32_t const flat = blockIdx.x, p = owner[flat];
  BfTsvdBatchItem const *it = items + p;
  uint32_t pair, ti, tj;
  if (!words[p].active || blockIdx.y >= it->chunks || !bfTsvdBatchPair(it->nt, it->pairBase, flat, step, &pair, &ti, &tj)) return;
  bfTsvdPairGramBody(it->B, it->M, it->ld, step, it->chunkRows, it->part, blockIdx.y, pair, it->nt / 2);
}

__global__ __launch_bounds__(256) void bfTsvdBatchPairSolveKernel(BfTsvdBatchItem const *items, BfTsvdBatchWords *words, uint32_t const *owner, uint32_t step) {
  uint32_t const flat = blockIdx.x, p = owner[flat];
  BfTsvdBatchItem const *it = items + p;
  uint32_t pair, ti, tj;
  if (!words[p].active || !bfTsvdBatchPair(it->nt, it->pairBase, flat, step, &pair, &ti, &tj)) return;
  bfTsvdPairSolveBody(it->part, it->chunks, it->thr, words[p].noiseAbs, it->Q, it->flag, &words[p].state, pair, it->nt / 2);
}

__global__ __launch_bounds__(64) void bfTsvdBatchPairRotateKernel(BfTsvdBatchItem const *items, BfTsvdBatchWords const *words, uint32_t const *owner,
                                                                  uint32_t step) {
  uint32_t const flat = blockIdx.x, p = owner[flat];
  BfTsvdBatchItem const *it = items + p;
  uint32_t pair, ti, tj;
  if (!words[p].active || (uint64_t)blockIdx.y * 16 >= it->M || !bfTsvdBatchPair(it->nt, it->pairBase, flat, step, &pair, &ti, &tj)) return;
  bfTsvdPairRotateBody(it->B, it->M, it->ld, step, it->Q, it->flag, pair, blockIdx.y, gridDim.y);
}

// one thread per problem: the end of a sweep
__global__ __launch_bounds__(256) void bfTsvdBatchEndSweepKernel(BfTsvdBatchWords *words, uint32_t count, uint32_t maxSweeps) {
  uint32_t const p = blockIdx.x * 256 + threadIdx.x;
  if (p >= count) return;
  BfTsvdBatchWords *w = words + p;
  if (!w->active) return;
  uint32_t const s = w->sweeps + 1;
  w->sweeps = s;
  if (!w->state.rotated || s >= maxSweeps) w->active = 0;
  else { w->state.rotated = 0; w->state.offBits = 0; }
}

__global__ __launch_bounds__(256) void bfTsvdBatchSumSqKernel(BfTsvdBatchItem const *items) {
  BfTsvdBatchItem const *it = items + blockIdx.x;
  if (blockIdx.y >= it->chunks) return;
  bfTsvdSumSqBody(it->B, it->M, it->ld, it->chunkRows, it->part, blockIdx.y);
}

__global__ __launch_bounds__(256) void bfTsvdBatchReduceKernel(BfTsvdBatchItem const *items) {
  BfTsvdBatchItem const *it = items + blockIdx.x;
  if (blockIdx.y * 256u >= it->ld) return;
  bfTsvdReduceBody(it->part, it->chunks, it->ld, it->sumSq, blockIdx.y);
}

__global__ __launch_bounds__(256) void bfTsvdBatchSigmaKernel(BfTsvdBatchFin const *fin) {
  BfTsvdBatchFin const *f = fin + blockIdx.x;
  if (!(f->ops & BF_TSVD_FIN_SIGMA)) return;
  for (uint64_t e = (uint64_t)blockIdx.y * 256 + threadIdx.x; e < f->N; e += (uint64_t)gridDim.y * 256) f->dSigma[e] = f->sigma[e];
}

__global__ __launch_bounds__(256) void bfTsvdBatchGatherKernel(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin) {
  BfTsvdBatchFin const *f = fin + blockIdx.x;
  BfTsvdBatchItem const *it = items + blockIdx.x;
  if (!(f->ops & BF_TSVD_FIN_GATHER) || (uint64_t)blockIdx.y * 256 >= it->M * f->kld) return;
  bfTsvdGatherBody(it->B, it->M, it->ld, f->perm, f->scale, f->k, f->Bs, f->kld, blockIdx.y, gridDim.y);
}

__global__ __launch_bounds__(256) void bfTsvdBatchGatherTKernel(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin) {
  BfTsvdBatchFin const *f = fin + blockIdx.x;
  BfTsvdBatchItem const *it = items + blockIdx.x;
  if (!(f->ops & BF_TSVD_FIN_GATHERT) || (uint64_t)blockIdx.y * 256 >= it->M * f->k) return;
  bfTsvdGatherTBody(it->B, it->M, it->ld, f->perm, f->k, f->dW, f->ldw, blockIdx.y, gridDim.y);
}

__global__ __launch_bounds__(256) void bfTsvdBatchCopyColsKernel(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin) {
  BfTsvdBatchFin const *f = fin + blockIdx.x;
  BfTsvdBatchItem const *it = items + blockIdx.x;
  if (!(f->ops & BF_TSVD_FIN_COPY) || (uint64_t)blockIdx.y * 256 >= it->M * f->k) return;
  bfTsvdCopyColsBody(f->Bs, it->M, f->kld, f->k, f->dU, f->ldu, blockIdx.y, gridDim.y);
}

// the operands of a problem's one contraction.  Tall: W = U^T A (X = the gathered block, Y = A).  Wide: U = (A^T)^T (B_k diag(..))
// (X = B reloaded with A^T, Y = the gathered block)
struct BfTsvdBatchContractArgs { double const *X, *Y; uint64_t ldx, nx, ldy, ny, ldo; double *out; };
static __device__ __forceinline__ BfTsvdBatchContractArgs bfTsvdBatchContractOf(BfTsvdBatchItem const *it, BfTsvdBatchFin const *f) {
  BfTsvdBatchContractArgs a;
  if (!it->transposed) { a.X = f->Bs; a.ldx = f->kld; a.nx = f->k; a.Y = it->A; a.ldy = it->lda; a.ny = it->n; a.out = f->dW; a.ldo = f->ldw; }
  else { a.X = it->B; a.ldx = it->ld; a.nx = f->N; a.Y = f->Bs; a.ldy = f->kld; a.ny = f->k; a.out = f->dU; a.ldo = f->ldu; }
  return a;
}

// grid: (problems, chunks of the largest, tile work of the largest capped at 65535 and walked with that stride)
__global__ __launch_bounds__(64) void bfTsvdBatchContractKernel(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin) {
  BfTsvdBatchFin const *f = fin + blockIdx.x;
  BfTsvdBatchItem const *it = items + blockIdx.x;
  if (!(f->ops & BF_TSVD_FIN_CONTRACT) || blockIdx.y >= f->cchunks) return;
  BfTsvdBatchContractArgs const a = bfTsvdBatchContractOf(it, f);
  uint32_t const tilesX = (uint32_t)((a.nx + 15) / 16), tilesY = (uint32_t)((a.ny + 15) / 16), groups = (tilesY + 3) / 4;
  for (uint32_t w = blockIdx.z; w < tilesX * groups; w += gridDim.z)
    bfTsvdContractBody(a.X, a.ldx, a.nx, a.Y, a.ldy, a.ny, it->M, f->crows, tilesY, f->cpart, blockIdx.y, w / groups, tilesX, w % groups);
}

__global__ __launch_bounds__(256) void bfTsvdBatchContractStoreKernel(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin) {
  BfTsvdBatchFin const *f = fin + blockIdx.x;
  BfTsvdBatchItem const *it = items + blockIdx.x;
  if (!(f->ops & BF_TSVD_FIN_CONTRACT)) return;
  BfTsvdBatchContractArgs const a = bfTsvdBatchContractOf(it, f);
  if ((uint64_t)blockIdx.y * 256 >= a.nx * a.ny) return;
  bfTsvdContractStoreBody(f->cpart, f->cchunks, (a.nx + 15) / 16 * 16, (a.ny + 15) / 16 * 16, a.nx, a.ny, a.out, a.ldo, blockIdx.y, gridDim.y);
}

// ---- batched launches ----------------------------------------------------------------------------------------------------
static inline uint32_t tsvdBatchWgs(uint64_t maxItems) {
  uint64_t const need = (maxItems + 255) / 256;
  return (uint32_t)(need < BF_TSVD_BATCH_WGS ? (need ? need : 1) : BF_TSVD_BATCH_WGS);
}

int bfdevTsvdBatchLoad(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream) {
  hipLaunchKernelGGL(bfTsvdBatchLoadKernel, dim3(count, tsvdBatchWgs(maxElems)), dim3(256), 0, (hipStream_t)stream, items, fin);
  return bfHipFail(hipGetLastError(), "batched truncated SVD load launch");
}

int bfdevTsvdBatchStep(BfTsvdBatchItem const *items, BfTsvdBatchWords *words, uint32_t const *owner, uint32_t totalPairs, uint32_t step,
                       uint32_t maxChunks, uint64_t maxRows, void *stream) {
  int rc;
  hipLaunchKernelGGL(bfTsvdBatchPairGramKernel, dim3(totalPairs, maxChunks), dim3(64), 0, (hipStream_t)stream, items, words, owner, step);
  if ((rc = bfHipFail(hipGetLastError(), "batched truncated SVD pair Gram launch"))) return rc;
  hipLaunchKernelGGL(bfTsvdBatchPairSolveKernel, dim3(totalPairs), dim3(256), 0, (hipStream_t)stream, items, words, owner, step);
  if ((rc = bfHipFail(hipGetLastError(), "batched truncated SVD pair solve launch"))) return rc;
  uint64_t const rowBlocks = (maxRows + 15) / 16;
  hipLaunchKernelGGL(bfTsvdBatchPairRotateKernel, dim3(totalPairs, (uint32_t)(rowBlocks < 4096 ? rowBlocks : 4096)), dim3(64), 0, (hipStream_t)stream, items,
                     words, owner, step);
  return bfHipFail(hipGetLastError(), "batched truncated SVD pair rotate launch");
}

int bfdevTsvdBatchEndSweep(BfTsvdBatchWords *words, uint32_t count, uint32_t maxSweeps, void *stream) {
  hipLaunchKernelGGL(bfTsvdBatchEndSweepKernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, words, count, maxSweeps);
  return bfHipFail(hipGetLastError(), "batched truncated SVD end-of-sweep launch");
}

int bfdevTsvdBatchSumSq(BfTsvdBatchItem const *items, uint32_t count, uint32_t maxChunks, uint32_t maxLd, void *stream) {
  hipLaunchKernelGGL(bfTsvdBatchSumSqKernel, dim3(count, maxChunks), dim3(256), 0, (hipStream_t)stream, items);
  int const rc = bfHipFail(hipGetLastError(), "batched truncated SVD column norms launch");
  if (rc) return rc;
  hipLaunchKernelGGL(bfTsvdBatchReduceKernel, dim3(count, (maxLd + 255) / 256), dim3(256), 0, (hipStream_t)stream, items);
  return bfHipFail(hipGetLastError(), "batched truncated SVD reduce launch");
}

int bfdevTsvdBatchSigma(BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxN, void *stream) {
  hipLaunchKernelGGL(bfTsvdBatchSigmaKernel, dim3(count, tsvdBatchWgs(maxN)), dim3(256), 0, (hipStream_t)stream, fin);
  return bfHipFail(hipGetLastError(), "batched truncated SVD sigma launch");
}

int bfdevTsvdBatchGather(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream) {
  hipLaunchKernelGGL(bfTsvdBatchGatherKernel, dim3(count, tsvdBatchWgs(maxElems)), dim3(256), 0, (hipStream_t)stream, items, fin);
  return bfHipFail(hipGetLastError(), "batched truncated SVD gather launch");
}

int bfdevTsvdBatchGatherT(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream) {
  hipLaunchKernelGGL(bfTsvdBatchGatherTKernel, dim3(count, tsvdBatchWgs(maxElems)), dim3(256), 0, (hipStream_t)stream, items, fin);
  return bfHipFail(hipGetLastError(), "batched truncated SVD transposed gather launch");
}

int bfdevTsvdBatchCopyCols(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream) {
  hipLaunchKernelGGL(bfTsvdBatchCopyColsKernel, dim3(count, tsvdBatchWgs(maxElems)), dim3(256), 0, (hipStream_t)stream, items, fin);
  return bfHipFail(hipGetLastError(), "batched truncated SVD copy launch");
}

int bfdevTsvdBatchContract(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint32_t maxChunks, uint64_t maxTileWork, void *stream) {
  hipLaunchKernelGGL(bfTsvdBatchContractKernel, dim3(count, maxChunks, (uint32_t)(maxTileWork < 65535 ? (maxTileWork ? maxTileWork : 1) : 65535)), dim3(64), 0,
                     (hipStream_t)stream, items, fin);
  return bfHipFail(hipGetLastError(), "batched truncated SVD contraction launch");
}

int bfdevTsvdBatchContractStore(BfTsvdBatchItem const *items, BfTsvdBatchFin const *fin, uint32_t count, uint64_t maxElems, void *stream) {
  hipLaunchKernelGGL(bfTsvdBatchContractStoreKernel, dim3(count, tsvdBatchWgs(maxElems)), dim3(256), 0, (hipStream_t)stream, items, fin);
  return bfHipFail(hipGetLastError(), "batched truncated SVD contraction store launch");
}
