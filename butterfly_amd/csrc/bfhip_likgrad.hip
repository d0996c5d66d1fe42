// bfhip_likgrad.hip -- the kernels of the likelihood gradient in the density's parameters on the Chebyshev route
// (bfhipChebCovCondLogLikGradDevice, include/bfhip.h; host side: bfhip_cheb.c).  Everything is
// double; every index into a matrix is 64 bits; no atomics: each output element has one owner and every sum a fixed order
// that depends on the shapes alone.
//
//   d logLik / d theta_t = < X M, X'_t >_F,   M = alpha alpha^T - K^-1 [k x k],   X = Bt [n x k],   X'_t = q_t(S) D E_obs
//
// walked in panels of pc <= 64 observed columns.  Matrices (row-major): X [n x k] packed at k; Mp [k x 64] = the panel's
// columns of M, of which columns >= pc are never read; Y [n x 64] = X Mp; Xp [n x pc] packed at pc = the panel of X'_t as
// the recurrence leaves it.
//
//   bfLikGradUnitKernel      the panel's columns of the identity, packed at pc (the right-hand sides of the two solves)
//   bfLikGradMKernel         Mp[a, c] = alpha[a] alpha[c0 + c] - Kinv[a, c]
//   bfLikGradContractKernel  Y = X Mp                                           v_mfma_f64_16x16x4_f64
//   bfLikGradDotKernel       part[chunk] = sum over the chunk's rows and c < pc of Y[r, c] Xp[r, c]
//   bfLikGradSumKernel       grad[t] (+)= sum_chunk part[t][chunk] in chunk order, one thread per t

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bfhip_cond.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"

#define BF_LIKGRAD_LD 64u                // columns of Mp and Y: a panel
#define BF_LIKGRAD_MAX_GRID (1u << 20)
typedef double bf_d4 __attribute__((ext_vector_type(4)));      // the C/D fragment of v_mfma_f64_16x16x4_f64

// ---------------------------------------------------------------------------
// the panel of M
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bfLikGradUnitKernel(double *E, uint32_t k, uint32_t c0, uint32_t pc) {
  uint64_t const e = (uint64_t)blockIdx.x * 256 + threadIdx.x, total = (uint64_t)k * pc;
  if (e >= total) return;
  uint64_t const a = e / pc, c = e - a * pc;
  E[e] = a == c0 + c ? 1.0 : 0.0;
}

// One rounding per element: fma(alpha[a], alpha[c0 + c], -Kinv[a, c]).  Columns pc .. 63 are written as zeros.
__global__ __launch_bounds__(256) void bfLikGradMKernel(double *Mp, double const *alpha, double const *Kinv, uint32_t k, uint32_t c0, uint32_t pc) {
  uint64_t const e = (uint64_t)blockIdx.x * 256 + threadIdx.x, total = (uint64_t)k * BF_LIKGRAD_LD;
  if (e >= total) return;
  uint32_t const a = (uint32_t)(e / BF_LIKGRAD_LD), c = (uint32_t)(e % BF_LIKGRAD_LD);
  Mp[e] = c < pc ? fma(alpha[a], alpha[c0 + c], -Kinv[(uint64_t)a * pc + c]) : 0.0;
}

// ---------------------------------------------------------------------------
// the contraction Y = X Mp on the FP64 matrix cores
// ---------------------------------------------------------------------------
// The lane layout of bfEigsRotateKernel (bfhip_eigs.hip): one wavefront per workgroup owns 16 rows and the NT = ceil(pc / 16)
// live tile columns of the panel.  The contraction index is walked in blocks of 16: lane (m = l & 15, kq = l >> 4) holds
// X[r0 + m][k16 + 4 kq + e], e < 4 (the four lanes of a row cover 128 contiguous bytes), and MFMA e of the block contracts
// over the slots kq with B slot kq = Mp[k16 + 4 kq + e][.]: every index below k is used exactly once, in a fixed order.
// k is ragged (any value, rows of X need not be 32-byte aligned): every load is one double under a guard, an index at or past
// k loads zero for both operands, and so does a row at or past n or a column at or past pc -- nothing outside X [n x k] and the
// first pc columns of Mp's k rows is read.  The loads of the next block are requested before the four MFMAs of this one.
// Columns pc .. 63 of Y are written as exact zeros (+0: tiles without a live column are stored without an MFMA, and the dead
// columns of a live tile accumulate fma(x, +0, +0) with finite x).
template <int NT> struct BfLikGradFrag { double a[4]; double b[4][NT]; };

template <int NT> static __device__ __forceinline__ void bfLikGradLoad(BfLikGradFrag<NT> &f, double const *xrow, bool okA, double const *Mp, uint32_t k,
                                                                       uint32_t pc, uint32_t k16, uint32_t kq, uint32_t col) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    uint32_t const kk = k16 + 4 * kq + e;
    bool const okK = kk < k;
    f.a[e] = (okA && okK) ? xrow[kk] : 0.0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      uint32_t const c = 16 * t + col;
      f.b[e][t] = (okK && c < pc) ? Mp[(uint64_t)kk * BF_LIKGRAD_LD + c] : 0.0;
    }
  }
}

template <int NT> static __device__ __forceinline__ void bfLikGradTiles(double *Y, double const *X, uint64_t n, uint32_t k, double const *Mp, uint32_t pc,
                                                                        uint64_t r0) {
  uint32_t const lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  uint64_t const rowA = r0 + col;
  bool const okA = rowA < n;
  double const *xrow = X + (okA ? rowA : 0) * k;
  bf_d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = bf_d4{0, 0, 0, 0};
  BfLikGradFrag<NT> cur, nxt;
  bfLikGradLoad<NT>(cur, xrow, okA, Mp, k, pc, 0, kq, col);
  nxt = cur;
  for (uint32_t k16 = 0; k16 < k; k16 += 16) {
    if (k16 + 16 < k) bfLikGradLoad<NT>(nxt, xrow, okA, Mp, k, pc, k16 + 16, kq, col);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.a[e], cur.b[e][t], acc[t], 0, 0, 0);
    cur = nxt;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    uint64_t const row = r0 + kq + 4 * g;
    if (row < n) {
#pragma unroll
      for (int t = 0; t < 4; ++t) Y[row * BF_LIKGRAD_LD + 16 * t + col] = t < NT ? acc[t < NT ? t : 0][g] : 0.0;
    }
  }
}

__global__ __launch_bounds__(64) void bfLikGradContractKernel(double *Y, double const *X, uint64_t n, uint32_t k, double const *Mp, uint32_t pc) {
  uint32_t const nt = (pc + 15) / 16;
  for (uint64_t r0 = (uint64_t)blockIdx.x * 16; r0 < n; r0 += (uint64_t)gridDim.x * 16)
    switch (nt) {
      case 4: bfLikGradTiles<4>(Y, X, n, k, Mp, pc, r0); break;
      case 3: bfLikGradTiles<3>(Y, X, n, k, Mp, pc, r0); break;
      case 2: bfLikGradTiles<2>(Y, X, n, k, Mp, pc, r0); break;
      default: bfLikGradTiles<1>(Y, X, n, k, Mp, pc, r0); break;
    }
}

// ---------------------------------------------------------------------------
// the dot and the owner's sum
// ---------------------------------------------------------------------------
// Workgroup `chunk` walks the BF_COND_CHUNK rows of its chunk: thread t takes the elements t, t + 256, ... of the chunk's
// rows x pc block of Xp (contiguous) by fma from zero, then the 256 sums meet in LDS and are halved in a fixed order
// (s[i] += s[i + w], w = 128 .. 1).  Columns >= pc of Y are not read.  part[chunk] is written, not added to.
__global__ __launch_bounds__(256) void bfLikGradDotKernel(double *part, double const *Y, double const *Xp, uint64_t n, uint32_t pc) {
  __shared__ double sh[256];
  uint64_t const r0 = (uint64_t)blockIdx.x * BF_COND_CHUNK, r1 = r0 + BF_COND_CHUNK < n ? r0 + BF_COND_CHUNK : n;
  uint32_t const total = (uint32_t)(r1 - r0) * pc;
  double const *xp = Xp + r0 * pc, *y = Y + r0 * BF_LIKGRAD_LD;
  double s = 0.0;
  for (uint32_t e = threadIdx.x; e < total; e += 256) {
    uint32_t const r = e / pc, c = e - r * pc;
    s = fma(y[(uint64_t)r * BF_LIKGRAD_LD + c], xp[e], s);
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (uint32_t w = 128; w; w >>= 1) {
    if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// grad[t] = (first ? 0 : grad[t]) + (part[t][0] + part[t][1] + ...): the panels in order, each panel's chunks in order
__global__ __launch_bounds__(64) void bfLikGradSumKernel(double *grad, double const *part, uint64_t chunks, uint32_t numParams, int first) {
  uint32_t const t = blockIdx.x * 64 + threadIdx.x;
  if (t >= numParams) return;
  double s = 0.0;
  for (uint64_t c = 0; c < chunks; ++c) s += part[(uint64_t)t * chunks + c];
  grad[t] = first ? s : grad[t] + s;
}

// ---- launches ------------------------------------------------------------------------------------------------------------
int bfdevLikGradUnit(double *E, uint32_t k, uint32_t c0, uint32_t pc, void *stream) {
  if (!k || !pc || pc > BF_LIKGRAD_LD || c0 + pc > k) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "gradient unit block: a panel of 1 .. 64 columns inside k");
  hipLaunchKernelGGL(bfLikGradUnitKernel, dim3((uint32_t)(((uint64_t)k * pc + 255) / 256)), dim3(256), 0, (hipStream_t)stream, E, k, c0, pc);
  return bfHipFail(hipGetLastError(), "gradient unit block launch");
}

int bfdevLikGradM(double *Mp, double const *alpha, double const *Kinv, uint32_t k, uint32_t c0, uint32_t pc, void *stream) {
  if (!k || !pc || pc > BF_LIKGRAD_LD || c0 + pc > k) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "gradient M panel: a panel of 1 .. 64 columns inside k");
  hipLaunchKernelGGL(bfLikGradMKernel, dim3((uint32_t)(((uint64_t)k * BF_LIKGRAD_LD + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Mp, alpha, Kinv, k, c0, pc);
  return bfHipFail(hipGetLastError(), "gradient M panel launch");
}

int bfdevLikGradContract(double *Y, double const *X, uint64_t n, uint32_t k, double const *Mp, uint32_t pc, void *stream) {
  if (!n || !k || !pc || pc > BF_LIKGRAD_LD) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "gradient contraction: n, k >= 1 and a panel of 1 .. 64 columns");
  uint64_t const need = (n + 15) / 16;
  dim3 const grid((uint32_t)(need < BF_LIKGRAD_MAX_GRID ? need : BF_LIKGRAD_MAX_GRID)), block(64);
  hipLaunchKernelGGL(bfLikGradContractKernel, grid, block, 0, (hipStream_t)stream, Y, X, n, k, Mp, pc);
  return bfHipFail(hipGetLastError(), "gradient contraction launch");
}

int bfdevLikGradDot(double *part, double const *Y, double const *Xp, uint64_t n, uint32_t pc, void *stream) {
  if (!n || !pc || pc > BF_LIKGRAD_LD || !bfdevCondFits(n)) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "gradient dot: 1 .. 65535 chunks and a panel of 1 .. 64 columns");
  uint64_t const chunks = (n + BF_COND_CHUNK - 1) / BF_COND_CHUNK;
  hipLaunchKernelGGL(bfLikGradDotKernel, dim3((uint32_t)chunks), dim3(256), 0, (hipStream_t)stream, part, Y, Xp, n, pc);
  return bfHipFail(hipGetLastError(), "gradient dot launch");
}

int bfdevLikGradSum(double *grad, double const *part, uint64_t chunks, uint32_t numParams, int first, void *stream) {
  if (!numParams) return 0;
  hipLaunchKernelGGL(bfLikGradSumKernel, dim3((numParams + 63) / 64), dim3(64), 0, (hipStream_t)stream, grad, part, chunks, numParams, first);
  return bfHipFail(hipGetLastError(), "gradient sum launch");
}
