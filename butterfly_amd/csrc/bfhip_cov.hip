// bfhip_cov.hip -- the vector plumbing of the batched covariance entries (bfhipCovSampleBlockDevice,
// bfhipCovMatvecBlockDevice, bfhipCovDrawDevice, bfhipCovMomentsDevice, bfhipFillNormalDevice; host side: bfhip_api.c).
// Nothing here is a stage kernel: the operator is applied by runPlan, these kernels prepare its input block and consume its
// result block.  All blocks are row-major rows x nrhs, densely packed; every index is 64 bits (1M rows x 64 columns of
// fp32 is 256 MiB, and an element index of the F64 block passes 2^32 in bytes long before that).
//
// All three kernels are bound by memory traffic (the fill by log / cos on 4M elements: microseconds), move every byte
// once, and use 16-byte accesses wherever a row is a whole number of them.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"
#include "../../include/bfhip_synth.h"

#define BF_COV_MAX_GRID 65536u          // workgroups per launch; the rest is walked with a grid stride

template <typename S> struct CovVec;      // 16 bytes of S
template <> struct CovVec<double> { using V = double2; static constexpr int N = 2; };
template <> struct CovVec<float> { using V = float4; static constexpr int N = 4; };

// workgroup shape shared by the kernels below: `lanes` (a power of two <= 256) neighbouring threads walk one row, so a
// workgroup of 256 covers 256 / lanes rows; lanes = 1 at one column is the thread-per-element shape of bfScalePermuteKernel
static uint32_t covLanes(uint64_t perRow, uint32_t cap) {
  uint32_t l = 1;
  while (l < perRow && l < cap) l <<= 1;
  return l;
}
static uint32_t covGrid(uint64_t rows, uint32_t lanes) {
  uint64_t const perWg = 256 / lanes, need = (rows + perWg - 1) / perWg;
  return (uint32_t)(need < BF_COV_MAX_GRID ? need : BF_COV_MAX_GRID);
}

// ---------------------------------------------------------------------------
// block scale / scatter: dst[perm ? perm[i] : i, :] = src[i, :] * (scale ? scale[i]^power : 1)
// ---------------------------------------------------------------------------
// bfScalePermuteKernel (bfhip_device.hip) on rows of `nrhs` elements, with the same arithmetic per element (v * g, or
// v * (g * g) at power 2: one column gives the single-vector entries' bits).  A thread owns piece c of row i, for
// c = lane, lane + lanes, ...: a 16-byte piece (VEC: a row is a whole number of them and both bases are 16-byte
// aligned) or one element.  scale[i] and perm[i] are read once per row by each of the row's lanes -- one address per
// row, one request -- and kept in registers across the row's pieces.  Every piece is read and written by the same
// thread, so src == dst is legal when perm == NULL (the matvec scales its intermediate in place); with a permutation
// the caller passes distinct buffers.  A row index outside the block (not a permutation) is dropped, never written.
template <typename S, bool VEC>
__global__ __launch_bounds__(256) void bfCovScalePermuteKernel(S *dst, S const *src, S const *scale, int power, uint64_t const *perm,
                                                               uint64_t rows, uint32_t nrhs, uint32_t lanesLog2) {
  using V = typename CovVec<S>::V;
  constexpr uint32_t N = CovVec<S>::N;
  uint32_t const lanes = 1u << lanesLog2, lane = threadIdx.x & (lanes - 1), rowsPerWg = 256u >> lanesLog2;
  uint32_t const perRow = VEC ? nrhs / N : nrhs;
  for (uint64_t i = (uint64_t)blockIdx.x * rowsPerWg + (threadIdx.x >> lanesLog2); i < rows; i += (uint64_t)gridDim.x * rowsPerWg) {
    S g = 1;
    if (scale) { S const s = scale[i]; g = power == 2 ? s * s : s; }
    uint64_t const j = perm ? perm[i] : i;
    if (j >= rows) continue;
    if (VEC) {
      V const *in = (V const *)(src + i * nrhs);
      V *out = (V *)(dst + j * nrhs);
      for (uint32_t c = lane; c < perRow; c += lanes) {
        V v = in[c];
        if (scale) {
          v.x *= g; v.y *= g;
          if constexpr (N == 4) { v.z *= g; v.w *= g; }
        }
        out[c] = v;
      }
    } else {
      S const *in = src + i * nrhs;
      S *out = dst + j * nrhs;
      for (uint32_t c = lane; c < perRow; c += lanes) {
        S v = in[c];
        if (scale) v *= g;
        out[c] = v;
      }
    }
  }
}

int bfdevCovScalePermute(void *dst, void const *src, void const *scale, int power, uint64_t const *perm, uint64_t rows, uint32_t nrhs, uint32_t dtype, void *stream) {
  if (!rows || !nrhs) return 0;
  if (dtype != BFHIP_F64 && dtype != BFHIP_F32) return bfhipFail(BFABI_ERROR_TYPE_ERROR, "block scale/permute: real element types only");
  size_t const es = dtype == BFHIP_F64 ? 8 : 4;
  bool const vec = (nrhs * es) % 16 == 0 && (((uintptr_t)dst | (uintptr_t)src) & 15) == 0;
  uint32_t const lanes = covLanes(vec ? nrhs * es / 16 : nrhs, 256);
  uint32_t const lg = (uint32_t)__builtin_ctz(lanes);
  dim3 const grid(covGrid(rows, lanes)), block(256);
  hipStream_t const s = (hipStream_t)stream;
#define BF_COV_SP(S, VEC) hipLaunchKernelGGL((bfCovScalePermuteKernel<S, VEC>), grid, block, 0, s, (S *)dst, (S const *)src, (S const *)scale, power, perm, rows, nrhs, lg)
  if (dtype == BFHIP_F64) { if (vec) BF_COV_SP(double, true); else BF_COV_SP(double, false); }
  else { if (vec) BF_COV_SP(float, true); else BF_COV_SP(float, false); }
#undef BF_COV_SP
  return bfHipFail(hipGetLastError(), "block scale/permute launch");
}

// ---------------------------------------------------------------------------
// normals
// ---------------------------------------------------------------------------
// d[t] = N(seed, firstIdx + t): bfhip_normal_value in double, rounded once for float.  One element per thread and
// grid stride: the kernel is bound by log / cos, its stores are coalesced.
template <typename S>
__global__ __launch_bounds__(256) void bfNormalFillKernel(S *d, uint64_t count, uint64_t firstIdx, uint64_t seed) {
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < count; t += (uint64_t)gridDim.x * 256)
    d[t] = (S)bfhip_normal_value(seed, firstIdx + t);
}

// The input block of a draw, fused with the GammaLam scale: w[j, s] = S(N(seed, (firstSample + s) * cols + j)) * gamma[j]
// for s < nrhs -- sample-major indices (a sample's normals do not depend on the batch it is drawn in) written into the
// column-of-samples layout the apply takes.  The normal is rounded to S BEFORE the product, which is formed in S: the
// very bits bfCovScalePermuteKernel makes of a block filled by bfNormalFillKernel.  Threads as above: `lanes` per row j,
// gamma[j] read once per row and lane; consecutive lanes write consecutive elements.
template <typename S>
__global__ __launch_bounds__(256) void bfCovDrawFillKernel(S *w, S const *gamma, uint64_t cols, uint32_t nrhs, uint64_t seed, uint64_t firstSample, uint32_t lanesLog2) {
  uint32_t const lanes = 1u << lanesLog2, lane = threadIdx.x & (lanes - 1), rowsPerWg = 256u >> lanesLog2;
  for (uint64_t j = (uint64_t)blockIdx.x * rowsPerWg + (threadIdx.x >> lanesLog2); j < cols; j += (uint64_t)gridDim.x * rowsPerWg) {
    S const g = gamma ? gamma[j] : (S)1;
    S *out = w + j * nrhs;
    for (uint32_t s = lane; s < nrhs; s += lanes) {
      S v = (S)bfhip_normal_value(seed, (firstSample + s) * cols + j);
      if (gamma) v *= g;
      out[s] = v;
    }
  }
}

int bfdevFillNormal(void *d, uint64_t count, uint64_t firstIdx, uint32_t dtype, uint64_t seed, void *stream) {
  if (!count) return 0;
  uint64_t const need = (count + 255) / 256;
  dim3 const grid((uint32_t)(need < BF_COV_MAX_GRID ? need : BF_COV_MAX_GRID)), block(256);
  if (dtype == BFHIP_F64) hipLaunchKernelGGL(bfNormalFillKernel<double>, grid, block, 0, (hipStream_t)stream, (double *)d, count, firstIdx, seed);
  else if (dtype == BFHIP_F32) hipLaunchKernelGGL(bfNormalFillKernel<float>, grid, block, 0, (hipStream_t)stream, (float *)d, count, firstIdx, seed);
  else return bfhipFail(BFABI_ERROR_TYPE_ERROR, "normal fill: real element types only");
  return bfHipFail(hipGetLastError(), "normal fill launch");
}

int bfdevCovDrawFill(void *w, void const *gamma, uint64_t cols, uint32_t nrhs, uint32_t dtype, uint64_t seed, uint64_t firstSample, void *stream) {
  if (!cols || !nrhs) return 0;
  uint32_t const lanes = covLanes(nrhs, 64), lg = (uint32_t)__builtin_ctz(lanes);
  dim3 const grid(covGrid(cols, lanes)), block(256);
  if (dtype == BFHIP_F64) hipLaunchKernelGGL(bfCovDrawFillKernel<double>, grid, block, 0, (hipStream_t)stream, (double *)w, (double const *)gamma, cols, nrhs, seed, firstSample, lg);
  else if (dtype == BFHIP_F32) hipLaunchKernelGGL(bfCovDrawFillKernel<float>, grid, block, 0, (hipStream_t)stream, (float *)w, (float const *)gamma, cols, nrhs, seed, firstSample, lg);
  else return bfhipFail(BFABI_ERROR_TYPE_ERROR, "draw fill: real element types only");
  return bfHipFail(hipGetLastError(), "draw fill launch");
}

// ---------------------------------------------------------------------------
// streaming moments: sum[perm[i]] += sum_q T[i, q], sumSq[perm[i]] += sum_q T[i, q]^2 over the b columns of a batch
// ---------------------------------------------------------------------------
// A row of T is b * es contiguous bytes (256 at b = 64 in fp32, 512 in fp64).  One lane per row would have every lane of
// a wavefront on a line of its own; here 16 neighbouring lanes share a row (a wavefront covers 4 rows, a workgroup 16),
// each loading 16-byte pieces c = lane, lane + 16, ... of it (VEC), or single elements at the same stride when b * es is
// no multiple of 16 (partial batches of any width).  Everything is widened to double first (exact for float) and then:
//   1. a lane adds its values in increasing column order, the squares as fma(v, v, acc);
//   2. the 16 partial sums are combined by an xor butterfly at distances 8, 4, 2, 1 (__shfl_xor inside the 16 lanes;
//      every lane of a group ends with the same bits, since each step adds the same two numbers in either order);
//   3. lane 0 of the group, the one owner of output row perm[i], adds the total to what is there.
// The shape depends on b alone, never on the grid or on timing: no atomics, identical results from run to run.
// Rows past the end run the shuffles with zeros (the whole wavefront stays converged) and store nothing.
template <typename S, bool VEC>
__global__ __launch_bounds__(256) void bfCovMomentsKernel(S const *t, uint64_t rows, uint32_t b, uint64_t const *perm, double *sum, double *sumSq) {
  using V = typename CovVec<S>::V;
  constexpr uint32_t N = CovVec<S>::N;
  uint32_t const lane = threadIdx.x & 15;
  uint64_t const rounds = (rows + (uint64_t)gridDim.x * 16 - 1) / ((uint64_t)gridDim.x * 16);
  for (uint64_t r = 0; r < rounds; ++r) {
    uint64_t const i = (r * gridDim.x + blockIdx.x) * 16 + (threadIdx.x >> 4);
    double a1 = 0, a2 = 0;
    if (i < rows) {
      if (VEC) {
        V const *in = (V const *)(t + i * b);
        for (uint32_t c = lane; c < b / N; c += 16) {
          V const v = in[c];
          double const x0 = v.x, x1 = v.y;
          a1 += x0; a2 = fma(x0, x0, a2);
          a1 += x1; a2 = fma(x1, x1, a2);
          if constexpr (N == 4) {
            double const x2 = v.z, x3 = v.w;
            a1 += x2; a2 = fma(x2, x2, a2);
            a1 += x3; a2 = fma(x3, x3, a2);
          }
        }
      } else {
        S const *in = t + i * b;
        for (uint32_t c = lane; c < b; c += 16) {
          double const x = in[c];
          a1 += x; a2 = fma(x, x, a2);
        }
      }
    }
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) {
      a1 += __shfl_xor(a1, d, 16);
      a2 += __shfl_xor(a2, d, 16);
    }
    if (i < rows && lane == 0) {
      uint64_t const j = perm ? perm[i] : i;
      if (j < rows) {
        if (sum) sum[j] += a1;
        if (sumSq) sumSq[j] += a2;
      }
    }
  }
}

int bfdevCovMoments(void const *t, uint64_t rows, uint32_t b, uint32_t dtype, uint64_t const *perm, double *sum, double *sumSq, void *stream) {
  if (!rows || !b) return 0;
  if (dtype != BFHIP_F64 && dtype != BFHIP_F32) return bfhipFail(BFABI_ERROR_TYPE_ERROR, "moments: real element types only");
  size_t const es = dtype == BFHIP_F64 ? 8 : 4;
  bool const vec = (b * es) % 16 == 0 && ((uintptr_t)t & 15) == 0;
  dim3 const grid(covGrid(rows, 16)), block(256);
  hipStream_t const s = (hipStream_t)stream;
#define BF_COV_MOM(S, VEC) hipLaunchKernelGGL((bfCovMomentsKernel<S, VEC>), grid, block, 0, s, (S const *)t, rows, b, perm, sum, sumSq)
  if (dtype == BFHIP_F64) { if (vec) BF_COV_MOM(double, true); else BF_COV_MOM(double, false); }
  else { if (vec) BF_COV_MOM(float, true); else BF_COV_MOM(float, false); }
#undef BF_COV_MOM
  return bfHipFail(hipGetLastError(), "moments launch");
}
