// bfhip_extract.hip -- gfx950 kernels of the dense extraction A[I, J] (bfhip_extract.c drives them) and the stream helpers the
// host entry overlaps its copies with.
//
// An extraction applies the operator to panels of <= 64 unit vectors (the 64-RHS matrix-core kernel's width) and gathers the
// wanted rows of each result panel.  Three kernels, none of them needs scratch, atomics or inline assembly:
//
//   * unit panel: the input panel (ext x p, ld = p) is zeroed once per call; per panel ONE workgroup clears the previous
//     panel's p ones and then sets X[idx[k], k] = 1 -- O(p) work instead of an ext x p memset.  The two phases are
//     separated by a workgroup barrier, so a one that stays where it was (same index, same column) is cleared and set again
//     in that order, and a ragged last panel (a narrower ld) starts from an all-zero buffer.
//   * forward gather: Out[i * ldOut + k] = Y[rows[i] * p + k]; threads over (i, k) with k fastest, so reads of a panel row and
//     writes of an output row are contiguous.  Moves bits only: one instantiation per element size (16, 8, 4 bytes).
//   * transposed gather (the adjoint route): Out[k * ldOut + j] = P[cols[j] * p + k].  A tile of TJ output columns x p panel
//     columns goes through LDS: it is read with k fastest (contiguous rows of P) and written with j fastest (contiguous rows
//     of Out).  The tile's rows are padded by one element, so a column walk (fixed k, varying j) steps the 64 x 4 B banks by
//     p + 1 elements instead of landing on one bank (MI355X_MICROARCH.md, LDS).
//
// Every index the kernels read was checked on the host (bfhip_extract.c); each is still compared with the extent it indexes,
// and an out-of-range one is skipped (unit panel) or reads as zero (gathers), so no access leaves its buffer.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"

#define BF_EX_THREADS 256
#define BF_EX_GATHER_BLOCKS_MAX 65535u

// value of index k of an index list: idx[base + k], or base + k for the identity (idx == NULL)
__device__ __forceinline__ uint64_t bfExIndex(uint64_t const *idx, uint64_t base, uint64_t k) { return idx ? idx[base + k] : base + k; }

template <typename E> struct BfExOne;
template <> struct BfExOne<double2> { __device__ static double2 one() { return make_double2(1.0, 0.0); } __device__ static double2 zero() { return make_double2(0.0, 0.0); } };
template <> struct BfExOne<float2> { __device__ static float2 one() { return make_float2(1.0f, 0.0f); } __device__ static float2 zero() { return make_float2(0.0f, 0.0f); } };
template <> struct BfExOne<double> { __device__ static double one() { return 1.0; } __device__ static double zero() { return 0.0; } };
template <> struct BfExOne<float> { __device__ static float one() { return 1.0f; } __device__ static float zero() { return 0.0f; } };

// one workgroup of 64 threads: clear the previous panel's ones (prevCount of them, ld prevLd), then set the new ones
template <typename E>
__global__ __launch_bounds__(64) void bfExtractUnitKernel(E *X, uint64_t ext, uint64_t const *prevIdx, uint64_t prevBase, uint32_t prevCount,
                                                          uint32_t prevLd, uint64_t const *idx, uint64_t base, uint32_t count, uint32_t ld) {
  uint32_t const k = threadIdx.x;
  if (k < prevCount) {
    uint64_t const r = bfExIndex(prevIdx, prevBase, k);
    if (r < ext) X[r * prevLd + k] = BfExOne<E>::zero();
  }
  __syncthreads();
  if (k < count) {
    uint64_t const r = bfExIndex(idx, base, k);
    if (r < ext) X[r * ld + k] = BfExOne<E>::one();
  }
}

// Out[i * ldOut + k] = Y[rows[rowBase + i] * p + k] for i < numRows, k < p (grid-stride over numRows * p)
template <typename T>
__global__ __launch_bounds__(BF_EX_THREADS) void bfExtractGatherKernel(T *__restrict__ Out, uint64_t ldOut, T const *__restrict__ Y, uint64_t ext,
                                                                       uint32_t p, uint64_t const *__restrict__ rows, uint64_t rowBase, uint64_t numRows) {
  uint64_t const total = numRows * p;
  for (uint64_t e = (uint64_t)blockIdx.x * BF_EX_THREADS + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BF_EX_THREADS) {
    uint64_t const i = e / p, k = e - i * p;
    uint64_t const r = bfExIndex(rows, rowBase, i);
    T v;
    if (r < ext) v = Y[r * p + k];
    else v = T{};
    Out[i * ldOut + k] = v;
  }
}

// Out[k * ldOut + j] = P[cols[colBase + j] * p + k] for k < p, j < numCols; one workgroup per tile of TJ columns j, through LDS
template <typename T, uint32_t TJ>
__global__ __launch_bounds__(BF_EX_THREADS) void bfExtractGatherTKernel(T *__restrict__ Out, uint64_t ldOut, T const *__restrict__ P, uint64_t ext,
                                                                        uint32_t p, uint64_t const *__restrict__ cols, uint64_t colBase, uint64_t numCols) {
  __shared__ T tile[TJ][64 + 1];
  for (uint64_t j0 = (uint64_t)blockIdx.x * TJ; j0 < numCols; j0 += (uint64_t)gridDim.x * TJ) {
    uint32_t const tj = numCols - j0 < TJ ? (uint32_t)(numCols - j0) : TJ;
    for (uint32_t e = threadIdx.x; e < tj * p; e += BF_EX_THREADS) {          // k fastest: a contiguous row of P per j
      uint32_t const j = e / p, k = e - j * p;
      uint64_t const c = bfExIndex(cols, colBase, j0 + j);
      T v;
      if (c < ext) v = P[c * p + k];
      else v = T{};
      tile[j][k] = v;
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < tj * p; e += BF_EX_THREADS) {          // j fastest: a contiguous row of Out per k
      uint32_t const k = e / tj, j = e - k * tj;
      Out[(uint64_t)k * ldOut + j0 + j] = tile[j][k];
    }
    __syncthreads();
  }
}

static dim3 bfExGrid(uint64_t work, uint64_t per) {
  uint64_t b = (work + per - 1) / per;
  if (b > BF_EX_GATHER_BLOCKS_MAX) b = BF_EX_GATHER_BLOCKS_MAX;
  return dim3((uint32_t)(b ? b : 1));
}

extern "C" {

int bfdevExtractUnit(void *X, uint32_t dtype, uint64_t ext, uint64_t const *prevIdx, uint64_t prevBase, uint32_t prevCount, uint32_t prevLd,
                     uint64_t const *idx, uint64_t base, uint32_t count, uint32_t ld, void *stream) {
  if (prevCount > 64 || count > 64) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "unit panel wider than 64 columns");
  if (!prevCount && !count) return 0;
  hipStream_t const s = (hipStream_t)stream;
  switch (dtype) {
    case BFHIP_C128: hipLaunchKernelGGL(bfExtractUnitKernel<double2>, dim3(1), dim3(64), 0, s, (double2 *)X, ext, prevIdx, prevBase, prevCount, prevLd, idx, base, count, ld); break;
    case BFHIP_C64: hipLaunchKernelGGL(bfExtractUnitKernel<float2>, dim3(1), dim3(64), 0, s, (float2 *)X, ext, prevIdx, prevBase, prevCount, prevLd, idx, base, count, ld); break;
    case BFHIP_F64: hipLaunchKernelGGL(bfExtractUnitKernel<double>, dim3(1), dim3(64), 0, s, (double *)X, ext, prevIdx, prevBase, prevCount, prevLd, idx, base, count, ld); break;
    case BFHIP_F32: hipLaunchKernelGGL(bfExtractUnitKernel<float>, dim3(1), dim3(64), 0, s, (float *)X, ext, prevIdx, prevBase, prevCount, prevLd, idx, base, count, ld); break;
    default: return bfhipFail(BFABI_ERROR_TYPE_ERROR, "unit panel: unknown dtype %u", dtype);
  }
  return bfHipFail(hipGetLastError(), "extract unit-panel launch");
}

int bfdevExtractGather(void *Out, uint64_t ldOut, void const *Y, uint64_t ext, uint32_t p, uint64_t const *rows, uint64_t rowBase, uint64_t numRows,
                       uint32_t elemSize, void *stream) {
  if (!numRows || !p) return 0;
  hipStream_t const s = (hipStream_t)stream;
  dim3 const g = bfExGrid(numRows * p, BF_EX_THREADS);
  switch (elemSize) {
    case 16: hipLaunchKernelGGL(bfExtractGatherKernel<double2>, g, dim3(BF_EX_THREADS), 0, s, (double2 *)Out, ldOut, (double2 const *)Y, ext, p, rows, rowBase, numRows); break;
    case 8: hipLaunchKernelGGL(bfExtractGatherKernel<uint64_t>, g, dim3(BF_EX_THREADS), 0, s, (uint64_t *)Out, ldOut, (uint64_t const *)Y, ext, p, rows, rowBase, numRows); break;
    case 4: hipLaunchKernelGGL(bfExtractGatherKernel<uint32_t>, g, dim3(BF_EX_THREADS), 0, s, (uint32_t *)Out, ldOut, (uint32_t const *)Y, ext, p, rows, rowBase, numRows); break;
    default: return bfhipFail(BFABI_ERROR_TYPE_ERROR, "gather: element size %u", elemSize);
  }
  return bfHipFail(hipGetLastError(), "extract gather launch");
}

int bfdevExtractGatherT(void *Out, uint64_t ldOut, void const *P, uint64_t ext, uint32_t p, uint64_t const *cols, uint64_t colBase, uint64_t numCols,
                        uint32_t elemSize, void *stream) {
  if (!numCols || !p) return 0;
  if (p > 64) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "transposed gather: panel wider than 64 columns");
  hipStream_t const s = (hipStream_t)stream;
  switch (elemSize) {      // tiles of 32 (16-byte elements, 33 KiB of LDS) or 64 columns (<= 33 KiB)
    case 16: hipLaunchKernelGGL((bfExtractGatherTKernel<double2, 32>), bfExGrid(numCols, 32), dim3(BF_EX_THREADS), 0, s, (double2 *)Out, ldOut, (double2 const *)P, ext, p, cols, colBase, numCols); break;
    case 8: hipLaunchKernelGGL((bfExtractGatherTKernel<uint64_t, 64>), bfExGrid(numCols, 64), dim3(BF_EX_THREADS), 0, s, (uint64_t *)Out, ldOut, (uint64_t const *)P, ext, p, cols, colBase, numCols); break;
    case 4: hipLaunchKernelGGL((bfExtractGatherTKernel<uint32_t, 64>), bfExGrid(numCols, 64), dim3(BF_EX_THREADS), 0, s, (uint32_t *)Out, ldOut, (uint32_t const *)P, ext, p, cols, colBase, numCols); break;
    default: return bfhipFail(BFABI_ERROR_TYPE_ERROR, "transposed gather: element size %u", elemSize);
  }
  return bfHipFail(hipGetLastError(), "extract transposed-gather launch");
}

// a stream that does not synchronise with the legacy default stream (the host entry's copies overlap the applies on it)
int bfdevStreamCreateNonBlocking(void **stream) { return bfHipFail(hipStreamCreateWithFlags((hipStream_t *)stream, hipStreamNonBlocking), "hipStreamCreateWithFlags"); }
void bfdevStreamDestroy(void *stream) { if (stream) (void)hipStreamDestroy((hipStream_t)stream); }
int bfdevStreamWaitEvent(void *stream, void *ev) { return bfHipFail(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)ev, 0), "hipStreamWaitEvent"); }
// rows of `width` bytes from src (pitch spitch) to dst (pitch dpitch); any memory kinds
int bfdevMemcpy2DAsync(void *dst, size_t dpitch, void const *src, size_t spitch, size_t width, size_t height, void *stream) {
  if (!width || !height) return 0;
  return bfHipFail(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDefault, (hipStream_t)stream), "hipMemcpy2DAsync");
}

}  // extern "C"
