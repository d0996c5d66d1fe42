// bfhip_precond.hip -- gfx950 kernels of the block-Jacobi preconditioner (bfhip_precond.c drives them).
//
// Three kernels, one workgroup of 256 threads per diagonal block (gather, inversion) or per piece of the result (fill).  None
// needs scratch, atomics or inline assembly; every block is private to its workgroup, so the only ordering is the workgroup
// barrier (a CU's vector L1 is shared by the waves of a workgroup: stores before __syncthreads() are seen after it).
//
//   * gather: the block's m x m row-major working copy (complex double, or double for the real family) is zeroed, then the
//     block's tasks -- sub-rectangles of the operator's direct pieces, identity runs, the 1s of uncovered rows -- are added
//     one after the other, a barrier between two tasks.  Inside a task every element is a distinct entry of the block, so the
//     sums are formed in the task order whatever the thread count: repeated builds are bit-identical.  Reads run along the
//     stored dimension of the piece (down a column of a column-major piece, along a row of a row-major one).
//   * inversion: Gauss-Jordan with partial pivoting in place on the working copy (DESIGN.md section 13 says why the copy stays
//     in global memory rather than in LDS).  Step k: the pivot is the largest |re| + |im| (|x| for real) of column k at or
//     below the diagonal, ties to the smaller row; rows k and p are swapped; the scaled pivot row goes to LDS (rowK, its
//     k-th entry 1/pivot) with the eliminated column (colF); then every entry is updated, A(i, j) = [j != k] A(i, j) - colF(i)
//     rowK(j) for i != k and A(k, j) = rowK(j).  At the end the columns are swapped back in reverse step order.  A zero or
//     non-finite pivot stops the block and is reported (status, step); so does a pivot whose reciprocal is not finite (a
//     subnormal pivot: 1 / 2^-1074 overflows) and a scaled pivot row with a non-finite entry.  The host refuses the build.
//   * fill: writes a piece of the result's arena (its plan's column-major mrPad x ncols or row-major mr x ld layout, padding
//     zero) from the working copy, rounding to the result's element type on the store.
//
// Indices come from the host; each is still compared with the extent it indexes and an out-of-range one is skipped (gather)
// or reads as zero (fill).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"

#define BF_BJ_THREADS 256
#define BF_BJ_MAX_M 256      // BFHIP_BJ_MAX_BLOCK: the inversion keeps one LDS entry per row / column of a block

// ---- element helpers: W = working type (double2 / double), S / O = stored types ----
__device__ __forceinline__ double2 bjWiden(double2 v) { return v; }
__device__ __forceinline__ double2 bjWiden(float2 v) { return make_double2((double)v.x, (double)v.y); }
__device__ __forceinline__ double bjWiden(double v) { return v; }
__device__ __forceinline__ double bjWiden(float v) { return (double)v; }

template <typename O> __device__ __forceinline__ O bjNarrow(double2 v);
template <> __device__ __forceinline__ double2 bjNarrow<double2>(double2 v) { return v; }
template <> __device__ __forceinline__ float2 bjNarrow<float2>(double2 v) { return make_float2((float)v.x, (float)v.y); }
template <typename O> __device__ __forceinline__ O bjNarrow(double v);
template <> __device__ __forceinline__ double bjNarrow<double>(double v) { return v; }
template <> __device__ __forceinline__ float bjNarrow<float>(double v) { return (float)v; }

__device__ __forceinline__ double2 bjAdd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double bjAdd(double a, double b) { return a + b; }
// a - f * r
__device__ __forceinline__ double2 bjSubMul(double2 a, double2 f, double2 r) {
  return make_double2(a.x - (f.x * r.x - f.y * r.y), a.y - (f.x * r.y + f.y * r.x));
}
__device__ __forceinline__ double bjSubMul(double a, double f, double r) { return a - f * r; }
__device__ __forceinline__ double2 bjMul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double bjMul(double a, double b) { return a * b; }
// 1 / v, scaled so that neither |v|^2 over- nor underflows on its own
__device__ __forceinline__ double2 bjRecip(double2 v) {
  double const s = fmax(fabs(v.x), fabs(v.y));
  double const a = v.x / s, b = v.y / s, d = a * a + b * b;
  return make_double2(a / d / s, -b / d / s);
}
__device__ __forceinline__ double bjRecip(double v) { return 1.0 / v; }
__device__ __forceinline__ double bjAbs1(double2 v) { return fabs(v.x) + fabs(v.y); }     // the pivot search's magnitude (LAPACK's cabs1)
__device__ __forceinline__ double bjAbs1(double v) { return fabs(v); }
__device__ __forceinline__ double bjAbs(double2 v) { return hypot(v.x, v.y); }
__device__ __forceinline__ double bjAbs(double v) { return fabs(v); }
__device__ __forceinline__ bool bjFinite(double2 v) { return fabs(v.x) <= 1.79769313486231570815e308 && fabs(v.y) <= 1.79769313486231570815e308; }
__device__ __forceinline__ bool bjFinite(double v) { return fabs(v) <= 1.79769313486231570815e308; }
template <typename W> __device__ __forceinline__ W bjZero();
template <> __device__ __forceinline__ double2 bjZero<double2>() { return make_double2(0.0, 0.0); }
template <> __device__ __forceinline__ double bjZero<double>() { return 0.0; }
template <typename W> __device__ __forceinline__ W bjOne();
template <> __device__ __forceinline__ double2 bjOne<double2>() { return make_double2(1.0, 0.0); }
template <> __device__ __forceinline__ double bjOne<double>() { return 1.0; }

// ---- gather ----
template <typename S, typename W>
__global__ __launch_bounds__(BF_BJ_THREADS) void bfBjGatherKernel(W *__restrict__ ws, S const *__restrict__ arena, uint64_t arenaElems,
                                                                  BfBjBlock const *__restrict__ blocks, BfBjTask const *__restrict__ tasks) {
  BfBjBlock const B = blocks[blockIdx.x];
  W *A = ws + B.wsOff;
  uint32_t const m = B.m, tid = threadIdx.x;
  for (uint32_t e = tid; e < m * m; e += BF_BJ_THREADS) A[e] = bjZero<W>();
  __syncthreads();
  for (uint32_t t = B.taskBegin; t < B.taskEnd; ++t) {
    BfBjTask const T = tasks[t];
    if (T.ldr == 0 && T.ldc == 0) {         // identity run: 1 at (br + r, bc + r)
      for (uint32_t r = tid; r < T.nr; r += BF_BJ_THREADS)
        if (T.br + r < m && T.bc + r < m) A[(T.br + r) * m + T.bc + r] = bjAdd(A[(T.br + r) * m + T.bc + r], bjOne<W>());
    } else {
      uint32_t const total = T.nr * T.nc;
      int const downCols = T.ldr == 1;      // column-major piece: consecutive threads walk down a column
      for (uint32_t e = tid; e < total; e += BF_BJ_THREADS) {
        uint32_t r, c;
        if (downCols) { c = e / T.nr; r = e - c * T.nr; }
        else { r = e / T.nc; c = e - r * T.nc; }
        uint64_t const src = T.dataOff + (uint64_t)r * T.ldr + (uint64_t)c * T.ldc;
        if (src < arenaElems && T.br + r < m && T.bc + c < m) {
          uint32_t const d = (T.br + r) * m + T.bc + c;
          A[d] = bjAdd(A[d], bjWiden(arena[src]));
        }
      }
    }
    __syncthreads();
  }
}

// ---- inversion ----
template <typename W>
__global__ __launch_bounds__(BF_BJ_THREADS) void bfBjInvertKernel(W *__restrict__ ws, BfBjBlock const *__restrict__ blocks, BfBjResult *__restrict__ res) {
  __shared__ W rowK[BF_BJ_MAX_M];
  __shared__ W colF[BF_BJ_MAX_M];
  __shared__ double key[BF_BJ_THREADS];
  __shared__ uint32_t kidx[BF_BJ_THREADS];
  __shared__ uint32_t perm[BF_BJ_MAX_M];
  __shared__ uint32_t rowBad;               // a scaled pivot row held a non-finite entry (set once, the block stops)
  BfBjBlock const B = blocks[blockIdx.x];
  W *A = ws + B.wsOff;
  uint32_t const m = B.m < BF_BJ_MAX_M ? B.m : BF_BJ_MAX_M, tid = threadIdx.x;
  // the update's thread layout: column j = tid % m, rows g, g + groups, ... (groups = 256 / m workgroup slices)
  uint32_t const groups = m ? BF_BJ_THREADS / m : 1, j = m ? tid % m : 0, g = m ? tid / m : 1;

  // the largest |B(i, j)| (a NaN or infinity counts as infinite)
  double mx = 0.0;
  for (uint32_t e = tid; e < m * m; e += BF_BJ_THREADS) {
    double const a = bjAbs(A[e]);
    mx = (a != a) ? INFINITY : fmax(mx, a);
  }
  key[tid] = mx;
  if (tid == 0) rowBad = 0;
  __syncthreads();
  for (uint32_t s = BF_BJ_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) key[tid] = fmax(key[tid], key[tid + s]);
    __syncthreads();
  }
  double const maxAbs = key[0];
  __syncthreads();

  double minPiv = INFINITY;
  uint32_t status = 0, stepBad = 0;
  for (uint32_t k = 0; k < m; ++k) {
    // pivot: the largest magnitude of column k at or below row k, ties to the smaller row
    double kv = -1.0;
    if (tid >= k && tid < m) {
      double const a = bjAbs1(A[tid * m + k]);
      kv = (a != a) ? INFINITY : a;
    }
    key[tid] = kv;
    kidx[tid] = tid;
    __syncthreads();
    for (uint32_t s = BF_BJ_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) {
        double const o = key[tid + s];
        uint32_t const oi = kidx[tid + s];
        if (o > key[tid] || (o == key[tid] && oi < kidx[tid])) { key[tid] = o; kidx[tid] = oi; }
      }
      __syncthreads();
    }
    uint32_t const p = kidx[0];
    W const piv = A[p * m + k];             // the same value in every thread: the break below is uniform
    double const pa = bjAbs(piv);
    W const inv = bjRecip(piv);
    // a zero or non-finite pivot, or a finite one whose reciprocal overflows (subnormal pivots)
    if (!(pa > 0.0) || !(pa <= 1.79769313486231570815e308) || !bjFinite(inv)) { status = 1; stepBad = k; break; }
    minPiv = fmin(minPiv, pa);
    __syncthreads();                        // every thread has read row p's entry and kidx[0] before they change
    if (p != k)
      for (uint32_t c = tid; c < m; c += BF_BJ_THREADS) { W const t = A[k * m + c]; A[k * m + c] = A[p * m + c]; A[p * m + c] = t; }
    if (tid == 0) perm[k] = p;
    __syncthreads();
    for (uint32_t c = tid; c < m; c += BF_BJ_THREADS) {
      W const rk = c == k ? inv : bjMul(A[k * m + c], inv);
      if (!bjFinite(rk)) rowBad = 1;        // every writer stores the same value
      rowK[c] = rk;
      colF[c] = c == k ? bjZero<W>() : A[c * m + k];
    }
    __syncthreads();
    if (rowBad) { status = 1; stepBad = k; break; }     // read after the barrier by every thread: uniform
    if (g < groups) {
      W const rk = rowK[j];
      for (uint32_t i = g; i < m; i += groups) {
        W *a = &A[i * m + j];
        if (i == k) *a = rk;
        else *a = bjSubMul(j == k ? bjZero<W>() : *a, colF[i], rk);
      }
    }
    __syncthreads();
  }
  if (!status) {
    // A now holds inv(P B) = inv(B) P^T: undo the row exchanges on the columns, last step first (each thread owns whole rows)
    for (uint32_t i = tid; i < m; i += BF_BJ_THREADS)
      for (uint32_t k = m; k-- > 0;) {
        uint32_t const p = perm[k];
        if (p != k) { W const t = A[i * m + k]; A[i * m + k] = A[i * m + p]; A[i * m + p] = t; }
      }
  }
  if (tid == 0) {
    BfBjResult r;
    r.minPivot = status ? 0.0 : (m ? minPiv : 0.0);
    r.maxAbs = maxAbs;
    r.status = status;
    r.step = stepBad;
    res[blockIdx.x] = r;
  }
}

// ---- fill ----
template <typename W, typename O>
__global__ __launch_bounds__(BF_BJ_THREADS) void bfBjFillKernel(O *__restrict__ arena, W const *__restrict__ ws, BfBjFillPiece const *__restrict__ pieces) {
  BfBjFillPiece const P = pieces[blockIdx.x];
  W const *A = ws + P.wsOff;
  uint32_t const m = P.m;
  if (P.rowMajor) {
    uint32_t const total = P.mr * P.ld;
    for (uint32_t e = threadIdx.x; e < total; e += BF_BJ_THREADS) {
      uint32_t const r = e / P.ld, c = e - r * P.ld;
      uint32_t const i = P.row0 + r, jj = P.col0 + c;
      W const v = (c < P.ncols && i < m && jj < m) ? A[i * m + jj] : bjZero<W>();
      arena[P.dataOff + e] = bjNarrow<O>(v);
    }
  } else {
    uint32_t const total = P.mrPad * P.ncols;
    for (uint32_t e = threadIdx.x; e < total; e += BF_BJ_THREADS) {
      uint32_t const c = e / P.mrPad, r = e - c * P.mrPad;
      uint32_t const i = P.row0 + r, jj = P.col0 + c;
      W const v = (r < P.mr && i < m && jj < m) ? A[i * m + jj] : bjZero<W>();
      arena[P.dataOff + e] = bjNarrow<O>(v);
    }
  }
}

extern "C" {

int bfdevBjGather(void *ws, void const *arena, uint64_t arenaElems, uint32_t srcDtype, BfBjBlock const *dBlocks, BfBjTask const *dTasks,
                  uint64_t numBlocks, void *stream) {
  if (!numBlocks) return 0;
  if (numBlocks > 0x7fffffffull) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "too many diagonal blocks");
  hipStream_t const s = (hipStream_t)stream;
  dim3 const grid((uint32_t)numBlocks), block(BF_BJ_THREADS);
  switch (srcDtype) {
    case BFHIP_C128: hipLaunchKernelGGL((bfBjGatherKernel<double2, double2>), grid, block, 0, s, (double2 *)ws, (double2 const *)arena, arenaElems, dBlocks, dTasks); break;
    case BFHIP_C64: hipLaunchKernelGGL((bfBjGatherKernel<float2, double2>), grid, block, 0, s, (double2 *)ws, (float2 const *)arena, arenaElems, dBlocks, dTasks); break;
    case BFHIP_F64: hipLaunchKernelGGL((bfBjGatherKernel<double, double>), grid, block, 0, s, (double *)ws, (double const *)arena, arenaElems, dBlocks, dTasks); break;
    case BFHIP_F32: hipLaunchKernelGGL((bfBjGatherKernel<float, double>), grid, block, 0, s, (double *)ws, (float const *)arena, arenaElems, dBlocks, dTasks); break;
    default: return bfhipFail(BFABI_ERROR_TYPE_ERROR, "block-Jacobi gather: unknown dtype %u", srcDtype);
  }
  return bfHipFail(hipGetLastError(), "block-Jacobi gather launch");
}

int bfdevBjInvert(void *ws, int cplx, BfBjBlock const *dBlocks, BfBjResult *dResults, uint64_t numBlocks, void *stream) {
  if (!numBlocks) return 0;
  if (numBlocks > 0x7fffffffull) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "too many diagonal blocks");
  hipStream_t const s = (hipStream_t)stream;
  dim3 const grid((uint32_t)numBlocks), block(BF_BJ_THREADS);
  if (cplx) hipLaunchKernelGGL((bfBjInvertKernel<double2>), grid, block, 0, s, (double2 *)ws, dBlocks, dResults);
  else hipLaunchKernelGGL((bfBjInvertKernel<double>), grid, block, 0, s, (double *)ws, dBlocks, dResults);
  return bfHipFail(hipGetLastError(), "block-Jacobi inversion launch");
}

int bfdevBjFill(void *arena, uint32_t outDtype, void const *ws, BfBjFillPiece const *dPieces, uint64_t numPieces, void *stream) {
  if (!numPieces) return 0;
  if (numPieces > 0x7fffffffull) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "too many result pieces");
  hipStream_t const s = (hipStream_t)stream;
  dim3 const grid((uint32_t)numPieces), block(BF_BJ_THREADS);
  switch (outDtype) {
    case BFHIP_C128: hipLaunchKernelGGL((bfBjFillKernel<double2, double2>), grid, block, 0, s, (double2 *)arena, (double2 const *)ws, dPieces); break;
    case BFHIP_C64: hipLaunchKernelGGL((bfBjFillKernel<double2, float2>), grid, block, 0, s, (float2 *)arena, (double2 const *)ws, dPieces); break;
    case BFHIP_F64: hipLaunchKernelGGL((bfBjFillKernel<double, double>), grid, block, 0, s, (double *)arena, (double const *)ws, dPieces); break;
    case BFHIP_F32: hipLaunchKernelGGL((bfBjFillKernel<double, float>), grid, block, 0, s, (float *)arena, (double const *)ws, dPieces); break;
    default: return bfhipFail(BFABI_ERROR_TYPE_ERROR, "block-Jacobi fill: unknown dtype %u", outDtype);
  }
  return bfHipFail(hipGetLastError(), "block-Jacobi fill launch");
}

}  // extern "C"
