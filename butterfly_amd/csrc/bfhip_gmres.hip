// bfhip_gmres.hip -- gfx950 kernels of the device-resident solvers: the GMRES building blocks (bfhip_gmres.c drives them)
// and the demote / promote / scale / update kernels of the mixed-precision refinement (bfhip_refine.c).  Streaming kernels
// over n x nrhs row-major vectors; none is a stage kernel and none shares a helper with bfhip_device.hip.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"

// ---------------------------------------------------------------------------
// device-resident GMRES building blocks (reference caller of the apply path:
// bfSolveGMRES, src/linalg.c:47-317: residual :127-131, column norms :139,
// modified Gram-Schmidt :174-184, normalisation :197-198, solution :245-285)
// ---------------------------------------------------------------------------
#define BF_GM_THREADS 256

__device__ __forceinline__ double2 bfBlockReduce2(double2 v, double2 *sh) {
  // fixed-order tree over the 256 threads of the block
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = BF_GM_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { sh[threadIdx.x].x += sh[threadIdx.x + s].x; sh[threadIdx.x].y += sh[threadIdx.x + s].y; }
    __syncthreads();
  }
  double2 r = sh[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ void bfRowRange(uint64_t n, uint32_t nb, uint64_t &r0, uint64_t &r1) {
  uint64_t per = (n + nb - 1) / nb;
  r0 = (uint64_t)blockIdx.x * per;
  r1 = r0 + per < n ? r0 + per : n;
  if (r0 > n) r0 = n;
}

// fixed-order tree over the 256 threads: .x summed, .y the maximum
__device__ __forceinline__ double2 bfBlockReduceSumMax(double2 v, double2 *sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = BF_GM_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { sh[threadIdx.x].x += sh[threadIdx.x + s].x; sh[threadIdx.x].y = fmax(sh[threadIdx.x].y, sh[threadIdx.x + s].y); }
    __syncthreads();
  }
  double2 r = sh[0];
  __syncthreads();
  return r;
}

// W = B - AX0 (AX0 may be null); partialOut[q*nb + bx] = (sum |W|^2, largest |component| of W) over the block's rows
__global__ __launch_bounds__(BF_GM_THREADS) void bfGmresResidualKernel(double2 const *B, double2 const *AX0, double2 *W,
                                                                      double2 *partialOut, uint64_t n, uint32_t nrhs, uint32_t nb) {
  __shared__ double2 sh[BF_GM_THREADS];
  uint32_t const q = blockIdx.y;
  uint64_t r0, r1;
  bfRowRange(n, nb, r0, r1);
  double acc = 0.0, big = 0.0;
  for (uint64_t r = r0 + threadIdx.x; r < r1; r += BF_GM_THREADS) {
    double2 v = B[r * nrhs + q];
    if (AX0) { double2 y = AX0[r * nrhs + q]; v.x -= y.x; v.y -= y.y; }
    W[r * nrhs + q] = v;
    acc += v.x * v.x + v.y * v.y;
    big = fmax(big, fmax(fabs(v.x), fabs(v.y)));
  }
  double2 t = bfBlockReduceSumMax(make_double2(acc, big), sh);
  if (threadIdx.x == 0) partialOut[(uint64_t)q * nb + blockIdx.x] = t;
}

// Per column q: e = the binary exponent of the largest |component| (the .y of bfGmresResidualKernel's partials; 0 for a zero or
// non-finite column); W *= 2^-e exactly (ldexp), so that the largest component lies in [1/2, 1) and the sum of squares can
// neither underflow nor overflow; expOut[q] = e; partialOut = per-block |W|^2 of the scaled column.
__global__ __launch_bounds__(BF_GM_THREADS) void bfGmresScaleKernel(double2 *W, double2 const *partialIn, double *expOut, double2 *partialOut,
                                                                   uint64_t n, uint32_t nrhs, uint32_t nb) {
  __shared__ double2 sh[BF_GM_THREADS];
  uint32_t const q = blockIdx.y;
  double big = 0.0;
  for (uint32_t b = threadIdx.x; b < nb; b += BF_GM_THREADS) big = fmax(big, partialIn[(uint64_t)q * nb + b].y);
  big = bfBlockReduceSumMax(make_double2(0.0, big), sh).y;
  int e = 0;
  if (big > 0.0 && isfinite(big)) frexp(big, &e);
  if (blockIdx.x == 0 && threadIdx.x == 0) expOut[q] = (double)e;
  uint64_t r0, r1;
  bfRowRange(n, nb, r0, r1);
  double acc = 0.0;
  for (uint64_t r = r0 + threadIdx.x; r < r1; r += BF_GM_THREADS) {
    double2 v = W[r * nrhs + q];
    v = make_double2(ldexp(v.x, -e), ldexp(v.y, -e));
    W[r * nrhs + q] = v;
    acc += v.x * v.x + v.y * v.y;
  }
  double2 t = bfBlockReduce2(make_double2(acc, 0.0), sh);
  if (threadIdx.x == 0) partialOut[(uint64_t)q * nb + blockIdx.x] = t;
}

__global__ __launch_bounds__(BF_GM_THREADS) void bfGmresDotKernel(double2 const *Vi, double2 const *W, double2 *partialOut,
                                                                 uint64_t n, uint32_t nrhs, uint32_t nb) {
  __shared__ double2 sh[BF_GM_THREADS];
  uint32_t const q = blockIdx.y;
  uint64_t r0, r1;
  bfRowRange(n, nb, r0, r1);
  double ar = 0.0, ai = 0.0;
  for (uint64_t r = r0 + threadIdx.x; r < r1; r += BF_GM_THREADS) {
    double2 v = Vi[r * nrhs + q], w = W[r * nrhs + q];
    ar += v.x * w.x + v.y * w.y;      // conj(v) * w
    ai += v.x * w.y - v.y * w.x;
  }
  double2 t = bfBlockReduce2(make_double2(ar, ai), sh);
  if (threadIdx.x == 0) partialOut[(uint64_t)q * nb + blockIdx.x] = t;
}

__device__ __forceinline__ double2 bfSumPartials(double2 const *partial, uint32_t q, uint32_t nb, double2 *sh) {
  double2 a = make_double2(0.0, 0.0);
  for (uint32_t b = threadIdx.x; b < nb; b += BF_GM_THREADS) { double2 v = partial[(uint64_t)q * nb + b]; a.x += v.x; a.y += v.y; }
  return bfBlockReduce2(a, sh);
}

__global__ __launch_bounds__(BF_GM_THREADS) void bfGmresMgsKernel(double2 const *Vi, double2 const *Vnext, double2 *W,
                                                                 double2 const *partialIn, double2 *partialOut, double2 *hOut,
                                                                 uint64_t n, uint32_t nrhs, uint32_t nb) {
  __shared__ double2 sh[BF_GM_THREADS];
  uint32_t const q = blockIdx.y;
  double2 const h = bfSumPartials(partialIn, q, nb, sh);
  if (blockIdx.x == 0 && threadIdx.x == 0) hOut[q] = h;
  uint64_t r0, r1;
  bfRowRange(n, nb, r0, r1);
  double ar = 0.0, ai = 0.0;
  for (uint64_t r = r0 + threadIdx.x; r < r1; r += BF_GM_THREADS) {
    double2 v = Vi[r * nrhs + q], w = W[r * nrhs + q];
    w.x -= h.x * v.x - h.y * v.y;
    w.y -= h.x * v.y + h.y * v.x;
    W[r * nrhs + q] = w;
    if (Vnext) {
      double2 u = Vnext[r * nrhs + q];
      ar += u.x * w.x + u.y * w.y;
      ai += u.x * w.y - u.y * w.x;
    } else {
      ar += w.x * w.x + w.y * w.y;
    }
  }
  double2 t = bfBlockReduce2(make_double2(ar, ai), sh);
  if (threadIdx.x == 0) partialOut[(uint64_t)q * nb + blockIdx.x] = t;
}

__global__ __launch_bounds__(BF_GM_THREADS) void bfGmresFinishKernel(double2 const *W, double2 const *partialIn, double2 *Vout,
                                                                    double2 *hOut, uint64_t n, uint32_t nrhs, uint32_t nb) {
  __shared__ double2 sh[BF_GM_THREADS];
  uint32_t const q = blockIdx.y;
  double2 const s = bfSumPartials(partialIn, q, nb, sh);
  double const nrm = sqrt(s.x);
  if (blockIdx.x == 0 && threadIdx.x == 0) hOut[q] = make_double2(nrm, 0.0);
  // a zero column (zero residual, or an exhausted Krylov space) gives V = 0, not 0/0: the host stops that column there
  bool const live = nrm > 0.0;
  uint64_t r0, r1;
  bfRowRange(n, nb, r0, r1);
  for (uint64_t r = r0 + threadIdx.x; r < r1; r += BF_GM_THREADS) {
    double2 w = W[r * nrhs + q];
    Vout[r * nrhs + q] = live ? make_double2(w.x / nrm, w.y / nrm) : make_double2(0.0, 0.0);
  }
}

__global__ __launch_bounds__(BF_GM_THREADS) void bfGmresUpdateKernel(double2 const *X0, double2 const *V, double2 const *y, uint32_t j,
                                                                    double2 *X, uint64_t n, uint32_t nrhs) {
  uint64_t e = (uint64_t)blockIdx.x * BF_GM_THREADS + threadIdx.x;
  uint64_t total = n * nrhs;
  if (e >= total) return;
  uint32_t q = (uint32_t)(e % nrhs);
  double2 x = X0 ? X0[e] : make_double2(0.0, 0.0);
  for (uint32_t i = 0; i < j; ++i) {
    double2 v = V[(uint64_t)i * total + e], c = y[(uint64_t)i * nrhs + q];
    if (c.x == 0.0 && c.y == 0.0) continue;      // a column that stopped early: x0 is kept bit for bit
    x.x += v.x * c.x - v.y * c.y;
    x.y += v.x * c.y + v.y * c.x;
  }
  X[e] = x;
}

// ---- batched Gram-Schmidt (CGS2): all projections of an iteration in one launch --------------------
// The reference orthogonalises W against V_0..V_j one vector at a time (modified Gram-Schmidt,
// src/linalg.c:174-184): j + 1 dependent BLAS-1 passes, each a few microseconds of work behind a launch.
// Here one pass is three launches whatever j is -- all dots h_i = V_i^H W (W read once per group of 8
// basis vectors), their reduction over row blocks, and W -= sum_i h_i V_i -- and the pass is run twice
// (classical Gram-Schmidt with reorthogonalisation, as stable as MGS); H[:, j] = h(pass 1) + h(pass 2).
#define BF_GM_GROUP 8

__device__ __forceinline__ double bfWaveSum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);      // fixed butterfly: deterministic
  return v;
}

// partial[((q * numVec + i) * nb) + bx] = sum over the block's rows of conj(V_i) * W   (i in this group of 8)
__global__ __launch_bounds__(BF_GM_THREADS) void bfGmresDotsKernel(double2 const *V, double2 const *W, double2 *partial, uint64_t n,
                                                                  uint32_t nrhs, uint32_t nb, uint32_t numVec) {
  __shared__ double2 sh[BF_GM_THREADS / 64][BF_GM_GROUP];
  uint32_t const q = blockIdx.y, i0 = blockIdx.z * BF_GM_GROUP;
  uint32_t const cnt = numVec - i0 < BF_GM_GROUP ? numVec - i0 : BF_GM_GROUP;
  uint64_t const vecLen = n * nrhs;
  uint64_t r0, r1;
  bfRowRange(n, nb, r0, r1);
  double ar[BF_GM_GROUP], ai[BF_GM_GROUP];
#pragma unroll
  for (int k = 0; k < BF_GM_GROUP; ++k) ar[k] = ai[k] = 0.0;
  for (uint64_t r = r0 + threadIdx.x; r < r1; r += BF_GM_THREADS) {
    double2 const w = W[r * nrhs + q];
#pragma unroll
    for (int k = 0; k < BF_GM_GROUP; ++k)
      if ((uint32_t)k < cnt) {
        double2 const v = V[(uint64_t)(i0 + k) * vecLen + r * nrhs + q];
        ar[k] += v.x * w.x + v.y * w.y;
        ai[k] += v.x * w.y - v.y * w.x;
      }
  }
  int const wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < BF_GM_GROUP; ++k) {
    double const sr = bfWaveSum(ar[k]), si = bfWaveSum(ai[k]);
    if (lane == 0) sh[wave][k] = make_double2(sr, si);
  }
  __syncthreads();
  if (threadIdx.x < cnt) {
    double2 t = sh[0][threadIdx.x];
    for (int w2 = 1; w2 < BF_GM_THREADS / 64; ++w2) { t.x += sh[w2][threadIdx.x].x; t.y += sh[w2][threadIdx.x].y; }
    partial[((uint64_t)q * numVec + i0 + threadIdx.x) * nb + blockIdx.x] = t;
  }
}

// h[i * nrhs + q] = sum_b partial; hSum[i * nrhs + q] = h + (hPrev ? hPrev[i * nrhs + q] : 0)
__global__ __launch_bounds__(BF_GM_THREADS) void bfGmresDotsFinishKernel(double2 const *partial, double2 const *hPrev, double2 *h, double2 *hSum,
                                                                        uint32_t nrhs, uint32_t nb, uint32_t numVec) {
  __shared__ double2 sh[BF_GM_THREADS];
  uint32_t const i = blockIdx.x, q = blockIdx.y;
  double2 a = make_double2(0.0, 0.0);
  for (uint32_t b = threadIdx.x; b < nb; b += BF_GM_THREADS) { double2 v = partial[((uint64_t)q * numVec + i) * nb + b]; a.x += v.x; a.y += v.y; }
  double2 const t = bfBlockReduce2(a, sh);
  if (threadIdx.x == 0) {
    h[(uint64_t)i * nrhs + q] = t;
    if (hSum) { double2 p = hPrev ? hPrev[(uint64_t)i * nrhs + q] : make_double2(0.0, 0.0); hSum[(uint64_t)i * nrhs + q] = make_double2(t.x + p.x, t.y + p.y); }
  }
}

// W -= sum_i h_i V_i; partialOut (optional) = per-block sum |W|^2 of the result
__global__ __launch_bounds__(BF_GM_THREADS) void bfGmresProjectKernel(double2 const *V, double2 *W, double2 const *h, double2 *partialOut, uint64_t n,
                                                                     uint32_t nrhs, uint32_t nb, uint32_t numVec) {
  __shared__ double2 sh[BF_GM_THREADS];
  uint32_t const q = blockIdx.y;
  uint64_t const vecLen = n * nrhs;
  uint64_t r0, r1;
  bfRowRange(n, nb, r0, r1);
  double acc = 0.0;
  for (uint64_t r = r0 + threadIdx.x; r < r1; r += BF_GM_THREADS) {
    double2 w = W[r * nrhs + q];
    for (uint32_t i = 0; i < numVec; ++i) {
      double2 const v = V[(uint64_t)i * vecLen + r * nrhs + q], c = h[(uint64_t)i * nrhs + q];   // h: uniform, cached
      w.x -= c.x * v.x - c.y * v.y;
      w.y -= c.x * v.y + c.y * v.x;
    }
    W[r * nrhs + q] = w;
    acc += w.x * w.x + w.y * w.y;
  }
  if (partialOut) {
    double2 const t = bfBlockReduce2(make_double2(acc, 0.0), sh);
    if (threadIdx.x == 0) partialOut[(uint64_t)q * nb + blockIdx.x] = t;
  }
}

// ---- mixed-precision GMRES refinement (bfhip_refine.c): the complex64 inner operator sits between a demote and a promote of
// the complex128 Krylov vectors; the outer loop scales each residual column to norm 1 and adds the scaled correction.  Streaming
// kernels, one complex element per thread, bounds-checked against count = n * nrhs.
__global__ __launch_bounds__(BF_GM_THREADS) void bfRefineDemoteKernel(double2 const *src, float2 *dst, uint64_t count) {
  uint64_t const e = (uint64_t)blockIdx.x * BF_GM_THREADS + threadIdx.x;
  if (e >= count) return;
  double2 const v = src[e];
  dst[e] = make_float2((float)v.x, (float)v.y);      // round to nearest, each component
}

__global__ __launch_bounds__(BF_GM_THREADS) void bfRefinePromoteKernel(float2 const *src, double2 *dst, uint64_t count) {
  uint64_t const e = (uint64_t)blockIdx.x * BF_GM_THREADS + threadIdx.x;
  if (e >= count) return;
  float2 const v = src[e];
  dst[e] = make_double2((double)v.x, (double)v.y);
}

// R and partialIn are bfGmresScaleKernel's: the residual column scaled by 2^-e (e = expIn[q]) and the per-block |R|^2 of the scaled
// column, which neither underflow nor overflow.  Per column q: nrm = sqrt(sum of the partials); scale[q] = 2^e nrm, the norm of
// the unscaled column (as computed: the host reads it); Rhat = R / nrm, or the unit vector 1/sqrt(n) where nrm is not positive
// (a zero column must not become 0/0).  Where the unscaled squares would not have left the range, 2^e nrm and Rhat are what the
// unscaled column gives, bit for bit: the power of two commutes with every rounding on the way.
__global__ __launch_bounds__(BF_GM_THREADS) void bfRefineScaleKernel(double2 const *R, double2 const *partialIn, double const *expIn, double2 *Rhat,
                                                                    double *scale, uint64_t n, uint32_t nrhs, uint32_t nb) {
  __shared__ double2 sh[BF_GM_THREADS];
  uint32_t const q = blockIdx.y;
  double2 const s = bfSumPartials(partialIn, q, nb, sh);
  double const nrm = sqrt(s.x);
  if (blockIdx.x == 0 && threadIdx.x == 0) scale[q] = ldexp(nrm, (int)expIn[q]);
  bool const live = nrm > 0.0;
  double const unit = 1.0 / sqrt((double)n);
  uint64_t r0, r1;
  bfRowRange(n, nb, r0, r1);
  for (uint64_t r = r0 + threadIdx.x; r < r1; r += BF_GM_THREADS) {
    if (live) { double2 const v = R[r * nrhs + q]; Rhat[r * nrhs + q] = make_double2(v.x / nrm, v.y / nrm); }
    else Rhat[r * nrhs + q] = make_double2(unit, 0.0);
  }
}

// Xout = Xin + scale[q] * D; where scale[q] is not positive the column is Xin bit for bit (D is not read)
__global__ __launch_bounds__(BF_GM_THREADS) void bfRefineUpdateKernel(double2 const *Xin, double2 const *D, double const *scale, double2 *Xout,
                                                                     uint64_t n, uint32_t nrhs) {
  uint64_t const e = (uint64_t)blockIdx.x * BF_GM_THREADS + threadIdx.x;
  if (e >= n * nrhs) return;
  double const s = scale[e % nrhs];
  double2 x = Xin ? Xin[e] : make_double2(0.0, 0.0);
  if (s > 0.0) {
    double2 const d = D[e];
    x.x += s * d.x;
    x.y += s * d.y;
  }
  Xout[e] = x;
}

extern "C" {

int bfdevGmresResidual(void const *B, void const *AX0, void *W, void *partialOut, uint64_t n, uint32_t nrhs, uint32_t nb, void *expOut,
                       void *partialScaled, void *stream) {
  hipLaunchKernelGGL(bfGmresResidualKernel, dim3(nb, nrhs), dim3(BF_GM_THREADS), 0, (hipStream_t)stream, (double2 const *)B, (double2 const *)AX0, (double2 *)W, (double2 *)partialOut, n, nrhs, nb);
  int rc = bfHipFail(hipGetLastError(), "gmres residual launch");
  if (rc || !expOut) return rc;
  hipLaunchKernelGGL(bfGmresScaleKernel, dim3(nb, nrhs), dim3(BF_GM_THREADS), 0, (hipStream_t)stream, (double2 *)W, (double2 const *)partialOut, (double *)expOut, (double2 *)partialScaled, n, nrhs, nb);
  return bfHipFail(hipGetLastError(), "gmres scale launch");
}
int bfdevGmresDot(void const *Vi, void const *W, void *partialOut, uint64_t n, uint32_t nrhs, uint32_t nb, void *stream) {
  hipLaunchKernelGGL(bfGmresDotKernel, dim3(nb, nrhs), dim3(BF_GM_THREADS), 0, (hipStream_t)stream, (double2 const *)Vi, (double2 const *)W, (double2 *)partialOut, n, nrhs, nb);
  return bfHipFail(hipGetLastError(), "gmres dot launch");
}
int bfdevGmresMgsStep(void const *Vi, void const *Vnext, void *W, void const *partialIn, void *partialOut, void *hOut,
                      uint64_t n, uint32_t nrhs, uint32_t nb, void *stream) {
  hipLaunchKernelGGL(bfGmresMgsKernel, dim3(nb, nrhs), dim3(BF_GM_THREADS), 0, (hipStream_t)stream, (double2 const *)Vi, (double2 const *)Vnext, (double2 *)W, (double2 const *)partialIn, (double2 *)partialOut, (double2 *)hOut, n, nrhs, nb);
  return bfHipFail(hipGetLastError(), "gmres mgs launch");
}
int bfdevGmresFinish(void const *W, void const *partialIn, void *Vout, void *hOut, uint64_t n, uint32_t nrhs, uint32_t nb, void *stream) {
  hipLaunchKernelGGL(bfGmresFinishKernel, dim3(nb, nrhs), dim3(BF_GM_THREADS), 0, (hipStream_t)stream, (double2 const *)W, (double2 const *)partialIn, (double2 *)Vout, (double2 *)hOut, n, nrhs, nb);
  return bfHipFail(hipGetLastError(), "gmres finish launch");
}
int bfdevGmresDots(void const *V, void const *W, void *partial, uint64_t n, uint32_t nrhs, uint32_t nb, uint32_t numVec, void *stream) {
  hipLaunchKernelGGL(bfGmresDotsKernel, dim3(nb, nrhs, (numVec + BF_GM_GROUP - 1) / BF_GM_GROUP), dim3(BF_GM_THREADS), 0, (hipStream_t)stream,
                     (double2 const *)V, (double2 const *)W, (double2 *)partial, n, nrhs, nb, numVec);
  return bfHipFail(hipGetLastError(), "gmres dots launch");
}
int bfdevGmresDotsFinish(void const *partial, void const *hPrev, void *h, void *hSum, uint32_t nrhs, uint32_t nb, uint32_t numVec, void *stream) {
  hipLaunchKernelGGL(bfGmresDotsFinishKernel, dim3(numVec, nrhs), dim3(BF_GM_THREADS), 0, (hipStream_t)stream, (double2 const *)partial,
                     (double2 const *)hPrev, (double2 *)h, (double2 *)hSum, nrhs, nb, numVec);
  return bfHipFail(hipGetLastError(), "gmres dots-finish launch");
}
int bfdevGmresProject(void const *V, void *W, void const *h, void *partialOut, uint64_t n, uint32_t nrhs, uint32_t nb, uint32_t numVec, void *stream) {
  hipLaunchKernelGGL(bfGmresProjectKernel, dim3(nb, nrhs), dim3(BF_GM_THREADS), 0, (hipStream_t)stream, (double2 const *)V, (double2 *)W,
                     (double2 const *)h, (double2 *)partialOut, n, nrhs, nb, numVec);
  return bfHipFail(hipGetLastError(), "gmres project launch");
}
int bfdevGmresUpdate(void const *X0, void const *V, void const *y, uint32_t j, void *X, uint64_t n, uint32_t nrhs, void *stream) {
  uint64_t total = n * nrhs;
  hipLaunchKernelGGL(bfGmresUpdateKernel, dim3((uint32_t)((total + BF_GM_THREADS - 1) / BF_GM_THREADS)), dim3(BF_GM_THREADS), 0, (hipStream_t)stream, (double2 const *)X0, (double2 const *)V, (double2 const *)y, j, (double2 *)X, n, nrhs);
  return bfHipFail(hipGetLastError(), "gmres update launch");
}
static inline dim3 bfRefineGrid(uint64_t count) { return dim3((uint32_t)((count + BF_GM_THREADS - 1) / BF_GM_THREADS)); }
int bfdevRefineDemote(void const *src128, void *dst64, uint64_t count, void *stream) {
  if (!count) return 0;
  hipLaunchKernelGGL(bfRefineDemoteKernel, bfRefineGrid(count), dim3(BF_GM_THREADS), 0, (hipStream_t)stream, (double2 const *)src128, (float2 *)dst64, count);
  return bfHipFail(hipGetLastError(), "refine demote launch");
}
int bfdevRefinePromote(void const *src64, void *dst128, uint64_t count, void *stream) {
  if (!count) return 0;
  hipLaunchKernelGGL(bfRefinePromoteKernel, bfRefineGrid(count), dim3(BF_GM_THREADS), 0, (hipStream_t)stream, (float2 const *)src64, (double2 *)dst128, count);
  return bfHipFail(hipGetLastError(), "refine promote launch");
}
int bfdevRefineScale(void const *R, void const *partialIn, double const *expIn, void *Rhat, double *scale, uint64_t n, uint32_t nrhs, uint32_t nb,
                     void *stream) {
  hipLaunchKernelGGL(bfRefineScaleKernel, dim3(nb, nrhs), dim3(BF_GM_THREADS), 0, (hipStream_t)stream, (double2 const *)R, (double2 const *)partialIn,
                     expIn, (double2 *)Rhat, scale, n, nrhs, nb);
  return bfHipFail(hipGetLastError(), "refine scale launch");
}
int bfdevRefineUpdate(void const *Xin, void const *D, double const *scale, void *Xout, uint64_t n, uint32_t nrhs, void *stream) {
  if (!n) return 0;
  hipLaunchKernelGGL(bfRefineUpdateKernel, bfRefineGrid(n * nrhs), dim3(BF_GM_THREADS), 0, (hipStream_t)stream, (double2 const *)Xin, (double2 const *)D,
                     scale, (double2 *)Xout, n, nrhs);
  return bfHipFail(hipGetLastError(), "refine update launch");
}

}  // extern "C"
