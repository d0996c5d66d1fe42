// bfhip_build.hip -- gfx950 device layer of the fac_helm2 value builder: the value side
// (include/bfhip_build.h).
//
// What runs here replaces, for every dense leaf of a Helmholtz butterfly,
//   * bfHelm2GetKernelMatrix (single layer)        reference src/helm2.c:93-125
//       -> bfEvalKernel: one Hankel evaluation per matrix element, all kernel
//          matrices of a batch in one launch (flat tile list, binary search);
//   * the leaf -> packed-arena copy that bfhip_api.c does on the host for
//     host-valued operands -> bfPackKernel.
// Plus bfHelm2DenseKernel, the matrix-free N x N kernel matvec used as the
// acceptance check (examples/simple/bf_all_blocks.c:132-153).
// The re-expansion matrices (truncated least squares) are in bfhip_lstsq.hip.
//
// None of these kernels is on the apply path; they are compute-bound FP64 VALU
// work (Bessel functions) and are written for clarity first: fixed
// summation orders, no atomics in any result.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"
#include "../../include/bfhip_build.h"

// ---------------------------------------------------------------------------
// points and the kernel
// ---------------------------------------------------------------------------
__device__ __forceinline__ void bfPoint(BfBuildPts const &ps, uint32_t i, double const *pts, double const *tpts, double &x, double &y) {
  if (ps.kind != BFHIP_PTS_CIRCLE) {
    double const *base = ps.kind == BFHIP_PTS_TREE ? pts : tpts;
    x = base[2 * (ps.first + i)];
    y = base[2 * (ps.first + i) + 1];
  } else {
    // bfCircle2SamplePoints, src/circle.c:12-35
    double const theta = (6.283185307179586 / (double)ps.count) * (double)i;
    x = ps.r * cos(theta) + ps.cx;
    y = ps.r * sin(theta) + ps.cy;
  }
}

// S : (i/4) H0^(1)(k r)                           = (-Y0 + i J0)(kr) / 4            src/helm2.c:111-117
// S': (i/4) k H1^(1)(k r)/r  n_tgt.(x_tgt - x_src)  = (-Y1 + i J1)(kr) k dot / (4 r)  src/helm2.c:155-163
// D : the same with the SOURCE normal                                                src/helm2.c:200-208
// combined field: alpha S + beta D                                                   src/helm2.c:253-266
// all 0 at r == 0.  (dx, dy) = x_tgt - x_src; (nx, ny) = the normal the potential uses.
__device__ __forceinline__ double2 bfHelm2G(double k, double dx, double dy) {
  double const r = hypot(dx, dy);
  if (r == 0.0) return make_double2(0.0, 0.0);
  double const kr = k * r;
  return make_double2(-0.25 * y0(kr), 0.25 * j0(kr));
}
__device__ __forceinline__ double2 bfHelm2Sp(double k, double dx, double dy, double nx, double ny) {
  double const r = hypot(dx, dy);
  if (r == 0.0) return make_double2(0.0, 0.0);
  double const kr = k * r;
  double const sc = 0.25 * k * (nx * dx + ny * dy) / r;
  return make_double2(-sc * y1(kr), sc * j1(kr));
}

// Kapur-Rokhlin end-point corrections of the punctured trapezoid rule for a log-singular kernel
// (Kapur & Rokhlin, SIAM J. Numer. Anal. 34, 1997, Table 6).  Orders 2 and 6 are the tables the reference
// applies (src/quadrature.c:12-26).  Order 10 departs from it on purpose: the reference's printing
// (src/quadrature.c:29-40) lost the decimal exponents of the paper's table, sums to -4.48 instead of 1/2 and
// converges at order 1; the values here are the paper's (sum 0.49999999999982, observed order 10: DESIGN.md
// section 23).
__constant__ double bfKrWeights[18] = {
    1.825748064736159, -1.325748064736159,
    4.967362978287758, -16.20501504859126, 25.85153761832639, -22.22599466791883, 9.930104998037539, -1.817995878141594,
    7.832432020568779e+00, -4.565161670374749e+01, 1.452168846354677e+02, -2.901348302886379e+02, 3.870862162579900e+02,
    -3.523821383570681e+02, 2.172421547519342e+02, -8.707796087382991e+01, 2.053584266072635e+01, -2.166984103403823e+00};

struct EvalEnvDev {
  double const *pts, *normals, *colWeights, *tpts, *tnormals;
  uint64_t const *orig;
  double k, selfRe, selfIm;
  double2 alpha, beta;
  uint64_t n;
  uint32_t krOrder, krBase;          // krBase: offset of the order's table in bfKrWeights
  unsigned long long *krHits;
};

// 1 + w_KR[d-1] if original indices a, b are d = 1..order apart on the closed curve, else 1
__device__ __forceinline__ double bfKrFactor(EvalEnvDev const &E, uint64_t a, uint64_t b, bool &hit) {
  uint64_t const fwd = a >= b ? a - b : a + E.n - b;        // (a - b) mod n
  uint64_t const d = fwd <= E.n - fwd ? fwd : E.n - fwd;
  hit = d >= 1 && d <= E.krOrder;
  return hit ? 1.0 + bfKrWeights[E.krBase + d - 1] : 1.0;
}

// kernel value for potential `pot`: (sx, sy) source normal, (tx, ty) target normal (used as needed)
__device__ __forceinline__ double2 bfKernelValue(EvalEnvDev const &E, uint32_t pot, double dx, double dy, double snx, double sny,
                                                  double tnx, double tny) {
  switch (pot) {
    case 1: return bfHelm2Sp(E.k, dx, dy, tnx, tny);
    case 2: return bfHelm2Sp(E.k, dx, dy, snx, sny);
    case 3: {
      double2 const S = bfHelm2G(E.k, dx, dy), D = bfHelm2Sp(E.k, dx, dy, snx, sny);
      return make_double2(E.alpha.x * S.x - E.alpha.y * S.y + E.beta.x * D.x - E.beta.y * D.y,
                          E.alpha.x * S.y + E.alpha.y * S.x + E.beta.x * D.y + E.beta.y * D.x);
    }
    default: return bfHelm2G(E.k, dx, dy);
  }
}

// unit normal at point i of a point set: stored normals for tree points, the radial direction for a
// sampled circle (bfCircle2SampleUnitNormals, src/circle.c:36-58)
__device__ __forceinline__ void bfNormal(EvalEnvDev const &E, BfBuildPts const &ps, uint32_t i, double &nx, double &ny) {
  if (ps.kind != BFHIP_PTS_CIRCLE) {
    double const *base = ps.kind == BFHIP_PTS_TREE ? E.normals : E.tnormals;
    nx = base[2 * (ps.first + i)];
    ny = base[2 * (ps.first + i) + 1];
  } else {
    double const theta = (6.283185307179586 / (double)ps.count) * (double)i;
    nx = cos(theta);
    ny = sin(theta);
  }
}

// one entry of a kernel matrix: target i of `tgt`, source j of `src`
__device__ __forceinline__ double2 bfKernelEntry(EvalEnvDev const &E, BfBuildPts const &src, BfBuildPts const &tgt, uint32_t i, uint32_t j,
                                                  uint32_t pot, uint32_t decorate) {
  double tx, ty, sx, sy;
  bfPoint(tgt, i, E.pts, E.tpts, tx, ty);
  bfPoint(src, j, E.pts, E.tpts, sx, sy);
  bool const bothTree = src.kind == BFHIP_PTS_TREE && tgt.kind == BFHIP_PTS_TREE;
  if (decorate && bothTree && tgt.first + i == src.first + j) return make_double2(E.selfRe, E.selfIm);
  double snx = 0, sny = 0, tnx = 0, tny = 0;
  if (pot == 1) bfNormal(E, tgt, i, tnx, tny);       // S' leaves have tree targets (checked on the host)
  if (pot >= 2) bfNormal(E, src, j, snx, sny);
  double2 g = bfKernelValue(E, pot, tx - sx, ty - sy, snx, sny, tnx, tny);
  if (decorate && E.krOrder && bothTree) {
    bool hit;
    double const f = bfKrFactor(E, E.orig[tgt.first + i], E.orig[src.first + j], hit);
    g.x *= f; g.y *= f;
    if (hit && E.krHits) atomicAdd(E.krHits, 1ull);          // bookkeeping only: every pair must be met exactly once
  }
  if (decorate && E.colWeights && src.kind == BFHIP_PTS_TREE) {
    double const w = E.colWeights[src.first + j];
    g.x *= w; g.y *= w;
  }
  return g;
}

__global__ __launch_bounds__(256) void bfEvalKernel(BfEvalMat const *mats, uint64_t const *prefix, uint32_t numMats, EvalEnvDev const E,
                                                    uint64_t tileBase) {
  uint64_t const tile = tileBase + blockIdx.x;
  uint32_t lo = 0, hi = numMats;                   // prefix[lo] <= tile < prefix[hi]
  while (hi - lo > 1) {
    uint32_t const mid = (lo + hi) >> 1;
    if (prefix[mid] <= tile) lo = mid; else hi = mid;
  }
  BfEvalMat const M = mats[lo];
  uint64_t const total = (uint64_t)M.tgt.count * M.src.count;
  uint64_t const e0 = (tile - prefix[lo]) * BF_EVAL_TILE;
  double2 *dst = (double2 *)M.dst;
#pragma unroll
  for (int q = 0; q < (int)(BF_EVAL_TILE / 256); ++q) {
    uint64_t const e = e0 + (uint64_t)q * 256 + threadIdx.x;
    if (e >= total) break;
    uint32_t const i = (uint32_t)(e % M.tgt.count), j = (uint32_t)(e / M.tgt.count);
    dst[e] = bfKernelEntry(E, M.src, M.tgt, i, j, M.pot, M.decorate);
  }
}

static EvalEnvDev toDev(BfEvalEnv const *env) {
  EvalEnvDev E;
  E.pts = (double const *)env->dPoints; E.normals = (double const *)env->dNormals; E.colWeights = (double const *)env->dColWeights;
  E.tpts = (double const *)env->dTgtPoints; E.tnormals = (double const *)env->dTgtNormals;
  E.k = env->wavenumber; E.selfRe = env->selfRe; E.selfIm = env->selfIm;
  E.alpha = make_double2(env->alphaRe, env->alphaIm); E.beta = make_double2(env->betaRe, env->betaIm);
  E.orig = (uint64_t const *)env->dOrigIndex; E.n = env->numPoints;
  E.krOrder = env->dOrigIndex ? env->krOrder : 0;
  E.krBase = env->krOrder == 2 ? 0 : env->krOrder == 6 ? 2 : 8;
  E.krHits = env->dKrHits;
  return E;
}

int bfdevBuildEval(BfEvalMat const *hostMats, uint64_t const *hostTilePrefix, uint64_t numMats, BfEvalEnv const *env) {
  if (!numMats) return 0;
  BfEvalMat *dM = NULL;
  uint64_t *dP = NULL;
  int rc = uploadArrayB(&dM, hostMats, numMats, "eval matrices");
  if (!rc) rc = uploadArrayB(&dP, hostTilePrefix, numMats + 1, "eval tile prefix");
  uint64_t const tiles = hostTilePrefix[numMats];
  for (uint64_t done = 0; done < tiles && !rc;) {
    uint32_t const n = (uint32_t)(tiles - done > (1u << 30) ? (1u << 30) : tiles - done);
    hipLaunchKernelGGL(bfEvalKernel, dim3(n), dim3(256), 0, 0, dM, dP, (uint32_t)numMats, toDev(env), done);
    rc = bfHipFail(hipGetLastError(), "kernel-matrix evaluation launch");
    done += n;
  }
  if (!rc) rc = bfHipFail(hipDeviceSynchronize(), "kernel-matrix evaluation");
  (void)hipFree(dM);
  (void)hipFree(dP);
  return rc;
}

// ---------------------------------------------------------------------------
// leaf store (column-major leaves of one batch) -> packed arena pieces
// ---------------------------------------------------------------------------
// The arena element of a store value: complex128 copied, complex64 with each component rounded to nearest even once
// (what packPiece does on the host for a complex64 plan, bfhip_api.c).
template <typename T> __device__ __forceinline__ T bfPackCvt(double2 v);
template <> __device__ __forceinline__ double2 bfPackCvt<double2>(double2 v) { return v; }
template <> __device__ __forceinline__ float2 bfPackCvt<float2>(double2 v) { return make_float2((float)v.x, (float)v.y); }

// One workgroup per piece.  Column-major pieces: lanes run along the padded rows, contiguous in the arena and (within a column)
// in the store.  Row-major pieces (a few rows, real-family plans only): a lane owns a column of the padded row, reads that
// column's mr consecutive store elements and writes one element per row, so for a fixed row consecutive lanes write
// consecutive elements.  The padding (rows mr..mrPad, columns ncols..ld) is written: the stage kernels read it.
template <typename T>
__global__ __launch_bounds__(256) void bfPackKernel(T *arena, double2 const *store, BfPackPiece const *pieces, uint64_t base) {
  BfPackPiece const pc = pieces[base + blockIdx.x];
  T *dst = arena + pc.dataOff;
  double2 const *src = store + pc.srcOff;
  double2 const zero = make_double2(0.0, 0.0);
  if (pc.rowMajor) {
    for (uint32_t c = threadIdx.x; c < pc.ld; c += 256) {
      double2 const *col = src + (uint64_t)c * pc.srcLd;
      for (uint32_t r = 0; r < pc.mr; ++r) dst[(uint64_t)r * pc.ld + c] = bfPackCvt<T>(c < pc.ncols ? col[r] : zero);
    }
    return;
  }
  uint32_t const total = pc.mrPad * pc.ncols;
  for (uint32_t e = threadIdx.x; e < total; e += 256) {
    uint32_t const r = e % pc.mrPad, c = e / pc.mrPad;
    dst[e] = bfPackCvt<T>(r < pc.mr ? src[(uint64_t)c * pc.srcLd + r] : zero);
  }
}

int bfdevBuildPack(void *arena, uint32_t outDtype, void const *store, BfPackPiece const *hostPieces, uint64_t count) {
  if (!count) return 0;
  if (outDtype != BFHIP_C128 && outDtype != BFHIP_C64) return bfhipFail(BFABI_ERROR_TYPE_ERROR, "the builder packs complex128 or complex64 arenas");
  BfPackPiece *d = NULL;
  int rc = uploadArrayB(&d, hostPieces, count, "pack pieces");
  for (uint64_t done = 0; done < count && !rc;) {
    uint32_t const n = (uint32_t)(count - done > (1u << 30) ? (1u << 30) : count - done);
    if (outDtype == BFHIP_C64)
      hipLaunchKernelGGL(bfPackKernel<float2>, dim3(n), dim3(256), 0, 0, (float2 *)arena, (double2 const *)store, d, done);
    else
      hipLaunchKernelGGL(bfPackKernel<double2>, dim3(n), dim3(256), 0, 0, (double2 *)arena, (double2 const *)store, d, done);
    rc = bfHipFail(hipGetLastError(), "pack launch");
    done += n;
  }
  if (!rc) rc = bfHipFail(hipDeviceSynchronize(), "pack");
  (void)hipFree(d);
  return rc;
}

// ---------------------------------------------------------------------------
// matrix-free dense apply: y_i = sum_j G(p_i, p_j) x_j.  A workgroup owns 256
// targets and one slice of the sources (staged through LDS, 256 at a time);
// slices are summed afterwards in fixed order.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bfHelm2DenseKernel(EvalEnvDev const E, uint32_t pot, uint64_t n, uint64_t m, bool square,
                                                          double2 const *x, double2 *partial, uint64_t sliceLen) {
  __shared__ double sx[256], sy[256], sw[256];
  __shared__ double2 xv[256];
  __shared__ uint64_t so[256];
  __shared__ double snx[256], sny[256];
  uint64_t const i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t const j0 = (uint64_t)blockIdx.y * sliceLen;
  uint64_t const j1 = j0 + sliceLen < n ? j0 + sliceLen : n;
  double tx = 0, ty = 0, nx = 0, ny = 0;
  uint64_t oi = 0;
  double const *tp = square ? E.pts : E.tpts, *tn = square ? E.normals : E.tnormals;
  bool const kr = square && E.krOrder;
  if (i < m) {
    tx = tp[2 * i]; ty = tp[2 * i + 1];
    if (pot == 1) { nx = tn[2 * i]; ny = tn[2 * i + 1]; }
    if (kr) oi = E.orig[i];
  }
  double ar = 0, ai = 0;
  for (uint64_t jb = j0; jb < j1; jb += 256) {
    uint64_t const j = jb + threadIdx.x;
    __syncthreads();
    if (j < j1) {
      sx[threadIdx.x] = E.pts[2 * j]; sy[threadIdx.x] = E.pts[2 * j + 1]; xv[threadIdx.x] = x[j];
      sw[threadIdx.x] = E.colWeights ? E.colWeights[j] : 1.0;
      so[threadIdx.x] = kr ? E.orig[j] : 0;
      snx[threadIdx.x] = pot >= 2 ? E.normals[2 * j] : 0.0;
      sny[threadIdx.x] = pot >= 2 ? E.normals[2 * j + 1] : 0.0;
    }
    __syncthreads();
    uint32_t const cnt = (uint32_t)(j1 - jb < 256 ? j1 - jb : 256);
    if (i < m)
      for (uint32_t t = 0; t < cnt; ++t) {
        double2 g;
        if (square && jb + t == i) g = make_double2(E.selfRe, E.selfIm);
        else {
          g = bfKernelValue(E, pot, tx - sx[t], ty - sy[t], snx[t], sny[t], nx, ny);
          bool hit;
          double const f = sw[t] * (kr ? bfKrFactor(E, oi, so[t], hit) : 1.0);
          g.x *= f; g.y *= f;
        }
        double2 const v = xv[t];
        ar = fma(g.x, v.x, ar); ar = fma(-g.y, v.y, ar);
        ai = fma(g.x, v.y, ai); ai = fma(g.y, v.x, ai);
      }
  }
  if (i < m) partial[(uint64_t)blockIdx.y * m + i] = make_double2(ar, ai);
}

__global__ __launch_bounds__(256) void bfSliceSumKernel(double2 const *partial, uint64_t n, uint32_t slices, double2 *y) {
  uint64_t const i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double sr = 0, si = 0;
  for (uint32_t s = 0; s < slices; ++s) { double2 const v = partial[(uint64_t)s * n + i]; sr += v.x; si += v.y; }
  y[i] = make_double2(sr, si);
}

int bfdevMemFree(uint64_t *freeBytes) {
  size_t f = 0, t = 0;
  int rc = bfHipFail(hipMemGetInfo(&f, &t), "hipMemGetInfo");
  *freeBytes = f;
  return rc;
}

int bfdevHelm2Dense(BfEvalEnv const *env, uint32_t pot, uint64_t n, uint64_t numTgt, void const *dX, void *dY, void *stream) {
  if (!n) return 0;
  hipStream_t const s = (hipStream_t)stream;
  bool const square = numTgt == 0;
  uint64_t const m = square ? n : numTgt;
  uint32_t const tb = (uint32_t)((m + 255) / 256);
  // enough workgroups to fill 256 CUs several times over, slices of >= 256 sources
  uint32_t slices = tb >= 4096 ? 1 : (4096 + tb - 1) / tb;
  if ((uint64_t)slices * 256 > n) slices = (uint32_t)((n + 255) / 256);
  uint64_t const sliceLen = ((n + slices - 1) / slices + 255) / 256 * 256;
  slices = (uint32_t)((n + sliceLen - 1) / sliceLen);
  double2 *partial = NULL;
  int rc = bfHipFail(hipMalloc((void **)&partial, (size_t)slices * m * sizeof(double2)), "hipMalloc(dense apply partials)");
  if (rc) return rc;
  hipLaunchKernelGGL(bfHelm2DenseKernel, dim3(tb, slices), dim3(256), 0, s, toDev(env), pot, n, m, square, (double2 const *)dX, partial, sliceLen);
  rc = bfHipFail(hipGetLastError(), "dense apply launch");
  if (!rc) {
    hipLaunchKernelGGL(bfSliceSumKernel, dim3(tb), dim3(256), 0, s, partial, m, slices, (double2 *)dY);
    rc = bfHipFail(hipGetLastError(), "dense apply sum launch");
  }
  if (!rc) rc = bfHipFail(hipStreamSynchronize(s), "dense apply");
  (void)hipFree(partial);
  return rc;
}
