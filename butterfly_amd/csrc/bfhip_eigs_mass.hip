// bfhip_eigs_mass.hip -- the kernels the consistent-mass pencil S u = theta B u adds to the filtered subspace iteration
// (BFHIP_EIGS_CONSISTENT_MASS, include/bfhip.h; host side: bfhip_eigs.c, bfhip_eigs_mass.c).  B = D M D lies
// on S's CSR pattern with values of its own; the blocks are bfhip_eigs.hip's (row-major n x ld doubles, the first p columns in
// use, the padding zero and never written).
//
//   bfEigsMassStepKernel  out = alpha (B b1) + beta b1 + gamma b2 + delta w    B X, and every step of the mass solve
//   bfEigsCombineKernel   out = a z + b y1 + g y2                              the filter's three-term combination
//   bfEigsDualProductKernel  Y = S b1 and T = B b1 from one gather             Rayleigh-Ritz (0.64 of two launches, section 28)
//
// The projection against locked vectors in the B inner product is bfhip_eigs.hip's two deflation kernels on (Q, B X).  No
// atomics and no sum whose order depends on anything but (n, p): two calls give the same bits.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"
#include "bfhip_cheb_gather.h"

#define BF_EIGS_MAX_GRID (1u << 20)

// bfEigsStepKernel (bfhip_eigs.hip) with one more block stream, w: the lane layout, the gather groups and the row sum of
// bfhip_cheb_gather.h.  Per element: r = alpha * sum; r = fma(beta, b1, r); r = fma(gamma, b2, r); r = fma(delta, w, r) -- the
// same sequence for every p, so column j of a p-column block equals the one-column result bit for bit.  A NULL b2 or w drops
// its fma; a NULL b1 gathers nothing (sum = 0, own = 0).  out may be b2 (an element's owner is the only reader of its b2
// element) and nothing else the kernel reads.
__global__ __launch_bounds__(256) void bfEigsMassStepKernel(BfEigsMassStep a, uint32_t lanesLog2) {
  uint32_t const lanes = 1u << lanesLog2, lane = threadIdx.x & (lanes - 1), rowsPerWg = 256u >> lanesLog2;
  uint64_t const p = a.p, ld = a.ld;
  for (uint64_t i = (uint64_t)blockIdx.x * rowsPerWg + (threadIdx.x >> lanesLog2); i < a.n; i += (uint64_t)gridDim.x * rowsPerWg) {
    uint64_t beg = 0, end = 0;
    if (a.b1) { beg = a.rowptr[i]; end = a.rowptr[i + 1]; }
    for (uint64_t c0 = 0; c0 < p; c0 += lanes) {
      uint64_t const c = c0 + lane;
      bool const live = c < p;
      double own = 0, old = 0, rhs = 0;
      if (live) {
        if (a.b1) own = a.b1[i * ld + c];
        if (a.b2) old = a.b2[i * ld + c];
        if (a.w) rhs = a.w[i * ld + c];
      }
      double const acc = bfChebRowGather(a.colind, a.val, beg, end, a.b1, ld, c, lane, lanes, live);
      double r = a.alpha * acc;
      r = fma(a.beta, own, r);
      if (a.b2) r = fma(a.gamma, old, r);
      if (a.w) r = fma(a.delta, rhs, r);
      if (live) a.out[i * ld + c] = r;
    }
  }
}

// out[i][c] = fma(g, y2, fma(b, y1, a * z)), c < p: one thread per element of the live columns, rows by a grid stride
__global__ __launch_bounds__(256) void bfEigsCombineKernel(double const *z, double const *y1, double const *y2, double *out, uint64_t n, uint32_t p,
                                                           uint32_t ld, double a, double b, double g) {
  uint64_t const total = n * p;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
    uint64_t const i = e / p, k = i * ld + (e - i * p);
    double r = a * z[k];
    r = fma(b, y1[k], r);
    if (y2) r = fma(g, y2[k], r);
    out[k] = r;
  }
}

// Y = S b1 and T = B b1 from one gather of b1's rows: bfChebRowGather with two value arrays and two sums, each in the order the
// single kernels use, so both outputs equal the two single launches bit for bit.
__global__ __launch_bounds__(256) void bfEigsDualProductKernel(uint64_t const *rowptr, uint32_t const *colind, double const *valS, double const *valB,
                                                               uint64_t n, uint32_t p, uint32_t ld, double const *b1, double *outS, double *outB,
                                                               uint32_t lanesLog2) {
  constexpr int G = BF_CHEB_GATHERS;
  uint32_t const lanes = 1u << lanesLog2, lane = threadIdx.x & (lanes - 1), rowsPerWg = 256u >> lanesLog2;
  bool const shared = lanes >= (uint32_t)G;
  for (uint64_t i = (uint64_t)blockIdx.x * rowsPerWg + (threadIdx.x >> lanesLog2); i < n; i += (uint64_t)gridDim.x * rowsPerWg) {
    uint64_t const beg = rowptr[i], end = rowptr[i + 1];
    for (uint64_t c0 = 0; c0 < p; c0 += lanes) {
      uint64_t const c = c0 + lane;
      bool const live = c < p;
      double accS = 0, accB = 0;
      for (uint64_t j = beg; j < end; j += G) {
        double vs[G], vb[G];
        uint32_t col[G];
        if (shared) {
          uint64_t const mine = j + (lane & (G - 1)) < end ? j + (lane & (G - 1)) : end - 1;
          double const ps = valS[mine], pb = valB[mine];
          uint32_t const pc = colind[mine];
#pragma unroll
          for (int t = 0; t < G; ++t) {
            vs[t] = __shfl(ps, t, (int)lanes);
            vb[t] = __shfl(pb, t, (int)lanes);
            col[t] = __shfl(pc, t, (int)lanes);
          }
        } else {
#pragma unroll
          for (int t = 0; t < G; ++t) {
            uint64_t const jj = j + t < end ? j + t : end - 1;
            vs[t] = valS[jj]; vb[t] = valB[jj];
            col[t] = colind[jj];
          }
        }
        if (live) {
          double x[G];
#pragma unroll
          for (int t = 0; t < G; ++t) x[t] = j + t < end ? b1[(uint64_t)col[t] * ld + c] : 0.0;
#pragma unroll
          for (int t = 0; t < G; ++t)
            if (j + t < end) { accS = fma(vs[t], x[t], accS); accB = fma(vb[t], x[t], accB); }
        }
      }
      if (live) { outS[i * ld + c] = accS; outB[i * ld + c] = accB; }
    }
  }
}

// ---- launches ------------------------------------------------------------------------------------------------------------
int bfdevEigsMassStep(BfEigsMassStep const *s, void *stream) {
  if (!s || !s->out || (s->b1 && (!s->rowptr || !s->colind || !s->val)))
    return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "eigensolver mass step: NULL argument");
  if (s->p > s->ld) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "eigensolver mass step: p is more than ld");
  if (!s->n || !s->p) return 0;
  uint32_t lg = 0;
  while ((1u << lg) < s->p && lg < 6) ++lg;
  uint64_t const perWg = 256u >> lg, need = (s->n + perWg - 1) / perWg;
  dim3 const grid((uint32_t)(need < BF_EIGS_MAX_GRID ? need : BF_EIGS_MAX_GRID)), block(256);
  hipLaunchKernelGGL(bfEigsMassStepKernel, grid, block, 0, (hipStream_t)stream, *s, lg);
  return bfHipFail(hipGetLastError(), "eigensolver mass step launch");
}

int bfdevEigsDualProduct(uint64_t const *rowptr, uint32_t const *colind, double const *valS, double const *valB, uint64_t n, uint32_t p, uint32_t ld,
                         double const *b1, double *outS, double *outB, void *stream) {
  if (!rowptr || !colind || !valS || !valB || !b1 || !outS || !outB) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "eigensolver dual product: NULL argument");
  if (p > ld) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "eigensolver dual product: p is more than ld");
  if (!n || !p) return 0;
  uint32_t lg = 0;
  while ((1u << lg) < p && lg < 6) ++lg;
  uint64_t const perWg = 256u >> lg, need = (n + perWg - 1) / perWg;
  dim3 const grid((uint32_t)(need < BF_EIGS_MAX_GRID ? need : BF_EIGS_MAX_GRID)), block(256);
  hipLaunchKernelGGL(bfEigsDualProductKernel, grid, block, 0, (hipStream_t)stream, rowptr, colind, valS, valB, n, p, ld, b1, outS, outB, lg);
  return bfHipFail(hipGetLastError(), "eigensolver dual product launch");
}

// The three-term Chebyshev semi-iteration for B z = t on [lo, hi] (Golub and Varga, Numer. Math. 3, 1961; Saad, Iterative
// Methods for Sparse Linear Systems, section 12.3): with theta = (hi + lo) / 2, sigma = theta / ((hi - lo) / 2),
//   z_1 = t / theta,   z_{j+1} = z_{j-1} + omega_{j+1} ((t - B z_j) / theta + z_j - z_{j-1}),
//   omega_2 = 2 sigma^2 / (2 sigma^2 - 1),   omega_{j+1} = 1 / (1 - omega_j / (4 sigma^2)),
// z_{j+1} written over z_{j-1}.  The error after k steps is at most 2 rho^k / (1 + rho^2k) of ||B^-1 t||_2.  The two blocks
// alternate so that step `steps` lands in z.
int bfdevEigsMassSolve(BfEigsMassSolve const *s, void *stream) {
  if (!s || !s->t || !s->z || !s->work) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "eigensolver mass solve: NULL argument");
  if (!s->steps) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "eigensolver mass solve: no steps");
  if (!(s->lo > 0) || !(s->hi > s->lo) || s->hi > 1.79e308) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "eigensolver mass solve: 0 < lo < hi, finite");
  double const theta = (s->hi + s->lo) / 2, sigma = theta / ((s->hi - s->lo) / 2), inv = 1 / theta;
  double *cur = s->steps & 1 ? s->z : s->work, *prev = s->steps & 1 ? s->work : s->z;
  BfEigsMassStep st = { s->rowptr, s->colind, s->val, s->n, s->p, s->ld, NULL, NULL, s->t, cur, 0.0, 0.0, 0.0, inv };
  int rc = bfdevEigsMassStep(&st, stream);
  double omega = 1;
  for (uint32_t j = 1; !rc && j < s->steps; ++j) {
    omega = j == 1 ? 2 * sigma * sigma / (2 * sigma * sigma - 1) : 1 / (1 - omega / (4 * sigma * sigma));
    st.b1 = cur; st.b2 = j == 1 ? NULL : prev; st.out = prev;
    st.alpha = -omega * inv; st.beta = omega; st.gamma = 1 - omega; st.delta = omega * inv;
    rc = bfdevEigsMassStep(&st, stream);
    double *t = prev; prev = cur; cur = t;
  }
  return rc;
}

int bfdevEigsCombine(double const *z, double const *y1, double const *y2, double *out, uint64_t n, uint32_t p, uint32_t ld, double a,
                                double b, double g, void *stream) {
  if (!z || !y1 || !out) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "eigensolver combine: NULL argument");
  if (p > ld) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "eigensolver combine: p is more than ld");
  if (!n || !p) return 0;
  uint64_t const need = (n * p + 255) / 256;
  dim3 const grid((uint32_t)(need < BF_EIGS_MAX_GRID ? need : BF_EIGS_MAX_GRID)), block(256);
  hipLaunchKernelGGL(bfEigsCombineKernel, grid, block, 0, (hipStream_t)stream, z, y1, y2, out, n, p, ld, a, b, g);
  return bfHipFail(hipGetLastError(), "eigensolver combine launch");
}

// one pass X <- X - Q (Q^T BX) over all m locked columns, BX = B X as it was before the pass: the coefficients of every panel
// come from the same BX (the locked vectors are B-orthonormal, so the panels' corrections do not interact), then the update
int bfdevEigsProjectMass(double const *dQ, uint64_t ldq, uint64_t m, double const *BX, double *X, uint64_t n, uint32_t ld, double *part,
                                    double *C, void *stream) {
  for (uint64_t m0 = 0; m0 < m; m0 += 256) {
    uint32_t const mq = (uint32_t)(m - m0 < 256 ? m - m0 : 256);
    int rc;
    if ((rc = bfdevEigsCrossGram(dQ, ldq, m0, mq, BX, n, ld, part, C, stream)) || (rc = bfdevEigsDeflate(dQ, ldq, m0, mq, C, X, n, ld, stream))) return rc;
  }
  return 0;
}
