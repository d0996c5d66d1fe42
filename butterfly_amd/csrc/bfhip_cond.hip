// bfhip_cond.hip -- the kernels of conditioning on observations (bfhipCovCond*, include/bfhip.h; host side: bfhip_cond.c).
// Nothing here is a stage kernel.  Everything is double except the operator's own blocks (S = double / float), which are
// widened exactly on the way in and rounded once on the way out.  Every index into a matrix is 64 bits; no atomics: each
// output element has one owner and every sum a fixed order that depends on the shapes alone.
//
// Matrices (all row-major, densely packed unless a leading dimension is named):
//   Bt  [n x k]   the observed rows of P Phi Gamma, transposed: Bt[j, a] = Phi[i_a, j] * gamma[j]
//   G   [k x k]   G + D, then its Cholesky factor L in the lower triangle (the strict upper triangle stays zero)
//   R   [k x b]   the residual block, solved in place into alpha            (b <= 64 columns a pass)
//
// One tile routine does every contraction: a workgroup of 256 threads owns a 32 x 64 tile of C = sum_p A(i, p) B(p, s),
// thread (ty, tx) of 16 x 16 owns rows 2 ty .. + 1 and columns 4 tx .. + 3, and p runs in slabs of 32 staged through LDS
// (sa 32 x 33 and sb 32 x 65 doubles: 25 KiB).  A(i, p) = A[i sAi + p sAp], B(p, s) = B[p sBp + s sBs]: the staging loop
// puts neighbouring threads on the unit stride of each operand, so both layouts of Bt and of L are read in whole lines.
// Out-of-range i, s, p are staged as zeros: fma(0, 0, acc) leaves acc as it is.  Each accumulator is one fma chain in
// increasing p.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bfhip_operator.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"

#define BF_COND_TI 32u           // tile rows
#define BF_COND_TS 64u           // tile columns
#define BF_COND_TP 32u           // slab of the contracted index
#define BF_COND_NB 32u           // block size of the Cholesky factorization and of the triangular solves

template <typename TB>
__device__ __forceinline__ void bfCondTileAcc(double (&acc)[2][4], double const *A, uint64_t sAi, uint64_t sAp, uint64_t M, uint64_t i0,
                                              TB const *B, uint64_t sBp, uint64_t sBs, uint64_t Nn, uint64_t s0, uint64_t p0, uint64_t p1,
                                              double (*sa)[BF_COND_TI + 1], double (*sb)[BF_COND_TS + 1]) {
  uint32_t const t = threadIdx.x, ty = t >> 4, tx = t & 15;
  for (uint64_t pp = p0; pp < p1; pp += BF_COND_TP) {
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      uint32_t const e = t + 256 * r;
      uint32_t const pl = sAi == 1 ? e >> 5 : e & 31, il = sAi == 1 ? e & 31 : e >> 5;
      uint64_t const p = pp + pl, i = i0 + il;
      sa[pl][il] = (p < p1 && i < M) ? A[i * sAi + p * sAp] : 0.0;
    }
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
      uint32_t const e = t + 256 * r;
      uint32_t const pl = sBs == 1 ? e >> 6 : e & 31, sl = sBs == 1 ? e & 63 : e >> 5;
      uint64_t const p = pp + pl, s = s0 + sl;
      sb[pl][sl] = (B && p < p1 && s < Nn) ? (double)B[p * sBp + s * sBs] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (uint32_t pl = 0; pl < BF_COND_TP; ++pl) {
      double const a0 = sa[pl][2 * ty], a1 = sa[pl][2 * ty + 1];
#pragma unroll
      for (uint32_t v = 0; v < 4; ++v) {
        double const bv = sb[pl][4 * tx + v];
        acc[0][v] = fma(a0, bv, acc[0][v]);
        acc[1][v] = fma(a1, bv, acc[1][v]);
      }
    }
    __syncthreads();
  }
}

#define BF_COND_TILE_LDS __shared__ double sa[BF_COND_TP][BF_COND_TI + 1]; __shared__ double sb[BF_COND_TP][BF_COND_TS + 1]
// the 2 x 4 elements a thread owns: rows i, columns s of the tile at (blockIdx.x, blockIdx.y)
#define BF_COND_FOR_OWNED(i, s) \
  for (uint32_t u = 0; u < 2; ++u) \
    for (uint32_t v = 0; v < 4; ++v) \
      if (uint64_t const i = (uint64_t)blockIdx.x * BF_COND_TI + 2 * (threadIdx.x >> 4) + u; true) \
        if (uint64_t const s = (uint64_t)blockIdx.y * BF_COND_TS + 4 * (threadIdx.x & 15) + v; true)

// ---------------------------------------------------------------------------
// the observed rows: inverse of the scatter, restricted to the observed indices
// ---------------------------------------------------------------------------
// perm scatters: out[perm[i]] = in[i], so observation a (index o_a of the output) is row i_a with perm[i_a] = o_a.  obs is
// sorted, slot[] names the observation of each sorted entry.  Two launches, no atomics: in the first every row i that hits
// an observed index writes rows[a] = i (if two rows hit the same index one of the stores stays, whichever); in the second
// every such row reads rows[a] back and raises the flag if it holds another row.  An index no row hits keeps the sentinel
// the host wrote.  Exactly once <=> no flag and no sentinel.
__global__ __launch_bounds__(256) void bfCondInvertPermKernel(uint64_t const *perm, uint64_t m, uint64_t const *obs, uint32_t const *slot, uint32_t k,
                                                              uint64_t *rows, uint32_t *flag, int verify) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
    uint64_t const o = perm[i];
    uint32_t lo = 0, hi = k;                  // first entry >= o
    while (lo < hi) { uint32_t const mid = (lo + hi) >> 1; if (obs[mid] < o) lo = mid + 1; else hi = mid; }
    if (lo < k && obs[lo] == o) {
      uint32_t const a = slot[lo];
      if (a < k) {
        if (!verify) rows[a] = i;
        else if (rows[a] != i) *flag = 1;
      }
    }
  }
}

int bfdevCondDeviceSync(void) { return bfHipFail(hipDeviceSynchronize(), "hipDeviceSynchronize"); }

int bfdevCondInvertPerm(uint64_t const *dPerm, uint64_t m, uint64_t const *dObsSorted, uint32_t const *dObsSlot, uint32_t k, uint64_t *dRows, uint32_t *dFlag, void *stream) {
  uint64_t const need = (m + 255) / 256;
  dim3 const grid((uint32_t)(need < 65536 ? need : 65536)), block(256);
  for (int verify = 0; verify < 2; ++verify)
    hipLaunchKernelGGL(bfCondInvertPermKernel, grid, block, 0, (hipStream_t)stream, dPerm, m, dObsSorted, dObsSlot, k, dRows, dFlag, verify);
  return bfHipFail(hipGetLastError(), "permutation inverse launch");
}

// ---------------------------------------------------------------------------
// unit panel and pack
// ---------------------------------------------------------------------------
// V [m x p] is zero (the host clears it); column c gets its one at row rows[c].  rows[] were checked on the host (< m).
template <typename S>
__global__ void bfCondUnitKernel(S *V, uint64_t m, uint32_t p, uint64_t const *rows) {
  uint32_t const c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < p) { uint64_t const i = rows[c]; if (i < m) V[i * p + c] = (S)1; }
}

int bfdevCondUnitPanel(void *V, uint64_t m, uint32_t p, uint64_t const *dRows, uint32_t dtype, void *stream) {
  if (!p) return 0;
  if (dtype == BFHIP_F64) hipLaunchKernelGGL(bfCondUnitKernel<double>, dim3((p + 63) / 64), dim3(64), 0, (hipStream_t)stream, (double *)V, m, p, dRows);
  else if (dtype == BFHIP_F32) hipLaunchKernelGGL(bfCondUnitKernel<float>, dim3((p + 63) / 64), dim3(64), 0, (hipStream_t)stream, (float *)V, m, p, dRows);
  else return bfhipFail(BFABI_ERROR_TYPE_ERROR, "unit panel: real element types only");
  return bfHipFail(hipGetLastError(), "unit panel launch");
}

// Bt[j, c0 + c] = double(T[j, c]) * double(gamma[j]) for the adjoint panel T [n x p]: both factors widened exactly, one
// rounding in double.  One thread per element, consecutive threads on consecutive c.
template <typename S>
__global__ __launch_bounds__(256) void bfCondPackKernel(double *Bt, uint64_t n, uint32_t k, uint32_t c0, S const *T, uint32_t p, S const *gamma) {
  uint64_t const total = n * p;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
    uint64_t const j = e / p;
    uint32_t const c = (uint32_t)(e - j * p);
    double const g = gamma ? (double)gamma[j] : 1.0;
    Bt[j * k + c0 + c] = (double)T[e] * g;
  }
}

int bfdevCondPack(double *Bt, uint64_t n, uint32_t k, uint32_t c0, void const *T, uint32_t p, void const *gamma, uint32_t dtype, void *stream) {
  if (!n || !p) return 0;
  uint64_t const need = (n * p + 255) / 256;
  dim3 const grid((uint32_t)(need < 65536 ? need : 65536)), block(256);
  if (dtype == BFHIP_F64) hipLaunchKernelGGL(bfCondPackKernel<double>, grid, block, 0, (hipStream_t)stream, Bt, n, k, c0, (double const *)T, p, (double const *)gamma);
  else if (dtype == BFHIP_F32) hipLaunchKernelGGL(bfCondPackKernel<float>, grid, block, 0, (hipStream_t)stream, Bt, n, k, c0, (float const *)T, p, (float const *)gamma);
  else return bfhipFail(BFABI_ERROR_TYPE_ERROR, "pack: real element types only");
  return bfHipFail(hipGetLastError(), "pack launch");
}

// ---------------------------------------------------------------------------
// Gram: G[a, b] = sum_j Bt[j, a] Bt[j, b] + (a == b ? D[a] : 0), lower triangle
// ---------------------------------------------------------------------------
// A workgroup owns a tile of G and walks all of n: chunk by chunk (BF_COND_CHUNK rows of Bt), one partial per chunk formed
// from zero, the partials added in chunk order.  The order of every sum depends on (n, k) alone.  Tiles that lie wholly
// above the diagonal are skipped, elements above it are not written (the host cleared G).
__global__ __launch_bounds__(256) void bfCondGramKernel(double *G, double const *Bt, uint64_t n, uint32_t k, double const *noiseVar) {
  BF_COND_TILE_LDS;
  uint64_t const i0 = (uint64_t)blockIdx.x * BF_COND_TI, s0 = (uint64_t)blockIdx.y * BF_COND_TS;
  if (s0 > i0 + BF_COND_TI - 1) return;
  double tot[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  for (uint64_t j0 = 0; j0 < n; j0 += BF_COND_CHUNK) {
    double acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    uint64_t const j1 = j0 + BF_COND_CHUNK < n ? j0 + BF_COND_CHUNK : n;
    bfCondTileAcc<double>(acc, Bt, 1, k, k, i0, Bt, k, 1, k, s0, j0, j1, sa, sb);
    for (uint32_t u = 0; u < 2; ++u) for (uint32_t v = 0; v < 4; ++v) tot[u][v] += acc[u][v];
  }
  BF_COND_FOR_OWNED(i, s) {
    if (i < k && s <= i) G[i * k + s] = i == s ? tot[u][v] + (noiseVar ? noiseVar[i] : 0.0) : tot[u][v];
  }
}

int bfdevCondGram(double *G, double const *Bt, uint64_t n, uint32_t k, double const *dNoiseVar, void *stream) {
  dim3 const grid((k + BF_COND_TI - 1) / BF_COND_TI, (k + BF_COND_TS - 1) / BF_COND_TS), block(256);
  hipLaunchKernelGGL(bfCondGramKernel, grid, block, 0, (hipStream_t)stream, G, Bt, n, k, dNoiseVar);
  return bfHipFail(hipGetLastError(), "Gram launch");
}

// ---------------------------------------------------------------------------
// C -= A B on tiles: the symmetric update of the factorization and the block updates of the triangular solves
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bfCondSubKernel(double *C, uint64_t ldc, double const *A, uint64_t sAi, uint64_t sAp, uint64_t M,
                                                       double const *B, uint64_t sBp, uint64_t sBs, uint64_t Nn, uint32_t P, int lowerOnly) {
  BF_COND_TILE_LDS;
  uint64_t const i0 = (uint64_t)blockIdx.x * BF_COND_TI, s0 = (uint64_t)blockIdx.y * BF_COND_TS;
  if (lowerOnly && s0 > i0 + BF_COND_TI - 1) return;
  double acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  bfCondTileAcc<double>(acc, A, sAi, sAp, M, i0, B, sBp, sBs, Nn, s0, 0, P, sa, sb);
  BF_COND_FOR_OWNED(i, s) {
    if (i < M && s < Nn && (!lowerOnly || s <= i)) C[i * ldc + s] -= acc[u][v];
  }
}

static int condSub(double *C, uint64_t ldc, double const *A, uint64_t sAi, uint64_t sAp, uint64_t M, double const *B, uint64_t sBp, uint64_t sBs,
                   uint64_t Nn, uint32_t P, int lowerOnly, hipStream_t s) {
  if (!M || !Nn || !P) return 0;
  dim3 const grid((uint32_t)((M + BF_COND_TI - 1) / BF_COND_TI), (uint32_t)((Nn + BF_COND_TS - 1) / BF_COND_TS)), block(256);
  hipLaunchKernelGGL(bfCondSubKernel, grid, block, 0, s, C, ldc, A, sAi, sAp, M, B, sBp, sBs, Nn, P, lowerOnly);
  return bfHipFail(hipGetLastError(), "block update launch");
}

// ---------------------------------------------------------------------------
// Cholesky, blocked (BF_COND_NB): diagonal tile, panel below it, symmetric update of the rest
// ---------------------------------------------------------------------------
// The diagonal tile of `nb` <= 32 rows at j0, in LDS, by one workgroup; right-looking, so element (r, c) loses its
// products in increasing column order.  A pivot (the value under the root) that is <= 0 or not finite records its step
// j0 + c in stat->failStep, once (the first one stays); the arithmetic goes on (NaN from there on, no index depends on data).
__global__ __launch_bounds__(256) void bfCondCholDiagKernel(double *G, uint32_t k, uint32_t j0, uint32_t nb, BfCondStat *stat) {
  __shared__ double t[BF_COND_NB][BF_COND_NB + 1];
  uint32_t const tid = threadIdx.x;
  for (uint32_t e = tid; e < BF_COND_NB * BF_COND_NB; e += 256) {
    uint32_t const r = e >> 5, c = e & 31;
    t[r][c] = (r < nb && c <= r) ? G[(uint64_t)(j0 + r) * k + j0 + c] : 0.0;
  }
  __syncthreads();
  double lo = INFINITY, hi = -INFINITY;
  uint32_t fail = 0xffffffffu;
  for (uint32_t c = 0; c < nb; ++c) {
    if (tid == 0) {
      double const d = t[c][c];
      if (d > 0.0 && isfinite(d)) { lo = fmin(lo, d); hi = fmax(hi, d); }
      else if (fail == 0xffffffffu) fail = j0 + c;
      t[c][c] = sqrt(d);
    }
    __syncthreads();
    double const piv = t[c][c];
    if (tid > c && tid < nb) t[tid][c] /= piv;
    __syncthreads();
    for (uint32_t e = tid; e < BF_COND_NB * BF_COND_NB; e += 256) {
      uint32_t const r = e >> 5, cc = e & 31;
      if (r < nb && cc > c && cc <= r) t[r][cc] = fma(-t[r][c], t[cc][c], t[r][cc]);
    }
    __syncthreads();
  }
  for (uint32_t e = tid; e < BF_COND_NB * BF_COND_NB; e += 256) {
    uint32_t const r = e >> 5, c = e & 31;
    if (r < nb && c < nb) G[(uint64_t)(j0 + r) * k + j0 + c] = c <= r ? t[r][c] : 0.0;
  }
  if (tid == 0) {
    if (fail != 0xffffffffu && stat->failStep == 0xffffffffu) stat->failStep = fail;
    if (lo < stat->minPivot) stat->minPivot = lo;
    if (hi > stat->maxPivot) stat->maxPivot = hi;
  }
}

// the tile of L at (j0, j0) into LDS (identity beyond nb: never read)
__device__ __forceinline__ void bfCondLoadDiag(double (*t)[BF_COND_NB + 1], double const *L, uint32_t k, uint32_t j0, uint32_t nb) {
  for (uint32_t e = threadIdx.x; e < BF_COND_NB * BF_COND_NB; e += blockDim.x) {
    uint32_t const r = e >> 5, c = e & 31;
    t[r][c] = (r < nb && c <= r) ? L[(uint64_t)(j0 + r) * k + j0 + c] : (r == c ? 1.0 : 0.0);
  }
  __syncthreads();
}

// x L11^T = a for the rows below the diagonal tile: a thread owns a row; its unknowns live in a column of LDS that no
// other thread touches (xs[c][thread]: conflict-free), eliminated right-looking, so unknown d loses its products in
// increasing c.
#define BF_COND_PANEL_ROWS 128u
__global__ __launch_bounds__(BF_COND_PANEL_ROWS) void bfCondCholPanelKernel(double *G, uint32_t k, uint32_t j0, uint32_t nb) {
  __shared__ double t[BF_COND_NB][BF_COND_NB + 1];
  __shared__ double xs[BF_COND_NB][BF_COND_PANEL_ROWS];
  bfCondLoadDiag(t, G, k, j0, nb);
  uint32_t const l = threadIdx.x;
  uint64_t const i = (uint64_t)j0 + nb + (uint64_t)blockIdx.x * BF_COND_PANEL_ROWS + l;
  if (i >= k) return;
  double *row = G + i * k + j0;
  for (uint32_t c = 0; c < nb; ++c) xs[c][l] = row[c];
  for (uint32_t c = 0; c < nb; ++c) {
    double const xc = xs[c][l] / t[c][c];
    row[c] = xc;
    for (uint32_t d = c + 1; d < nb; ++d) xs[d][l] = fma(-xc, t[d][c], xs[d][l]);
  }
}

int bfdevCondCholesky(double *G, uint32_t k, BfCondStat *dStat, void *stream) {
  hipStream_t const s = (hipStream_t)stream;
  for (uint32_t j0 = 0; j0 < k; j0 += BF_COND_NB) {
    uint32_t const nb = k - j0 < BF_COND_NB ? k - j0 : BF_COND_NB, r0 = j0 + nb, below = k - r0;
    hipLaunchKernelGGL(bfCondCholDiagKernel, dim3(1), dim3(256), 0, s, G, k, j0, nb, dStat);
    if (!below) break;
    hipLaunchKernelGGL(bfCondCholPanelKernel, dim3((below + BF_COND_PANEL_ROWS - 1) / BF_COND_PANEL_ROWS), dim3(BF_COND_PANEL_ROWS), 0, s, G, k, j0, nb);
    // A22 -= L21 L21^T, lower triangle: A(i, p) = L[r0 + i, j0 + p], B(p, c) = L[r0 + c, j0 + p]
    double *panel = G + (uint64_t)r0 * k + j0;
    int const rc = condSub(G + (uint64_t)r0 * k + r0, k, panel, k, 1, below, panel, 1, k, below, nb, 1, s);
    if (rc) return rc;
  }
  return bfHipFail(hipGetLastError(), "Cholesky launch");
}

// ---------------------------------------------------------------------------
// triangular solves on R [k x b], b <= 64: L then L^T, block by block
// ---------------------------------------------------------------------------
// The diagonal tile: thread s owns column s of the block's rows; its unknowns live in a column of LDS of its own
// (xs[c][s]), eliminated right-looking (a column of L is read when its unknown is known).  Forward: unknown c loses the
// products with unknowns 0 .. c - 1 in that order; backward (L^T): with unknowns nb - 1 .. c + 1 in that order.
template <bool TRANS>
__global__ __launch_bounds__(64) void bfCondSolveDiagKernel(double const *L, uint32_t k, uint32_t j0, uint32_t nb, double *R, uint32_t b) {
  __shared__ double t[BF_COND_NB][BF_COND_NB + 1];
  __shared__ double xs[BF_COND_NB][64];
  bfCondLoadDiag(t, L, k, j0, nb);
  uint32_t const s = threadIdx.x;
  if (s >= b) return;
  double *col = R + (uint64_t)j0 * b + s;
  for (uint32_t c = 0; c < nb; ++c) xs[c][s] = col[(uint64_t)c * b];
  if (!TRANS) {
    for (uint32_t c = 0; c < nb; ++c) {
      double const xc = xs[c][s] / t[c][c];
      col[(uint64_t)c * b] = xc;
      for (uint32_t d = c + 1; d < nb; ++d) xs[d][s] = fma(-t[d][c], xc, xs[d][s]);
    }
  } else {
    for (uint32_t c = nb; c-- > 0;) {
      double const xc = xs[c][s] / t[c][c];
      col[(uint64_t)c * b] = xc;
      for (uint32_t d = c; d-- > 0;) xs[d][s] = fma(-t[c][d], xc, xs[d][s]);
    }
  }
}

int bfdevCondSolve(double const *L, uint32_t k, double *R, uint32_t b, void *stream) {
  hipStream_t const s = (hipStream_t)stream;
  int rc;
  if (!b || b > 64) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "triangular solve: 1 .. 64 columns a pass");
  uint32_t const last = (k - 1) / BF_COND_NB * BF_COND_NB;
  for (uint32_t j0 = 0; j0 < k; j0 += BF_COND_NB) {                    // L x = r
    uint32_t const nb = k - j0 < BF_COND_NB ? k - j0 : BF_COND_NB, r0 = j0 + nb;
    hipLaunchKernelGGL(bfCondSolveDiagKernel<false>, dim3(1), dim3(64), 0, s, L, k, j0, nb, R, b);
    // rows below: R[r0 + i, :] -= sum_p L[r0 + i, j0 + p] X[j0 + p, :]
    if ((rc = condSub(R + (uint64_t)r0 * b, b, L + (uint64_t)r0 * k + j0, k, 1, k - r0, R + (uint64_t)j0 * b, b, 1, b, nb, 0, s))) return rc;
  }
  for (uint32_t j0 = last;; j0 -= BF_COND_NB) {                        // L^T alpha = x
    uint32_t const nb = k - j0 < BF_COND_NB ? k - j0 : BF_COND_NB;
    hipLaunchKernelGGL(bfCondSolveDiagKernel<true>, dim3(1), dim3(64), 0, s, L, k, j0, nb, R, b);
    // rows above: R[i, :] -= sum_p L[j0 + p, i] X[j0 + p, :]
    if ((rc = condSub(R, b, L + (uint64_t)j0 * k, 1, k, j0, R + (uint64_t)j0 * b, b, 1, b, nb, 0, s))) return rc;
    if (!j0) break;
  }
  return bfHipFail(hipGetLastError(), "triangular solve launch");
}

// ---------------------------------------------------------------------------
// contraction 1: R = y 1^T - Bt^T W - E
// ---------------------------------------------------------------------------
// part[c][a, s] = sum over the rows j of chunk c of Bt[j, a] W[j, s] (from zero, increasing j); then one thread per (a, s)
// adds the partials in chunk order and forms (y[a] - sum) - E[a, s].  W == NULL stands for zeros (the mean): no partials
// are formed and the sum is +0.  W has leading dimension ldw (a pass of a wider block), so has E.
template <typename S>
__global__ __launch_bounds__(256) void bfCondResidualPartKernel(double *part, double const *Bt, uint64_t n, uint32_t k, S const *W, uint64_t ldw, uint32_t b) {
  BF_COND_TILE_LDS;
  uint64_t const i0 = (uint64_t)blockIdx.x * BF_COND_TI, s0 = (uint64_t)blockIdx.y * BF_COND_TS;
  uint64_t const j0 = (uint64_t)blockIdx.z * BF_COND_CHUNK, j1 = j0 + BF_COND_CHUNK < n ? j0 + BF_COND_CHUNK : n;
  double acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  bfCondTileAcc<S>(acc, Bt, 1, k, k, i0, W, ldw, 1, b, s0, j0, j1, sa, sb);
  double *out = part + (uint64_t)blockIdx.z * k * b;
  BF_COND_FOR_OWNED(i, s) {
    if (i < k && s < b) out[i * b + s] = acc[u][v];
  }
}

__global__ __launch_bounds__(256) void bfCondResidualKernel(double *R, double const *part, uint32_t numChunks, uint32_t k, uint32_t b, double const *y,
                                                            double const *E, uint64_t lde) {
  uint64_t const e = (uint64_t)blockIdx.x * 256 + threadIdx.x, total = (uint64_t)k * b;
  if (e >= total) return;
  uint64_t const a = e / b, s = e - a * b;
  double sum = 0.0;
  for (uint32_t c = 0; c < numChunks; ++c) sum += part[(uint64_t)c * total + e];
  double r = y[a] - sum;
  if (E) r -= E[a * lde + s];
  R[e] = r;
}

int bfdevCondResidual(double *R, double *part, double const *Bt, uint64_t n, uint32_t k, double const *dY, void const *W, uint64_t ldw, uint32_t dtype,
                      double const *E, uint64_t lde, uint32_t b, void *stream) {
  hipStream_t const s = (hipStream_t)stream;
  if (!b || b > 64) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "residual: 1 .. 64 columns a pass");
  uint64_t const chunks = W ? (n + BF_COND_CHUNK - 1) / BF_COND_CHUNK : 0;
  if (chunks > 65535) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "conditioning: more than 65535 chunks of %u columns", BF_COND_CHUNK);
  if (chunks) {
    dim3 const grid((k + BF_COND_TI - 1) / BF_COND_TI, (b + BF_COND_TS - 1) / BF_COND_TS, (uint32_t)chunks), block(256);
    if (dtype == BFHIP_F64) hipLaunchKernelGGL(bfCondResidualPartKernel<double>, grid, block, 0, s, part, Bt, n, k, (double const *)W, ldw, b);
    else if (dtype == BFHIP_F32) hipLaunchKernelGGL(bfCondResidualPartKernel<float>, grid, block, 0, s, part, Bt, n, k, (float const *)W, ldw, b);
    else return bfhipFail(BFABI_ERROR_TYPE_ERROR, "residual: real element types only");
  }
  hipLaunchKernelGGL(bfCondResidualKernel, dim3((uint32_t)(((uint64_t)k * b + 255) / 256)), dim3(256), 0, s, R, part, (uint32_t)chunks, k, b, dY, E, lde);
  return bfHipFail(hipGetLastError(), "residual launch");
}

// ---------------------------------------------------------------------------
// contraction 2: W' = W + Bt alpha, rounded once to S
// ---------------------------------------------------------------------------
// One owner per element: sum_a Bt[j, a] alpha[a, s] from zero in increasing a, in double; then W[j, s] (widened) is added
// and the result rounded to S.  Wout is packed at b columns (the block sample starts from it), W has leading dimension ldw.
template <typename S>
__global__ __launch_bounds__(256) void bfCondUpdateKernel(S *Wout, double const *Bt, uint64_t n, uint32_t k, double const *alpha, S const *W, uint64_t ldw, uint32_t b) {
  BF_COND_TILE_LDS;
  uint64_t const i0 = (uint64_t)blockIdx.x * BF_COND_TI, s0 = (uint64_t)blockIdx.y * BF_COND_TS;
  double acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  bfCondTileAcc<double>(acc, Bt, k, 1, n, i0, alpha, b, 1, b, s0, 0, k, sa, sb);
  BF_COND_FOR_OWNED(i, s) {
    if (i < n && s < b) Wout[i * b + s] = (S)((W ? (double)W[i * ldw + s] : 0.0) + acc[u][v]);
  }
}

int bfdevCondUpdate(void *Wout, double const *Bt, uint64_t n, uint32_t k, double const *alpha, void const *W, uint64_t ldw, uint32_t dtype, uint32_t b, void *stream) {
  hipStream_t const s = (hipStream_t)stream;
  if (!b || b > 64) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "update: 1 .. 64 columns a pass");
  uint64_t const tiles = (n + BF_COND_TI - 1) / BF_COND_TI;
  if (tiles > 0x7fffffffu) return bfhipFail(BFABI_ERROR_INVALID_ARGUMENTS, "conditioning: too many columns");
  dim3 const grid((uint32_t)tiles, (b + BF_COND_TS - 1) / BF_COND_TS), block(256);
  if (dtype == BFHIP_F64) hipLaunchKernelGGL(bfCondUpdateKernel<double>, grid, block, 0, s, (double *)Wout, Bt, n, k, alpha, (double const *)W, ldw, b);
  else if (dtype == BFHIP_F32) hipLaunchKernelGGL(bfCondUpdateKernel<float>, grid, block, 0, s, (float *)Wout, Bt, n, k, alpha, (float const *)W, ldw, b);
  else return bfhipFail(BFABI_ERROR_TYPE_ERROR, "update: real element types only");
  return bfHipFail(hipGetLastError(), "update launch");
}
