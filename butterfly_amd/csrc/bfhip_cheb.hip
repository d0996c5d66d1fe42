// bfhip_cheb.hip -- the one kernel of the matrix-free Chebyshev covariance (bfhipChebCov*, include/bfhip.h; host side:
// bfhip_cheb.c).  Not a stage kernel: there is no plan and no arena, the operator is a CSR matrix S in HBM and the
// vectors are row-major n x q blocks of doubles, densely packed.
//
// One launch is one degree of Clenshaw's recurrence for all q columns:
//   out[i, :] = ck * (wScale ? wScale[i] : 1) * w[i, :] + alpha * sum_j S[i][j] * b1[col_j, :] + beta * b1[i, :] - b2[i, :]
// (then * outScale[i] at the last step).  The gather needs every row of b1, hence one launch per degree; w and b2 are
// streamed, out is written over b2.  Per degree the kernel moves three block streams (w, b2, out), the matrix once and
// the gathered rows of b1 (about 7 per row on a triangle mesh, found in L2 when the mesh is ordered with any locality).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bfhip_internal.h"
#include "../../include/bfhip_abi.h"
#include "bfhip_hip.h"
#include "bfhip_cheb_gather.h"          // BF_CHEB_GATHERS and the row gather (shared with bfhip_eigs.hip)

#define BF_CHEB_MAX_GRID (1u << 20)     // workgroups per launch; the rest is walked with a grid stride

// Threads: lanes = min(64, next power of two >= q) neighbouring lanes own row i, so a wavefront covers 64 / lanes rows and
// a workgroup of 256 covers 256 / lanes.  A lane owns columns lane, lane + lanes, ... : at q <= 64 one column, beyond
// that one column of every panel of 64; at q = 64 a wavefront reads a gathered row as one contiguous 512-byte request.
//
// The sum of a row runs over its nonzeros in CSR order by fma, in groups of BF_CHEB_GATHERS whose gathers are all issued
// before the first is used; the rest of the step is the same sequence for every q -- column j of a result does not
// depend on q, on the panel or on the launch.  One owner per output element and out == b2 only through the element's
// owner: no atomics, no LDS memory.  All indices are 64 bits.
//
// The (col, value) pairs of a group are loaded once per row: lane t of the row's lanes loads pair t (two vector memory
// instructions instead of 2 x BF_CHEB_GATHERS; a lane past the row's end re-reads its last pair, so every load stays
// inside the row) and every lane reads pair t from lane t by a shuffle.  Measured at q = 64 on a mesh of 7 nonzeros per
// row: with every lane loading the pairs for itself a row costs 30 vector memory instructions and
// the kernel moved 2.5 TB/s of algorithmic bytes, with 4 or with 8 gathers in flight; with 16 instructions per row 3.0.
// Rows owned by fewer lanes than a group has pairs (q <= BF_CHEB_GATHERS / 2) load them per lane: there a wavefront
// covers 16 rows or more and the instructions are shared by all of them.
__global__ __launch_bounds__(256) void bfChebStepKernel(BfChebStep a, uint32_t lanesLog2) {
  uint32_t const lanes = 1u << lanesLog2, lane = threadIdx.x & (lanes - 1), rowsPerWg = 256u >> lanesLog2;
  uint64_t const q = a.q;
  for (uint64_t i = (uint64_t)blockIdx.x * rowsPerWg + (threadIdx.x >> lanesLog2); i < a.n; i += (uint64_t)gridDim.x * rowsPerWg) {
    uint64_t const beg = a.rowptr[i], end = a.rowptr[i + 1];
    double const ws = a.wScale ? a.wScale[i] : 1.0, os = a.outScale ? a.outScale[i] : 1.0;
    // every lane of the row walks every panel (the shuffles below need them all); one past the block's width computes nothing
    for (uint64_t c0 = 0; c0 < q; c0 += lanes) {
      uint64_t const c = c0 + lane;
      bool const live = c < q;
      // the three streamed values first: their loads are in flight while the row's pairs and the gather arrive
      double r = 0, own = 0, old = 0;
      if (live) {
        r = a.w[i * q + c];
        if (a.b1) own = a.b1[i * q + c];
        if (a.b2) old = a.b2[i * q + c];
      }
      if (a.wScale) r *= ws;
      r *= a.ck;
      if (a.b1) {
        double const acc = bfChebRowGather(a.colind, a.val, beg, end, a.b1, q, c, lane, lanes, live);
        r = fma(a.alpha, acc, r);
        r = fma(a.beta, own, r);
      }
      if (a.b2) r -= old;
      if (a.outScale) r *= os;
      if (live) a.out[i * q + c] = r;
    }
  }
}

// The scaled unit panel of conditioning (bfhip_cheb.c: chebCondPanel): U [n x p] = D E for the p <= 64 vertices rows[0 .. p),
// cleared and filled in one launch.  One thread per element, consecutive threads on consecutive columns; every element
// is written by its owner alone (d[j] where j == rows[c], else 0), so repeated or out-of-range rows could not reach
// outside the block (the host refuses both before).
__global__ __launch_bounds__(256) void bfChebUnitPanelKernel(double *U, uint64_t n, uint32_t p, uint64_t const *rows, double const *d) {
  uint64_t const total = n * p;
  for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
    uint64_t const j = e / p;
    uint32_t const c = (uint32_t)(e - j * p);
    U[e] = rows[c] == j ? d[j] : 0.0;
  }
}

int bfdevChebUnitPanel(double *U, uint64_t n, uint32_t p, uint64_t const *dRows, double const *d, void *stream) {
  if (!n || !p) return 0;
  uint64_t const need = (n * p + 255) / 256;
  dim3 const grid((uint32_t)(need < 65536 ? need : 65536)), block(256);
  hipLaunchKernelGGL(bfChebUnitPanelKernel, grid, block, 0, (hipStream_t)stream, U, n, p, dRows, d);
  return bfHipFail(hipGetLastError(), "Chebyshev unit panel launch");
}

int bfdevChebStep(BfChebStep const *s, void *stream) {
  if (!s->n || !s->q) return 0;
  uint32_t lg = 0;
  while ((1u << lg) < s->q && lg < 6) ++lg;
  uint64_t const perWg = 256u >> lg, need = (s->n + perWg - 1) / perWg;
  dim3 const grid((uint32_t)(need < BF_CHEB_MAX_GRID ? need : BF_CHEB_MAX_GRID)), block(256);
  hipLaunchKernelGGL(bfChebStepKernel, grid, block, 0, (hipStream_t)stream, *s, lg);
  return bfHipFail(hipGetLastError(), "Chebyshev step launch");
}
