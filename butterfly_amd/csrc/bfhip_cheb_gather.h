// bfhip_cheb_gather.h -- the row gather shared by bfChebStepKernel (bfhip_cheb.hip), bfEigsStepKernel (bfhip_eigs.hip) and
// bfEigsMassStepKernel (bfhip_eigs_mass.hip, with the mass values in the place of S's):
// sum_j S[i][j] * b1[col_j, c] for one row i and one column c of a row-major block, the lane layout and the gather groups
// described at bfChebStepKernel.  Included by those three files only, after <hip/hip_runtime.h>.
#ifndef BFHIP_CHEB_GATHER_H
#define BFHIP_CHEB_GATHER_H

#include <stdint.h>

#ifndef BF_CHEB_GATHERS
#define BF_CHEB_GATHERS 8               // gathered rows in flight per output row, a power of two (tools/cheb_cov_rate.py)
#endif
static_assert(BF_CHEB_GATHERS >= 1 && BF_CHEB_GATHERS <= 64 && (BF_CHEB_GATHERS & (BF_CHEB_GATHERS - 1)) == 0, "BF_CHEB_GATHERS: a power of two <= 64");

// The nonzeros [beg, end) of the row in CSR order by fma, in groups of BF_CHEB_GATHERS whose gathers are all issued before
// the first is used.  `lanes` neighbouring lanes own the row and ALL of them call this together (the shuffles need them);
// a lane that is not `live` (its column is past the block's width) loads the pairs and gathers nothing.  `ld` is the
// block's row stride in doubles.  The sequence of operations per (row, column) does not depend on lanes, ld or the launch.
static __device__ __forceinline__ double bfChebRowGather(uint32_t const *colind, double const *val, uint64_t beg, uint64_t end,
                                                         double const *b1, uint64_t ld, uint64_t c, uint32_t lane, uint32_t lanes, bool live) {
  constexpr int G = BF_CHEB_GATHERS;
  bool const shared = lanes >= (uint32_t)G;
  double acc = 0;
  for (uint64_t j = beg; j < end; j += G) {
    double v[G];
    uint32_t col[G];
    if (shared) {
      uint64_t const mine = j + (lane & (G - 1)) < end ? j + (lane & (G - 1)) : end - 1;
      double const pv = val[mine];
      uint32_t const pc = colind[mine];
#pragma unroll
      for (int t = 0; t < G; ++t) {
        v[t] = __shfl(pv, t, (int)lanes);
        col[t] = __shfl(pc, t, (int)lanes);
      }
    } else {
#pragma unroll
      for (int t = 0; t < G; ++t) {
        uint64_t const jj = j + t < end ? j + t : end - 1;
        v[t] = val[jj];
        col[t] = colind[jj];
      }
    }
    if (live) {
      double x[G];
#pragma unroll
      for (int t = 0; t < G; ++t) x[t] = j + t < end ? b1[(uint64_t)col[t] * ld + c] : 0.0;
#pragma unroll
      for (int t = 0; t < G; ++t)
        if (j + t < end) acc = fma(v[t], x[t], acc);
    }
  }
  return acc;
}

#endif
