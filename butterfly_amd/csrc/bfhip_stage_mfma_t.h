// bfhip_stage_mfma_t.h -- transposed (shared-leaf adjoint) stage kernel for blocks of right-hand sides, all four element types:
// the items and pieces of the transposed plan exactly as bfStageKernelT reads them (an item = mr <= 64 columns of A, a piece = a
// forward piece read with lanes on its columns), contracted on the FP64 matrix cores (v_mfma_f64_16x16x4_f64).  Every leaf element
// is loaded ONCE per pass of up to 64 right-hand sides; bfStageBodyT walks the whole item once per right-hand side.  Opt-in per
// operator (bfhipSetAdjointRhsBlocks).  Included by bfhip_device.hip only, after bfhip_stage_mfma_real.h.
//
// One wavefront per item, narrow, wide and formerly shared (coop) items alike; the four wavefronts of a workgroup take four list
// neighbours and never split an item.  A pass = MS <= 2 slabs of 16 columns of A x NT <= 4 tiles of 16 right-hand sides, over
// all pieces of the item; an item of more than 32 columns takes two passes, each over its own columns of every piece, so a pass
// reads each leaf element it covers once (x is read once per pass: it is the re-read, cached operand).
//
// Fragment maps (cdna_hip_programming.md section 3; as in bfhip_stage_mfma_c64.h) with A^T as the A operand: lane l = (i = l & 15,
// k = l >> 4) holds column c0 + 16 m + i of A at the lane's step, B is X[step][rhs j = l & 15], D register v of lane l =
// (column 4 v + (l >> 4), rhs l & 15).  The step index is affine inside a piece, so there is no table and no LDS: which steps a
// lane takes within a k-group is free as long as both fragments agree.
//   * a k-group is 4 EPL steps and EPL MFMAs per (slab, tile); MFMA e contracts slot e of the four k, and the x fragment of a
//     slot is the input row of its step;
//   * column-major pieces (element (step s, column j) at dataOff + j ld + s): lane k takes the 16-byte unit 4 g + k of its column
//     (steps (4 g + k) EPL + e: ONE load per slab);
//   * ROWMAJOR pieces (real family; element (s, j) at dataOff + s ld + j, at most 2 EPL steps: one group): slot e of lane k is
//     step 4 e + k: element loads, 16 consecutive columns per k; slots past the piece cost MFMAs on zeros;
//   * identity pieces add input rows inOff + column at the store, in double, before the one rounding.
// Element types: F32 and complex64 fragments are widened exactly (v_cvt_f64_f32), everything accumulates in double and is rounded
// once to the storage type at the store.  Complex products take the four-real-product form with two accumulator sets (Re += Ar Xr,
// Re += (-Ai) Xi, Im += Ar Xi, Im += Ai Xr), so results are componentwise what zgemm gives; BFHIP_FLAG_EXACT_COMPLEX changes nothing.
//
// Padding never meets data.  A step past the piece's ncols: the unit / row index is clamped into the piece for the address and
// BOTH fragments are replaced by zeros before they are widened or multiplied.  Columns past mr and right-hand sides past nrhs are
// clamped copies of the last real one that are never stored; a column of the product depends on that column of A, a right-hand
// side on that column of X only.  Nothing is read outside the extents tests/plan_emulator.py asserts for transposed pieces: units
// of a column up to ceil(ncols / EPL), columns below mr.  One owner per output, no atomics: bit-identical from apply to apply.
//
// Budget (hipcc -Rpass-analysis=kernel-resource-usage, asserted by tests/test_adjoint_rhs_blocks_cpu.py): no LDS, no scratch, no
// spills.  Wavefronts per SIMD (amdgpu_waves_per_eu): the real types hold 16 MS NT <= 64 accumulator registers and are built for
// 4 (<= 128 VGPRs) at every tile count; the complex types hold twice that: 4 at 1 and 2 tiles, 2 (<= 256 VGPRs) at 4 tiles.
#ifndef BFHIP_STAGE_MFMA_T_H
#define BFHIP_STAGE_MFMA_T_H

#define BF_TM_WG_WAVES 4

template <typename S, int NC> struct __attribute__((aligned(sizeof(S) * NC))) BfTmElem { S v[NC]; };
// the fragments of one k-group as they come from memory: SUB steps per lane
template <typename S, int NC, int SUB, int NT, int MS> struct BfTmRaw { BfTmElem<S, NC> a[MS][SUB], x[NT][SUB]; };

// the piece as a pass sees it (wave-uniform: the bases live in scalar registers)
template <typename S> struct BfTmPiece {
  S const *a;           // element (step 0, column 0)
  S const *x;           // X[inOff][q0]
  uint32_t n, ld;       // steps, elements between columns (column-major) or between steps (ROWMAJOR)
};

// Group g of a piece = its steps [s0, s0 + 4 SUB), s0 = 4 g SUB.  Slot e of lane k holds step s0 + k SUB + e of a column-major
// piece (the lane's 16-byte unit: one load per slab) or step s0 + 4 e + k of a ROWMAJOR piece (element loads, 16 consecutive
// columns per k); MFMA e contracts slot e of all four k.  Both layouts fill the SAME fragment registers and feed the same MFMAs
// (two code paths through the accumulators cost a second copy of them in registers).  Returns the mask of slots whose step
// exists; the others were read at a clamped address inside the piece.  Every address is a wave-uniform 64-bit base (the piece's,
// advanced to s0) plus a 32-bit lane offset: below 64 columns x ld for the leaf, below 16 nrhs + 64 elements for x.
template <typename S, int NC, int SUB, int NT, int MS>
__device__ __forceinline__ uint32_t bfTmLoad(BfTmRaw<S, NC, SUB, NT, MS> &f, BfTmPiece<S> const &pc, bool rm, uint32_t g, uint32_t lk, uint32_t nrhs,
                                             uint32_t const (&acol)[MS], uint32_t const (&xq)[NT]) {
  using E = BfTmElem<S, NC>;
  constexpr uint32_t EB = sizeof(E);
  struct __attribute__((aligned(16))) U { E e[SUB]; };
  static_assert(sizeof(U) == 16, "one 16-byte unit per lane");
  uint32_t const s0 = 4u * g * SUB, left = pc.n - s0;  // >= 1
  char const *xb = (char const *)pc.x + (uint64_t)s0 * nrhs * EB;
  uint32_t mask = 0, rowc[SUB];
#pragma unroll
  for (int e = 0; e < SUB; ++e) {
    uint32_t const rel = rm ? 4u * e + lk : lk * SUB + e;
    mask |= rel < left ? 1u << e : 0u;
    rowc[e] = rel < left ? rel : left - 1u;
  }
  if (SUB > 1 && rm) {                                 // wave-uniform
    char const *ab = (char const *)pc.a + (uint64_t)s0 * pc.ld * EB;
#pragma unroll
    for (int m = 0; m < MS; ++m)
#pragma unroll
      for (int e = 0; e < SUB; ++e) f.a[m][e] = *(E const *)(ab + (rowc[e] * pc.ld + acol[m]) * EB);
  } else {
    uint32_t const unitsLeft = (left + SUB - 1u) / SUB, urel = lk < unitsLeft ? lk : unitsLeft - 1u;
    char const *ab = (char const *)pc.a + (uint64_t)s0 * EB;
#pragma unroll
    for (int m = 0; m < MS; ++m) {
      U const v = *(U const *)(ab + (acol[m] * pc.ld + urel * SUB) * EB);
#pragma unroll
      for (int e = 0; e < SUB; ++e) f.a[m][e] = v.e[e];
    }
  }
#pragma unroll
  for (int e = 0; e < SUB; ++e)
#pragma unroll
    for (int t = 0; t < NT; ++t) f.x[t][e] = *(E const *)(xb + (rowc[e] * nrhs + xq[t]) * EB);
  return mask;
}

// the MFMAs of one k-group: SUB k-steps; a lane whose step lies past the piece contributes zeros on both sides
template <typename S, int NC, int SUB, int NT, int MS>
__device__ __forceinline__ void bfTmStep(bf_d4 (&acc)[NC][MS][NT], BfTmRaw<S, NC, SUB, NT, MS> const &f, uint32_t mask) {
#pragma unroll
  for (int e = 0; e < SUB; ++e) {
    bool const valid = (mask >> e) & 1u;
    double a[MS][NC];
#pragma unroll
    for (int m = 0; m < MS; ++m)
#pragma unroll
      for (int c = 0; c < NC; ++c) a[m][c] = (double)(valid ? f.a[m][e].v[c] : S(0));
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      double x[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) x[c] = (double)(valid ? f.x[t][e].v[c] : S(0));
#pragma unroll
      for (int m = 0; m < MS; ++m) {
        acc[0][m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m][0], x[0], acc[0][m][t], 0, 0, 0);
        if constexpr (NC == 2) {
          acc[0][m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[m][1], x[1], acc[0][m][t], 0, 0, 0);
          acc[1][m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m][0], x[1], acc[1][m][t], 0, 0, 0);
          acc[1][m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m][1], x[0], acc[1][m][t], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);                 // one k-step's widened fragments live at a time
  }
}

// One dense piece, group by group.  The loads of a group (MS or MS SUB of the leaf, SUB NT of x) are in flight together; the
// latency between groups and between pieces is covered by the other wavefronts of the SIMD (a second register set for the next
// group's fragments was tried: it spilled in seven of the twelve instantiations).
template <typename S, int NC, int SUB, int NT, int MS>
__device__ __forceinline__ void bfTmPieceRun(bf_d4 (&acc)[NC][MS][NT], BfTmPiece<S> const &pc, bool rm, uint32_t nrhs, uint32_t lk,
                                             uint32_t const (&acol)[MS], uint32_t const (&xq)[NT]) {
  uint32_t const ngroups = (pc.n + 4u * SUB - 1u) / (4u * SUB);      // wave-uniform
#pragma unroll 1
  for (uint32_t g = 0; g < ngroups; ++g) {
    BfTmRaw<S, NC, SUB, NT, MS> f;
    uint32_t const mask = bfTmLoad<S, NC, SUB, NT, MS>(f, pc, rm, g, lk, nrhs, acol, xq);
    bfTmStep<S, NC, SUB, NT, MS>(acc, f, mask);
  }
}

// One pass = columns [c0, c0 + 16 MS) of the item x RHS [q0, q0 + 16 NT), over all its pieces.
template <int DT, int NT, int MS>
__device__ __forceinline__ void bfTmPass(StageParams const &p, BfDevItem const &it, uint32_t mr, uint32_t c0, uint32_t q0, int lane) {
  using S = typename Traits<DT>::S;
  constexpr int EPL = Traits<DT>::EPL;
  constexpr int NC = Traits<DT>::CPLX ? 2 : 1;
  using E = BfTmElem<S, NC>;
  uint32_t const nrhs = p.nrhs;
  uint32_t const li = lane & 15, lk = lane >> 4;
  uint32_t const qleft = nrhs - q0;                    // >= 1
  bf_d4 acc[NC][MS][NT];                               // real: the sums; complex: Re, Im
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int m = 0; m < MS; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[c][m][t] = (bf_d4){0, 0, 0, 0};
  // columns past the item's end / right-hand sides past nrhs: copies of the last real one, never stored
  uint32_t acol[MS], xq[NT];
#pragma unroll
  for (int m = 0; m < MS; ++m) { uint32_t const c = c0 + 16u * m + li; acol[m] = c < mr ? c : mr - 1u; }
#pragma unroll
  for (int t = 0; t < NT; ++t) { uint32_t const q = 16u * t + li; xq[t] = q < qleft ? q : qleft - 1u; }
  bool hasIdentity = false;
  uint32_t const np = it.numPieces;
  for (uint32_t wbase = 0; wbase < np; wbase += 64u) {
    uint32_t const wn = np - wbase < 64u ? np - wbase : 64u;
    BfPieceWin const win = bfPieceWinLoad(p.pieces + it.pieceBegin + wbase, wn, lane);
    for (uint32_t pi = 0; pi < wn; ++pi) {
      BfDevPiece const d = bfPieceWinGet(win, pi);
      if (d.flags & BF_PIECE_IDENTITY) { hasIdentity = true; continue; }
      if (!d.ncols) continue;
      BfTmPiece<S> pc;
      pc.a = (S const *)p.arena + d.dataOff * NC;
      pc.x = ((d.flags & BF_PIECE_IN_X) ? (S const *)p.x : (S const *)p.temp) + ((uint64_t)d.inOff * nrhs + q0) * NC;
      pc.n = d.ncols;
      pc.ld = d.ld;
      bfTmPieceRun<S, NC, EPL, NT, MS>(acc, pc, EPL > 1 && (d.flags & BF_PIECE_ROWMAJOR) != 0, nrhs, lk, acol, xq);
    }
  }
  // ---- the pass's columns x right-hand sides out of the accumulators, rounded to the element type once
  E *out = (it.mrFlags & BF_ITEM_OUT_Y) ? (E *)p.y : (E *)p.temp;
  // (the lane's coordinates are derived again from an opaque copy: the store addresses are not carried through the piece loop)
  uint32_t lane2 = (uint32_t)lane;
  asm volatile("" : "+v"(lane2));
  uint32_t const li2 = lane2 & 15u, lk2 = lane2 >> 4;
#pragma unroll
  for (int m = 0; m < MS; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        uint32_t const col = c0 + 16u * m + 4u * v + lk2, q = 16u * t + li2;
        if (col < mr && q < qleft) {
          double sum[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c) sum[c] = acc[c][m][t][v];
          if (hasIdentity) {
            for (uint32_t k = 0; k < np; ++k) {
              BfDevPiece const d = p.pieces[it.pieceBegin + k];
              if (!(d.flags & BF_PIECE_IDENTITY)) continue;
              E const *xin = (d.flags & BF_PIECE_IN_X) ? (E const *)p.x : (E const *)p.temp;
              E const xv = xin[((uint64_t)d.inOff + col) * nrhs + q0 + q];
#pragma unroll
              for (int c = 0; c < NC; ++c) sum[c] += (double)xv.v[c];
            }
          }
          E r;
#pragma unroll
          for (int c = 0; c < NC; ++c) r.v[c] = (S)sum[c];
          out[((uint64_t)it.outOff + col) * nrhs + q0 + q] = r;
        }
      }
}

template <int DT, int MS, int MAXNT>
__device__ __forceinline__ void bfTmDispatch(uint32_t nt, StageParams const &p, BfDevItem const &it, uint32_t mr, uint32_t c0, uint32_t q0, int lane) {
  if (MAXNT >= 4 && nt == 4) bfTmPass<DT, 4, MS>(p, it, mr, c0, q0, lane);
  else if (MAXNT >= 3 && nt == 3) bfTmPass<DT, 3, MS>(p, it, mr, c0, q0, lane);
  else if (MAXNT >= 2 && nt == 2) bfTmPass<DT, 2, MS>(p, it, mr, c0, q0, lane);
  else bfTmPass<DT, 1, MS>(p, it, mr, c0, q0, lane);
}

// DT = any element type; MAXNT = the widest pass the launch needs (RHS tiles of 16: 1, 2 or 4); WAVES = wavefronts per SIMD the
// instantiation is built for (see the budget above).
template <int DT, int MAXNT, int WAVES>
__global__ __launch_bounds__(BF_TM_WG_WAVES * 64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void bfStageKernelTMfma(StageParams p) {
  int const wave = threadIdx.x >> 6;
  int const lane = threadIdx.x & 63;
  uint32_t const item = __builtin_amdgcn_readfirstlane(blockIdx.x * BF_TM_WG_WAVES + wave);
  if (item >= p.numItems) return;
  BfDevItem const it = p.items[item];
  uint32_t const mr = it.mrFlags & 0xffffu;
  uint32_t const nrhs = p.nrhs;
  for (uint32_t q0 = 0; q0 < nrhs; q0 += 64) {
    uint32_t const nt = (nrhs - q0 >= 64) ? 4u : (nrhs - q0 + 15u) / 16u;
    uint32_t c0 = 0;
    while (c0 < mr) {
      if (mr - c0 > 16) { bfTmDispatch<DT, 2, MAXNT>(nt, p, it, mr, c0, q0, lane); c0 += 32; }
      else { bfTmDispatch<DT, 1, MAXNT>(nt, p, it, mr, c0, q0, lane); c0 += 16; }
    }
  }
}
#endif
