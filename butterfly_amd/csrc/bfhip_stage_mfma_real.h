// bfhip_stage_mfma_real.h -- forward stage kernel of the real element types (F64, F32) for blocks of right-hand sides: the items
// and packed pieces of the real family's plan exactly as bfStageKernelReal / bfStageKernelSmall read them, contracted on the FP64
// matrix cores (v_mfma_f64_16x16x4_f64).  Every leaf element is loaded ONCE per pass of up to 64 right-hand sides; the default
// kernels run the whole item once per right-hand side.  Opt-in per operator (bfhipSetRealRhsBlocks).  Included by bfhip_device.hip
// only, after bfhip_stage_mfma_c64.h, whose structure it follows and whose table (BfM64Tab), constants and invariants it shares:
// one wavefront per item, a per-segment LDS table with one entry per leaf column, a flat k-loop of 4 leaf columns per step, passes
// of MS <= 2 slabs of 16 rows x NT <= 4 tiles of 16 right-hand sides, two fragment register sets taken in turn.  The complex64
// kernel is not touched: nothing here is shared with it but the table type, the constants and bfPieceWin*.
//
// What differs from complex64: one scalar per fragment and ONE MFMA per (slab, tile) per k-step (no Gauss sums), one accumulator
// set (the 4-tile kernel holds 32 accumulator doubles, not 96).  The element size es is 8 (F64) or 4 (F32): the lane granule of
// the plan is EPL = 16 / es rows (mrPad = the item's rows padded to it), column-major pieces have row stride es and column stride
// mrPad es, ROWMAJOR pieces row stride ld es, x offsets are (row nrhs + q) es, and the 32-bit span limit counts bytes of es.
//   * F64: plain double fragments, no converts; products and sums in double as in the default kernels, in another order.
//   * F32: fragments are loaded as float, widened exactly (v_cvt_f64_f32), contracted in double and rounded to float ONCE at the
//     store.  The default F32 kernels accumulate in float; an item sum of the block path carries one rounding u32 plus K u64.
//     The fp32 matrix pipe is not used.
// Fragment maps (cdna_hip_programming.md section 3): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D reg v of lane l =
// D[i = 4 v + (l >> 4)][j = l & 15].
//
// Padding never meets data.  A lane of a k-step whose column lies past the end of the segment reads the table's padding (the
// segment's first leaf element, its first input row: addresses the item reads anyway) and BOTH its fragments are replaced by
// zeros before use: no zero is ever multiplied by a value of x.  Rows past the item's end and right-hand sides past nrhs are
// clamped to the last real row / column: those lanes compute copies that are never stored.  Identity pieces are added at the
// store, in double, before the one rounding; an item without dense pieces stores its identity terms, or zeros.  One owner per
// output, no atomics: results are bit-identical from one apply to the next.
//
// Budget (hipcc -Rpass-analysis=kernel-resource-usage, asserted by tests/test_real_rhs_blocks_cpu.py): no scratch, no spills.
// VGPRs of the 1 / 2 / 4-tile instantiations: F64 52 / 74 / 118, F32 50 / 70 / 112 -- all below the 128 of four wavefronts per
// SIMD.  WAVES = 4 for all six: the 9.2 KiB table of a one-wavefront workgroup lets 17 workgroups share a CU's 160 KiB of LDS, so
// a fifth wavefront per SIMD that the 1- and 2-tile register counts would allow has no table to work with.
#ifndef BFHIP_STAGE_MFMA_REAL_H
#define BFHIP_STAGE_MFMA_REAL_H

// the fragments of one k-step as they come from memory: one element per lane each
template <typename E, int NT, int MS> struct BfMRealRaw { E a[MS], x[NT]; };

template <typename E, int NT, int MS>
__device__ __forceinline__ void bfMRealLoad(BfMRealRaw<E, NT, MS> &f, BfM64Tab const *tab, uint32_t c, char const *abase, char const *xbase,
                                            uint32_t const (&arow)[MS], uint32_t const (&xoff)[NT]) {
  // (no branch: a column past the end reads the table's padding and bfMRealStep replaces both fragments by zeros)
  uint32_t const xo = tab->x[c], ao = tab->a[c], as = tab->s[c];
#pragma unroll
  for (int m = 0; m < MS; ++m) f.a[m] = __builtin_nontemporal_load((E const *)(abase + (ao + arow[m] * as)));      // the leaf stream: read once
#pragma unroll
  for (int t = 0; t < NT; ++t) f.x[t] = *(E const *)(xbase + (xo + xoff[t]));
}

// the MFMAs of one k-step: widen (exact; nothing to do for F64), MS NT matrix instructions
template <typename E, int NT, int MS>
__device__ __forceinline__ void bfMRealStep(bf_d4 (&acc)[MS][NT], BfMRealRaw<E, NT, MS> const &f, bool valid) {
  double a[MS];
#pragma unroll
  for (int m = 0; m < MS; ++m) a[m] = (double)(valid ? f.a[m] : E(0));
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    double const x = (double)(valid ? f.x[t] : E(0));
#pragma unroll
    for (int m = 0; m < MS; ++m) acc[m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], x, acc[m][t], 0, 0, 0);
  }
}

// One pass = rows [s0, s0 + 16 MS) x RHS [q0, q0 + 16 NT) of one item, over all its segments.
template <int DT, int NT, int MS>
__device__ __forceinline__ void bfMRealPass(StageParams const &p, BfDevItem const &it, uint32_t mr, uint32_t s0, uint32_t q0, BfM64Tab *tab, int lane) {
  using E = typename Traits<DT>::E;
  constexpr uint32_t ES = sizeof(E), EPL = Traits<DT>::EPL;
  uint32_t const nrhs = p.nrhs;
  uint32_t const li = lane & 15, lk = lane >> 4;
  uint32_t const mrPad = (mr + EPL - 1u) / EPL * EPL;
  uint32_t const qleft = nrhs - q0;                    // >= 1
  bf_d4 acc[MS][NT];
#pragma unroll
  for (int m = 0; m < MS; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[m][t] = (bf_d4){0, 0, 0, 0};
  // rows past the item's end / right-hand sides past nrhs: copies of the last real one, never stored
  uint32_t arow[MS], xoff[NT];
#pragma unroll
  for (int m = 0; m < MS; ++m) { uint32_t const r = s0 + 16u * m + li; arow[m] = r < mr ? r : mr - 1u; }
#pragma unroll
  for (int t = 0; t < NT; ++t) { uint32_t const q = 16u * t + li; xoff[t] = (q < qleft ? q : qleft - 1u) * ES; }
  bool hasIdentity = false;
  uint32_t const np = it.numPieces;
  uint32_t const spanRows = BF_M64_SPAN_BYTES / (nrhs * ES);     // >= 4096 > BF_M64_TABCAP: a table's worth of one piece always fits
  uint32_t pi = 0, pj = 0;                             // the next piece, and the first column of it that no segment has taken yet
  while (pi < np) {
    // ---- the next segment: its table into LDS, its extent into scalars (the descriptor window is loaded again for every
    // segment: six registers that must not stay live across the k-loop)
    uint32_t cols = 0, minRow = 0, maxRow = 0, inX = 0;
    uint64_t aBase = 0;
    bool started = false;
    BfPieceWin win;
    uint32_t wbase = 0xffffff00u;
    while (pi < np) {
      if (pi - wbase >= 64u) {
        wbase = pi;
        win = bfPieceWinLoad(p.pieces + it.pieceBegin + wbase, np - wbase < 64u ? np - wbase : 64u, lane);
      }
      BfDevPiece const pc = bfPieceWinGet(win, pi - wbase);
      if (pc.flags & BF_PIECE_IDENTITY) { hasIdentity = true; ++pi; pj = 0; continue; }
      uint32_t n = pc.ncols - pj;
      if (n > BF_M64_TABCAP - cols) n = BF_M64_TABCAP - cols;
      if (!n) break;                                   // the table is full
      bool const rm = (pc.flags & BF_PIECE_ROWMAJOR) != 0;
      uint32_t const px = pc.flags & BF_PIECE_IN_X, first = pc.inOff + pj, last = first + n - 1u;
      uint64_t const extent = rm ? (uint64_t)(mr - 1u) * pc.ld + pc.ncols : (uint64_t)mrPad * pc.ncols;      // elements of the whole piece
      uint32_t lo = first, hi = last;
      uint64_t rel = 0;
      if (started) {
        rel = pc.dataOff - aBase;                      // (wraps for a piece stored ahead of the segment's first: a new segment)
        if (px != inX || rel >= BF_M64_SPAN_BYTES / ES || rel + extent >= BF_M64_SPAN_BYTES / ES) break;
        lo = minRow < lo ? minRow : lo;
        hi = maxRow > hi ? maxRow : hi;
        if (hi - lo >= spanRows) break;
      } else {
        started = true;
        aBase = pc.dataOff;
        inX = px;
      }
      minRow = lo;
      maxRow = hi;
      uint32_t const colStride = rm ? ES : mrPad * ES, rowStride = rm ? pc.ld * ES : ES;
      uint32_t const a0 = (uint32_t)rel * ES + pj * colStride;
      for (uint32_t j = (uint32_t)lane; j < n; j += 64u) {
        tab->x[cols + j] = first + j;
        tab->a[cols + j] = a0 + j * colStride;
        tab->s[cols + j] = rowStride;
      }
      cols += n;
      pj += n;
      if (pj == pc.ncols) { ++pi; pj = 0; }
    }
    if (!cols) break;                                  // identity pieces only
    waveSync();
    // rows -> byte offsets from the segment's first row (fits 32 bits: spanRows)
    for (uint32_t j = (uint32_t)lane; j < cols; j += 64u) tab->x[j] = (tab->x[j] - minRow) * (nrhs * ES);
    // columns past the end, as far as the last k-step's requests reach: any address of the segment will do
    if ((uint32_t)lane < BF_M64_TABPAD) { tab->x[cols + lane] = 0; tab->a[cols + lane] = 0; tab->s[cols + lane] = 0; }
    waveSync();
    char const *abase = (char const *)p.arena + aBase * ES;
    char const *xbase = (inX ? (char const *)p.x : (char const *)p.temp) + ((uint64_t)minRow * nrhs + q0) * ES;
    uint32_t const ksteps = (cols + 3u) / 4u;
    // the k-loop: the fragments of k-step ks + 1 are requested before the MFMAs of k-step ks.  Two register sets taken in turn
    // and no copy between them; the scheduling barriers keep the requests ahead of the MFMAs they overlap.  An odd number of
    // k-steps ends with a k-step whose fragments are zeros.
    BfMRealRaw<E, NT, MS> f0, f1;
    uint32_t c = lk;
    bfMRealLoad<E, NT, MS>(f0, tab, c, abase, xbase, arow, xoff);
    for (uint32_t ks = 0; ks < ksteps; ks += 2) {
      __builtin_amdgcn_sched_barrier(0);
      bfMRealLoad<E, NT, MS>(f1, tab, c + 4u, abase, xbase, arow, xoff);
      __builtin_amdgcn_sched_barrier(0);
      bfMRealStep<E, NT, MS>(acc, f0, c < cols);
      __builtin_amdgcn_sched_barrier(0);
      bfMRealLoad<E, NT, MS>(f0, tab, c + 8u, abase, xbase, arow, xoff);
      __builtin_amdgcn_sched_barrier(0);
      bfMRealStep<E, NT, MS>(acc, f1, c + 4u < cols);
      c += 8u;
    }
    waveSync();                                        // the table is rewritten by the next segment
  }
  // ---- the pass's rows x right-hand sides out of the accumulators, rounded to the element type once
  E *out = (it.mrFlags & BF_ITEM_OUT_Y) ? (E *)p.y : (E *)p.temp;
  // (the lane's coordinates are derived again from an opaque copy: the store addresses are not carried through the k-loop)
  uint32_t lane2 = (uint32_t)lane;
  asm volatile("" : "+v"(lane2));
  uint32_t const li2 = lane2 & 15u, lk2 = lane2 >> 4;
#pragma unroll
  for (int m = 0; m < MS; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        uint32_t const row = s0 + 16u * m + 4u * v + lk2, q = 16u * t + li2;
        if (row < mr && q < qleft) {
          double sum = acc[m][t][v];
          if (hasIdentity) {
            for (uint32_t k = 0; k < np; ++k) {
              BfDevPiece const pc = p.pieces[it.pieceBegin + k];
              if (!(pc.flags & BF_PIECE_IDENTITY)) continue;
              E const *xin = (pc.flags & BF_PIECE_IN_X) ? (E const *)p.x : (E const *)p.temp;
              sum += (double)xin[((uint64_t)pc.inOff + row) * nrhs + q0 + q];
            }
          }
          out[((uint64_t)it.outOff + row) * nrhs + q0 + q] = (E)sum;
        }
      }
}

template <int DT, int MS, int MAXNT>
__device__ __forceinline__ void bfMRealDispatch(uint32_t nt, StageParams const &p, BfDevItem const &it, uint32_t mr, uint32_t s0, uint32_t q0, BfM64Tab *tab, int lane) {
  if (MAXNT >= 4 && nt == 4) bfMRealPass<DT, 4, MS>(p, it, mr, s0, q0, tab, lane);
  else if (MAXNT >= 3 && nt == 3) bfMRealPass<DT, 3, MS>(p, it, mr, s0, q0, tab, lane);
  else if (MAXNT >= 2 && nt == 2) bfMRealPass<DT, 2, MS>(p, it, mr, s0, q0, tab, lane);
  else bfMRealPass<DT, 1, MS>(p, it, mr, s0, q0, tab, lane);
}

// DT = BFHIP_F64 / BFHIP_F32; MAXNT = the widest pass the launch needs (RHS tiles of 16); WAVES = wavefronts per SIMD the
// instantiation is built for (see the budget above).
template <int DT, int MAXNT, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void bfStageKernelRealMfma(StageParams p) {
  __shared__ BfM64Tab tab;
  int const lane = threadIdx.x & 63;
  uint32_t const item = blockIdx.x;
  if (item >= p.numItems) return;
  BfDevItem const it = p.items[item];
  uint32_t const mr = it.mrFlags & 0xffffu;
  uint32_t const nrhs = p.nrhs;
  for (uint32_t q0 = 0; q0 < nrhs; q0 += 64) {
    uint32_t const nt = (nrhs - q0 >= 64) ? 4u : (nrhs - q0 + 15u) / 16u;
    uint32_t s0 = 0;
    while (s0 < mr) {
      if (mr - s0 > 16) { bfMRealDispatch<DT, 2, MAXNT>(nt, p, it, mr, s0, q0, &tab, lane); s0 += 32; }
      else { bfMRealDispatch<DT, 1, MAXNT>(nt, p, it, mr, s0, q0, &tab, lane); s0 += 16; }
    }
  }
}
#endif
