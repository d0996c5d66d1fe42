// bfhip_stage_mfma_blocks.h -- stage kernels of the real family's plans (F64, F32, complex64) and of the transposed plan (all four
// element types) for blocks of right-hand sides, contracted on the FP64 matrix cores (v_mfma_f64_16x16x4_f64).  Every leaf element
// is loaded ONCE per pass of up to 64 right-hand sides; the default kernels walk the whole item once per right-hand side.  Opt-in
// per operator: bfhipSetRhsBlocks (complex64 forward), bfhipSetRealRhsBlocks (F64 / F32 forward), bfhipSetAdjointRhsBlocks (the
// adjoint plan: bfStageKernelTMfma when it shares the forward leaves, the forward kernels when it is packed).  Included by
// bfhip_device.hip only, after bfhip_stage_mfma.h (the complex128 forward kernels), whose structure the forward kernels follow.
//
// Common to all of them: one wavefront per item; a pass = MS <= 2 slabs of 16 rows of the item x NT <= 4 tiles of 16 right-hand
// sides, over everything the item reads; F32 and complex64 fragments are widened exactly (v_cvt_f64_f32), every product and sum is
// in double, and a value is rounded to the storage type ONCE, at the store (the default F32 kernels accumulate in float: an item
// sum of the block path carries one rounding u32 plus K u64).  Identity pieces are added at the store, in double, before that
// rounding; an item without dense pieces stores its identity terms, or zeros.  One owner per output, no atomics: results are
// bit-identical from one apply to the next; the order of summation differs from the default kernels'.  Fragment maps
// (cdna_hip_programming.md section 3): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D reg v of lane l = D[i = 4 v +
// (l >> 4)][j = l & 15].
//
// Padding never meets data, forward or transposed.  A lane of a k-step that has no leaf column reads an address the item reads
// anyway and BOTH its fragments are replaced by zeros before they are widened or multiplied: no zero is ever multiplied by a value
// of x.  Rows past the item's end and right-hand sides past nrhs are clamped to the last real row / column: those lanes compute
// copies that are never stored, and a row (column) of the product depends on that row of A (column of X) only.
//
// ---- Forward (bfStageKernelC64Mfma, bfStageKernelRealMfma): the items and packed pieces exactly as bfStageKernelReal /
// bfStageKernelSmall read them.  An item is walked in SEGMENTS of at most BF_M64_TABCAP leaf columns; bfBlkSegment builds a
// segment's LDS table, one entry per leaf column c: the byte offset of its input row, the byte offset of its element of row 0, and
// its ROW stride in bytes.  The k-loop is flat over the table, 4 leaf columns per step.  With es the element size and EPL = 16 / es
// the lane granule of the plan (mrPad = the item's rows padded to it):
//   * column-major pieces: element (r, c) at dataOff + c mrPad + r: row stride es.  MERGED items and runs of narrow pieces are one
//     segment whatever the number of pieces;
//   * ROWMAJOR pieces (few-row wide leaves; every dense piece of a SMALL item): element (r, c) at dataOff + r ld + c: row stride
//     ld es -- only the per-lane offsets differ.  A piece wider than the table is cut into segments of BF_M64_TABCAP columns (pj
//     is the first column of piece pi that no segment has taken yet);
//   * pieces that read x and pieces that read the vector arena are different segments (the input base is per segment);
//   * spans: table entries are 32-bit byte offsets from the segment's first leaf element and its lowest input row, so a segment
//     ends before its leaf data or its input rows would span BF_M64_SPAN_BYTES;
//   * padding: the BF_M64_TABPAD entries after the last column, as far as the last k-step's requests reach, are zeros: the
//     segment's first leaf element and first input row.
// Every address is a base taken from an arena offset that validateStage has checked plus an offset below the piece's own extent.
// Items of <= 4 rows waste most of a 16-row slab; they are bound by their loads, not by the pipe.
//
// Complex64: Gauss's three real MFMAs per complex product and three accumulator sets: with T1 = sum Ar Xr, T2 = sum Ai Xi, T3 =
// sum (Ar + Ai)(Xr + Xi): Re = T1 - T2, Im = T3 - T1 - T2.  The sums Ar + Ai and Xr + Xi are formed in double from exactly widened
// floats; what Gauss's form adds to the imaginary part is a few u64 of |A||x|, 2^29 below the store's rounding, so results agree
// with the default kernels' to the last float bit or differ in it.  es = 8, EPL = 2.
//
// F64 / F32: one scalar per fragment, ONE MFMA per (slab, tile) per k-step, one accumulator set.  es = 8 / 4, EPL = 2 / 4.  F64
// has no converts; the fp32 matrix pipe is not used.
//
// ---- Transposed (bfStageKernelTMfma): the items and pieces of the transposed plan exactly as bfStageKernelT reads them (an item
// = mr <= 64 columns of A, a piece = a forward piece read with lanes on its columns), narrow, wide and formerly shared (coop) items
// alike; the four wavefronts of a workgroup take four list neighbours and never split an item.  An item of more than 32 columns
// takes two passes, each over its own columns of every piece, so a pass reads each leaf element it covers once (x is read once per
// pass: it is the re-read, cached operand).  A^T is the A operand: lane l = (i = l & 15, k = l >> 4) holds column c0 + 16 m + i of
// A at the lane's step, B is X[step][rhs j = l & 15].  The step index is affine inside a piece, so there is no table and no LDS:
// which steps a lane takes within a k-group is free as long as both fragments agree.
//   * a k-group is 4 EPL steps and EPL MFMAs per (slab, tile); MFMA e contracts slot e of the four k, and the x fragment of a
//     slot is the input row of its step;
//   * column-major pieces (element (step s, column j) at dataOff + j ld + s): lane k takes the 16-byte unit 4 g + k of its column
//     (steps (4 g + k) EPL + e: ONE load per slab);
//   * ROWMAJOR pieces (real family; element (s, j) at dataOff + s ld + j, at most 2 EPL steps: one group): slot e of lane k is
//     step 4 e + k: element loads, 16 consecutive columns per k; slots past the piece cost MFMAs on zeros.
// A step past the piece's ncols: the unit / row index is clamped into the piece for the address.  Nothing is read outside the
// extents tests/plan_emulator.py asserts for transposed pieces: units of a column up to ceil(ncols / EPL), columns below mr.
// Complex products take the four-real-product form with two accumulator sets (Re += Ar Xr, Re += (-Ai) Xi, Im += Ar Xi, Im += Ai
// Xr), so results are componentwise what zgemm gives; BFHIP_FLAG_EXACT_COMPLEX changes nothing.
//
// What is shared and what is not.  The element type (BfBlkElem), the store (bfBlkStore) and the driver of the passes (bfBlkDrive)
// serve forward and transposed; the forward segment builder, loader, k-loop and pass are one each for the three element types.
// The k-step is bfBlkStep (forward: Gauss for complex) and bfTmStep (transposed: the four-product form, EPL steps per group): two
// arithmetic contracts, kept apart on purpose.
//
// Budget (hipcc -Rpass-analysis=kernel-resource-usage, asserted by tests/test_c64_rhs_blocks_cpu.py, test_real_rhs_blocks_cpu.py
// and test_adjoint_rhs_blocks_cpu.py): no scratch, no spills anywhere.
//   * forward: 9.2 KiB of LDS per one-wavefront workgroup, which lets 17 workgroups share a CU's 160 KiB.  Complex64: the 4-tile
//     instantiation keeps its 96 accumulator doubles (192 registers) and fits two wavefronts per SIMD, which is what the matrix
//     pipe needs; with fewer right-hand sides the kernel is bound by the leaf stream and it is wavefronts (bytes in flight) that
//     count: WAVES = 4 / 3 / 2 at 1 / 2 / 4 tiles.  The widening converts and the fragment sums are VALU work inside the k-loop
//     (per k-step at MS = 2, NT = 4: 12 converts, 6 adds against 24 MFMAs of 8 passes each); they run while the other wavefront
//     of the SIMD owns the pipe.  Real: VGPRs of the 1 / 2 / 4-tile instantiations: F64 49 / 68 / 112, F32 49 / 67 / 106 -- all
//     below the 128 of four wavefronts per SIMD.  WAVES = 4 for all six: a fifth wavefront per SIMD that the 1- and 2-tile
//     register counts would allow has no table to work with.
//   * transposed: no LDS.  The real types hold 16 MS NT <= 64 accumulator registers and are built for 4 wavefronts per SIMD
//     (<= 128 VGPRs) at every tile count; the complex types hold twice that: 4 at 1 and 2 tiles, 2 (<= 256 VGPRs) at 4 tiles.
#ifndef BFHIP_STAGE_MFMA_BLOCKS_H
#define BFHIP_STAGE_MFMA_BLOCKS_H

#define BF_M64_TABCAP 768u           /* columns of one segment: 3 x 4 bytes each */
#define BF_M64_TABPAD 16u
#define BF_M64_SPAN_BYTES (1u << 31) /* a segment's input rows, and its leaf data, span less than this many bytes (32-bit offsets) */
#define BF_TM_WG_WAVES 4             /* wavefronts (items) per workgroup of the transposed kernel; the forward kernels have one */

struct BfM64Tab { uint32_t x[BF_M64_TABCAP + BF_M64_TABPAD], a[BF_M64_TABCAP + BF_M64_TABPAD], s[BF_M64_TABCAP + BF_M64_TABPAD]; };

// one element as it lies in memory: NC scalars (complex: re, im)
template <typename S, int NC> struct __attribute__((aligned(sizeof(S) * NC))) BfBlkElem { S v[NC]; };
template <int N> using BfInt = std::integral_constant<int, N>;

// ---------------------------------------------------------------------------
// shared by forward and transposed
// ---------------------------------------------------------------------------
// The rows [s0, s0 + 16 MS) x right-hand sides [q0, q0 + 16 NT) of a pass out of its accumulators: val(c, m, t, v) is component c
// of register v of (slab m, tile t); identity pieces are added in double, and the sum is rounded to the storage type once.
template <typename S, int NC, int NT, int MS, typename Val>
__device__ __forceinline__ void bfBlkStore(StageParams const &p, BfDevItem const &it, uint32_t mr, uint32_t s0, uint32_t q0, bool hasIdentity, int lane, Val const &val) {
  using E = BfBlkElem<S, NC>;
  uint32_t const nrhs = p.nrhs, qleft = nrhs - q0, np = it.numPieces;
  E *out = (it.mrFlags & BF_ITEM_OUT_Y) ? (E *)p.y : (E *)p.temp;
  // (the lane's coordinates are derived again from an opaque copy, as in bfMfmaStore: the store addresses are not carried through the k-loop)
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
          double sum[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c) sum[c] = val(c, m, t, v);
          if (hasIdentity) {
            for (uint32_t k = 0; k < np; ++k) {
              BfDevPiece const pc = p.pieces[it.pieceBegin + k];
              if (!(pc.flags & BF_PIECE_IDENTITY)) continue;
              E const *xin = (pc.flags & BF_PIECE_IN_X) ? (E const *)p.x : (E const *)p.temp;
              E const xv = xin[((uint64_t)pc.inOff + row) * nrhs + q0 + q];
#pragma unroll
              for (int c = 0; c < NC; ++c) sum[c] += (double)xv.v[c];
            }
          }
          E r;
#pragma unroll
          for (int c = 0; c < NC; ++c) r.v[c] = (S)sum[c];
          out[((uint64_t)it.outOff + row) * nrhs + q0 + q] = r;
        }
      }
}

// The passes of one item: right-hand sides in blocks of 64 (NT = the tiles of 16 the block needs, at most MAXNT = the widest
// pass the launch needs), rows in slabs of 32 while more than 16 are left.  pass(BfInt<NT>, BfInt<MS>, s0, q0) runs one.
template <int MAXNT, typename Pass>
__device__ __forceinline__ void bfBlkDrive(uint32_t mr, uint32_t nrhs, Pass const &pass) {
  for (uint32_t q0 = 0; q0 < nrhs; q0 += 64) {
    uint32_t const nt = (nrhs - q0 >= 64) ? 4u : (nrhs - q0 + 15u) / 16u;
    auto const tiles = [=](auto ms, uint32_t s0) __attribute__((always_inline)) {
      if (MAXNT >= 4 && nt == 4) pass(BfInt<4>{}, ms, s0, q0);
      else if (MAXNT >= 3 && nt == 3) pass(BfInt<3>{}, ms, s0, q0);
      else if (MAXNT >= 2 && nt == 2) pass(BfInt<2>{}, ms, s0, q0);
      else pass(BfInt<1>{}, ms, s0, q0);
    };
    uint32_t s0 = 0;
    while (s0 < mr) {
      if (mr - s0 > 16) { tiles(BfInt<2>{}, s0); s0 += 32; }
      else { tiles(BfInt<1>{}, s0); s0 += 16; }
    }
  }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
struct BfBlkSeg {
  uint32_t cols;        // leaf columns in the table; 0: nothing but identity pieces was left
  uint32_t minRow;      // the lowest input row: table entries x are byte offsets from it
  uint32_t inX;         // the input rows are rows of x (else of the vector arena)
  uint64_t aBase;       // element offset of the segment's first leaf element: table entries a are byte offsets from it
};

// The next segment of an item (see the header): its table into LDS, its extent into scalars; pi / pj move past what it took and
// hasIdentity is set for identity pieces met on the way.  ES = bytes per element, EPL = the plan's lane granule; nothing here
// depends on the pass's shape or the fragment type.  The descriptor window is loaded again for every segment: six registers that
// must not stay live across the k-loop.
template <uint32_t ES, uint32_t EPL>
__device__ __forceinline__ BfBlkSeg bfBlkSegment(StageParams const &p, BfDevItem const &it, uint32_t mr, BfM64Tab *tab, int lane,
                                                 uint32_t &pi, uint32_t &pj, bool &hasIdentity) {
  uint32_t const nrhs = p.nrhs, np = it.numPieces;
  uint32_t const mrPad = (mr + EPL - 1u) / EPL * EPL;
  uint32_t const spanRows = BF_M64_SPAN_BYTES / (nrhs * ES);     // >= 4096 > BF_M64_TABCAP: a table's worth of one piece always fits
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
    if (!n) break;                                     // the table is full
    bool const rm = (pc.flags & BF_PIECE_ROWMAJOR) != 0;
    uint32_t const px = pc.flags & BF_PIECE_IN_X, first = pc.inOff + pj, last = first + n - 1u;
    uint64_t const extent = rm ? (uint64_t)(mr - 1u) * pc.ld + pc.ncols : (uint64_t)mrPad * pc.ncols;      // elements of the whole piece
    uint32_t lo = first, hi = last;
    uint64_t rel = 0;
    if (started) {
      rel = pc.dataOff - aBase;                        // (wraps for a piece stored ahead of the segment's first: a new segment)
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
  BfBlkSeg const sg = {cols, minRow, inX, aBase};
  if (!cols) return sg;                                // identity pieces only
  waveSync();
  // rows -> byte offsets from the segment's first row (fits 32 bits: spanRows)
  for (uint32_t j = (uint32_t)lane; j < cols; j += 64u) tab->x[j] = (tab->x[j] - minRow) * (nrhs * ES);
  // columns past the end, as far as the last k-step's requests reach: any address of the segment will do
  if ((uint32_t)lane < BF_M64_TABPAD) { tab->x[cols + lane] = 0; tab->a[cols + lane] = 0; tab->s[cols + lane] = 0; }
  waveSync();
  return sg;
}

// the fragments of one k-step as they come from memory: one element per lane each
template <typename S, int NC, int NT, int MS> struct BfBlkRaw { BfBlkElem<S, NC> a[MS], x[NT]; };

template <typename S, int NC, int NT, int MS>
__device__ __forceinline__ void bfBlkLoad(BfBlkRaw<S, NC, NT, MS> &f, BfM64Tab const *tab, uint32_t c, char const *abase, char const *xbase,
                                          uint32_t const (&arow)[MS], uint32_t const (&xoff)[NT]) {
  // (no branch: a column past the end reads the table's padding -- the segment's first leaf element and first input row, both
  //  addresses the item reads anyway -- and bfBlkStep replaces both fragments by zeros)
  typedef S V __attribute__((ext_vector_type(NC)));
  uint32_t const xo = tab->x[c], ao = tab->a[c], as = tab->s[c];
#pragma unroll
  for (int m = 0; m < MS; ++m) {
    V const v = __builtin_nontemporal_load((V const *)(abase + (ao + arow[m] * as)));              // the leaf stream: read once
#pragma unroll
    for (int k = 0; k < NC; ++k) f.a[m].v[k] = v[k];
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) f.x[t] = *(BfBlkElem<S, NC> const *)(xbase + (xo + xoff[t]));
}

// the MFMAs of one k-step: widen (exact; nothing to do for double), then per (slab, tile) one matrix instruction (real) or
// Gauss's sums and three (complex: accumulator sets T1, T2, T3)
template <typename S, int NC, int NT, int MS>
__device__ __forceinline__ void bfBlkStep(bf_d4 (&acc)[NC == 2 ? 3 : 1][MS][NT], BfBlkRaw<S, NC, NT, MS> const &f, bool valid) {
  constexpr int NG = NC == 2 ? 3 : 1;
  double a[MS][NG];
#pragma unroll
  for (int m = 0; m < MS; ++m) {
#pragma unroll
    for (int k = 0; k < NC; ++k) a[m][k] = (double)(valid ? f.a[m].v[k] : S(0));
    if constexpr (NC == 2) a[m][2] = a[m][0] + a[m][1];
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    double x[NG];
#pragma unroll
    for (int k = 0; k < NC; ++k) x[k] = (double)(valid ? f.x[t].v[k] : S(0));
    if constexpr (NC == 2) x[2] = x[0] + x[1];
#pragma unroll
    for (int m = 0; m < MS; ++m)
#pragma unroll
      for (int g = 0; g < NG; ++g) acc[g][m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m][g], x[g], acc[g][m][t], 0, 0, 0);
  }
}

// The k-loop of one segment: the fragments of k-step ks + 1 are requested before the MFMAs of k-step ks.  Two register sets taken
// in turn and no copy between them (with `cur = nxt` at the bottom hipcc waits for the NEXT k-step's loads before this one's
// MFMAs); the scheduling barriers keep the requests ahead of the MFMAs they overlap.  An odd number of k-steps ends with a k-step
// whose fragments are zeros.
template <typename S, int NC, int NT, int MS>
__device__ __forceinline__ void bfBlkKLoop(bf_d4 (&acc)[NC == 2 ? 3 : 1][MS][NT], BfM64Tab const *tab, uint32_t cols, uint32_t lk,
                                           char const *abase, char const *xbase, uint32_t const (&arow)[MS], uint32_t const (&xoff)[NT]) {
  uint32_t const ksteps = (cols + 3u) / 4u;
  BfBlkRaw<S, NC, NT, MS> f0, f1;
  uint32_t c = lk;
  bfBlkLoad<S, NC, NT, MS>(f0, tab, c, abase, xbase, arow, xoff);
  for (uint32_t ks = 0; ks < ksteps; ks += 2) {
    __builtin_amdgcn_sched_barrier(0);
    bfBlkLoad<S, NC, NT, MS>(f1, tab, c + 4u, abase, xbase, arow, xoff);
    __builtin_amdgcn_sched_barrier(0);
    bfBlkStep<S, NC, NT, MS>(acc, f0, c < cols);
    __builtin_amdgcn_sched_barrier(0);
    bfBlkLoad<S, NC, NT, MS>(f0, tab, c + 8u, abase, xbase, arow, xoff);
    __builtin_amdgcn_sched_barrier(0);
    bfBlkStep<S, NC, NT, MS>(acc, f1, c + 4u < cols);
    c += 8u;
  }
}

// One pass = rows [s0, s0 + 16 MS) x RHS [q0, q0 + 16 NT) of one item, over all its segments.  DT = F64, F32 or C64.
template <int DT, int NT, int MS>
__device__ __forceinline__ void bfBlkPass(StageParams const &p, BfDevItem const &it, uint32_t mr, uint32_t s0, uint32_t q0, BfM64Tab *tab, int lane) {
  using S = typename Traits<DT>::S;
  constexpr int NC = Traits<DT>::CPLX ? 2 : 1, NG = NC == 2 ? 3 : 1;
  constexpr uint32_t ES = sizeof(S) * NC, EPL = Traits<DT>::EPL;
  uint32_t const nrhs = p.nrhs;
  uint32_t const li = lane & 15, lk = lane >> 4;
  uint32_t const qleft = nrhs - q0;                    // >= 1
  bf_d4 acc[NG][MS][NT];                               // real: the sums; complex: T1, T2, T3
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int m = 0; m < MS; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[g][m][t] = (bf_d4){0, 0, 0, 0};
  // rows past the item's end / right-hand sides past nrhs: copies of the last real one, never stored
  uint32_t arow[MS], xoff[NT];
#pragma unroll
  for (int m = 0; m < MS; ++m) { uint32_t const r = s0 + 16u * m + li; arow[m] = r < mr ? r : mr - 1u; }
#pragma unroll
  for (int t = 0; t < NT; ++t) { uint32_t const q = 16u * t + li; xoff[t] = (q < qleft ? q : qleft - 1u) * ES; }
  bool hasIdentity = false;
  uint32_t pi = 0, pj = 0;                             // the next piece, and the first column of it that no segment has taken yet
  while (pi < it.numPieces) {
    BfBlkSeg const sg = bfBlkSegment<ES, EPL>(p, it, mr, tab, lane, pi, pj, hasIdentity);
    if (!sg.cols) break;
    char const *abase = (char const *)p.arena + sg.aBase * ES;
    char const *xbase = (sg.inX ? (char const *)p.x : (char const *)p.temp) + ((uint64_t)sg.minRow * nrhs + q0) * ES;
    bfBlkKLoop<S, NC, NT, MS>(acc, tab, sg.cols, lk, abase, xbase, arow, xoff);
    waveSync();                                        // the table is rewritten by the next segment
  }
  bfBlkStore<S, NC, NT, MS>(p, it, mr, s0, q0, hasIdentity, lane, [&](int c, int m, int t, int v) __attribute__((always_inline)) {
    if constexpr (NC == 2) return c ? acc[2][m][t][v] - acc[0][m][t][v] - acc[1][m][t][v] : acc[0][m][t][v] - acc[1][m][t][v];
    else return acc[0][m][t][v];
  });
}

// the body of a forward kernel: one wavefront (workgroup) per item
template <int DT, int MAXNT>
__device__ __forceinline__ void bfBlkForward(StageParams const &p, BfM64Tab *tab) {
  int const lane = threadIdx.x & 63;
  uint32_t const item = blockIdx.x;
  if (item >= p.numItems) return;
  BfDevItem const it = p.items[item];
  uint32_t const mr = it.mrFlags & 0xffffu;
  bfBlkDrive<MAXNT>(mr, p.nrhs, [=](auto nt, auto ms, uint32_t s0, uint32_t q0) __attribute__((always_inline)) {
    bfBlkPass<DT, decltype(nt)::value, decltype(ms)::value>(p, it, mr, s0, q0, tab, lane);
  });
}

// MAXNT = the widest pass the launch needs (RHS tiles of 16: 1, 2 or 4); WAVES = wavefronts per SIMD the instantiation is built
// for (see the budget above)
template <int MAXNT, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void bfStageKernelC64Mfma(StageParams p) {
  __shared__ BfM64Tab tab;
  bfBlkForward<BFHIP_C64, MAXNT>(p, &tab);
}

// DT = BFHIP_F64 / BFHIP_F32
template <int DT, int MAXNT, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void bfStageKernelRealMfma(StageParams p) {
  __shared__ BfM64Tab tab;
  bfBlkForward<DT, MAXNT>(p, &tab);
}

// ---------------------------------------------------------------------------
// transposed
// ---------------------------------------------------------------------------
// the fragments of one k-group as they come from memory: SUB steps per lane
template <typename S, int NC, int SUB, int NT, int MS> struct BfTmRaw { BfBlkElem<S, NC> a[MS][SUB], x[NT][SUB]; };

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
  using E = BfBlkElem<S, NC>;
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
  bfBlkStore<S, NC, NT, MS>(p, it, mr, c0, q0, hasIdentity, lane, [&](int c, int m, int t, int v) __attribute__((always_inline)) { return acc[c][m][t][v]; });
}

// DT = any element type
template <int DT, int MAXNT, int WAVES>
__global__ __launch_bounds__(BF_TM_WG_WAVES * 64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void bfStageKernelTMfma(StageParams p) {
  int const wave = threadIdx.x >> 6;
  int const lane = threadIdx.x & 63;
  uint32_t const item = __builtin_amdgcn_readfirstlane(blockIdx.x * BF_TM_WG_WAVES + wave);
  if (item >= p.numItems) return;
  BfDevItem const it = p.items[item];
  uint32_t const mr = it.mrFlags & 0xffffu;
  bfBlkDrive<MAXNT>(mr, p.nrhs, [=](auto nt, auto ms, uint32_t c0, uint32_t q0) __attribute__((always_inline)) {
    bfTmPass<DT, decltype(nt)::value, decltype(ms)::value>(p, it, mr, c0, q0, lane);
  });
}
#endif
