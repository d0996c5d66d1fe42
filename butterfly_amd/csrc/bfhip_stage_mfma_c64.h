// bfhip_stage_mfma_c64.h -- forward stage kernel of the 8-byte complex element type (complex64) for blocks of right-hand sides:
// the items and packed pieces of the real family's plan exactly as bfStageKernelReal / bfStageKernelSmall read them, contracted on
// the FP64 matrix cores (v_mfma_f64_16x16x4_f64) after an exact widening (v_cvt_f64_f32).  Every leaf element is loaded ONCE per
// pass of up to 64 right-hand sides; the default kernels load it once per right-hand side.  Opt-in per operator
// (bfhipSetRhsBlocks).  Included by bfhip_device.hip only, after bfhip_stage_mfma.h, whose structure it follows: one wavefront
// per item, a per-segment LDS table with one entry per leaf column, a flat k-loop of 4 leaf columns per step, MS 16-row slabs x
// NT 16-RHS tiles, Gauss's three real MFMAs per complex product.
//
// The element type's contract is unchanged: complex MACs in double, ONE rounding to complex64 at the store.  Fragment maps
// (cdna_hip_programming.md section 3): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], D reg v of lane l = D[i = 4 v + (l >> 4)]
// [j = l & 15]; with T1 = sum Ar Xr, T2 = sum Ai Xi, T3 = sum (Ar + Ai)(Xr + Xi): Re = T1 - T2, Im = T3 - T1 - T2.  The sums
// Ar + Ai and Xr + Xi are formed in double from exactly widened floats; what Gauss's form adds to the imaginary part is a few
// u64 of |A||x|, 2^29 below the store's rounding.  The order of summation differs from the default kernels': results agree with
// theirs to the last float bit or differ in it, and are bit-identical from one apply to the next (one owner per output, no atomics).
//
// What the real family's plan holds that the complex128 plan never does, and what the kernel does with it.  A table entry per
// leaf column c of a segment: the byte offset of its input row, the byte offset of its element of row 0, and its ROW stride in bytes:
//   * column-major pieces (column stride mrPad = the item's rows padded to the lane granule, 2): element (r, c) at dataOff +
//     c mrPad + r: row stride 8 bytes.  MERGED items and runs of narrow pieces are one segment whatever the number of pieces;
//   * ROWMAJOR pieces (few-row wide leaves; every dense piece of a SMALL item): element (r, c) at dataOff + r ld + c: row stride
//     8 ld bytes -- only the per-lane offsets differ.  A piece wider than the table is cut into segments of BF_M64_TABCAP columns;
//   * identity pieces are added at the store (in double, before the one rounding); an item without dense pieces stores its
//     identity terms, or zeros;
//   * pieces that read x and pieces that read the vector arena are different segments (the input base is per segment).
// Items of <= 4 rows waste most of a 16-row slab; they are bound by their loads, not by the pipe.
//
// Padding never meets data.  A lane of a k-step whose column lies past the end of the segment reads the table's padding (the
// segment's first leaf element, its first input row: addresses the item reads anyway) and BOTH its fragments are replaced by
// zeros before they are widened: no zero is ever multiplied by a value of x.  Rows past the item's end and right-hand sides
// past nrhs are clamped to the last real row / column: those lanes compute copies that are never stored, and a row (column) of the product
// depends on that row of A (column of X) only.  Every address is a base taken from an arena offset that validateStage has
// checked plus an offset below the piece's own extent.
//
// Budget (hipcc -Rpass-analysis=kernel-resource-usage, asserted by tests/test_c64_rhs_blocks_cpu.py): no scratch, no spills;
// the 4-tile instantiation keeps its 96 accumulator doubles (192 registers) and fits two wavefronts per SIMD; 9.2 KiB of LDS per
// one-wavefront workgroup.  The widening converts and the fragment sums are VALU work inside the k-loop (per k-step at MS = 2,
// NT = 4: 12 converts, 6 adds against 24 MFMAs of 8 passes each); they run while the other wavefront of the SIMD owns the pipe.
//
// Only complex64 is built here.  The real element types (F64, F32) have the same kernel with one scalar per fragment and one MFMA
// per product in bfhip_stage_mfma_real.h (bfhipSetRealRhsBlocks), which reuses this file's table and constants.
#ifndef BFHIP_STAGE_MFMA_C64_H
#define BFHIP_STAGE_MFMA_C64_H

#define BF_M64_TABCAP 768u           /* columns of one segment: 3 x 4 bytes each */
#define BF_M64_TABPAD 16u
#define BF_M64_SPAN_BYTES (1u << 31) /* a segment's input rows, and its leaf data, span less than this many bytes (32-bit offsets) */

struct BfM64Tab { uint32_t x[BF_M64_TABCAP + BF_M64_TABPAD], a[BF_M64_TABCAP + BF_M64_TABPAD], s[BF_M64_TABCAP + BF_M64_TABPAD]; };

// the fragments of one k-step as they come from memory: complex64, 8 bytes per lane each
template <int NT, int MS> struct BfM64Raw { float2 a[MS], x[NT]; };

template <int NT, int MS>
__device__ __forceinline__ void bfM64Load(BfM64Raw<NT, MS> &f, BfM64Tab const *tab, uint32_t c, char const *abase, char const *xbase,
                                          uint32_t const (&arow)[MS], uint32_t const (&xoff)[NT]) {
  // (no branch: a column past the end reads the table's padding -- the segment's first leaf element and first input row, both
  //  addresses the item reads anyway -- and bfM64Step replaces both fragments by zeros)
  uint32_t const xo = tab->x[c], ao = tab->a[c], as = tab->s[c];
#pragma unroll
  for (int m = 0; m < MS; ++m) {
    typedef float bf_f2 __attribute__((ext_vector_type(2)));
    bf_f2 const v = __builtin_nontemporal_load((bf_f2 const *)(abase + (ao + arow[m] * as)));      // the leaf stream: read once
    f.a[m] = make_float2(v.x, v.y);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) f.x[t] = *(float2 const *)(xbase + (xo + xoff[t]));
}

// the MFMAs of one k-step: widen (exact), Gauss's sums, 3 MS NT matrix instructions
template <int NT, int MS>
__device__ __forceinline__ void bfM64Step(bf_d4 (&acc)[3][MS][NT], BfM64Raw<NT, MS> const &f, bool valid) {
  double ar[MS], ai[MS], as[MS];
#pragma unroll
  for (int m = 0; m < MS; ++m) { ar[m] = (double)(valid ? f.a[m].x : 0.f); ai[m] = (double)(valid ? f.a[m].y : 0.f); as[m] = ar[m] + ai[m]; }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    double const xr = (double)(valid ? f.x[t].x : 0.f), xi = (double)(valid ? f.x[t].y : 0.f), xs = xr + xi;
#pragma unroll
    for (int m = 0; m < MS; ++m) {
      acc[0][m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[m], xr, acc[0][m][t], 0, 0, 0);
      acc[1][m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[m], xi, acc[1][m][t], 0, 0, 0);
      acc[2][m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[m], xs, acc[2][m][t], 0, 0, 0);
    }
  }
}

// One pass = rows [s0, s0 + 16 MS) x RHS [q0, q0 + 16 NT) of one item, over all its segments.
template <int NT, int MS>
__device__ __forceinline__ void bfM64Pass(StageParams const &p, BfDevItem const &it, uint32_t mr, uint32_t s0, uint32_t q0, BfM64Tab *tab, int lane) {
  uint32_t const nrhs = p.nrhs;
  uint32_t const li = lane & 15, lk = lane >> 4;
  uint32_t const mrPad = (mr + 1u) & ~1u;
  uint32_t const qleft = nrhs - q0;                    // >= 1
  bf_d4 acc[3][MS][NT];                                // T1, T2, T3
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int m = 0; m < MS; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[g][m][t] = (bf_d4){0, 0, 0, 0};
  // rows past the item's end / right-hand sides past nrhs: copies of the last real one, never stored
  uint32_t arow[MS], xoff[NT];
#pragma unroll
  for (int m = 0; m < MS; ++m) { uint32_t const r = s0 + 16u * m + li; arow[m] = r < mr ? r : mr - 1u; }
#pragma unroll
  for (int t = 0; t < NT; ++t) { uint32_t const q = 16u * t + li; xoff[t] = (q < qleft ? q : qleft - 1u) * 8u; }
  bool hasIdentity = false;
  uint32_t const np = it.numPieces;
  uint32_t const spanRows = BF_M64_SPAN_BYTES / (nrhs * 8u);     // >= 4096 > BF_M64_TABCAP: a table's worth of one piece always fits
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
        if (px != inX || rel >= BF_M64_SPAN_BYTES / 8u || rel + extent >= BF_M64_SPAN_BYTES / 8u) break;
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
      uint32_t const colStride = rm ? 8u : mrPad * 8u, rowStride = rm ? pc.ld * 8u : 8u;
      uint32_t const a0 = (uint32_t)rel * 8u + pj * colStride;
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
    for (uint32_t j = (uint32_t)lane; j < cols; j += 64u) tab->x[j] = (tab->x[j] - minRow) * (nrhs * 8u);
    // columns past the end, as far as the last k-step's requests reach: any address of the segment will do
    if ((uint32_t)lane < BF_M64_TABPAD) { tab->x[cols + lane] = 0; tab->a[cols + lane] = 0; tab->s[cols + lane] = 0; }
    waveSync();
    char const *abase = (char const *)p.arena + aBase * 8u;
    char const *xbase = (inX ? (char const *)p.x : (char const *)p.temp) + ((uint64_t)minRow * nrhs + q0) * 8u;
    uint32_t const ksteps = (cols + 3u) / 4u;
    // the k-loop: the fragments of k-step ks + 1 are requested before the MFMAs of k-step ks.  Two register sets taken in turn
    // and no copy between them (with `cur = nxt` at the bottom hipcc waits for the NEXT k-step's loads before this one's MFMAs);
    // the scheduling barriers keep the requests ahead of the MFMAs they overlap.  An odd number of k-steps ends with a k-step
    // whose leaf fragments are zeros.
    BfM64Raw<NT, MS> f0, f1;
    uint32_t c = lk;
    bfM64Load<NT, MS>(f0, tab, c, abase, xbase, arow, xoff);
    for (uint32_t ks = 0; ks < ksteps; ks += 2) {
      __builtin_amdgcn_sched_barrier(0);
      bfM64Load<NT, MS>(f1, tab, c + 4u, abase, xbase, arow, xoff);
      __builtin_amdgcn_sched_barrier(0);
      bfM64Step<NT, MS>(acc, f0, c < cols);
      __builtin_amdgcn_sched_barrier(0);
      bfM64Load<NT, MS>(f0, tab, c + 8u, abase, xbase, arow, xoff);
      __builtin_amdgcn_sched_barrier(0);
      bfM64Step<NT, MS>(acc, f1, c + 4u < cols);
      c += 8u;
    }
    waveSync();                                        // the table is rewritten by the next segment
  }
  // ---- the pass's rows x right-hand sides out of the accumulators, rounded to complex64 once
  float2 *out = (it.mrFlags & BF_ITEM_OUT_Y) ? (float2 *)p.y : (float2 *)p.temp;
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
          double re = acc[0][m][t][v] - acc[1][m][t][v];
          double im = acc[2][m][t][v] - acc[0][m][t][v] - acc[1][m][t][v];
          if (hasIdentity) {
            for (uint32_t k = 0; k < np; ++k) {
              BfDevPiece const pc = p.pieces[it.pieceBegin + k];
              if (!(pc.flags & BF_PIECE_IDENTITY)) continue;
              float2 const *xin = (pc.flags & BF_PIECE_IN_X) ? (float2 const *)p.x : (float2 const *)p.temp;
              float2 const xv = xin[((uint64_t)pc.inOff + row) * nrhs + q0 + q];
              re += (double)xv.x; im += (double)xv.y;
            }
          }
          out[((uint64_t)it.outOff + row) * nrhs + q0 + q] = make_float2((float)re, (float)im);
        }
      }
}

template <int MS, int MAXNT>
__device__ __forceinline__ void bfM64Dispatch(uint32_t nt, StageParams const &p, BfDevItem const &it, uint32_t mr, uint32_t s0, uint32_t q0, BfM64Tab *tab, int lane) {
  if (MAXNT >= 4 && nt == 4) bfM64Pass<4, MS>(p, it, mr, s0, q0, tab, lane);
  else if (MAXNT >= 3 && nt == 3) bfM64Pass<3, MS>(p, it, mr, s0, q0, tab, lane);
  else if (MAXNT >= 2 && nt == 2) bfM64Pass<2, MS>(p, it, mr, s0, q0, tab, lane);
  else bfM64Pass<1, MS>(p, it, mr, s0, q0, tab, lane);
}

// MAXNT = the widest pass the launch needs (RHS tiles of 16); WAVES = wavefronts per SIMD the instantiation is built for: the
// 4-tile kernel's accumulators leave two, which is what the matrix pipe needs; with fewer right-hand sides the kernel is bound by
// the leaf stream and it is wavefronts (bytes in flight) that count.
template <int MAXNT, int WAVES>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void bfStageKernelC64Mfma(StageParams p) {
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
      if (mr - s0 > 16) { bfM64Dispatch<2, MAXNT>(nt, p, it, mr, s0, q0, &tab, lane); s0 += 32; }
      else { bfM64Dispatch<1, MAXNT>(nt, p, it, mr, s0, q0, &tab, lane); s0 += 16; }
    }
  }
}
#endif
