// bfhip_stage_mfma.h -- complex128 stage kernel for blocks of right-hand sides (nrhs >= 2): the same items and the
// same packed pieces as bfStageKernelC128, contracted on the FP64 matrix cores (v_mfma_f64_16x16x4_f64).  It replaces
// the cblas_zgemm of every leaf of a level (reference src/mat_dense_complex.c:1704-1765) and the view / accumulate
// passes around it (src/mat_block_coo.c:404-418, src/mat_block_diag.c:387-399).  Included by bfhip_device.hip only.
//
// Shape of the work.  An item is <= 64 rows of one output row group; its dense pieces are stored back to back,
// column-major with the item's row count as the column stride, so the item's leaf data is ONE column-major
// mr x C matrix (C = the sum of the pieces' widths) -- a *segment* -- whose column c multiplies one row of the
// input vector.  The kernel writes tab[] (that row's byte offset, 32 bits per column) into LDS once per segment and then runs
// one flat k-loop over the segment: piece boundaries do not exist inside the loop.  (A segment ends where the next
// piece is not contiguous, reads another vector (x / intermediates), or the table is full; fac_helm2 items are one
// segment, two in the last stage.)
//
// One pass = MS 16-row slabs x NT 16-RHS tiles.  Fragment maps (cdna_hip_programming.md section 3): A[i = l & 15][k = l >> 4],
// B[k = l >> 4][j = l & 15], D reg v of lane l = D[i = 4 v + (l >> 4)][j = l & 15].  A complex multiply-accumulate is
//   * by default THREE real MFMAs (Gauss: T1 = Ar Xr, T2 = Ai Xi, T3 = (Ar + Ai)(Xr + Xi); Re = T1 - T2, Im = T3 - T1 - T2):
//     3 MS NT MFMAs per k-step (4 leaf columns), three accumulators per tile.  Normwise as accurate as zgemm's four
//     multiplications; componentwise the imaginary part carries an error of eps * (|Ar| + |Ai|)(|Xr| + |Xi|) summed over the
//     contraction, whatever its own size;
//   * with BFHIP_FLAG_EXACT_COMPLEX the FOUR real MFMAs of the textbook product (GAUSS = false below: Re += Ar Xr - Ai Xi,
//     Im += Ar Xi + Ai Xr, the -Ai Xi term through the NEG bit of the instruction -- blgp bit 0 negates A on the f64 MFMA:
//     tools/mfma_probe.hip), two accumulators per tile: componentwise what cblas_zgemm's own recurrence gives
//     (src/mat_dense_complex.c:1704-1765), a third more matrix-pipe work.
//
// The ragged last slab of an item (1 - 12 of its 16 rows real) runs as QUARTER slabs on v_mfma_f64_4x4x4 in the 64-RHS kernel
// (bfMfmaSegmentQ below): the X fragment is that instruction's B operand as it stands.
//
// What the inner loops are made of, and why (tools/mfma_probe.hip, tools/mfma_loop_probe.hip, profiles/r4_mfma_probe.json):
//   * ONE wavefront cannot keep the FP64 matrix pipe busy (0.75 of peak with 16 independent accumulators), two or more
//     can (0.99): every cycle a wavefront spends on anything else costs a quarter of the pipe, so the loop holds no
//     VALU address arithmetic, no selects and no register copies.  Fragments come through buffer loads -- a loop
//     invariant VGPR offset, the k-step advance in an SGPR, columns / rows past the end of the segment returned as
//     zeros by the range check (which includes the SGPR offset) instead of clamps + selects.
//   * The loads are asm statements and the waits are placed by hand: hipcc's wait insertion treats every load pending
//     at a loop header as one lump (s_waitcnt vmcnt(0) at the top: the fragment requested last would be waited for
//     first).  Loads return in order, so vmcnt(n) = "all but the n youngest have arrived".
//   * bfMfmaSegment (all three kernels): fragments land in registers, two sets for the leaf stream (requested one k-step ahead),
//     one for the X tiles (requested again right after the MFMAs that read them).
//   * Two other loops were built and measured in round 5, bit-identical and slower, and are not part of this file: fragments landing
//     in a two-slot LDS ring per wavefront two k-steps ahead of their use (2 - 4 % slower), and X tiles fetched once per workgroup of
//     four wavefronts (1.5 - 2 % slower on the whole apply).  The bare loops live beside their probes in tools/mfma_setaside_loops.h;
//     DESIGN.md section 9 has the measurements.
#ifndef BFHIP_STAGE_MFMA_H
#define BFHIP_STAGE_MFMA_H

#define BF_MF_TABCAP 1792u          /* columns of one segment: 7.1 KiB of LDS per wavefront -- 20 wavefronts per CU (the 1-tile instantiation) fit 160 KiB */
#define BF_MF_TABPAD 24u
#define BF_MF_SPAN_BYTES (1u << 31) /* a segment's input rows span less than this many bytes (32-bit buffer offsets) */
#ifndef BF_MFMA_WAVES_PER_SIMD
#define BF_MFMA_WAVES_PER_SIMD 2
#endif
#ifndef BF_MF_XCD_RUN
#define BF_MF_XCD_RUN 32u           /* workgroups */
#endif
#ifndef BF_MF_WG_WAVES
#define BF_MF_WG_WAVES 1u
#endif
#ifndef BF_MFMA_MIN_RHS
#define BF_MFMA_MIN_RHS 2
#endif
#ifndef BF_MF_QUARTER
#define BF_MF_QUARTER 1            /* the 64-RHS kernel runs the ragged last slab of an item on v_mfma_f64_4x4x4 (A/B builds: 0) */
#endif
// (Round 5, measured and removed: with BF_MF_WG_WAVES = 2 / 4 / 8 an s_barrier every pair of k-steps, so that list neighbours -- which
// walk the same X rows -- pace each other and their X requests reach the L2 together: 31.38 / 31.67 / 34.07 ms against 30.91 with
// one-wavefront workgroups; 4 wavefronts without the barrier 31.51.  DESIGN.md section 9.)

typedef double bf_d4 __attribute__((ext_vector_type(4)));
typedef int bf_i4 __attribute__((ext_vector_type(4)));
union BfFrag { bf_u4 u; double d[2]; };

// a raw buffer descriptor in SGPRs: 48-bit base, stride 0, num_records in bytes
__device__ __forceinline__ bf_i4 bfMakeRsrc(void const *base, uint32_t bytes) {
  uint64_t const b = (uint64_t)base;
  bf_i4 r;
  r.x = __builtin_amdgcn_readfirstlane((int)(uint32_t)b);
  r.y = __builtin_amdgcn_readfirstlane((int)((uint32_t)(b >> 32) & 0xffffu));
  r.z = __builtin_amdgcn_readfirstlane((int)bytes);
  r.w = 0x00020000;
  return r;
}
// cache policy of the leaf stream (read once per apply): "nt" = non-temporal; A/B builds try others (-DBF_MF_A_POLICY='"sc0 sc1 nt"')
#ifndef BF_MF_A_POLICY
#define BF_MF_A_POLICY "nt"
#endif
template <int STREAM, int OFF> __device__ __forceinline__ void bfFragLoad(BfFrag &f, uint32_t voff, bf_i4 rsrc, uint32_t soff) {
  if (STREAM) asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:%4 " BF_MF_A_POLICY : "=v"(f.u) : "v"(voff), "s"(rsrc), "s"(soff), "n"(OFF));
  else asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:%4" : "=v"(f.u) : "v"(voff), "s"(rsrc), "s"(soff), "n"(OFF));
}
template <int N> __device__ __forceinline__ void bfFragWait(BfFrag &f) { asm volatile("s_waitcnt vmcnt(%1)" : "+v"(f.u) : "n"(N)); }
template <int N> __device__ __forceinline__ void bfFragWait(BfFrag &f, BfFrag &g) { asm volatile("s_waitcnt vmcnt(%2)" : "+v"(f.u), "+v"(g.u) : "n"(N)); }

// What a segment's k-loop needs besides the table.
struct BfMfSeg {
  bf_i4 ra, rx;          // leaf matrix (mr x cols, column-major), input rows [minRow, maxRow] x the pass's RHS
  uint32_t voffA;        // lane: (column lk of a k-step, row s0 + li); slab 1 is +256 bytes
  uint32_t cX;           // lane: li * 16; + tab[column] = byte offset of the lane's X fragment
  uint32_t stepA;        // 4 columns = 4 * mr * 16 bytes
  uint32_t ksteps;
};

// The k-loop of one segment: MS slabs x NT tiles.
//
// Complex products by Gauss's three multiplications: with T1 = Ar Xr, T2 = Ai Xi, T3 = (Ar + Ai)(Xr + Xi) summed over
// the segment, Re = T1 - T2 and Im = T3 - T1 - T2 -- 3 real MFMAs per complex multiply-accumulate instead of 4, paid
// for with MS + NT v_add_f64 per k-step (the fragment sums) and a third accumulator per tile (24 x 8 = 192 VGPRs: two
// wavefronts per SIMD still fit).  The kernel is clock-bound, not issue-bound (the pipe stays 93 % busy and
// the clock follows the traffic beyond L2 in every variant of this loop), so a quarter fewer MFMAs is a quarter less time.  Normwise as accurate as
// the four-multiplication form (the imaginary part loses relative accuracy only where it is small next to |A||X|).
//
// Registers and requests.  A fragments (streamed from HBM, the long latency) have TWO sets: the A of k-step ks + 1 is
// requested at the top of k-step ks.  X fragments (L2) have ONE set: tile t is requested again right after the 3 MS
// MFMAs that read it, 3 MS (NT - 1) MFMAs before its next use (tile-outer, slab-inner order).  Requests return in order,
// so in front of every tile "all but the NT - 1 + MS youngest have arrived" is the wait (s_waitcnt vmcnt).
// An odd number of k-steps ends with a k-step of zeros (the leaf fragments past the end of the segment).
// the four real products of a complex multiply-accumulate (BFHIP_FLAG_EXACT_COMPLEX): Re += Ar Xr - Ai Xi, Im += Ar Xi + Ai Xr
__device__ __forceinline__ void bfMfmaExact(bf_d4 &re, bf_d4 &im, BfFrag const &a, BfFrag const &x) {
  re = __builtin_amdgcn_mfma_f64_16x16x4f64(a.d[0], x.d[0], re, 0, 0, 0);
  re = __builtin_amdgcn_mfma_f64_16x16x4f64(a.d[1], x.d[1], re, 0, 0, 1);      // blgp bit 0: -A
  im = __builtin_amdgcn_mfma_f64_16x16x4f64(a.d[0], x.d[1], im, 0, 0, 0);
  im = __builtin_amdgcn_mfma_f64_16x16x4f64(a.d[1], x.d[0], im, 0, 0, 0);
}
template <int MS, int SET>
__device__ __forceinline__ void bfMfmaRequestA(BfFrag (&a)[2][2], BfMfSeg const &sg, uint32_t soffA) {
  bfFragLoad<1, 0>(a[SET][0], sg.voffA, sg.ra, soffA);
  if (MS > 1) bfFragLoad<1, 256>(a[SET][1], sg.voffA, sg.ra, soffA);
}
template <int T>
__device__ __forceinline__ void bfMfmaRequestX(BfFrag (&x)[4], BfMfSeg const &sg, uint32_t voffX) {
  bfFragLoad<0, 256 * T>(x[T], voffX, sg.rx, 0);
}
template <int NT, int MS, int SET, int T, bool GAUSS>
__device__ __forceinline__ void bfMfmaTile(bf_d4 (&acc)[3][2][4], BfFrag (&a)[2][2], BfFrag (&x)[4], double (&as)[2], BfMfSeg const &sg, uint32_t voffXnext) {
  if (T < NT) {
    constexpr int TT = T < NT ? T : 0;
    constexpr int pending = NT - 1 + MS;
    if (T == 0 && MS > 1) asm volatile("s_waitcnt vmcnt(%3)" : "+v"(a[SET][0].u), "+v"(a[SET][1].u), "+v"(x[0].u) : "n"(pending));
    else if (T == 0) asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a[SET][0].u), "+v"(x[0].u) : "n"(pending));
    else asm volatile("s_waitcnt vmcnt(%1)" : "+v"(x[TT].u) : "n"(pending));
    if (GAUSS) {
      if (T == 0) {
        as[0] = a[SET][0].d[0] + a[SET][0].d[1];
        if (MS > 1) as[1] = a[SET][1].d[0] + a[SET][1].d[1];
      }
      double const xs = x[TT].d[0] + x[TT].d[1];
#pragma unroll
      for (int m = 0; m < MS; ++m) {
        acc[0][m][TT] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[SET][m].d[0], x[TT].d[0], acc[0][m][TT], 0, 0, 0);
        acc[1][m][TT] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[SET][m].d[1], x[TT].d[1], acc[1][m][TT], 0, 0, 0);
        acc[2][m][TT] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[m], xs, acc[2][m][TT], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int m = 0; m < MS; ++m) bfMfmaExact(acc[0][m][TT], acc[1][m][TT], a[SET][m], x[TT]);
    }
    __builtin_amdgcn_sched_barrier(0);
    bfMfmaRequestX<TT>(x, sg, voffXnext);
    __builtin_amdgcn_sched_barrier(0);
  }
}
template <int NT, int MS, bool GAUSS = true>
__device__ __forceinline__ void bfMfmaSegment(bf_d4 (&acc)[3][2][4], BfMfSeg const &sg, uint32_t const *tab, uint32_t lk) {
  BfFrag a[2][2], x[4];
  double as[2];
  uint32_t ti = lk;
  uint32_t soffA = 0;
  {
    uint32_t const v0 = tab[ti] + sg.cX;
    bfMfmaRequestA<MS, 0>(a, sg, soffA);
    bfMfmaRequestX<0>(x, sg, v0);
    if (NT > 1) bfMfmaRequestX<1>(x, sg, v0);
    if (NT > 2) bfMfmaRequestX<2>(x, sg, v0);
    if (NT > 3) bfMfmaRequestX<3>(x, sg, v0);
  }
  uint32_t t1 = tab[ti + 4], t2 = tab[ti + 8];      // read an iteration ahead of their use
  ti += 12;
  for (uint32_t ks = 0; ks < sg.ksteps; ks += 2) {
    uint32_t const v1 = t1 + sg.cX, v2 = t2 + sg.cX;
    t1 = tab[ti];                                    // the table is padded past the last k-step (BF_MF_TABPAD)
    t2 = tab[ti + 4];
    ti += 8;
    soffA += sg.stepA;
    __builtin_amdgcn_sched_barrier(0);
    bfMfmaRequestA<MS, 1>(a, sg, soffA);
    __builtin_amdgcn_sched_barrier(0);
    bfMfmaTile<NT, MS, 0, 0, GAUSS>(acc, a, x, as, sg, v1);
    bfMfmaTile<NT, MS, 0, 1, GAUSS>(acc, a, x, as, sg, v1);
    bfMfmaTile<NT, MS, 0, 2, GAUSS>(acc, a, x, as, sg, v1);
    bfMfmaTile<NT, MS, 0, 3, GAUSS>(acc, a, x, as, sg, v1);
    soffA += sg.stepA;
    bfMfmaRequestA<MS, 0>(a, sg, soffA);
    __builtin_amdgcn_sched_barrier(0);
    bfMfmaTile<NT, MS, 1, 0, GAUSS>(acc, a, x, as, sg, v2);
    bfMfmaTile<NT, MS, 1, 1, GAUSS>(acc, a, x, as, sg, v2);
    bfMfmaTile<NT, MS, 1, 2, GAUSS>(acc, a, x, as, sg, v2);
    bfMfmaTile<NT, MS, 1, 3, GAUSS>(acc, a, x, as, sg, v2);
  }
  // the requests of the k-steps past the end (zeros from the range check / a padded table row) must land before the
  // registers are used again
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(a[0][0].u), "+v"(a[0][MS > 1 ? 1 : 0].u), "+v"(x[0].u), "+v"(x[NT > 1 ? 1 : 0].u), "+v"(x[NT > 2 ? 2 : 0].u), "+v"(x[NT > 3 ? 3 : 0].u));
}

// ---- the ragged last slab of a pass on v_mfma_f64_4x4x4 (round 5) ----------------------------------------------------------------------
// Row groups are ranks of (target, source) pairs -- 17 - 24 rows are common -- and an item's last 16-row slab is mostly padding (N =
// 262144: 4.4 % of all MFMA time, N = 65536: 10 %).  v_mfma_f64_4x4x4 computes four independent 4 x 4 x 4 blocks in a quarter of the
// big instruction's time (tools/mfma_4x4x4_probe.hip: A[i][k] in lane 16 k + 4 b + i, B[k][j] in lane 16 k + 4 b + j, D[i][j] in lane
// 16 i + 4 b + j for block b; 0.88 of the big instruction's flop rate).  Its B operand is the 16 x 16 x 4 X FRAGMENT AS IT STANDS -- block
// b = right-hand sides 4 b ... 4 b + 3 -- and the SAME four leaf rows go to every block: a quarter fragment is one more leaf load whose
// lanes take row (lane & 3) instead of row (lane & 15).  A tail of t = 1 ... 12 rows runs as ceil(t / 4) quarter slabs (QT), next to MS = 0
// or 1 full slabs; 13 ... 16 rows stay a full slab.  Accumulators: one double per lane, tile and product.  Same waits as bfMfmaSegment
// with MS + QT leaf requests per k-step.  (The sums of a 4 x 4 x 4 block and of a 16 x 16 x 4 tile may round differently: results are not
// bit-identical to the all-full-slab kernel, equally accurate.)
template <int MS, int QT, int SET>
__device__ __forceinline__ void bfMfmaRequestAQ(BfFrag (&a)[2], BfFrag (&aq)[2][3], BfMfSeg const &sg, uint32_t voffAq, uint32_t soffA) {
  if (MS > 0) bfFragLoad<1, 0>(a[SET], sg.voffA, sg.ra, soffA);
  bfFragLoad<1, 256 * MS>(aq[SET][0], voffAq, sg.ra, soffA);
  if (QT > 1) bfFragLoad<1, 256 * MS + 64>(aq[SET][1], voffAq, sg.ra, soffA);
  if (QT > 2) bfFragLoad<1, 256 * MS + 128>(aq[SET][2], voffAq, sg.ra, soffA);
}
template <int MS, int QT, int SET, int T>
__device__ __forceinline__ void bfMfmaTileQ(bf_d4 (&acc)[3][4], double (&accq)[3][3][4], BfFrag (&a)[2], BfFrag (&aq)[2][3], BfFrag (&x)[4], double &as, double (&asq)[3],
                                            BfMfSeg const &sg, uint32_t voffXnext) {
  constexpr int pending = 4 - 1 + MS + QT;
  if (T == 0) {      // this k-step's leaf fragments and tile 0 (never the same variable twice in one statement)
    if (MS > 0 && QT == 1) asm volatile("s_waitcnt vmcnt(%3)" : "+v"(a[SET].u), "+v"(aq[SET][0].u), "+v"(x[0].u) : "n"(pending));
    else if (MS > 0 && QT == 2) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a[SET].u), "+v"(aq[SET][0].u), "+v"(aq[SET][1].u), "+v"(x[0].u) : "n"(pending));
    else if (MS > 0) asm volatile("s_waitcnt vmcnt(%5)" : "+v"(a[SET].u), "+v"(aq[SET][0].u), "+v"(aq[SET][1].u), "+v"(aq[SET][2].u), "+v"(x[0].u) : "n"(pending));
    else if (QT == 1) asm volatile("s_waitcnt vmcnt(%2)" : "+v"(aq[SET][0].u), "+v"(x[0].u) : "n"(pending));
    else if (QT == 2) asm volatile("s_waitcnt vmcnt(%3)" : "+v"(aq[SET][0].u), "+v"(aq[SET][1].u), "+v"(x[0].u) : "n"(pending));
    else asm volatile("s_waitcnt vmcnt(%4)" : "+v"(aq[SET][0].u), "+v"(aq[SET][1].u), "+v"(aq[SET][2].u), "+v"(x[0].u) : "n"(pending));
    if (MS > 0) as = a[SET].d[0] + a[SET].d[1];
#pragma unroll
    for (int q = 0; q < QT; ++q) asq[q] = aq[SET][q].d[0] + aq[SET][q].d[1];
  } else asm volatile("s_waitcnt vmcnt(%1)" : "+v"(x[T].u) : "n"(pending));
  double const xs = x[T].d[0] + x[T].d[1];
  if (MS > 0) {
    acc[0][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[SET].d[0], x[T].d[0], acc[0][T], 0, 0, 0);
    acc[1][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[SET].d[1], x[T].d[1], acc[1][T], 0, 0, 0);
    acc[2][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(as, xs, acc[2][T], 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < QT; ++q) {
    accq[0][q][T] = __builtin_amdgcn_mfma_f64_4x4x4f64(aq[SET][q].d[0], x[T].d[0], accq[0][q][T], 0, 0, 0);
    accq[1][q][T] = __builtin_amdgcn_mfma_f64_4x4x4f64(aq[SET][q].d[1], x[T].d[1], accq[1][q][T], 0, 0, 0);
    accq[2][q][T] = __builtin_amdgcn_mfma_f64_4x4x4f64(asq[q], xs, accq[2][q][T], 0, 0, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
  bfMfmaRequestX<T>(x, sg, voffXnext);
  __builtin_amdgcn_sched_barrier(0);
}
// the k-loop of one segment: MS (0 or 1) full slabs + QT (1 ... 3) quarter slabs x 4 tiles, Gauss's three multiplications
template <int MS, int QT>
__device__ __forceinline__ void bfMfmaSegmentQ(bf_d4 (&acc)[3][4], double (&accq)[3][3][4], BfMfSeg const &sg, uint32_t voffAq, uint32_t const *tab, uint32_t lk) {
  BfFrag a[2], aq[2][3], x[4];
  double as = 0, asq[3];
  uint32_t ti = lk;
  uint32_t soffA = 0;
  {
    uint32_t const v0 = tab[ti] + sg.cX;
    bfMfmaRequestAQ<MS, QT, 0>(a, aq, sg, voffAq, soffA);
    bfMfmaRequestX<0>(x, sg, v0);
    bfMfmaRequestX<1>(x, sg, v0);
    bfMfmaRequestX<2>(x, sg, v0);
    bfMfmaRequestX<3>(x, sg, v0);
  }
  uint32_t t1 = tab[ti + 4], t2 = tab[ti + 8];      // read an iteration ahead of their use
  ti += 12;
  for (uint32_t ks = 0; ks < sg.ksteps; ks += 2) {
    uint32_t const v1 = t1 + sg.cX, v2 = t2 + sg.cX;
    t1 = tab[ti];                                    // the table is padded past the last k-step (BF_MF_TABPAD)
    t2 = tab[ti + 4];
    ti += 8;
    soffA += sg.stepA;
    __builtin_amdgcn_sched_barrier(0);
    bfMfmaRequestAQ<MS, QT, 1>(a, aq, sg, voffAq, soffA);
    __builtin_amdgcn_sched_barrier(0);
    bfMfmaTileQ<MS, QT, 0, 0>(acc, accq, a, aq, x, as, asq, sg, v1);
    bfMfmaTileQ<MS, QT, 0, 1>(acc, accq, a, aq, x, as, asq, sg, v1);
    bfMfmaTileQ<MS, QT, 0, 2>(acc, accq, a, aq, x, as, asq, sg, v1);
    bfMfmaTileQ<MS, QT, 0, 3>(acc, accq, a, aq, x, as, asq, sg, v1);
    soffA += sg.stepA;
    bfMfmaRequestAQ<MS, QT, 0>(a, aq, sg, voffAq, soffA);
    __builtin_amdgcn_sched_barrier(0);
    bfMfmaTileQ<MS, QT, 1, 0>(acc, accq, a, aq, x, as, asq, sg, v2);
    bfMfmaTileQ<MS, QT, 1, 1>(acc, accq, a, aq, x, as, asq, sg, v2);
    bfMfmaTileQ<MS, QT, 1, 2>(acc, accq, a, aq, x, as, asq, sg, v2);
    bfMfmaTileQ<MS, QT, 1, 3>(acc, accq, a, aq, x, as, asq, sg, v2);
  }
  // the requests of the k-steps past the end (set 0 of the leaf fragments, every X tile) must land before the registers are used again
  if (MS > 0) asm volatile("s_waitcnt vmcnt(0)" : "+v"(a[0].u) :: "memory");
  if (QT == 1) asm volatile("s_waitcnt vmcnt(0)" : "+v"(aq[0][0].u), "+v"(x[0].u), "+v"(x[1].u), "+v"(x[2].u), "+v"(x[3].u));
  else if (QT == 2) asm volatile("s_waitcnt vmcnt(0)" : "+v"(aq[0][0].u), "+v"(aq[0][1].u), "+v"(x[0].u), "+v"(x[1].u), "+v"(x[2].u), "+v"(x[3].u));
  else asm volatile("s_waitcnt vmcnt(0)" : "+v"(aq[0][0].u), "+v"(aq[0][1].u), "+v"(aq[0][2].u), "+v"(x[0].u), "+v"(x[1].u), "+v"(x[2].u), "+v"(x[3].u));
}
// the rows of the quarter slabs out of their accumulators: lane (i = lane >> 4, j = lane & 15) holds D[i][j] of every quarter and tile
template <int MS, int QT>
__device__ __forceinline__ void bfMfmaStoreQ(StageParams const &p, BfDevItem const &it, uint32_t mr, uint32_t s0, uint32_t q0, double (&accq)[3][3][4], bool hasIdentity, int lane) {
  uint32_t const nrhs = p.nrhs, np = it.numPieces;
  double2 *out = (it.mrFlags & BF_ITEM_OUT_Y) ? (double2 *)p.y : (double2 *)p.temp;
  uint32_t const qmax = nrhs - 1 - q0;
  uint32_t lane2 = (uint32_t)lane;
  asm volatile("" : "+v"(lane2));
  uint32_t const li2 = lane2 & 15u, lk2 = lane2 >> 4;
#pragma unroll
  for (int q = 0; q < QT; ++q)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      uint32_t const row = s0 + 16u * MS + 4u * q + lk2;
      if (row < mr && 16u * t + li2 <= qmax) {
        double re = accq[0][q][t] - accq[1][q][t];
        double im = accq[2][q][t] - accq[0][q][t] - accq[1][q][t];
        if (hasIdentity) {
          for (uint32_t k = 0; k < np; ++k) {
            BfDevPiece const pc = p.pieces[it.pieceBegin + k];
            if (!(pc.flags & BF_PIECE_IDENTITY)) continue;
            double2 const *xin = (pc.flags & BF_PIECE_IN_X) ? (double2 const *)p.x : (double2 const *)p.temp;
            double2 xv = xin[((uint64_t)pc.inOff + row) * nrhs + q0 + 16 * t + li2];
            re += xv.x; im += xv.y;
          }
        }
        out[((uint64_t)it.outOff + row) * nrhs + q0 + 16 * t + li2] = make_double2(re, im);
      }
    }
}

// The pass's rows x right-hand sides out of the accumulators (Gauss: Re = T1 - T2, Im = T3 - T1 - T2) into y / the intermediate.
template <int NT, int MS, bool GAUSS>
__device__ __forceinline__ void bfMfmaStore(StageParams const &p, BfDevItem const &it, uint32_t mr, uint32_t s0, uint32_t q0, bf_d4 (&acc)[3][2][4], bool hasIdentity, int lane) {
  uint32_t const nrhs = p.nrhs, np = it.numPieces;
  double2 *out = (it.mrFlags & BF_ITEM_OUT_Y) ? (double2 *)p.y : (double2 *)p.temp;
  uint32_t const qmax = nrhs - 1 - q0;
  // (the lane's coordinates are derived again from an opaque copy: hipcc otherwise computes the store addresses
  // before the k-loop and carries them through it, which costs the third wavefront per SIMD)
  uint32_t lane2 = (uint32_t)lane;
  asm volatile("" : "+v"(lane2));
  uint32_t const li2 = lane2 & 15u, lk2 = lane2 >> 4;
#pragma unroll
  for (int m = 0; m < MS; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        uint32_t const row = s0 + 16u * m + 4 * v + lk2;
        if (row < mr && 16u * t + li2 <= qmax) {
          double re = GAUSS ? acc[0][m][t][v] - acc[1][m][t][v] : acc[0][m][t][v];
          double im = GAUSS ? acc[2][m][t][v] - acc[0][m][t][v] - acc[1][m][t][v] : acc[1][m][t][v];
          if (hasIdentity) {      // rare (real-operand zoo; complex operands have none)
            for (uint32_t k = 0; k < np; ++k) {
              BfDevPiece const pc = p.pieces[it.pieceBegin + k];
              if (!(pc.flags & BF_PIECE_IDENTITY)) continue;
              double2 const *xin = (pc.flags & BF_PIECE_IN_X) ? (double2 const *)p.x : (double2 const *)p.temp;
              double2 xv = xin[((uint64_t)pc.inOff + row) * nrhs + q0 + 16 * t + li2];
              re += xv.x; im += xv.y;
            }
          }
          out[((uint64_t)it.outOff + row) * nrhs + q0 + 16 * t + li2] = make_double2(re, im);
        }
      }
  // (stores and fragment requests share vmcnt: the NEXT pass of the wavefront, if there is one, waits for these stores before it
  //  requests anything -- bfMfmaPass; the last pass ends with its stores in flight and frees its slot that much earlier)
}

// One pass = rows [s0, s0 + 16 MS) x RHS [q0, q0 + 16 NT) of one item, over all its segments.
// (QT > 0: MS = 0 or 1 full slabs and QT quarter slabs on v_mfma_f64_4x4x4, four tiles, Gauss -- bfMfmaSegmentQ)
template <int NT, int MS, bool GAUSS, int QT = 0>
__device__ __forceinline__ void bfMfmaPass(StageParams const &p, BfDevItem const &it, uint32_t mr, uint32_t s0, uint32_t q0, uint32_t *tab, int lane) {
  static_assert(QT == 0 || (NT == 4 && MS <= 1 && GAUSS), "quarter slabs: the 4-tile Gauss register loop");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the stores of the wavefront's previous pass: nothing may be pending when the k-loop counts
  uint32_t const nrhs = p.nrhs;
  uint32_t const li = lane & 15, lk = lane >> 4;
  bf_d4 acc[3][2][4];            // T1 = sum Ar Xr, T2 = sum Ai Xi, T3 = sum (Ar + Ai)(Xr + Xi)
  bf_d4 accs[3][4];              // QT > 0: the one full slab
  double accq[3][3][4];          // QT > 0: the quarter slabs
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int m = 0; m < MS; ++m)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[g][m][t] = (bf_d4){0, 0, 0, 0};
  if (QT > 0) {
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        accs[g][t] = (bf_d4){0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 3; ++q) accq[g][q][t] = 0.0;
      }
  }
  bool hasIdentity = false;
  uint32_t const np = it.numPieces;
  uint32_t const spanRows = BF_MF_SPAN_BYTES / (nrhs * 16u);
  uint32_t pi = 0;
  while (pi < np) {
    // ---- the next segment: its row table into LDS, its extent into scalars.  (The descriptor window is loaded
    // again for every segment: six registers that must not stay live across the k-loop.)
    uint32_t cols = 0, minRow = 0, maxRow = 0, inX = 0;
    uint64_t aOff = 0, expect = 0;
    bool started = false;
    BfPieceWin win;
    uint32_t wbase = 0xffffff00u;
    while (pi < np) {
      if (pi - wbase >= 64u) {
        wbase = pi;
        win = bfPieceWinLoad(p.pieces + it.pieceBegin + wbase, np - wbase < 64u ? np - wbase : 64u, lane);
      }
      BfDevPiece const pc = bfPieceWinGet(win, pi - wbase);
      if (pc.flags & BF_PIECE_IDENTITY) { hasIdentity = true; ++pi; continue; }
      uint32_t const px = pc.flags & BF_PIECE_IN_X, last = pc.inOff + pc.ncols - 1;
      uint32_t lo = pc.inOff, hi = last;
      if (started) {
        if (pc.dataOff != expect || px != inX || cols + pc.ncols > BF_MF_TABCAP) break;
        lo = minRow < lo ? minRow : lo;
        hi = maxRow > hi ? maxRow : hi;
        if (hi - lo >= spanRows) break;
      } else {
        started = true;
        aOff = pc.dataOff;
        inX = px;
      }
      minRow = lo;
      maxRow = hi;
      for (uint32_t j = (uint32_t)lane; j < pc.ncols; j += 64u) tab[cols + j] = pc.inOff + j;
      cols += pc.ncols;
      expect = pc.dataOff + (uint64_t)mr * pc.ncols;
      ++pi;
    }
    if (!cols) break;                      // identity pieces only
    // columns past the end: the leaf fragment is zero there (range check), any row of the segment will do
    if ((uint32_t)lane < BF_MF_TABPAD) tab[cols + lane] = minRow;
    waveSync();
    // rows -> byte offsets from the segment's first row (fits 32 bits: spanRows)
    for (uint32_t j = (uint32_t)lane; j < cols + BF_MF_TABPAD; j += 64u) tab[j] = (tab[j] - minRow) * (nrhs * 16u);
    waveSync();
    BfMfSeg sg;
    sg.stepA = 4u * mr * 16u;
    sg.ksteps = (cols + 3u) / 4u;
    sg.ra = bfMakeRsrc((double2 const *)p.arena + aOff, mr * cols * 16u);
    char const *xin = inX ? (char const *)p.x : (char const *)p.temp;
    // the last row ends with this pass's RHS (lanes past nrhs read zeros there, the next row's values elsewhere:
    // columns of the product that are never stored)
    sg.rx = bfMakeRsrc(xin + ((uint64_t)minRow * nrhs + q0) * 16u, ((maxRow - minRow) * nrhs + (nrhs - q0)) * 16u);
    sg.voffA = (lk * mr + s0 + li) * 16u;          // rows past the item's end alias the next column: rows of the product that are never stored
    sg.cX = li * 16u;
    if constexpr (QT > 0) bfMfmaSegmentQ<MS, QT>(accs, accq, sg, (lk * mr + s0 + (li & 3u)) * 16u, tab, lk);      // a quarter fragment: row (lane & 3) of its four
    else bfMfmaSegment<NT, MS, GAUSS>(acc, sg, tab, lk);
    waveSync();                                      // the table is rewritten by the next segment
  }
  if constexpr (QT > 0) {
    bfMfmaStoreQ<MS, QT>(p, it, mr, s0, q0, accq, hasIdentity, lane);
    if (MS > 0) {
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[g][0][t] = accs[g][t];
    }
  }
  bfMfmaStore<NT, MS, GAUSS>(p, it, mr, s0, q0, acc, hasIdentity, lane);
}

template <int MS, int MAXNT, bool GAUSS>
__device__ __forceinline__ void bfMfmaDispatch(uint32_t nt, StageParams const &p, BfDevItem const &it, uint32_t mr, uint32_t s0, uint32_t q0, uint32_t *tab, int lane) {
  if (MAXNT >= 4 && nt == 4) bfMfmaPass<4, MS, GAUSS>(p, it, mr, s0, q0, tab, lane);
  else if (MAXNT >= 3 && nt == 3) bfMfmaPass<3, MS, GAUSS>(p, it, mr, s0, q0, tab, lane);
  else if (MAXNT >= 2 && nt == 2) bfMfmaPass<2, MS, GAUSS>(p, it, mr, s0, q0, tab, lane);
  else bfMfmaPass<1, MS, GAUSS>(p, it, mr, s0, q0, tab, lane);
}

// MAXNT = the widest pass the launch needs (RHS tiles of 16): the accumulators of 4 tiles x 2 slabs x 3 products leave two
// wavefronts per SIMD, which is what the matrix pipe needs at 64 RHS -- but with 2 - 32 RHS the kernel is bound by the leaf
// stream, not by the pipe, and then it is wavefronts (bytes in flight) that count: the 1- and 2-tile instantiations need
// a third / half of the registers and run WAVES = 5 / 3 wavefronts per SIMD (N = 262144: 2 - 16 RHS 14.3 - 15.9 -> see
// DESIGN_EXPERIMENTS.md section 4).
template <int MAXNT, int WAVES, bool GAUSS = true>
__device__ __forceinline__ void bfStageBodyC128Mfma(StageParams const &p, uint32_t (*tabs)[BF_MF_TABCAP + BF_MF_TABPAD]) {
  int const lane = threadIdx.x & 63;
  uint32_t const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t *tab = tabs[wave];
  // The wavefronts of a workgroup take neighbours of the item list: row chunks of one row group and of its sibling
  // groups (same cost, same input rows: the planner's order for RHS-block operators).  Workgroups are dealt to the 8 XCDs
  // round robin: runs of BF_MF_XCD_RUN workgroups that are neighbours in the list go to ONE XCD, so that a row of X is
  // fetched into that L2 once for all of them.
  uint32_t wg = blockIdx.x;
  uint32_t const numWg = (p.numItems + BF_MF_WG_WAVES - 1u) / BF_MF_WG_WAVES;
  if (BF_MF_XCD_RUN > 1) {
    uint32_t const blk = 8u * BF_MF_XCD_RUN;
    if (wg < numWg / blk * blk) { uint32_t const r = wg % blk; wg = wg - r + (r % 8u) * BF_MF_XCD_RUN + r / 8u; }
  }
  uint32_t const item = wg * BF_MF_WG_WAVES + wave;
  if (item >= p.numItems) return;
  BfDevItem const it = p.items[item];
  uint32_t const mr = it.mrFlags & 0xffffu;
  uint32_t const nrhs = p.nrhs;
  for (uint32_t q0 = 0; q0 < nrhs; q0 += 64) {
    uint32_t const nt = (nrhs - q0 >= 64) ? 4u : (nrhs - q0 + 15u) / 16u;
    uint32_t s0 = 0;
    while (s0 < mr) {
      uint32_t const left = mr - s0;
      if (BF_MF_QUARTER && MAXNT == 4 && GAUSS && nt == 4 && left < 32 && (left & 15u) && (left & 15u) <= 12u) {
        // the last pass of the item ends in 1 ... 12 rows: quarter slabs (v_mfma_f64_4x4x4) instead of a mostly padded full one
        if constexpr (MAXNT == 4 && GAUSS) {
          uint32_t const qt = ((left & 15u) + 3u) / 4u;
          if (left > 16) {
            if (qt == 1) bfMfmaPass<4, 1, true, 1>(p, it, mr, s0, q0, tab, lane);
            else if (qt == 2) bfMfmaPass<4, 1, true, 2>(p, it, mr, s0, q0, tab, lane);
            else bfMfmaPass<4, 1, true, 3>(p, it, mr, s0, q0, tab, lane);
          } else {
            if (qt == 1) bfMfmaPass<4, 0, true, 1>(p, it, mr, s0, q0, tab, lane);
            else if (qt == 2) bfMfmaPass<4, 0, true, 2>(p, it, mr, s0, q0, tab, lane);
            else bfMfmaPass<4, 0, true, 3>(p, it, mr, s0, q0, tab, lane);
          }
        }
        s0 = mr;
      }
      else if (left > 16) { bfMfmaDispatch<2, MAXNT, GAUSS>(nt, p, it, mr, s0, q0, tab, lane); s0 += 32; }
      else { bfMfmaDispatch<1, MAXNT, GAUSS>(nt, p, it, mr, s0, q0, tab, lane); s0 += 16; }
    }
  }
}

// The k-loop of the 4-tile kernel.  Measured (tools/mfma_loop_probe.hip with --pmc, profiles/r5_mfma_loop_probe*.json): the register
// loop keeps the matrix pipe busy 0.93 - 0.94 of the cycles WHEREVER its operands come from -- it is not bound by their latency --
// and what the traffic beyond L2 costs is CLOCK: 2.37 GHz with the leaf stream and the X rows in L2, 2.23 with the leaf stream from HBM,
// 2.06 / 2.04 with the X rows from the Infinity Cache / HBM as well.  The LDS-ring loop (tools/mfma_setaside_loops.h) holds the same
// clocks and loses 4 % of the pipe to the ds_read bubble at the top of each k-step (busy 0.89): prefetching deeper buys nothing here.
__global__ __launch_bounds__(64 * BF_MF_WG_WAVES) __attribute__((amdgpu_waves_per_eu(BF_MFMA_WAVES_PER_SIMD, BF_MFMA_WAVES_PER_SIMD))) void bfStageKernelC128Mfma(StageParams p) {
  __shared__ uint32_t tabs[BF_MF_WG_WAVES][BF_MF_TABCAP + BF_MF_TABPAD];
  bfStageBodyC128Mfma<4, BF_MFMA_WAVES_PER_SIMD>(p, tabs);
}
// <= 32 right-hand sides (2 tiles): 3 wavefronts per SIMD
__global__ __launch_bounds__(64 * BF_MF_WG_WAVES) __attribute__((amdgpu_waves_per_eu(3, 3))) void bfStageKernelC128Mfma2(StageParams p) {
  __shared__ uint32_t tabs[BF_MF_WG_WAVES][BF_MF_TABCAP + BF_MF_TABPAD];
  bfStageBodyC128Mfma<2, 3>(p, tabs);
}
// <= 16 right-hand sides (1 tile): 5 wavefronts per SIMD
__global__ __launch_bounds__(64 * BF_MF_WG_WAVES) __attribute__((amdgpu_waves_per_eu(5, 5))) void bfStageKernelC128Mfma1(StageParams p) {
  __shared__ uint32_t tabs[BF_MF_WG_WAVES][BF_MF_TABCAP + BF_MF_TABPAD];
  bfStageBodyC128Mfma<1, 5>(p, tabs);
}
// BFHIP_FLAG_EXACT_COMPLEX: the same three kernels with the four real products of every complex one (componentwise zgemm's recurrence)
__global__ __launch_bounds__(64 * BF_MF_WG_WAVES) __attribute__((amdgpu_waves_per_eu(BF_MFMA_WAVES_PER_SIMD, BF_MFMA_WAVES_PER_SIMD))) void bfStageKernelC128MfmaExact(StageParams p) {
  __shared__ uint32_t tabs[BF_MF_WG_WAVES][BF_MF_TABCAP + BF_MF_TABPAD];
  bfStageBodyC128Mfma<4, BF_MFMA_WAVES_PER_SIMD, false>(p, tabs);
}
__global__ __launch_bounds__(64 * BF_MF_WG_WAVES) __attribute__((amdgpu_waves_per_eu(3, 3))) void bfStageKernelC128Mfma2Exact(StageParams p) {
  __shared__ uint32_t tabs[BF_MF_WG_WAVES][BF_MF_TABCAP + BF_MF_TABPAD];
  bfStageBodyC128Mfma<2, 3, false>(p, tabs);
}
__global__ __launch_bounds__(64 * BF_MF_WG_WAVES) __attribute__((amdgpu_waves_per_eu(5, 5))) void bfStageKernelC128Mfma1Exact(StageParams p) {
  __shared__ uint32_t tabs[BF_MF_WG_WAVES][BF_MF_TABCAP + BF_MF_TABPAD];
  bfStageBodyC128Mfma<1, 5, false>(p, tabs);
}
#endif
