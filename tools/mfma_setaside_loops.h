// mfma_setaside_loops.h -- two k-loops of the complex128 64-RHS stage kernel that were built, measured slower than the product's
// register loop (bfMfmaSegment of butterfly_amd/csrc/bfhip_stage_mfma.h) and set aside in round 5.  Only the bare loops are here, for
// the probes that measure them and compare them bit for bit with the product's loop:
//   * bfMfmaSegmentDma (tools/mfma_loop_probe.hip): every fragment prefetched through a two-slot LDS ring per wavefront;
//   * bfSxSegment (tools/mfma_sharedx_probe.hip): the X tiles of a k-step fetched once per workgroup of four wavefronts.
// Include it after bfhip_stage_c128.h and bfhip_stage_mfma.h; nothing under butterfly_amd/ includes it.  The kernels that ran these
// loops on real stages (pass, body and __global__ definitions behind -DBF_MF_DMA=1 / -DBF_MF_BUNDLES=1, and the device copy of the
// planner's bundle table they read) are gone from the tree: commit 4d8b3c1 is the last one that holds them, and DESIGN.md section 9
// and profiles/r5_mfma_loop_probe*.json, profiles/r5_bundle_kernel_experiment.json keep what they measured.
#ifndef MFMA_SETASIDE_LOOPS_H
#define MFMA_SETASIDE_LOOPS_H

// ---- the same k-loop with its fragments prefetched through LDS (round 5: built, measured, NOT the product's loop) -------------------
// The question it answers (tools/mfma_loop_probe.hip: the loops on the bare machine, no items, no tables rebuilt, no tails): the
// register loop reaches 0.88 of the FP64 matrix peak with the leaf fragments streamed from HBM, 0.80 when the X rows miss L2 and
// 0.93 when the leaf fragments come from L2 -- is that the latency of requests made only one k-step (24 MFMAs = 1536 cycles of a
// SIMD that two wavefronts share, ~1.3 us) ahead?  Requests return in order (one counter), so a deeper prefetch needs a place to
// land that is not a register: every fragment of k-step ks + 2 is requested, during k-step
// ks, as an LDS-DMA (buffer_load ... lds: no VGPR destination) into a ring of two 6 KiB slots per wavefront; at the top of a k-step
// its slot is complete (s_waitcnt vmcnt(F): only the F requests of the next k-step may be pending), the fragments are read with six
// ds_read_b128 into ONE register set, the slot is handed to the requests of k-step ks + 2 right away, and the MFMAs run from
// registers.  Same MFMAs in the same order: bit-identical to bfMfmaSegment (the probe compares them on ragged segments).  2 x 6 KiB
// + the 7.1 KiB table per one-wavefront workgroup: eight of them (two per SIMD) fit a CU's 160 KiB.
// The answer is NO: with twice the prefetch distance the leaf stream from HBM and the X rows from beyond L2 cost exactly what they
// cost the register loop (counters: the same clocks, see the note after the loop), and the ds_read bubble costs 4 % on top.
//   * LDS-DMA writes M0 + lane * 16 (M0 is written in the statement that uses it: the compiler does not keep it); every instruction
//     uses offset:0, tile / slab offsets travel in the SGPR offset.
//   * Columns / rows past the end of the segment: out-of-range lanes of an LDS-DMA deliver zeros like a register load (probed:
//     tools/mfma_loop_probe.hip `dma_oob`), the padded table rows are rows of the segment.
#define BF_MF_DMA_SLOT 6144u            /* MS + NT <= 6 fragments of 1 KiB */
#define BF_MF_DMA_RING (2u * BF_MF_DMA_SLOT)
template <int STREAM> __device__ __forceinline__ void bfDmaLoad(uint32_t ldsDst, uint32_t voff, bf_i4 rsrc, uint32_t soff) {
  if (STREAM) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen nt lds" :: "s"(ldsDst), "v"(voff), "s"(rsrc), "s"(soff));
  else asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(ldsDst), "v"(voff), "s"(rsrc), "s"(soff));
}
// All R = MS + NT fragments of a slot into registers: the wait for the slot's LDS-DMAs, the ds_reads and the wait for THEIR data are
// ONE asm statement with early-clobber outputs -- hipcc treats an asm output as written when the statement ends, and with the
// wait in a statement of its own it is free to copy a fragment register before the data has landed (it did: v_mov of the A fragment
// between the ds_read and the s_waitcnt in the instantiations that needed a copy; cdna_hip_programming.md section 5.7 item 1).
template <int R, int BASE> __device__ __forceinline__ void bfLdsReadSlot(BfFrag (&f)[6], uint32_t laneLds) {
  static_assert(R >= 2 && R <= 6, "one to two slabs, one to four tiles");
  if constexpr (R == 6)
    asm volatile("s_waitcnt vmcnt(6)\n\tds_read_b128 %0, %6 offset:%7\n\tds_read_b128 %1, %6 offset:%8\n\tds_read_b128 %2, %6 offset:%9\n\tds_read_b128 %3, %6 offset:%10\n\t"
                 "ds_read_b128 %4, %6 offset:%11\n\tds_read_b128 %5, %6 offset:%12\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(f[0].u), "=&v"(f[1].u), "=&v"(f[2].u), "=&v"(f[3].u), "=&v"(f[4].u), "=&v"(f[5].u)
                 : "v"(laneLds), "n"(BASE), "n"(BASE + 1024), "n"(BASE + 2048), "n"(BASE + 3072), "n"(BASE + 4096), "n"(BASE + 5120));
  else if constexpr (R == 5)
    asm volatile("s_waitcnt vmcnt(5)\n\tds_read_b128 %0, %5 offset:%6\n\tds_read_b128 %1, %5 offset:%7\n\tds_read_b128 %2, %5 offset:%8\n\tds_read_b128 %3, %5 offset:%9\n\t"
                 "ds_read_b128 %4, %5 offset:%10\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(f[0].u), "=&v"(f[1].u), "=&v"(f[2].u), "=&v"(f[3].u), "=&v"(f[4].u)
                 : "v"(laneLds), "n"(BASE), "n"(BASE + 1024), "n"(BASE + 2048), "n"(BASE + 3072), "n"(BASE + 4096));
  else if constexpr (R == 4)
    asm volatile("s_waitcnt vmcnt(4)\n\tds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\tds_read_b128 %3, %4 offset:%8\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(f[0].u), "=&v"(f[1].u), "=&v"(f[2].u), "=&v"(f[3].u)
                 : "v"(laneLds), "n"(BASE), "n"(BASE + 1024), "n"(BASE + 2048), "n"(BASE + 3072));
  else if constexpr (R == 3)
    asm volatile("s_waitcnt vmcnt(3)\n\tds_read_b128 %0, %3 offset:%4\n\tds_read_b128 %1, %3 offset:%5\n\tds_read_b128 %2, %3 offset:%6\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(f[0].u), "=&v"(f[1].u), "=&v"(f[2].u)
                 : "v"(laneLds), "n"(BASE), "n"(BASE + 1024), "n"(BASE + 2048));
  else
    asm volatile("s_waitcnt vmcnt(2)\n\tds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(f[0].u), "=&v"(f[1].u)
                 : "v"(laneLds), "n"(BASE), "n"(BASE + 1024));
}
// (a buffer instruction's scalar offset is an SGPR or an inline constant, never a literal: the tile offsets are made opaque to hipcc)
template <uint32_t V> __device__ __forceinline__ uint32_t bfSgprConst() { uint32_t v; asm("s_movk_i32 %0, %1" : "=s"(v) : "n"(V)); return v; }
template <int NT, int MS, int SLOT>
__device__ __forceinline__ void bfMfmaDmaRequest(BfMfSeg const &sg, uint32_t ring, uint32_t soffA, uint32_t voffX) {
  constexpr uint32_t base = SLOT * BF_MF_DMA_SLOT;
  bfDmaLoad<1>(ring + base, sg.voffA, sg.ra, soffA);
  if (MS > 1) bfDmaLoad<1>(ring + base + 1024u, sg.voffA, sg.ra, soffA + 256u);
  bfDmaLoad<0>(ring + base + MS * 1024u, voffX, sg.rx, bfSgprConst<0>());
  if (NT > 1) bfDmaLoad<0>(ring + base + (MS + 1) * 1024u, voffX, sg.rx, bfSgprConst<256>());
  if (NT > 2) bfDmaLoad<0>(ring + base + (MS + 2) * 1024u, voffX, sg.rx, bfSgprConst<512>());
  if (NT > 3) bfDmaLoad<0>(ring + base + (MS + 3) * 1024u, voffX, sg.rx, bfSgprConst<768>());
}
// one k-step out of slot SLOT; soffA / voffX: what is requested into the slot once it has been read (k-step + 2)
template <int NT, int MS, int SLOT, bool GAUSS>
__device__ __forceinline__ void bfMfmaDmaStep(bf_d4 (&acc)[3][2][4], BfMfSeg const &sg, uint32_t ring, uint32_t laneLds, uint32_t soffA, uint32_t voffX) {
  constexpr uint32_t base = SLOT * BF_MF_DMA_SLOT;
  // this slot's MS + NT requests are the oldest (complete once only the other slot's may be pending): wait, read, wait -- one statement
  BfFrag f[6];
  bfLdsReadSlot<MS + NT, base>(f, laneLds);
  BfFrag (&a)[6] = f;
  BfFrag *const x = f + MS;
  __builtin_amdgcn_sched_barrier(0);
  bfMfmaDmaRequest<NT, MS, SLOT>(sg, ring, soffA, voffX);        // the slot is free: everything of it is in registers
  __builtin_amdgcn_sched_barrier(0);
  if (GAUSS) {
    double as[2];
    as[0] = a[0].d[0] + a[0].d[1];
    if (MS > 1) as[1] = a[1].d[0] + a[1].d[1];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      double const xs = x[t].d[0] + x[t].d[1];
#pragma unroll
      for (int m = 0; m < MS; ++m) {
        acc[0][m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m].d[0], x[t].d[0], acc[0][m][t], 0, 0, 0);
        acc[1][m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m].d[1], x[t].d[1], acc[1][m][t], 0, 0, 0);
        acc[2][m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[m], xs, acc[2][m][t], 0, 0, 0);
      }
    }
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int m = 0; m < MS; ++m) bfMfmaExact(acc[0][m][t], acc[1][m][t], a[m], x[t]);
  }
  __builtin_amdgcn_sched_barrier(0);
}
template <int NT, int MS, bool GAUSS = true>
__device__ __forceinline__ void bfMfmaSegmentDma(bf_d4 (&acc)[3][2][4], BfMfSeg const &sg, uint32_t const *tab, uint32_t lk, uint32_t ring, uint32_t laneLds) {
  uint32_t ti = lk;
  uint32_t soffA = 0;
  bfMfmaDmaRequest<NT, MS, 0>(sg, ring, soffA, tab[ti] + sg.cX);
  soffA += sg.stepA;
  bfMfmaDmaRequest<NT, MS, 1>(sg, ring, soffA, tab[ti + 4] + sg.cX);
  soffA += sg.stepA;
  uint32_t t2 = tab[ti + 8], t3 = tab[ti + 12];      // the rows of k-steps 2 and 3, read an iteration ahead of their use
  ti += 16;
  for (uint32_t ks = 0; ks < sg.ksteps; ks += 2) {
    uint32_t const v2 = t2 + sg.cX, v3 = t3 + sg.cX;
    t2 = tab[ti];                                     // the table is padded past the last k-step (BF_MF_TABPAD)
    t3 = tab[ti + 4];
    ti += 8;
    bfMfmaDmaStep<NT, MS, 0, GAUSS>(acc, sg, ring, laneLds, soffA, v2);
    soffA += sg.stepA;
    bfMfmaDmaStep<NT, MS, 1, GAUSS>(acc, sg, ring, laneLds, soffA, v3);
    soffA += sg.stepA;
  }
  // the requests of the k-steps past the end must land before the ring (and the table) are used again
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Which loop the 4-tile kernel runs, measured (tools/mfma_loop_probe.hip with --pmc, profiles/r5_mfma_loop_probe*.json): the register
// loop keeps the matrix pipe busy 0.93 - 0.94 of the cycles WHEREVER its operands come from -- it is not bound by their latency --
// and what the traffic beyond L2 costs is CLOCK: 2.37 GHz with the leaf stream and the X rows in L2, 2.23 with the leaf stream from HBM,
// 2.06 / 2.04 with the X rows from the Infinity Cache / HBM as well.  The LDS-ring loop holds the same clocks and loses 4 % of the
// pipe to the ds_read bubble at the top of each k-step (busy 0.89): prefetching deeper buys nothing here.

// ---- bundles (round 5: built, measured, NOT the product's kernel; only the shared-X k-loop is kept here) -----------------------------
// A workgroup of four wavefronts whose items read the SAME X rows.  The row chunks of a row group and the sibling groups of a radix-4
// stage (reference src/fac_helm2.c:277-318) multiply different leaf rows by the same rows of the input; the planner keeps them
// together in the list and bfPlanBundles marks runs of four with equal inputs, <= 32 rows and the same number of slabs (SHARED
// bundles: ONE pass each, the same number of k-steps); everything else went four unrelated items to a workgroup (MIXED bundles, the
// one-wavefront passes of bfMfmaPass -- a workgroup must keep its four wavefronts alive: a new workgroup needs a free slot on EVERY SIMD
// (tools/wave_placement_probe.hip: its four wavefronts always land on four different SIMDs), so survivors of workgroups whose other
// wavefronts had exited block the CU as soon as one SIMD holds two of them -- such workgroups ran at a fifth of the rate).  In a shared bundle every wavefront streams its own leaf fragments into registers exactly as bfMfmaSegment does; the
// four X tiles of a k-step are fetched ONCE per workgroup -- wavefront w brings tile w as an LDS-DMA, two k-steps ahead, into a ring of
// three 4 KiB slots -- and every wavefront reads them with ds_read_b128 right after the MFMAs that used the previous k-step's copy.
// One workgroup barrier per k-step: behind it the next k-step's slot is complete and nobody still reads the slot before the current
// one, which is the one requested into next.  Same MFMAs in the same order per accumulator: bit-identical to the register loop
// (tools/mfma_sharedx_probe.hip compares them; the GPU suite passed with either kernel).
// What it does (N = 262144, 64 RHS, counters over the shared bundles alone, 83 - 93 % of a stage's work): HBM traffic 1.08x the
// algorithmic bytes instead of 1.4x, clock +6 % -- and the matrix pipe busy 0.80 of the cycles instead of 0.87: four wavefronts
// that wait for each other at every k-step and at every segment's first requests (and, in the first version, for the ONE table that
// wavefront 0 wrote: every wavefront writes its own copy now, 1 % of the apply).
// On the bare machine (the probe: no items, no tables) the loop is 9 - 17 % faster than the register loop; in the kernel the shared
// bundles are 2 - 5 % faster per unit of work, the mixed ones 2 % slower than one-wavefront workgroups, the whole apply 30.65 - 30.88 ms
// against 30.13 - 30.22 for the one-wavefront kernel, same box.  Not the barrier itself (without it, wrong results: the same time) and
// not the order of the bundles (shuffled inside their cost buckets: the same time).  DESIGN.md section 9.
#define BF_MF_SX_SLOT 4096u
#define BF_MF_SX_RING (3u * BF_MF_SX_SLOT)

template <int MS, int SET, bool GAUSS>
__device__ __forceinline__ void bfSxStep(bf_d4 (&acc)[3][2][4], BfFrag (&a)[2][2], BfFrag (&x)[4], BfMfSeg const &sg, uint32_t &soffA, uint32_t voffXnext2,
                                         uint32_t slotNext, uint32_t slotFree, uint32_t laneLds, uint32_t mine) {
  // everything this wavefront asked for has arrived: the leaf fragments of this k-step, its tiles of the NEXT k-step's X (LDS-DMA),
  // the X fragments of this k-step (ds_read) ...
  if (MS > 1) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(a[SET][0].u), "+v"(a[SET][1].u), "+v"(x[0].u), "+v"(x[1].u), "+v"(x[2].u), "+v"(x[3].u));
  else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(a[SET][0].u), "+v"(x[0].u), "+v"(x[1].u), "+v"(x[2].u), "+v"(x[3].u));
  // ... and everybody else's
  asm volatile("s_barrier" ::: "memory");
  soffA += sg.stepA;
  bfMfmaRequestA<MS, SET ^ 1>(a, sg, soffA);
  if (mine & 1u) bfDmaLoad<0>(slotFree, voffXnext2, sg.rx, bfSgprConst<0>());
  if (mine & 2u) bfDmaLoad<0>(slotFree + 1024u, voffXnext2, sg.rx, bfSgprConst<256>());
  if (mine & 4u) bfDmaLoad<0>(slotFree + 2048u, voffXnext2, sg.rx, bfSgprConst<512>());
  if (mine & 8u) bfDmaLoad<0>(slotFree + 3072u, voffXnext2, sg.rx, bfSgprConst<768>());
  uint32_t const vaddr = laneLds + slotNext;
  double as[2];
  if (GAUSS) {
    as[0] = a[SET][0].d[0] + a[SET][0].d[1];
    if (MS > 1) as[1] = a[SET][1].d[0] + a[SET][1].d[1];
  }
  __builtin_amdgcn_sched_barrier(0);
#define BF_SX_TILE(T) do { \
    if (GAUSS) { \
      double const xs = x[T].d[0] + x[T].d[1]; \
      _Pragma("unroll") for (int m = 0; m < MS; ++m) { \
        acc[0][m][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[SET][m].d[0], x[T].d[0], acc[0][m][T], 0, 0, 0); \
        acc[1][m][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[SET][m].d[1], x[T].d[1], acc[1][m][T], 0, 0, 0); \
        acc[2][m][T] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[m], xs, acc[2][m][T], 0, 0, 0); \
      } \
    } else { \
      _Pragma("unroll") for (int m = 0; m < MS; ++m) bfMfmaExact(acc[0][m][T], acc[1][m][T], a[SET][m], x[T]); \
    } \
    __builtin_amdgcn_sched_barrier(0); \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(x[T].u) : "v"(vaddr), "n"(1024 * T)); \
    __builtin_amdgcn_sched_barrier(0); \
  } while (0)
  BF_SX_TILE(0); BF_SX_TILE(1); BF_SX_TILE(2); BF_SX_TILE(3);
#undef BF_SX_TILE
}

// the k-loop of one segment for one wavefront of a bundle (4 tiles, MS slabs); `mine`: bit t = this wavefront fetches tile t
template <int MS, bool GAUSS>
__device__ __forceinline__ void bfSxSegment(bf_d4 (&acc)[3][2][4], BfMfSeg const &sg, uint32_t const *tab, uint32_t lk, uint32_t ring, uint32_t lane, uint32_t mine) {
  BfFrag a[2][2], x[4];
  uint32_t const laneLds = lane * 16u;
  uint32_t ti = lk, soffA = 0;
  uint32_t s0 = ring, s1 = ring + BF_MF_SX_SLOT, s2 = ring + 2u * BF_MF_SX_SLOT;      // slots of k-steps ks, ks + 1, ks + 2 (wave-uniform)
  {
    uint32_t const v0 = tab[ti] + sg.cX, v1 = tab[ti + 4] + sg.cX;
    if (mine & 1u) { bfDmaLoad<0>(s0, v0, sg.rx, bfSgprConst<0>()); bfDmaLoad<0>(s1, v1, sg.rx, bfSgprConst<0>()); }
    if (mine & 2u) { bfDmaLoad<0>(s0 + 1024u, v0, sg.rx, bfSgprConst<256>()); bfDmaLoad<0>(s1 + 1024u, v1, sg.rx, bfSgprConst<256>()); }
    if (mine & 4u) { bfDmaLoad<0>(s0 + 2048u, v0, sg.rx, bfSgprConst<512>()); bfDmaLoad<0>(s1 + 2048u, v1, sg.rx, bfSgprConst<512>()); }
    if (mine & 8u) { bfDmaLoad<0>(s0 + 3072u, v0, sg.rx, bfSgprConst<768>()); bfDmaLoad<0>(s1 + 3072u, v1, sg.rx, bfSgprConst<768>()); }
  }
  bfMfmaRequestA<MS, 0>(a, sg, soffA);
  uint32_t t2 = tab[ti + 8], t3 = tab[ti + 12];      // the rows of k-steps 2 and 3 (the table is padded past the last k-step: BF_MF_TABPAD)
  ti += 16;
  // (never the same variable twice in one statement: hipcc then copies it BEFORE the wait and may keep the copy)
  if (MS > 1) asm volatile("s_waitcnt vmcnt(0)" : "+v"(a[0][0].u), "+v"(a[0][1].u));
  else asm volatile("s_waitcnt vmcnt(0)" : "+v"(a[0][0].u));
  asm volatile("s_barrier" ::: "memory");
  {
    uint32_t const vaddr = laneLds + s0;
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\tds_read_b128 %2, %4 offset:2048\n\tds_read_b128 %3, %4 offset:3072"
                 : "=&v"(x[0].u), "=&v"(x[1].u), "=&v"(x[2].u), "=&v"(x[3].u) : "v"(vaddr));
  }
  for (uint32_t ks = 0; ks < sg.ksteps; ks += 2) {
    uint32_t const v2 = t2 + sg.cX, v3 = t3 + sg.cX;
    t2 = tab[ti];
    t3 = tab[ti + 4];
    ti += 8;
    bfSxStep<MS, 0, GAUSS>(acc, a, x, sg, soffA, v2, s1, s2, laneLds, mine);
    bfSxStep<MS, 1, GAUSS>(acc, a, x, sg, soffA, v3, s2, s0, laneLds, mine);
    uint32_t const o0 = s0, o1 = s1;
    s0 = s2; s1 = o0; s2 = o1;                       // two k-steps on
  }
  // the requests of the k-steps past the end (zeros from the range check / padded table rows) must land before the registers, the
  // ring and the table are used again, by anybody
  if (MS > 1) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(a[0][0].u), "+v"(a[0][1].u), "+v"(a[1][0].u), "+v"(a[1][1].u), "+v"(x[0].u), "+v"(x[1].u), "+v"(x[2].u), "+v"(x[3].u));
  else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(a[0][0].u), "+v"(a[1][0].u), "+v"(x[0].u), "+v"(x[1].u), "+v"(x[2].u), "+v"(x[3].u));
  asm volatile("s_barrier" ::: "memory");
}

#endif
