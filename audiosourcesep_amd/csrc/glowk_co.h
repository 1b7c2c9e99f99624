// k_net_h3c: the CO-RESIDENT form of the forward coupling network on v_mfma_f32_16x16x32_f16 (round-3 verdict, item 2).
//
// k_net_h3s runs ONE 8-wave / 256-pixel workgroup per CU (255 VGPRs, 105-150 KB of LDS): its gather prologue, the phase barriers of
// all eight waves and the fused coupling tail overlap nothing.  Here a workgroup is FOUR waves / 128 pixels -- one wave per SIMD,
// each wave keeping the two 16-pixel halves of k_net_h3s (same A-fragment reuse, same accumulators, same arithmetic order: results
// are bit for bit those of k_net_h3s) -- and TWO such workgroups share a CU (2 x <= 80 KB of LDS, 2 x 4 waves x 256 VGPRs), each with
// its own barrier domain and its own weight ring, started at different times by the dispatcher: while one gathers, waits at a barrier
// or runs its coupling tail, the other's waves own the matrix pipe.
//
// Ring of 16-KiB UNITS (half a 32-KiB chunk of the NP = 2 image: the row blocks of one half of the pass's hidden half -- the image
// itself is the one k_net_h3s reads).  Per hidden block i of a pass the ops are
//     X_i    conv1 of block i + ReLU + split                      (reads K[i & 1])
//     Ya_i   conv2 contribution of block i to row blocks 0 .. NFH-1        (reads M0 = unit 2 i)
//     Yb_i   ... to row blocks NFH .. 2 NFH - 1                            (reads M1 = unit 2 i + 1)
// then Z_0 .. Z_{NMT-1} (conv3, one unit of NFH tiles each: D, M0, M1).  All four waves run the same op; every op ends with a
// workgroup barrier.  A unit's DMA is issued in the op that follows the barrier after its slot's last reader and has at least
// one X or two Y halves to land:
//     X_i  issues unit 2 i + 1 -> M1      Ya_i issues conv1 operands of block i + 2 -> K[i & 1]      Yb_i issues unit 2 i + 2 -> M0
//     Z_0  issues conv3 unit 2 -> M1      Z_1  issues the next pass's conv3 unit 0 -> D              Z_2  issues the next pass's unit 0 -> M0
// (conv3 unit 0 sits in a slot of its own, D, because nothing separates Yb_{NF-1} from Z_0; conv3 unit 1 -> M0 is issued by Yb_{NF-1}
// as "unit 2 NF").  The waits are counted: vmcnt counts in issue order, so "everything but the n youngest DMA instructions of this
// wave has landed" is exactly what each op boundary needs (4 pieces per wave and unit, 1 per conv1 block); the barrier publishes it.
// The slots are distinct static __shared__ objects with static roles (glowk_kernels.h, rule 1): M0 always holds the first halves.
//
// Directions (net_dir<MODE>): the plain forward network (NET_FWD, NET_FWD2), the forward network of the gradient path (NET_FWD_SAVE: ReLU masks
// stored from X and Z) and the backward network (NET_BWD, 4-channel level: 18 output rows = two conv3 units; the forward pass's masks
// of the workgroup's four 32-pixel blocks in LDS; every pixel's gradient normalised by a power of two) -- the mask layout is that of the
// eight-wave 16x16x32 kernels (one entry per 32-pixel block of a wave), so either form can follow the other.  MODE | NET_FUSE: the coupling
// fused in (forward modes).  SPLIT: grid.y = 2 and every workgroup runs ONE pass (small grids: 2 x Q/128 workgroups of four waves,
// two to a CU; each pass leaves its own partial P).  MODE | NET_STORE (NET_FWD_SAVE, NET_BWD): the training sweep's launches, which also store
// their hidden tensors planar (NetArgs::st1 / st2) -- lane n of a wave then holds the ADJACENT pixels 2 n, 2 n + 1 (not n, 16 + n), so
// that the values leave as 8-byte pairs, one full 128-byte line per hidden row and instruction; the stores are counted into the op-end
// waits (they stay in flight across a barrier), which is why the host takes the form only where every wave is full (Q % 128 == 0).
//
// DOUBLE-BUFFERED ring (RingC::DB: the fused plain forward launches, MODE | NET_FUSE with NET_FWD / NET_FWD2 and 36 output rows, both
// passes in one workgroup; every NF).  The three-slot ring above is that shallow, with three barriers per hidden block, only because
// the fused form also held an LDS copy of P (36 x CO_PSTR floats), which is written in the very last ops alone.  Here P goes into unit
// slots that are dead by then, a fourth slot fits beside two workgroups per CU, and the ring is a plain double buffer of PAIRS:
// block i reads (S0, S1) when i is even and (S2, S3) when i is odd; S0 / S2 hold first halves.  Per pass
//     X_i         conv1 MFMAs on operands that are already in registers (kf), then vmcnt(0) lgkmcnt(0) + the block's barrier, then the reads
//                 of Y_i's first A group from the block's pair, then ReLU + split -- the block's VALU work -- while those reads return;
//                 issues nothing.  kf of block 0 is read in front of the pass (K0 was published long before)
//     Y_i         reads its pair (Ya_i then Yb_i, no barrier between; the A-fragment prefetch runs across).  Each group of 12 MFMAs issues the
//                 next group's reads BEHIND its first four MFMAs -- the last group reads kf of block i + 1 from K[(i + 1) & 1] instead.
//                 Issues, in the groups of its FIRST half, one piece of each of the two units of block i + 1 -> the other pair, and in
//                 group 0 the conv1 operands of block i + 2 -> K[i & 1]; Y_{NF-1}: conv3 units 0, 1 -> S0, S1.      ends: nothing
//                                                                                    (Y_{NF-1}: vmcnt(0) lgkmcnt(0), barrier)
//     Z_0         reads S0          conv3 unit 2 -> S2                                          ends: lgkmcnt(0), barrier
//     Z_1         reads S1          pass 0: the next pass's unit 0 -> S0                        ends: vmcnt(PPW or 0) lgkmcnt(0), barrier
//     Z_2         reads S2          pass 0: the next pass's unit 1 -> S1                        ends: lgkmcnt(0), barrier (last pass: the
//                                                                                                     barrier in front of fused_couple)
// One barrier per hidden block, no counted wait in the loop.  No LDS read is waited for right after it is issued: while a DMA is in
// flight the compiler's wait in front of an MFMA that needs LDS data is always lgkmcnt(0), so every read is issued eight MFMAs (two-term
// mode: four), or the activation (group 0), in front of the MFMA that needs it, and nothing younger is outstanding at that wait.  A unit's last
// piece leaves in the middle of Y_{i-1} and has its second half and X_i's MFMAs to land.  The per-wave MFMA order is that of the
// three-slot ring: results are bit for bit the same (GLOWK_CO_RING3=1 launches the three-slot instance, which stays compiled as
// k_net_h3c<..., RING3 = true>).
// The block's barrier, checked against the invariants below:
//   - it follows every wave's last read of the other pair (Y_{i-1}: consumed by that Y's MFMAs) and of K[i & 1] (kf: consumed by X_i's
//     MFMAs); lgkmcnt(0) retires them;
//   - Y_i's DMAs into the other pair and into K[i & 1] come behind it (behind group 0's first four MFMAs);
//   - the reads of pair i (X_i's A group, Y_i) come behind it, and it follows each wave's own vmcnt(0) for the pieces of pair i and of
//     K[(i + 1) & 1] (issued in Y_{i-1}); K[(i + 1) & 1] is read at the end of Y_i and not written again before Y_{i+1}, behind the
//     next barrier.  Block 0: the prologue's (pass 1: Z_1 / Z_2's and Y_{NF-1}'s) pieces, waited for at the same place;
//   - the last Y of a pass reads K0 (block 0's operands, valid) into kf and drops them.
// P: the last pass's closing tiles write row tile 0 (rows 0-15) to S0, tile 1 to S1, tile 2 (rows 32-35) to S3, [16][CO_PSTR] floats
// each.  By then S0 was last read in Z_0, S1 in Z_1, S3 in Y_{NF-1}, each behind a barrier, and a last pass issues no DMA into them
// (its Z_1 ends with vmcnt(0)).  A slot is therefore max(unit, P tile) bytes: 16 KiB at F = 512, 9 KiB at F <= 256.
// Invariants:
//   - a DMA into a slot is issued only after a barrier that every wave passes after its last read of that slot;
//   - a slot is read only after a barrier that every wave passes after its own wait for that slot's pieces;
//   - every op end that precedes a refill is s_waitcnt ... lgkmcnt(0) + the raw s_barrier (an LDS read still in
//     flight when the wave passes the barrier would race the refill);
//   - no memory operation with a VGPR destination while a DMA is in flight (glowk_kernels.h, rule 2): the im2col gather and the
//     vstash / epl loads stay in the prologue.
#pragma once
#include "glowk_kernels.h"

constexpr int CO_PX = 128;          // pixels per workgroup
constexpr int CO_PSTR = 132;        // fused coupling: floats per LDS row of P (4 * 132 = 16 mod 64 banks: the four row quarters of a tile apart)

template <int KIN, int MOUT, int NF, int MODE>
struct RingC {
  static constexpr int MODE7 = net_dir<MODE>;
  using S = RingS<KIN, MOUT, NF, MODE7, 2>;            // per-wave tiling, weight image, epilogue constants: those of the two-pass form
  static constexpr bool FUSE = (MODE & NET_FUSE) != 0;
  static constexpr bool SAVE = MODE7 == NET_FWD_SAVE, BWD = MODE7 == NET_BWD;
  static constexpr bool MERGE = S::NMT <= 3;           // two passes in one workgroup: pass 0's sums of P stay in registers, P is written once
                                                       // (five row blocks, the 8-channel level: 40 registers the kernel does not have -- two partial buffers)
  static constexpr bool M0LAST = S::NMT % 3 == 2;      // the pass's last conv3 unit sits in M0 (units cycle D, M0, M1): the next pass asks for its unit 0 itself
  static constexpr bool STORE = (MODE & NET_STORE) != 0;   // training: the launch also leaves its hidden tensors planar (NetArgs::st1 / st2)
  static constexpr int MODEX = net_dir<MODE> | (MODE & NET_STORE);   // what h3s_X sees: the mode and the store bit
  static constexpr int NFH = S::NFH, NRB = S::NRB, NMT = S::NMT, KS = S::KS;
  static constexpr int UNITP = S::MAINP / 2;            // 1-KiB pieces per unit
  static constexpr int UNIT4 = S::MAIN4 / 2;            // float4 per unit
  static constexpr int PPW = UNITP / 4;                 // DMA instructions per wave and unit
  static constexpr int NG = NFH / 2;                    // groups of 12 MFMAs (two row blocks x two pixel halves x three terms) per Y half
  static constexpr int K1PW = (S::K1P + 3) / 4;         // DMA instructions per wave and conv1 block
  static constexpr int EPN = BWD ? 0 : S::EPN;          // (the backward network has no epilogue constants)
  static constexpr int MASKN = BWD ? 2 * 4 * NF * 64 : 0;   // backward: LDS copy of the masks [mask1 | mask2][wave][hidden block][lane], entries
  static constexpr size_t LDS_BYTES = (size_t)3 * UNIT4 * 16 + (size_t)2 * S::K14 * 16 + (size_t)EPN * 4 + (size_t)MASKN * 2 +
                                      (FUSE ? (size_t)36 * CO_PSTR * 4 + CO_PX * 16 : 0);
  // the double-buffered ring (header): four slots, each a unit or a 16-row tile of P, whichever is larger (whole 1-KiB pieces)
  static constexpr bool DB = FUSE && (MODE7 == NET_FWD || MODE7 == NET_FWD2) && MOUT == 36;
  static constexpr int PTILE4 = (16 * CO_PSTR * 4 + 1023) / 1024 * 64;
  static constexpr int DBSLOT4 = UNIT4 > PTILE4 ? UNIT4 : PTILE4;
  static constexpr size_t LDS_BYTES_DB = (size_t)4 * DBSLOT4 * 16 + (size_t)2 * S::K14 * 16 + (size_t)EPN * 4 + CO_PX * 16;
  static constexpr bool FITS = (MODE7 == NET_FWD || MODE7 == NET_FWD2 || SAVE || BWD) && !(MODE & NET_HALF) && (!STORE || ((SAVE || BWD) && !FUSE)) && S::NGRP == 1 && (NMT == 2 || NMT == 3 || (NMT == 5 && !STORE && !BWD)) &&
                               (!FUSE || (MOUT == 36 && !BWD)) && KS <= 3 && NF % 4 == 0 && NFH >= 2 && NFH % 2 == 0 && UNITP % 4 == 0 && PPW == NG &&
                               2 * LDS_BYTES <= 160 * 1024 + 1;   // (diagnostic paddings aside)
  // training: vector-memory stores an op issues per wave (8 pairs of values per activated hidden block from X and from Z; a saving launch adds
  // the block's ReLU mask).  The host only takes the form where every wave is full (Q % CO_PX == 0), so the counts are static.
  // (lane n of a wave holds the adjacent pixels 2 n, 2 n + 1 there, and the values leave as 8-byte pairs: full 128-byte lines)
  static constexpr int XST = STORE ? 8 : 0;
  static constexpr int z_acts(int z) { int n = 0; for (int t = z * NFH; t < (z + 1) * NFH; ++t) n += (t % NMT == 0) ? 1 : 0; return n; }
  static constexpr int z_st(int z) { return STORE ? z_acts(z) * (8 + (SAVE ? 1 : 0)) : 0; }
  __device__ static const float4* main_unit(const float4* img, int pass, int i, int half) { return S::main_chunk(img, pass, i) + (size_t)half * UNIT4; }
  __device__ static const float4* out_unit(const float4* img, int pass, int z) { return S::out_chunk(img, pass, 0) + (size_t)z * UNIT4; }
};

// end of an op without a unit to wait for: this wave's LDS reads have retired (a DMA into the slot they read may follow the barrier)
__device__ __forceinline__ void co_bar() {
  __builtin_amdgcn_s_waitcnt(0xC07F);     // lgkmcnt(0) alone
  h3_barrier();
}

// end of an op: all but the n youngest vector-memory operations of this wave are done, its LDS reads have retired, then the workgroup
// barrier.  (lgkmcnt(0): the first build waited on vmcnt alone and lost ~0.2 % of the waves' results under a co-resident partner -- an
// LDS read still in flight when the wave passed the barrier after which another wave's DMA refills the slot)
template <int N>
__device__ __forceinline__ void co_end() {
  __builtin_amdgcn_s_waitcnt((N & 15) | 0x0070 | ((N >> 4) << 14));   // vmcnt(N) and lgkmcnt(0)
  h3_barrier();
}
// ... with `more` extra operations (the op's stores: a saving launch's ReLU mask) allowed to stay in flight, decided per wave at run time
template <int N>
__device__ __forceinline__ void co_end_st(bool more) {
  if (more) co_end<N + 1>();
  else co_end<N>();
}

struct CoCtx {
  float4 *m0, *m1, *d;      // unit slots (distinct static __shared__ arrays)
  const float4* img;
  int w4;
  unsigned voff;
};

// one Y half: conv2 contribution of the current hidden block to row blocks H NFH .. H NFH + NFH - 1 (unit in `slot`), the A fragments of
// the next group read while the current one computes (as h3s_Y), and this wave's share of one DMA -- a unit (one piece per group) or
// the conv1 operands of a later block (first group) -- issued between the groups
// (H = 0: the conv1 operands, src = block image, dst = its K slot; H = 1: a unit, dst = M0)
template <int NFH, int MODE7, int H, int TAG, int K1P>
__device__ __forceinline__ void co_Y(const float4* slot, const h8 (&bh)[2], const h8 (&bl)[2], f32x4 (&acc2)[2 * NFH][2], int lane,
                                     const float4* src, float4* dst, int w4, unsigned voff) {
  const h8* buf = reinterpret_cast<const h8*>(slot) + lane;
  const char* ub = uniform_ptr(src);
  constexpr int NG = NFH / 2;
  h8 A[2][4];
  auto load = [&](h8 (&d)[4], int gi) { y_group_read(buf, gi, d); };
  load(A[0], 0);
#pragma unroll
  for (int gi = 0; gi < NG; ++gi) {
    const int o0 = H * NFH + 2 * gi, o1 = o0 + 1;
    if (gi + 1 < NG) load(A[(gi + 1) & 1], gi + 1);
    if constexpr (H == 1) {
      const int piece = gi * 4 + w4;
      glds16(reinterpret_cast<const float4*>(ub + (size_t)piece * 1024 + voff), dst + piece * 64);
      asm volatile("; dma site %0" ::"n"(TAG * 16 + gi));
    } else if (gi == 0) {
      stage4<K1P, TAG * 16 + 15>(src, dst, w4, voff);
    }
    __builtin_amdgcn_sched_barrier(0);
    const h8 (&af)[4] = A[gi & 1];
    y_group_first<2>(af, bh, acc2[o0], acc2[o1]);
    y_group_rest<2, MODE7 != NET_FWD2>(af, bh, bl, acc2[o0], acc2[o1]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Z: conv3 unit z of a pass = NFH tiles (16 rows x one hidden block) in (hidden block, row block) order.  Two passes in one workgroup:
// pass 0 keeps its sums (bias included) in `keep`, the last pass adds them and writes the rows -- to HBM (P, one buffer) or, fused, to
// the workgroup's LDS copy; SOLO (one pass per workgroup): every pass writes its own partial P.
// DMA duties with a next pass in the workgroup (NEXT): three units (NMT = 3: D, M0, M1): Z_0 -> conv3 unit 2 into M1 (always), Z_1 -> the
// next pass's conv3 unit 0 into D, Z_2 -> its unit 0 into M0 (its X_0 then asks for unit 1 -> M1); two units (NMT = 2: D, M0): Z_0 -> the
// next pass's unit 1 into M1, Z_1 -> its conv3 unit 0 into D (its X_0 asks for unit 0 -> M0 and waits for it).
template <int KIN, int MOUT, int NF, int MODE, int PASS, bool SOLO, int Z>
__device__ __forceinline__ void co_Z(const NetArgs& a, const H3Ctx& hc, const CoCtx& c, const float* epl, float* pl,
                                     f32x4 (&acc2)[(RingC<KIN, MOUT, NF, MODE>::NRB)][2], f32x4 (&acc3)[(RingC<KIN, MOUT, NF, MODE>::NMT)][2], h8 (&bh)[2],
                                     h8 (&bl)[2], const int (&q)[2], const bool (&qok)[2], int lane, int kq,
                                     f32x4 (&keep)[(RingC<KIN, MOUT, NF, MODE>::NMT)][2]) {
  using G = RingC<KIN, MOUT, NF, MODE>;
  constexpr int NFH = G::NFH, NMT = G::NMT, M3 = MOUT, MODE7 = G::MODE7;
  constexpr bool NEXT = !SOLO && PASS == 0;            // another pass follows in this workgroup
  constexpr bool LAST = !SOLO && PASS == 1;            // ... this is the second: it completes pass 0's sums
  if constexpr (NMT == 3) {
    if constexpr (Z == 0) stage4<G::UNITP, 70>(G::out_unit(c.img, PASS, 2), c.m1, c.w4, c.voff);
    if constexpr (Z == 1 && NEXT) stage4<G::UNITP, 71>(G::out_unit(c.img, PASS + 1, 0), c.d, c.w4, c.voff);
    if constexpr (Z == 2 && NEXT) stage4<G::UNITP, 72>(G::main_unit(c.img, PASS + 1, 0, 0), c.m0, c.w4, c.voff);
  } else if constexpr (NMT == 2) {
    if constexpr (Z == 0 && NEXT) stage4<G::UNITP, 75>(G::main_unit(c.img, PASS + 1, 0, 1), c.m1, c.w4, c.voff);
    if constexpr (Z == 1 && NEXT) stage4<G::UNITP, 76>(G::out_unit(c.img, PASS + 1, 0), c.d, c.w4, c.voff);
  } else {      // five units (the 8-channel level): Z_z asks for conv3 unit z + 2 into the slot Z_{z-1} read; then the next pass's unit 1 -> M1, conv3 unit 0 -> D
    static_assert(NMT == 5, "conv3 units");
    if constexpr (Z == 0) stage4<G::UNITP, 80>(G::out_unit(c.img, PASS, 2), c.m1, c.w4, c.voff);
    if constexpr (Z == 1) stage4<G::UNITP, 81>(G::out_unit(c.img, PASS, 3), c.d, c.w4, c.voff);
    if constexpr (Z == 2) stage4<G::UNITP, 82>(G::out_unit(c.img, PASS, 4), c.m0, c.w4, c.voff);
    if constexpr (Z == 3 && NEXT) stage4<G::UNITP, 83>(G::main_unit(c.img, PASS + 1, 0, 1), c.m1, c.w4, c.voff);
    if constexpr (Z == 4 && NEXT) stage4<G::UNITP, 84>(G::out_unit(c.img, PASS + 1, 0), c.d, c.w4, c.voff);
  }
  const float4* slot = Z % 3 == 0 ? c.d : Z % 3 == 1 ? c.m0 : c.m1;
  const h8* buf = reinterpret_cast<const h8*>(slot) + lane;
  const float* pb = epl + NF * 32;
#pragma unroll
  for (int tp = 0; tp < NFH; ++tp) {
    const int t = Z * NFH + tp;
    const int fo = t / NMT, ml = t % NMT;
    if (ml == 0) {
      unsigned mask = 0, bits = 0;
      if (G::BWD) mask = hc.mkl[((size_t)(threadIdx.x >> 6) * NF + PASS * NFH + fo) * 64 + lane];        // mask1: the ReLU after conv1
      if constexpr (G::STORE)
        bits = h3s_act_pair<MODE7, true, split_fma<KIN>>(acc2[2 * fo][0], acc2[2 * fo + 1][0], acc2[2 * fo][1], acc2[2 * fo + 1][1], a.sc2, mask, bh, bl,
                                         uniform_fptr(a.st2 + (size_t)(PASS * NFH + fo) * 32 * a.Q), ((unsigned)(4 * kq) * (unsigned)a.Q + (unsigned)q[0]) * 4u,
                                         (unsigned)a.Q * 4u);
      else {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) bits |= h3s_act<MODE7, false, split_fma<KIN>>(acc2[2 * fo][hf], acc2[2 * fo + 1][hf], a.sc2, mask >> (8 * hf), bh[hf], bl[hf]) << (8 * hf);
      }
      if (G::SAVE && hc.wok) a.mask2[(hc.wblk * NF + PASS * NFH + fo) * 64 + lane] = (unsigned short)bits;
    }
    if (fo == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) { acc3[ml][0][r] = 0.0f; acc3[ml][1][r] = 0.0f; }
    }
    const h8 ah = buf[(tp * 2 + 0) * 64], al = buf[(tp * 2 + 1) * 64];
    acc3[ml][0] = mfma3s<MODE7 == NET_FWD2>(ah, al, bh[0], bl[0], acc3[ml][0]);
    acc3[ml][1] = mfma3s<MODE7 == NET_FWD2>(ah, al, bh[1], bl[1], acc3[ml][1]);
    if (fo == NFH - 1) {
      if constexpr (G::S::C3P) {     // (the 8-channel level: one accumulator group of five tiles, two partial buffers)
        static_assert(!G::MERGE && !G::FUSE && NMT == 5, "the pre-sum writes per-pass partials");
        if (a.pw) {     // as h3s_Z: the sums stay in acc3, scaled; the last tile adds the horizontal taps and stores
#pragma unroll
          for (int hf = 0; hf < 2; ++hf)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              acc3[ml][hf][r] = PASS == 0 ? fmaf(acc3[ml][hf][r], a.sc3, pb[c3_row<typename G::S>(ml, r, kq)]) : acc3[ml][hf][r] * a.sc3;
          if (ml == NMT - 1) c3_presum_store<NMT, 2>(acc3, a.P + (size_t)PASS * a.pstride, a.Q, a.pw, 0, q, qok, lane, kq);
          continue;
        }
      }
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = c3_row<typename G::S>(ml, r, kq);
          const float part = G::BWD ? acc3[ml][hf][r] * (a.sc3 * hc.ub[hf]) : PASS == 0 ? fmaf(acc3[ml][hf][r], a.sc3, pb[m]) : acc3[ml][hf][r] * a.sc3;
          if constexpr (NEXT && G::MERGE) { keep[ml][hf][r] = part; continue; }
          const float val = (LAST && G::MERGE) ? part + keep[ml][hf][r] : part;
          if constexpr (G::FUSE) {
            if (m < M3) pl[m * CO_PSTR + (int)(threadIdx.x >> 6) * 32 + 16 * hf + (lane & 15)] = val;
          } else {
            float* Pp = a.P + ((SOLO || !G::MERGE) ? (size_t)PASS * a.pstride : (size_t)0);
            if (m < M3 && qok[hf]) Pp[(size_t)m * a.Q + q[hf]] = val;
          }
        }
    }
  }
  // next op and what it reads: Z_1 <- conv3 unit 1 (issued by Yb_{NF-1}); Z_2 <- conv3 unit 2 (issued by Z_0); X_0 of the next pass <- conv1
  // operands that landed long ago.  A saving launch's mask stores ride in between: it waits for everything (three short ops per pass).
  // A training launch's hidden stores stay in flight (vmcnt counts in issue order: what the next op reads is older than the count allowed
  // to remain -- Z_2's unit was asked for by Z_0, BEFORE Z_0's stores; the counter holds 63).
  constexpr bool ISSUED = NMT == 3 ? (Z == 0 || NEXT) : NMT == 2 ? (Z <= 1 && NEXT) : (Z <= 2 || NEXT);     // this op issued a unit
  if constexpr (Z + 1 < NMT) {
    if constexpr (G::STORE) {
      constexpr int after = (ISSUED ? G::PPW : 0) + G::z_st(Z) + ((NMT == 3 && Z == 1) ? G::z_st(0) : 0);
      co_end<(after < 63 ? after : 63)>();
    } else if constexpr (G::SAVE) co_end<0>();
    else co_end<(ISSUED ? G::PPW : 0)>();
  } else co_bar();
}

template <int KIN, int MOUT, int NF, int MODE, int PASS, bool SOLO>
__device__ __forceinline__ void co_pass(const NetArgs& a, const H3Ctx& hc, const CoCtx& c, const float* epl, float* pl,
                                        const h8 (&xh)[(RingC<KIN, MOUT, NF, MODE>::KS)][2], const h8 (&xl)[(RingC<KIN, MOUT, NF, MODE>::KS)][2],
                                        const int (&q)[2], const bool (&qok)[2], int lane, int kq, f32x4 (&keep)[(RingC<KIN, MOUT, NF, MODE>::NMT)][2]) {
  using G = RingC<KIN, MOUT, NF, MODE>;
  using S = typename G::S;
  constexpr int NRB = G::NRB, NFH = G::NFH, MODE7 = G::MODE7;
  constexpr int f2base = PASS * NFH * 32;
  constexpr bool SECOND = !SOLO && PASS == 1;          // units 0 / 1 were not loaded by the prologue
  f32x4 acc2[NRB][2];
#pragma unroll
  for (int ob = 0; ob < NRB; ++ob)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float b = G::BWD ? 0.0f : epl[f2base + ob * 16 + 4 * kq + r];   // conv2 bias (scaled)
      acc2[ob][0][r] = b;
      acc2[ob][1][r] = b;
    }
  const bool st = G::SAVE && PASS == 0 && hc.wok;      // this wave stores a ReLU mask from every X of this pass (h3s_X)
  constexpr int XST = PASS == 0 ? G::XST : 0;          // ... and a training launch the block's 16 values per lane
  h8 bh[2], bl[2];
#pragma nounroll
  for (int i0 = 0; i0 < NF; i0 += 2) {
    // ---- hidden block i0 (conv1 operands in K0).  Its second unit (-> M1): the prologue's in a first pass' block 0; with two conv3 units
    //      a second pass' block 0 finds unit 1 requested by Z_0 and asks for unit 0 (-> M0) itself
    if (i0 > 0 || (SECOND && !G::M0LAST)) stage4<G::UNITP, 73>(G::main_unit(c.img, PASS, i0, 1), c.m1, c.w4, c.voff);
    if constexpr (SECOND && G::M0LAST) {
      if (i0 == 0) stage4<G::UNITP, 77>(G::main_unit(c.img, PASS, 0, 0), c.m0, c.w4, c.voff);
    }
    h3s_X<KIN, MOUT, NF, G::MODEX, 2, 0, PASS, G::STORE>(a, hc, i0, xh, xl, lane, bh, bl);
    if (SECOND && G::M0LAST && i0 == 0) co_end<0>();            // (the unit this very op asked for)
    else co_end_st<G::PPW + XST>(st);                   // unit 2 i0 (M0) landed; this op's unit (and its stores) may still be in flight
    co_Y<NFH, MODE7, 0, 1, S::K1P>(c.m0, bh, bl, acc2, lane, hc.k1img + (size_t)((i0 + 2) % NF) * S::K14, hc.k1s0, c.w4, c.voff);
    co_end_st<G::K1PW + XST>(st);                       // unit 2 i0 + 1 (M1) landed (asked for before X's stores: they may stay in flight)
    co_Y<NFH, MODE7, 1, 2, S::K1P>(c.m1, bh, bl, acc2, lane, G::main_unit(c.img, PASS, i0 + 1, 0), c.m0, c.w4, c.voff);
    co_bar();                                           // (M1 free for the next X's unit)
    // ---- hidden block i0 + 1 (conv1 operands in K1)
    stage4<G::UNITP, 74>(G::main_unit(c.img, PASS, i0 + 1, 1), c.m1, c.w4, c.voff);
    h3s_X<KIN, MOUT, NF, G::MODEX, 2, 1, PASS, G::STORE>(a, hc, i0 + 1, xh, xl, lane, bh, bl);
    co_end_st<G::PPW + XST>(st);
    co_Y<NFH, MODE7, 0, 3, S::K1P>(c.m0, bh, bl, acc2, lane, hc.k1img + (size_t)((i0 + 3) % NF) * S::K14, hc.k1s1, c.w4, c.voff);
    co_end_st<G::K1PW + XST>(st);
    // (after the last block: conv3 unit 1 takes the place of "unit 2 NF")
    co_Y<NFH, MODE7, 1, 4, S::K1P>(c.m1, bh, bl, acc2, lane, i0 + 2 < NF ? G::main_unit(c.img, PASS, i0 + 2, 0) : G::out_unit(c.img, PASS, 1), c.m0,
                                   c.w4, c.voff);
    co_bar();
  }
  f32x4 acc3[G::NMT][2];
  co_Z<KIN, MOUT, NF, MODE, PASS, SOLO, 0>(a, hc, c, epl, pl, acc2, acc3, bh, bl, q, qok, lane, kq, keep);
  co_Z<KIN, MOUT, NF, MODE, PASS, SOLO, 1>(a, hc, c, epl, pl, acc2, acc3, bh, bl, q, qok, lane, kq, keep);
  if constexpr (G::NMT >= 3) co_Z<KIN, MOUT, NF, MODE, PASS, SOLO, 2>(a, hc, c, epl, pl, acc2, acc3, bh, bl, q, qok, lane, kq, keep);
  if constexpr (G::NMT >= 4) co_Z<KIN, MOUT, NF, MODE, PASS, SOLO, 3>(a, hc, c, epl, pl, acc2, acc3, bh, bl, q, qok, lane, kq, keep);
  if constexpr (G::NMT >= 5) co_Z<KIN, MOUT, NF, MODE, PASS, SOLO, 4>(a, hc, c, epl, pl, acc2, acc3, bh, bl, q, qok, lane, kq, keep);
}

// ---- the double-buffered ring (RingC::DB; header comment) ----------------------------------------------------------------------
struct CoCtxDB {
  float4 *s0, *s1, *s2, *s3;   // unit slots (distinct static __shared__ arrays): block i reads (s0, s1) when i is even, (s2, s3) when odd
  const float4* img;
  int w4;
  unsigned voff;
};

// Y of one hidden block: co_Y's two halves back to back (row blocks 0 .. NFH-1 from `sa`, NFH .. 2 NFH - 1 from `sb`), the A-fragment
// prefetch running across the boundary.  Group 0's fragments arrive in A[0] (read by the X in front, behind its barrier); the last group,
// which has no next group to read, reads the NEXT block's conv1 operands from `kslot` into kf instead.  This wave's share of the next
// block's units goes out in the first half, one piece of each unit per group (srca -> dsta, srcb -> dstb), so that the last piece has
// the second half of Y and the next X's MFMAs to land; the conv1 operands of a later block in the first group
template <int NFH, int MODE7, int TAG, int K1P, int NKF>
__device__ __forceinline__ void co_Ydb(const float4* sa, const float4* sb, const h8 (&bh)[2], const h8 (&bl)[2], f32x4 (&acc2)[2 * NFH][2], int lane,
                                       h8 (&A)[2][4], h8 (&kf)[NKF], const float4* kslot, const float4* srca, float4* dsta, const float4* srcb,
                                       float4* dstb, const float4* k1src, float4* k1dst, int w4, unsigned voff) {
  const h8* bufa = reinterpret_cast<const h8*>(sa) + lane;
  const h8* bufb = reinterpret_cast<const h8*>(sb) + lane;
  const h8* kbuf = reinterpret_cast<const h8*>(kslot) + lane;
  const char* uba = uniform_ptr(srca);
  const char* ubb = uniform_ptr(srcb);
  constexpr int NG = NFH / 2;
  auto load = [&](h8 (&d)[4], int g) { y_group_read(g < NG ? bufa : bufb, g % NG, d); };
#pragma unroll
  for (int g = 0; g < 2 * NG; ++g) {
    const int gi = g % NG;
    const int o0 = (g / NG) * NFH + 2 * gi, o1 = o0 + 1;
    const h8 (&af)[4] = A[g & 1];
    y_group_first<2>(af, bh, acc2[o0], acc2[o1]);
    // the reads and DMA of this group go out BEHIND its first four MFMAs: the wait the compiler puts in front of a group's first MFMA is
    // always lgkmcnt(0) while a DMA is in flight, so reads issued in front of it would be waited for at once -- now it only finds reads
    // that have had the rest of the previous group to return
    __builtin_amdgcn_sched_barrier(0);
    if (g + 1 < 2 * NG) load(A[(g + 1) & 1], g + 1);
    else {
#pragma unroll
      for (int i = 0; i < NKF; ++i) kf[i] = kbuf[i * 64];
    }
    if (g < NG) {                                   // (PPW = NG pieces per wave and unit)
      const int piece = g * 4 + w4;
      glds16(reinterpret_cast<const float4*>(uba + (size_t)piece * 1024 + voff), dsta + piece * 64);
      asm volatile("; dma site %0" ::"n"(TAG * 16 + g));
      glds16(reinterpret_cast<const float4*>(ubb + (size_t)piece * 1024 + voff), dstb + piece * 64);
      asm volatile("; dma site %0" ::"n"(TAG * 16 + NG + g));
    }
    if (g == 0) stage4<K1P, TAG * 16 + 15>(k1src, k1dst, w4, voff);
    __builtin_amdgcn_sched_barrier(0);
    y_group_rest<2, MODE7 != NET_FWD2>(af, bh, bl, acc2[o0], acc2[o1]);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// X of one hidden block in the double-buffered ring: the conv1 MFMAs on operands that are already in registers (kf: read under the end of
// the previous Y, or in front of the pass), the block's wait and barrier, the reads of Y's first A group from the block's pair (`sa`),
// and the activation -- the block's VALU work -- while those reads are in flight
template <int KIN, int MOUT, int NF, int MODE>
__device__ __forceinline__ void co_Xdb(const NetArgs& a, const h8 (&xh)[(RingC<KIN, MOUT, NF, MODE>::KS)][2], const h8 (&xl)[(RingC<KIN, MOUT, NF, MODE>::KS)][2],
                                       int lane, const h8 (&kf)[(RingC<KIN, MOUT, NF, MODE>::S::KSX * 2)], const float4* sa, h8 (&A0)[4], h8 (&bh)[2],
                                       h8 (&bl)[2]) {
  using G = RingC<KIN, MOUT, NF, MODE>;
  f32x4 h1[2][2];
  h3s_X_mma<typename G::S>(kf, xh, xl, h1);
#pragma unroll
  for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(h1[i >> 1][i & 1]));      // (the MFMAs stay in front of the barrier: their results are only used behind it)
  __builtin_amdgcn_sched_barrier(0);
  co_end<0>();      // this wave's pieces of this block's units and of the other K slot have landed; its reads of the other pair and of kf retired
  const h8* buf = reinterpret_cast<const h8*>(sa) + lane;
#pragma unroll
  for (int j = 0; j < 4; ++j) A0[j] = buf[j * 64];      // row blocks 0, 1 (hi, lo): co_Ydb's group 0
  __builtin_amdgcn_sched_barrier(0);
  h3s_X_act<G::MODE7, split_fma<KIN>>(h1, a.sc1, bh, bl);
  __builtin_amdgcn_sched_barrier(0);
}

// Z: conv3 unit Z of a pass (co_Z's tiles and arithmetic; three units, merged passes, fused).  Pass 0 keeps its sums in `keep`; the
// last pass writes P's row tile ml into the dead slot S0 / S1 / S3.
template <int KIN, int MOUT, int NF, int MODE, int PASS, int Z>
__device__ __forceinline__ void co_Zdb(const NetArgs& a, const CoCtxDB& c, const float* epl, f32x4 (&acc2)[(RingC<KIN, MOUT, NF, MODE>::NRB)][2],
                                       f32x4 (&acc3)[3][2], h8 (&bh)[2], h8 (&bl)[2], int lane, int kq, f32x4 (&keep)[3][2]) {
  using G = RingC<KIN, MOUT, NF, MODE>;
  constexpr int NFH = G::NFH, NMT = G::NMT, M3 = MOUT, MODE7 = G::MODE7;
  static_assert(NMT == 3 && G::MERGE && G::FUSE, "the double-buffered ring: three conv3 units, merged passes, fused coupling");
  constexpr bool NEXT = PASS == 0;                     // another pass follows in this workgroup
  if constexpr (Z == 0) stage4<G::UNITP, 90>(G::out_unit(c.img, PASS, 2), c.s2, c.w4, c.voff);
  if constexpr (Z == 1 && NEXT) stage4<G::UNITP, 91>(G::main_unit(c.img, PASS + 1, 0, 0), c.s0, c.w4, c.voff);
  if constexpr (Z == 2 && NEXT) stage4<G::UNITP, 92>(G::main_unit(c.img, PASS + 1, 0, 1), c.s1, c.w4, c.voff);
  const float4* slot = Z == 0 ? c.s0 : Z == 1 ? c.s1 : c.s2;
  const h8* buf = reinterpret_cast<const h8*>(slot) + lane;
  const float* pb = epl + NF * 32;
#pragma unroll
  for (int tp = 0; tp < NFH; ++tp) {
    const int t = Z * NFH + tp;
    const int fo = t / NMT, ml = t % NMT;
    if (ml == 0) {
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) h3s_act<MODE7, false, split_fma<KIN>>(acc2[2 * fo][hf], acc2[2 * fo + 1][hf], a.sc2, 0u, bh[hf], bl[hf]);
    }
    if (fo == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) { acc3[ml][0][r] = 0.0f; acc3[ml][1][r] = 0.0f; }
    }
    const h8 ah = buf[(tp * 2 + 0) * 64], al = buf[(tp * 2 + 1) * 64];
    acc3[ml][0] = mfma3s<MODE7 == NET_FWD2>(ah, al, bh[0], bl[0], acc3[ml][0]);
    acc3[ml][1] = mfma3s<MODE7 == NET_FWD2>(ah, al, bh[1], bl[1], acc3[ml][1]);
    if (fo == NFH - 1) {
      float* pt = reinterpret_cast<float*>(ml == 0 ? c.s0 : ml == 1 ? c.s1 : c.s3);      // (NFH = 2: tile 0 closes in Z_1, behind Z_0's barrier)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = ml * 16 + 4 * kq + r;
          const float part = PASS == 0 ? fmaf(acc3[ml][hf][r], a.sc3, pb[m]) : acc3[ml][hf][r] * a.sc3;
          if constexpr (NEXT) { keep[ml][hf][r] = part; continue; }
          const float val = part + keep[ml][hf][r];
          if (m < M3) pt[(4 * kq + r) * CO_PSTR + (int)(threadIdx.x >> 6) * 32 + 16 * hf + (lane & 15)] = val;
        }
    }
  }
  if constexpr (Z == 0) co_bar();                      // (conv3 unit 2 is Z_2's: it has Z_1 to land)
  if constexpr (Z == 1) co_end<(NEXT ? G::PPW : 0)>();  // conv3 unit 2 landed; the next pass's unit 0 may still be in flight
  if constexpr (Z == 2 && NEXT) co_bar();              // (last pass: the barrier in front of fused_couple)
}

template <int KIN, int MOUT, int NF, int MODE, int PASS>
__device__ __forceinline__ void co_pass_db(const NetArgs& a, const H3Ctx& hc, const CoCtxDB& c, const float* epl,
                                           const h8 (&xh)[(RingC<KIN, MOUT, NF, MODE>::KS)][2], const h8 (&xl)[(RingC<KIN, MOUT, NF, MODE>::KS)][2],
                                           int lane, int kq, f32x4 (&keep)[3][2]) {
  using G = RingC<KIN, MOUT, NF, MODE>;
  using S = typename G::S;
  constexpr int NRB = G::NRB, NFH = G::NFH, MODE7 = G::MODE7;
  constexpr int f2base = PASS * NFH * 32;
  f32x4 acc2[NRB][2];
#pragma unroll
  for (int ob = 0; ob < NRB; ++ob)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float b = epl[f2base + ob * 16 + 4 * kq + r];   // conv2 bias (scaled)
      acc2[ob][0][r] = b;
      acc2[ob][1][r] = b;
    }
  h8 bh[2], bl[2];
  constexpr int NKF = S::KSX * 2;      // conv1 operands: one register fragment per stacked k-step and row block
  h8 A[2][4];        // co_Ydb's A fragments; [0] is filled by the X in front
  h8 kf[NKF];        // conv1 operands of the next X: block 0's are read here (K0 was published long before), the others under the end of Y
  h3s_X_load<S, 0>(hc, lane, kf);
  __builtin_amdgcn_sched_barrier(0);
#pragma nounroll
  for (int i0 = 0; i0 < NF; i0 += 2) {
    // ---- hidden block i0: conv1 operands from K0, units in (S0, S1) -- the prologue's, or the previous pass's Z_1 / Z_2's
    co_Xdb<KIN, MOUT, NF, MODE>(a, xh, xl, lane, kf, c.s0, A[0], bh, bl);
    co_Ydb<NFH, MODE7, 1, S::K1P, NKF>(c.s0, c.s1, bh, bl, acc2, lane, A, kf, hc.k1s1, G::main_unit(c.img, PASS, i0 + 1, 0), c.s2,
                                       G::main_unit(c.img, PASS, i0 + 1, 1), c.s3, hc.k1img + (size_t)((i0 + 2) % NF) * S::K14, hc.k1s0, c.w4, c.voff);
    // ---- hidden block i0 + 1: conv1 operands from K1, units in (S2, S3)
    co_Xdb<KIN, MOUT, NF, MODE>(a, xh, xl, lane, kf, c.s2, A[0], bh, bl);
    // (after the last block: conv3 units 0, 1 take the place of "block NF"; the operands read from K0 are those of block 0 and go unused)
    const bool more = i0 + 2 < NF;
    co_Ydb<NFH, MODE7, 2, S::K1P, NKF>(c.s2, c.s3, bh, bl, acc2, lane, A, kf, hc.k1s0, more ? G::main_unit(c.img, PASS, i0 + 2, 0) : G::out_unit(c.img, PASS, 0),
                                       c.s0, more ? G::main_unit(c.img, PASS, i0 + 2, 1) : G::out_unit(c.img, PASS, 1), c.s1,
                                       hc.k1img + (size_t)((i0 + 3) % NF) * S::K14, hc.k1s1, c.w4, c.voff);
  }
  co_end<0>();                                          // Y_{NF-1}: conv3 units 0, 1 landed
  f32x4 acc3[3][2];
  co_Zdb<KIN, MOUT, NF, MODE, PASS, 0>(a, c, epl, acc2, acc3, bh, bl, lane, kq, keep);
  co_Zdb<KIN, MOUT, NF, MODE, PASS, 1>(a, c, epl, acc2, acc3, bh, bl, lane, kq, keep);
  co_Zdb<KIN, MOUT, NF, MODE, PASS, 2>(a, c, epl, acc2, acc3, bh, bl, lane, kq, keep);
}

// RING3: the three-slot ring where the instance also has the double-buffered one (GLOWK_CO_RING3: parity tests, in-process A/B)
template <int KIN, int MOUT, int NF, int MODE, bool SPLIT, bool RING3 = false>
__global__ __launch_bounds__(256, 2) void k_net_h3c(NetArgs a) {
  using G = RingC<KIN, MOUT, NF, MODE>;
  using S = typename G::S;
  constexpr int KS = G::KS;
  constexpr int SGN = G::BWD ? -1 : 1;                 // backward gathers at q - d(tap)
  static_assert(G::FITS, "shape");
  static_assert(!(G::FUSE && SPLIT), "the fused coupling needs both passes in one workgroup");
  constexpr bool DB = G::DB && !SPLIT && !RING3;       // the double-buffered ring
  static_assert(!RING3 || G::DB, "RING3 names the three-slot form of an instance that has both");
  static_assert(!DB || 2 * G::LDS_BYTES_DB <= 160 * 1024, "two workgroups per CU");

  const int tid = threadIdx.x;
  // (aligned 1024: the LDS layout is sorted by alignment first, so the DMA targets take the lowest addresses and the fused form's
  //  copy of P the highest)
  CoCtx c;
  CoCtxDB cd;
  if constexpr (DB) {
    __shared__ __attribute__((aligned(1024))) float4 slotS0[G::DBSLOT4];
    __shared__ __attribute__((aligned(1024))) float4 slotS1[G::DBSLOT4];
    __shared__ __attribute__((aligned(1024))) float4 slotS2[G::DBSLOT4];
    __shared__ __attribute__((aligned(1024))) float4 slotS3[G::DBSLOT4];
    cd.s0 = slotS0; cd.s1 = slotS1; cd.s2 = slotS2; cd.s3 = slotS3;
  } else {
    __shared__ __attribute__((aligned(1024))) float4 slotM0[G::UNIT4];
    __shared__ __attribute__((aligned(1024))) float4 slotM1[G::UNIT4];
    __shared__ __attribute__((aligned(1024))) float4 slotD[G::UNIT4];
    c.m0 = slotM0; c.m1 = slotM1; c.d = slotD;
  }
  __shared__ __attribute__((aligned(1024))) float4 k1slot0[S::K14];
  __shared__ __attribute__((aligned(1024))) float4 k1slot1[S::K14];
  float* epl = nullptr;                                 // conv2 accumulator init | per-row constants of P (forward modes)
  if constexpr (!G::BWD) { __shared__ float epl_arr[S::EPN]; epl = epl_arr; }
  unsigned short* mkl = nullptr;                        // backward: the forward pass's ReLU decisions of the workgroup's four 32-pixel blocks
  if constexpr (G::BWD) { __shared__ __attribute__((aligned(1024))) unsigned short mkl_arr[G::MASKN]; mkl = mkl_arr; }
  float* plds = nullptr;                                // fused coupling: the workgroup's per-tap outputs (double-buffered ring: in dead slots) ...
  float4* vstash = nullptr;                             // ... and its pixels' four input channels
  if constexpr (G::FUSE && !DB) { __shared__ float plds_arr[36 * CO_PSTR]; plds = plds_arr; }
  if constexpr (G::FUSE) { __shared__ float4 vstash_arr[CO_PX]; vstash = vstash_arr; }
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n16 = lane & 15;
  const int kq = lane >> 4;
  const int qbase = ((int)blockIdx.x * 4 + wave) * 32;
  // (training form: adjacent pixels per lane -- its hidden stores are 8-byte pairs; masks and P follow q, so the pair of launches agrees)
  const int q[2] = {G::STORE ? qbase + 2 * n16 : qbase + n16, G::STORE ? qbase + 2 * n16 + 1 : qbase + 16 + n16};
  const bool qok[2] = {q[0] < a.Q, q[1] < a.Q};
  const int pass0 = SPLIT ? (int)blockIdx.y : 0;       // the (first) pass this workgroup runs

  H3Ctx hc;                    // what h3s_X reads: conv1 operand slots and image, masks
  hc.sA = hc.sB = hc.sD = nullptr; hc.k1s0 = k1slot0; hc.k1s1 = k1slot1;
  hc.k1img = a.RSp; hc.img = a.RSp; hc.mkl = mkl; hc.mk2off = 4 * NF * 64; hc.pl = plds;
  hc.wblk = (size_t)blockIdx.x * 4 + wave;             // this wave's 32-pixel block: the unit of the ReLU-mask arrays
  hc.wok = (long)hc.wblk * 32 < a.Q;
  hc.w4 = wave; hc.voff = (unsigned)lane * 16u; hc.ub[0] = hc.ub[1] = 1.0f;
  c.img = a.RSp; c.w4 = wave; c.voff = (unsigned)lane * 16u;
  cd.img = a.RSp; cd.w4 = wave; cd.voff = (unsigned)lane * 16u;

  if constexpr (DB) {          // block 0's pair
    stage4<G::UNITP, 58>(G::main_unit(cd.img, 0, 0, 0), cd.s0, c.w4, c.voff);
    stage4<G::UNITP, 59>(G::main_unit(cd.img, 0, 0, 1), cd.s1, c.w4, c.voff);
  } else {
    stage4<G::UNITP, 60>(G::main_unit(c.img, pass0, 0, 0), c.m0, c.w4, c.voff);
    stage4<G::UNITP, 61>(G::main_unit(c.img, pass0, 0, 1), c.m1, c.w4, c.voff);
    stage4<G::UNITP, 62>(G::out_unit(c.img, pass0, 0), c.d, c.w4, c.voff);
  }
  stage4<S::K1P, 63>(hc.k1img, k1slot0, c.w4, c.voff);
  stage4<S::K1P, 64>(hc.k1img + S::K14, k1slot1, c.w4, c.voff);
  if constexpr (G::BWD) {      // [mask1 | mask2][wave][hidden block][lane]: 4 NF 64 entries = NF / 2 pieces each
    stage4<NF / 2, 65>(reinterpret_cast<const float4*>(a.mask1 + (size_t)blockIdx.x * 4 * NF * 64), reinterpret_cast<float4*>(mkl), c.w4, c.voff);
    stage4<NF / 2, 66>(reinterpret_cast<const float4*>(a.mask2 + (size_t)blockIdx.x * 4 * NF * 64), reinterpret_cast<float4*>(mkl + 4 * NF * 64), c.w4, c.voff);
  }

  // im2col fragments of this lane's two pixels: k-step s holds k = 32 s + 8 kq + j (natural order), scaled and split
  // (stacked forward conv1, RingS::STK: xh[s] / xl[s] = the B fragments of stacked k-steps 2 s / 2 s + 1)
  h8 xh[KS][2], xl[KS][2];
  float xmax = 0.0f;                 // range guard: largest |network input| (scaled) this lane gathers
  {
    const int hw = a.h * a.w;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int qq = qok[hf] ? q[hf] : 0;
      const int rem = qq % hw;
      const int i = rem / a.w, j0 = rem % a.w;
      const float* base = a.vin + (long)qq * a.in_stride + a.in_off;
      if constexpr (G::BWD) {
        // linear network: the pixel's gradient vector (held by its four lanes kq = 0..3) is normalised by a power of two
        float v[KS][8];
        float pm = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          gather8<KIN, false, SGN>(base, i, j0, a.h, a.w, a.in_stride, qok[hf], 32 * s + 8 * kq, v[s]);
          pm = range8(pm, v[s]);
        }
        pm = nan_max(pm, __shfl_xor(pm, 16, 64));
        pm = nan_max(pm, __shfl_xor(pm, 32, 64));
        xmax = nan_max(xmax, pm);
        const float fac = G::STORE ? 1.0f : pixel_norm(pm, a.bnorm, hc.ub[hf]);     // (training: one scale per launch, BwdArgs::go_scale)
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          split8(v[s], fac, xh[s][hf], xl[s][hf]);
        }
      } else if constexpr (S::STK) {
        xmax = gather_stacked<KIN, SGN, G::MODE7 == NET_FWD2, KS, S::KSX>(base, i, j0, a.h, a.w, a.in_stride, qok[hf], kq, xh, xl, hf, xmax);
      } else {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          float v[8];
          gather8<KIN, true, SGN>(base, i, j0, a.h, a.w, a.in_stride, qok[hf], 32 * s + 8 * kq, v);
          xmax = range8(xmax, v);
          split8(v, 1.0f, xh[s][hf], xl[s][hf]);
        }
      }
    }
  }
  if constexpr (G::FUSE) {
    if (tid < CO_PX) {
      const int qv = (int)blockIdx.x * CO_PX + tid;
      vstash[tid] = qv < a.Q ? *reinterpret_cast<const float4*>(a.vin + (size_t)qv * 4) : float4{0.f, 0.f, 0.f, 0.f};
    }
  }
  if constexpr (!G::BWD)
    for (int i = tid; i < S::EPN; i += 256) epl[i] = a.eph[i];
  // forward: the static bound; backward (normalised per pixel): only a non-finite gradient can leave the range
  if (((G::BWD && !G::STORE) ? !(xmax <= 3.0e38f) : !(xmax <= a.xlim)) && a.flag) *a.flag = 1;
  if (a.xmax_out) range_probe(a.xmax_out, xmax);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  f32x4 keep[G::NMT][2];
  if constexpr (DB) {
    co_pass_db<KIN, MOUT, NF, MODE, 0>(a, hc, cd, epl, xh, xl, lane, kq, keep);
    co_pass_db<KIN, MOUT, NF, MODE, 1>(a, hc, cd, epl, xh, xl, lane, kq, keep);
    __syncthreads();       // every wave's LDS writes of P are complete and visible (lgkmcnt(0) + barrier)
    fused_couple<CO_PX, CO_PSTR>(a, reinterpret_cast<const float*>(cd.s0), reinterpret_cast<const float*>(cd.s1), reinterpret_cast<const float*>(cd.s3), vstash, tid);
  } else if constexpr (SPLIT) {
    if (pass0 == 0) co_pass<KIN, MOUT, NF, MODE, 0, true>(a, hc, c, epl, plds, xh, xl, q, qok, lane, kq, keep);
    else co_pass<KIN, MOUT, NF, MODE, 1, true>(a, hc, c, epl, plds, xh, xl, q, qok, lane, kq, keep);
  } else {
    co_pass<KIN, MOUT, NF, MODE, 0, false>(a, hc, c, epl, plds, xh, xl, q, qok, lane, kq, keep);
    co_pass<KIN, MOUT, NF, MODE, 1, false>(a, hc, c, epl, plds, xh, xl, q, qok, lane, kq, keep);
  }
  if constexpr (G::FUSE && !DB) {
    __syncthreads();       // every wave's LDS writes of P are complete and visible (lgkmcnt(0) + barrier)
    fused_couple<CO_PX, CO_PSTR>(a, plds, vstash, tid);
  }
}
