// Launch policy of the coupling-network kernels (which kernel family, how many passes, split or not), as templates over the
// level shape.  The heavy kernels are instantiated ONLY through launch_net_t<CI, NF>; each (CI, NF) pair is explicitly
// instantiated in its own translation unit (glowk_net_inst.hip, compiled once per pair), so the ~100 kernel instances build
// in parallel; glowk.hip sees extern template declarations.
#pragma once
#include "glowk_kernels.h"
#include "glowk_co.h"
#include "glowk_q.h"

#include <cstdlib>
#include <string>

// The 16 level shapes (CI, NF) with a launch_net_t instance: CI = c / 2 of a level, NF = n_filters / 32 (512, 384, 256, 128).
// __graft_entry__.NET_SHAPES builds one glowk_net_inst.hip object per shape; a shape missing there fails the link.
#define GLOWK_NET_SHAPES(X) X(2, 16) X(4, 16) X(8, 16) X(16, 16) X(2, 12) X(4, 12) X(8, 12) X(16, 12) \
                            X(2, 8) X(4, 8) X(8, 8) X(16, 8) X(2, 4) X(4, 4) X(8, 4) X(16, 4)

// A launch request.  dir: NET_FWD (plain forward network), NET_FWD_SAVE (the gradient path's forward network, which saves the ReLU
// masks) or NET_BWD (the backward network).  arith: the exact fp32 kernel (k_net_f32) or the fp16 hi + lo split kernels, three terms
// per product or two (the two-term form exists for the plain forward network only).  store: training -- the launch also stores its
// hidden tensors planar (NetArgs::st1 / st2), in exact fp32 in any direction, in the three-term split for NET_FWD_SAVE / NET_BWD.
enum NetArith { NET_EXACT, NET_SPLIT3, NET_SPLIT2 };
struct NetCall { int dir; NetArith arith; bool store = false; };

// The counters of glowk_kernel_families, in the order include/glowk.h documents
enum NetFamily { FAM_F32, FAM_H3, FAM_H3S, FAM_H3S_HALF, FAM_FUSED, FAM_CO, FAM_Q, FAM_COUNT };

// What a launch took.  A dry call answers the same without launching (the consumers of P need the answer before the launch).
struct NetLaunch {
  int np = 0;               // partial P buffers written (P + p * pstride); 0: this form was not taken -- or the coupling was fused
  int family = FAM_F32;     // the kernel family that ran (FAM_F32 .. FAM_FUSED)
  bool co = false;          // ... in its co-resident form (k_net_h3c, glowk_co.h: four-wave / 128-pixel workgroups, two to a CU)
  bool q = false;           // ... in its small-grid form with all conv1 blocks first (k_net_h3q, glowk_q.h)
  int fused_px = 0;         // > 0: the coupling ran inside the kernel (fused_couple), in workgroups of this many pixels: no P was
                            // written, the step's output is in place but for the rows k_couple_edge finishes
  bool failed = false;      // launch_fail() has set glowk_last_error()
  bool presum = false;      // P was written with conv3's horizontal taps already added: [3 c][Q] per partial (NetArgs::pw; the forward
                            // launches of the 16x16x32 families at c = 8, 16) -- the coupling kernel is told (CoupleArgs::presum)
  int passes = 0;           // passes over the hidden width of the instance that ran: 2 or 4; 0: the exact kernel (one sweep, no passes)
  bool split = false;       // ... each pass as workgroups of its own (grid.y = passes) rather than all in one workgroup
  explicit operator bool() const { return np > 0 || fused_px > 0; }   // a form was taken
};

namespace glowk_detail {

int num_cus();                          // compute units of the current device (queried once); glowk.hip
void launch_fail(const std::string&);   // sets glowk_last_error(); glowk.hip

// Switches (parity tests of one launch form against another): environment variables, read ONCE -- when the library is loaded and
// again by glowk_reload_env() -- not per launch (round-3 verdict: six getenv() scans per flow step sat on the latency-bound path,
// ~1 200 per 30-tile gradient call).  glowk.hip owns the instance.
struct EnvSwitches {
  bool bwd_light_4;         // GLOWK_BWD_LIGHT_4: k_bwd_light with four lanes per pixel whatever the grid
  bool no_fuse;             // GLOWK_NO_FUSE: network + coupling as two kernels at the 4-channel level
  bool wgrad_plain;         // GLOWK_WGRAD_PLAIN: the weight-gradient GEMM's plain (not fenced) round
  bool co_off;              // GLOWK_CO_OFF: never the co-resident (two workgroups per CU) form of the forward network
  bool co_ring3;            // GLOWK_CO_RING3: the fused co-resident launches keep the three-slot weight ring (glowk_co.h: RingC::DB)
  bool q_off;               // GLOWK_Q_OFF: never the all-conv1-first small-grid form (glowk_q.h)
  bool co_train_off;        // GLOWK_CO_TRAIN_OFF: the training sweep stays on the 32x32x16 family
  bool train_recompute;     // GLOWK_TRAIN_RECOMPUTE: the training sweep recomputes each step's forward pass instead of keeping it
  bool train_perstep;       // GLOWK_TRAIN_PERSTEP: one saving forward launch per step instead of the level's chain
  bool no_presum;           // GLOWK_NO_PRESUM: the forward 16x16x32 kernels write per-tap P at the 8- and 16-channel levels too (NetArgs::pw = 0)
  bool pg_join;             // GLOWK_PG_JOIN: glowk_param_grad joins the caller's stream on the host first, as before the side stream
};
const EnvSwitches& env();

// kernel shape of a direction at a level: the forward networks map CI channels to 18 CI outputs (9 taps x log s, t), the backward
// network 2 CI gradient channels back to 9 CI
template <int CI, int DIR>
struct NetShape {
  static constexpr int KIN = DIR == NET_BWD ? 2 * CI : CI;
  static constexpr int MOUT = DIR == NET_BWD ? 9 * CI : 18 * CI;
};

// the exact fp32 kernel (the fallback of every split request whose shape has no instance)
template <int CI, int NF, int DIR, bool STORE>
NetLaunch launch_f32(const NetArgs& a, hipStream_t s, bool dry) {
  using Sh = NetShape<CI, DIR>;
  if (!dry) hipLaunchKernelGGL((k_net_f32<Sh::KIN, Sh::MOUT, NF, DIR, STORE>), dim3((a.Q + 127) / 128), dim3(256), 0, s, a);
  return {1, FAM_F32};
}

// k_net_h3 / k_net_h3s launch forms.  NP = passes over the hidden width: 4 where that has an instance, the caller has room for four
// partial P buffers (max_np) and the four passes fit the CUs as workgroups of their own or NP = 2 has no instance; else 2.  Where NP
// workgroups per wgs still fit the CUs in one round the passes become workgroups of their own (split): 1/NP of the latency per launch.
// np = NP partial P buffers; 0: no instance fits.
struct Passes { int np; bool split; };
// r, with the passes of the instance that ran and whether they were workgroups of their own (what the launch trace reports)
inline NetLaunch took(NetLaunch r, int passes, bool split) { r.passes = passes; r.split = split; return r; }
inline Passes pick_passes(bool fits4, bool fits2, int wgs, int max_np) {
  const int cus = num_cus();
  if (fits4 && max_np >= 4 && (4 * wgs <= cus || !fits2)) return {4, 4 * wgs <= cus};
  if (fits2) return {2, 2 * wgs <= cus};
  return {0, false};
}
// the launch of KERNEL<..., MODE_, NP_, SPLIT> (eight-wave workgroups) for a run-time split
#define GLOWK_LAUNCH_PASSES(KERNEL, MODE_, NP_, split_)                                                                  \
  do {                                                                                                                 \
    if (split_) hipLaunchKernelGGL((KERNEL<KIN, MOUT, NF, MODE_, NP_, true>), dim3(wgs, NP_), dim3(512), 0, s, a);      \
    else hipLaunchKernelGGL((KERNEL<KIN, MOUT, NF, MODE_, NP_, false>), dim3(wgs), dim3(512), 0, s, a);                 \
  } while (0)

template <int KIN, int MOUT, int NF, int MODE>
NetLaunch launch_h3(const NetArgs& a, hipStream_t s, bool dry) {
  constexpr bool F2 = RingH<KIN, MOUT, NF, MODE, 2>::FITS, F4 = RingH<KIN, MOUT, NF, MODE, 4>::FITS;
  const int wgs = (a.Q + 255) / 256;
  const Passes p = pick_passes(F4, F2, wgs, a.max_np);
  if constexpr (F4) {
    if (p.np == 4) {
      if (!dry) GLOWK_LAUNCH_PASSES(k_net_h3, MODE, 4, p.split);
      return took({4, FAM_H3}, 4, p.split);
    }
  }
  if constexpr (F2) {
    if (p.np == 2) {
      if (!dry) GLOWK_LAUNCH_PASSES(k_net_h3, MODE, 2, p.split);
      return took({2, FAM_H3}, 2, p.split);
    }
  }
  return {};
}

// does the runtime place two workgroups of this co-resident instance on a CU?  (asked once per instance: one device type per process)
template <class Kernel>
inline bool co_two_per_cu(Kernel kernel) {
  static int blocks = -1;
  if (blocks < 0) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, 0) != hipSuccess) { (void)hipGetLastError(); n = 0; }
    blocks = n;
  }
  return blocks >= 2;
}

template <int KIN, int MOUT, int NF, int MODE>
NetLaunch launch_h3s(const NetArgs& a, hipStream_t s, bool dry) {
  static_assert(!(MODE & NET_STORE), "no storing launches here: the co-resident branch does not check Q % 128 (launch_co_train does)");
  constexpr bool F2 = RingS<KIN, MOUT, NF, MODE, 2>::FITS, F4 = RingS<KIN, MOUT, NF, MODE, 4>::FITS;
  const int wgs = (a.Q + 255) / 256, cus = num_cus();
  const Passes p = pick_passes(F4, F2, wgs, a.max_np);
  if constexpr (F4) {
    if (p.np == 4) {
      if (!dry) GLOWK_LAUNCH_PASSES(k_net_h3s, MODE, 4, p.split);
      return took({4, FAM_H3S}, 4, p.split);
    }
  }
  if constexpr (F2) {
    // the coupling fused into the kernel (glowk_kernels.h: fused_couple) where the caller asks for it (NetArgs::fuse: plain forward
    // direction, geometry checked by the host), the level has four channels and both passes run in one workgroup
    // the co-resident form (glowk_co.h: four-wave / 128-pixel workgroups, two to a CU), where the caller allows it (NetArgs::co) and it
    // has an instance: on grids that fill the chip with it both passes in one workgroup -- fused (forward modes at the 4-channel
    // level) or writing P once --, on small grids (2 x Q/128 workgroups fit two to a CU) one pass per workgroup (2 partial P buffers)
    if constexpr (RingC<KIN, MOUT, NF, MODE>::FITS) {
      const int wgc = (a.Q + CO_PX - 1) / CO_PX;
      const bool co_ok = a.co && !env().co_off;
      // (grids in between -- more 128-pixel workgroups than CUs, fewer than four per CU, e.g. BASIS' 30 mixture tiles at the reference's
      //  96 x 64: the eight-wave kernel would run one two-pass workgroup on 70 % of the CUs; this form runs its workgroups two to a CU in
      //  one round up to 2 x CUs, two rounds up to 4 x CUs)
      if (co_ok && wgc > cus) {
        if constexpr (RingC<KIN, MOUT, NF, MODE | NET_FUSE>::FITS) {
          // (the form only pays with TWO workgroups per CU -- 2 x 78.8 KB of LDS, 2 x 4 x 248 VGPRs: ask the runtime once per instance, and
          //  keep the eight-wave kernel where a driver / device leaves room for one)
          // (plain forward directions: the double-buffered ring, RingC::DB, unless GLOWK_CO_RING3 asks for the three-slot instance)
          if constexpr (RingC<KIN, MOUT, NF, MODE | NET_FUSE>::DB) {
            if (a.fuse && env().co_ring3 && co_two_per_cu(k_net_h3c<KIN, MOUT, NF, MODE | NET_FUSE, false, true>)) {
              if (!dry) hipLaunchKernelGGL((k_net_h3c<KIN, MOUT, NF, MODE | NET_FUSE, false, true>), dim3(wgc), dim3(256), 0, s, a);
              return took({0, FAM_FUSED, true, false, CO_PX}, 2, false);
            }
          }
          if (a.fuse && co_two_per_cu(k_net_h3c<KIN, MOUT, NF, MODE | NET_FUSE, false>)) {
            if (!dry) hipLaunchKernelGGL((k_net_h3c<KIN, MOUT, NF, MODE | NET_FUSE, false>), dim3(wgc), dim3(256), 0, s, a);
            return took({0, FAM_FUSED, true, false, CO_PX}, 2, false);
          }
        }
        if (!a.fuse && co_two_per_cu(k_net_h3c<KIN, MOUT, NF, MODE, false>)) {
          if (!dry) hipLaunchKernelGGL((k_net_h3c<KIN, MOUT, NF, MODE, false>), dim3(wgc), dim3(256), 0, s, a);
          return took({RingC<KIN, MOUT, NF, MODE>::MERGE ? 1 : 2, FAM_H3S, true}, 2, false);
        }
      }
      if (co_ok && p.split && wgc <= cus && a.max_np >= 2 && co_two_per_cu(k_net_h3c<KIN, MOUT, NF, MODE, true>)) {
        if (!dry) hipLaunchKernelGGL((k_net_h3c<KIN, MOUT, NF, MODE, true>), dim3(wgc, 2), dim3(256), 0, s, a);
        return took({2, FAM_H3S, true}, 2, true);
      }
    }
    if constexpr ((MODE == NET_FWD || MODE == NET_FWD2 || MODE == NET_FWD_SAVE) && MOUT == 36) {
      if constexpr (RingS<KIN, MOUT, NF, MODE | NET_FUSE, 2>::FITS && RingS<KIN, MOUT, NF, MODE | NET_FUSE, 2>::MERGE) {
        if (a.fuse && !p.split) {
          if (!dry) hipLaunchKernelGGL((k_net_h3s<KIN, MOUT, NF, MODE | NET_FUSE, 2, false>), dim3(wgs), dim3(512), 0, s, a);
          return took({0, FAM_FUSED, false, false, 256}, 2, false);
        }
      }
    }
    if (!dry) GLOWK_LAUNCH_PASSES(k_net_h3s, MODE, 2, p.split);
    return took({(!p.split && RingS<KIN, MOUT, NF, MODE, 2>::MERGE) ? 1 : 2, FAM_H3S}, 2, p.split);   // (merged: the two passes' sums leave the kernel as one buffer)
  }
  return {};
}

// The 16x16x32 family with ONE 16-pixel half per wave (MODE | NET_HALF: 128-pixel workgroups, always four passes).  Twice the
// workgroups at half the work per phase: chosen where the 256-pixel workgroups with their passes as workgroups of their own
// still leave half the CUs idle (latency-bound grids: the deeper levels at the reference's batch sizes of 30 / 32 tiles), and for
// shapes whose small-conv fragments only fit the registers at one half per wave (the 32-channel level's backward network: K = 288).
inline bool half_wave_grid(const NetArgs& a) { return 8 * ((a.Q + 255) / 256) <= num_cus(); }

template <int KIN, int MOUT, int NF, int MODE>
NetLaunch launch_h3s_half(const NetArgs& a, hipStream_t s, bool dry) {
  if constexpr (RingS<KIN, MOUT, NF, MODE | NET_HALF, 4>::FITS) {
    const int wgs = (a.Q + 127) / 128;
    const Passes p = pick_passes(true, false, wgs, a.max_np);
    if (p.np != 4) return {};
    // passes as workgroups of their own, each alone on its CU: the form with all conv1 blocks first (glowk_q.h), where it has an instance
    if constexpr (RingQ<KIN, MOUT, NF, MODE>::FITS) {
      if (p.split && !env().q_off) {
        if (!dry) hipLaunchKernelGGL((k_net_h3q<KIN, MOUT, NF, MODE>), dim3(wgs, 4), dim3(512), 0, s, a);
        return took({4, FAM_H3S_HALF, false, true}, 4, true);
      }
    }
    if (!dry) GLOWK_LAUNCH_PASSES(k_net_h3s, MODE | NET_HALF, 4, p.split);
    return took({4, FAM_H3S_HALF}, 4, p.split);
  }
  return {};
}
#undef GLOWK_LAUNCH_PASSES

// the saving forward pass and the backward pass of a level must agree on the form (their ReLU-mask layouts differ: one entry per
// pixel block of a wave): both have a half-wave instance (STORE: the training sweep's launches, which also store their hiddens)
template <int CI, int NF, int STORE = 0>
constexpr bool half_ok() {
  return RingS<CI, 18 * CI, NF, NET_FWD_SAVE | STORE | NET_HALF, 4>::FITS && RingS<2 * CI, 9 * CI, NF, NET_BWD | STORE | NET_HALF, 4>::FITS;
}
// ... and for this level the half-wave form is the ONLY split form of the gradient path (no 256-pixel instance of the backward network)
template <int CI, int NF>
constexpr bool half_only() {
  return half_ok<CI, NF>() && !(RingS<2 * CI, 9 * CI, NF, NET_BWD, 2>::FITS || RingS<2 * CI, 9 * CI, NF, NET_BWD, 4>::FITS) &&
         !(RingH<2 * CI, 9 * CI, NF, NET_BWD, 2>::FITS || RingH<2 * CI, 9 * CI, NF, NET_BWD, 4>::FITS);
}
// ... of the training sweep: no 32x32x16 instance of both storing launches
template <int CI, int NF>
constexpr bool half_train_only() {
  constexpr int FS = NET_FWD_SAVE | NET_STORE, BS = NET_BWD | NET_STORE;
  return half_ok<CI, NF, NET_STORE>() && !((RingH<CI, 18 * CI, NF, FS, 2>::FITS || RingH<CI, 18 * CI, NF, FS, 4>::FITS) &&
                                           (RingH<2 * CI, 9 * CI, NF, BS, 2>::FITS || RingH<2 * CI, 9 * CI, NF, BS, 4>::FITS));
}
template <int CI, int NF>
inline bool use_half_train(const NetArgs& a) {
  if constexpr (!half_ok<CI, NF, NET_STORE>()) return false;
  return a.fam16 && a.max_np >= 4 && (half_train_only<CI, NF>() || half_wave_grid(a));
}

template <int CI, int NF>
inline bool use_half(const NetArgs& a) {
  if constexpr (!half_ok<CI, NF>()) return false;
  return a.fam16 && a.max_np >= 4 && (half_only<CI, NF>() || half_wave_grid(a));
}

// a level's saving forward pass and its backward pass run in ONE kernel family (their ReLU-mask layouts differ): the
// 16x16x32 family if both have an instance that works whatever the batch size (NP = 4 if NP = 2 does not fit needs room
// for four partial buffers, which the save buffers may not have)
// ... and only where the grid fills the chip (measured: +3.3 % at 1024 tiles, -2.5 % at 30, where the launches are split
// into passes and latency-bound).  Both launches of a level see the same pixel count, so they decide alike.
// (re-measured in round 3 with the 16x16x32 family at every grid size: 8.72 vs 8.72 ms for the gradient of 30 tiles, within +-1 % at
//  8 ... 128 tiles: no reason to change the rule the fuzz runs validated)
inline bool big_grid(const NetArgs& a) { return 2 * ((a.Q + 255) / 256) > num_cus(); }

// ... or where both launches take the one-pass-per-workgroup co-resident form (k_net_h3c<..., SPLIT>: four-wave workgroups two to a CU
// instead of one eight-wave pass-workgroup per CU): the same question for the saving and the backward launch of a level, same answer
template <int CI, int NF>
inline bool co_split_grad(const NetArgs& a) {
  if constexpr (RingC<CI, 18 * CI, NF, NET_FWD_SAVE>::FITS && RingC<2 * CI, 9 * CI, NF, NET_BWD>::FITS) {
    const int wgc = (a.Q + CO_PX - 1) / CO_PX, cus = num_cus();
    return a.co && !env().co_off && a.fam16 && a.max_np >= 2 && 2 * ((a.Q + 255) / 256) <= cus && wgc <= cus &&
           co_two_per_cu(k_net_h3c<CI, 18 * CI, NF, NET_FWD_SAVE, true>) && co_two_per_cu(k_net_h3c<2 * CI, 9 * CI, NF, NET_BWD, true>);
  }
  return false;
}

template <int CI, int NF>
constexpr bool fam16_ok() {
  return RingS<CI, 18 * CI, NF, NET_FWD_SAVE, 2>::FITS && (RingS<2 * CI, 9 * CI, NF, NET_BWD, 2>::FITS || RingS<2 * CI, 9 * CI, NF, NET_BWD, 4>::FITS);
}

// The training sweep of a level in the co-resident form (k_net_h3c<..., DIR | NET_STORE>): where both the saving forward and the
// backward network have an instance and every workgroup is full (the kernels count their stores: Q % CO_PX == 0): more workgroups
// than CUs with both passes in a workgroup (np = 1), otherwise a workgroup per pass (np = 2).  Same question, same answer for the two
// launches of a level (their ReLU-mask layouts must agree).
template <int CI, int NF, int DIR>
NetLaunch launch_co_train(const NetArgs& a, hipStream_t s, bool dry) {
  constexpr int FS = NET_FWD_SAVE | NET_STORE, BS = NET_BWD | NET_STORE;
  if constexpr (RingC<CI, 18 * CI, NF, FS>::FITS && RingC<2 * CI, 9 * CI, NF, BS>::FITS) {
    const int wgc = (a.Q + CO_PX - 1) / CO_PX, cus = num_cus();
    if (!(a.co && !env().co_off && !env().co_train_off && a.fam16 && a.Q % CO_PX == 0 && a.max_np >= 2)) return {};
    using Sh = NetShape<CI, DIR>;
    if (wgc > cus) {
      if (!(co_two_per_cu(k_net_h3c<CI, 18 * CI, NF, FS, false>) && co_two_per_cu(k_net_h3c<2 * CI, 9 * CI, NF, BS, false>))) return {};
      if (!dry) hipLaunchKernelGGL((k_net_h3c<Sh::KIN, Sh::MOUT, NF, DIR | NET_STORE, false>), dim3(wgc), dim3(256), 0, s, a);
      return took({1, FAM_H3S, true}, 2, false);
    }
    if (!(co_two_per_cu(k_net_h3c<CI, 18 * CI, NF, FS, true>) && co_two_per_cu(k_net_h3c<2 * CI, 9 * CI, NF, BS, true>))) return {};
    if (!dry) hipLaunchKernelGGL((k_net_h3c<Sh::KIN, Sh::MOUT, NF, DIR | NET_STORE, true>), dim3(wgc, 2), dim3(256), 0, s, a);
    return took({2, FAM_H3S, true}, 2, true);
  }
  return {};
}

// The plain forward network in the three-term split (half: the half-wave form may be taken); shapes without an instance run the
// exact fp32 kernel
template <int CI, int NF>
NetLaunch launch_split3_fwd(const NetArgs& a, bool half, hipStream_t s, bool dry) {
  NetLaunch r;
  if (half && a.RSp && half_wave_grid(a) && !a.fuse) r = launch_h3s_half<CI, 18 * CI, NF, NET_FWD>(a, s, dry);
  if (!r && a.RSp) r = launch_h3s<CI, 18 * CI, NF, NET_FWD>(a, s, dry);
  if (!r && a.RHp) r = launch_h3<CI, 18 * CI, NF, NET_FWD>(a, s, dry);
  if (!r) r = launch_f32<CI, NF, NET_FWD, false>(a, s, dry);
  return r;
}
// ... in the two-term split (GLOWK_PREC_F16X2): the 16x16x32 kernel only (NET_FWD2); without an instance, the three-term forms but
// the half-wave one
template <int CI, int NF>
NetLaunch launch_split2_fwd(const NetArgs& a, hipStream_t s, bool dry) {
  NetLaunch r;
  if (a.RSp) r = launch_h3s<CI, 18 * CI, NF, NET_FWD2>(a, s, dry);
  return r ? r : launch_split3_fwd<CI, NF>(a, false, s, dry);
}

// The gradient path's saving forward (DIR = NET_FWD_SAVE) or backward network (NET_BWD) in the three-term split.  The two launches
// of a level ask the same questions, so they take the same family.
template <int CI, int NF, int DIR>
NetLaunch launch_split_grad(const NetArgs& a, hipStream_t s, bool dry) {
  using Sh = NetShape<CI, DIR>;
  NetLaunch r;
  if (use_half<CI, NF>(a)) r = launch_h3s_half<Sh::KIN, Sh::MOUT, NF, DIR>(a, s, dry);
  if constexpr (fam16_ok<CI, NF>()) {
    if (!r && a.fam16 && (big_grid(a) || co_split_grad<CI, NF>(a))) r = launch_h3s<Sh::KIN, Sh::MOUT, NF, DIR>(a, s, dry);
  }
  if (!r && a.RHp) r = launch_h3<Sh::KIN, Sh::MOUT, NF, DIR>(a, s, dry);
  if (!r) r = launch_f32<CI, NF, DIR, false>(a, s, dry);
  return r;
}

inline NetLaunch net_failed(const std::string& m) { launch_fail(m); NetLaunch r; r.failed = true; return r; }

// The training sweep in the three-term split: the same two launches, storing their hiddens.  No exact fallback (the sweep's weight
// gradients expect the split units): not taken if the shape has no instance -- glowk_param_grad asks dry before it chooses the
// arithmetic of the sweep.
template <int CI, int NF, int DIR>
NetLaunch launch_split_train(const NetArgs& a, hipStream_t s, bool dry) {
  using Sh = NetShape<CI, DIR>;
  constexpr int MODE = DIR | NET_STORE;
  NetLaunch r;
  if (use_half_train<CI, NF>(a)) r = launch_h3s_half<Sh::KIN, Sh::MOUT, NF, MODE>(a, s, dry);
  if (!r) r = launch_co_train<CI, NF, DIR>(a, s, dry);
  if (!r && a.RHp) r = launch_h3<Sh::KIN, Sh::MOUT, NF, MODE>(a, s, dry);
  if (!r && !dry) return net_failed("no split-arithmetic training instance for this shape");
  return r;
}

// exact fp32: the kernel of the direction, storing or not
template <int CI, int NF, bool STORE>
NetLaunch launch_exact(const NetArgs& a, int dir, hipStream_t s, bool dry) {
  if (dir == NET_FWD) return launch_f32<CI, NF, NET_FWD, STORE>(a, s, dry);
  if (dir == NET_FWD_SAVE) return launch_f32<CI, NF, NET_FWD_SAVE, STORE>(a, s, dry);
  return launch_f32<CI, NF, NET_BWD, STORE>(a, s, dry);
}

// The policy: which kernel instance a request launches, on which grid.  A request with no launch form (a two-term or storing plain
// forward split, a two-term saving or backward network, an unknown direction) fails.
template <int CI, int NF>
NetLaunch launch_net_t(const NetArgs& a, NetCall call, hipStream_t s, bool dry) {
  const bool save = call.dir == NET_FWD_SAVE;
  if (call.dir != NET_FWD && !save && call.dir != NET_BWD) return net_failed("bad k_net mode");
  NetLaunch r;
  if (call.arith == NET_EXACT) {
    r = !call.store ? launch_exact<CI, NF, false>(a, call.dir, s, dry) : launch_exact<CI, NF, true>(a, call.dir, s, dry);
  } else if (call.store) {
    if (call.dir == NET_FWD || call.arith != NET_SPLIT3) return net_failed("bad k_net mode");
    r = save ? launch_split_train<CI, NF, NET_FWD_SAVE>(a, s, dry) : launch_split_train<CI, NF, NET_BWD>(a, s, dry);
  } else if (call.dir == NET_FWD) {
    r = call.arith == NET_SPLIT3 ? launch_split3_fwd<CI, NF>(a, true, s, dry) : launch_split2_fwd<CI, NF>(a, s, dry);
  } else {
    if (call.arith != NET_SPLIT3) return net_failed("bad k_net mode");
    r = save ? launch_split_grad<CI, NF, NET_FWD_SAVE>(a, s, dry) : launch_split_grad<CI, NF, NET_BWD>(a, s, dry);
  }
  if (!dry && !r.failed) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return net_failed(std::string("k_net: ") + hipGetErrorString(e));
  }
  // every forward form of the 16x16x32 families closes with the same conv3 ops (h3s_Z / co_Z), which pre-sum where the host set the width
  r.presum = a.pw != 0 && call.dir != NET_BWD && (r.family == FAM_H3S || r.family == FAM_H3S_HALF) && RingS<CI, 18 * CI, NF, NET_FWD, 2>::C3P;
  return r;
}

}  // namespace glowk_detail
