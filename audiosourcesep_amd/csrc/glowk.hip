// glowk engine core: weight store, launch sequencing and the inference part of the C ABI of include/glowk.h.
// Build: __graft_entry__.build (hipcc --offload-arch=gfx950; one object per translation unit, linked into libglowk.so)
#include "glowk_engine.h"
#include "glowk_light.h"

namespace glowk_eng {
thread_local std::string g_err;
}
using namespace glowk_eng;

namespace glowk_detail {
int num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0; hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
    if (n <= 0) n = 256;
  }
  return n;
}
void launch_fail(const std::string& m) { fail(m); }
static EnvSwitches read_env() {
  auto on = [](const char* n) { return getenv(n) != nullptr; };
  return EnvSwitches{on("GLOWK_BWD_LIGHT_4"), on("GLOWK_NO_FUSE"), on("GLOWK_WGRAD_PLAIN"), on("GLOWK_CO_OFF"), on("GLOWK_CO_RING3"), on("GLOWK_Q_OFF"), on("GLOWK_CO_TRAIN_OFF"),
                     on("GLOWK_TRAIN_RECOMPUTE"), on("GLOWK_TRAIN_PERSTEP"), on("GLOWK_NO_PRESUM"), on("GLOWK_PG_JOIN")};
}
static EnvSwitches g_env = read_env();
const EnvSwitches& env() { return g_env; }
void reload_env() { g_env = read_env(); }
// instantiated in glowk_net_inst.hip, one translation unit per (CI, NF)
#define GLOWK_EXTERN_NET(CI_, NF_) extern template NetLaunch launch_net_t<CI_, NF_>(const NetArgs&, NetCall, hipStream_t, bool);
GLOWK_NET_SHAPES(GLOWK_EXTERN_NET)
#undef GLOWK_EXTERN_NET
}  // namespace glowk_detail

namespace glowk_eng {
using glowk_detail::num_cus;
using glowk_detail::launch_net_t;

// The network launch of direction dir in the handle's arithmetic: exact fp32 in GLOWK_PREC_F32 or where the step has no split image
// for it (split = false); otherwise the three-term split, but for the plain forward network of GLOWK_PREC_F16X2 (the only two-term
// launch).  store: a training launch that also stores its hiddens.
NetCall net_call(const glowk_handle* h, int dir, bool store, bool split) {
  if (h->precision == GLOWK_PREC_F32 || !split) return NetCall{dir, NET_EXACT, store};
  return NetCall{dir, h->precision == GLOWK_PREC_F16X2 && dir == NET_FWD && !store ? NET_SPLIT2 : NET_SPLIT3, store};
}

// the light kernels raise the sticky range flag only for calls in a split arithmetic (in exact fp32 a non-finite value is the
// reference's own result, and the fp32 re-run of the FALLBACK policy must not re-arm it)
int* flagp(const glowk_handle* h) { return h->precision == GLOWK_PREC_F32 ? nullptr : h->d_flag; }

// normalisation target of the split backward kernels for a step whose static bound allows inputs up to xlim_b (scaled units):
// the largest power of two T with 2 T <= xlim_b, at most 2^10; 0 if even 2^-4 does not fit
float bwd_norm_target(float xlim_b) {
  if (!(xlim_b >= 0.125f)) return 0.0f;
  int e = 0;
  std::frexp(xlim_b * 0.5f, &e);                 // xlim_b / 2 = f 2^e, f in [0.5, 1): largest power of two <= it is 2^(e-1)
  return std::ldexp(1.0f, std::min(e - 1, 10));
}

NetLaunch launch_net_raw(int c, int F, const NetArgs& a, NetCall call, hipStream_t s, bool dry) {
#define NETCASE(CI_, NF_) if (c == 2 * CI_ && F == 32 * NF_) return launch_net_t<CI_, NF_>(a, call, s, dry);
  GLOWK_NET_SHAPES(NETCASE)
#undef NETCASE
  return glowk_detail::net_failed("unsupported (channels, n_filters) combination: c=" + std::to_string(c) + " F=" + std::to_string(F));
}

// One record of the launch trace (glowk_net_trace_begin): the request and what the launch functions report they took (NetLaunch);
// nothing is derived a second time here.  Called only while the trace is armed.
static void trace_net(glowk_handle* h, int level, const NetArgs& a, NetCall call, const NetLaunch& r) {
  glowk_net_record rec;
  rec.level = level; rec.dir = call.dir; rec.arith = (int)call.arith; rec.store = call.store ? 1 : 0; rec.Q = a.Q;
  rec.family = r.family; rec.passes = r.passes; rec.split = r.split ? 1 : 0; rec.np = r.np; rec.co = r.co ? 1 : 0; rec.q = r.q ? 1 : 0;
  rec.fused_px = r.fused_px; rec.presum = r.presum ? 1 : 0;
  h->net_trace.push_back(rec);
}

// out: what the launch took (NetLaunch::np partial P buffers, for the consumer).  Counts the launch into glowk_kernel_families; the
// calls of launch_net_raw alone (the recompute launch of the training sweep, dry queries) are not counted.
int launch_net(glowk_handle* h, int level, int c, int F, const NetArgs& a, hipStream_t s, NetCall call, NetLaunch* out = nullptr) {
  if (h->profiling) {
    while (h->ev_pool.size() < h->ev_used + 2) {
      OwnedEvent e;
      HIPCHK(event_create(e, hipEventDefault));
      h->ev_pool.push_back(std::move(e));
    }
    HIPCHK(hipEventRecord(h->ev_pool[h->ev_used], s));
  }
  const NetLaunch r = launch_net_raw(c, F, a, call, s);
  if (!r.failed) {
    ++h->family_launches[r.family];
    if (r.co) ++h->family_launches[FAM_CO];
    if (r.q) ++h->family_launches[FAM_Q];
    if (h->net_tracing) trace_net(h, level, a, call, r);
  }
  if (h->profiling) {
    HIPCHK(hipEventRecord(h->ev_pool[h->ev_used + 1], s));
    h->ev_used += 2;
    h->ev_level.push_back(level);
  }
  if (out) *out = r;
  return r.failed ? 1 : 0;
}

// light backward kernel of one step: 16 lanes per pixel where the batch is small and the level deep (few pixels, many channels and
// partial buffers: the gathers' dependent loads are what the launch waits for), one where the grid is large, else 4
int bwd_light_lanes(int c, const BwdArgs& a) {
  if (glowk_detail::env().bwd_light_4) return 4;
  // large grids: one lane per pixel (the planar Pg gathers and the 16-byte rows of the [Q][C] arrays are then fully coalesced)
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if ((a.Q + 255) / 256 >= 2 * num_cus() && al16(a.ghalf_in) && al16(a.v) && al16(a.osave) && al16(a.g_o) && al16(a.ghalf_out) &&
      al16(a.gu_out) && al16(a.gv_out)) return 1;
  return c >= 8 && (a.Q + 15) / 16 <= 8 * num_cus() ? 16 : 4;
}

int launch_bwd_light(int c, const BwdArgs& a, hipStream_t s) {
#define BWD_LIGHT(LPP_) CDISPATCH(c, hipLaunchKernelGGL((k_bwd_light<CC, LPP_>), dim3((a.Q + 256 / LPP_ - 1) / (256 / LPP_)), dim3(256), 0, s, a))
  switch (bwd_light_lanes(c, a)) {
    case 1: BWD_LIGHT(1); break;
    case 16: BWD_LIGHT(16); break;
    default: BWD_LIGHT(4);
  }
#undef BWD_LIGHT
  LAUNCHCHK("k_bwd_light");
  return 0;
}

// log-det slots of the flat-grid coupling kernel (k_couple_flat): slot[n * stride + base + workgroup within the sample]
struct FlatLd { double* slot; int stride, base; };

// Launch form of the coupling: a flat grid over the pixels (k_couple_flat: 4 or 16 lanes per pixel, 256 threads) or one workgroup of
// `threads` per sample (k_couple: 1 or 4 lanes per pixel)
struct CoupleForm { bool flat; int lanes, threads; };

// slots: the caller has log-det slots for the flat grid (FlatLd), which a launch with a log-det needs there
CoupleForm couple_form(int c, const CoupleArgs& a, int N, bool slots) {
  const int hw = a.h * a.w;
  // few samples: a flat grid over the pixels instead of one workgroup per sample (30 tiles: 30 workgroups on 256 CUs); sixteen
  // lanes per pixel where the level is deep (c >= 8) and small
  if (N < 2 * num_cus() && hw % 64 == 0 && (!a.logdet || slots)) return {true, c >= 8 && (a.Q + 15) / 16 <= 8 * num_cus() ? 16 : 4, 256};
  if (N >= 2 * num_cus()) return {false, 1, 256};   // enough per-sample workgroups to fill the chip: one lane per pixel
  return {false, 4, hw >= 256 ? 1024 : hw > 64 ? 512 : 256};   // four lanes per pixel, up to 256 pixels in flight per sample
}

// (PDISPATCH: the instances that read the pre-summed P, which only the 8- and 16-channel levels write; the launches keep their order, and so the kernels their offsets)
#define PDISPATCH(c, CALL)                                                                     \
  switch (c) {                                                                                 \
    case 8: { constexpr int CC = 8; CALL; } break;                                             \
    case 16: { constexpr int CC = 16; CALL; } break;                                           \
    default: return fail("pre-summed P at channel count " + std::to_string(c));                \
  }
#define COUPLE_FLAT(DISPATCH, LPP_, PRE_) \
  DISPATCH(c, hipLaunchKernelGGL((k_couple_flat<CC, LPP_, PRE_>), dim3((a.Q + 256 / LPP_ - 1) / (256 / LPP_)), dim3(256), 0, s, a, slots, stride, base))
#define COUPLE_TILE(DISPATCH, QUAD_, PRE_) DISPATCH(c, hipLaunchKernelGGL((k_couple<CC, QUAD_, PRE_>), dim3(N), dim3(f.threads), 0, s, a))

int launch_couple(int c, CoupleArgs a, int N, hipStream_t s, const FlatLd* fl = nullptr, bool* flat_used = nullptr) {
  const CoupleForm f = couple_form(c, a, N, fl && fl->slot);
  double* slots = f.flat && a.logdet ? fl->slot : nullptr;   // flat: the log-det goes to the slots (k_ld_fold adds them up)
  if (slots && flat_used) *flat_used = true;
  if (f.flat) a.logdet = nullptr;
  const int stride = fl ? fl->stride : 0, base = fl ? fl->base : 0;
  if (f.flat && a.presum) { if (f.lanes == 16) { COUPLE_FLAT(PDISPATCH, 16, true); } else { COUPLE_FLAT(PDISPATCH, 4, true); } }
  else if (f.flat) { if (f.lanes == 16) { COUPLE_FLAT(CDISPATCH, 16, false); } else { COUPLE_FLAT(CDISPATCH, 4, false); } }
  else if (f.lanes == 1) { if (a.presum) { COUPLE_TILE(PDISPATCH, false, true); } else { COUPLE_TILE(CDISPATCH, false, false); } }
  else { if (a.presum) { COUPLE_TILE(PDISPATCH, true, true); } else { COUPLE_TILE(CDISPATCH, true, false); } }
  LAUNCHCHK((f.flat ? "k_couple_flat" : "k_couple"));
  return 0;
}
#undef COUPLE_TILE
#undef COUPLE_FLAT
#undef PDISPATCH

// One flow step's coupling network + coupling.  Plain forward direction of the split arithmetics at the 4-channel level with a grid
// that fills the chip: ONE kernel (k_net_h3s<..., MODE | NET_FUSE>: the per-tap conv3 outputs never leave the workgroup) plus
// k_couple_edge for the pixel rows whose 3 x 3 neighbourhood straddles two workgroups and the per-sample log-det; otherwise k_net
// (P to HBM) + k_couple.  na: the network launch (na.P / pstride as for launch_net); ca: the coupling as k_couple takes it, but for
// P / np / pstride, which the network launch decides.
bool fuse_geometry_ok(int h, int w, int pxw = 256) {     // pxw: pixels per workgroup of the fused kernel
  const int hw = h * w;
  if (w < 4 || w > FUSE_EW || (w & (w - 1)) || pxw % w) return false;
  if (hw % pxw == 0) return true;
  return hw >= 32 && hw < pxw && (hw & (hw - 1)) == 0;
}

// k_couple_edge after the fused launch na of the coupling ca, in workgroups of pxw pixels
EdgeArgs edge_args(const CoupleArgs& ca, const NetArgs& na, int pxw) {
  EdgeArgs ea;
  ea.vin = ca.vin; ea.edge = na.fz_edge; ea.ldpart = na.fz_ldpart; ea.A = ca.A; ea.b = ca.b;
  ea.out = ca.out; ea.out_stride = ca.out_stride; ea.out_off = ca.out_off; ea.inverse = ca.inverse;
  ea.logdet = ca.logdet; ea.osave = ca.o_save; ea.h = ca.h; ea.w = ca.w; ea.flag = ca.flag; ea.pxw = pxw;
  return ea;
}
// the coupling a reading what the network launch r left in P
CoupleArgs couple_reads(CoupleArgs a, const float* P, size_t pstride, const NetLaunch& r) {
  a.P = P; a.np = r.np; a.pstride = pstride; a.presum = r.presum ? 1 : 0;
  return a;
}

int net_and_couple(glowk_handle* h, int lvl, int c, int F, NetArgs na, CoupleArgs ca, int N, hipStream_t s, NetCall call, const FlatLd* fl = nullptr,
                   bool* flat_used = nullptr) {
  const bool no_fuse = glowk_detail::env().no_fuse;            // (A/B timing and the fused-vs-unfused parity test, which calls glowk_reload_env)
  const bool fusable = call.arith != NET_EXACT && call.dir != NET_BWD && !call.store;   // the split forward networks, saving or not
  const int hw = ca.h * ca.w;
  if (!no_fuse && c == 4 && fusable && na.RSp && ca.vin && !ca.log_s_out && ca.out && na.in_stride == 4 &&
      ca.out_stride % 4 == 0 && ca.out_off % 4 == 0 && fuse_geometry_ok(ca.h, ca.w) && na.P == h->bufP) {
    // (scratch sized for the co-resident form's 128-pixel workgroups when it may be taken: twice the edge slots)
    const size_t pxw = (na.co && fuse_geometry_ok(ca.h, ca.w, CO_PX)) ? CO_PX : 256;
    if (pxw == 256) na.co = 0;
    const size_t wgs = ((size_t)ca.Q + pxw - 1) / pxw;
    const size_t edge_floats = (wgs * 4 * FUSE_EW * 4 + 3) & ~(size_t)3;
    const size_t nld = wgs * (pxw / 32);                                  // one fp64 log-det partial per wave (32 pixels), idle waves of a ragged last workgroup included
    if ((edge_floats + 2 * nld + 4) <= 4 * h->pstride) {                // (the scratch lives in the P buffers the fused launch does not use)
      na.fuse = 1;
      na.fz_b3 = ca.b3; na.fz_A = ca.A; na.fz_b = ca.b; na.fz_out = ca.out; na.fz_out_stride = ca.out_stride; na.fz_out_off = ca.out_off;
      na.fz_inverse = ca.inverse;
      na.fz_osave = ca.o_save;
      na.fz_edge = h->bufP;
      na.fz_ldpart = ca.logdet ? reinterpret_cast<double*>(h->bufP + edge_floats) : nullptr;
    }
  }
  NetLaunch r;
  if (int rc = launch_net(h, lvl, c, F, na, s, call, &r)) return rc;
  if (!r.fused_px) return launch_couple(c, couple_reads(ca, na.P, na.pstride, r), N, s, fl, flat_used);
  ++h->fused_steps;
  const int pxw = r.fused_px;
  if (hw > pxw || ca.logdet) {
    hipLaunchKernelGGL(k_couple_edge, dim3(N), dim3(256), 0, s, edge_args(ca, na, pxw));
    LAUNCHCHK("k_couple_edge");
  }
  return 0;
}

PreArgs pre_args(const glowk_config& cfg) { return PreArgs{cfg.minval, cfg.maxval, cfg.alpha, cfg.use_logit}; }

// ---- device memory of a handle: ONE description of every buffer, used by the allocators and by glowk_workspace_bytes ----
struct WsSizes {      // forward / inverse workspace for N tiles (bytes)
  size_t act, P, ld;  // bufA, bufB, bufZ (each) | bufP (4 partial per-tap buffers) | bufLd
  size_t slots;       // bufLdSlot: per-sample log-det slots of the flat-grid coupling kernel (small batches only)
  size_t total() const { return 3 * act + P + ld + slots; }
};
// log-det slots per sample: one per flow step and 16 pixels of its level
int ld_slots_per_sample(const glowk_handle* h) {
  int n = 0;
  for (const Level& lv : h->levels) n += h->cfg.K * ((lv.h * lv.w + 15) / 16);
  return n;
}
WsSizes ws_sizes(const glowk_handle* h, size_t N) {
  const size_t E = (size_t)h->cfg.H * h->cfg.W * h->cfg.C;
  return WsSizes{N * E * 4, 4 * 9 * N * E * 4, N * 8, std::min(N, (size_t)2 * num_cus()) * ld_slots_per_sample(h) * 8};
}
// pixel blocks of the ReLU-mask arrays of a level with Q pixels (one 16-bit entry per lane, hidden block and pixel block of a wave):
// 32-pixel blocks of whole 256-pixel workgroups -- or 16-pixel blocks of 128-pixel workgroups where the launch policy may pick the
// half-wave form of the 16x16x32 family (glowk_launch.h: use_half -- small grids, and the 32-channel level at any size)
// MONOTONE in Q (round-3 advisor): the per-step offsets (offM) are laid out once for the largest batch a handle has seen and a later,
// smaller call computes its own mask2 = mask1 + blocks inside that layout -- so a smaller Q must never need MORE blocks.  The
// half-wave form needs ceil(Q / 128) * 8 blocks up to the largest Q the policy picks it for (Qh = 256 * floor(CUs / 8) pixels) and
// the 256-pixel form ceil(Q / 256) * 8 beyond: the bound is the larger of the latter and the former capped at Qh.
size_t mask_blocks(const Level& lv, size_t Q) {
  const size_t b256 = ((Q + 255) / 256) * 8;
  if (lv.c == 32) return ((Q + 127) / 128) * 8;
  const size_t Qh = (size_t)256 * (size_t)(num_cus() / 8);
  return std::max(b256, ((std::min(Q, Qh) + 127) / 128) * 8);
}

struct SaveSizes {    // input-gradient path for N tiles: per-step saves + scratch
  size_t v, p, m;     // floats of saveV, floats of saveP, shorts of saveM
  int np;             // (1: kept for the size formula)
  size_t gz, c;       // bytes of bufGz, bufC
  size_t total() const { return v * 4 + (size_t)np * p * 4 + m * 2 + gz + c; }
};
SaveSizes save_sizes(const glowk_handle* h, size_t N, std::vector<size_t>* offV = nullptr, std::vector<size_t>* offP = nullptr,
                     std::vector<size_t>* offM = nullptr) {
  const int K = h->cfg.K, L = h->cfg.L, NF = h->cfg.F / 32;
  SaveSizes S{0, 0, 0, 1, 0, 0};
  if (offV) { offV->assign((size_t)L * K, 0); offP->assign((size_t)L * K, 0); offM->assign((size_t)L * K, 0); }
  for (int lvl = 0; lvl < L; ++lvl) {
    const Level& lv = h->levels[lvl];
    const size_t Q = N * lv.h * lv.w;
    const size_t blocks = mask_blocks(lv, Q);
    for (int j = 0; j < K; ++j) {
      const size_t sidx = (size_t)lvl * K + j;
      if (offV) { (*offV)[sidx] = S.v; (*offP)[sidx] = S.p; (*offM)[sidx] = S.m; }
      S.v += Q * lv.c;
      S.p += Q * (lv.c / 2);
      S.m += 2 * blocks * NF * 64;   // mask1 then mask2
    }
  }
  const size_t E = (size_t)h->cfg.H * h->cfg.W * h->cfg.C;
  S.gz = N * E * 4;
  S.c = N * E * 4;
  return S;
}

int ensure_flag(glowk_handle* h) {
  if (h->d_flag) return 0;
  DeviceMem<int> d_flag;      // both words, or neither: moved in once both exist
  PinnedMem<int> h_flag;
  HIPCHK(dev_alloc(d_flag, 16));
  HIPCHK(hipMemset(d_flag, 0, 16));
  HIPCHK(pinned_alloc(h_flag, 16));
  h_flag[0] = 0;
  h->d_flag = std::move(d_flag);
  h->h_flag = std::move(h_flag);
  return 0;
}

int ensure_ws(glowk_handle* h, int N) {
  if (int rc = ensure_flag(h)) return rc;
  if (N <= h->wsN) return 0;
  HIPCHK(hipDeviceSynchronize());
  h->bufA.reset(); h->bufB.reset(); h->bufP.reset(); h->bufZ.reset(); h->bufLd.reset(); h->bufLdSlot.reset(); h->wsN = 0;
  const WsSizes W = ws_sizes(h, (size_t)N);
  HIPCHK(dev_alloc(h->bufA, W.act));
  HIPCHK(dev_alloc(h->bufB, W.act));
  h->pstride = W.P / 16;          // floats per partial
  HIPCHK(dev_alloc(h->bufP, W.P));
  HIPCHK(dev_alloc(h->bufZ, W.act));
  HIPCHK(dev_alloc(h->bufLd, W.ld));
  HIPCHK(dev_alloc(h->bufLdSlot, W.slots));
  h->wsN = N;
  return 0;
}

// scratch tensor of the gradient path / the ActNorm initialisation (one level tensor)
int ensure_c(glowk_handle* h, int N) {
  if ((size_t)N <= h->cN) return 0;
  HIPCHK(hipDeviceSynchronize());
  h->bufC.reset(); h->cN = 0;
  HIPCHK(dev_alloc(h->bufC, (size_t)N * h->cfg.H * h->cfg.W * h->cfg.C * 4));
  h->cN = (size_t)N;
  return 0;
}

// pixel and element indices of a call are 32-bit in the light kernels: one call takes at most 2^28 elements (1 GiB of tiles,
// 22 GB of workspace); larger batches are the caller's loop (the Python mirror chunks by glowk_max_tiles)
int max_tiles(const glowk_handle* h) {
  const long long E = (long long)h->cfg.H * h->cfg.W * h->cfg.C;
  const long long m = (1LL << 28) / E;
  return m < 1 ? 1 : (int)m;
}

int check_batch(const glowk_handle* h, int N) {
  if (N <= 0) return fail("batch size must be positive");
  if (N > max_tiles(h)) return fail("batch of " + std::to_string(N) + " tiles exceeds glowk_max_tiles() = " + std::to_string(max_tiles(h)) +
                                    " (32-bit indices within one call): split the batch");
  return 0;
}

int check_ready(glowk_handle* h, int N) {
  if (!h) return fail("null handle");
  if (h->finalized && h->split_stale && h->precision != GLOWK_PREC_F32)   // trained since the f16 images were packed: re-pack (host, ~0.3 s)
    if (int rc = glowk_finalize_weights(h)) return rc;
  if (!h->finalized) return fail("glowk_finalize_weights has not been called");
  if (int rc = check_batch(h, N)) return rc;
  return ensure_ws(h, N);
}

// The network launch of step sd of level lv on vin, as the plain forward network takes it (the gradient path's launches add their masks,
// the backward network swaps in its own images, net_and_couple adds the coupling of a fused launch)
NetArgs net_args(glowk_handle* h, const Level& lv, const StepDev& sd, const float* vin, int in_stride, int in_off, int N) {
  NetArgs a;
  a.vin = vin; a.in_stride = in_stride; a.in_off = in_off;
  a.Q = N * lv.h * lv.w; a.h = lv.h; a.w = lv.w;
  a.K1p = sd.K1p; a.ep = sd.ep; a.R0p = sd.R0p; a.P = h->bufP; a.pstride = h->pstride;
  a.RHp = sd.RHp; a.RSp = sd.RSp; a.fam16 = (sd.RSp && sd.RSBp) ? 1 : 0; a.eph = sd.epH; a.sc1 = sd.sc1; a.sc2 = sd.sc2; a.sc3 = sd.sc3;
  a.flag = flagp(h); a.xlim = sd.xlim_f;
  a.co = glowk_detail::env().co_off ? 0 : 1;
  // conv3's horizontal taps added in the forward 16x16x32 kernels (c3_presum_store): the level shape alone decides, so that every launch
  // form of a shape -- whatever the batch size selects -- writes the same layout and adds in the same order
  a.pw = (!glowk_detail::env().no_presum && (lv.c == 8 || lv.c == 16) && lv.w >= 4 && lv.w <= 16 && (lv.w & (lv.w - 1)) == 0) ? lv.w : 0;
  a.xmax_out = h->d_probe ? h->d_probe + ((&lv - h->levels.data()) * h->cfg.K + (&sd - lv.dev.data())) : nullptr;
  return a;
}

// The coupling of step sd of level lv on vin, result to out (element (q, co) at out[q * out_stride + out_off + co]; null: none).  The
// caller adds what its call has beyond that (the following affine, log-det, saves, dumps); which P the kernel reads is the network
// launch's answer (couple_reads).
CoupleArgs couple_args(const glowk_handle* h, const Level& lv, const StepDev& sd, const float* vin, int N, int inverse, float* out,
                       int out_stride, int out_off = 0) {
  CoupleArgs a;
  a.vin = vin; a.b3 = sd.b3; a.out = out; a.out_stride = out_stride; a.out_off = out_off;
  a.Q = N * lv.h * lv.w; a.h = lv.h; a.w = lv.w; a.inverse = inverse; a.flag = flagp(h);
  return a;
}

// The light backward launch of level lv: geometry, flag and the scale that undoes the sweep's power of two on the network gradients
// (bfac: BwdArgs::go_scale of the level's launches that write g_o).  The caller adds the gradient's source, the affine and the coupling.
BwdArgs bwd_args(const glowk_handle* h, const Level& lv, int N, float bfac) {
  BwdArgs a;
  a.Q = N * lv.h * lv.w; a.h = lv.h; a.w = lv.w; a.flag = flagp(h); a.pg_scale = 1.0f / bfac;
  return a;
}

// per-step save buffers of the input-gradient path, forward order index sidx = level*K + (K-1-k)
int ensure_save(glowk_handle* h, int N) {
  if (int rc = ensure_c(h, N)) return rc;
  if (N <= h->saveN) return 0;
  const int Na = std::max(N, h->saveN);
  HIPCHK(hipDeviceSynchronize());
  h->saveV.reset(); h->saveP.reset(); h->saveM.reset(); h->bufGz.reset(); h->saveN = 0;
  SaveSizes S = save_sizes(h, (size_t)Na, &h->offV, &h->offP, &h->offM);
  HIPCHK(dev_alloc(h->saveV, S.v * 4));
  HIPCHK(dev_alloc(h->saveP, S.p * 4));
  HIPCHK(dev_alloc(h->saveM, S.m * 2));
  HIPCHK(dev_alloc(h->bufGz, S.gz));
  h->saveN = Na;
  return 0;
}

// data -> latent (+ log-det accumulated in h->bufLd); z_dst [N,Hl,Wl,Cl].  save: keep every step's coupling input v,
// per-tap conv3 outputs P and the two ReLU masks for run_backward.
int run_forward(glowk_handle* h, const float* x, int N, float* z_dst, hipStream_t s, bool save, bool keep_hidden) {
  const glowk_config& cfg = h->cfg;
  const int K = cfg.K, L = cfg.L, NF = cfg.F / 32;
  float* cur = save ? h->saveV + h->offV[0] : h->bufA;
  float* oth = h->bufB;
  // small batches: the coupling kernels run on a flat pixel grid and leave their log-det shares in per-workgroup slots (k_couple_flat)
  const int nslots = ld_slots_per_sample(h);
  // (the plain forward direction and the saving pass of the split arithmetics: network + coupling may run as one kernel, net_and_couple)
  const NetCall call = net_call(h, save ? NET_FWD_SAVE : NET_FWD, keep_hidden);
  const bool flat_ok = N < 2 * num_cus() && h->bufLdSlot;
  bool flat_used = false;
  int slot_base = 0;
  if (flat_ok) HIPCHK(hipMemsetAsync(h->bufLdSlot, 0, (size_t)N * nslots * 8, s));
  {
    const Level& lv = h->levels[0];
    const StepDev& first = lv.dev[K - 1];
    CDISPATCH(lv.c, hipLaunchKernelGGL((k_in<CC>), dim3(N), dim3(256), 0, s, x, cfg.H, cfg.W, pre_args(cfg), 1,
                                       first.Afwd, first.bfwd, cur, h->bufLd, h->ld_const + h->ld_pre_const));
    LAUNCHCHK("k_in");
  }
  for (int lvl = 0; lvl < L; ++lvl) {
    const Level& lv = h->levels[lvl];
    const size_t Q = (size_t)N * lv.h * lv.w;
    const size_t blocks = mask_blocks(lv, Q);
    for (int k = K - 1; k >= 0; --k) {   // tfb.Chain applies right to left: step K-1 first (flow_glow.py:51-52)
      const StepDev& sd = lv.dev[k];
      const size_t sidx = (size_t)lvl * K + (K - 1 - k);
      NetArgs na = net_args(h, lv, sd, cur, lv.c, lv.c / 2, N);
      if (save) {
        na.mask1 = h->saveM + h->offM[sidx];
        na.mask2 = na.mask1 + blocks * NF * 64;
      }
      if (keep_hidden) {   // training: this launch also leaves relu(conv1 + b1), relu(conv2 + b2) planar for the weight gradients
        na.st1 = h->trKeep + h->trKeepOff[sidx] * (size_t)N;
        na.st2 = na.st1 + (size_t)cfg.F * Q;
      }
      float* next = save && k > 0 ? h->saveV + h->offV[sidx + 1] : oth;
      const bool last = k == 0 && lvl == L - 1;    // the last step of all writes its slice of the latent
      CoupleArgs ca = last ? couple_args(h, lv, sd, cur, N, 0, z_dst, h->Cl, lv.z_off) : couple_args(h, lv, sd, cur, N, 0, k > 0 ? next : oth, lv.c);
      ca.logdet = h->bufLd;
      if (save) ca.o_save = h->saveP + h->offP[sidx];
      if (k > 0) { ca.A = lv.dev[k - 1].Afwd; ca.b = lv.dev[k - 1].bfwd; }    // the next step's ActNorm + 1x1
      const FlatLd fl{flat_ok ? h->bufLdSlot : nullptr, nslots, slot_base};
      slot_base += (lv.h * lv.w + 15) / 16;
      if (int rc = net_and_couple(h, lvl, lv.c, cfg.F, na, ca, N, s, call, &fl, &flat_used)) return rc;
      if (k > 0) {
        if (save) cur = next; else std::swap(cur, oth);
      } else if (lvl < L - 1) {
        // block output sits in oth; split + squeeze + first ActNorm/1x1 of the next block
        float* nv = save ? h->saveV + h->offV[sidx + 1] : cur;
        const StepDev& nfirst = h->levels[lvl + 1].dev[K - 1];
        CDISPATCH(lv.c, hipLaunchKernelGGL((k_split<CC>), dim3(N), dim3(256), 0, s, (const float*)oth, lv.h, lv.w, z_dst, h->Hl * h->Wl, h->Cl,
                                           lv.z_off, lv.Cz, nfirst.Afwd, nfirst.bfwd, nv));
        LAUNCHCHK("k_split");
        cur = nv;
        if (!save) oth = (cur == h->bufA) ? h->bufB : h->bufA;
      }
    }
  }
  if (flat_used) {
    hipLaunchKernelGGL(k_ld_fold, dim3(N), dim3(64), 0, s, h->bufLd, (const double*)h->bufLdSlot, nslots);
    LAUNCHCHK("k_ld_fold");
  }
  return 0;
}

// d sum_n log_prob[n] / dx, after run_forward(save = true) on the same x; z is that run's latent.
// tc != null: the training sweep -- exact fp32 kernels, and every step also leaves its weight gradients in tc->grad.
int run_backward(glowk_handle* h, const float* x, const float* z, int N, float* dx, hipStream_t s, TrainCtx* tc) {
  const glowk_config& cfg = h->cfg;
  const int K = cfg.K, L = cfg.L, NF = cfg.F / 32;
  const int E = h->Hl * h->Wl * h->Cl;
  {
    const size_t total = (size_t)N * E;
    hipLaunchKernelGGL(k_prior_grad, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, z, total, E, h->d_loc, h->d_log_scale, h->bufGz);
    LAUNCHCHK("k_prior_grad");
  }
  float* gh_a = h->bufA;    // [g_va, g_yb] ping-pong
  float* gh_b = h->bufB;
  float* g_o = h->bufC;     // gradient wrt the network output
  float* Pg = h->bufP;      // per-tap partial input gradients
  float* gu = h->bufZ;      // block-level results (g_u of a block / g_y of the previous block's last step)
  const float* gy_src = nullptr;   // upstream gradient wrt the current block's output o (set per block)
  for (int lvl = L - 1; lvl >= 0; --lvl) {
    const Level& lv = h->levels[lvl];
    const int Q = N * lv.h * lv.w;
    const size_t blocks = mask_blocks(lv, (size_t)Q);
    int npg = 1;                    // partials of Pg the previous network launch of this level left in bufP
    // split training sweep: g_o (and with it everything linear in it: the backward network, its stored hiddens, the im2col of g_o,
    // the weight-gradient GEMMs) is carried times a power of two sized on the previous sweep's gradient magnitudes
    const float bfac = (tc && tc->split && !h->tr_bfac.empty()) ? h->tr_bfac[lvl] : 1.0f;
    // training sweep: per-step slots of g_o, g_v, M1 / M2 when the level's weight-gradient work runs as one batch after its sweep
    const bool level_batch = tc && h->trNB == K && K > 1;
    const size_t go_slot = level_batch ? (size_t)Q * lv.c : 0, m_slot = level_batch ? (size_t)cfg.F * Q : 0;
    const ptrdiff_t v_bs = K > 1 ? (ptrdiff_t)h->offV[(size_t)lvl * K] - (ptrdiff_t)h->offV[(size_t)lvl * K + 1] : 0;   // saved inputs: forward order
    // (1) + (2) of BwdArgs for a launch that merges the network gradient the level's previous launch left in Pg, then goes through step
    // ks's fused ActNorm + 1x1
    auto merged = [&](int ks) {
      BwdArgs ba = bwd_args(h, lv, N, bfac);
      ba.ghalf_in = gh_a; ba.Pg = Pg; ba.npg = npg; ba.pgstride = h->pstride; ba.A = lv.dev[ks].Afwd;
      return ba;
    };
    for (int k = 0; k < K; ++k) {   // reverse of the forward order K-1 .. 0
      const StepDev& sd = lv.dev[k];
      const size_t sidx = (size_t)lvl * K + (K - 1 - k);
      float* go_k = tc ? h->trGo + (size_t)k * go_slot : g_o;
      // gradient wrt the block output: the latent slice itself (last block) or what k_bwd_split assembled -- or merge step k-1's network
      // gradient and go through its fused ActNorm + 1x1; then this step's coupling
      BwdArgs ba = k > 0 ? merged(k - 1) : bwd_args(h, lv, N, bfac);
      if (k == 0 && lvl == L - 1) { ba.gv_direct = h->bufGz; ba.gvd_stride = h->Cl; ba.gvd_off = lv.z_off; }
      else if (k == 0)            { ba.gv_direct = gy_src;   ba.gvd_stride = lv.c; }
      ba.go_scale = bfac; ba.gmax = (tc && h->tr_gmax) ? h->tr_gmax + 16 * lvl : nullptr;
      ba.v = h->saveV + h->offV[sidx]; ba.osave = h->saveP + h->offP[sidx];
      ba.g_o = go_k; ba.ghalf_out = gh_b;
      if (tc && k > 0) ba.gv_out = h->trGv + (size_t)(k - 1) * go_slot;
      if (int rc = launch_bwd_light(lv.c, ba, s)) return rc;
      if (tc && k > 0 && !level_batch)   // g_v of step k-1 is complete: its ActNorm + 1x1 gradient sums
        if (int rc = train_affine_sums(h, lvl, k - 1, 1, h->saveV + h->offV[sidx + 1], 0, h->trGv, 0, N, s)) return rc;
      std::swap(gh_a, gh_b);   // gh_a now holds this step's [g_va, g_yb]
      NetArgs na = net_args(h, lv, sd, go_k, lv.c, 0, N);
      na.K1p = sd.K3bp; na.R0p = sd.RBp; na.P = Pg;
      na.mask1 = h->saveM + h->offM[sidx];
      na.mask2 = na.mask1 + blocks * NF * 64;
      const NetCall call = net_call(h, NET_BWD, tc != nullptr, sd.RHBp || sd.RSBp);   // (c = 32: 16x16x32 image only)
      if (call.arith != NET_EXACT) {
        na.RHp = sd.RHBp; na.RSp = sd.RSBp; na.eph = nullptr; na.sc1 = sd.scb1; na.sc2 = sd.scb2; na.sc3 = sd.scb3; na.xlim = sd.xlim_b;
        // the backward network is linear, so the kernels normalise every pixel's gradient vector to [T, 2T) (a power of two, exact;
        // glowk_kernels.h: pixel_norm): T = the largest power of two for which the host's worst-case bound (xlim_b: L1 norms of the
        // folded transposed weights) rules an fp16 overflow out.  Weights so large that even T = 2^-4 is not safe (the low bits of
        // the smaller components would go) are handled like a tripped guard: the call's range policy decides.
        na.bnorm = tc ? 1.0f : bwd_norm_target(sd.xlim_b);      // (training: one scale per launch instead, see bfac)
        if (na.bnorm == 0.0f) {
          na.bnorm = 1.0f;
          if (na.flag) HIPCHK(hipMemsetAsync(na.flag, 1, sizeof(int), s));
        }
      }
      if (na.xmax_out) na.xmax_out += (size_t)cfg.L * cfg.K;     // (range probe: the backward launches' half)
      if (tc) { na.st1 = h->trM2 + (size_t)k * m_slot; na.st2 = h->trM1 + (size_t)k * m_slot; }
      NetLaunch r;
      if (int rc = launch_net(h, lvl, lv.c, cfg.F, na, s, call, &r)) return rc;
      npg = r.np;
      if (tc && !level_batch) {
        // R1 / R2: kept by the saving forward pass, or recomputed now from the saved input (the P output of that launch goes to a
        // scratch partial of bufP)
        const float* R1 = h->trR1;
        if (h->trKeep && N <= h->trKeepN) R1 = h->trKeep + h->trKeepOff[sidx] * (size_t)N;   // (blocks are per tile: they scale with the batch)
        else {
          NetArgs nf = net_args(h, lv, sd, h->saveV + h->offV[sidx], lv.c, lv.c / 2, N);
          nf.P = h->bufP + 2 * h->pstride; nf.st1 = h->trR1; nf.st2 = h->trR1 + (size_t)cfg.F * Q;
          const NetCall rcall = net_call(h, NET_FWD, true);
          const NetLaunch rr = launch_net_raw(lv.c, cfg.F, nf, rcall, s);   // (exact fp32: a split sweep keeps its hiddens)
          if (rr.failed) return 1;
          if (h->net_tracing) trace_net(h, lvl, nf, rcall, rr);
        }
        if (int rc = train_network_grads(h, tc, lvl, k, 1, h->saveV + h->offV[sidx], 0, go_k, 0, R1, 0, h->trM1, h->trM2, 0, N, s, bfac)) return rc;
      }
    }
    // first forward step of the block (k = K-1): merge, then through its ActNorm + 1x1 -> g_u of the squeezed block input
    {
      BwdArgs ba = merged(K - 1);
      ba.gu_out = g_o;   // reuse g_o as g_u
      if (tc) ba.gv_out = h->trGv + (size_t)(K - 1) * go_slot;
      if (int rc = launch_bwd_light(lv.c, ba, s)) return rc;
      if (tc && !level_batch)
        if (int rc = train_affine_sums(h, lvl, K - 1, 1, h->saveV + h->offV[(size_t)lvl * K], 0, h->trGv, 0, N, s)) return rc;
    }
    if (level_batch) {
      // the level's sweep is over: weight gradients of its K steps in one batch of launches.  Step k (backward order) saved its input at
      // forward position K-1-k (v_bs < 0) and kept R1 / R2 there; M1 / M2, g_o, g_v sit in slot k.
      const float* v0 = h->saveV + h->offV[(size_t)lvl * K + (K - 1)];
      const float* R10 = h->trKeep + h->trKeepOff[(size_t)lvl * K + (K - 1)] * (size_t)N;
      const ptrdiff_t r_bs = -(ptrdiff_t)(2 * (size_t)cfg.F * Q);
      // (the ActNorm / 1x1 sums first: after the last level's the host has all it needs for its share of the step, which then runs beside
      //  this level's GEMMs -- glowk_param_grad)
      if (int rc = train_affine_sums(h, lvl, 0, K, v0, v_bs, h->trGv, (ptrdiff_t)go_slot, N, s)) return rc;
      if (lvl == 0 && tc->sums_ready) { HIPCHK(hipEventRecord(tc->sums_ready, s)); tc->sums_ready = nullptr; }
      if (int rc = train_network_grads(h, tc, lvl, 0, K, v0, v_bs, h->trGo, (ptrdiff_t)go_slot, R10, r_bs, h->trM1, h->trM2, (ptrdiff_t)m_slot, N, s, bfac)) return rc;
    }
    if (lvl > 0) {
      const Level& pv = h->levels[lvl - 1];
      CDISPATCH(pv.c, hipLaunchKernelGGL((k_bwd_split<CC>), dim3(N), dim3(256), 0, s, (const float*)h->bufGz, h->Hl * h->Wl, h->Cl, pv.z_off,
                                         pv.Cz, (const float*)g_o, pv.h, pv.w, gu));
      LAUNCHCHK("k_bwd_split");
      gy_src = gu;
    } else {
      CDISPATCH(lv.c, hipLaunchKernelGGL((k_bwd_in<CC>), dim3(N), dim3(256), 0, s, (const float*)g_o, x, lv.h, lv.w, pre_args(cfg), dx));
      LAUNCHCHK("k_bwd_in");
    }
  }
  if (tc && tc->sums_ready) { HIPCHK(hipEventRecord(tc->sums_ready, s)); tc->sums_ready = nullptr; }     // (step-by-step mode: the sums end the sweep)
  return 0;
}

// latent -> data
int run_inverse(glowk_handle* h, const float* z, int N, float* x, hipStream_t s) {
  const glowk_config& cfg = h->cfg;
  const int K = cfg.K, L = cfg.L;
  float* cur = h->bufA;
  float* oth = h->bufB;
  for (int lvl = L - 1; lvl >= 0; --lvl) {
    const Level& lv = h->levels[lvl];
    const float* unext = (lvl == L - 1) ? nullptr : cur;
    CDISPATCH(lv.c, hipLaunchKernelGGL((k_unsplit<CC>), dim3(N), dim3(256), 0, s, z, h->Hl * h->Wl, h->Cl, lv.z_off, lv.Cz, unext,
                                       lv.h, lv.w, oth));
    LAUNCHCHK("k_unsplit");
    std::swap(cur, oth);
    for (int k = 0; k < K; ++k) {   // Chain.inverse: step 0 first
      const StepDev& sd = lv.dev[k];
      CoupleArgs ca = couple_args(h, lv, sd, cur, N, 1, oth, lv.c);
      ca.A = sd.Ainv; ca.b = sd.binv;
      if (int rc = net_and_couple(h, lvl, lv.c, cfg.F, net_args(h, lv, sd, cur, lv.c, lv.c / 2, N), ca, N, s, net_call(h, NET_FWD))) return rc;
      std::swap(cur, oth);
    }
  }
  const Level& l0 = h->levels[0];
  CDISPATCH(l0.c, hipLaunchKernelGGL((k_out<CC>), dim3(N), dim3(256), 0, s, cur, l0.h, l0.w, pre_args(cfg), 1, x));
  LAUNCHCHK("k_out");
  return 0;
}

// log_prob (or the log-det alone) from the latent and the accumulated log-det: the prior kernel, for callers outside this unit
int launch_prior(glowk_handle* h, const float* z, int N, float* logp_dev, hipStream_t s) {
  hipLaunchKernelGGL(k_prior, dim3(N), dim3(256), 0, s, z, h->Hl * h->Wl * h->Cl, h->d_loc, h->d_log_scale, (const double*)h->bufLd, logp_dev, (float*)nullptr);
  LAUNCHCHK("k_prior");
  return 0;
}

// device that owns a device pointer (the handle-free entry points launch there); the current device if HIP cannot tell
int ptr_device(const void* p) {
  hipPointerAttribute_t a;
  int cur = 0;
  (void)hipGetDevice(&cur);
  if (hipPointerGetAttributes(&a, p) == hipSuccess && a.device >= 0) return a.device;
  (void)hipGetLastError();
  return cur;
}

// The range guard around one compute call (include/glowk.h: glowk_range_policy).  `run` issues the call's launches.
template <class Run>
int guarded(glowk_handle* h, hipStream_t s, Run&& run) {
  if (int rc = run()) return rc;
  if (h->precision == GLOWK_PREC_F32 || h->range_policy == GLOWK_RANGE_IGNORE) return 0;
  HIPCHK(hipMemcpyAsync(h->h_flag, h->d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (!h->h_flag[0]) return 0;
  h->h_flag[0] = 0;
  HIPCHK(hipMemsetAsync(h->d_flag, 0, sizeof(int), s));
  if (h->range_policy == GLOWK_RANGE_ERROR) {
    g_err = "a hidden activation left the fp16 range of the split arithmetic (|a| >= 16 376) or the input is not finite: "
            "the outputs of this call are not usable -- use GLOWK_PREC_F32 or GLOWK_RANGE_FALLBACK";
    return GLOWK_ERR_RANGE;
  }
  const int prec = h->precision;   // FALLBACK: the same call on the exact kernels, in-process
  h->precision = GLOWK_PREC_F32;
  ++h->range_fallbacks;
  const int rc = run();
  h->precision = prec;
  return rc;
}

}  // namespace glowk_eng

// =================================================================================================
// =================================================================================================
extern "C" {

int glowk_version(void) { return GLOWK_VERSION; }
void glowk_reload_env(void) { glowk_detail::reload_env(); }
const char* glowk_last_error(void) { return g_err.c_str(); }

int glowk_create(const glowk_config* cfg, int device, glowk_handle** out) {
  if (!cfg || !out) return fail("null argument");
  if (cfg->L < 2 || cfg->L > 4) return fail("L should be 2, 3 or 4");  // flow_builder.py:76-77
  const int s = 1 << cfg->L;
  if (cfg->H <= 0 || cfg->W <= 0 || cfg->C <= 0 || cfg->H % s || cfg->W % s) return fail("H and W must be positive multiples of 2^L");
  if (cfg->K <= 0) return fail("K must be positive");
  if (cfg->F != 128 && cfg->F != 256 && cfg->F != 384 && cfg->F != 512) return fail("n_filters must be 128, 256, 384 or 512 (the instantiated coupling-network widths)");
  glowk_handle* h = new glowk_handle();
  h->cfg = *cfg;
  h->device = device;
  h->Hl = cfg->H / s; h->Wl = cfg->W / s; h->Cl = cfg->C * s * s;
  int hh = cfg->H, ww = cfg->W, cc = cfg->C, off = 0, rem = h->Cl;
  for (int l = 0; l < cfg->L; ++l) {
    Level lv;
    hh /= 2; ww /= 2; cc *= 4;
    lv.h = hh; lv.w = ww; lv.c = cc;
    if (l < cfg->L - 1) {
      lv.z_width = rem / 2; lv.z_off = off; off += lv.z_width; rem -= lv.z_width;
      lv.Cz = (hh * ww * (cc / 2)) / (h->Hl * h->Wl);
    } else {
      lv.z_width = rem; lv.z_off = off; lv.Cz = 0;
    }
    for (int t = 0; t < GLOWK_NUM_STEP_TENSORS; ++t) {
      lv.host[t].resize(cfg->K);
      for (int k = 0; k < cfg->K; ++k) lv.host[t][k].assign(step_tensor_size(*cfg, lv, t), 0.0f);
    }
    lv.dev.resize(cfg->K);
    h->levels.push_back(std::move(lv));
    cc /= 2;
  }
  const size_t E = (size_t)h->Hl * h->Wl * h->Cl;
  h->prior_loc.assign(E, 0.0f);
  h->prior_log_scale.assign(E, 0.0f);
  *out = h;
  return 0;
}

int glowk_destroy(glowk_handle* h) {
  if (!h) return 0;
  DeviceGuard dg(h->device);
  // work still queued on the handle's buffers, streams or pinned staging ends before the owners release them (one synchronise, not a member order)
  (void)hipDeviceSynchronize();
  delete h;
  return 0;
}

size_t glowk_tensor_size(const glowk_handle* h, int level, int tensor_id) {
  if (!h) return 0;
  if (tensor_id == GLOWK_PRIOR_LOC || tensor_id == GLOWK_PRIOR_LOG_SCALE) return h->prior_loc.size();
  if (level < 0 || level >= (int)h->levels.size() || tensor_id < 0 || tensor_id >= GLOWK_NUM_STEP_TENSORS) return 0;
  return step_tensor_size(h->cfg, h->levels[level], tensor_id);
}

static std::vector<float>* locate(glowk_handle* h, int level, int step, int id) {
  if (id == GLOWK_PRIOR_LOC) return &h->prior_loc;
  if (id == GLOWK_PRIOR_LOG_SCALE) return &h->prior_log_scale;
  if (level < 0 || level >= (int)h->levels.size() || id < 0 || id >= GLOWK_NUM_STEP_TENSORS) return nullptr;
  if (step < 0 || step >= h->cfg.K) return nullptr;
  return &h->levels[level].host[id][step];
}

int glowk_set_tensor(glowk_handle* h, int level, int step, int tensor_id, const float* host, size_t n) {
  if (!h || !host) return fail("null argument");
  if (h->host_stale) { DeviceGuard dg(h->device); if (int rc = sync_host(h)) return rc; }
  h->tr_active = false;      // the device master copy of a training run no longer holds the current parameters
  std::vector<float>* v = locate(h, level, step, tensor_id);
  if (!v) return fail("no such tensor");
  if (v->size() != n) return fail("tensor size mismatch: expected " + std::to_string(v->size()) + ", got " + std::to_string(n));
  std::memcpy(v->data(), host, n * sizeof(float));
  h->finalized = false;
  return 0;
}

int glowk_get_tensor(const glowk_handle* h, int level, int step, int tensor_id, float* host, size_t n) {
  if (!h || !host) return fail("null argument");
  if (h->host_stale) { DeviceGuard dg(h->device); if (int rc = sync_host(const_cast<glowk_handle*>(h))) return rc; }
  const std::vector<float>* v = locate(const_cast<glowk_handle*>(h), level, step, tensor_id);
  if (!v) return fail("no such tensor");
  if (v->size() != n) return fail("tensor size mismatch");
  std::memcpy(host, v->data(), n * sizeof(float));
  if (tensor_id == GLOWK_INV1X1_P_INV) {   // never loaded: what the reference initialises it to, inv(P)
    bool set = false;
    for (size_t i = 0; i < n; ++i) set |= host[i] != 0.0f;
    if (!set) {
      const int c = h->levels[level].c;
      const std::vector<float>& P = h->levels[level].host[GLOWK_INV1X1_P][step];
      Mat Pm(P.begin(), P.end()), Pi;
      if (invert(Pm, c, Pi))
        for (size_t i = 0; i < n; ++i) host[i] = (float)Pi[i];
    }
  }
  return 0;
}

int glowk_finalize_weights(glowk_handle* h) {
  if (!h) return fail("null handle");
  if (h->host_stale) { DeviceGuard dg0(h->device); if (int rc = sync_host(h)) return rc; }
  const glowk_config& cfg = h->cfg;
  for (const Level& lv : h->levels)
    if (lv.c != 4 && lv.c != 8 && lv.c != 16 && lv.c != 32)
      return fail("unsupported channel count " + std::to_string(lv.c) + " (this build: 4, 8, 16, 32)");
  size_t total = 0;
  for (const Level& lv : h->levels) total += step_layout(lv.c, cfg.F).total * cfg.K;
  const size_t E = h->prior_loc.size();
  const size_t prior_off = total;
  total += 2 * pad4(E);
  std::vector<float> stage(total, 0.0f);
  // every step packs into its own block of the staging arena: steps are packed by a few host threads
  std::vector<PackJob> jobs;
  std::vector<size_t> offs;
  {
    size_t o = 0;
    for (size_t l = 0; l < h->levels.size(); ++l)
      for (int k = 0; k < cfg.K; ++k) {
        jobs.push_back(PackJob{l, k, o, 0.0, {1, 1, 1, 1, 1, 1, 0, 0}, std::string(), false});
        offs.push_back(o);
        o += step_layout(h->levels[l].c, cfg.F).total;
      }
  }
  {
    unsigned nthr = std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) nthr = std::min<unsigned>(nthr ? nthr : 1, (unsigned)CPU_COUNT(&set));
    pack_all_steps(cfg, h->levels, stage.data(), jobs, std::min<unsigned>(nthr, 16u));
  }
  for (const PackJob& jb : jobs)    // (a packer error leaves the handle as it was: the images it has, split_stale, finalized)
    if (!jb.ok) return fail("level " + std::to_string(jb.l) + " step " + std::to_string(jb.k) + ": " + jb.err);
  h->finalized = false;             // from here until the new images and step pointers are in place
  h->ld_step.assign((size_t)cfg.L * cfg.K, 0.0);
  h->ld_const = 0.0;
  for (const PackJob& jb : jobs) {
    StepDev& d = h->levels[jb.l].dev[jb.k];
    h->ld_step[jb.l * cfg.K + jb.k] = jb.ldc;
    d.sc1 = jb.sc[0]; d.sc2 = jb.sc[1]; d.sc3 = jb.sc[2];
    d.scb1 = jb.sc[3]; d.scb2 = jb.sc[4]; d.scb3 = jb.sc[5];
    d.xlim_f = jb.sc[6]; d.xlim_b = jb.sc[7];
    h->ld_const += jb.ldc;
  }
  std::memcpy(stage.data() + prior_off, h->prior_loc.data(), E * 4);
  std::memcpy(stage.data() + prior_off + pad4(E), h->prior_log_scale.data(), E * 4);
  // data-independent preprocessing log-det (flow_tfp_bijectors.py:390-396)
  const double npx = (double)cfg.H * cfg.W * cfg.C;
  h->ld_pre_const = -npx * std::log((double)cfg.maxval - (double)cfg.minval);
  if (cfg.use_logit) h->ld_pre_const += npx * std::log(1.0 - 2.0 * (double)cfg.alpha);

  DeviceGuard dg(h->device);
  HIPCHK(hipDeviceSynchronize());
  h->arena.reset();
  HIPCHK(dev_alloc(h->arena, total * 4));
  HIPCHK(hipMemcpy(h->arena, stage.data(), total * 4, hipMemcpyHostToDevice));
  size_t idx = 0;
  for (Level& lv : h->levels) {
    const StepLayout SL = step_layout(lv.c, cfg.F);
    for (int k = 0; k < cfg.K; ++k) {
      StepDev& d = lv.dev[k];
      d.arena_off = offs[idx];
      const float* base = h->arena + offs[idx++];
      d.K1p = base + SL.K1p; d.ep = base + SL.ep;
      d.R0p = reinterpret_cast<const float4*>(base + SL.R0p);
      d.RHp = SL.slotH ? reinterpret_cast<const float4*>(base + SL.RHp) : nullptr;
      d.epH = (SL.slotH || SL.slotS) ? base + SL.epH : nullptr;
      d.RSp = SL.slotS ? reinterpret_cast<const float4*>(base + SL.RSp) : nullptr;
      d.RSBp = SL.slotSB ? reinterpret_cast<const float4*>(base + SL.RSBp) : nullptr;
      d.RHBp = SL.slotHB ? reinterpret_cast<const float4*>(base + SL.RHBp) : nullptr;
      d.K3bp = base + SL.K3bp;
      d.RBp = reinterpret_cast<const float4*>(base + SL.RBp);
      d.Afwd = base + SL.Afwd; d.bfwd = base + SL.bfwd; d.Ainv = base + SL.Ainv; d.binv = base + SL.binv; d.b3 = base + SL.b3;
    }
  }
  h->d_loc = cfg.learntop ? h->arena + prior_off : nullptr;
  h->d_log_scale = cfg.learntop ? h->arena + prior_off + pad4(E) : nullptr;
  h->finalized = true;
  h->split_stale = false;
  return 0;
}

namespace glowk_eng {
constexpr int STAT_BLOCKS = 256;

// one flow step on a materialised tensor: u (cur) -> ActNorm+1x1 -> tmp; network; coupling -> cur
int run_step_inplace(glowk_handle* h, int lvl, int k, float* cur, float* tmp, int Nl, hipStream_t s) {
  const Level& lv = h->levels[lvl];
  const StepDev& sd = lv.dev[k];
  const int Q = Nl * lv.h * lv.w;
  CDISPATCH(lv.c, hipLaunchKernelGGL((k_affine<CC>), dim3((Q + 255) / 256), dim3(256), 0, s, (const float*)cur, Q, sd.Afwd, sd.bfwd, tmp));
  LAUNCHCHK("k_affine");
  NetArgs na = net_args(h, lv, sd, tmp, lv.c, lv.c / 2, Nl);
  if (int rc = launch_net(h, lvl, lv.c, h->cfg.F, na, s, NetCall{NET_FWD, NET_EXACT})) return rc;
  CoupleArgs ca = couple_args(h, lv, sd, tmp, Nl, 0, cur, lv.c);
  ca.P = h->bufP;       // (the exact kernel: one partial)
  ca.flag = nullptr;
  return launch_couple(lv.c, ca, Nl, s);
}

// re-fold ActNorm+1x1 of one step after its ActNorm tensors changed and upload the small affine block
int refresh_step_affine(glowk_handle* h, int lvl, int k, hipStream_t s) {
  Level& lv = h->levels[lvl];
  const StepLayout SL = step_layout(lv.c, h->cfg.F);
  std::vector<float> tmp(SL.total - SL.Afwd + SL.Afwd, 0.0f);   // pack_affine indexes from the block start
  std::string err;
  double ldc = 0;
  if (!pack_affine(h->cfg, lv, k, tmp.data(), &ldc, &err)) return fail(err);
  h->ld_step[(size_t)lvl * h->cfg.K + k] = ldc;
  HIPCHK(hipMemcpyAsync(h->arena + lv.dev[k].arena_off + SL.Afwd, tmp.data() + SL.Afwd, (SL.total - SL.Afwd) * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}
}  // namespace glowk_eng

int glowk_actnorm_data_init(glowk_handle* h, const float* x_dev, int N, int runtime_order, int raw_minibatch_quirk, void* stream) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (int rc = check_ready(h, N)) return rc;
  if (!x_dev) return fail("null tensor");
  hipStream_t s = (hipStream_t)stream;
  const glowk_config& cfg = h->cfg;
  const int K = cfg.K, L = cfg.L;
  const size_t E = (size_t)cfg.H * cfg.W * cfg.C;
  if (int rc = ensure_c(h, N)) return rc;
  if (h->host_stale) if (int rc = sync_host(h)) return rc;
  h->tr_active = false;
  if (!h->bufStat) HIPCHK(dev_alloc(h->bufStat, (size_t)(STAT_BLOCKS + 1) * 32 * 8));
  // y = SpecPreprocessing.forward(minibatch) (flow_builder.py:121), kept in bufZ
  hipLaunchKernelGGL(k_pre_only, dim3(N), dim3(256), 0, s, x_dev, (int)E, pre_args(cfg), 0, h->bufZ, (float*)nullptr, 0.0);
  LAUNCHCHK("k_pre_only");
  PreArgs nopre = {0, 1, 0, 0};
  float* blk_in = h->bufC;      // input of the current block (squeezed), kept for the block forward
  float* cur = h->bufA;
  float* tmp = h->bufB;
  const bool quirk = raw_minibatch_quirk && L > 2;
  std::vector<double> part((size_t)STAT_BLOCKS * 32), mean(32), var(32);
  for (int lvl = 0; lvl < L; ++lvl) {
    Level& lv = h->levels[lvl];
    int Nl = N;
    if (lvl == 0) {
      CDISPATCH(lv.c, hipLaunchKernelGGL((k_in<CC>), dim3(N), dim3(256), 0, s, (const float*)h->bufZ, cfg.H, cfg.W, nopre, 0,
                                         (const float*)nullptr, (const float*)nullptr, blk_in, (double*)nullptr, 0.0));
      LAUNCHCHK("k_in");
    } else if (quirk) {
      // Squeeze([2h,2w,c/4]).forward(raw minibatch): reshape(-1, ...) reinterprets it as more, smaller samples
      Nl = (int)((size_t)N * E / ((size_t)lv.h * lv.w * lv.c));
      CDISPATCH(lv.c, hipLaunchKernelGGL((k_in<CC>), dim3(Nl), dim3(256), 0, s, (const float*)h->bufZ, 2 * lv.h, 2 * lv.w, nopre, 0,
                                         (const float*)nullptr, (const float*)nullptr, blk_in, (double*)nullptr, 0.0));
      LAUNCHCHK("k_in");
    } else {
      // second half of the previous block's output (held in cur), squeezed (flow_glow.py:96-97)
      const Level& pv = h->levels[lvl - 1];
      CDISPATCH(pv.c, hipLaunchKernelGGL((k_split<CC>), dim3(N), dim3(256), 0, s, (const float*)cur, pv.h, pv.w, (float*)nullptr, 0, 0, 0, 1,
                                         (const float*)nullptr, (const float*)nullptr, blk_in));
      LAUNCHCHK("k_split");
    }
    const int Q = Nl * lv.h * lv.w;
    HIPCHK(hipMemcpyAsync(cur, blk_in, (size_t)Q * lv.c * 4, hipMemcpyDeviceToDevice, s));
    for (int idx = 0; idx < K; ++idx) {
      const int k = runtime_order ? K - 1 - idx : idx;
      double* d_part = h->bufStat;
      double* d_mean = h->bufStat + (size_t)STAT_BLOCKS * 32;
      for (int pass = 0; pass < 2; ++pass) {
        CDISPATCH(lv.c, hipLaunchKernelGGL((k_chan_stats<CC>), dim3(STAT_BLOCKS), dim3(256), 0, s, (const float*)cur, Q,
                                           pass ? (const double*)d_mean : (const double*)nullptr, d_part));
        LAUNCHCHK("k_chan_stats");
        HIPCHK(hipMemcpyAsync(part.data(), d_part, (size_t)STAT_BLOCKS * lv.c * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int c = 0; c < lv.c; ++c) {
          double t = 0;
          for (int b = 0; b < STAT_BLOCKS; ++b) t += part[(size_t)b * lv.c + c];
          (pass ? var : mean)[c] = t / Q;
        }
        if (!pass) HIPCHK(hipMemcpyAsync(d_mean, mean.data(), lv.c * 8, hipMemcpyHostToDevice, s));
      }
      for (int c = 0; c < lv.c; ++c) {
        // std_init = reduce_std + 1e-8 (the reference adds it in fp32); scale = 1/std; shift = -mean/std
        const double sd_ = (double)((float)std::sqrt(var[c]) + 1e-8f);
        lv.host[GLOWK_ACTNORM_LOG_SCALE][k][c] = (float)std::log(1.0 / sd_);
        lv.host[GLOWK_ACTNORM_SHIFT][k][c] = (float)(-mean[c] / sd_);
      }
      if (int rc = refresh_step_affine(h, lvl, k, s)) return rc;
      if (int rc = run_step_inplace(h, lvl, k, cur, tmp, Nl, s)) return rc;   // minibatch_updated = step.forward(...)
    }
    if (lvl < L - 1 && !quirk && !runtime_order) {
      // glow_block.forward(minibatch): the block as tfb.Chain applies it (K-1 .. 0) on the block's own input
      HIPCHK(hipMemcpyAsync(cur, blk_in, (size_t)Q * lv.c * 4, hipMemcpyDeviceToDevice, s));
      for (int k = K - 1; k >= 0; --k)
        if (int rc = run_step_inplace(h, lvl, k, cur, tmp, Nl, s)) return rc;
    }
  }
  h->ld_const = 0.0;
  for (double v : h->ld_step) h->ld_const += v;
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

int glowk_set_precision(glowk_handle* h, int precision) {
  if (!h) return fail("null handle");
  if (precision != GLOWK_PREC_F32 && precision != GLOWK_PREC_F16X3 && precision != GLOWK_PREC_F16X2) return fail("unknown precision mode");
  h->precision = precision;
  return 0;
}

int glowk_get_precision(const glowk_handle* h) { return h ? h->precision : -1; }

int glowk_set_range_policy(glowk_handle* h, int policy) {
  if (!h) return fail("null handle");
  if (policy != GLOWK_RANGE_IGNORE && policy != GLOWK_RANGE_ERROR && policy != GLOWK_RANGE_FALLBACK) return fail("unknown range policy");
  h->range_policy = policy;
  return 0;
}

int glowk_get_range_policy(const glowk_handle* h) { return h ? h->range_policy : -1; }

int glowk_range_status(glowk_handle* h, int* tripped, int64_t* fallbacks, void* stream) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (fallbacks) *fallbacks = h->range_fallbacks;
  if (tripped) {
    *tripped = 0;
    if (h->d_flag) {
      hipStream_t s = (hipStream_t)stream;
      HIPCHK(hipMemcpyAsync(h->h_flag, h->d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (h->h_flag[0]) {
        *tripped = 1;
        h->h_flag[0] = 0;
        HIPCHK(hipMemsetAsync(h->d_flag, 0, sizeof(int), s));
      }
    }
  }
  return 0;
}

int glowk_range_probe_begin(glowk_handle* h) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  const size_t n = (size_t)2 * h->cfg.L * h->cfg.K;
  if (!h->d_probe) HIPCHK(dev_alloc(h->d_probe, n * sizeof(unsigned)));
  HIPCHK(hipMemset(h->d_probe, 0, n * sizeof(unsigned)));
  return 0;
}

int glowk_range_probe_end(glowk_handle* h, float* fwd_ratio, float* bwd_ratio, void* stream) {
  if (!h) return fail("null handle");
  if (!h->d_probe) return fail("glowk_range_probe_end without glowk_range_probe_begin");
  DeviceGuard dg(h->device);
  const int LK = h->cfg.L * h->cfg.K;
  std::vector<float> v((size_t)2 * LK);
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  HIPCHK(hipMemcpy(v.data(), h->d_probe, v.size() * sizeof(float), hipMemcpyDeviceToHost));
  h->d_probe.reset();
  float rf = 0.f, rb = 0.f;
  for (int l = 0; l < h->cfg.L; ++l)
    for (int k = 0; k < h->cfg.K; ++k) {
      const StepDev& sd = h->levels[l].dev[k];
      const int i = l * h->cfg.K + k;
      if (sd.xlim_f > 0.f) rf = std::max(rf, v[i] / sd.xlim_f);
      // (the backward kernels normalise their inputs per pixel: what can fail is the STATIC requirement 2 * 2^-4 <= xlim_b;
      //  reported as that ratio -- the recorded gradient magnitudes v[LK + i] no longer matter for the range)
      if (sd.xlim_b > 0.f && v[LK + i] > 0.f) rb = std::max(rb, 0.125f / sd.xlim_b);
    }
  if (fwd_ratio) *fwd_ratio = rf;
  if (bwd_ratio) *bwd_ratio = rb;
  return 0;
}

size_t glowk_workspace_bytes(const glowk_handle* h, int N, int with_grad) {
  if (!h || N <= 0) return 0;
  size_t b = ws_sizes(h, (size_t)N).total() + 16 /* range flag */;
  if (with_grad) b += save_sizes(h, (size_t)N).total();
  return b;
}

int glowk_max_tiles(const glowk_handle* h) { return h ? max_tiles(h) : 0; }

int glowk_reserve(glowk_handle* h, int N, int with_grad) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (int rc = check_batch(h, N)) return rc;
  if (int rc = ensure_ws(h, N)) return rc;
  if (with_grad) {
    if (!h->finalized) return fail("glowk_finalize_weights must run before reserving the gradient path (its size depends on the launch policy)");
    return ensure_save(h, N);
  }
  return 0;
}

int glowk_forward(glowk_handle* h, const float* x_dev, int N, float* z_dev, float* logdet_dev, void* stream) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (int rc = check_ready(h, N)) return rc;
  if (!x_dev || !z_dev) return fail("null tensor");
  hipStream_t s = (hipStream_t)stream;
  return guarded(h, s, [&]() -> int {
    if (int rc = run_forward(h, x_dev, N, z_dev, s)) return rc;
    if (logdet_dev) {
      hipLaunchKernelGGL(k_prior, dim3(N), dim3(256), 0, s, (const float*)nullptr, 0, (const float*)nullptr, (const float*)nullptr,
                         (const double*)h->bufLd, (float*)nullptr, logdet_dev);
      LAUNCHCHK("k_prior(logdet)");
    }
    return 0;
  });
}

int glowk_inverse(glowk_handle* h, const float* z_dev, int N, float* x_dev, void* stream) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (int rc = check_ready(h, N)) return rc;
  if (!x_dev || !z_dev) return fail("null tensor");
  hipStream_t s = (hipStream_t)stream;
  return guarded(h, s, [&]() -> int { return run_inverse(h, z_dev, N, x_dev, s); });
}

int glowk_log_prob(glowk_handle* h, const float* x_dev, int N, float* logp_dev, float* z_dev, void* stream) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (int rc = check_ready(h, N)) return rc;
  if (!x_dev || !logp_dev) return fail("null tensor");
  hipStream_t s = (hipStream_t)stream;
  float* z = z_dev ? z_dev : h->bufZ;
  return guarded(h, s, [&]() -> int {
    if (int rc = run_forward(h, x_dev, N, z, s)) return rc;
    hipLaunchKernelGGL(k_prior, dim3(N), dim3(256), 0, s, (const float*)z, h->Hl * h->Wl * h->Cl, h->d_loc, h->d_log_scale,
                       (const double*)h->bufLd, logp_dev, (float*)nullptr);
    LAUNCHCHK("k_prior");
    return 0;
  });
}

int glowk_log_prob_sum(glowk_handle* h, const float* x_dev, int N, float* logp_dev, float* z_dev, double* sum_dev, int accumulate, void* stream) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (int rc = check_ready(h, N)) return rc;
  if (!x_dev || !logp_dev || !sum_dev) return fail("null tensor");
  hipStream_t s = (hipStream_t)stream;
  float* z = z_dev ? z_dev : h->bufZ;
  // The reduction runs AFTER the range guard has accepted the call (round-3 advisor): inside the guarded lambda a tripped call's
  // rejected partial sum would already sit in *sum_dev when the fp32 re-run of the FALLBACK policy adds its own (accumulate != 0:
  // double-counted or NaN), and under the ERROR policy *sum_dev would be left modified by a call that reports failure.
  const int rc = guarded(h, s, [&]() -> int {
    if (int rc = run_forward(h, x_dev, N, z, s)) return rc;
    hipLaunchKernelGGL(k_prior, dim3(N), dim3(256), 0, s, (const float*)z, h->Hl * h->Wl * h->Cl, h->d_loc, h->d_log_scale,
                       (const double*)h->bufLd, logp_dev, (float*)nullptr);
    LAUNCHCHK("k_prior");
    return 0;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(k_sum_f64, dim3(1), dim3(1024), 0, s, (const float*)logp_dev, (size_t)N, sum_dev, accumulate, 1.0);
  LAUNCHCHK("k_sum_f64");
  return 0;
}

int glowk_sum_f64(const float* v_dev, size_t n, double* out_dev, int accumulate, double scale, void* stream) {
  if (!out_dev || (!v_dev && n)) return fail("null tensor");
  DeviceGuard dg(ptr_device(out_dev));
  hipLaunchKernelGGL(k_sum_f64, dim3(1), dim3(1024), 0, (hipStream_t)stream, v_dev, n, out_dev, accumulate, scale);
  LAUNCHCHK("k_sum_f64");
  return 0;
}

int glowk_log_prob_grad(glowk_handle* h, const float* x_dev, int N, float* logp_dev, float* dx_dev, void* stream) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (int rc = check_ready(h, N)) return rc;
  if (!x_dev || !logp_dev || !dx_dev) return fail("null tensor");
  if (int rc = ensure_save(h, N)) return rc;
  hipStream_t s = (hipStream_t)stream;
  float* z = h->bufGz;   // the latent lives in bufGz until the prior gradient overwrites it in place
  return guarded(h, s, [&]() -> int {
    if (int rc = run_forward(h, x_dev, N, z, s, true)) return rc;
    hipLaunchKernelGGL(k_prior, dim3(N), dim3(256), 0, s, (const float*)z, h->Hl * h->Wl * h->Cl, h->d_loc, h->d_log_scale,
                       (const double*)h->bufLd, logp_dev, (float*)nullptr);
    LAUNCHCHK("k_prior");
    return run_backward(h, x_dev, z, N, dx_dev, s);
  });
}

int glowk_sample(glowk_handle* h, const float* eps_dev, int N, float* x_dev, void* stream) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (int rc = check_ready(h, N)) return rc;
  if (!eps_dev || !x_dev) return fail("null tensor");
  hipStream_t s = (hipStream_t)stream;
  const int E = h->Hl * h->Wl * h->Cl;
  const size_t total = (size_t)N * E;
  return guarded(h, s, [&]() -> int {
    hipLaunchKernelGGL(k_prior_sample, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, eps_dev, total, E, h->d_loc, h->d_log_scale,
                       h->bufZ);
    LAUNCHCHK("k_prior_sample");
    return run_inverse(h, h->bufZ, N, x_dev, s);
  });
}

int glowk_prior_log_prob(glowk_handle* h, const float* z_dev, int N, float* logp_dev, void* stream) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (int rc = check_ready(h, N)) return rc;
  if (!z_dev || !logp_dev) return fail("null tensor");
  hipLaunchKernelGGL(k_prior, dim3(N), dim3(256), 0, (hipStream_t)stream, z_dev, h->Hl * h->Wl * h->Cl, h->d_loc, h->d_log_scale,
                     (const double*)nullptr, logp_dev, (float*)nullptr);
  LAUNCHCHK("k_prior");
  return 0;
}

int64_t glowk_fused_steps(const glowk_handle* h) { return h ? h->fused_steps : -1; }

int glowk_kernel_families(const glowk_handle* h, int64_t* out7) {
  if (!h || !out7) return fail("null argument");
  for (int i = 0; i < FAM_COUNT; ++i) out7[i] = h->family_launches[i];
  return 0;
}

int glowk_profile_begin(glowk_handle* h) {
  if (!h) return fail("null handle");
  h->profiling = true;
  h->ev_used = 0;
  h->ev_level.clear();
  return 0;
}

int glowk_profile_end(glowk_handle* h, glowk_profile* out) {
  if (!h || !out) return fail("null argument");
  std::memset(out, 0, sizeof(*out));
  h->profiling = false;
  DeviceGuard dg(h->device);
  HIPCHK(hipDeviceSynchronize());
  for (size_t i = 0; i < h->ev_level.size(); ++i) {
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, h->ev_pool[2 * i], h->ev_pool[2 * i + 1]));
    const int l = h->ev_level[i];
    if (l >= 0 && l < 4) { out->net_ms[l] += ms; out->net_launches[l] += 1; }
  }
  h->ev_used = 0;
  h->ev_level.clear();
  return 0;
}

int glowk_net_trace_begin(glowk_handle* h) {
  if (!h) return fail("null handle");
  h->net_trace.clear();
  h->net_tracing = true;
  return 0;
}

int glowk_net_trace_end(glowk_handle* h, glowk_net_record* out, int cap, int* count) {
  if (!h || !count || cap < 0 || (cap > 0 && !out)) return fail("bad argument");
  h->net_tracing = false;
  const size_t n = h->net_trace.size();
  if (n > (size_t)INT32_MAX) return fail("more launches traced than the count can hold");
  for (size_t i = 0; i < n && i < (size_t)cap; ++i) out[i] = h->net_trace[i];
  *count = (int)n;
  if (n <= (size_t)cap) std::vector<glowk_net_record>().swap(h->net_trace);   // (a caller whose buffer was too small asks again)
  return 0;
}

int glowk_squeeze(const float* x_dev, int N, int H, int W, int C, float* y_dev, void* stream) {
  if (!x_dev || !y_dev) return fail("null tensor");
  if (N <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2) return fail("squeeze needs even H and W");  // flow_tfp_bijectors.py:165-166
  if ((long long)N * H * W * C > (1LL << 28)) return fail("squeeze: more than 2^28 elements in one call; split the batch");
  DeviceGuard dg(ptr_device(x_dev));
  PreArgs p = {0, 1, 0, 0};
  const int c = 4 * C;
  CDISPATCH(c, hipLaunchKernelGGL((k_in<CC>), dim3(N), dim3(256), 0, (hipStream_t)stream, x_dev, H, W, p, 0, (const float*)nullptr,
                                  (const float*)nullptr, y_dev, (double*)nullptr, 0.0));
  LAUNCHCHK("k_in(squeeze)");
  return 0;
}

int glowk_unsqueeze(const float* y_dev, int N, int hh, int ww, int c4, float* x_dev, void* stream) {
  if (!x_dev || !y_dev) return fail("null tensor");
  if (N <= 0 || hh <= 0 || ww <= 0 || c4 % 4) return fail("unsqueeze needs a channel count divisible by 4");
  if ((long long)N * hh * ww * c4 > (1LL << 28)) return fail("unsqueeze: more than 2^28 elements in one call; split the batch");
  DeviceGuard dg(ptr_device(y_dev));
  PreArgs p = {0, 1, 0, 0};
  CDISPATCH(c4, hipLaunchKernelGGL((k_out<CC>), dim3(N), dim3(256), 0, (hipStream_t)stream, y_dev, hh, ww, p, 0, x_dev));
  LAUNCHCHK("k_out(unsqueeze)");
  return 0;
}

int glowk_preprocess_forward(glowk_handle* h, const float* x_dev, int N, float* y_dev, float* logdet_dev, void* stream) {
  if (!h || !x_dev || !y_dev) return fail("null argument");
  DeviceGuard dg(h->device);
  if (int rc = check_batch(h, N)) return rc;
  const int E = h->cfg.H * h->cfg.W * h->cfg.C;
  double ldc = -(double)E * std::log((double)h->cfg.maxval - (double)h->cfg.minval);
  if (h->cfg.use_logit) ldc += (double)E * std::log(1.0 - 2.0 * (double)h->cfg.alpha);
  hipLaunchKernelGGL(k_pre_only, dim3(N), dim3(256), 0, (hipStream_t)stream, x_dev, E, pre_args(h->cfg), 0, y_dev, logdet_dev, ldc);
  LAUNCHCHK("k_pre_only");
  return 0;
}

int glowk_preprocess_inverse(glowk_handle* h, const float* y_dev, int N, float* x_dev, void* stream) {
  if (!h || !x_dev || !y_dev) return fail("null argument");
  DeviceGuard dg(h->device);
  if (int rc = check_batch(h, N)) return rc;
  const int E = h->cfg.H * h->cfg.W * h->cfg.C;
  hipLaunchKernelGGL(k_pre_only, dim3(N), dim3(256), 0, (hipStream_t)stream, y_dev, E, pre_args(h->cfg), 1, x_dev, (float*)nullptr, 0.0);
  LAUNCHCHK("k_pre_only");
  return 0;
}

int glowk_step_forward(glowk_handle* h, int level, int step, const float* u_dev, int N, float* y_dev, float* logdet_dev, void* stream) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (int rc = check_ready(h, N)) return rc;
  if (level < 0 || level >= h->cfg.L || step < 0 || step >= h->cfg.K) return fail("no such step");
  if (!u_dev || !y_dev) return fail("null tensor");
  hipStream_t s = (hipStream_t)stream;
  const Level& lv = h->levels[level];
  const StepDev& sd = lv.dev[step];
  const int Q = N * lv.h * lv.w;
  return guarded(h, s, [&]() -> int {
    CDISPATCH(lv.c, hipLaunchKernelGGL((k_affine<CC>), dim3((Q + 255) / 256), dim3(256), 0, s, u_dev, Q, sd.Afwd, sd.bfwd, h->bufA));
    LAUNCHCHK("k_affine");
    NetLaunch r;
    if (int rc = launch_net(h, level, lv.c, h->cfg.F, net_args(h, lv, sd, h->bufA, lv.c, lv.c / 2, N), s, net_call(h, NET_FWD), &r)) return rc;
    if (logdet_dev) {
      // logdet accumulator starts at the step's constant h*w*(sum log_scale + sum log_S)
      std::vector<double> init(N, h->ld_step[(size_t)level * h->cfg.K + step]);
      HIPCHK(hipMemcpyAsync(h->bufLd, init.data(), (size_t)N * 8, hipMemcpyHostToDevice, s));
      HIPCHK(hipStreamSynchronize(s));
    }
    CoupleArgs ca = couple_reads(couple_args(h, lv, sd, h->bufA, N, 0, y_dev, lv.c), h->bufP, h->pstride, r);
    if (logdet_dev) ca.logdet = h->bufLd;
    if (int rc = launch_couple(lv.c, ca, N, s)) return rc;
    if (logdet_dev) {
      hipLaunchKernelGGL(k_prior, dim3(N), dim3(256), 0, s, (const float*)nullptr, 0, (const float*)nullptr, (const float*)nullptr,
                         (const double*)h->bufLd, (float*)nullptr, logdet_dev);
      LAUNCHCHK("k_prior(logdet)");
    }
    return 0;
  });
}

int glowk_step_inverse(glowk_handle* h, int level, int step, const float* y_dev, int N, float* u_dev, void* stream) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (int rc = check_ready(h, N)) return rc;
  if (level < 0 || level >= h->cfg.L || step < 0 || step >= h->cfg.K) return fail("no such step");
  if (!u_dev || !y_dev) return fail("null tensor");
  hipStream_t s = (hipStream_t)stream;
  const Level& lv = h->levels[level];
  const StepDev& sd = lv.dev[step];
  return guarded(h, s, [&]() -> int {
    NetLaunch r;
    if (int rc = launch_net(h, level, lv.c, h->cfg.F, net_args(h, lv, sd, y_dev, lv.c, lv.c / 2, N), s, net_call(h, NET_FWD), &r)) return rc;
    CoupleArgs ca = couple_reads(couple_args(h, lv, sd, y_dev, N, 1, u_dev, lv.c), h->bufP, h->pstride, r);
    ca.A = sd.Ainv; ca.b = sd.binv;
    return launch_couple(lv.c, ca, N, s);
  });
}

int glowk_coupling_net(glowk_handle* h, int level, int step, const float* xb_dev, int N, float* log_s_dev, float* t_dev, void* stream) {
  if (!h) return fail("null handle");
  DeviceGuard dg(h->device);
  if (int rc = check_ready(h, N)) return rc;
  if (level < 0 || level >= h->cfg.L || step < 0 || step >= h->cfg.K) return fail("no such step");
  if (!xb_dev || !log_s_dev || !t_dev) return fail("null tensor");
  hipStream_t s = (hipStream_t)stream;
  const Level& lv = h->levels[level];
  const StepDev& sd = lv.dev[step];
  return guarded(h, s, [&]() -> int {
    NetLaunch r;
    if (int rc = launch_net(h, level, lv.c, h->cfg.F, net_args(h, lv, sd, xb_dev, lv.c / 2, 0, N), s, net_call(h, NET_FWD), &r)) return rc;
    CoupleArgs ca = couple_reads(couple_args(h, lv, sd, nullptr, N, 0, nullptr, 0), h->bufP, h->pstride, r);   // the dumps alone
    ca.log_s_out = log_s_dev; ca.t_out = t_dev;
    return launch_couple(lv.c, ca, N, s);
  });
}

}  // extern "C"
