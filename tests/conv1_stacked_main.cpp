// Host-only check of the conv1 operands in the forward image of the 16x16x32 kernels (audiosourcesep_amd/csrc/glowk_pack.h, the RSp
// image; tests/test_conv1_stacked.py builds this under -fsanitize=address,undefined).  For the level shapes c = 4, 8, 16 at F = 128 and
// 512 a step with random weights is packed, the conv1 part of the image is read back the way the kernels read it -- k-step s, lane
// (n16, kq), register j; stacked along K where glowk_conv1_stacked says so (c = 4, 8), three split terms otherwise (c = 16) -- against
// the B fragment of a random im2col vector split as the kernels split it (hi = fp16(x), lo = fp16(x - hi)), and the fp64 sum over the
// slots is compared with the fp64  sum_k w_k x_k + bias  of the scaled, BatchNorm-folded weights the packer split.
//
// The bound, per output row:  2^-20 * sum_k |w_k x_k|.  hi + lo represents a value to 2^-22 relative (11 significant bits each), so the
// weight's and the activation's representation errors and the dropped lo.lo product are 2^-22 |w x| each: three in all, rounded up to
// a power of two.  Both sums are taken in fp64.
//
// Stacked shapes also: every slot beyond 3 K1 + 2 is zero, and in map mode (the device-side refresh of the images after an optimizer
// step) every conv1 weight code appears exactly twice as a hi half and once as a lo half, a bias-row code once as hi and once as lo, and
// every map entry reproduces, bit for bit, the half the value mode wrote at that position.
#include "../audiosourcesep_amd/csrc/glowk_pack.h"

#include <cstdio>
#include <random>

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails < 40) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } ++fails; } } while (0)

static Level make_level(const glowk_config& cfg, int c, std::mt19937& rng) {
  Level lv;
  lv.h = 8; lv.w = 8; lv.c = c; lv.z_off = 0; lv.z_width = 0; lv.Cz = 0;
  std::normal_distribution<float> nd(0.0f, 0.05f);
  for (int id = 0; id < GLOWK_NUM_STEP_TENSORS; ++id) {
    lv.host[id].resize(1);
    std::vector<float>& t = lv.host[id][0];
    t.assign(step_tensor_size(cfg, lv, id), 0.0f);
    for (float& v : t) v = nd(rng);
  }
  // a well-conditioned 1x1: P = a cyclic shift, unit lower L, U with a +-e^{log_S} diagonal
  std::vector<float>& P = lv.host[GLOWK_INV1X1_P][0];
  std::fill(P.begin(), P.end(), 0.0f);
  for (int i = 0; i < c; ++i) P[(size_t)i * c + (i + 1) % c] = 1.0f;
  for (int i = 0; i < c; ++i) lv.host[GLOWK_INV1X1_SIGN_S][0][i] = (i & 1) ? -1.0f : 1.0f;
  std::fill(lv.host[GLOWK_INV1X1_P_INV][0].begin(), lv.host[GLOWK_INV1X1_P_INV][0].end(), 0.0f);
  for (float& v : lv.host[GLOWK_BN1_VAR][0]) v = 1.0f + std::fabs(v);
  for (float& v : lv.host[GLOWK_BN2_VAR][0]) v = 1.0f + std::fabs(v);
  for (float& v : lv.host[GLOWK_BN1_GAMMA][0]) v += 1.0f;
  for (float& v : lv.host[GLOWK_BN2_GAMMA][0]) v += 1.0f;
  return lv;
}

int main() {
  std::mt19937 rng(4321);
  const int shapes[][2] = {{4, 128}, {8, 128}, {16, 128}, {4, 512}, {8, 512}, {16, 512}};
  for (const auto& sh : shapes) {
    const int c = sh[0], F = sh[1], CI = c / 2, NF = F / 32, K1 = 9 * CI;
    glowk_config cfg{};
    cfg.H = 16; cfg.W = 16; cfg.C = 1; cfg.L = 2; cfg.K = 1; cfg.F = F; cfg.learntop = 1; cfg.use_logit = 0;
    cfg.minval = -100.f; cfg.maxval = 20.f; cfg.alpha = 1e-10f; cfg.bn_eps = 1e-3f;
    const StepLayout SL = step_layout(c, F);
    CHECK(SL.slotS != 0, "c=%d F=%d: no image for the 16x16x32 kernels", c, F);
    if (!SL.slotS) continue;
    const Level lv = make_level(cfg, c, rng);
    std::vector<float> img(SL.total, 0.0f);
    double ldc; float sc[8]; std::string err;
    CHECK(pack_step(cfg, lv, 0, img.data(), &ldc, sc, &err), "c=%d F=%d: %s", c, F, err.c_str());

    // the weights the packer split: conv1 kernel rows and the bias row, each output channel scaled by the power of two of its
    // BatchNorm factor (K1f), then by the layer's power of two S1 (sc[0] = 2^-S1)
    const float* ep = img.data() + SL.ep;            // [b1 | g1 | ...]
    const float* Kc = lv.host[GLOWK_CONV1_KERNEL][0].data();
    const int S1 = -std::ilogb(sc[0]);
    CHECK(std::ldexp(1.0f, -S1) == sc[0], "c=%d F=%d: conv1 scale %g is not a power of two", c, F, sc[0]);
    std::vector<float> K1f((size_t)(K1 + 1) * F);
    for (int f = 0; f < F; ++f) {
      int e = 0;
      std::frexp((double)ep[F + f], &e);
      if (ep[F + f] == 0.0f) e = 0;
      for (int kk = 0; kk <= K1; ++kk) K1f[(size_t)kk * F + f] = std::ldexp(kk < K1 ? Kc[(size_t)kk * F + f] : ep[f], e);
    }
    auto ws = [&](int kk, int f) { return (double)std::ldexp(K1f[(size_t)kk * F + f], S1); };

    // a random im2col vector in the kernels' scaled units, split as split8 does
    std::normal_distribution<float> nd(0.0f, 1.0f);
    std::vector<float> x(K1);
    std::vector<double> xh(K1), xl(K1);
    for (int k = 0; k < K1; ++k) {
      x[k] = nd(rng) * GLOWK_ACT_SCALE;
      const uint16_t h = f32_to_f16(x[k]);
      xh[k] = f16_to_f32(h);
      xl[k] = f16_to_f32(f32_to_f16(x[k] - f16_to_f32(h)));
    }
    const double cb = GLOWK_ACT_SCALE;              // the constant that carries the bias (its lo half is zero)

    const bool stk = glowk_conv1_stacked(K1);
    CHECK(stk == (c <= 8), "c=%d: stacked = %d", c, (int)stk);
    const int KSS = glowk_conv1_ks(K1), KSX = stk ? glowk_conv1_ks_stacked(K1) : KSS;
    CHECK(!stk || KSX == (c == 4 ? 2 : 4), "c=%d: %d stacked k-steps", c, KSX);
    const size_t blk_halves = (size_t)KSS * 4 * 64 * 8;      // per hidden block: 4 KSS pieces of 64 lanes x 8 halves, either layout
    const uint16_t* i16 = reinterpret_cast<const uint16_t*>(img.data() + SL.RSp);
    auto half_at = [&](int blk, int piece, int lane, int j) { return (double)f16_to_f32(i16[(size_t)blk * blk_halves + ((size_t)piece * 64 + lane) * 8 + j]); };
    double worst = 0.0;
    for (int blk = 0; blk < NF; ++blk)
      for (int row = 0; row < 32; ++row) {
        const int rb = row >> 4, n16 = row & 15, f = blk * 32 + row;
        double got = 0.0, ref = ws(K1, f) * cb, mag = 0.0;
        for (int k = 0; k < K1; ++k) { ref += ws(k, f) * (double)x[k]; mag += std::fabs(ws(k, f) * (double)x[k]); }
        if (stk) {
          for (int s = 0; s < 2 * KSS; ++s)
            for (int kq = 0; kq < 4; ++kq)
              for (int j = 0; j < 8; ++j) {
                const int p = 32 * s + 8 * kq + j;
                const double a = half_at(blk, s * 2 + rb, kq * 16 + n16, j);
                const double b = p < K1 ? xh[p] : p < 2 * K1 ? xl[p - K1] : p < 3 * K1 ? xh[p - 2 * K1] : p < 3 * K1 + 2 ? cb : 0.0;
                if (p >= 3 * K1 + 2 || s >= KSX) CHECK(a == 0.0, "c=%d F=%d block %d row %d: slot %d beyond the stacked contraction holds %g", c, F, blk, row, p, a);
                if (s < KSX) got += a * b;          // (the kernels run KSX k-steps)
              }
        } else {
          for (int s = 0; s < KSS; ++s)
            for (int kq = 0; kq < 4; ++kq)
              for (int j = 0; j < 8; ++j) {
                const int k = 32 * s + 8 * kq + j;
                const double ah = half_at(blk, (s * 2 + rb) * 2 + 0, kq * 16 + n16, j), al = half_at(blk, (s * 2 + rb) * 2 + 1, kq * 16 + n16, j);
                const double bh = k < K1 ? xh[k] : k == K1 ? cb : 0.0, bl = k < K1 ? xl[k] : 0.0;
                got += al * bh + ah * bl + ah * bh;
              }
        }
        const double bound = std::ldexp(mag, -20);
        CHECK(std::fabs(got - ref) <= bound, "c=%d F=%d block %d row %d: |%.17g - %.17g| = %.3g > %.3g", c, F, blk, row, got, ref, std::fabs(got - ref), bound);
        if (mag > 0.0) worst = std::max(worst, std::fabs(got - ref) / mag);
      }
    std::printf("c=%d F=%d %s: worst |sum - ref| / sum|w x| = %.3g (bound %.3g)\n", c, F, stk ? "stacked" : "three-term", worst, std::ldexp(1.0, -20));

    if (stk) {
      // map mode: the codes of the conv1 part, and the halves they stand for against the halves the value mode wrote
      std::vector<float> stage(SL.total, 0.0f);
      std::vector<int> map(SL.total * 2, -1);
      CHECK(pack_step(cfg, lv, 0, stage.data(), &ldc, sc, &err, map.data()), "c=%d F=%d map mode: %s", c, F, err.c_str());
      const F16Codes QC = f16_code_bases(c, F);
      const size_t n1 = (size_t)(K1 + 1) * F;
      std::vector<int> nhi(n1, 0), nlo(n1, 0);
      const size_t base = SL.RSp * 2;
      for (size_t pos = 0; pos < (size_t)NF * blk_halves; ++pos) {
        const int mv = map[base + pos];
        CHECK(mv >= 0, "c=%d F=%d: conv1 half %zu is not in the map", c, F, pos);
        if (mv < 0) continue;
        const int lo = (mv >> 30) & 1;
        const size_t code = (size_t)(mv & 0x3FFFFFFF);
        uint16_t want = 0;
        if (code) {
          CHECK(code > QC.A && code <= QC.A + n1, "c=%d F=%d: conv1 half %zu maps to code %zu of another tensor", c, F, pos, code);
          if (!(code > QC.A && code <= QC.A + n1)) continue;
          const size_t i = code - 1 - QC.A;
          ++(lo ? nlo : nhi)[i];
          const float w = std::ldexp(K1f[i], S1);
          const uint16_t hi = f32_to_f16(w);
          want = lo ? f32_to_f16(w - f16_to_f32(hi)) : hi;
        } else CHECK(!lo, "c=%d F=%d: a zero element with the lo bit at half %zu", c, F, pos);
        CHECK(i16[pos] == want, "c=%d F=%d: half %zu is %04x, its map entry gives %04x", c, F, pos, (unsigned)i16[pos], (unsigned)want);
      }
      for (size_t i = 0; i < n1; ++i) {
        const bool bias = i >= (size_t)K1 * F;
        CHECK(nhi[i] == (bias ? 1 : 2) && nlo[i] == 1, "c=%d F=%d: K1f element %zu appears %d times as hi, %d times as lo", c, F, i, nhi[i], nlo[i]);
      }
    }
  }
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("CONV1_STACKED_OK\n");
  return 0;
}
