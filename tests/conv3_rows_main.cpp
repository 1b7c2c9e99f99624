// Host-only check of the conv3 row order in the forward image of the 16x16x32 kernels (audiosourcesep_amd/csrc/glowk_act_scale.h:
// glowk_conv3_row; the RSp image of glowk_pack.h; tests/test_conv3_rows.py builds this under -fsanitize=address,undefined).
// At c = 8 and 16 the rows are ordered so that registers 3 u, 3 u + 1, 3 u + 2 of a lane group hold the taps dx = -1, 0, +1 of one
// (dy, channel) and the kernels can add them before they store.  For c = 8, 16 at F = 128 and 512:
//   * the map is a bijection of the 16 NMT image rows onto the 9 c (tap, channel) pairs plus zero padding;
//   * every triplet lies in one lane group and one accumulator group, dx in register order; its pre-summed row is the one the
//     kernels store to (32 gi + 4 u + kq = (dy + 1) c + channel), and the natural row of lane group kq is that of lane group 0 plus
//     kq (the kernels' decode);
//   * the conv3 part of a packed image, read tile by tile the way the kernels read it, holds in every row exactly the halves of the
//     split of the scaled, BatchNorm-folded conv3 weights of that row's (tap, channel), zeros in the padding rows;
//   * the map mode (device-side refresh) points every half at the same source element.
// For c = 4 (and 32 where it has an image) the map is the identity and the image is compared, half by half, with the natural order.
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

// the accumulator groups of the kernels (RingS: groups of <= 6 row tiles)
static int grp_n(int nmt, int gi) { return nmt - 6 * gi < 6 ? nmt - 6 * gi : 6; }

static void check_map(int c) {
  const int nmt = (9 * c + 15) / 16, M = 9 * c;
  std::vector<int> seen(M, 0);
  int pad = 0;
  for (int m = 0; m < 16 * nmt; ++m) {
    const int n = glowk_conv3_row(c, m);
    CHECK(n >= 0 && n <= M, "c=%d: row %d maps to %d", c, m, n);
    if (n >= 0 && n < M) ++seen[n]; else ++pad;
  }
  for (int n = 0; n < M; ++n) CHECK(seen[n] == 1, "c=%d: (tap %d, channel %d) is held by %d rows", c, n / c, n % c, seen[n]);
  CHECK(pad == 16 * nmt - M, "c=%d: %d padding rows", c, pad);
  if (!glowk_conv3_permuted(c)) {
    for (int m = 0; m < 16 * nmt; ++m) CHECK(glowk_conv3_row(c, m) == (m < M ? m : M), "c=%d: row %d is not in natural order", c, m);
    return;
  }
  // triplets: lane group kq, accumulator group gi, registers s = 4 ml + r of the group
  std::vector<int> rows(3 * c, 0);
  for (int gi = 0; gi * 6 < nmt; ++gi) {
    const int gn = grp_n(nmt, gi), ntrip = 4 * gn / 3;
    for (int kq = 0; kq < 4; ++kq) {
      for (int u = 0; u < ntrip; ++u) {
        int dyi = -1, co = -1;
        for (int d = 0; d < 3; ++d) {
          const int s = 3 * u + d, ml = s / 4, r = s % 4;
          CHECK(ml < gn, "c=%d: triplet %d of group %d leaves the group", c, u, gi);
          const int m = 16 * (6 * gi + ml) + 4 * kq + r;
          const int n = glowk_conv3_row(c, m);
          CHECK(n < M, "c=%d: register %d of a triplet is padding", c, s);
          const int tap = n / c;
          CHECK(tap % 3 == d, "c=%d group %d lane group %d register %d: dx = %d", c, gi, kq, s, tap % 3 - 1);
          if (d == 0) { dyi = tap / 3; co = n % c; }
          else CHECK(tap / 3 == dyi && n % c == co, "c=%d group %d lane group %d register %d: another (dy, channel)", c, gi, kq, s);
          // the kernels' decode: lane group 0's natural row plus kq; the pre-summed row 32 gi + 4 u + kq
          CHECK(n == glowk_conv3_row(c, 16 * (6 * gi + ml) + r) + kq, "c=%d row %d: not lane group 0's row + kq", c, m);
          CHECK(glowk_conv3_triplet(c, m) == 3 * (32 * gi + 4 * u + kq) + d, "c=%d row %d: triplet code", c, m);
        }
        const int T = 32 * gi + 4 * u + kq;
        CHECK(T == dyi * c + co, "c=%d: triplet row %d holds (dy %d, channel %d)", c, T, dyi - 1, co);
        if (T >= 0 && T < 3 * c) ++rows[T];
      }
      for (int s = 3 * ntrip; s < 4 * gn; ++s)      // spare registers: padding
        CHECK(glowk_conv3_row(c, 16 * (6 * gi + s / 4) + 4 * kq + s % 4) == M, "c=%d: spare register %d is not padding", c, s);
    }
  }
  for (int T = 0; T < 3 * c; ++T) CHECK(rows[T] == 1, "c=%d: pre-summed row %d is written %d times", c, T, rows[T]);
  CHECK(c != 8 || (nmt == 5 && 4 * grp_n(nmt, 0) / 3 == 6), "c=8: one group of five tiles, six triplets per lane group");
  CHECK(c != 16 || (nmt == 9 && grp_n(nmt, 0) == 6 && grp_n(nmt, 1) == 3), "c=16: groups of six and three tiles");
}

int main() {
  std::mt19937 rng(8765);
  for (int c : {4, 8, 16, 32}) check_map(c);
  const int shapes[][2] = {{4, 128}, {8, 128}, {16, 128}, {4, 512}, {8, 512}, {16, 512}};
  for (const auto& sh : shapes) {
    const int c = sh[0], F = sh[1], CI = c / 2, NF = F / 32, NFH = NF / 2;
    glowk_config cfg{};
    cfg.H = 16; cfg.W = 16; cfg.C = 1; cfg.L = 2; cfg.K = 1; cfg.F = F; cfg.learntop = 1; cfg.use_logit = 0;
    cfg.minval = -100.f; cfg.maxval = 20.f; cfg.alpha = 1e-10f; cfg.bn_eps = 1e-3f;
    const StepLayout SL = step_layout(c, F);
    CHECK(SL.slotS != 0, "c=%d F=%d: no image for the 16x16x32 kernels", c, F);
    if (!SL.slotS) continue;
    const Level lv = make_level(cfg, c, rng);
    std::vector<float> img(SL.total, 0.0f), stage(SL.total, 0.0f);
    std::vector<int> map(SL.total * 2, -1);
    double ldc; float sc[8]; std::string err;
    CHECK(pack_step(cfg, lv, 0, img.data(), &ldc, sc, &err), "c=%d F=%d: %s", c, F, err.c_str());
    CHECK(pack_step(cfg, lv, 0, stage.data(), &ldc, sc, &err, map.data()), "c=%d F=%d map mode: %s", c, F, err.c_str());

    // the weights the packer split: K3f[tap][f][co] = K3 * mantissa of the BatchNorm factor g2[f], scaled by 2^S3 (sc[2] = 2^-S3 / act)
    const float* ep = img.data() + SL.ep;            // [b1 | g1 | d1 | b2 | g2 | d2]
    const float* K3 = lv.host[GLOWK_CONV3_KERNEL][0].data();
    const int S3 = -std::ilogb(sc[2] * GLOWK_ACT_SCALE);
    CHECK(std::ldexp(1.0f, -S3) / GLOWK_ACT_SCALE == sc[2], "c=%d F=%d: conv3 scale %g", c, F, sc[2]);
    std::vector<float> K3f((size_t)9 * F * c);
    for (int tap = 0; tap < 9; ++tap)
      for (int f = 0; f < F; ++f) {
        int e;
        const double m2 = std::frexp((double)ep[4 * F + f], &e);
        for (int co = 0; co < c; ++co) K3f[((size_t)tap * F + f) * c + co] = (float)((double)K3[((size_t)tap * F + f) * c + co] * m2);
      }
    const F16Codes QC = f16_code_bases(c, F);

    // the conv3 chunks of the image as the kernels read them: pass ps, chunk NF + s, tile position tp -> tile t = s TPC + tp ->
    // (hidden block fo, row tile mt) in group order; lane (n16, kq) holds row 16 mt + n16 of A, k slot (kq, j)
    const int KSS = (9 * CI + 1 + 31) / 32, NMS = (9 * c + 15) / 16, TPC = 2 * NFH, NT = NFH * NMS, NCH = (NT + TPC - 1) / TPC;
    const size_t k1blkS = (size_t)KSS * 4 * 256, chunkf = (size_t)NFH * 1024;
    size_t nhalves = 0, nzero = 0;
    for (int ps = 0; ps < 2; ++ps)
      for (int s = 0; s < NCH; ++s)
        for (int tp = 0; tp < TPC; ++tp) {
          const size_t tile = SL.RSp + (size_t)NF * k1blkS + ((size_t)ps * (NF + NCH) + NF + s) * chunkf + (size_t)(tp * 2) * 256;   // floats
          const int t = s * TPC + tp;
          const int gi = t / (NFH * 6), gn = grp_n(NMS, gi), tl = t - gi * NFH * 6;
          const int fo = tl / gn, mt = 6 * gi + tl % gn;
          for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j)
              for (int hl = 0; hl < 2; ++hl) {
                const size_t pos = tile * 2 + (size_t)hl * 512 + (size_t)l * 8 + j;       // in halves from the start of the step
                const uint16_t got = reinterpret_cast<const uint16_t*>(img.data())[pos];
                const int n16 = l & 15, kq = l >> 4;
                // register r of lane group g holds A row 4 g + r: image row 16 mt + n16 is register n16 % 4 of lane group n16 / 4
                int n = 9 * c;
                if (t < NT) n = glowk_conv3_permuted(c) ? glowk_conv3_row(c, 16 * mt + (n16 & 3)) + (n16 >> 2) : 16 * mt + n16;   // c = 4: the natural order, spelled out
                uint16_t want = 0;
                size_t code = 0;
                if (n < 9 * c) {
                  const int f = (ps * NFH + fo) * 32 + 16 * (j >> 2) + 4 * kq + (j & 3);
                  const size_t idx = ((size_t)(n / c) * F + f) * c + n % c;
                  const float w = std::ldexp(K3f[idx], S3);
                  const uint16_t hi = f32_to_f16(w);
                  want = hl ? f32_to_f16(w - f16_to_f32(hi)) : hi;
                  code = QC.C + idx + 1;
                } else ++nzero;
                ++nhalves;
                CHECK(got == want, "c=%d F=%d pass %d tile %d lane %d half %d.%d: %04x, the split of row %d gives %04x", c, F, ps, t, l, j, hl, (unsigned)got,
                      n, (unsigned)want);
                const int mv = map[pos];
                CHECK(mv >= 0 && (size_t)(mv & 0x3FFFFFFF) == code && ((mv >> 30) & 1) == (code ? hl : (mv >> 30) & 1),
                      "c=%d F=%d pass %d tile %d lane %d half %d.%d: map entry %08x, source code %zu", c, F, ps, t, l, j, hl, (unsigned)mv, code);
              }
        }
    std::printf("c=%d F=%d: %zu conv3 halves of the image match the split of their rows (%zu in padding rows / tiles)\n", c, F, nhalves, nzero);
  }
  if (fails) { std::fprintf(stderr, "%d check(s) failed\n", fails); return 1; }
  std::printf("CONV3_ROWS_OK\n");
  return 0;
}
