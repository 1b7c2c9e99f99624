// The index rules of the convolutive NMF kernels (audiosourcesep_amd/csrc/glowk_nmfd_index.h, the functions the kernels and the entry
// points call) run on the host under -fsanitize=address,undefined (tests/test_nmfd_cpu.py) against straightforward loops: the walk over
// the stacked components two at a time without a division, exactly as the kernels clamp it; the H update's plane, written by the first
// launch and read by the second, in a heap buffer of exactly the stated size; an H tensor of exactly K frames floats under every
// shifted, clamped load; and the workspace size.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../audiosourcesep_amd/csrc/glowk_nmfd_index.h"

using namespace glowk_nmfd;

// the kernels' walk of one lane half over [lo, hi) of KS stacked components: (k, tau) of min(s, KS - 1) without a division; every load
// of H[k][clamp(f - tau)] lands in a heap buffer of K * F floats; a kept operand is the stacked activation's own element
static int check_walk(int K, int Tw, int F, int lo, int hi, int f) {
  const int KS = K * Tw;
  std::vector<float> h((size_t)K * F);
  for (size_t i = 0; i < h.size(); ++i) h[i] = (float)(i + 1);
  for (int half = 0; half < 2; ++half) {
    int k, tau;
    nmfd_split(lo + half < KS - 1 ? lo + half : KS - 1, Tw, k, tau);
    for (int s0 = lo; s0 < hi; s0 += 2) {
      const int s = s0 + half, ts = f - tau;
      if (k < 0 || k >= K || tau < 0 || tau >= Tw) { std::printf("walk(%d, %d): s %d -> (%d, %d)\n", K, Tw, s, k, tau); return 1; }
      const float b = h.at((size_t)k * F + (ts > 0 ? ts : 0));
      if (s < hi) {
        if (k != s / Tw || tau != s % Tw) { std::printf("walk(%d, %d): s %d -> (%d, %d)\n", K, Tw, s, k, tau); return 1; }
        const float want = f - s % Tw >= 0 ? h[(size_t)(s / Tw) * F + (f - s % Tw)] : 0.0f;
        if ((ts >= 0 ? b : 0.0f) != want) return 1;
      }
      nmfd_advance2(Tw, k, tau, s + 2 < KS);
    }
  }
  return 0;
}

// the plane: every (which, s, t) has its own slot in a buffer of exactly nmfd_plane_floats entries, and the second launch reads, for
// every (k, t), exactly the slots (k Tw + tau, t + tau) with t + tau < frames
static int check_plane(int K, int Tw, int F) {
  const int KS = K * Tw;
  const int64_t n = nmfd_plane_floats(KS, F);
  std::vector<unsigned char> seen((size_t)n, 0);
  for (int which = 0; which < 2; ++which)
    for (int s = 0; s < KS; ++s)
      for (int t = 0; t < F; ++t) {
        const int64_t i = nmfd_plane_index(which, s, t, KS, F);
        if (i < 0 || i >= n || seen.at((size_t)i)++) { std::printf("plane(%d, %d, %d): slot %lld\n", K, Tw, F, (long long)i); return 1; }
      }
  int64_t reads = 0;
  for (int k = 0; k < K; ++k)
    for (int t = 0; t < F; ++t) {
      const int taps = nmfd_taps(Tw, F, t);
      int want = 0;
      for (int tau = 0; tau < Tw; ++tau) want += t + tau < F;
      if (taps != want || taps < 1) { std::printf("taps(%d, %d, %d) = %d\n", Tw, F, t, taps); return 1; }
      for (int tau = 0; tau < taps; ++tau, ++reads)
        for (int which = 0; which < 2; ++which)
          if (seen.at((size_t)nmfd_plane_index(which, k * Tw + tau, t + tau, KS, F)) != 1) return 1;
    }
  return reads > 0 ? 0 : 1;
}

static int check_work(int rows, int F, int K, int Tw) {
  const int KS = K * Tw;
  const NmfPlan p = nmf_plan(rows, F, KS);
  int64_t m = (int64_t)8 * p.nch * rows * KS;
  if ((int64_t)8 * p.rtiles * p.nch > m) m = (int64_t)8 * p.rtiles * p.nch;
  if ((int64_t)8 * KS * F > m) m = (int64_t)8 * KS * F;
  const size_t one = nmfd_work_bytes(1, rows, F, K, Tw);
  if (one != (size_t)m || one % 8 || nmfd_work_bytes(0, rows, F, K, Tw) != 0) { std::printf("work(%d, %d, %d, %d)\n", rows, F, K, Tw); return 1; }
  if (one < glowk_nmf::nmf_work_bytes(1, rows, F, KS)) return 1;
  for (int nsig : {2, 3, 7, 65535})
    if (nmfd_work_bytes(nsig, rows, F, K, Tw) != one * (size_t)nsig) return 1;
  return 0;
}

int main() {
  long walks = 0;
  for (int Tw = 1; Tw <= MAX_TW; ++Tw)
    for (int K = 1; K * Tw <= MAX_STACK; ++K) {
      const int KS = K * Tw;
      for (int F : {1, 2, Tw - 1 > 0 ? Tw - 1 : 1, Tw, Tw + 1, 33})
        for (int f : {0, 1, Tw - 1, Tw, F - 1}) {
          if (f < 0 || f >= F) continue;
          // the whole range, padded as the update kernels pad it; and the ranges of sources, odd and even starts and lengths
          if (check_walk(K, Tw, F, 0, KS, f)) return 1;
          for (int k0 = 0; k0 < K; k0 += (K > 6 ? K / 3 : 1))
            for (int k1 = k0 + 1; k1 <= K; k1 += (K > 6 ? K / 3 : 1), ++walks)
              if (check_walk(K, Tw, F, k0 * Tw, k1 * Tw, f)) return 1;
        }
      if (KS <= 64 || Tw == 1 || K == 1)
        for (int F : {1, 3, Tw, Tw + 1, 70})
          if (check_plane(K, Tw, F)) return 1;
      for (int rows : {1, 33, 1025, 4096})
        for (int F : {1, 3, 97, 130, 5626, 32768})
          if (check_work(rows, F, K, Tw)) return 1;
    }
  // the shapes the GPU tests use
  const int shapes[][4] = {{1, 1, 1, 1}, {5, 3, 2, 4}, {33, 95, 3, 5}, {65, 33, 4, 32}, {64, 64, 1, 32}, {257, 130, 16, 8}, {1025, 97, 11, 3}, {40, 70, 128, 1}};
  for (const auto& s : shapes)
    if (check_plane(s[2], s[3], s[1]) || check_work(s[0], s[1], s[2], s[3])) return 1;
  // the padded walk of the update kernels: 2 kk + half up to 32 kt, held at the last stacked component of the lane's parity
  for (int Tw = 1; Tw <= MAX_TW; ++Tw)
    for (int K = 1; K * Tw <= MAX_STACK; ++K) {
      const int KS = K * Tw, KP = (KS + 31) / 32 * 32;
      for (int half = 0; half < 2; ++half) {
        int k, tau;
        nmfd_split(half < KS - 1 ? half : KS - 1, Tw, k, tau);
        for (int kk = 0; kk < KP / 2; ++kk) {
          const int s = 2 * kk + half;
          if (k < 0 || k >= K || tau < 0 || tau >= Tw) { std::printf("padded walk(%d, %d) at %d\n", K, Tw, s); return 1; }
          if (s < KS && (k != s / Tw || tau != s % Tw)) { std::printf("padded walk(%d, %d) at %d\n", K, Tw, s); return 1; }
          nmfd_advance2(Tw, k, tau, s + 2 < KS);
        }
      }
    }
  std::printf("NMFD_INDEX_SANITIZE_OK %ld walks\n", walks);
  return 0;
}
