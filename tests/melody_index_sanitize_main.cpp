// The host-side rules of the melody kernels (audiosourcesep_amd/csrc/glowk_melody_index.h, the functions the kernels and the entry
// points call) run on the host under -fsanitize=address,undefined (tests/test_melody_cpu.py) against straightforward loops: the
// position table into heap buffers of exactly B H entries (every read of a live term inside the spectrogram), the salience grid (every
// (bin, frame) in exactly one thread), the emission's chunks, the track's thread and chunk rules (every back pointer of a chunk inside
// the LDS array and inside the workspace), and the fused call's workspace layout.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../audiosourcesep_amd/csrc/glowk_melody_index.h"

using namespace glowk_melody;

static int check_positions(int B, int H, double fmin, double per_octave, double bin_hz, int rows) {
  std::vector<double> f0(B);
  for (int b = 0; b < B; ++b) f0[b] = fmin * std::pow(2.0, b / per_octave);
  if (!grid_ok(f0.data(), B, bin_hz)) { std::printf("grid_ok(%d, %g)\n", B, fmin); return 1; }
  int32_t* idx = (int32_t*)std::malloc((size_t)B * H * sizeof(int32_t));      // exactly the stated sizes: one past the end is an overflow
  double* frac = (double*)std::malloc((size_t)B * H * sizeof(double));
  positions(f0.data(), B, H, bin_hz, rows, idx, frac);
  int rc = 0, dead = 0;
  for (int b = 0; b < B && !rc; ++b)
    for (int h = 1; h <= H; ++h) {
      const double p = h * f0[b] / bin_hz;
      long long i = 0;
      while ((double)(i + 1) <= p && i < rows) ++i;                               // floor by counting (past the last row it is dead anyway)
      const int32_t got = idx[(size_t)b * H + h - 1];
      const double a = frac[(size_t)b * H + h - 1];
      if (i + 1 <= rows - 1) {
        if (got != i || a != p - (double)i || !(a >= 0.0 && a < 1.0)) { std::printf("position(%d, %d): %d %g, expected %lld\n", b, h, got, a, i); rc = 1; break; }
        if (got + 1 > rows - 1) { std::printf("read(%d, %d)\n", b, h); rc = 1; break; }   // the term's second read, row i + 1
      } else {
        ++dead;
        if (got != -1 || a != 0.0) { std::printf("dead(%d, %d): %d %g\n", b, h, got, a); rc = 1; break; }
      }
    }
  std::free(idx);
  std::free(frac);
  return rc ? -1 : dead;
}

static int check_salience(int B, int frames) {
  const int blocks = sal_blocks(B, frames);
  const int64_t cells = (int64_t)B * frames;
  if ((int64_t)blocks * SAL_THREADS < cells || (int64_t)(blocks - 1) * SAL_THREADS >= cells) { std::printf("sal_blocks(%d, %d) = %d\n", B, frames, blocks); return 1; }
  // the last workgroup's threads, as the kernel maps them: q -> (bin, frame), the frame fastest
  for (int64_t q = (int64_t)(blocks - 1) * SAL_THREADS; q < (int64_t)blocks * SAL_THREADS; ++q) {
    if (q >= cells) continue;
    const int b = (int)(q / frames), t = (int)(q - (int64_t)b * frames);
    if (b < 0 || b >= B || t < 0 || t >= frames || (int64_t)b * frames + t != q) return 1;
  }
  return 0;
}

static int check_emission(int64_t cells) {
  const int groups = emi_groups(cells);
  int want = 0;
  for (int64_t c = 0; c < cells && want < EMI_MAX_GROUPS; c += EMI_MIN_CELLS) ++want;
  if (groups != want || groups < 1 || groups > EMI_THREADS) { std::printf("groups(%lld) = %d\n", (long long)cells, groups); return 1; }
  int64_t next = 0;
  for (int g = 0; g < groups; ++g) {
    int64_t c0, c1;
    emi_chunk(cells, g, c0, c1);
    if (c0 != next || c1 <= c0 || c1 > cells) { std::printf("chunk(%lld)[%d] = [%lld, %lld)\n", (long long)cells, g, (long long)c0, (long long)c1); return 1; }
    next = c1;
  }
  if (next != cells) return 1;
  const int blocks = emi_blocks(cells);
  if ((int64_t)blocks * EMI_THREADS * EMI_PER_THREAD < cells || (int64_t)(blocks - 1) * EMI_THREADS * EMI_PER_THREAD >= cells) return 1;
  return 0;
}

static int check_track(int B, int frames) {
  const int threads = trk_threads(B), ub = trk_unvoiced_thread(B);
  if (threads % 64 || threads < 64 || threads > TRK_MAX_THREADS || threads < B || (threads < B + 1 && B != TRK_MAX_THREADS)) { std::printf("threads(%d) = %d\n", B, threads); return 1; }
  if (threads >= B + 1 + 64) { std::printf("threads(%d) = %d: a whole wave idle\n", B, threads); return 1; }
  if (ub < 0 || ub >= threads || (ub != B && !(B == TRK_MAX_THREADS && ub == 0))) { std::printf("unvoiced(%d) = %d\n", B, ub); return 1; }
  const int tc = trk_chunk_frames(B);
  if (tc < 1 || (int64_t)tc * (B + 1) > TRK_CHUNK || (int64_t)(tc + 1) * (B + 1) <= TRK_CHUNK) { std::printf("chunk_frames(%d) = %d\n", B, tc); return 1; }
  // the back-trace as the kernel walks it: every frame t >= 1 in exactly one chunk, latest first; every index inside the LDS array and
  // inside a workspace of exactly the stated size
  const size_t bytes = trk_bp_bytes(B, frames);
  if (bytes % 8 || bytes < (size_t)frames * (B + 1) * 2 || bytes >= (size_t)frames * (B + 1) * 2 + 8) return 1;
  uint16_t* bp = (uint16_t*)std::calloc(bytes / 2, 2);
  uint16_t* lds = (uint16_t*)std::calloc(TRK_CHUNK, 2);
  int expect = frames - 1, rc = 0;
  for (int hi = frames - 1; hi > 0 && !rc; hi -= tc) {
    const int lo = hi - tc > 0 ? hi - tc : 0;
    const int n = (hi - lo) * (B + 1);
    const uint16_t* src = bp + (size_t)(lo + 1) * (B + 1);
    for (int k = 0; k < n; ++k) lds[k] = src[k];
    for (int t = hi; t > lo; --t) {
      if (t != expect) { rc = 1; break; }
      --expect;
      if (lds[(t - lo - 1) * (B + 1) + B] != 0) { rc = 1; break; }
    }
  }
  if (expect != 0) rc = 1;
  if (rc) std::printf("back-trace(%d, %d)\n", B, frames);
  std::free(bp);
  std::free(lds);
  return rc;
}

static int check_fit(int nsig, int B, int frames) {
  const FitPlan p = fit_plan(nsig, B, frames);
  const size_t cells = (size_t)nsig * B * frames;
  const size_t ends[4][2] = {{p.emi, cells * 8}, {p.sal, cells * 4}, {p.part, emi_work_bytes(nsig, B, frames)}, {p.bp, trk_work_bytes(nsig, B, frames)}};
  size_t next = 0;
  for (const auto& e : ends) {
    if (e[0] % 8 || e[0] < next) { std::printf("fit_plan(%d, %d, %d)\n", nsig, B, frames); return 1; }
    next = e[0] + e[1];
  }
  if (p.bytes < next || p.bytes >= next + 8) return 1;
  if (emi_work_bytes(nsig, B, frames) < (size_t)nsig * emi_groups((int64_t)B * frames) * 4) return 1;
  if (trk_work_bytes(nsig, B, frames) != (size_t)nsig * trk_bp_bytes(B, frames)) return 1;
  return 0;
}

int main() {
  long checks = 0;
  for (int B = 1; B <= MAX_BINS; ++B)
    for (int frames : {1, 2, 63, 64, 65, 255, 256, 257, 5626, 32767, 32768}) {
      if (check_salience(B, frames)) return 1;
      ++checks;
    }
  for (int64_t cells = 1; cells <= 20000; ++cells, ++checks)
    if (check_emission(cells)) return 1;
  for (int64_t cells : {(int64_t)4096 * 255, (int64_t)4096 * 255 + 1, (int64_t)4096 * 256, (int64_t)4096 * 256 + 1, (int64_t)300 * 5626, (int64_t)1024 * 32768})
    if (check_emission(cells)) return 1;
  for (int B = 1; B <= MAX_BINS; ++B)
    for (int frames : {1, 2, 3, 17, 18, 19, 61, 62, 63, 257, 1000}) {
      if (check_track(B, frames)) return 1;
      ++checks;
    }
  if (check_track(3, 4100) || check_track(3, 32768) || check_track(300, 5626)) return 1;
  if (trk_threads(62) != 64 || trk_threads(63) != 64 || trk_threads(64) != 128 || trk_threads(1023) != 1024 || trk_threads(1024) != 1024) { std::printf("thread counts\n"); return 1; }
  if (trk_chunk_frames(300) != 61 || trk_chunk_frames(1024) != 17) { std::printf("chunk frames\n"); return 1; }
  const int shapes[][3] = {{1, 1, 1}, {2, 5, 7}, {3, 65, 65}, {1, 300, 126}, {1, 1024, 257}, {1, 300, 5626}, {65535, 1, 1}, {1, 1024, 32768}, {63, 1024, 32768}};
  for (const auto& s : shapes)
    if (check_fit(s[0], s[1], s[2])) return 1;
  // position tables: the default grid on the default spectra, grids with harmonics beyond the last row, the extremes of the ranges
  long dead = 0;
  const double grids[][3] = {{55.0, 60.0, 7.8125}, {55.0, 12.0, 7.8125}, {7.8125, 1.0, 7.8125}, {1.0, 600.0, 0.37}, {3000.0, 60.0, 7.8125}};
  for (const auto& g : grids)
    for (int rows : {2, 3, 17, 129, 1025, 4096})
      for (int B : {1, 2, 63, 300, 1024})
        for (int H : {1, 2, 8, 32}) {
          if (g[1] == 1.0 && B > 40) continue;                                    // 2^B Hz overflows the table's int32
          const int d = check_positions(B, H, g[0], g[1], g[2], rows);
          if (d < 0) return 1;
          dead += d;
          ++checks;
        }
  if (dead == 0) { std::printf("no grid reached beyond the last row\n"); return 1; }
  // the grids the library refuses
  const double bad[][3] = {{1.0, 1.0, 2.0}, {2.0, 1.0, 3.0}, {0.0, 1.0, 2.0}, {-1.0, 1.0, 2.0}, {1.0, 2.0, INFINITY}, {1.0, NAN, 3.0}};
  for (const auto& f : bad)
    if (grid_ok(f, 3, 7.8125)) { std::printf("a bad grid was accepted\n"); return 1; }
  const double good[3] = {1.0, 2.0, 3.0};
  if (!grid_ok(good, 3, 7.8125) || grid_ok(good, 3, 0.0) || grid_ok(good, 3, -1.0) || grid_ok(good, 3, NAN) || grid_ok(good, 3, INFINITY)) return 1;
  // the ranges
  if (!sizes_ok(0, 2, 1, 1) || !sizes_ok(65535, 4096, 8, 1) || sizes_ok(65535, 4096, 9, 1) || sizes_ok(1, 1, 1, 1) || sizes_ok(1, 4097, 1, 1) || sizes_ok(1, 2, 0, 1) ||
      sizes_ok(1, 2, 32769, 1) || sizes_ok(1, 2, 1, 0) || sizes_ok(1, 2, 1, 1025) || sizes_ok(-1, 2, 1, 1) || sizes_ok(65536, 2, 1, 1) || sizes_ok(64, 2, 32768, 1024) ||
      !sizes_ok(63, 2, 32768, 1024)) { std::printf("sizes_ok\n"); return 1; }
  std::printf("MELODY_INDEX_SANITIZE_OK %ld checks, %ld dead terms\n", checks, dead);
  return 0;
}
