// The integer and range rules of DUET (audiosourcesep_amd/csrc/glowk_duet_index.h, the functions the kernels and the entry points call)
// run on the host under -fsanitize=address,undefined (tests/test_duet_cpu.py) against straightforward loops: ceil_log2 and the
// headroom of the shift, the half-open binning at and around its edges and for values no cast survives, the quantiser, the grid's
// strided and unrolled cover of a signal through a heap row of exactly `cells` entries, the smoothing taps through heap planes of
// exactly bins cells, the exclusion rule, and the greedy picks against a brute-force restatement.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../audiosourcesep_amd/csrc/glowk_duet_index.h"

using namespace glowk_duet;

static int fail(const char* what, long a, long b, long c) {
  std::printf("%s(%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

static uint64_t lcg(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 33;
}

// every cell of a signal is visited exactly once by workgroup g, thread t, step k, slot u: c = g THREADS + t + (k UNROLL + u) groups THREADS
static int sweep_cover(int64_t cells) {
  const int groups = hist_groups(cells);
  if (groups < 1 || groups > HIST_MAX_GROUPS) return 1;
  std::vector<unsigned char> hit((size_t)cells, 0);
  const int64_t stride = (int64_t)groups * HIST_THREADS;
  for (int g = 0; g < groups; ++g)
    for (int t = 0; t < HIST_THREADS; ++t)
      for (int64_t k0 = (int64_t)g * HIST_THREADS + t; k0 < cells; k0 += HIST_UNROLL * stride)
        for (int u = 0; u < HIST_UNROLL; ++u)
          if (k0 + u * stride < cells) ++hit[(size_t)(k0 + u * stride)];
  for (unsigned char v : hit)
    if (v != 1) return 1;
  return 0;
}

static int sweep_peaks(int n_a, int n_d, int smooth, int nsrc, int da, int dd, int kind, uint64_t seed) {
  const int bins = n_a * n_d;
  std::vector<int64_t> plane((size_t)bins), tmp((size_t)bins), ref((size_t)bins), ref2((size_t)bins);
  for (int c = 0; c < bins; ++c) {
    const int64_t v = kind == 0 ? (int64_t)(lcg(seed) % 1000003) : kind == 1 ? (int64_t)(lcg(seed) % 3) : kind == 2 ? 7 : 0;
    plane[(size_t)c] = ref[(size_t)c] = v;
  }
  std::vector<int32_t> peaks((size_t)(2 * nsrc));
  const int found = pick_peaks_host(plane.data(), tmp.data(), n_a, n_d, smooth, nsrc, da, dd, peaks.data());
  // brute force: 3 x 3 weights per pass, then exhaustive picks
  for (int pass = 0; pass < smooth; ++pass) {
    for (int i = 0; i < n_a; ++i)
      for (int j = 0; j < n_d; ++j) {
        int64_t s = 0;
        for (int u = -1; u <= 1; ++u)
          for (int v = -1; v <= 1; ++v)
            if (i + u >= 0 && i + u < n_a && j + v >= 0 && j + v < n_d) s += (2 - std::abs(u)) * (2 - std::abs(v)) * ref[(size_t)((i + u) * n_d + j + v)];
        ref2[(size_t)(i * n_d + j)] = s;
      }
    ref.swap(ref2);
  }
  for (int c = 0; c < bins; ++c)
    if (ref[(size_t)c] != plane[(size_t)c]) return 1;
  std::vector<char> ex((size_t)bins, 0);
  int k = 0;
  for (; k < nsrc; ++k) {
    int at = -1;
    for (int c = 0; c < bins; ++c)
      if (!ex[(size_t)c] && ref[(size_t)c] > 0 && (at < 0 || ref[(size_t)c] > ref[(size_t)at])) at = c;
    if (at < 0) break;
    if (k >= found || peaks[(size_t)(2 * k)] != at / n_d || peaks[(size_t)(2 * k + 1)] != at % n_d) return 1;
    for (int c = 0; c < bins; ++c)
      if (std::abs(c / n_d - at / n_d) <= da && std::abs(c % n_d - at % n_d) <= dd) {
        if (!excluded_by(c / n_d, c % n_d, at / n_d, at % n_d, da, dd)) return 1;
        ex[(size_t)c] = 1;
      } else if (excluded_by(c / n_d, c % n_d, at / n_d, at % n_d, da, dd)) {
        return 1;
      }
  }
  if (k != found) return 1;
  for (int m = found; m < nsrc; ++m)
    if (peaks[(size_t)(2 * m)] != -1 || peaks[(size_t)(2 * m + 1)] != -1) return 1;
  return 0;
}

int main() {
  // ceil_log2 and the shift: cells 2^s 16^smooth <= 2^62 for every size the entry points admit
  for (int64_t n = 1; n <= 70000; ++n) {
    int k = 0;
    while (((int64_t)1 << k) < n) ++k;
    if (ceil_log2(n) != k) return fail("ceil_log2", (long)n, k, ceil_log2(n));
  }
  for (int b = 0; b <= 27; ++b)
    for (int64_t n : {((int64_t)1 << b) - 1, (int64_t)1 << b, ((int64_t)1 << b) + 1}) {
      if (n < 1 || n > (int64_t)MAX_ROWS * MAX_FRAMES) continue;
      for (int smooth = 0; smooth <= MAX_SMOOTH; ++smooth) {
        const int s = hist_shift(n, smooth);
        if (s < 1 || s > MAX_SHIFT) return fail("hist_shift range", (long)n, smooth, s);
        if (s + ceil_log2(n < 2 ? 2 : n) + 4 * smooth > 62) return fail("hist_shift headroom", (long)n, smooth, s);
      }
    }
  // binning: against the integer count on exact grids, at the edges, and for values that no int holds
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (int n : {1, 3, 35, 50, 51, 127, 128, 129, 16384}) {
    const double lo = -3.0, hi = 3.0;
    if (bin_of(lo, lo, hi, n) != 0) return fail("bin_of lo", n, 0, 0);
    if (bin_of(hi, lo, hi, n) != -1) return fail("bin_of hi", n, 0, 0);
    if (bin_of(std::nextafter(lo, -inf), lo, hi, n) != -1) return fail("bin_of below lo", n, 0, 0);
    const int top = bin_of(std::nextafter(hi, lo), lo, hi, n);
    if (top != n - 1 && top != -1) return fail("bin_of below hi", n, top, 0);
    for (double v : {inf, -inf, nan, 1e300, -1e300, 1.7976931348623157e308, -1.7976931348623157e308})
      if (bin_of(v, lo, hi, n) != -1) return fail("bin_of huge", n, 0, 0);
    for (int i = 0; i < n; ++i) {
      const double c = bin_centre(lo, hi, n, i);
      if (bin_of(c, lo, hi, n) != i) return fail("bin_of centre", n, i, bin_of(c, lo, hi, n));
    }
  }
  // power-of-two grid: exact arithmetic, every point against the integer rule
  for (int k = -40; k < 72; ++k) {
    const int want = k >= 0 && k < 32 ? k / 4 : -1;
    if (bin_of((double)k * 0.25, 0.0, 8.0, 8) != want) return fail("bin_of grid", k, want, 0);
  }
  // the quantiser and the exponent
  for (double wmax : {1.0, 0.75, 3.0, 1e-300, 1e300, 4.9406564584124654e-324, 1.7976931348623157e308, 0.5}) {
    const int e = weight_exponent(wmax);
    if (!(wmax < std::ldexp(1.0, e)) && e < 1024) return fail("weight_exponent", e, 0, 0);
    if (!(wmax >= std::ldexp(1.0, e - 1))) return fail("weight_exponent low", e, 0, 0);
    for (int s : {1, 23, 40}) {
      const int64_t v = quantise(wmax, s - e);
      if (v < 0 || v > ((int64_t)1 << s)) return fail("quantise", e, s, (long)v);
      if (quantise(wmax * 0.5, s - e) > v) return fail("quantise monotone", e, s, 0);
    }
  }
  if (weight_counts(0.0) || weight_counts(-1.0) || weight_counts(inf) || weight_counts(nan) || !weight_counts(4.9406564584124654e-324) ||
      !weight_counts(1.7976931348623157e308))
    return fail("weight_counts", 0, 0, 0);
  // the strided cover and the plan
  for (int64_t cells : {(int64_t)1, (int64_t)2, (int64_t)15, (int64_t)511, (int64_t)512, (int64_t)513, (int64_t)8191, (int64_t)8192, (int64_t)8193,
                        (int64_t)33 * 64, (int64_t)1025 * 96, (int64_t)4096 * 34, (int64_t)512 * 16 * 512 - 1, (int64_t)512 * 16 * 512 + 1, (int64_t)1025 * 5626})
    if (sweep_cover(cells)) return fail("sweep_cover", (long)cells, 0, 0);
  for (int n_a : {1, 3, 35, 50, 127, 128})
    for (int n_d : {1, 5, 51, 50, 129, 128}) {
      if (n_a * n_d > MAX_BINS) continue;
      const HistPlan p = hist_plan(3, 1025 * 96, n_a, n_d);
      if (p.lds_bytes != (size_t)n_a * n_d * 8 || p.lds_bytes > (size_t)MAX_BINS * 8) return fail("hist_plan lds", n_a, n_d, 0);
      if (p.bytes != (size_t)3 * p.groups * 8) return fail("hist_plan bytes", n_a, n_d, 0);
    }
  // smoothing and picks
  uint64_t seed = 12345;
  for (int n_a : {1, 2, 3, 7, 35})
    for (int n_d : {1, 2, 5, 8, 51})
      for (int smooth = 0; smooth <= MAX_SMOOTH; ++smooth)
        for (int kind = 0; kind < 4; ++kind)
          for (int dist : {0, 1, 5, 100}) {
            if (sweep_peaks(n_a, n_d, smooth, 1, dist, dist, kind, ++seed)) return fail("sweep_peaks 1", n_a, n_d, smooth);
            if (sweep_peaks(n_a, n_d, smooth, 5, dist, dist / 2, kind, ++seed)) return fail("sweep_peaks 5", n_a, n_d, smooth);
            if (sweep_peaks(n_a, n_d, smooth, MAX_SRC, dist / 2, dist, kind, ++seed)) return fail("sweep_peaks 16", n_a, n_d, smooth);
          }
  if (omega_of(0, 1) != 0.0 || omega_of(0, 1025) != 0.0 || omega_of(1024, 1025) != TWO_PI * 1024.0 / 2048.0) return fail("omega_of", 0, 0, 0);
  if (peaks_bytes(2, 35, 51) != (size_t)2 * 2 * 35 * 51 * 8 || assign_bytes(2, 4, 1025) != (size_t)2 * 4 * 1025 * 32) return fail("bytes", 0, 0, 0);
  std::printf("DUET_INDEX_SANITIZE_OK\n");
  return 0;
}
