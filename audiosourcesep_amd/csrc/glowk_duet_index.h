// glowk: the integer and range rules of DUET (glowk_duet.h), in plain C++ so that a host program can run them without HIP
// (tests/duet_index_sanitize_main.cpp sweeps them under AddressSanitizer + UBSan against straightforward loops).  The kernels and
// the entry points call the same functions.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GLOWK_DUET_HD __host__ __device__ inline
#else
#define GLOWK_DUET_HD inline
#endif

namespace glowk_duet {

constexpr int MAX_SIG = 65535, MAX_ROWS = 4096, MAX_FRAMES = 32768;
constexpr int MAX_BINS = 16384;             // n_a n_d: one workgroup holds the plane in LDS as 64-bit cells (128 KB)
constexpr int MAX_SRC = 16, MAX_SMOOTH = 3;
constexpr int MAX_SHIFT = 40;               // a counted weight becomes an integer below 2^40
constexpr int HIST_THREADS = 512;           // k_duet_wmax, k_duet_hist: threads per workgroup
constexpr int HIST_PER_THREAD = 16;         // cells per thread that size the grid
constexpr int HIST_MAX_GROUPS = 512;        // workgroups per signal, at most
constexpr int HIST_UNROLL = 4;              // cells whose loads a thread issues before it uses the first
constexpr int PEAK_THREADS = 512;           // k_duet_peaks: one workgroup per signal
constexpr double TWO_PI = 6.283185307179586476925286766559;

GLOWK_DUET_HD int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The smallest k with 2^k >= n, n >= 1.
GLOWK_DUET_HD int ceil_log2(int64_t n) {
  int k = 0;
  while (k < 62 && ((int64_t)1 << k) < n) ++k;
  return k;
}

// s: a counted weight w <= wmax < 2^e becomes rint(w 2^(s - e)) <= 2^s; `cells` of them sum to at most 2^(s + ceil_log2 cells), and
// every pass of the [1 2 1] x [1 2 1] kernel multiplies a bound by 16 = 2^4: with this s every sum stays at or below 2^62.
GLOWK_DUET_HD int hist_shift(int64_t cells, int smooth) {
  const int s = 62 - ceil_log2(cells < 2 ? 2 : cells) - 4 * smooth;
  return s < MAX_SHIFT ? s : MAX_SHIFT;
}

// The bin of v on [lo, hi) cut into n: floor((v - lo) n / (hi - lo)) in fp64 when it lies in [0, n), else -1 (not counted: outside,
// or not finite).  The comparison is made in fp64, before the conversion: a huge v never reaches the cast.
GLOWK_DUET_HD int bin_of(double v, double lo, double hi, int n) {
  const double f = floor((v - lo) * (double)n / (hi - lo));
  return f >= 0.0 && f < (double)n ? (int)f : -1;    // NaN fails both comparisons
}

// A weight counts when it is finite and positive.
GLOWK_DUET_HD bool weight_counts(double w) { return w > 0.0 && w <= 1.7976931348623157e308; }

// e with wmax < 2^e (wmax = m 2^e, 0.5 <= m < 1), for a finite wmax > 0.
GLOWK_DUET_HD int weight_exponent(double wmax) {
  int e;
  (void)frexp(wmax, &e);
  return e;
}

// The integer a counted weight adds to its cell: rint(w 2^shift), shift = s - e (ldexp is exact here: the result is at most 2^40).
GLOWK_DUET_HD int64_t quantise(double w, int shift) { return (int64_t)rint(ldexp(w, shift)); }

// The centre of bin i of [lo, hi) cut into n.
GLOWK_DUET_HD double bin_centre(double lo, double hi, int n, int i) { return lo + ((double)i + 0.5) * (hi - lo) / (double)n; }

// omega_r = 2 pi r / n_fft, n_fft = 2 (rows - 1); 0 for row 0 (also when rows == 1 and n_fft == 0).
GLOWK_DUET_HD double omega_of(int r, int rows) { return r == 0 ? 0.0 : TWO_PI * (double)r / (double)(2 * (rows - 1)); }

// Cell (i, j) is excluded by a pick at (pi, pj) when |i - pi| <= dist_a and |j - pj| <= dist_d.
GLOWK_DUET_HD bool excluded_by(int i, int j, int pi, int pj, int dist_a, int dist_d) {
  const int di = i > pi ? i - pi : pi - i, dj = j > pj ? j - pj : pj - j;
  return di <= dist_a && dj <= dist_d;
}

// One [1 2 1] tap along an axis of n cells with stride `stride`, zero beyond the edges; c is the cell's offset, k its index on the axis.
GLOWK_DUET_HD int64_t tap121(const int64_t* p, int64_t c, int k, int n, int64_t stride) {
  return (k > 0 ? p[c - stride] : 0) + 2 * p[c] + (k < n - 1 ? p[c + stride] : 0);
}

// Workgroups per signal of the two histogram passes: a function of the cell count alone.  (The sums are integers, so the result
// does not depend on it; the grid does.)
GLOWK_DUET_HD int hist_groups(int64_t cells) {
  const int64_t g = ceil_div64(cells, (int64_t)HIST_THREADS * HIST_PER_THREAD);
  return (int)(g < 1 ? 1 : g > HIST_MAX_GROUPS ? HIST_MAX_GROUPS : g);
}
struct HistPlan {
  int groups;
  size_t lds_bytes;                         // bins * 8
  size_t bytes;                             // workspace: nsig * groups partial maxima (fp64)
};
GLOWK_DUET_HD HistPlan hist_plan(int nsig, int64_t cells, int n_a, int n_d) {
  HistPlan p;
  const int bins = n_a * n_d;
  p.groups = hist_groups(cells);
  p.lds_bytes = (size_t)bins * 8;
  p.bytes = (size_t)nsig * p.groups * 8;
  return p;
}

// k_duet_peaks smooths between two planes per signal in the workspace.
GLOWK_DUET_HD size_t peaks_bytes(int nsig, int n_a, int n_d) { return (size_t)nsig * 2 * n_a * n_d * 8; }

// k_duet_assign reads one entry of four doubles per (signal, source, row): a cos, -a sin, 1 / (1 + a^2), 0.
GLOWK_DUET_HD size_t assign_bytes(int nsig, int num_sources, int rows) { return (size_t)nsig * num_sources * rows * 32; }

// The peaks of one plane on the host, as k_duet_peaks finds them: smooth passes between plane and tmp (both bins cells, plane is
// overwritten with the smoothed plane), then num_sources picks.  Returns n_found; peaks[2 k], peaks[2 k + 1] = (i, j) or -1.
inline int pick_peaks_host(int64_t* plane, int64_t* tmp, int n_a, int n_d, int smooth, int num_sources, int dist_a, int dist_d, int32_t* peaks) {
  const int bins = n_a * n_d;
  for (int pass = 0; pass < smooth; ++pass) {
    for (int c = 0; c < bins; ++c) tmp[c] = tap121(plane, c, c % n_d, n_d, 1);
    for (int c = 0; c < bins; ++c) plane[c] = tap121(tmp, c, c / n_d, n_a, n_d);
  }
  int found = 0;
  for (int k = 0; k < 2 * num_sources; ++k) peaks[k] = -1;
  for (; found < num_sources; ++found) {
    int64_t best = 0;
    int at = -1;
    for (int c = 0; c < bins; ++c) {
      bool ex = false;
      for (int k = 0; k < found && !ex; ++k) ex = excluded_by(c / n_d, c % n_d, peaks[2 * k], peaks[2 * k + 1], dist_a, dist_d);
      if (!ex && plane[c] > best) best = plane[c], at = c;
    }
    if (at < 0) break;
    peaks[2 * found] = at / n_d;
    peaks[2 * found + 1] = at % n_d;
  }
  return found;
}

}  // namespace glowk_duet
