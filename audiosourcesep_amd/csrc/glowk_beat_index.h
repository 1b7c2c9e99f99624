// glowk: the integer rules of REPET's front end (glowk_beat.h), in plain C++ so that a host program can run them without HIP
// (tests/beat_index_sanitize_main.cpp sweeps them under AddressSanitizer + UBSan against straightforward loops).  The kernels
// call the same functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GLOWK_HD __host__ __device__ inline
#else
#define GLOWK_HD inline
#endif

namespace glowk_beat {

// Window t of the beat spectrogram: frames [t step - win / 2, t step - win / 2 + win) cut to [0, frames); win = 0 is the one window
// [0, frames).  first: its first frame, n: its frame count (>= 1 for t step < frames, win >= 2).
GLOWK_HD void beat_window(int t, int win, int step, int frames, int& first, int& n) {
  if (win == 0) { first = 0; n = frames; return; }
  const int64_t lo = (int64_t)t * step - win / 2, hi = lo + win;
  first = (int)(lo < 0 ? 0 : lo);
  n = (int)(hi > frames ? frames : hi) - first;
}

// The period of frame j: max(1, period[min((j + step / 2) / step, nper - 1)]).
GLOWK_HD int period_of(const int32_t* period, int nper, int step, int j) {
  int w = (j + step / 2) / step;
  if (w > nper - 1) w = nper - 1;
  const int p = period[w];
  return p < 1 ? 1 : p;
}

// The list of frame j at period p >= 1: j + i p for i = 0, -1, +1, -2, +2, .. in that order, those in [0, frames) kept until k are
// kept, -1 after them.  out[0 .. k) is written, nothing else.  Returns the number kept.
GLOWK_HD int period_list(int j, int p, int frames, int k, int32_t* out) {
  int n = 0;
  if (k > 0) out[n++] = j;
  for (int64_t off = p; n < k; off += p) {                  // 64-bit: p may be any positive int32
    const int64_t lo = j - off, hi = j + off;
    if (lo < 0 && hi >= frames) break;                      // neither side has a frame left
    if (lo >= 0) out[n++] = (int32_t)lo;
    if (n < k && hi < frames) out[n++] = (int32_t)hi;
  }
  for (int t = n; t < k; ++t) out[t] = -1;
  return n;
}

}  // namespace glowk_beat
