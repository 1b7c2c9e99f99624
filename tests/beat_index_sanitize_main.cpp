// The integer rules of REPET's front end (audiosourcesep_amd/csrc/glowk_beat_index.h, the functions the kernels call) run on the host
// under -fsanitize=address,undefined (tests/test_repet_beat_cpu.py) against straightforward loops: the periodic neighbour list for
// every frames <= 70, p <= 80, k <= 12 into heap buffers of exactly k entries, the period of a frame, and the windows.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../audiosourcesep_amd/csrc/glowk_beat_index.h"

// the rule as the header states it: i = 0, -1, +1, -2, +2, ..; every frame in range is kept until k are kept
static std::vector<int32_t> list_by_loop(int j, int p, int frames, int k) {
  std::vector<int32_t> out;
  for (int i = 0; (int)out.size() < k && i <= frames; ++i) {
    for (int sign = -1; sign <= 1; sign += 2) {
      if (i == 0 && sign == 1) continue;
      const long f = (long)j + (long)sign * i * p;
      if (f >= 0 && f < frames && (int)out.size() < k) out.push_back((int32_t)f);
    }
  }
  out.resize(k, -1);
  return out;
}

int main() {
  long lists = 0;
  for (int frames = 1; frames <= 70; ++frames)
    for (int p = 1; p <= 80; ++p)
      for (int k = 1; k <= 12; ++k)
        for (int j = 0; j < frames; ++j) {
          int32_t* out = (int32_t*)std::malloc(sizeof(int32_t) * k);   // exactly k entries: one past the end is a heap overflow
          const int n = glowk_beat::period_list(j, p, frames, k, out);
          const std::vector<int32_t> want = list_by_loop(j, p, frames, k);
          int kept = 0;
          for (int t = 0; t < k; ++t) {
            if (out[t] != want[t]) {
              std::printf("period_list(j=%d, p=%d, frames=%d, k=%d)[%d] = %d, expected %d\n", j, p, frames, k, t, out[t], want[t]);
              return 1;
            }
            kept += want[t] >= 0;
          }
          std::free(out);
          if (n != kept) { std::printf("period_list returned %d, kept %d\n", n, kept); return 1; }
          ++lists;
        }
  // the largest period an int32 holds: only the frame itself
  {
    int32_t out[3];
    if (glowk_beat::period_list(69, INT32_MAX, 70, 3, out) != 1 || out[0] != 69 || out[1] != -1 || out[2] != -1) { std::printf("INT32_MAX\n"); return 1; }
  }
  // the period of a frame: entry min((j + step / 2) / step, nper - 1), at least 1
  for (int nper = 1; nper <= 9; ++nper)
    for (int step = 1; step <= 40; ++step) {
      std::vector<int32_t> per(nper);
      for (int w = 0; w < nper; ++w) per[w] = w % 3 == 2 ? -w : w;       // zeros and negatives count as 1
      for (int j = 0; j < 70; ++j) {
        int w = (j + step / 2) / step;
        if (w >= nper) w = nper - 1;
        const int want = per[w] < 1 ? 1 : per[w];
        if (glowk_beat::period_of(per.data(), nper, step, j) != want) { std::printf("period_of(nper=%d, step=%d, j=%d)\n", nper, step, j); return 1; }
      }
    }
  // the windows: frame f is in window t exactly if t step - win / 2 <= f < t step - win / 2 + win
  for (int frames = 2; frames <= 70; ++frames)
    for (int win = 2; win <= frames; ++win)
      for (int step = 1; step <= win; ++step)
        for (int t = 0; t * step < frames; ++t) {
          int first, n;
          glowk_beat::beat_window(t, win, step, frames, first, n);
          int lo = -1, cnt = 0;
          for (int f = 0; f < frames; ++f)
            if (f >= t * step - win / 2 && f < t * step - win / 2 + win) { if (lo < 0) lo = f; ++cnt; }
          if (cnt < 1 || first != lo || n != cnt) { std::printf("beat_window(t=%d, win=%d, step=%d, frames=%d)\n", t, win, step, frames); return 1; }
        }
  {
    int first, n;
    glowk_beat::beat_window(0, 0, 0, 32768, first, n);
    if (first != 0 || n != 32768) return 1;
    glowk_beat::beat_window(32767, 32768, 1, 32768, first, n);
    if (first != 16383 || n != 16385) return 1;
  }
  std::printf("BEAT_INDEX_SANITIZE_OK %ld lists\n", lists);
  return 0;
}
