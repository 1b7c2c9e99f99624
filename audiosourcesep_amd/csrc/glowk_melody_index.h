// glowk: the host-side rules of the melody kernels (glowk_melody.h), in plain C++ so that a host program can run them without HIP
// (tests/melody_index_sanitize_main.cpp sweeps them under AddressSanitizer + UBSan against straightforward loops): the table of
// interpolation positions, which is IEEE fp64 on the host whatever the device's division does, and every launch-geometry rule.  The
// kernels and the entry points call the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define GLOWK_MELODY_HD __host__ __device__ inline
#else
#define GLOWK_MELODY_HD inline
#endif

namespace glowk_melody {

constexpr int MAX_SIG = 65535, MIN_ROWS = 2, MAX_ROWS = 4096, MAX_FRAMES = 32768, MAX_BINS = 1024, MAX_HARM = 32, MAX_JUMP = 1023,
              MAX_MASK_HARM = 1024;
constexpr int64_t MAX_ELEMENTS = 2147483647;
constexpr double FLOOR = 0x1p-40;           // the least divisor of the emission

// ---- the position table ------------------------------------------------------------------------------------------------------------
// f0 [B] strictly ascending, positive and finite; bin_hz positive and finite.
inline bool grid_ok(const double* f0, int B, double bin_hz) {
  if (!(std::isfinite(bin_hz) && bin_hz > 0)) return false;
  for (int b = 0; b < B; ++b) {
    if (!(std::isfinite(f0[b]) && f0[b] > 0)) return false;
    if (b && !(f0[b] > f0[b - 1])) return false;
  }
  return true;
}

// Term (b, h), h = 1 .. H: p = h f0_b / bin_hz, i = floor(p), a = p - i; live iff i + 1 <= rows - 1.  idx [B][H] holds i, or -1 for a
// dead term; frac [B][H] holds a (0 for a dead term).
inline void positions(const double* f0, int B, int H, double bin_hz, int rows, int32_t* idx, double* frac) {
  for (int b = 0; b < B; ++b)
    for (int h = 1; h <= H; ++h) {
      const double p = (double)h * f0[b] / bin_hz;
      const double fl = std::floor(p);
      const size_t o = (size_t)b * H + (h - 1);
      if (fl + 1.0 <= (double)(rows - 1)) {
        idx[o] = (int32_t)fl;
        frac[o] = p - fl;
      } else {
        idx[o] = -1;
        frac[o] = 0.0;
      }
    }
}

// ---- salience: a thread per (bin, frame) --------------------------------------------------------------------------------------------
constexpr int SAL_THREADS = 256;
// workgroups per signal
GLOWK_MELODY_HD int sal_blocks(int B, int frames) { return (int)(((int64_t)B * frames + SAL_THREADS - 1) / SAL_THREADS); }

// ---- emission: the plane's maximum in `groups` partial maxima, then the division -----------------------------------------------------
constexpr int EMI_THREADS = 256, EMI_MAX_GROUPS = 256, EMI_MIN_CELLS = 4096, EMI_PER_THREAD = 4;
GLOWK_MELODY_HD int emi_groups(int64_t cells) {
  const int64_t g = (cells + EMI_MIN_CELLS - 1) / EMI_MIN_CELLS;
  return g > EMI_MAX_GROUPS ? EMI_MAX_GROUPS : (int)g;
}
// the cells [c0, c1) of group g (never empty)
GLOWK_MELODY_HD void emi_chunk(int64_t cells, int g, int64_t& c0, int64_t& c1) {
  const int groups = emi_groups(cells);
  const int64_t per = (cells + groups - 1) / groups;
  c0 = per * g;
  c1 = c0 + per < cells ? c0 + per : cells;
}
// workgroups of the division per signal
GLOWK_MELODY_HD int emi_blocks(int64_t cells) {
  const int64_t per = (int64_t)EMI_THREADS * EMI_PER_THREAD;
  return (int)((cells + per - 1) / per);
}
GLOWK_MELODY_HD size_t emi_work_bytes(int nsig, int B, int frames) {
  const size_t n = (size_t)nsig * emi_groups((int64_t)B * frames) * 4;
  return (n + 7) / 8 * 8;
}

// ---- track: one workgroup per signal, thread b <-> state b ---------------------------------------------------------------------------
constexpr int TRK_MAX_THREADS = 1024;
constexpr int TRK_CHUNK = 18432;            // back pointers (uint16) of the frames one back-trace chunk holds in LDS
// threads: the B + 1 states rounded up to whole waves, at most 1024
GLOWK_MELODY_HD int trk_threads(int B) {
  const int t = (B + 1 + 63) / 64 * 64;
  return t > TRK_MAX_THREADS ? TRK_MAX_THREADS : t;
}
// the thread that owns the unvoiced state: thread B, or thread 0 (beside its bin) when all 1024 threads own a bin
GLOWK_MELODY_HD int trk_unvoiced_thread(int B) { return B < trk_threads(B) ? B : 0; }
// frames of back pointers per back-trace chunk
GLOWK_MELODY_HD int trk_chunk_frames(int B) { return TRK_CHUNK / (B + 1); }
// back pointers [frames][B + 1] uint16 per signal, rounded up to 8 bytes
GLOWK_MELODY_HD size_t trk_bp_bytes(int B, int frames) { return ((size_t)frames * (B + 1) * 2 + 7) / 8 * 8; }
GLOWK_MELODY_HD size_t trk_work_bytes(int nsig, int B, int frames) { return (size_t)nsig * trk_bp_bytes(B, frames); }

// ---- mask -----------------------------------------------------------------------------------------------------------------------------
constexpr int MSK_THREADS = 256;
GLOWK_MELODY_HD int msk_blocks(int rows, int frames) { return (int)(((int64_t)rows * frames + MSK_THREADS - 1) / MSK_THREADS); }

// ---- the fused call's workspace: emission (float64), salience (float32), the partial maxima, the back pointers -------------------------
struct FitPlan {
  size_t sal, emi, part, bp, bytes;         // byte offsets, and the total
};
GLOWK_MELODY_HD FitPlan fit_plan(int nsig, int B, int frames) {
  FitPlan p;
  const size_t cells = (size_t)nsig * B * frames;
  p.emi = 0;                                             // the doubles first: every part stays 8-byte aligned
  p.sal = p.emi + cells * 8;
  p.part = p.sal + (cells * 4 + 7) / 8 * 8;
  p.bp = p.part + emi_work_bytes(nsig, B, frames);
  p.bytes = p.bp + trk_work_bytes(nsig, B, frames);
  return p;
}

// the ranges of include/glowk.h; 0 when all hold
GLOWK_MELODY_HD bool sizes_ok(int nsig, int rows, int frames, int B) {
  if (nsig < 0 || nsig > MAX_SIG || rows < MIN_ROWS || rows > MAX_ROWS || frames < 1 || frames > MAX_FRAMES || B < 1 || B > MAX_BINS) return false;
  if ((int64_t)nsig * rows * frames > MAX_ELEMENTS) return false;
  if ((int64_t)nsig * (B + 1) * frames > MAX_ELEMENTS) return false;
  return true;
}

}  // namespace glowk_melody
