// glowk: the plan rules of the NMF kernels (glowk_nmf.h), in plain C++ so that a host program can run them without HIP
// (tests/nmf_index_sanitize_main.cpp sweeps them under AddressSanitizer + UBSan against straightforward loops).  The kernels and
// the entry points call the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GLOWK_NMF_HD __host__ __device__ inline
#else
#define GLOWK_NMF_HD inline
#endif

namespace glowk_nmf {

constexpr int MAX_SIG = 65535, MAX_ROWS = 4096, MAX_FRAMES = 32768, MAX_K = 128, MAX_SRC = 16, MAX_ITER = 100000;
constexpr int TILE = 32;                    // one MFMA tile: rows of a row tile, frames of a frame tile
constexpr int WAVES = 4;                    // waves per workgroup; each walks every fourth tile
constexpr int TARGET_GROUPS = 256;          // workgroups per signal the W update's cut stays within (one per compute unit: at K > 32 a
                                            // compute unit holds one workgroup, and a 257th would run alone in a second round)

// How one signal is cut up; a function of (rows, frames, K) alone, never of nsig, so a batch adds in the order its signals do alone.
//   rtiles, ftiles  tiles of 32 rows and of 32 frames
//   kt              tiles of 32 components: K padded with exact zeros to 32 kt
//   nch, tpc        the W update and the divergence cut the frame tiles into nch chunks of tpc tiles (the last may be shorter, never
//                   empty): chunk ch holds the tiles [ch tpc, min((ch + 1) tpc, ftiles))
struct NmfPlan {
  int rtiles, ftiles, kt, nch, tpc;
};

GLOWK_NMF_HD NmfPlan nmf_plan(int rows, int frames, int K) {
  NmfPlan p;
  p.rtiles = (rows + TILE - 1) / TILE;
  p.ftiles = (frames + TILE - 1) / TILE;
  p.kt = (K + TILE - 1) / TILE;
  int want = TARGET_GROUPS / p.rtiles < 1 ? 1 : TARGET_GROUPS / p.rtiles;   // the most chunks that stay within the target
  const int most = p.ftiles / WAVES < 1 ? 1 : p.ftiles / WAVES;   // but every wave of a chunk should have a tile
  if (want > most) want = most;
  p.tpc = (p.ftiles + want - 1) / want;
  p.nch = (p.ftiles + p.tpc - 1) / p.tpc;
  return p;
}

// The frame tiles [t0, t1) of chunk ch.
GLOWK_NMF_HD void nmf_chunk(const NmfPlan& p, int ch, int& t0, int& t1) {
  t0 = ch * p.tpc;
  t1 = t0 + p.tpc < p.ftiles ? t0 + p.tpc : p.ftiles;
}

// The row of a 32 x 32 MFMA result that accumulator register r of lane half `half` holds (the column is lane & 31).
GLOWK_NMF_HD int nmf_rho(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// Floats of the W update's partial numerators and denominators, and doubles of the divergence's partial sums, per signal.
GLOWK_NMF_HD int64_t nmf_w_part_floats(const NmfPlan& p, int rows, int K) { return (int64_t)2 * p.nch * rows * K; }
GLOWK_NMF_HD int64_t nmf_div_parts(const NmfPlan& p) { return (int64_t)p.rtiles * p.nch; }

// The bytes of workspace glowk_nmf_fit and glowk_nmf_divergence need (the larger of the two uses).
GLOWK_NMF_HD size_t nmf_work_bytes(int nsig, int rows, int frames, int K) {
  const NmfPlan p = nmf_plan(rows, frames, K);
  const int64_t a = nmf_w_part_floats(p, rows, K) * 4, b = nmf_div_parts(p) * 8;
  return (size_t)nsig * (size_t)(a > b ? a : b);
}

// Offset of (chunk ch, which = 0 numerator / 1 denominator, row, k) in one signal's partial sums.
GLOWK_NMF_HD int64_t nmf_w_part_index(int ch, int which, int row, int k, int rows, int K) {
  return (((int64_t)ch * 2 + which) * rows + row) * K + k;
}

}  // namespace glowk_nmf
