// glowk: the integer rules of the 2-D DFT and the peak mask (glowk_dft2.h), in plain C++ so that a host program can run them without
// HIP (tests/dft2_index_sanitize_main.cpp sweeps them under AddressSanitizer + UBSan against straightforward loops).  The kernels
// and the entry points call the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GLOWK_DFT2_HD __host__ __device__ inline
#else
#define GLOWK_DFT2_HD inline
#endif

namespace glowk_dft2 {

constexpr int MAX_SIG = 65535, MAX_ROWS = 4096, MAX_FRAMES = 32768, MAX_NB = 127;
constexpr int TILE = 32;                    // one MFMA tile: 32 x 32 outputs per wave
constexpr int WAVES = 4;                    // waves per workgroup, side by side along the contiguous output axis
constexpr int NT_FWD = 2, NT_ROWS = 1, NT_INV = 4;   // output tiles per wave, side by side along that axis: k_rdft_frames, k_cdft_rows, k_irdft_frames
constexpr int LDS_TAB_MAX = 8192;           // a twiddle table of at most this many entries (64 KB) is staged in LDS
constexpr int PK_SEG = 256;                 // k_peak_cols: columns per workgroup
constexpr int PK_TR = 32, PK_TC = 32;       // k_peak_rows: the tile of one workgroup
constexpr int STD_MAX_BLOCKS = 256, STD_PER_BLOCK = 4096;

// The periodic map: i mod n in [0, n) for any int i (a neighbourhood longer than the axis wraps as often as it needs to).
GLOWK_DFT2_HD int wrap_index(int i, int n) {
  i %= n;
  return i < 0 ? i + n : i;
}

// The table index of the product a b: (a b) mod n for 0 <= a, b < 32768 (a b < 2^30: 32-bit arithmetic is enough), 1 <= n <= 32768.
GLOWK_DFT2_HD unsigned tw_index(unsigned a, unsigned b, unsigned n) { return (a * b) % n; }

// One step of the index along the summed axis: (idx + step) mod n for idx, step in [0, n), by one conditional subtraction.
GLOWK_DFT2_HD unsigned tw_step(unsigned idx, unsigned step, unsigned n) {
  idx += step;
  return idx >= n ? idx - n : idx;
}

// How the two GEMM stages are cut up: a function of the shapes alone.
struct Dft2Plan {
  int fc;                                   // frames / 2 + 1 half-spectrum columns
  int64_t m_frames;                         // nsig * rows: the rows of the stage along frames, signals batched
  int64_t fwd_frames_blocks, rows_blocks, inv_frames_blocks;
  size_t tab_t_off, tab_r_off, mid_off;     // byte offsets in the workspace: two tables of (cos, sin), the plane between the stages
  size_t bytes;
};
GLOWK_DFT2_HD int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }
GLOWK_DFT2_HD int64_t groups_of(int64_t n, int nt) { return ceil_div64(ceil_div64(n, TILE), WAVES * nt); }   // workgroups along an axis of n outputs
GLOWK_DFT2_HD Dft2Plan dft2_plan(int nsig, int rows, int frames) {
  Dft2Plan p;
  p.fc = frames / 2 + 1;
  p.m_frames = (int64_t)nsig * rows;
  p.fwd_frames_blocks = ceil_div64(p.m_frames, TILE) * groups_of(p.fc, NT_FWD);
  p.rows_blocks = (int64_t)nsig * ceil_div64(rows, TILE) * groups_of(p.fc, NT_ROWS);
  p.inv_frames_blocks = ceil_div64(p.m_frames, TILE) * groups_of(frames, NT_INV);
  p.tab_t_off = 0;
  p.tab_r_off = (size_t)frames * 8;
  p.mid_off = p.tab_r_off + (size_t)rows * 8;
  p.bytes = p.mid_off + (size_t)nsig * rows * p.fc * 8;
  return p;
}

// The workgroups per signal of k_plane_sum: a function of n alone, so a batch adds in the order its signals do alone.
GLOWK_DFT2_HD int std_blocks(int64_t n) {
  const int64_t b = ceil_div64(n, STD_PER_BLOCK);
  return (int)(b < 1 ? 1 : b > STD_MAX_BLOCKS ? STD_MAX_BLOCKS : b);
}
// The elements [first, first + count) of workgroup b of nb (count may be 0 for the last ones).
GLOWK_DFT2_HD void std_chunk(int64_t n, int nb, int b, int64_t& first, int64_t& count) {
  const int64_t per = ceil_div64(n, nb);
  first = per * b;
  if (first > n) first = n;
  count = n - first < per ? n - first : per;
}

}  // namespace glowk_dft2
