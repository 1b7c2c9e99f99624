// glowk: the host-side rules of the kernel-additive-modelling kernels (glowk_kam.h), in plain C++ so that a host program can run them
// without HIP (tests/kam_index_sanitize_main.cpp sweeps them under AddressSanitizer + UBSan against straightforward loops): the ranges
// of include/glowk.h, the offset table as the kernel receives it, the waves of a workgroup and its LDS, the unit (one wave: 64 frames of
// one row) a wave owns, the neighbour test and the workspace.  The kernels and the entry points call the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GLOWK_KAM_HD __host__ __device__ inline
#else
#define GLOWK_KAM_HD inline
#endif

namespace glowk_kam {

constexpr int MAX_SIG = 65535, MAX_ROWS = 4096, MAX_FRAMES = 32768, MAX_J = 8, MAX_ITER = 100;
constexpr int MAX_N = 127, MAX_DROW = 4095, MAX_DFRAME = 32767;
constexpr int64_t MAX_ELEMENTS = 2147483647;

// ---- the offset table ------------------------------------------------------------------------------------------------------------------
// n pairs (d_row, d_frame) as int16, passed to the kernel by value in its launch arguments.  The kernel walks the table eight entries at
// a time and reads whole groups, so the array is padded to a multiple of eight past MAX_N; the padding is zero and never used as a
// neighbour (entry e counts only for e < n).
constexpr int TABLE_STEP = 8, TABLE_ENTRIES = (MAX_N + TABLE_STEP - 1) / TABLE_STEP * TABLE_STEP;
struct Table {
  int16_t d[TABLE_ENTRIES][2];
};
GLOWK_KAM_HD bool offsets_ok(const int32_t* offsets, int n) {
  if (n < 1 || n > MAX_N || !offsets) return false;
  for (int e = 0; e < n; ++e) {
    const int32_t dr = offsets[2 * e], df = offsets[2 * e + 1];
    if (dr < -MAX_DROW || dr > MAX_DROW || df < -MAX_DFRAME || df > MAX_DFRAME) return false;
  }
  return true;
}
// needs offsets_ok
inline Table pack(const int32_t* offsets, int n) {
  Table t = {};
  for (int e = 0; e < n; ++e) {
    t.d[e][0] = (int16_t)offsets[2 * e];
    t.d[e][1] = (int16_t)offsets[2 * e + 1];
  }
  return t;
}
// the last group of eight the kernel reads ends inside the table
GLOWK_KAM_HD constexpr int table_reads(int n) { return (n + TABLE_STEP - 1) / TABLE_STEP * TABLE_STEP; }

// ---- the ranges of include/glowk.h --------------------------------------------------------------------------------------------------------
GLOWK_KAM_HD bool sizes_ok(int nsig, int rows, int frames, int J) {
  if (nsig < 0 || nsig > MAX_SIG || rows < 1 || rows > MAX_ROWS || frames < 1 || frames > MAX_FRAMES || J < 1 || J > MAX_J) return false;
  return (int64_t)nsig * J * rows * frames <= MAX_ELEMENTS;
}

// ---- the neighbours of a cell ---------------------------------------------------------------------------------------------------------------
// (r + d_row, t + d_frame) where it lies inside the plane; any other is skipped and never read
GLOWK_KAM_HD bool neighbour(int r, int t, int d_row, int d_frame, int rows, int frames) {
  const int rr = r + d_row, tt = t + d_frame;
  return rr >= 0 && rr < rows && tt >= 0 && tt < frames;
}
// the two sorted positions the median of m >= 1 values reads: both m / 2 for odd m, m / 2 - 1 and m / 2 for even m
GLOWK_KAM_HD constexpr int pos_low(int m) { return (m - 1) >> 1; }
GLOWK_KAM_HD constexpr int pos_high(int m) { return m >> 1; }

// ---- the launch ---------------------------------------------------------------------------------------------------------------------------
// A wave owns one unit: TILE_F consecutive frames of one row of one signal, and an LDS slab [n][TILE_F] floats, 256 n bytes.  A workgroup is
// MAX_WAVES waves where that many slabs fit the LDS_LIMIT a workgroup gets without opt-in (n <= 64), else one wave: the slabs, not the
// registers, bound how many waves a compute unit holds, and single-wave workgroups pack its LDS best (five slabs of n = 127 against two
// workgroups of two).  A function of n alone, so nsig never changes which wave computes a cell (it could not change the result either:
// a unit depends on nothing outside its signal).  Units are numbered frames fastest: unit = (signal rows + row) ftiles + frame tile.
// candidates(n): how many candidates share each read of a lane's column in the selection (the kernel's template argument).
constexpr int TILE_F = 64, MAX_WAVES = 4, LDS_LIMIT = 65536;
GLOWK_KAM_HD constexpr size_t slab_bytes(int n) { return (size_t)n * TILE_F * sizeof(float); }
GLOWK_KAM_HD constexpr int waves(int n) { return slab_bytes(n) * MAX_WAVES <= (size_t)LDS_LIMIT ? MAX_WAVES : 1; }
GLOWK_KAM_HD constexpr int candidates(int n) { return n > 28 ? 8 : 4; }
GLOWK_KAM_HD constexpr size_t lds_bytes(int n) { return slab_bytes(n) * waves(n); }
GLOWK_KAM_HD constexpr int ftiles(int frames) { return (frames + TILE_F - 1) / TILE_F; }
GLOWK_KAM_HD int64_t units(int nsig, int rows, int frames) { return (int64_t)nsig * rows * ftiles(frames); }       // <= nsig rows frames
GLOWK_KAM_HD int64_t blocks(int nsig, int rows, int frames, int n) { return (units(nsig, rows, frames) + waves(n) - 1) / waves(n); }
GLOWK_KAM_HD void unit_of(int64_t unit, int rows, int frames, int64_t& sig, int& row, int& f0) {
  const int ft = ftiles(frames);
  const int64_t line = unit / ft;
  f0 = (int)(unit % ft) * TILE_F;
  sig = line / rows;
  row = (int)(line % rows);
}

// ---- the workspace of glowk_kam_fit ---------------------------------------------------------------------------------------------------------
// The filtered estimates A [nsig][J][rows][frames] float32, rounded up to 8 bytes, then -- when a source has a frame-neighbour model --
// the workspace of glowk_nn_median for ONE signal (nn_bytes: glowk_nn_workspace_bytes(1, rows, frames, k), which does not depend on k):
// that filter runs signal by signal.
GLOWK_KAM_HD size_t round8(size_t b) { return (b + 7) / 8 * 8; }
GLOWK_KAM_HD size_t work_a_bytes(int nsig, int rows, int frames, int J) { return round8((size_t)nsig * J * rows * frames * sizeof(float)); }
GLOWK_KAM_HD size_t work_bytes(int nsig, int rows, int frames, int J, size_t nn_bytes) {
  return work_a_bytes(nsig, rows, frames, J) + round8(nn_bytes);
}

}  // namespace glowk_kam
