// glowk: the host-side rules of the PROJET kernels (glowk_projet.h), in plain C++ so that a host program can run them without HIP
// (tests/projet_index_sanitize_main.cpp sweeps them under AddressSanitizer + UBSan against straightforward loops): the padding of M,
// the workgroups of a signal and their chunks of cells, the longest addition chain behind one outer sum and the workspace.
// The kernels and the entry points call the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GLOWK_PROJET_HD __host__ __device__ inline
#else
#define GLOWK_PROJET_HD inline
#endif

namespace glowk_projet {

constexpr int MAX_SIG = 65535, MAX_ROWS = 4096, MAX_FRAMES = 32768, MAX_ITER = 100000;
constexpr int MIN_M = 2, MAX_M = 32, MAX_L = 128, MAX_J = 8;
constexpr int64_t MAX_ELEMENTS = 2147483647;
constexpr double FLOOR = 0x1p-40;

// ---- the matrix-core tiles -------------------------------------------------------------------------------------------------------------
// An and Ad are R^T P' with R [cells][M] and P' [cells][J].  One 16-row tile of the A operand holds TILE_M = 8 projections twice: rows
// 0 .. 7 their numerator weights V sigma^(beta - 2), rows 8 .. 15 their denominator weights sigma^(beta - 1), so that one instruction
// stream serves An and Ad and a lane computes V and sigma of a projection once.  M is padded to a multiple of 8 with all-zero rows (V = 0
// there: every term is an exact 0), J to 16 columns of zeros, four cells per v_mfma_f64_16x16x4_f64.
constexpr int TILE_ROWS = 16, TILE_M = TILE_ROWS / 2, TILE_J = 16, MFMA_CELLS = 4, MAX_TILES = MAX_M / TILE_M;
GLOWK_PROJET_HD int m_tiles(int M) { return (M + TILE_M - 1) / TILE_M; }
GLOWK_PROJET_HD int m_padded(int M) { return m_tiles(M) * TILE_M; }

// ---- the workgroups of a signal ----------------------------------------------------------------------------------------------------------
// A workgroup of THREADS threads (WAVES waves of 64) owns a contiguous chunk of the signal's rows * frames cells, a multiple of THREADS
// long but for the last, and walks it in steps of THREADS cells: thread t of step s has cell c0 + s THREADS + t.  Both the number of
// workgroups and the chunk are functions of the cell count alone, so no sum depends on nsig.
constexpr int THREADS = 256, WAVE = 64, WAVES = THREADS / WAVE, MAX_GROUPS = 1024;
GLOWK_PROJET_HD int64_t chunk_cells(int64_t cells) {
  int64_t g = (cells + THREADS - 1) / THREADS;
  if (g > MAX_GROUPS) g = MAX_GROUPS;
  if (g < 1) g = 1;
  const int64_t per = (cells + g - 1) / g;
  return (per + THREADS - 1) / THREADS * THREADS;
}
GLOWK_PROJET_HD int groups(int64_t cells) {
  const int64_t per = chunk_cells(cells);
  const int64_t g = (cells + per - 1) / per;
  return g < 1 ? 1 : (int)g;
}
GLOWK_PROJET_HD int chunk_steps(int64_t cells) { return (int)(chunk_cells(cells) / THREADS); }
GLOWK_PROJET_HD void chunk_of(int64_t cells, int g, int64_t& c0, int64_t& c1) {
  const int64_t per = chunk_cells(cells);
  c0 = per * g;
  if (c0 > cells) c0 = cells;
  c1 = c0 + per < cells ? c0 + per : cells;
}

// ---- the order of the outer sums ---------------------------------------------------------------------------------------------------------
// One element of An (or Ad): every wave adds its 64 cells of a step with 16 matrix-core instructions of four products each, step after
// step, into one accumulator that starts at 0.0; the workgroup adds its four waves in ascending order; the Q kernel adds the
// workgroups' partials in ascending order from 0.0.  The longest chain of additions behind one element:
GLOWK_PROJET_HD int64_t chain(int rows, int frames) {
  const int64_t cells = (int64_t)rows * frames;
  return (int64_t)chunk_steps(cells) * WAVE + WAVES + groups(cells);
}
// The divergence: a thread adds the M terms of its cell of every step in order, the workgroup's 256 sums go through a halving tree,
// the final kernel adds the partials in ascending order from 0.0: steps M + 8 + groups additions, never more than chain() for M <= 64.

// ---- the workspace -----------------------------------------------------------------------------------------------------------------------
// The partial outer sums [nsig][groups][2 (An, Ad)][M][J] doubles; the divergence's partials [nsig][groups] fit in the same bytes.
GLOWK_PROJET_HD size_t partial_doubles(int M, int J) { return (size_t)2 * M * J; }
GLOWK_PROJET_HD size_t work_bytes(int nsig, int M, int J, int rows, int frames) {
  return (size_t)nsig * groups((int64_t)rows * frames) * partial_doubles(M, J) * 8;
}

// the ranges of include/glowk.h
GLOWK_PROJET_HD bool sizes_ok(int nsig, int rows, int frames, int J) {
  if (nsig < 0 || nsig > MAX_SIG || rows < 1 || rows > MAX_ROWS || frames < 1 || frames > MAX_FRAMES || J < 1 || J > MAX_J) return false;
  return (int64_t)nsig * J * rows * frames <= MAX_ELEMENTS;
}
GLOWK_PROJET_HD bool model_ok(int M, int L, int J) { return M >= MIN_M && M <= MAX_M && L >= 1 && L <= MAX_L && J >= 1 && J <= MAX_J; }

}  // namespace glowk_projet
