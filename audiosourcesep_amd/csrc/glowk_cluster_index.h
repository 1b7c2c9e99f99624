// glowk: the host-side rules of the clustering kernels (glowk_cluster.h), in plain C++ so that a host program can run them without HIP
// (tests/cluster_index_sanitize_main.cpp sweeps them under AddressSanitizer + UBSan against straightforward loops): the columns of the
// moment matrix, the workgroups of a signal and their chunks of cells, the longest addition chain behind one statistic, the layout of
// the per-signal constants and the workspace.  The kernels and the entry points call the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GLOWK_CLUSTER_HD __host__ __device__ inline
#else
#define GLOWK_CLUSTER_HD inline
#endif

namespace glowk_cluster {

constexpr int MAX_SIG = 65535, MAX_ROWS = 4096, MAX_FRAMES = 32768, MAX_ITER = 100000;
constexpr int MAX_D = 8, MAX_J = 8;
constexpr int64_t MAX_ELEMENTS = 2147483647;
constexpr double DEAD = 0x1p-40, MIN_REG = 0x1p-40;
enum { STATUS_ZERO_WEIGHT = 1, STATUS_DEAD = 2, STATUS_CHOLESKY = 4 };

// ---- the moment matrix -------------------------------------------------------------------------------------------------------------------
// Phi of a cell has P = 1 + D + D (D + 1) / 2 + 1 columns: 1, u_0 .. u_{D-1}, u_a u_b for a <= b (a ascending, then b), lse.  The
// statistics of cluster j are row j of R^T Phi with R[cell][j] = w r_j: N_j, a_j and the upper triangle of B_j.  J is padded to the 16
// rows of the A operand of v_mfma_f64_16x16x4_f64; row LL_ROW = 8 of the padding holds w itself, so that its last column is LL = sum w
// lse (the rest of that row and the last column of the cluster rows are not stored).  P is padded to tiles(D) column tiles of 16; four
// cells per instruction.  A signal's statistics are [J][P - 1] doubles, then LL.
constexpr int TILE = 16, MFMA_CELLS = 4, MAX_TILES = 3, LL_ROW = 8;
GLOWK_CLUSTER_HD constexpr int tri(int D) { return D * (D + 1) / 2; }
GLOWK_CLUSTER_HD constexpr int columns(int D) { return 1 + D + tri(D) + 1; }
GLOWK_CLUSTER_HD constexpr int tiles(int D) { return (columns(D) + TILE - 1) / TILE; }
GLOWK_CLUSTER_HD constexpr int col_n() { return 0; }
GLOWK_CLUSTER_HD constexpr int col_a(int d) { return 1 + d; }
// the column of u_a u_b, a <= b < D
GLOWK_CLUSTER_HD constexpr int col_b(int D, int a, int b) { return 1 + D + a * D - a * (a - 1) / 2 + (b - a); }
GLOWK_CLUSTER_HD constexpr int col_ll(int D) { return columns(D) - 1; }

// ---- the workgroups of a signal ----------------------------------------------------------------------------------------------------------
// A workgroup of THREADS threads (WAVES waves of 64) owns a contiguous chunk of the signal's rows * frames cells, a multiple of THREADS
// long but for the last, and walks it in steps of THREADS cells: thread t of step s has cell c0 + s THREADS + t.  Both the number of
// workgroups and the chunk are functions of the cell count alone, so no sum depends on nsig, D or J.  (PROJET's partition.)
constexpr int THREADS = 256, WAVE = 64, WAVES = THREADS / WAVE, MAX_GROUPS = 1024;
GLOWK_CLUSTER_HD int64_t chunk_cells(int64_t cells) {
  int64_t g = (cells + THREADS - 1) / THREADS;
  if (g > MAX_GROUPS) g = MAX_GROUPS;
  if (g < 1) g = 1;
  const int64_t per = (cells + g - 1) / g;
  return (per + THREADS - 1) / THREADS * THREADS;
}
GLOWK_CLUSTER_HD int groups(int64_t cells) {
  const int64_t per = chunk_cells(cells);
  const int64_t g = (cells + per - 1) / per;
  return g < 1 ? 1 : (int)g;
}
GLOWK_CLUSTER_HD int chunk_steps(int64_t cells) { return (int)(chunk_cells(cells) / THREADS); }
GLOWK_CLUSTER_HD void chunk_of(int64_t cells, int g, int64_t& c0, int64_t& c1) {
  const int64_t per = chunk_cells(cells);
  c0 = per * g;
  if (c0 > cells) c0 = cells;
  c1 = c0 + per < cells ? c0 + per : cells;
}

// ---- the order of the sums ---------------------------------------------------------------------------------------------------------------
// One statistic: every wave adds its 64 cells of a step with 16 matrix-core instructions of four products each, step after step, into
// one accumulator that starts at 0.0; the workgroup adds its four waves in ascending order; the per-signal kernel adds the workgroups'
// partials in ascending order from 0.0.  The longest chain of additions:
GLOWK_CLUSTER_HD int64_t chain(int rows, int frames) {
  const int64_t cells = (int64_t)rows * frames;
  return (int64_t)chunk_steps(cells) * WAVE + WAVES + groups(cells);
}

// ---- the constants of a signal -----------------------------------------------------------------------------------------------------------
// What the statistics and posterior passes read, written by the per-signal kernels: the origin o [D], then per cluster k_j, mu_j [D]
// and Linv_j [D][D] (row-major, zeros above the diagonal).
GLOWK_CLUSTER_HD constexpr int cons_cluster(int D) { return 1 + D + D * D; }
GLOWK_CLUSTER_HD constexpr int cons_doubles(int D, int J) { return D + J * cons_cluster(D); }

// ---- the workspace -----------------------------------------------------------------------------------------------------------------------
// [nsig][groups][J (P - 1) + 1] partial statistics, [nsig][J (P - 1) + 1] statistics, [nsig][cons] constants, [nsig][2] loop state (the previous ll and the
// stop flag), all doubles.
GLOWK_CLUSTER_HD constexpr int stat_cluster(int D) { return columns(D) - 1; }
GLOWK_CLUSTER_HD size_t partial_doubles(int D, int J) { return (size_t)J * stat_cluster(D) + 1; }
GLOWK_CLUSTER_HD size_t work_partials(int nsig, int D, int J, int rows, int frames) {
  return (size_t)nsig * groups((int64_t)rows * frames) * partial_doubles(D, J);
}
GLOWK_CLUSTER_HD size_t work_bytes(int nsig, int D, int J, int rows, int frames) {
  return (work_partials(nsig, D, J, rows, frames) + (size_t)nsig * (partial_doubles(D, J) + cons_doubles(D, J) + 2)) * 8;
}

// the ranges of include/glowk.h
GLOWK_CLUSTER_HD bool sizes_ok(int nsig, int D, int J, int rows, int frames) {
  if (nsig < 0 || nsig > MAX_SIG || rows < 1 || rows > MAX_ROWS || frames < 1 || frames > MAX_FRAMES) return false;
  if (D < 1 || D > MAX_D || J < 1 || J > MAX_J) return false;
  const int m = D > J ? D : J;
  return (int64_t)nsig * m * rows * frames <= MAX_ELEMENTS;
}

}  // namespace glowk_cluster
