// glowk: the host-side rules of the WPE kernels (glowk_wpe.h), in plain C++ so that a host program can run them without HIP
// (tests/wpe_index_sanitize_main.cpp sweeps them under AddressSanitizer + UBSan against straightforward loops): the ranges, the stacked
// past and its halo, the frame chunks staged in LDS, the matrix-core tiles of one triangle and their waves, the packed triangle of the
// solver, the grids and the workspace.  The kernels and the entry points call the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GLOWK_WPE_HD __host__ __device__ inline
#else
#define GLOWK_WPE_HD inline
#endif

namespace glowk_wpe {

constexpr int MAX_SIG = 65535, MAX_ROWS = 4096, MAX_FRAMES = 32768, MAX_ITER = 1000;
constexpr int MAX_M = 4, MAX_K = 32, MAX_D = 64, MAX_DELAY = 16, MAX_CONTEXT = 8;
constexpr int64_t MAX_ELEMENTS = 2147483647;
constexpr int STATUS_OK = 0, STATUS_PIVOT = 1;        // the row's status word: a pivot of the Cholesky factor was not finite or not > 0

GLOWK_WPE_HD bool model_ok(int M, int K, int delay) {
  return M >= 1 && M <= MAX_M && K >= 1 && K <= MAX_K && M * K <= MAX_D && delay >= 1 && delay <= MAX_DELAY;
}
GLOWK_WPE_HD bool sizes_ok(int nsig, int M, int rows, int frames) {
  if (nsig < 0 || nsig > MAX_SIG || M < 1 || M > MAX_M || rows < 1 || rows > MAX_ROWS || frames < 1 || frames > MAX_FRAMES) return false;
  return (int64_t)nsig * M * rows * frames <= MAX_ELEMENTS;
}

// ---- the stacked past ------------------------------------------------------------------------------------------------------------------
// z(t) = [x~(t); x(t)] has E = D + M complex elements: element e < D = M K is x_m(t - delay - k) with k = e / M, m = e % M; element D + m
// is x_m(t).  shift_of(e) is how many frames back element e reads; the longest is the halo delay + K - 1.
GLOWK_WPE_HD int stacked(int M, int K) { return M * K; }
GLOWK_WPE_HD int elements(int M, int K) { return M * K + M; }
GLOWK_WPE_HD int channel_of(int e, int M, int K) { return e < M * K ? e % M : e - M * K; }
GLOWK_WPE_HD int shift_of(int e, int M, int K, int delay) { return e < M * K ? delay + e / M : 0; }
GLOWK_WPE_HD int halo(int K, int delay) { return delay + K - 1; }
constexpr int MAX_HALO = MAX_DELAY + MAX_K - 1;

// ---- the frame chunks --------------------------------------------------------------------------------------------------------------------
// A workgroup of THREADS threads stages CHUNK frames of the row's M channels plus the halo before them as doubles (real and imaginary
// planes) in LDS; every tap is a shifted read.  Frame t of chunk c sits at column t - c CHUNK + halo; columns of frames below 0 or from
// `frames` on hold zeros.  The chunks are walked in ascending order: the order of every sum is fixed by `frames` alone.
constexpr int THREADS = 256, WAVE = 64, WAVES = THREADS / WAVE, CHUNK = 256, MFMA_FRAMES = 4;
GLOWK_WPE_HD int frame_chunks(int frames) { return (frames + CHUNK - 1) / CHUNK; }
GLOWK_WPE_HD int staged_cols(int K, int delay) { return CHUNK + halo(K, delay); }
// the frame that column j of chunk c0's staging holds, or -1 for a column of zeros; the column of the chunk's frame number `col` less `shift`
GLOWK_WPE_HD int stage_frame(int c0, int H, int j, int frames) {
  const int t = c0 - H + j;
  return t >= 0 && t < frames ? t : -1;
}
GLOWK_WPE_HD int stage_col(int col, int H, int shift) { return col + H - shift; }
// the steps of four frames a chunk's matrix-core loop takes
GLOWK_WPE_HD int chunk_steps(int c0, int frames) {
  const int live = frames - c0 < CHUNK ? frames - c0 : CHUNK;
  return (live + MFMA_FRAMES - 1) / MFMA_FRAMES;
}
constexpr int MAX_COLS = CHUNK + MAX_HALO;
// the staging of the correlations and of the filter: the planes [2][M][cols] and the weights of the chunk
GLOWK_WPE_HD size_t stage_bytes(int M, int K, int delay) { return ((size_t)2 * M * staged_cols(K, delay) + CHUNK) * 8; }
constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr size_t STAGE_BYTES_MAX = ((size_t)2 * MAX_M * MAX_COLS + CHUNK) * 8;                 // what the kernels declare
constexpr size_t FILTER_BYTES_MAX = (size_t)2 * MAX_M * MAX_COLS * 8 + (size_t)MAX_D * MAX_M * 16;

// ---- the matrix-core tiles -------------------------------------------------------------------------------------------------------------
// C = sum_t w z z^H restricted to its first D rows is R (columns < D) and P (columns D .. E - 1).  It is cut into 16 x 16 tiles (I, J);
// only the tiles J >= I are computed, I < tiles(D), J < tiles(E): pair p counts them row by row.  Wave v of the workgroup owns the pairs
// v, v + WAVES, ..., at most PAIRS_PER_WAVE of them.  A tile is four accumulators (the real Gram sums of a a^T, b b^T, b a^T and a b^T)
// and four v_mfma_f64_16x16x4_f64 per four frames.  Of a diagonal tile only the elements i <= j are used; R[j][i] is stored as the
// conjugate of R[i][j], bit for bit.
constexpr int TILE = 16, MAX_ROW_TILES = MAX_D / TILE, MAX_COL_TILES = (MAX_D + MAX_M + TILE - 1) / TILE;
constexpr int MAX_PAIRS = 14, PAIRS_PER_WAVE = (MAX_PAIRS + WAVES - 1) / WAVES;
GLOWK_WPE_HD int tiles(int n) { return (n + TILE - 1) / TILE; }
GLOWK_WPE_HD int pairs(int M, int K) {
  const int rt = tiles(stacked(M, K)), ct = tiles(elements(M, K));
  int n = 0;
  for (int I = 0; I < rt; ++I) n += ct - I;
  return n;
}
GLOWK_WPE_HD void pair_of(int M, int K, int p, int& I, int& J) {
  const int ct = tiles(elements(M, K));
  I = 0;
  while (p >= ct - I) {
    p -= ct - I;
    ++I;
  }
  J = I + p;
}
// The element a lane holds in result register r of tile pair (I, J), and where it goes: STORE_NONE (padding, or the lower part of a
// diagonal tile), STORE_UPPER (R[i][j] and, conjugated, R[j][i]), STORE_DIAG (R[i][i], imaginary part 0) or STORE_P (P[i][j - D]).
constexpr int STORE_NONE = 0, STORE_UPPER = 1, STORE_DIAG = 2, STORE_P = 3;
GLOWK_WPE_HD int lane_row(int I, int lane, int r) { return I * TILE + (lane >> 4) + 4 * r; }
GLOWK_WPE_HD int lane_col(int J, int lane) { return J * TILE + (lane & 15); }
GLOWK_WPE_HD int store_target(int i, int j, int D, int E) {
  if (i >= D || j >= E) return STORE_NONE;
  if (j >= D) return STORE_P;
  return i < j ? STORE_UPPER : i == j ? STORE_DIAG : STORE_NONE;
}
// where a lane's row of A or column of B (element e) starts in a staged plane of MAX_COLS columns a channel
GLOWK_WPE_HD int lane_offset(int e, int M, int K, int delay) { return channel_of(e, M, K) * MAX_COLS + stage_col(0, halo(K, delay), shift_of(e, M, K, delay)); }
// the longest chain of additions behind one real Gram sum: one accumulator from 0.0, four products per instruction, one instruction per
// four frames; a component of R or P is the sum or the difference of two of them
GLOWK_WPE_HD int64_t chain(int frames) { return (int64_t)MFMA_FRAMES * ((frames + MFMA_FRAMES - 1) / MFMA_FRAMES); }

// ---- the solver ------------------------------------------------------------------------------------------------------------------------
// One wave per row: the lower triangle of the loaded R, then of L, packed row by row in LDS (i >= j at tri(i, j)), the right-hand sides
// beside it.
constexpr int SOLVE_THREADS = 64;
GLOWK_WPE_HD int tri(int i, int j) { return i * (i + 1) / 2 + j; }
constexpr int TRI_MAX = MAX_D * (MAX_D + 1) / 2;
GLOWK_WPE_HD size_t solve_bytes(int D, int M) { return ((size_t)D * (D + 1) / 2 + (size_t)D * M) * 16; }
constexpr size_t SOLVE_BYTES_MAX = ((size_t)TRI_MAX + (size_t)MAX_D * MAX_M) * 16;

// ---- the grids -------------------------------------------------------------------------------------------------------------------------
GLOWK_WPE_HD int64_t row_grid(int nsig, int rows) { return (int64_t)nsig * rows; }                                   // power, correlations, solve
GLOWK_WPE_HD int64_t filter_grid(int nsig, int rows, int frames) { return (int64_t)nsig * rows * frame_chunks(frames); }

// ---- the sizes and the workspace -------------------------------------------------------------------------------------------------------
// w [nsig][rows][frames] doubles; R [nsig][rows][D][D], P and G [nsig][rows][D][M] complex128.  glowk_wpe_fit's workspace is w, R, P.
GLOWK_WPE_HD size_t w_bytes(int nsig, int rows, int frames) { return (size_t)nsig * rows * frames * 8; }
GLOWK_WPE_HD size_t r_bytes(int nsig, int rows, int D) { return (size_t)nsig * rows * D * D * 16; }
GLOWK_WPE_HD size_t p_bytes(int nsig, int rows, int D, int M) { return (size_t)nsig * rows * D * M * 16; }
GLOWK_WPE_HD size_t x_bytes(int nsig, int M, int rows, int frames) { return (size_t)nsig * M * rows * frames * 8; }
GLOWK_WPE_HD size_t work_bytes(int nsig, int M, int K, int rows, int frames) {
  const int D = stacked(M, K);
  return w_bytes(nsig, rows, frames) + r_bytes(nsig, rows, D) + p_bytes(nsig, rows, D, M);
}

}  // namespace glowk_wpe
