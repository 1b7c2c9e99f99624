// The host-side rules of the WPE kernels (audiosourcesep_amd/csrc/glowk_wpe_index.h) against straightforward loops, compiled without
// HIP under AddressSanitizer + UBSan (tests/test_wpe_cpu.py) and swept over the whole documented ranges of M, K, delay, frames, rows
// and nsig: the stacked past and the halo, the chunk plans and every LDS column a lane, a stager or a filter thread touches (in arrays
// of the size the kernels declare, so a stray index is a sanitizer report), the tile pairs and their waves (every element of R and P
// stored exactly once), the solver's packed triangle, the LDS bytes against the 160 KiB limit, the workspace and the grids.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../audiosourcesep_amd/csrc/glowk_wpe_index.h"

using namespace glowk_wpe;

static int fail(const char* what, long a, long b, long c) {
  std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

// the stacked past by its definition, and the reads of every lane of the correlations and of every thread of the filter
static int check_model(int M, int K, int delay) {
  const int D = stacked(M, K), E = elements(M, K), H = halo(K, delay);
  if (D != M * K || E != D + M || D > MAX_D || H != delay + K - 1 || H > MAX_HALO || staged_cols(K, delay) > MAX_COLS) return fail("sizes", M, K, delay);
  int longest = 0;
  for (int k = 0, e = 0; k < K; ++k)
    for (int m = 0; m < M; ++m, ++e) {
      if (channel_of(e, M, K) != m || shift_of(e, M, K, delay) != delay + k) return fail("element", M, K, e);
      if (delay + k > longest) longest = delay + k;
    }
  for (int m = 0; m < M; ++m)
    if (channel_of(D + m, M, K) != m || shift_of(D + m, M, K, delay) != 0) return fail("present element", M, K, m);
  if (longest != H) return fail("halo", M, K, delay);

  // the planes as the kernels declare them; a lane's offset plus any column of a chunk stays inside its channel's row
  std::vector<double> plane((size_t)MAX_M * MAX_COLS, 0.0);
  for (int e = 0; e < E; ++e) {
    const int off = lane_offset(e, M, K, delay);
    if (off != channel_of(e, M, K) * MAX_COLS + H - shift_of(e, M, K, delay)) return fail("lane offset", e, off, 0);
    for (int col = 0; col < CHUNK; ++col) {
      const int at = off + col;
      if (at < channel_of(e, M, K) * MAX_COLS || at >= channel_of(e, M, K) * MAX_COLS + staged_cols(K, delay)) return fail("lane read", e, col, at);
      plane[(size_t)at] += 1.0;
    }
  }
  // the filter: thread tid reads column tid + H - delay - k
  for (int tid = 0; tid < THREADS; ++tid)
    for (int k = 0; k < K; ++k) {
      const int col = stage_col(tid, H, delay + k);
      if (col != tid + H - delay - k) return fail("stage_col", tid, k, col);
      if (col < 0 || col >= staged_cols(K, delay)) return fail("filter read", tid, k, col);
      plane[(size_t)col] += 1.0;
    }

  // the tile pairs: the upper triangle of tiles, row by row, each once, each with one wave and one slot
  const int rt = tiles(D), ct = tiles(E), np = pairs(M, K);
  if (rt > MAX_ROW_TILES || ct > MAX_COL_TILES || np > MAX_PAIRS || np < 1) return fail("tiles", rt, ct, np);
  std::vector<int> seen((size_t)rt * ct, 0);
  int want = 0;
  for (int I = 0; I < rt; ++I)
    for (int J = I; J < ct; ++J) {
      int i2, j2;
      pair_of(M, K, want, i2, j2);
      if (i2 != I || j2 != J) return fail("pair_of", want, I, J);
      ++seen[(size_t)I * ct + J];
      ++want;
    }
  if (want != np) return fail("pairs", want, np, 0);
  std::vector<int> slots(WAVES, 0);
  for (int p = 0; p < np; ++p) ++slots[p % WAVES];
  for (int v = 0; v < WAVES; ++v)
    if (slots[v] > PAIRS_PER_WAVE) return fail("slots", v, slots[v], 0);

  // the stores of the correlations: every element of R [D][D] and P [D][M] exactly once, inside its array
  std::vector<int> r((size_t)D * D, 0), pm((size_t)D * M, 0);
  for (int p = 0; p < np; ++p) {
    int I, J;
    pair_of(M, K, p, I, J);
    for (int lane = 0; lane < WAVE; ++lane)
      for (int reg = 0; reg < 4; ++reg) {
        const int i = lane_row(I, lane, reg), j = lane_col(J, lane);
        if (i != I * TILE + (lane >> 4) + 4 * reg || j != J * TILE + (lane & 15)) return fail("lane element", lane, reg, i);
        switch (store_target(i, j, D, E)) {                                   // the kernel's own switch: the vectors are the arrays' sizes
          case STORE_UPPER:
            if (!(i < j && j < D)) return fail("upper target", i, j, D);
            ++r[(size_t)i * D + j];
            ++r[(size_t)j * D + i];
            break;
          case STORE_DIAG:
            if (!(i == j && i < D)) return fail("diag target", i, j, D);
            ++r[(size_t)i * D + i];
            break;
          case STORE_P:
            if (!(i < D && j >= D && j < E)) return fail("P target", i, j, D);
            ++pm[(size_t)i * M + (j - D)];
            break;
          default:
            if (i < D && j < E && !(j < D && i > j)) return fail("dropped element", i, j, D);
        }
      }
  }
  for (int v : r)
    if (v != 1) return fail("R stores", M, K, v);
  for (int v : pm)
    if (v != 1) return fail("P stores", M, K, v);

  // the solver's packed triangle: a bijection onto [0, D (D + 1) / 2)
  std::vector<int> t((size_t)D * (D + 1) / 2, 0);
  for (int i = 0; i < D; ++i)
    for (int j = 0; j <= i; ++j) {
      const int at = tri(i, j);
      if (at < 0 || at >= D * (D + 1) / 2 || at >= TRI_MAX) return fail("tri", i, j, at);
      ++t[(size_t)at];
    }
  for (int v : t)
    if (v != 1) return fail("tri twice", D, v, 0);

  if (stage_bytes(M, K, delay) > STAGE_BYTES_MAX || STAGE_BYTES_MAX > LDS_LIMIT || FILTER_BYTES_MAX + CHUNK * 8 > LDS_LIMIT || solve_bytes(D, M) > SOLVE_BYTES_MAX ||
      SOLVE_BYTES_MAX + 64 > LDS_LIMIT)
    return fail("lds", M, K, delay);
  return 0;
}

// the staging of every chunk of a row: every frame of the row staged where the lanes look for it, zeros elsewhere, nothing outside
static int check_frames(int frames, int K, int delay) {
  const int H = halo(K, delay), nch = frame_chunks(frames), cols = staged_cols(K, delay);
  if (nch < 1 || (int64_t)nch * CHUNK < frames || (int64_t)(nch - 1) * CHUNK >= frames) return fail("chunks", frames, nch, 0);
  std::vector<int> covered((size_t)frames, 0);
  std::vector<int> col_frame((size_t)MAX_COLS);
  int64_t products = 0;
  for (int c = 0; c < nch; ++c) {
    const int c0 = c * CHUNK;
    for (int j = 0; j < cols; ++j) {
      const int t = c0 - H + j;
      col_frame[(size_t)j] = stage_frame(c0, H, j, frames);
      if (col_frame[(size_t)j] != ((t >= 0 && t < frames) ? t : -1)) return fail("stage_frame", frames, c, j);
    }
    const int live = frames - c0 < CHUNK ? frames - c0 : CHUNK;
    if (live < 1) return fail("empty chunk", frames, c, 0);
    const int steps = chunk_steps(c0, frames);
    if (steps != (live + MFMA_FRAMES - 1) / MFMA_FRAMES) return fail("chunk steps", frames, c, steps);
    for (int s = 0; s < steps; ++s)
      for (int lk = 0; lk < MFMA_FRAMES; ++lk) {
        const int col = s * MFMA_FRAMES + lk;
        if (col >= CHUNK) return fail("step column", frames, c, col);
        const int t = col_frame[(size_t)stage_col(col, H, 0)];
        if (t >= 0) {
          if (t != c0 + col) return fail("frame of column", frames, c, col);
          ++covered[(size_t)t];
        }
        ++products;
      }
  }
  for (int v : covered)
    if (v != 1) return fail("frame coverage", frames, v, 0);
  if (products != chain(frames) || chain(frames) < frames || chain(frames) >= frames + MFMA_FRAMES) return fail("chain", frames, (long)products, (long)chain(frames));
  return 0;
}

static int check_sizes() {
  // the ranges and the products at their corners: nothing wraps in 64 bits, the grids fit 32
  const int nsigs[] = {0, 1, 2, 3, 7, 127, 512, 65535}, rowss[] = {1, 2, 5, 513, 1025, 4096}, framess[] = {1, 4, 203, 1029, 5626, 32768};
  for (int nsig : nsigs)
    for (int rows : rowss)
      for (int frames : framess)
        for (int M = 1; M <= MAX_M; ++M) {
          const bool ok = (int64_t)nsig * M * rows * frames <= MAX_ELEMENTS;
          if (sizes_ok(nsig, M, rows, frames) != ok) return fail("sizes_ok", nsig, rows, frames);
          if (!ok) continue;
          if (row_grid(nsig, rows) != (int64_t)nsig * rows || row_grid(nsig, rows) > 2147483647LL) return fail("row grid", nsig, rows, 0);
          if (filter_grid(nsig, rows, frames) != (int64_t)nsig * rows * frame_chunks(frames) || filter_grid(nsig, rows, frames) > 2147483647LL)
            return fail("filter grid", nsig, rows, frames);
          for (int K = 1; K <= MAX_K; K += (K < 4 ? 1 : 7)) {
            if (M * K > MAX_D) continue;
            const unsigned __int128 D = (unsigned)(M * K);
            const unsigned __int128 want = (unsigned __int128)nsig * rows * ((unsigned __int128)frames * 8 + D * D * 16 + D * M * 16);
            if (want >> 63) return fail("workspace range", nsig, rows, frames);
            if ((unsigned __int128)work_bytes(nsig, M, K, rows, frames) != want) return fail("workspace", nsig, rows, frames);
          }
        }
  if (sizes_ok(-1, 1, 1, 1) || sizes_ok(65536, 1, 1, 1) || sizes_ok(1, 0, 1, 1) || sizes_ok(1, 5, 1, 1) || sizes_ok(1, 1, 0, 1) || sizes_ok(1, 1, 4097, 1) ||
      sizes_ok(1, 1, 1, 0) || sizes_ok(1, 1, 1, 32769) || sizes_ok(65535, 4, 4096, 32768))
    return fail("sizes_ok refusals", 0, 0, 0);
  if (model_ok(0, 1, 1) || model_ok(5, 1, 1) || model_ok(1, 0, 1) || model_ok(1, 33, 1) || model_ok(3, 22, 1) || model_ok(1, 1, 0) || model_ok(1, 1, 17) ||
      !model_ok(1, 32, 16) || !model_ok(4, 16, 1) || !model_ok(2, 32, 16) || !model_ok(3, 21, 3))
    return fail("model_ok", 0, 0, 0);
  return THREADS == WAVE * WAVES && CHUNK == THREADS && CHUNK % MFMA_FRAMES == 0 && TILE == 16 && SOLVE_THREADS >= MAX_D && MAX_PAIRS <= WAVES * PAIRS_PER_WAVE
             ? 0
             : fail("constants", 0, 0, 0);
}

int main() {
  int models = 0;
  for (int M = 1; M <= MAX_M; ++M)
    for (int K = 1; K <= MAX_K; ++K)
      for (int delay = 1; delay <= MAX_DELAY; ++delay) {
        if (!model_ok(M, K, delay)) {
          if (M * K <= MAX_D) return fail("model refused", M, K, delay);
          continue;
        }
        if (check_model(M, K, delay)) return 1;
        ++models;
      }
  // every frame count up to a few chunks, then a stride and the top; the halo at its ends
  const int halos[][2] = {{1, 1}, {3, 2}, {10, 3}, {32, 16}};
  for (const auto& h : halos) {
    for (int frames = 1; frames <= 3 * CHUNK + 5; ++frames)
      if (check_frames(frames, h[0], h[1])) return 1;
    for (int frames = 3 * CHUNK + 6; frames <= MAX_FRAMES; frames += 977)
      if (check_frames(frames, h[0], h[1])) return 1;
    if (check_frames(5626, h[0], h[1]) || check_frames(MAX_FRAMES, h[0], h[1])) return 1;
  }
  if (check_sizes()) return 1;
  std::printf("WPE_INDEX_SANITIZE_OK %d models\n", models);
  return 0;
}
