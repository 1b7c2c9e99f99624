// The host-side rules of the PROJET kernels (audiosourcesep_amd/csrc/glowk_projet_index.h) against straightforward loops, compiled
// without HIP under AddressSanitizer + UBSan (tests/test_projet_cpu.py): the tiles of M, the workgroups of a signal and their chunks
// (every cell owned once, by the thread and the step the kernels say), the chain behind an outer sum and the workspace.
// With the argument "chain" it prints chain(rows, frames) for the pairs on its command line, for the tests' own restatement of it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../audiosourcesep_amd/csrc/glowk_projet_index.h"

using namespace glowk_projet;

static int fail(const char* what, long a, long b, long c) {
  std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

static int check_tiles() {
  for (int M = MIN_M; M <= MAX_M; ++M) {
    int t = 0;
    while (t * TILE_M < M) ++t;
    if (m_tiles(M) != t || m_padded(M) != t * TILE_M || m_tiles(M) > MAX_TILES || m_padded(M) - M >= TILE_M) return fail("tiles", M, t, 0);
    // every (kind, m) has one row of one tile: rows 0 .. 7 the numerators, 8 .. 15 the denominators
    std::vector<int> seen((size_t)2 * m_padded(M), 0);
    for (int tile = 0; tile < m_tiles(M); ++tile)
      for (int row = 0; row < TILE_ROWS; ++row) {
        const int kind = row / TILE_M, m = tile * TILE_M + row % TILE_M;
        ++seen[(size_t)kind * m_padded(M) + m];
      }
    for (int v : seen)
      if (v != 1) return fail("tile rows", M, v, 0);
  }
  return TILE_ROWS == 16 && TILE_J == 16 && MFMA_CELLS == 4 && WAVE % MFMA_CELLS == 0 && THREADS == WAVE * WAVES ? 0 : fail("constants", 0, 0, 0);
}

// the chunks by the definition: as many workgroups as 256-cell steps, at most 1024; a chunk the smallest multiple of 256 that covers
// the cells with that many workgroups; then only the workgroups that own a cell
static int check_chunks(int64_t cells, bool walk) {
  int64_t want = 0;
  while (want * THREADS < cells) ++want;
  if (want > MAX_GROUPS) want = MAX_GROUPS;
  if (want < 1) want = 1;
  int64_t per = THREADS;
  while (per * want < cells) per += THREADS;
  int64_t g = 0;
  while (g * per < cells) ++g;
  if (g < 1) g = 1;
  if (chunk_cells(cells) != per || groups(cells) != g || chunk_steps(cells) != per / THREADS) return fail("chunk sizes", (long)cells, (long)per, (long)g);
  if (g > MAX_GROUPS || g > want) return fail("groups cap", (long)cells, (long)g, 0);
  int64_t next = 0;
  std::vector<unsigned char> owned(walk ? (size_t)cells : 0, 0);
  for (int64_t i = 0; i < g; ++i) {
    int64_t c0, c1;
    chunk_of(cells, (int)i, c0, c1);
    if (c0 != next || c1 < c0 || c1 > cells || c1 - c0 > per) return fail("chunk bounds", (long)cells, (long)i, (long)c0);
    if (cells > 0 && c1 == c0) return fail("empty chunk", (long)cells, (long)i, 0);
    next = c1;
    if (walk)
      for (int step = 0; step < chunk_steps(cells); ++step)
        for (int t = 0; t < THREADS; ++t) {
          const int64_t k = c0 + (int64_t)step * THREADS + t;   // the kernels' cell of (step, thread)
          if (k < c1) ++owned[(size_t)k];
        }
  }
  if (next != cells) return fail("chunk cover", (long)cells, (long)next, 0);
  for (unsigned char v : owned)
    if (v != 1) return fail("cell owners", (long)cells, v, 0);
  return 0;
}

static int check_chain_and_work(int rows, int frames) {
  const int64_t cells = (int64_t)rows * frames;
  // a wave's accumulator takes 64 cells a step; then the four waves; then the partials
  const int64_t c = (int64_t)chunk_steps(cells) * 64 + 4 + groups(cells);
  if (chain(rows, frames) != c || c < 64 + 4 + 1) return fail("chain", rows, frames, (long)c);
  // the divergence's chain is never longer (header comment): steps M + 8 + groups for M <= 32
  if ((int64_t)chunk_steps(cells) * MAX_M + 8 + groups(cells) > c + 4) return fail("divergence chain", rows, frames, 0);
  for (int M = MIN_M; M <= MAX_M; M += 5)
    for (int J = 1; J <= MAX_J; J += 7)
      for (int nsig : {1, 3}) {
        const size_t bytes = work_bytes(nsig, M, J, rows, frames);
        if (bytes != (size_t)nsig * groups(cells) * 2 * M * J * 8) return fail("work bytes", M, J, nsig);
        if (bytes < (size_t)nsig * groups(cells) * 8) return fail("divergence partials", M, J, nsig);
        // the last partial element the fused kernel writes and the last the Q kernel reads are inside
        const size_t last = ((size_t)(nsig - 1) * groups(cells) + (groups(cells) - 1)) * partial_doubles(M, J) + 2 * M * J - 1;
        if ((last + 1) * 8 != bytes) return fail("work last", M, J, nsig);
      }
  return 0;
}

static int check_ranges() {
  if (!sizes_ok(0, 1, 1, 1) || !sizes_ok(MAX_SIG, 1, 1, MAX_J) || sizes_ok(-1, 1, 1, 1) || sizes_ok(MAX_SIG + 1, 1, 1, 1)) return fail("nsig", 0, 0, 0);
  if (sizes_ok(1, 0, 1, 1) || sizes_ok(1, MAX_ROWS + 1, 1, 1) || sizes_ok(1, 1, 0, 1) || sizes_ok(1, 1, MAX_FRAMES + 1, 1)) return fail("plane", 0, 0, 0);
  if (sizes_ok(1, 1, 1, 0) || sizes_ok(1, 1, 1, MAX_J + 1)) return fail("J", 0, 0, 0);
  if (!sizes_ok(1, MAX_ROWS, MAX_FRAMES, MAX_J) || sizes_ok(2, MAX_ROWS, MAX_FRAMES, MAX_J) || sizes_ok(MAX_SIG, MAX_ROWS, MAX_FRAMES, 1)) return fail("2^31", 0, 0, 0);
  if (!model_ok(2, 1, 1) || !model_ok(32, 128, 8) || model_ok(1, 1, 1) || model_ok(33, 1, 1) || model_ok(2, 0, 1) || model_ok(2, 129, 1) || model_ok(2, 1, 0) ||
      model_ok(2, 1, 9))
    return fail("model", 0, 0, 0);
  return FLOOR == 1.0 / 1099511627776.0 ? 0 : fail("floor", 0, 0, 0);
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "chain")) {
    for (int i = 2; i + 1 < argc; i += 2) std::printf("%lld\n", (long long)chain(std::atoi(argv[i]), std::atoi(argv[i + 1])));
    return 0;
  }
  int bad = check_tiles() + check_ranges();
  for (int64_t cells = 1; cells <= 3000 && !bad; ++cells) bad += check_chunks(cells, true);
  for (int64_t cells : {(int64_t)261887, (int64_t)261888, (int64_t)261889, (int64_t)262143, (int64_t)262144, (int64_t)262145, (int64_t)262400, (int64_t)524288,
                        (int64_t)524289, (int64_t)5766650})
    if (!bad) bad += check_chunks(cells, true);
  for (int64_t cells = 1; cells <= (int64_t)MAX_ROWS * MAX_FRAMES && !bad; cells += 100003) bad += check_chunks(cells, false);
  if (!bad) bad += check_chunks((int64_t)MAX_ROWS * MAX_FRAMES, false);
  const int shapes[][2] = {{1, 1}, {2, 1}, {3, 5}, {33, 40}, {17, 24}, {65, 130}, {129, 257}, {1025, 24}, {4096, 5}, {1, 257}, {512, 512}, {545, 481}, {1025, 5626},
                           {4096, 32768}};
  for (const auto& s : shapes)
    if (!bad) bad += check_chain_and_work(s[0], s[1]);
  if (bad) return 1;
  std::printf("PROJET_INDEX_SANITIZE_OK\n");
  return 0;
}
