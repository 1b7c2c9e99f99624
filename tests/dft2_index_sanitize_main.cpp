// The integer rules of the 2-D DFT and the peak mask (audiosourcesep_amd/csrc/glowk_dft2_index.h, the functions the kernels and the
// entry points call) run on the host under -fsanitize=address,undefined (tests/test_ft2d_cpu.py) against straightforward loops: the
// wrap map through heap rows of exactly n entries for every halo the kernels read, the stepped twiddle index against the 64-bit
// product, the tiling plan (every output in exactly one wave's tile, every block inside the grid), the workspace layout, and the
// chunks of the standard deviation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../audiosourcesep_amd/csrc/glowk_dft2_index.h"

using namespace glowk_dft2;

static int fail(const char* what, long a, long b, long c) {
  std::printf("%s(%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

// the GEMM grid of one stage: blocks = mtiles * groups, wave w of block b owns the nt n-tiles from ((b % groups) * WAVES + w) * nt on
// of m-tile b / groups
static int sweep_tiles(int64_t M, int64_t N, int64_t blocks, int nt_per_wave) {
  const int64_t groups = groups_of(N, nt_per_wave), mtiles = ceil_div64(M, TILE);
  if (blocks != mtiles * groups) return 1;
  std::vector<int> hit((size_t)(M * N), 0);
  for (int64_t b = 0; b < blocks; ++b)
    for (int w = 0; w < WAVES * nt_per_wave; ++w) {
      const int64_t mt = b / groups, nt = (b % groups) * WAVES * nt_per_wave + w;
      if (nt * TILE >= N) continue;
      for (int i = 0; i < TILE; ++i)
        for (int j = 0; j < TILE; ++j) {
          const int64_t m = mt * TILE + i, n = nt * TILE + j;
          if (m < M && n < N) ++hit[(size_t)(m * N + n)];
        }
    }
  for (int v : hit)
    if (v != 1) return 1;
  return 0;
}

int main() {
  long checks = 0;
  // the wrap map: every index a halo of nb / 2 <= 63 cells can reach around a segment or a tile, read through a row of exactly n
  for (int n = 1; n <= 70; ++n) {
    int* row = (int*)std::malloc(sizeof(int) * n);
    for (int i = 0; i < n; ++i) row[i] = i;
    for (int i = -200; i <= n + PK_SEG + 200; ++i) {
      int want = i;
      while (want < 0) want += n;
      while (want >= n) want -= n;
      if (row[wrap_index(i, n)] != want) return fail("wrap_index", i, n, 0);
      ++checks;
    }
    std::free(row);
  }
  for (int n : {4096, 32768})
    for (int i : {-63, -1, 0, n - 1, n, n + 63, n + PK_SEG + 126})
      if (wrap_index(i, n) != ((i % n) + n) % n) return fail("wrap_index", i, n, 1);
  // the twiddle index: stepping from (a * first) mod n by (a * stride) mod n equals the 64-bit product, and stays inside the table
  for (unsigned n : {1u, 2u, 3u, 5u, 31u, 32u, 33u, 64u, 257u, 600u, 1025u, 4096u, 5626u, 32767u, 32768u}) {
    float* table = (float*)std::malloc(sizeof(float) * 2 * n);    // (cos, sin) pairs: idx >= n is a heap overflow
    for (unsigned i = 0; i < 2 * n; ++i) table[i] = (float)i;
    for (unsigned a = 0; a < n; a += (n > 700 ? n / 97 + 1 : 1))
      for (unsigned stride = 1; stride <= 2; ++stride)
        for (unsigned first = 0; first < stride; ++first) {
          unsigned idx = first ? a % n : 0u;
          const unsigned step = (stride * a) % n;
          for (unsigned k = first; k < n + 3; k += stride) {       // (past the end: the dead K slots still step)
            const unsigned want = (unsigned)(((uint64_t)a * k) % n);
            if (idx != want || table[2 * idx + 1] != (float)(2 * want + 1)) return fail("tw_step", a, k, n);
            if (k < 32768 && a < 32768 && tw_index(a, k, n) != want) return fail("tw_index", a, k, n);
            idx = tw_step(idx, step, n);
            ++checks;
          }
        }
    std::free(table);
  }
  if (tw_index(32767, 32767, 32768) != (unsigned)((32767ull * 32767ull) % 32768ull)) return fail("tw_index", 32767, 32767, 32768);
  // the plan: the three grids cover every output once; the workspace regions are disjoint, 8-byte aligned and add up
  for (int nsig : {1, 2, 3})
    for (int rows : {1, 2, 31, 32, 33, 65, 129})
      for (int frames : {1, 2, 3, 31, 32, 33, 62, 63, 64, 65, 66, 127, 128, 129, 130, 254, 255, 256, 257, 258, 510, 511, 512, 513, 514}) {
        const Dft2Plan p = dft2_plan(nsig, rows, frames);
        if (p.fc != frames / 2 + 1 || p.m_frames != (int64_t)nsig * rows) return fail("plan", nsig, rows, frames);
        if (sweep_tiles(p.m_frames, p.fc, p.fwd_frames_blocks, NT_FWD)) return fail("fwd_frames_blocks", nsig, rows, frames);
        if (sweep_tiles(p.m_frames, frames, p.inv_frames_blocks, NT_INV)) return fail("inv_frames_blocks", nsig, rows, frames);
        if (p.rows_blocks % nsig || sweep_tiles(rows, p.fc, p.rows_blocks / nsig, NT_ROWS)) return fail("rows_blocks", nsig, rows, frames);
        if (p.tab_t_off != 0 || p.tab_r_off != (size_t)frames * 8 || p.mid_off != p.tab_r_off + (size_t)rows * 8 ||
            p.bytes != p.mid_off + (size_t)nsig * rows * p.fc * 8 || p.bytes % 8)
          return fail("layout", nsig, rows, frames);
        ++checks;
      }
  {
    const Dft2Plan p = dft2_plan(1, 1025, 5626), q = dft2_plan(2, 1025, 5626);
    if (p.bytes != 8ull * (5626 + 1025 + 1025ull * 2814) || q.bytes - p.bytes != 8ull * 1025 * 2814) return fail("bytes", 1, 1025, 5626);
    const Dft2Plan big = dft2_plan(65535, 1, 32767);              // the largest batch: the grids stay below 2^31
    if (big.fwd_frames_blocks > INT32_MAX || big.inv_frames_blocks > INT32_MAX || big.rows_blocks > INT32_MAX) return fail("blocks", 65535, 1, 32767);
    const Dft2Plan tall = dft2_plan(1, 1, 1);
    if (tall.fwd_frames_blocks != 1 || tall.rows_blocks != 1 || tall.inv_frames_blocks != 1 || tall.bytes != 24) return fail("plan", 1, 1, 1);
  }
  // the chunks of the standard deviation: consecutive, inside [0, n), every element once
  for (int64_t n : {1ll, 2ll, 255ll, 256ll, 4095ll, 4096ll, 4097ll, 8193ll, 1048575ll, 1048576ll, 1048577ll, 5766650ll, 2147483647ll}) {
    const int nb = std_blocks(n);
    int64_t want = (n + STD_PER_BLOCK - 1) / STD_PER_BLOCK;
    want = want > STD_MAX_BLOCKS ? STD_MAX_BLOCKS : want;
    if (nb != want) return fail("std_blocks", n, nb, want);
    int64_t next = 0;
    for (int b = 0; b < nb; ++b) {
      int64_t first, count;
      std_chunk(n, nb, b, first, count);
      if (count < 0 || first + count > n || (count > 0 && first != next)) return fail("std_chunk", n, nb, b);
      next = count > 0 ? first + count : next;
      ++checks;
    }
    if (next != n) return fail("std_chunk covers", n, nb, next);
  }
  std::printf("DFT2_INDEX_SANITIZE_OK %ld checks\n", checks);
  return 0;
}
