// The plan rules of the NMF kernels (audiosourcesep_amd/csrc/glowk_nmf_index.h, the functions the kernels and the entry points call)
// run on the host under -fsanitize=address,undefined (tests/test_nmf_cpu.py) against straightforward loops: the cut of the frame
// tiles into chunks (every tile in exactly one chunk, in order, no chunk empty, the same for every nsig), the accumulator-row
// permutation, the offsets of the W update's partial sums into a heap buffer of exactly the stated size, and the workspace size.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../audiosourcesep_amd/csrc/glowk_nmf_index.h"

using namespace glowk_nmf;

static int check_plan(int rows, int frames, int K) {
  const NmfPlan p = nmf_plan(rows, frames, K);
  int rtiles = 0, ftiles = 0, kt = 0;
  for (int r = 0; r < rows; r += 32) ++rtiles;
  for (int f = 0; f < frames; f += 32) ++ftiles;
  for (int k = 0; k < K; k += 32) ++kt;
  if (p.rtiles != rtiles || p.ftiles != ftiles || p.kt != kt) { std::printf("tiles(%d, %d, %d)\n", rows, frames, K); return 1; }
  // the cut as the header states it: as many chunks as keep the workgroups of a signal within 256, at most one per four frame tiles
  int want = 1;
  while ((want + 1) * rtiles <= 256) ++want;
  const int most = ftiles / 4 < 1 ? 1 : ftiles / 4;
  if (want > most) want = most;
  int tpc = 1;
  while (tpc * want < ftiles) ++tpc;
  if (p.tpc != tpc || p.nch < 1 || p.nch > want) { std::printf("cut(%d, %d, %d): tpc %d nch %d, expected tpc %d\n", rows, frames, K, p.tpc, p.nch, tpc); return 1; }
  std::vector<int> owner(ftiles, -1);
  int next = 0;
  for (int ch = 0; ch < p.nch; ++ch) {
    int t0, t1;
    nmf_chunk(p, ch, t0, t1);
    if (t0 != next || t1 <= t0 || t1 > ftiles || t1 - t0 > p.tpc) { std::printf("chunk(%d, %d, %d)[%d] = [%d, %d)\n", rows, frames, K, ch, t0, t1); return 1; }
    for (int t = t0; t < t1; ++t) owner.at(t) = ch;
    next = t1;
  }
  if (next != ftiles) { std::printf("chunks(%d, %d, %d) end at %d of %d\n", rows, frames, K, next, ftiles); return 1; }
  for (int t = 0; t < ftiles; ++t)
    if (owner[t] < 0) return 1;
  // the workspace: the larger of the two uses, and a batch is its signals side by side
  const int64_t a = (int64_t)2 * p.nch * rows * K * 4, b = (int64_t)rtiles * p.nch * 8;
  const size_t one = nmf_work_bytes(1, rows, frames, K);
  if (one != (size_t)(a > b ? a : b) || nmf_work_bytes(0, rows, frames, K) != 0) { std::printf("work(%d, %d, %d)\n", rows, frames, K); return 1; }
  for (int nsig : {2, 3, 7, 65535})
    if (nmf_work_bytes(nsig, rows, frames, K) != one * (size_t)nsig) { std::printf("work(%d x %d, %d, %d)\n", nsig, rows, frames, K); return 1; }
  return 0;
}

// every (chunk, which, row, k) has its own slot in a buffer of exactly nmf_w_part_floats entries: one past the end is a heap overflow
static int check_parts(int rows, int frames, int K) {
  const NmfPlan p = nmf_plan(rows, frames, K);
  const int64_t n = nmf_w_part_floats(p, rows, K);
  unsigned char* seen = (unsigned char*)std::calloc((size_t)n, 1);
  for (int ch = 0; ch < p.nch; ++ch)
    for (int which = 0; which < 2; ++which)
      for (int row = 0; row < rows; ++row)
        for (int k = 0; k < K; ++k) {
          const int64_t i = nmf_w_part_index(ch, which, row, k, rows, K);
          if (i < 0 || i >= n || seen[i]++) { std::printf("part(%d, %d, %d): slot %lld\n", rows, frames, K, (long long)i); std::free(seen); return 1; }
          if (i != (int64_t)(2 * ch + which) * rows * K + (int64_t)row * K + k) { std::free(seen); return 1; }
        }
  for (int64_t i = 0; i < n; ++i)
    if (seen[i] != 1) { std::free(seen); return 1; }
  std::free(seen);
  return 0;
}

int main() {
  long plans = 0;
  const int some_rows[] = {1, 2, 31, 32, 33, 65, 257, 1025, 4095, 4096};
  const int some_k[] = {1, 2, 5, 31, 32, 33, 64, 65, 96, 97, 128};
  for (int rows : some_rows)
    for (int K : some_k) {
      for (int frames = 1; frames <= 2100; ++frames, ++plans)
        if (check_plan(rows, frames, K)) return 1;
      for (int frames : {4500, 5626, 8191, 8192, 8193, 32767, 32768}) {
        if (check_plan(rows, frames, K)) return 1;
        ++plans;
      }
    }
  for (int rows = 1; rows <= 4096; ++rows, ++plans)
    if (check_plan(rows, 5626, 128) || check_plan(rows, 32768, 1)) return 1;
  // the shapes the GPU tests use, and the largest workspace the ranges allow
  const int shapes[][3] = {{1, 1, 1}, {33, 95, 5}, {65, 33, 32}, {257, 130, 33}, {1025, 97, 128}, {2, 4500, 7}, {4096, 66, 2}, {32, 32768, 128}};
  for (const auto& s : shapes)
    if (check_parts(s[0], s[1], s[2])) return 1;
  if (nmf_plan(2, 4500, 7).nch < 3) { std::printf("4500 frames should span several chunks\n"); return 1; }
  // rho: the two lane halves' 16 registers name each of the 32 rows once
  int hit[32] = {0};
  for (int half = 0; half < 2; ++half)
    for (int r = 0; r < 16; ++r) {
      const int x = nmf_rho(r, half);
      if (x < 0 || x > 31 || hit[x]++) { std::printf("rho(%d, %d) = %d\n", r, half, x); return 1; }
    }
  std::printf("NMF_INDEX_SANITIZE_OK %ld plans\n", plans);
  return 0;
}
