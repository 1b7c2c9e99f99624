// The host-side rules of the clustering kernels (audiosourcesep_amd/csrc/glowk_cluster_index.h) swept against straightforward loops, in
// a stand-alone program for AddressSanitizer + UBSan (tests/test_cluster_cpu.py builds and runs it; no HIP, no Python).
//   no arguments: the sweep; prints CLUSTER_INDEX_SANITIZE_OK
//   chain R T [R T ..]: prints chain(R, T) of every pair
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../audiosourcesep_amd/csrc/glowk_cluster_index.h"

using namespace glowk_cluster;

static int fails = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++fails;                                                           \
    }                                                                    \
  } while (0)

// every column of Phi is named exactly once, in the documented order
static void sweep_columns() {
  for (int D = 1; D <= MAX_D; ++D) {
    const int P = columns(D);
    CHECK(P == 2 + D + D * (D + 1) / 2 && P <= MAX_TILES * TILE && tiles(D) * TILE >= P && (tiles(D) - 1) * TILE < P);
    std::vector<int> seen(P, 0);
    int next = 0;
    CHECK(col_n() == next);
    ++seen[col_n()], ++next;
    for (int d = 0; d < D; ++d) {
      CHECK(col_a(d) == next);
      ++seen[col_a(d)], ++next;
    }
    for (int a = 0; a < D; ++a)
      for (int b = a; b < D; ++b) {
        CHECK(col_b(D, a, b) == next);
        ++seen[col_b(D, a, b)], ++next;
      }
    CHECK(col_ll(D) == next && next == P - 1);
    ++seen[col_ll(D)];
    for (int c = 0; c < P; ++c) CHECK(seen[c] == 1);
    CHECK(stat_cluster(D) == P - 1);
    for (int J = 1; J <= MAX_J; ++J) {
      CHECK(partial_doubles(D, J) == (size_t)J * (P - 1) + 1);
      CHECK(cons_doubles(D, J) == D + J * (1 + D + D * D));
    }
  }
  CHECK(LL_ROW >= MAX_J && LL_ROW < TILE);
}

// the chunks of a signal cover its cells once, in order; thread t of step s of workgroup g never leaves the chunk's steps
static void sweep_partition(int64_t cells) {
  const int g = groups(cells);
  const int64_t per = chunk_cells(cells);
  const int steps = chunk_steps(cells);
  CHECK(g >= 1 && g <= MAX_GROUPS + 1 && per % THREADS == 0 && (int64_t)steps * THREADS == per);
  int64_t at = 0;
  for (int i = 0; i < g; ++i) {
    int64_t c0, c1;
    chunk_of(cells, i, c0, c1);
    CHECK(c0 == at && c1 > c0 && c1 - c0 <= per);
    if (i + 1 < g) CHECK(c1 - c0 == per);
    at = c1;
  }
  CHECK(at == cells);
  int64_t c0, c1;
  chunk_of(cells, g, c0, c1);                                    // one past the last: empty
  CHECK(c0 == c1);
}

static void sweep_sizes() {
  CHECK(sizes_ok(1, 1, 1, 1, 1) && sizes_ok(0, 8, 8, 4096, 32768) && sizes_ok(65535, 1, 1, 1, 1));
  CHECK(!sizes_ok(-1, 1, 1, 1, 1) && !sizes_ok(65536, 1, 1, 1, 1) && !sizes_ok(1, 0, 1, 1, 1) && !sizes_ok(1, 9, 1, 1, 1));
  CHECK(!sizes_ok(1, 1, 0, 1, 1) && !sizes_ok(1, 1, 9, 1, 1) && !sizes_ok(1, 1, 1, 0, 1) && !sizes_ok(1, 1, 1, 4097, 1));
  CHECK(!sizes_ok(1, 1, 1, 1, 0) && !sizes_ok(1, 1, 1, 1, 32769));
  CHECK(sizes_ok(1, 8, 8, 4096, 32768) && sizes_ok(1, 8, 8, 4096, 32768) && !sizes_ok(3, 8, 2, 4096, 32768) && sizes_ok(15, 1, 1, 4096, 32768));
  for (int nsig = 1; nsig <= 3; ++nsig)
    for (int D = 1; D <= MAX_D; ++D)
      for (int J = 1; J <= MAX_J; ++J) {
        const size_t g = groups(33 * 47);
        const size_t want = (nsig * g * partial_doubles(D, J) + nsig * (partial_doubles(D, J) + cons_doubles(D, J) + 2)) * 8;
        CHECK(work_bytes(nsig, D, J, 33, 47) == want);
      }
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "chain") == 0) {
    for (int i = 2; i + 1 < argc; i += 2) std::printf("%lld\n", (long long)chain(std::atoi(argv[i]), std::atoi(argv[i + 1])));
    return 0;
  }
  sweep_columns();
  for (int64_t cells = 1; cells <= 3000; ++cells) sweep_partition(cells);
  for (int64_t cells : {(int64_t)262143, (int64_t)262144, (int64_t)262145, (int64_t)264195, (int64_t)1025 * 5626, (int64_t)4096 * 32768, (int64_t)4096 * 32768 - 1})
    sweep_partition(cells);
  for (int64_t cells = 261000; cells <= 263500; cells += 7) sweep_partition(cells);
  // the longest chain: steps * 64 + 4 + groups, by a straightforward count
  for (int R : {1, 5, 17, 33, 64, 513, 1025, 4096})
    for (int T : {1, 7, 45, 64, 515, 5626, 32768}) {
      const int64_t cells = (int64_t)R * T;
      int64_t c0, c1, longest = 0;
      for (int g = 0; g < groups(cells); ++g) {
        chunk_of(cells, g, c0, c1);
        const int64_t steps = (c1 - c0 + THREADS - 1) / THREADS;
        if (steps > longest) longest = steps;
      }
      CHECK(longest == chunk_steps(cells));
      CHECK(chain(R, T) == longest * WAVE + WAVES + groups(cells));
    }
  sweep_sizes();
  if (fails) return 1;
  std::printf("CLUSTER_INDEX_SANITIZE_OK\n");
  return 0;
}
