// The host-side rules of the kernel-additive-modelling kernels (audiosourcesep_amd/csrc/glowk_kam_index.h) swept against straightforward
// loops, in a stand-alone program for AddressSanitizer + UBSan (tests/test_kam_cpu.py builds and runs it; no HIP, no Python).
//   no arguments: the sweep; prints KAM_INDEX_SANITIZE_OK
//   geometry nsig rows frames n [..]: prints waves, lds_bytes, units and blocks of every quadruple
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../audiosourcesep_amd/csrc/glowk_kam_index.h"

using namespace glowk_kam;

static int fails = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++fails;                                                           \
    }                                                                    \
  } while (0)

// the workgroup of every n: MAX_WAVES waves where their slabs fit the LDS a workgroup gets without opt-in, else one
static void sweep_waves() {
  for (int n = 1; n <= MAX_N; ++n) {
    const int w = (size_t)MAX_WAVES * n * TILE_F * sizeof(float) <= (size_t)LDS_LIMIT ? MAX_WAVES : 1;
    CHECK(waves(n) == w && (candidates(n) == 4 || candidates(n) == 8));
    CHECK(lds_bytes(n) == (size_t)w * n * 256 && lds_bytes(n) <= (size_t)LDS_LIMIT);
    CHECK(table_reads(n) >= n && table_reads(n) <= TABLE_ENTRIES && table_reads(n) % TABLE_STEP == 0);
    // a lane's column of a wave's slab: every slot it may write lies inside the workgroup's LDS
    for (int wave = 0; wave < w; ++wave)
      for (int lane = 0; lane < TILE_F; lane += TILE_F - 1) {
        const size_t last = ((size_t)wave * n * TILE_F + lane + (size_t)(n - 1) * TILE_F) * sizeof(float);
        CHECK(last + sizeof(float) <= lds_bytes(n));
      }
  }
  CHECK(sizeof(Table) == (size_t)TABLE_ENTRIES * 4 && sizeof(Table) <= 1024);
}

// the units cover every cell of every signal once; the last workgroup's spare waves have no unit
static void sweep_units(int nsig, int rows, int frames, int n) {
  const int64_t nu = units(nsig, rows, frames), nb = blocks(nsig, rows, frames, n);
  CHECK(nu == (int64_t)nsig * rows * ((frames + 63) / 64));
  CHECK(nb * waves(n) >= nu && (nb - 1) * waves(n) < nu);
  std::vector<unsigned char> seen((size_t)nsig * rows * frames, 0);
  for (int64_t b = 0; b < nb; ++b)
    for (int wave = 0; wave < waves(n); ++wave) {
      const int64_t u = b * waves(n) + wave;
      if (u >= nu) continue;
      int64_t sig;
      int row, f0;
      unit_of(u, rows, frames, sig, row, f0);
      CHECK(sig >= 0 && sig < nsig && row >= 0 && row < rows && f0 >= 0 && f0 < frames && f0 % TILE_F == 0);
      for (int lane = 0; lane < TILE_F; ++lane)
        if (f0 + lane < frames) ++seen[((size_t)sig * rows + row) * frames + f0 + lane];
    }
  for (unsigned char c : seen) CHECK(c == 1);
}

// the table: the ranges, the packing, the neighbour test; a cell's neighbours as the kernel would read them stay inside the plane
static void sweep_table(int rows, int frames, const std::vector<int32_t>& off) {
  const int n = (int)off.size() / 2;
  CHECK(offsets_ok(off.data(), n));
  const Table t = pack(off.data(), n);
  std::vector<float> plane((size_t)rows * frames, 1.0f);
  for (int e = 0; e < TABLE_ENTRIES; ++e) {
    CHECK(t.d[e][0] == (e < n ? off[2 * e] : 0) && t.d[e][1] == (e < n ? off[2 * e + 1] : 0));
  }
  for (int r = 0; r < rows; ++r)
    for (int f = 0; f < frames; ++f) {
      int m = 0, want = 0;
      float sum = 0.0f;
      for (int e = 0; e < n; ++e) {
        const int rr = r + off[2 * e], ff = f + off[2 * e + 1];
        want += rr >= 0 && rr < rows && ff >= 0 && ff < frames;
        if (neighbour(r, f, t.d[e][0], t.d[e][1], rows, frames)) {
          sum += plane[(size_t)(r + t.d[e][0]) * frames + (f + t.d[e][1])];      // ASan: inside the plane
          ++m;
        }
      }
      CHECK(m == want && sum == (float)m);
      if (m > 0) CHECK(pos_low(m) == (m % 2 ? m / 2 : m / 2 - 1) && pos_high(m) == m / 2 && pos_low(m) >= 0 && pos_high(m) < m);
    }
}

static void sweep_ranges() {
  const int32_t good[4] = {-MAX_DROW, MAX_DFRAME, MAX_DROW, -MAX_DFRAME};
  CHECK(offsets_ok(good, 2) && !offsets_ok(good, 0) && !offsets_ok(nullptr, 1) && !offsets_ok(good, MAX_N + 1));
  for (int i = 0; i < 4; ++i) {
    int32_t bad[4] = {good[0], good[1], good[2], good[3]};
    bad[i] += bad[i] > 0 ? 1 : -1;
    CHECK(!offsets_ok(bad, 2));
  }
  CHECK(sizes_ok(0, 1, 1, 1) && sizes_ok(1, MAX_ROWS, MAX_FRAMES, 8) && sizes_ok(15, MAX_ROWS, MAX_FRAMES, 1) && !sizes_ok(16, MAX_ROWS, MAX_FRAMES, 1));
  CHECK(!sizes_ok(2, MAX_ROWS, MAX_FRAMES, 8) && !sizes_ok(-1, 1, 1, 1) && !sizes_ok(MAX_SIG + 1, 1, 1, 1) && !sizes_ok(1, 0, 1, 1) && !sizes_ok(1, MAX_ROWS + 1, 1, 1));
  CHECK(!sizes_ok(1, 1, 0, 1) && !sizes_ok(1, 1, MAX_FRAMES + 1, 1) && !sizes_ok(1, 1, 1, 0) && !sizes_ok(1, 1, 1, MAX_J + 1));
  // the largest plane: the unit and workgroup counts stay below 2^31
  CHECK(units(15, MAX_ROWS, MAX_FRAMES) <= MAX_ELEMENTS && blocks(15, MAX_ROWS, MAX_FRAMES, MAX_N) <= MAX_ELEMENTS);
}

static void sweep_work() {
  for (int nsig : {1, 2, 3})
    for (int J : {1, 2, 3, 8})
      for (int rows : {1, 3, 33})
        for (int frames : {1, 5, 64, 65}) {
          const size_t a = (size_t)nsig * J * rows * frames * 4;
          CHECK(work_a_bytes(nsig, rows, frames, J) % 8 == 0 && work_a_bytes(nsig, rows, frames, J) >= a && work_a_bytes(nsig, rows, frames, J) < a + 8);
          for (size_t nn : {(size_t)0, (size_t)12, (size_t)4096}) {
            const size_t w = work_bytes(nsig, rows, frames, J, nn);
            CHECK(w % 8 == 0 && w >= a + nn && w < a + nn + 16);
          }
        }
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "geometry")) {
    for (int i = 2; i + 3 < argc; i += 4) {
      const int nsig = std::atoi(argv[i]), rows = std::atoi(argv[i + 1]), frames = std::atoi(argv[i + 2]), n = std::atoi(argv[i + 3]);
      std::printf("%d %zu %lld %lld\n", waves(n), lds_bytes(n), (long long)units(nsig, rows, frames), (long long)blocks(nsig, rows, frames, n));
    }
    return 0;
  }
  sweep_waves();
  sweep_ranges();
  sweep_work();
  const int shapes[][3] = {{1, 1, 1}, {1, 3, 5}, {2, 33, 65}, {1, 65, 130}, {3, 17, 64}, {1, 257, 97}, {1, 4096, 3}, {1, 2, 4500}};
  for (const auto& s : shapes)
    for (int n : {1, 2, 8, 31, 64, 65, 127}) sweep_units(s[0], s[1], s[2], n);
  std::vector<int32_t> h, p, per, far = {MAX_DROW, 0, 0, MAX_DFRAME, -MAX_DROW, -MAX_DFRAME}, dup = {0, 0, 0, 0, 1, -1, 1, -1};
  for (int d = -15; d <= 15; ++d) {
    h.push_back(0), h.push_back(d);
    p.push_back(d), p.push_back(0);
  }
  for (int i = -8; i <= 8; ++i) per.push_back(0), per.push_back(24 * i);
  std::vector<int32_t> full;
  unsigned x = 12345u;
  for (int e = 0; e < MAX_N; ++e) {
    x = x * 1664525u + 1013904223u;
    full.push_back((int32_t)((x >> 8) % 21) - 10);
    x = x * 1664525u + 1013904223u;
    full.push_back((int32_t)((x >> 8) % 41) - 20);
  }
  for (const auto* t : {&h, &p, &per, &far, &dup, &full}) {
    sweep_table(1, 1, *t);
    sweep_table(3, 5, *t);
    sweep_table(17, 64, *t);
    sweep_table(33, 65, *t);
  }
  if (fails) return 1;
  std::printf("KAM_INDEX_SANITIZE_OK\n");
  return 0;
}
