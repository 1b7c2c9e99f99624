// The host-side rules of the RPCA kernels (audiosourcesep_amd/csrc/glowk_rpca_index.h) against straightforward loops, compiled without
// HIP under AddressSanitizer + UBSan (tests/test_rpca_cpu.py): the round-robin order of the Jacobi pairs, the tiles and the K split of
// the GEMM, the chunks of the fixed-order sums and the workspace plans.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../audiosourcesep_amd/csrc/glowk_rpca_index.h"

using namespace glowk_rpca;

static int fail(const char* what, long a, long b, long c) {
  std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

// the order as a list that is rotated: [x0, x1, .., x_{m-1}] -> [x0, x_{m-1}, x1, .., x_{m-2}]
static int check_round_robin(int n) {
  const int m = rr_players(n);
  if (m != n + (n & 1) || rr_pairs(n) != m / 2 || rr_rounds(n) != (n < 2 ? 0 : m - 1)) return fail("rr sizes", n, m, 0);
  std::vector<int> idx((size_t)m);
  for (int i = 0; i < m; ++i) idx[(size_t)i] = i;
  std::vector<char> met((size_t)m * m, 0);
  for (int r = 0; r < rr_rounds(n); ++r) {
    std::vector<char> used((size_t)m, 0);
    for (int i = 0; i < m / 2; ++i) {
      const int a = idx[(size_t)i], b = idx[(size_t)(m - 1 - i)];
      int p, q;
      const bool live = rr_pair(n, r, i, p, q);
      if (p != (a < b ? a : b) || q != (a < b ? b : a) || !(p < q) || q >= m) return fail("rr pair", n, r, i);
      if (live != (q < n)) return fail("rr bye", n, r, i);
      if (used[(size_t)p] || used[(size_t)q]) return fail("rr disjoint", n, r, i);
      used[(size_t)p] = used[(size_t)q] = 1;
      if (met[(size_t)p * m + q]) return fail("rr twice", n, p, q);
      met[(size_t)p * m + q] = 1;
    }
    std::vector<int> next((size_t)m);
    next[0] = idx[0];
    if (m > 1) next[1] = idx[(size_t)(m - 1)];
    for (int i = 2; i < m; ++i) next[(size_t)i] = idx[(size_t)(i - 1)];
    idx = next;
  }
  if (n >= 2)
    for (int p = 0; p < m; ++p)
      for (int q = p + 1; q < m; ++q)
        if (!met[(size_t)p * m + q]) return fail("rr missed", n, p, q);
  return 0;
}

static int check_gemm(int M, int K) {
  const int nt = gemm_tiles(M);
  if ((long)nt * GEMM_TILE < M || (long)(nt - 1) * GEMM_TILE >= M) return fail("tiles", M, nt, 0);
  int t = 0;
  for (int i = 0; i < nt; ++i)
    for (int j = i; j < nt; ++j, ++t) {
      int bi, bj;
      gemm_upper_tile(nt, t, bi, bj);
      if (bi != i || bj != j) return fail("upper tile", nt, t, 0);
    }
  if (t != gemm_upper_count(nt)) return fail("upper count", nt, t, 0);
  const int s = gemm_splits(K), len = gemm_split_len(K);
  if (s < 1 || s > GEMM_MAX_SPLIT || len % GEMM_BK || (long)s * len < K) return fail("split", K, s, len);
  if (s > 1 && (long)(s - 1) * len >= K) return fail("empty split", K, s, len);
  if (K <= GEMM_SPLIT_K && s != 1) return fail("needless split", K, s, len);
  std::vector<char> seen((size_t)K, 0);
  for (int part = 0; part < s; ++part) {
    const int ks = part * len, ke = ks + len < K ? ks + len : K;
    for (int k = ks; k < ke; ++k) {
      if (seen[(size_t)k]) return fail("k twice", K, part, k);
      seen[(size_t)k] = 1;
    }
  }
  for (int k = 0; k < K; ++k)
    if (!seen[(size_t)k]) return fail("k missed", K, k, 0);
  if (gemm_work_bytes(3, M, M, K) != (s == 1 ? (size_t)0 : (size_t)3 * s * M * M * 8)) return fail("gemm bytes", M, K, s);
  return 0;
}

static int check_chunks(int64_t cells) {
  const int g = ew_groups(cells);
  if (g < 1 || g > EW_MAX_GROUPS) return fail("groups", (long)cells, g, 0);
  int64_t next = 0;
  for (int i = 0; i < g; ++i) {
    int64_t c0, c1;
    ew_chunk(cells, i, c0, c1);
    if (c0 != next || c1 < c0 || c1 > cells) return fail("chunk", (long)cells, i, (long)c0);
    next = c1;
  }
  if (next != cells) return fail("chunks end", (long)cells, (long)next, g);
  return 0;
}

static int check_plans(int nsig, int rows, int frames) {
  const EighPlan e = eigh_plan(nsig, rows);
  if (e.cs != 0 || e.floor != (size_t)nsig * rr_pairs(rows) * 16 || e.flags != e.floor + (size_t)nsig * 8 || e.bytes % 8 || e.bytes < e.flags + (size_t)nsig * MAX_SWEEPS * 4) return fail("eigh plan", nsig, rows, 0);
  const SvtPlan s = svt_plan(nsig, rows, frames);
  const size_t nn = (size_t)nsig * rows * rows * 8, n1 = (size_t)nsig * rows * 8;
  const size_t offs[] = {s.g, s.v, s.p, s.l, s.gain, s.sweeps, s.status, s.gemm, s.eigh, s.bytes};
  const size_t least[] = {nn, nn, nn, n1, n1, (size_t)nsig * 4, (size_t)nsig * 4, gemm_work_bytes(nsig, rows, rows, frames), e.bytes};
  for (int i = 0; i < 9; ++i)
    if (offs[i] % 8 || offs[i + 1] < offs[i] + least[i]) return fail("svt plan", nsig, rows, i);
  const FitPlan f = fit_plan(nsig, rows, frames);
  const size_t cells = (size_t)nsig * rows * frames * 8;
  const int groups = ew_groups((int64_t)rows * frames);
  const size_t foffs[] = {f.y, f.a, f.state, f.tau, f.sums, f.maxes, f.active, f.svt, f.bytes};
  const size_t fleast[] = {cells, cells, (size_t)nsig * STATE_DOUBLES * 8, (size_t)nsig * 8, (size_t)nsig * groups * 16, (size_t)nsig * groups * 4, (size_t)nsig * 4,
                           s.bytes};
  for (int i = 0; i < 8; ++i)
    if (foffs[i] % 8 || foffs[i + 1] < foffs[i] + fleast[i]) return fail("fit plan", nsig, rows, i);
  return 0;
}

int main() {
  for (int n = 1; n <= 70; ++n)
    if (check_round_robin(n)) return 1;
  for (int n : {129, 130, 1025, 2048, 2049})
    if (check_round_robin(n)) return 1;
  for (int M : {1, 2, 16, 17, 63, 64, 65, 130, 1025, 2049})
    for (int K : {1, 3, 4, 15, 16, 17, 1024, 1025, 2049, 5626, 8192, 8193, 65535})
      if (check_gemm(M, K)) return 1;
  for (int64_t cells : {(int64_t)1, (int64_t)3, (int64_t)1023, (int64_t)1024, (int64_t)1025, (int64_t)262144, (int64_t)262145, (int64_t)1025 * 5626,
                        (int64_t)2049 * 65535, (int64_t)2147483647})
    if (check_chunks(cells)) return 1;
  const int shapes[][3] = {{1, 1, 1}, {1, 2, 3}, {1, 5, 1}, {2, 16, 12}, {1, 17, 40}, {3, 33, 80}, {1, 48, 20}, {1, 65, 203}, {1, 130, 67}, {1, 1025, 5626}, {1, 2049, 65535}};
  for (const auto& s : shapes)
    if (check_plans(s[0], s[1], s[2])) return 1;
  if (!sizes_ok(0, 1, 1) || !sizes_ok(1, 2049, 65535) || sizes_ok(1, 2050, 1) || sizes_ok(1, 0, 1) || sizes_ok(1, 1, 0) || sizes_ok(1, 1, 65536) || sizes_ok(-1, 1, 1) ||
      sizes_ok(65536, 1, 1) || sizes_ok(16, 2049, 65535) || sizes_ok(512, 2049, 1) || !sizes_ok(511, 2049, 1))
    return fail("sizes_ok", 0, 0, 0);
  std::printf("RPCA_INDEX_SANITIZE_OK\n");
  return 0;
}
