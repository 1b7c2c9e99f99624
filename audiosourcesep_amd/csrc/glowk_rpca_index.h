// glowk: the host-side rules of the RPCA kernels (glowk_rpca.h), in plain C++ so that a host program can run them without HIP
// (tests/rpca_index_sanitize_main.cpp sweeps them under AddressSanitizer + UBSan against straightforward loops): the round-robin
// order of the Jacobi pairs, the tiles and the K split of the fp64 GEMM, the groups of the fixed-order sums and the workspace plans.
// The kernels and the entry points call the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GLOWK_RPCA_HD __host__ __device__ inline
#else
#define GLOWK_RPCA_HD inline
#endif

namespace glowk_rpca {

constexpr int MAX_SIG = 65535, MAX_ROWS = 2049, MAX_FRAMES = 65535, MAX_ITER = 100000, MAX_SWEEPS = 30;
constexpr int64_t MAX_ELEMENTS = 2147483647;
constexpr double RHO = 1.5, MU0 = 1.25, MU_BAR = 1e7;
// status bits of a signal (glowk_rpca_eigh's and glowk_rpca_fit's status_dev)
constexpr int STATUS_SWEEP_CAP = 1;         // a solve reached MAX_SWEEPS sweeps and its last sweep still rotated

// ---- the round-robin ("tournament") order of the Jacobi pairs ------------------------------------------------------------------------
// m = n rounded up to even players sit at positions 0 .. m - 1; player 0 stays, the others move one position up per round (position
// m - 1 wraps to 1).  Round r in [0, m - 1) pairs the players at positions i and m - 1 - i, i in [0, m / 2).  Player n (odd n) is the bye.
GLOWK_RPCA_HD int rr_players(int n) { return n + (n & 1); }
GLOWK_RPCA_HD int rr_rounds(int n) { return n < 2 ? 0 : rr_players(n) - 1; }
GLOWK_RPCA_HD int rr_pairs(int n) { return rr_players(n) / 2; }
GLOWK_RPCA_HD int rr_at(int m, int round, int pos) {
  if (pos == 0) return 0;
  int j = (pos - 1 - round) % (m - 1);
  if (j < 0) j += m - 1;
  return 1 + j;
}
// pair i of a round as p < q; false for the bye's pair (q == n)
GLOWK_RPCA_HD bool rr_pair(int n, int round, int i, int& p, int& q) {
  const int m = rr_players(n);
  const int a = rr_at(m, round, i), b = rr_at(m, round, m - 1 - i);
  p = a < b ? a : b;
  q = a < b ? b : a;
  return q < n;
}

// ---- the fp64 GEMM: 64 x 64 tiles of C, 16 of K per stage, four waves of 32 x 32 each ------------------------------------------------------
constexpr int GEMM_TILE = 64, GEMM_BK = 16, GEMM_THREADS = 256;
constexpr int GEMM_SPLIT_K = 1024, GEMM_MAX_SPLIT = 8;
GLOWK_RPCA_HD int gemm_tiles(int n) { return (n + GEMM_TILE - 1) / GEMM_TILE; }
// parts of K, each a multiple of GEMM_BK long but the last; a function of K alone, so the bits do not depend on the grid
GLOWK_RPCA_HD int gemm_splits(int K) {
  const int s = (K + GEMM_SPLIT_K - 1) / GEMM_SPLIT_K;
  return s < 1 ? 1 : s > GEMM_MAX_SPLIT ? GEMM_MAX_SPLIT : s;
}
GLOWK_RPCA_HD int gemm_split_len(int K) {
  const int s = gemm_splits(K);
  const int per = (K + s - 1) / s;
  return (per + GEMM_BK - 1) / GEMM_BK * GEMM_BK;
}
// tile t of the upper triangle of an nt x nt grid of tiles, rows first: (0,0) (0,1) .. (0,nt-1) (1,1) ..
GLOWK_RPCA_HD int gemm_upper_count(int nt) { return nt * (nt + 1) / 2; }
GLOWK_RPCA_HD void gemm_upper_tile(int nt, int t, int& bi, int& bj) {
  int i = 0;
  while (t >= nt - i) {
    t -= nt - i;
    ++i;
  }
  bi = i;
  bj = i + t;
}
// the partial products of a split K: [nsig][splits][M][N] doubles; nothing without a split
GLOWK_RPCA_HD size_t gemm_work_bytes(int nsig, int M, int N, int K) {
  const int s = gemm_splits(K);
  return s == 1 ? 0 : (size_t)nsig * s * M * N * 8;
}

// ---- the elementwise passes and their fixed-order sums ------------------------------------------------------------------------------------
constexpr int EW_THREADS = 256, EW_PER_THREAD = 4, EW_MAX_GROUPS = 256;
// workgroups per signal: each owns a contiguous chunk of cells and leaves one partial per sum
GLOWK_RPCA_HD int ew_groups(int64_t cells) {
  const int64_t per = (int64_t)EW_THREADS * EW_PER_THREAD;
  const int64_t g = (cells + per - 1) / per;
  return g > EW_MAX_GROUPS ? EW_MAX_GROUPS : (int)g;
}
GLOWK_RPCA_HD void ew_chunk(int64_t cells, int g, int64_t& c0, int64_t& c1) {
  const int groups = ew_groups(cells);
  const int64_t per = (cells + groups - 1) / groups;
  c0 = per * g;
  if (c0 > cells) c0 = cells;
  c1 = c0 + per < cells ? c0 + per : cells;
}

// ---- Jacobi launches: rows, a workgroup per pair; columns, a workgroup per row of G and V with a thread per pair (strided) ------------------
constexpr int JAC_THREADS = 256;
constexpr double JAC_REL = 0x1p-52, JAC_ABS = 0x1p-51;   // rotate when |g_pq| > JAC_REL sqrt(|g_pp g_qq|) and > JAC_ABS max |G|

// ---- workspaces ----------------------------------------------------------------------------------------------------------------------------
// eigh: the rotations [nsig][pairs][2] doubles, the rotation floors [nsig] doubles, then the sweep flags [MAX_SWEEPS][nsig] int32
struct EighPlan {
  size_t cs, floor, flags, bytes;
};
GLOWK_RPCA_HD EighPlan eigh_plan(int nsig, int n) {
  EighPlan p;
  p.cs = 0;
  p.floor = p.cs + (size_t)nsig * rr_pairs(n) * 16;
  p.flags = p.floor + (size_t)nsig * 8;
  p.bytes = p.flags + ((size_t)nsig * MAX_SWEEPS * 4 + 7) / 8 * 8;
  return p;
}
// svt: G, V and P [nsig][rows][rows], l and g [nsig][rows], sweeps and status [nsig] int32, the Gram product's partials, the solver's
struct SvtPlan {
  size_t g, v, p, l, gain, sweeps, status, gemm, eigh, bytes;
};
GLOWK_RPCA_HD SvtPlan svt_plan(int nsig, int rows, int frames) {
  SvtPlan p;
  const size_t nn = (size_t)nsig * rows * rows * 8, n1 = (size_t)nsig * rows * 8, i1 = ((size_t)nsig * 4 + 7) / 8 * 8;
  p.g = 0;
  p.v = p.g + nn;
  p.p = p.v + nn;
  p.l = p.p + nn;
  p.gain = p.l + n1;
  p.sweeps = p.gain + n1;
  p.status = p.sweeps + i1;
  p.gemm = p.status + i1;
  p.eigh = p.gemm + gemm_work_bytes(nsig, rows, rows, frames);   // only A A^T splits K
  p.bytes = p.eigh + eigh_plan(nsig, rows).bytes;
  return p;
}
// fit: Y and A [nsig][rows][frames] doubles, the per-signal state, tau [nsig], the partial sums [nsig][groups][2], the partial maxima
// [nsig][groups] float32, the active flags [nsig] int32, the svt workspace
constexpr int STATE_DOUBLES = 8;            // mu, mu_bar, lam, n2, ninf, d (Y's first divisor), spare, spare
struct FitPlan {
  size_t y, a, state, tau, sums, maxes, active, svt, bytes;
};
GLOWK_RPCA_HD FitPlan fit_plan(int nsig, int rows, int frames) {
  FitPlan p;
  const size_t cells = (size_t)nsig * rows * frames * 8;
  const int groups = ew_groups((int64_t)rows * frames);
  p.y = 0;
  p.a = p.y + cells;
  p.state = p.a + cells;
  p.tau = p.state + (size_t)nsig * STATE_DOUBLES * 8;
  p.sums = p.tau + (size_t)nsig * 8;
  p.maxes = p.sums + (size_t)nsig * groups * 16;
  p.active = p.maxes + ((size_t)nsig * groups * 4 + 7) / 8 * 8;
  p.svt = p.active + ((size_t)nsig * 4 + 7) / 8 * 8;
  p.bytes = p.svt + svt_plan(nsig, rows, frames).bytes;
  return p;
}

// the ranges of include/glowk.h
GLOWK_RPCA_HD bool sizes_ok(int nsig, int rows, int frames) {
  if (nsig < 0 || nsig > MAX_SIG || rows < 1 || rows > MAX_ROWS || frames < 1 || frames > MAX_FRAMES) return false;
  if ((int64_t)nsig * rows * frames > MAX_ELEMENTS || (int64_t)nsig * rows * rows > MAX_ELEMENTS) return false;
  return true;
}

}  // namespace glowk_rpca
