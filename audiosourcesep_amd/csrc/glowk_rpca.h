// glowk: robust PCA (inexact augmented Lagrange multipliers, Lin et al. 2010) on a magnitude spectrogram: low-rank plus sparse.
// The singular value thresholding goes through the Gram matrix on the rows side and a symmetric eigendecomposition: an fp64 GEMM on
// the matrix cores (v_mfma_f64_16x16x4_f64) and a cyclic Jacobi solver in round-robin order, one round two launches.  Everything is
// fp64 without contraction after the float32 load of M; every order is fixed by the shapes, there are no atomics, no spin waits and
// no device loop whose trip count depends on data: launch boundaries are the only synchronisation between workgroups.
// Geometry and ordering rules: glowk_rpca_index.h.  Formulas and ranges: include/glowk.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glowk_rpca_index.h"

namespace glowk_rpca {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// a signal the fused loop has stopped (or never started) is skipped by every kernel: its state stays as it is
__device__ inline bool rpca_idle(const int* active, int sig) { return active && active[sig] == 0; }

// ---- the fp64 GEMM -------------------------------------------------------------------------------------------------------------------------
// C[i][j] = sum_k A[i][k] (scale[k] B(k, j)), A [M][K] row-major, B(k, j) = B[j][k] (TRANSB, B [N][K]) or B[k][j] (B [K][N]).  SYM
// (N == M): only the tiles on and above the diagonal are computed, and of those only the elements i <= j, each written to (i, j) and
// (j, i).  blockIdx: x the tile, y the part of K, z the signal.  With more than one part of K the workgroup writes its partial
// product to `partial` [sig][part][M][N] and k_rpca_gemm_reduce adds the parts in ascending order.
// The MFMA's lanes: A operand a[i = lane & 15][k = lane >> 4], B operand b[k = lane >> 4][j = lane & 15], result register r holds
// c[row = (lane >> 4) + 4 r][col = lane & 15] (the f64 form's own layout, not the f32 forms').
constexpr int GEMM_LD = GEMM_TILE + 1;

template <bool TRANSB, bool SYM>
__global__ __launch_bounds__(GEMM_THREADS) void k_rpca_gemm(const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ scale,
                                                            int M, int N, int K, int nsplit, int split_len, const int* __restrict__ active,
                                                            double* __restrict__ C, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double sA[GEMM_BK][GEMM_LD];
  __shared__ double sB[GEMM_BK][GEMM_LD];
  const int sig = blockIdx.z, part = blockIdx.y;
  if (rpca_idle(active, sig)) return;
  int bi, bj;
  if (SYM) {
    gemm_upper_tile(gemm_tiles(M), (int)blockIdx.x, bi, bj);
  } else {
    const int tn = gemm_tiles(N);
    bi = (int)blockIdx.x / tn;
    bj = (int)blockIdx.x % tn;
  }
  const int i0 = bi * GEMM_TILE, j0 = bj * GEMM_TILE;
  const int ks = part * split_len;
  const int ke = ks + split_len < K ? ks + split_len : K;
  const double* a = A + (size_t)sig * M * K;
  const double* b = B + (size_t)sig * N * K;
  const double* sc = scale ? scale + (size_t)sig * K : nullptr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int lr = lane & 15, lk = lane >> 4;
  f64x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4{0.0, 0.0, 0.0, 0.0};

  for (int k0 = ks; k0 < ke; k0 += GEMM_BK) {
#pragma unroll
    for (int e = 0; e < GEMM_TILE * GEMM_BK / GEMM_THREADS; ++e) {
      const int idx = tid + e * GEMM_THREADS;
      {
        const int kk = idx & (GEMM_BK - 1), i = idx / GEMM_BK;
        const int gi = i0 + i, gk = k0 + kk;
        sA[kk][i] = (gi < M && gk < ke) ? a[(size_t)gi * K + gk] : 0.0;
      }
      double v = 0.0;
      int kk, j;
      if (TRANSB) {
        kk = idx & (GEMM_BK - 1);
        j = idx / GEMM_BK;
        const int gj = j0 + j, gk = k0 + kk;
        if (gj < N && gk < ke) v = b[(size_t)gj * K + gk];
      } else {
        j = idx & (GEMM_TILE - 1);
        kk = idx / GEMM_TILE;
        const int gj = j0 + j, gk = k0 + kk;
        if (gj < N && gk < ke) v = b[(size_t)gk * N + gj];
      }
      if (sc && k0 + kk < ke) v = sc[k0 + kk] * v;
      sB[kk][j] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k4 = 0; k4 < GEMM_BK; k4 += 4) {
      double av[2], bv[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) av[mi] = sA[k4 + lk][wm + mi * 16 + lr];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) bv[ni] = sB[k4 + lk][wn + ni * 16 + lr];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
    }
    __syncthreads();
  }

  double* out = nsplit == 1 ? C + (size_t)sig * M * N : partial + ((size_t)sig * nsplit + part) * M * N;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = i0 + wm + mi * 16 + lk + 4 * r, gj = j0 + wn + ni * 16 + lr;
        if (gi >= M || gj >= N) continue;
        if (SYM && gi > gj) continue;
        const double v = acc[mi][ni][r];
        out[(size_t)gi * N + gj] = v;
        if (SYM && nsplit == 1 && gi != gj) out[(size_t)gj * N + gi] = v;
      }
}

// C = the parts added in ascending order (from 0.0 + part 0); SYM: the elements i <= j, mirrored
template <bool SYM>
__global__ __launch_bounds__(EW_THREADS) void k_rpca_gemm_reduce(const double* __restrict__ partial, int M, int N, int nsplit, int blocks,
                                                                 const int* __restrict__ active, double* __restrict__ C) {
#pragma clang fp contract(off)
  const int sig = (int)(blockIdx.x / blocks);
  if (rpca_idle(active, sig)) return;
  const int64_t cell = (int64_t)(blockIdx.x % blocks) * EW_THREADS + threadIdx.x, cells = (int64_t)M * N;
  if (cell >= cells) return;
  const int i = (int)(cell / N), j = (int)(cell % N);
  if (SYM && i > j) return;
  const double* p = partial + (size_t)sig * nsplit * cells + cell;
  double s = p[0];
  for (int k = 1; k < nsplit; ++k) s += p[(size_t)k * cells];
  double* c = C + (size_t)sig * cells;
  c[cell] = s;
  if (SYM && i != j) c[(size_t)j * N + i] = s;
}

// ---- the symmetric eigensolver ----------------------------------------------------------------------------------------------------------------
// V = I and the solve's sweep flags [MAX_SWEEPS][nsig] = 0
__global__ __launch_bounds__(EW_THREADS) void k_rpca_eye(double* __restrict__ V, int n, int blocks, int nsig, const int* __restrict__ active,
                                                         int* __restrict__ flags) {
  const int sig = (int)(blockIdx.x / blocks), blk = (int)(blockIdx.x % blocks);
  if (blk == 0 && threadIdx.x < MAX_SWEEPS) flags[(size_t)threadIdx.x * nsig + sig] = 0;   // an idle signal's too: the host reads them all
  if (rpca_idle(active, sig)) return;
  const int64_t cell = (int64_t)blk * EW_THREADS + threadIdx.x;
  if (cell >= (int64_t)n * n) return;
  V[(size_t)sig * n * n + cell] = (cell / n == cell % n) ? 1.0 : 0.0;
}

// floor [sig] = 2^-51 max |g_ij| of G as given (exact, so any order): below it a pair is not rotated
__global__ __launch_bounds__(EW_THREADS) void k_rpca_jacobi_floor(const double* __restrict__ G, int n, const int* __restrict__ active, double* __restrict__ floor) {
  __shared__ double red[EW_THREADS];
  const int sig = blockIdx.x;
  if (rpca_idle(active, sig)) return;
  const double* g = G + (size_t)sig * n * n;
  double best = 0.0;
  for (int64_t c = threadIdx.x; c < (int64_t)n * n; c += EW_THREADS) best = fmax(best, fabs(g[c]));
  red[threadIdx.x] = best;
  __syncthreads();
  for (int w = EW_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) floor[sig] = JAC_ABS * red[0];
}

// A signal's solve is over at sweep s > 0 when sweep s - 1 rotated nothing.
__device__ inline bool jac_over(const int* flags, int nsig, int sig, int sweep) { return sweep > 0 && flags[(size_t)(sweep - 1) * nsig + sig] == 0; }

// One workgroup per pair (p, q) of the round: the rotation from g_pp, g_qq, g_pq, then rows p and q of G.  The rotation (c, s), or
// (1, 0) where the pair is not rotated, goes to cs [sig][pair][2] for the column launch.  The pairs of a round are disjoint, so no
// workgroup reads what another writes.
__global__ __launch_bounds__(JAC_THREADS) void k_rpca_jacobi_rows(double* __restrict__ G, int n, int nsig, int sweep, int round, const int* __restrict__ active,
                                                                  const double* __restrict__ floor, double* __restrict__ cs, int* __restrict__ flags) {
#pragma clang fp contract(off)
  const int sig = blockIdx.y, pair = blockIdx.x;
  if (rpca_idle(active, sig) || jac_over(flags, nsig, sig, sweep)) return;
  __shared__ double rot[2];
  double* g = G + (size_t)sig * n * n;
  double* out = cs + ((size_t)sig * rr_pairs(n) + pair) * 2;
  int p, q;
  const bool live = rr_pair(n, round, pair, p, q);
  if (threadIdx.x == 0) {
    double c = 1.0, s = 0.0;
    if (live) {
      const double gpp = g[(size_t)p * n + p], gqq = g[(size_t)q * n + q], gpq = g[(size_t)p * n + q];
      if (fabs(gpq) > JAC_REL * sqrt(fabs(gpp * gqq)) && fabs(gpq) > floor[sig]) {
        const double th = (gqq - gpp) / (2.0 * gpq);
        const double t = th == 0.0 ? 1.0 : (th > 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
        c = 1.0 / sqrt(t * t + 1.0);
        s = t * c;
        flags[(size_t)sweep * nsig + sig] = 1;       // every writer stores the same value
      }
    }
    rot[0] = out[0] = c;
    rot[1] = out[1] = s;
  }
  __syncthreads();
  const double c = rot[0], s = rot[1];
  if (c == 1.0 && s == 0.0) return;
  for (int j = threadIdx.x; j < n; j += JAC_THREADS) {
    const double gp = g[(size_t)p * n + j], gq = g[(size_t)q * n + j];
    g[(size_t)p * n + j] = c * gp - s * gq;
    g[(size_t)q * n + j] = s * gp + c * gq;
  }
}

// One workgroup per row i of G and V: columns p and q of every rotated pair of the round.
__global__ __launch_bounds__(JAC_THREADS) void k_rpca_jacobi_cols(double* __restrict__ G, double* __restrict__ V, int n, int nsig, int sweep, int round,
                                                                  const int* __restrict__ active, const double* __restrict__ cs,
                                                                  const int* __restrict__ flags) {
#pragma clang fp contract(off)
  const int sig = blockIdx.y, i = blockIdx.x;
  if (rpca_idle(active, sig) || jac_over(flags, nsig, sig, sweep)) return;
  double* g = G + (size_t)sig * n * n + (size_t)i * n;
  double* v = V + (size_t)sig * n * n + (size_t)i * n;
  const int pairs = rr_pairs(n);
  const double* rot = cs + (size_t)sig * pairs * 2;
  for (int k = threadIdx.x; k < pairs; k += JAC_THREADS) {
    const double c = rot[2 * k], s = rot[2 * k + 1];
    if (c == 1.0 && s == 0.0) continue;
    int p, q;
    rr_pair(n, round, k, p, q);
    const double gp = g[p], gq = g[q];
    g[p] = c * gp - s * gq;
    g[q] = s * gp + c * gq;
    const double vp = v[p], vq = v[q];
    v[p] = c * vp - s * vq;
    v[q] = s * vp + c * vq;
  }
}

// l = diag(G); sweeps = the sweeps run (the last one rotated nothing, or the cap); the cap's bit is ORed into status
__global__ __launch_bounds__(EW_THREADS) void k_rpca_eigh_finish(const double* __restrict__ G, int n, int nsig, int swept, const int* __restrict__ active,
                                                                 const int* __restrict__ flags, double* __restrict__ l, int* __restrict__ sweeps,
                                                                 int* __restrict__ status) {
  const int sig = blockIdx.x;
  if (rpca_idle(active, sig)) return;
  for (int i = threadIdx.x; i < n; i += EW_THREADS) l[(size_t)sig * n + i] = G[(size_t)sig * n * n + (size_t)i * n + i];
  if (threadIdx.x == 0) {
    int s = 0;
    while (s < swept && flags[(size_t)s * nsig + sig] != 0) ++s;
    sweeps[sig] = s < swept ? s + 1 : swept;
    if (s >= MAX_SWEEPS) status[sig] |= STATUS_SWEEP_CAP;
  }
}

// ---- singular value thresholding --------------------------------------------------------------------------------------------------------------
// g_i = sigma_i > tau ? 1 - tau / sigma_i : 0, sigma_i = sqrt(max(l_i, 0))
__global__ __launch_bounds__(EW_THREADS) void k_rpca_gains(const double* __restrict__ l, const double* __restrict__ tau, int n, int blocks,
                                                           const int* __restrict__ active, double* __restrict__ gain) {
#pragma clang fp contract(off)
  const int sig = (int)(blockIdx.x / blocks);
  if (rpca_idle(active, sig)) return;
  const int i = (int)(blockIdx.x % blocks) * EW_THREADS + threadIdx.x;
  if (i >= n) return;
  const double li = l[(size_t)sig * n + i];
  const double sigma = sqrt(li > 0.0 ? li : 0.0), t = tau[sig];
  gain[(size_t)sig * n + i] = sigma > t ? 1.0 - t / sigma : 0.0;
}

// ---- elementwise passes -----------------------------------------------------------------------------------------------------------------------
__device__ inline double rpca_shrink(double t, double thr) {
#pragma clang fp contract(off)
  const double m = fabs(t) - thr;
  return m > 0.0 ? (t < 0.0 ? -m : m) : 0.0;
}

// out = sign(t) max(|t| - thr, 0), any fp64 array
__global__ __launch_bounds__(EW_THREADS) void k_rpca_shrink(const double* __restrict__ t, int64_t count, double thr, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x;
  if (i < count) out[i] = rpca_shrink(t[i], thr);
}

// float32 -> float64, exact
__global__ __launch_bounds__(EW_THREADS) void k_rpca_widen(const float* __restrict__ m, int64_t count, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x;
  if (i < count) out[i] = (double)m[i];
}

// the partial maxima of |M|: [sig][group] float32 (exact)
__global__ __launch_bounds__(EW_THREADS) void k_rpca_absmax(const float* __restrict__ m, int64_t cells, int groups, float* __restrict__ maxes) {
  __shared__ float red[EW_THREADS];
  const int sig = (int)(blockIdx.x / groups), grp = (int)(blockIdx.x % groups);
  int64_t c0, c1;
  ew_chunk(cells, grp, c0, c1);
  const float* x = m + (size_t)sig * cells;
  float best = 0.f;
  for (int64_t c = c0 + threadIdx.x; c < c1; c += EW_THREADS) best = fmaxf(best, fabsf(x[c]));
  red[threadIdx.x] = best;
  __syncthreads();
  for (int w = EW_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) maxes[(size_t)sig * groups + grp] = red[0];
}

// state [sig][STATE_DOUBLES]: mu, mu_bar, lam, n2, ninf, d.  One thread per signal does the two short scans in index order.
__global__ void k_rpca_init(const double* __restrict__ l, int n, const float* __restrict__ maxes, int groups, double lam, double* __restrict__ state,
                            double* __restrict__ tau, int* __restrict__ active, int* __restrict__ iters, const int* __restrict__ solve_status,
                            int* __restrict__ status) {
#pragma clang fp contract(off)
  const int sig = blockIdx.x;
  if (threadIdx.x != 0) return;
  status[sig] |= solve_status[sig];
  double lmax = 0.0;
  for (int i = 0; i < n; ++i) lmax = l[(size_t)sig * n + i] > lmax ? l[(size_t)sig * n + i] : lmax;
  float mx = 0.f;
  for (int g = 0; g < groups; ++g) mx = fmaxf(mx, maxes[(size_t)sig * groups + g]);
  const double n2 = sqrt(lmax), ninf = (double)mx;
  double* st = state + (size_t)sig * STATE_DOUBLES;
  const bool live = n2 > 0.0;
  const double mu = live ? MU0 / n2 : 0.0, byl = ninf / lam;
  st[0] = mu;
  st[1] = mu * MU_BAR;
  st[2] = lam;
  st[3] = n2;
  st[4] = ninf;
  st[5] = n2 > byl ? n2 : byl;
  st[6] = st[7] = 0.0;
  tau[sig] = live ? 1.0 / mu : 0.0;
  active[sig] = live ? 1 : 0;
  iters[sig] = 0;
}

// L = S = 0, Y = M / d (0 for a silent signal)
__global__ __launch_bounds__(EW_THREADS) void k_rpca_start(const float* __restrict__ m, int64_t cells, int blocks, const double* __restrict__ state,
                                                           const int* __restrict__ active, double* __restrict__ L, double* __restrict__ S,
                                                           double* __restrict__ Y) {
  const int sig = (int)(blockIdx.x / blocks);
  const int64_t c = (int64_t)(blockIdx.x % blocks) * EW_THREADS + threadIdx.x;
  if (c >= cells) return;
  const size_t o = (size_t)sig * cells + c;
  L[o] = 0.0;
  S[o] = 0.0;
  Y[o] = active[sig] ? (double)m[o] / state[(size_t)sig * STATE_DOUBLES + 5] : 0.0;
}

// S = shrink((M - L) + Y / mu, lam / mu), A = (M - S) + Y / mu
__global__ __launch_bounds__(EW_THREADS) void k_rpca_sparse(const float* __restrict__ m, const double* __restrict__ L, const double* __restrict__ Y,
                                                            int64_t cells, int blocks, const double* __restrict__ state, const int* __restrict__ active,
                                                            double* __restrict__ S, double* __restrict__ A) {
#pragma clang fp contract(off)
  const int sig = (int)(blockIdx.x / blocks);
  if (rpca_idle(active, sig)) return;
  const int64_t c = (int64_t)(blockIdx.x % blocks) * EW_THREADS + threadIdx.x;
  if (c >= cells) return;
  const size_t o = (size_t)sig * cells + c;
  const double mu = state[(size_t)sig * STATE_DOUBLES], lam = state[(size_t)sig * STATE_DOUBLES + 2];
  const double mv = (double)m[o], ym = Y[o] / mu;
  const double s = rpca_shrink((mv - L[o]) + ym, lam / mu);
  S[o] = s;
  A[o] = (mv - s) + ym;
}

// Z = (M - L) - S, Y += mu Z, and the chunk's sums of Z^2 and M^2: every thread adds its cells (c0 + tid, + 256, ..) in ascending order,
// then a pairwise tree over the threads.  sums [sig][group][2].
__global__ __launch_bounds__(EW_THREADS) void k_rpca_residual(const float* __restrict__ m, const double* __restrict__ L, const double* __restrict__ S,
                                                              int64_t cells, int groups, const double* __restrict__ state, const int* __restrict__ active,
                                                              double* __restrict__ Y, double* __restrict__ sums) {
#pragma clang fp contract(off)
  __shared__ double rz[EW_THREADS], rm[EW_THREADS];
  const int sig = (int)(blockIdx.x / groups), grp = (int)(blockIdx.x % groups);
  if (rpca_idle(active, sig)) return;
  int64_t c0, c1;
  ew_chunk(cells, grp, c0, c1);
  const double mu = state[(size_t)sig * STATE_DOUBLES];
  double sz = 0.0, sm = 0.0;
  for (int64_t c = c0 + threadIdx.x; c < c1; c += EW_THREADS) {
    const size_t o = (size_t)sig * cells + c;
    const double mv = (double)m[o];
    const double z = (mv - L[o]) - S[o];
    const double muz = mu * z;
    Y[o] = Y[o] + muz;
    const double zz = z * z, mm = mv * mv;
    sz = sz + zz;
    sm = sm + mm;
  }
  rz[threadIdx.x] = sz;
  rm[threadIdx.x] = sm;
  __syncthreads();
  for (int w = EW_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      rz[threadIdx.x] = rz[threadIdx.x] + rz[threadIdx.x + w];
      rm[threadIdx.x] = rm[threadIdx.x] + rm[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sums[((size_t)sig * groups + grp) * 2] = rz[0];
    sums[((size_t)sig * groups + grp) * 2 + 1] = rm[0];
  }
}

// the iteration's end for one signal: the partial sums in group order, the count, the stop test, the next mu and tau, the solver's status
__global__ void k_rpca_finish(const double* __restrict__ sums, int groups, double tol, double* __restrict__ state, double* __restrict__ tau,
                              int* __restrict__ active, int* __restrict__ iters, const int* __restrict__ solve_status, int* __restrict__ status) {
#pragma clang fp contract(off)
  const int sig = blockIdx.x;
  if (threadIdx.x != 0 || active[sig] == 0) return;
  double sz = 0.0, sm = 0.0;
  for (int g = 0; g < groups; ++g) {
    sz = sz + sums[((size_t)sig * groups + g) * 2];
    sm = sm + sums[((size_t)sig * groups + g) * 2 + 1];
  }
  double* st = state + (size_t)sig * STATE_DOUBLES;
  const double next = RHO * st[0];
  st[0] = next < st[1] ? next : st[1];
  tau[sig] = 1.0 / st[0];
  iters[sig] += 1;
  status[sig] |= solve_status[sig];
  if (sqrt(sz) / sqrt(sm) < tol) active[sig] = 0;
}

// ---- the binary mask of Huang et al. -----------------------------------------------------------------------------------------------------------
// fg = |S| > gain |L| ? 1 : 0; with X also bg = (1 - fg) X and fg X
__global__ __launch_bounds__(EW_THREADS) void k_rpca_binary_mask(const double* __restrict__ L, const double* __restrict__ S, const float2* __restrict__ X,
                                                                 int64_t count, double gain, float* __restrict__ mask, float2* __restrict__ bg,
                                                                 float2* __restrict__ fg) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x;
  if (i >= count) return;
  const bool f = fabs(S[i]) > gain * fabs(L[i]);
  mask[i] = f ? 1.f : 0.f;
  if (X) {
    const float2 x = X[i], z = {0.f, 0.f};
    bg[i] = f ? z : x;
    fg[i] = f ? x : z;
  }
}

}  // namespace glowk_rpca
