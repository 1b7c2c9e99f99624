// glowk: clustering of time-frequency cells by a weighted Gaussian mixture (nussl's clustering separators: `PrimitiveClustering`,
// Seetharaman et al. 2019, and `SpatialClustering`).  Every cell has D <= 8 float32 features and a weight; the posteriors of J <= 8
// full-covariance Gaussians fitted by EM are the masks.  Formulas and ranges in include/glowk.h, geometry and orders in
// glowk_cluster_index.h, design and measurements in DESIGN section 27.
//
//   k_cluster_stats      the E-step of a chunk of cells in registers and the weighted moments R^T Phi on the fp64 matrix cores, one
//                        partial per workgroup; mode UNIT is the same pass with one cluster and r = 1 (pass 0 and the start)
//   k_cluster_origin     the partials of pass 0 in order -> W, o
//   k_cluster_start      the partials about o in order -> Sigma0, its principal axis, the start, the constants
//   k_cluster_update     the partials in order -> the M-step, Cholesky, Linv, k_j, the stop rule, the constants; one workgroup per signal
//   k_cluster_prepare    a given state -> the constants (the staged calls); k_cluster_sum: the partials in order (the staged statistics)
//   k_cluster_posteriors the E-step per cell -> float32 masks and, with a spectrum, the masked spectra; one thread per cell
//   k_cluster_spatial    a stereo STFT -> the pan angle, optionally the delay, and the weight; one thread per cell
//
// Everything after the float32 loads is fp64 without contraction (the matrix-core instruction is the one fused operation); every order
// is fixed by the shapes; no atomics, no spin waits: launch boundaries are the only synchronisation between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glowk_cluster_index.h"
#include "glowk_duet_index.h"

namespace glowk_cluster {

typedef double f64x4 __attribute__((ext_vector_type(4)));

enum { MODE_EM = 0, MODE_UNIT = 1, MODE_UNIT_ZERO = 2 };
constexpr double HALF_LOG_2PI = 0.91893853320467274178;   // log(2 pi) / 2
constexpr double QUARTER_PI = 0.78539816339744830962;
constexpr int MAX_CONS = cons_doubles(MAX_D, MAX_J), MAX_STATS = MAX_J * stat_cluster(MAX_D) + 1;

// The E-step of one cell: l_j = k_j - |Linv_j (x - mu_j)|^2 / 2, m = max l_j, e_j = exp(l_j - m), s = sum e_j (j ascending), lse = m +
// log s, r_j = e_j / s.  `cons` is the signal's constants (LDS).  Every kernel inlines this one function: the same bits everywhere.
template <int D>
__device__ inline double cluster_estep(const double (&x)[D], const double* cons, int J, double (&r)[MAX_J]) {
#pragma clang fp contract(off)
  double l[MAX_J];
#pragma unroll
  for (int j = 0; j < MAX_J; ++j) {
    l[j] = -__builtin_inf();
    if (j < J) {
      const double* cj = cons + D + j * cons_cluster(D);
      double diff[D];
#pragma unroll
      for (int d = 0; d < D; ++d) diff[d] = x[d] - cj[1 + d];
      double q = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        double y = cj[1 + D + a * D] * diff[0];
#pragma unroll
        for (int b = 1; b <= a; ++b) y += cj[1 + D + a * D + b] * diff[b];
        q = a == 0 ? y * y : q + y * y;
      }
      l[j] = cj[0] - q * 0.5;
    }
  }
  double m = l[0];
#pragma unroll
  for (int j = 1; j < MAX_J; ++j)
    if (j < J && l[j] > m) m = l[j];
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < MAX_J; ++j) {
    r[j] = 0.0;
    if (j < J) {
      r[j] = exp(l[j] - m);
      s = j == 0 ? r[0] : s + r[j];
    }
  }
#pragma unroll
  for (int j = 0; j < MAX_J; ++j)
    if (j < J) r[j] = r[j] / s;
  return m + log(s);
}

__device__ inline void cluster_load_cons(double* s, const double* cons, int n) {
  for (int i = threadIdx.x; i < n; i += THREADS) s[i] = cons[i];
}

// ---- the statistics pass -----------------------------------------------------------------------------------------------------------------
// Workgroup (sig, g) walks its chunk in steps of THREADS cells.  A lane leaves R of its cell -- w r_j in rows 0 .. J - 1, zeros up to row
// 7, w in row LL_ROW -- and, tile after tile, 16 columns of Phi in the wave's LDS planes, and the wave adds its 64 cells to the tile's
// accumulator with 16 instructions: operand A is a[i = lane & 15][k = lane >> 4] = R[cell 4 q + k][row i] (0 for i > 8), operand B is
// b[k = lane >> 4][c = lane & 15] = Phi[cell 4 q + k][16 tile + c], result register r holds [row = (lane >> 4) + 4 r][c = lane & 15]:
// registers 0 and 1 are the clusters, register 2 of lanes 0 .. 15 is the w row.  A cell past the chunk's end leaves zeros.
constexpr int LDP = WAVE + 4;      // row stride of the wave's planes: conflict-free stores, two-way loads at eight bytes a lane
constexpr int R_ROWS = LL_ROW + 1;

template <int D>
__global__ __launch_bounds__(THREADS) void k_cluster_stats(const float* __restrict__ f, const float* __restrict__ w, int64_t cells, int J, int mode,
                                                            const double* __restrict__ cons, int cons_stride, double* __restrict__ partial) {
#pragma clang fp contract(off)
  constexpr int P = columns(D), NT = tiles(D);
  __shared__ double sCons[MAX_CONS];
  __shared__ double sR[WAVES][R_ROWS][LDP];
  __shared__ double sPhi[WAVES][TILE][LDP];
  __shared__ double sOut[R_ROWS][NT * TILE];
  const int ngroups = groups(cells);
  const size_t sig = blockIdx.x / ngroups;
  const int grp = blockIdx.x % ngroups;
  if (mode == MODE_EM) cluster_load_cons(sCons, cons + sig * cons_stride, cons_doubles(D, J));
  else
    for (int i = threadIdx.x; i < D; i += THREADS) sCons[i] = mode == MODE_UNIT ? cons[sig * cons_stride + i] : 0.0;
  __syncthreads();
  int64_t c0, c1;
  chunk_of(cells, grp, c0, c1);
  const int steps = chunk_steps(cells);
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int li = lane & 15, lk = lane >> 4;
  const float* fp = f + sig * D * cells;
  const float* wp = w + sig * cells;
  f64x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};

  for (int step = 0; step < steps; ++step) {                   // the same trip count in every thread: the barriers below are uniform
    const int64_t k = c0 + (int64_t)step * THREADS + tid;
    const bool live = k < c1;
    double x[D], r[MAX_J], wt = 0.0, lse = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = 0.0;
#pragma unroll
    for (int j = 0; j < MAX_J; ++j) r[j] = 0.0;
    if (live) {
      wt = (double)wp[k];
#pragma unroll
      for (int d = 0; d < D; ++d) x[d] = (double)fp[(size_t)d * cells + k];
      if (mode == MODE_EM) lse = cluster_estep<D>(x, sCons, J, r);
      else r[0] = 1.0;
    }
    // Phi of the cell: 1, u, the upper triangle of u u^T, lse, zeros up to the tile's end
    double phi[NT * TILE];
    {
      double u[D];
#pragma unroll
      for (int d = 0; d < D; ++d) u[d] = live ? x[d] - sCons[d] : 0.0;
      phi[0] = 1.0;
#pragma unroll
      for (int d = 0; d < D; ++d) phi[col_a(d)] = u[d];
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = a; b < D; ++b) phi[col_b(D, a, b)] = u[a] * u[b];
      phi[col_ll(D)] = lse;
#pragma unroll
      for (int c = P; c < NT * TILE; ++c) phi[c] = 0.0;
    }
#pragma unroll
    for (int j = 0; j < MAX_J; ++j) sR[wave][j][lane] = wt * r[j];
    sR[wave][LL_ROW][lane] = wt;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int i = 0; i < TILE; ++i) sPhi[wave][i][lane] = phi[t * TILE + i];
      __syncthreads();
      f64x4 a = acc[t];
#pragma unroll
      for (int q = 0; q < WAVE / MFMA_CELLS; ++q) {
        const double av = li < R_ROWS ? sR[wave][li < R_ROWS ? li : 0][q * MFMA_CELLS + lk] : 0.0;
        const double bv = sPhi[wave][li][q * MFMA_CELLS + lk];
        a = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, a, 0, 0, 0);
      }
      acc[t] = a;
      __syncthreads();
    }
  }

  // the four waves in ascending order, then the workgroup's partial: [J][P - 1], then LL
  for (int wv = 0; wv < WAVES; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
          const int row = lk + 4 * rr;
          if (row < R_ROWS) {
            const double v = acc[t][rr];
            sOut[row][t * TILE + li] = wv == 0 ? v : sOut[row][t * TILE + li] + v;
          }
        }
    }
    __syncthreads();
  }
  const int nstat = (int)partial_doubles(D, J);
  double* out = partial + (sig * ngroups + grp) * nstat;
  for (int i = tid; i < nstat - 1; i += THREADS) out[i] = sOut[i / (P - 1)][i % (P - 1)];
  if (tid == 0) out[nstat - 1] = sOut[LL_ROW][P - 1];
}

// ---- the per-signal kernels --------------------------------------------------------------------------------------------------------------
// s[i] = the partials of element i in ascending workgroup order from 0.0
constexpr int SUM_LOADS = 32;
__device__ inline void cluster_sum_partials(const double* __restrict__ part, int ngroups, int n, double* s) {
#pragma clang fp contract(off)
  for (int i = threadIdx.x; i < n; i += THREADS) {
    double acc = 0.0;
    for (int g0 = 0; g0 < ngroups; g0 += SUM_LOADS) {           // the loads of SUM_LOADS partials in flight, the additions in order
      double v[SUM_LOADS];
#pragma unroll
      for (int u = 0; u < SUM_LOADS; ++u) v[u] = g0 + u < ngroups ? part[(size_t)(g0 + u) * n + i] : 0.0;
#pragma unroll
      for (int u = 0; u < SUM_LOADS; ++u)
        if (g0 + u < ngroups) acc += v[u];
    }
    s[i] = acc;
  }
}

__global__ __launch_bounds__(THREADS) void k_cluster_sum(const double* __restrict__ partial, int ngroups, int n, double* __restrict__ stats) {
  const size_t sig = blockIdx.x;
  cluster_sum_partials(partial + sig * ngroups * n, ngroups, n, stats + sig * n);
}

// The constants of one cluster from pi, mu [D] and Sigma [D][D]: Cholesky Sigma = L L^T (row by row, the sums in ascending order), Linv
// by forward substitution, k = (log pi - sum_d log L[d][d]) - D log(2 pi) / 2.  False on a pivot that is not positive.  One thread.
__device__ inline bool cluster_constants(int D, double pi, const double* mu, const double* S, double* cj) {
#pragma clang fp contract(off)
  double L[MAX_D][MAX_D], Li[MAX_D][MAX_D];
  double logdet = 0.0;
  for (int a = 0; a < D; ++a) {
    for (int b = 0; b <= a; ++b) {
      double s = S[a * D + b];
      for (int c = 0; c < b; ++c) s -= L[a][c] * L[b][c];
      if (a == b) {
        if (!(s > 0.0)) return false;
        L[a][a] = sqrt(s);
        logdet = a == 0 ? log(L[0][0]) : logdet + log(L[a][a]);
      } else {
        L[a][b] = s / L[b][b];
      }
    }
  }
  for (int b = 0; b < D; ++b)                                  // column b of Linv
    for (int a = 0; a < D; ++a) {
      if (a < b) {
        Li[a][b] = 0.0;
        continue;
      }
      double s = a == b ? 1.0 : 0.0;
      for (int c = b; c < a; ++c) s -= L[a][c] * Li[c][b];
      Li[a][b] = s / L[a][a];
    }
  cj[0] = (log(pi) - logdet) - (double)D * HALF_LOG_2PI;
  for (int d = 0; d < D; ++d) cj[1 + d] = mu[d];
  for (int a = 0; a < D; ++a)
    for (int b = 0; b < D; ++b) cj[1 + D + a * D + b] = Li[a][b];
  return true;
}

// the constants that give every cell the posteriors 1 / J: l_j = 0
__device__ inline void cluster_uniform(int D, int J, double* cons) {
  for (int i = threadIdx.x; i < J * cons_cluster(D); i += THREADS) cons[D + i] = 0.0;
}

// pass 0: total = W, origin = sum w x / W (0 and the status bit when W == 0)
__global__ __launch_bounds__(THREADS) void k_cluster_origin(const double* __restrict__ partial, int ngroups, int D, int J, double* __restrict__ origin,
                                                             double* __restrict__ total, int32_t* __restrict__ status, double* __restrict__ cons) {
#pragma clang fp contract(off)
  __shared__ double sS[MAX_STATS];
  const size_t sig = blockIdx.x;
  const int n = (int)partial_doubles(D, 1);
  cluster_sum_partials(partial + sig * ngroups * n, ngroups, n, sS);
  __syncthreads();
  const double W = sS[0];
  if (threadIdx.x == 0) {
    total[sig] = W;
    status[sig] = W > 0.0 ? 0 : STATUS_ZERO_WEIGHT;
  }
  if ((int)threadIdx.x < D) {
    const double o = W > 0.0 ? sS[1 + threadIdx.x] / W : 0.0;
    origin[sig * D + threadIdx.x] = o;
    cons[sig * cons_doubles(D, J) + threadIdx.x] = o;
  }
}

// the start: Sigma0 = B / W - m m^T + reg I with m = a / W about o; v by 64 power-iteration steps from all ones; lambda = v^T Sigma0 v;
// mu_j = (o + m) + (z_j sqrt(lambda)) v; Sigma_j = Sigma0; pi_j = 1 / J; the constants
__global__ __launch_bounds__(THREADS) void k_cluster_start(const double* __restrict__ partial, int ngroups, int D, int J, const double* __restrict__ z, double reg,
                                                            const double* __restrict__ total, double* __restrict__ pi, double* __restrict__ mu,
                                                            double* __restrict__ sigma, int32_t* __restrict__ status, double* __restrict__ cons) {
#pragma clang fp contract(off)
  __shared__ double sS[MAX_STATS];
  __shared__ double sSig[MAX_D * MAX_D], sMean[MAX_D], sV[MAX_D], sAmp;
  __shared__ double sCons[MAX_CONS];
  __shared__ int sOk[MAX_J];
  const size_t sig = blockIdx.x;
  const int n = (int)partial_doubles(D, 1), ncons = cons_doubles(D, J);
  cluster_sum_partials(partial + sig * ngroups * n, ngroups, n, sS);
  __syncthreads();
  const double W = total[sig];
  double* cn = cons + sig * ncons;
  if (!(W > 0.0)) {                                             // nothing to fit: a unit model at the origin, posteriors 1 / J
    for (int i = threadIdx.x; i < J; i += THREADS) pi[sig * J + i] = 1.0 / (double)J;
    for (int i = threadIdx.x; i < J * D; i += THREADS) mu[sig * J * D + i] = 0.0;
    for (int i = threadIdx.x; i < J * D * D; i += THREADS) sigma[sig * J * D * D + i] = (i % (D * D)) / D == (i % (D * D)) % D ? 1.0 : 0.0;
    cluster_uniform(D, J, cn);
    return;
  }
  if (threadIdx.x == 0) {
    double m[MAX_D];
    for (int d = 0; d < D; ++d) {
      m[d] = sS[col_a(d)] / W;
      sMean[d] = cn[d] + m[d];
    }
    for (int a = 0; a < D; ++a)
      for (int b = a; b < D; ++b) {
        double s = sS[col_b(D, a, b)] / W - m[a] * m[b];
        if (a == b) s += reg;
        sSig[a * D + b] = s;
        sSig[b * D + a] = s;
      }
    double v[MAX_D], t[MAX_D];
    for (int d = 0; d < D; ++d) v[d] = 1.0;
    for (int it = 0; it < 64; ++it) {
      double nn = 0.0;
      for (int a = 0; a < D; ++a) {
        double s = sSig[a * D] * v[0];
        for (int b = 1; b < D; ++b) s += sSig[a * D + b] * v[b];
        t[a] = s;
        nn = a == 0 ? s * s : nn + s * s;
      }
      nn = sqrt(nn);
      for (int a = 0; a < D; ++a) v[a] = t[a] / nn;
    }
    int big = 0;
    for (int d = 1; d < D; ++d)
      if (fabs(v[d]) > fabs(v[big])) big = d;
    if (v[big] < 0.0)
      for (int d = 0; d < D; ++d) v[d] = -v[d];
    double lam = 0.0;
    for (int a = 0; a < D; ++a) {
      double s = sSig[a * D] * v[0];
      for (int b = 1; b < D; ++b) s += sSig[a * D + b] * v[b];
      lam = a == 0 ? v[0] * s : lam + v[a] * s;
    }
    sAmp = sqrt(lam);
    for (int d = 0; d < D; ++d) sV[d] = v[d];
  }
  __syncthreads();
  if ((int)threadIdx.x < J) {
    const int j = threadIdx.x;
    double m[MAX_D];
    const double t = z[j] * sAmp;
    for (int d = 0; d < D; ++d) m[d] = sMean[d] + t * sV[d];
    const double p = 1.0 / (double)J;
    sOk[j] = cluster_constants(D, p, m, sSig, sCons + D + j * cons_cluster(D)) ? 1 : 0;
    pi[sig * J + j] = p;
    for (int d = 0; d < D; ++d) mu[(sig * J + j) * D + d] = m[d];
    for (int i = 0; i < D * D; ++i) sigma[(sig * J + j) * D * D + i] = sSig[i];
  }
  __syncthreads();
  bool ok = true;
  for (int j = 0; j < J; ++j) ok = ok && sOk[j];
  if (ok) {
    for (int i = threadIdx.x; i < J * cons_cluster(D); i += THREADS) cn[D + i] = sCons[D + i];
  } else {
    cluster_uniform(D, J, cn);
    if (threadIdx.x == 0) status[sig] |= STATUS_CHOLESKY;
  }
}

// a given state -> the constants.  W == 0 or a failed factorisation: the status bit and the constants of posteriors 1 / J.
__global__ __launch_bounds__(THREADS) void k_cluster_prepare(int D, int J, const double* __restrict__ pi, const double* __restrict__ mu,
                                                              const double* __restrict__ sigma, const double* __restrict__ origin, const double* __restrict__ total,
                                                              int32_t* __restrict__ status, double* __restrict__ cons) {
  __shared__ double sCons[MAX_CONS];
  __shared__ int sOk[MAX_J];
  const size_t sig = blockIdx.x;
  double* cn = cons + sig * cons_doubles(D, J);
  if ((int)threadIdx.x < D) cn[threadIdx.x] = origin[sig * D + threadIdx.x];
  const bool zero = !(total[sig] > 0.0);
  if ((int)threadIdx.x < J) {
    const int j = threadIdx.x;
    sOk[j] = cluster_constants(D, pi[sig * J + j], mu + (sig * J + j) * D, sigma + (sig * J + j) * D * D, sCons + D + j * cons_cluster(D)) ? 1 : 0;
  }
  __syncthreads();
  bool ok = true;
  for (int j = 0; j < J; ++j) ok = ok && sOk[j];
  if (ok && !zero) {
    for (int i = threadIdx.x; i < J * cons_cluster(D); i += THREADS) cn[D + i] = sCons[D + i];
  } else {
    cluster_uniform(D, J, cn);
  }
  if (threadIdx.x == 0) status[sig] = (zero ? STATUS_ZERO_WEIGHT : 0) | (ok ? 0 : STATUS_CHOLESKY);
}

// The M-step of one signal from `ngroups` partials (the staged call passes the statistics as one partial: 0.0 + x = x).  ctl [nsig][2]
// (the previous ll, the stop flag), ll [nsig][ll_stride], iters [nsig] may be null: the staged update has no loop state.
__global__ __launch_bounds__(THREADS) void k_cluster_update(const double* __restrict__ partial, int ngroups, int D, int J, double reg, double tol, int it,
                                                             double* __restrict__ pi, double* __restrict__ mu, double* __restrict__ sigma,
                                                             const double* __restrict__ origin, const double* __restrict__ total, int32_t* __restrict__ status,
                                                             double* __restrict__ cons, double* __restrict__ ctl, double* __restrict__ ll, int ll_stride,
                                                             int32_t* __restrict__ iters) {
#pragma clang fp contract(off)
  __shared__ double sS[MAX_STATS];
  __shared__ double sPi[MAX_J], sMu[MAX_J * MAX_D], sSig[MAX_J * MAX_D * MAX_D];
  __shared__ double sCons[MAX_CONS];
  __shared__ int sOk[MAX_J], sDead[MAX_J];
  const size_t sig = blockIdx.x;
  const int n = (int)partial_doubles(D, J), SC = stat_cluster(D);
  cluster_sum_partials(partial + sig * ngroups * n, ngroups, n, sS);
  __syncthreads();
  const double W = total[sig];
  const bool stopped = ctl && ctl[sig * 2 + 1] != 0.0;
  if (stopped || !(W > 0.0)) {
    if (threadIdx.x == 0) {
      if (ll) ll[sig * ll_stride + it] = __builtin_nan("");
      if (!(W > 0.0)) status[sig] |= STATUS_ZERO_WEIGHT;
    }
    return;
  }
  const double llk = sS[n - 1] / W;
  if ((int)threadIdx.x < J) {
    const int j = threadIdx.x;
    const double* S = sS + j * SC;
    const double N = S[0];
    const bool dead = N < DEAD * W;
    sDead[j] = dead;
    if (dead) {
      sPi[j] = 0.0;
      for (int d = 0; d < D; ++d) sMu[j * D + d] = mu[(sig * J + j) * D + d];
      for (int i = 0; i < D * D; ++i) sSig[j * D * D + i] = sigma[(sig * J + j) * D * D + i];
    } else {
      double m[MAX_D];
      sPi[j] = N / W;
      for (int d = 0; d < D; ++d) {
        m[d] = S[col_a(d)] / N;
        sMu[j * D + d] = origin[sig * D + d] + m[d];
      }
      for (int a = 0; a < D; ++a)
        for (int b = a; b < D; ++b) {
          double s = S[col_b(D, a, b)] / N - m[a] * m[b];
          if (a == b) s += reg;
          sSig[j * D * D + a * D + b] = s;
          sSig[j * D * D + b * D + a] = s;
        }
    }
    sOk[j] = cluster_constants(D, sPi[j], sMu + j * D, sSig + j * D * D, sCons + D + j * cons_cluster(D)) ? 1 : 0;
  }
  __syncthreads();
  bool ok = true, any_dead = false;
  for (int j = 0; j < J; ++j) {
    ok = ok && sOk[j];
    any_dead = any_dead || sDead[j];
  }
  if (ok) {
    for (int i = threadIdx.x; i < J; i += THREADS) pi[sig * J + i] = sPi[i];
    for (int i = threadIdx.x; i < J * D; i += THREADS) mu[sig * J * D + i] = sMu[i];
    for (int i = threadIdx.x; i < J * D * D; i += THREADS) sigma[sig * J * D * D + i] = sSig[i];
    double* cn = cons + sig * cons_doubles(D, J);
    for (int i = threadIdx.x; i < J * cons_cluster(D); i += THREADS) cn[D + i] = sCons[D + i];
  }
  if (threadIdx.x == 0) {
    if (ll) ll[sig * ll_stride + it] = llk;
    if (!ok) status[sig] |= STATUS_CHOLESKY;
    else if (any_dead) status[sig] |= STATUS_DEAD;
    if (ok && iters) iters[sig] = it + 1;
    if (ctl) {
      const double prev = ctl[sig * 2];
      if (!ok || (tol > 0.0 && it >= 1 && llk - prev <= tol * fabs(llk))) ctl[sig * 2 + 1] = 1.0;
      ctl[sig * 2] = llk;
    }
  }
}

// the loop state of a fit: no previous ll, not stopped, no iterations
__global__ __launch_bounds__(THREADS) void k_cluster_reset(int nsig, double* __restrict__ ctl, int32_t* __restrict__ iters) {
  const int sig = blockIdx.x * THREADS + threadIdx.x;
  if (sig >= nsig) return;
  ctl[sig * 2] = 0.0;
  ctl[sig * 2 + 1] = 0.0;
  iters[sig] = 0;
}

// ---- the posteriors ----------------------------------------------------------------------------------------------------------------------
// mask [nsig][J][cells] float32 = r_j rounded; with x [nsig][C][cells] complex64 also y [nsig][J][C][cells] = mask_j x, each component
// one float32 product.  Workgroup (sig, b) of `blocks` per signal, one thread per cell.
template <int D>
__global__ __launch_bounds__(THREADS) void k_cluster_posteriors(const float* __restrict__ f, int64_t cells, int blocks, int J, const double* __restrict__ cons,
                                                                 const float2* __restrict__ x, int C, float* __restrict__ mask, float2* __restrict__ y) {
#pragma clang fp contract(off)
  __shared__ double sCons[MAX_CONS];
  const size_t sig = blockIdx.x / blocks;
  const int64_t k = (int64_t)(blockIdx.x % blocks) * THREADS + threadIdx.x;
  const int ncons = cons_doubles(D, J);
  cluster_load_cons(sCons, cons + sig * ncons, ncons);
  __syncthreads();
  if (k >= cells) return;
  double xd[D], r[MAX_J];
#pragma unroll
  for (int d = 0; d < D; ++d) xd[d] = (double)f[(sig * D + d) * cells + k];
  cluster_estep<D>(xd, sCons, J, r);
  float2 xc[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
  if (x)
    for (int c = 0; c < C; ++c) xc[c] = x[(sig * C + c) * cells + k];
#pragma unroll
  for (int j = 0; j < MAX_J; ++j)
    if (j < J) {
      const float m = (float)r[j];
      mask[(sig * J + j) * cells + k] = m;
      if (x)
        for (int c = 0; c < C; ++c) {
          float2 o;
          o.x = m * xc[c].x;
          o.y = m * xc[c].y;
          y[((sig * J + j) * C + c) * cells + k] = o;
        }
    }
}

// ---- the spatial features ----------------------------------------------------------------------------------------------------------------
// x [nsig][2][rows][frames] complex64 -> feat [nsig][1 or 2][cells] float32 (pan, then the delay) and wgt [nsig][cells] float32.
// pan = atan2(|X2|, |X1|) - pi / 4; delta = -arg(X2 conj X1) / omega_r clipped to +-max_delay (0 in row 0 and where a channel is 0);
// w = (|X1|^2 + |X2|^2)^(p / 2), 0 in row 0 and where both channels are 0.
__global__ __launch_bounds__(THREADS) void k_cluster_spatial(const float2* __restrict__ x, int64_t total, int rows, int frames, int delay, double max_delay, double p,
                                                              float* __restrict__ feat, float* __restrict__ wgt) {
#pragma clang fp contract(off)
  const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (c >= total) return;
  const int64_t cells = (int64_t)rows * frames, sig = c / cells, k = c - sig * cells;
  const int r = (int)(k / frames);
  const float2 x1 = x[sig * 2 * cells + k], x2 = x[sig * 2 * cells + cells + k];
  const double a = x1.x, b = x1.y, cc = x2.x, d = x2.y;
  const double p1 = a * a + b * b, p2 = cc * cc + d * d, e = p1 + p2;
  const int nf = delay ? 2 : 1;
  feat[sig * nf * cells + k] = (float)(atan2(sqrt(p2), sqrt(p1)) - QUARTER_PI);
  if (delay) {
    double dl = 0.0;
    if (r != 0 && p1 != 0.0 && p2 != 0.0) {
      dl = -atan2(d * a - cc * b, cc * a + d * b) / glowk_duet::omega_of(r, rows);
      dl = dl > max_delay ? max_delay : dl < -max_delay ? -max_delay : dl;
    }
    feat[sig * nf * cells + cells + k] = (float)dl;
  }
  double wv = 0.0;
  if (r != 0 && e != 0.0) wv = p == 1.0 ? sqrt(e) : p == 2.0 ? e : pow(e, p * 0.5);
  wgt[c] = (float)wv;
}

}  // namespace glowk_cluster
