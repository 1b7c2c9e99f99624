// glowk: PROJET (Fitzgerald, Liutkus & Badeau 2016; `Projet` in nussl) -- blind separation of a two-channel STFT into any number of
// panned sources: the mixture is projected on M directions, every projection is modelled as sum_j P_j(cell) (K Q)[m][j], and P and Q
// are fitted by multiplicative updates.  Formulas and ranges in include/glowk.h, geometry and orders in glowk_projet_index.h, design
// and measurements in DESIGN section 26.
//
//   k_projet_projections  X -> V [M] planes (fp64): the diagnostic and staging form
//   k_projet_gains        G = K Q, one workgroup per signal
//   k_projet_iterate      one pass over X and P: the P update (do_p) and/or the outer sums An, Ad = R^T P' on the fp64 matrix cores
//                         (do_sums), one partial per workgroup; c, V and sigma exist in registers alone
//   k_projet_q            the partials added in ascending order, the Q update, G = K Q'; one workgroup per signal
//   k_projet_divergence   the beta-divergence's partial per workgroup; k_projet_divergence_sum adds them in order
//   k_projet_separate     the soft filter on every projection, back through the pseudo-inverse; one thread per cell
//
// Everything after the float32 load of X is fp64 without contraction (the matrix-core instruction is the one fused operation); every
// order is fixed by the shapes; no atomics, no spin waits: launch boundaries are the only synchronisation between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glowk_projet_index.h"

namespace glowk_projet {

typedef double f64x4 __attribute__((ext_vector_type(4)));

enum { ALPHA_ONE = 1, ALPHA_TWO = 2, ALPHA_POW = 0 };

struct Proj {
  double re, im;
};

// c_m = U[m][0] X_1 + U[m][1] X_2: two products and one add per component
__device__ inline Proj projet_c(float2 x1, float2 x2, double u0, double u1) {
#pragma clang fp contract(off)
  Proj c;
  c.re = u0 * (double)x1.x + u1 * (double)x2.x;
  c.im = u0 * (double)x1.y + u1 * (double)x2.y;
  return c;
}

// V_m = |c_m|^alpha.  Every kernel inlines this one function, so the stored planes and the in-register values are the same bits.
__device__ inline double projet_v(Proj c, int amode, double half_alpha) {
#pragma clang fp contract(off)
  const double p = c.re * c.re + c.im * c.im;
  return amode == ALPHA_ONE ? sqrt(p) : amode == ALPHA_TWO ? p : pow(p, half_alpha);
}

// sigma_m = max(sum_j P_j G[m][j], FLOOR), j ascending; `raw` is the sum before the floor
template <int J>
__device__ inline double projet_sigma(const double (&P)[J], const double* g, double& raw) {
#pragma clang fp contract(off)
  double s = P[0] * g[0];
#pragma unroll
  for (int j = 1; j < J; ++j) s += P[j] * g[j];
  raw = s;
  return s < FLOOR ? FLOOR : s;
}

// wn = V sigma^(beta - 2), wd = sigma^(beta - 1), with divisions and products only
__device__ inline void projet_weights(double V, double s, int beta, double& wn, double& wd) {
#pragma clang fp contract(off)
  if (beta == 2) {
    wn = V;
    wd = s;
  } else if (beta == 1) {
    wn = V / s;
    wd = 1.0;
  } else {
    wn = V / (s * s);
    wd = 1.0 / s;
  }
}

// the tables of one signal in LDS: U [M][2] and G [M][MAX_J] (row stride MAX_J)
struct Tables {
  double u[MAX_M][2];
  double g[MAX_M][MAX_J];
};
__device__ inline void projet_load_tables(Tables& t, const double* U, const double* G, int M, int J) {
  for (int i = threadIdx.x; i < M * 2; i += THREADS) t.u[i >> 1][i & 1] = U[i];
  for (int i = threadIdx.x; i < M * MAX_J; i += THREADS) {
    const int m = i / MAX_J, j = i % MAX_J;
    t.g[m][j] = j < J ? G[(size_t)m * J + j] : 0.0;
  }
}

// x: [nsig][2][rows][frames] complex64 -> v [nsig][M][rows][frames].  One thread per cell.
__global__ __launch_bounds__(THREADS) void k_projet_projections(const float2* __restrict__ x, int64_t total, int64_t cells, const double* __restrict__ U, int M,
                                                                 int amode, double half_alpha, double* __restrict__ v) {
  __shared__ double su[MAX_M][2];
  for (int i = threadIdx.x; i < M * 2; i += THREADS) su[i >> 1][i & 1] = U[i];
  __syncthreads();
  const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (c >= total) return;
  const int64_t sig = c / cells, k = c - sig * cells;
  const float2 x1 = x[(size_t)sig * 2 * cells + k], x2 = x[(size_t)sig * 2 * cells + cells + k];
  for (int m = 0; m < M; ++m) v[((size_t)sig * M + m) * cells + k] = projet_v(projet_c(x1, x2, su[m][0], su[m][1]), amode, half_alpha);
}

// G[m][j] = sum_l K[m][l] Q[l][j], l ascending; q may live in LDS or in global memory
__device__ inline void projet_gains_of(const double* __restrict__ K, const double* q, int M, int L, int J, double* __restrict__ G) {
#pragma clang fp contract(off)
  for (int i = threadIdx.x; i < M * J; i += THREADS) {
    const int m = i / J, j = i % J;
    double s = K[(size_t)m * L] * q[j];
    for (int l = 1; l < L; ++l) s += K[(size_t)m * L + l] * q[(size_t)l * J + j];
    G[i] = s;
  }
}

__global__ __launch_bounds__(THREADS) void k_projet_gains(const double* __restrict__ K, const double* __restrict__ Q, int M, int L, int J, double* __restrict__ G) {
  const size_t sig = blockIdx.x;
  projet_gains_of(K, Q + sig * L * J, M, L, J, G + sig * M * J);
}

// ---- the fused iteration ---------------------------------------------------------------------------------------------------------------
// Workgroup (sig, g) walks its chunk in steps of THREADS cells.  do_p: P_j' = P_j g(num_j / max(den_j, FLOOR)) from the cell's own V and
// sigma, stored.  do_sums: with sigma' from P' (the P just computed, or the P given) the lane leaves the weights of one tile -- wn_m in
// rows 0 .. 7, wd_m in rows 8 .. 15, m = 8 tile + row -- and its P' in the wave's LDS planes, and the wave adds its 64 cells to the
// tile's accumulator with 16 instructions: operand A is a[i = lane & 15][k = lane >> 4] = w[row i][cell 4 q + k], operand B is
// b[k = lane >> 4][j = lane & 15] = P'[cell 4 q + k][j] (0 for j >= J), result register r holds c[row = (lane >> 4) + 4 r][j = lane & 15]:
// registers 0 and 1 are An, 2 and 3 are Ad.  A cell past the chunk's end leaves zeros.
constexpr int LDP = WAVE + 4;      // row stride of the wave's planes: conflict-free stores, two-way loads at eight bytes a lane

template <int J>
__global__ __launch_bounds__(THREADS) void k_projet_iterate(const float2* __restrict__ x, double* P, int64_t cells, const double* __restrict__ U,
                                                             const double* __restrict__ G, int M, int amode, double half_alpha, int beta, int do_p, int do_sums,
                                                             double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ Tables tb;
  __shared__ double sW[WAVES][TILE_ROWS][LDP];
  __shared__ double sP[WAVES][J][LDP];
  __shared__ double sOut[2][MAX_M][MAX_J];
  const int ngroups = groups(cells);
  const size_t sig = blockIdx.x / ngroups;
  const int grp = blockIdx.x % ngroups;
  projet_load_tables(tb, U, G + sig * M * J, M, J);
  __syncthreads();
  int64_t c0, c1;
  chunk_of(cells, grp, c0, c1);
  const int steps = chunk_steps(cells), tiles = m_tiles(M);
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int li = lane & 15, lk = lane >> 4;
  const float2* x1p = x + sig * 2 * cells;
  const float2* x2p = x1p + cells;
  double* Pp = P + sig * J * cells;
  f64x4 acc[MAX_TILES];
#pragma unroll
  for (int t = 0; t < MAX_TILES; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};

  for (int step = 0; step < steps; ++step) {                   // the same trip count in every thread: the barriers below are uniform
    const int64_t k = c0 + (int64_t)step * THREADS + tid;
    const bool live = k < c1;
    float2 x1 = {0.0f, 0.0f}, x2 = {0.0f, 0.0f};
    double p[J];
#pragma unroll
    for (int j = 0; j < J; ++j) p[j] = 0.0;
    if (live) {
      x1 = x1p[k];
      x2 = x2p[k];
#pragma unroll
      for (int j = 0; j < J; ++j) p[j] = Pp[(size_t)j * cells + k];
    }
    if (do_p && live) {
      double num[J], den[J];
#pragma unroll
      for (int j = 0; j < J; ++j) num[j] = den[j] = 0.0;
      for (int m = 0; m < M; ++m) {
        const double V = projet_v(projet_c(x1, x2, tb.u[m][0], tb.u[m][1]), amode, half_alpha);
        double raw, wn, wd;
        const double s = projet_sigma<J>(p, tb.g[m], raw);
        projet_weights(V, s, beta, wn, wd);
#pragma unroll
        for (int j = 0; j < J; ++j) {
          num[j] += tb.g[m][j] * wn;
          den[j] += tb.g[m][j] * wd;
        }
      }
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const double r = num[j] / (den[j] < FLOOR ? FLOOR : den[j]);
        p[j] = p[j] * (beta == 0 ? sqrt(r) : r);
        Pp[(size_t)j * cells + k] = p[j];
      }
    }
    if (!do_sums) continue;
#pragma unroll
    for (int j = 0; j < J; ++j) sP[wave][j][lane] = p[j];
#pragma unroll
    for (int t = 0; t < MAX_TILES; ++t) {
      if (t < tiles) {
        for (int i = 0; i < TILE_M; ++i) {
          const int m = t * TILE_M + i;
          double wn = 0.0, wd = 0.0;
          if (live && m < M) {
            const double V = projet_v(projet_c(x1, x2, tb.u[m][0], tb.u[m][1]), amode, half_alpha);
            double raw;
            const double s = projet_sigma<J>(p, tb.g[m], raw);
            projet_weights(V, s, beta, wn, wd);
          }
          sW[wave][i][lane] = wn;
          sW[wave][TILE_M + i][lane] = wd;
        }
        __syncthreads();
        f64x4 a = acc[t];
#pragma unroll
        for (int q = 0; q < WAVE / MFMA_CELLS; ++q) {
          const double av = sW[wave][li][q * MFMA_CELLS + lk];
          const double bv = li < J ? sP[wave][li < J ? li : 0][q * MFMA_CELLS + lk] : 0.0;
          a = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, a, 0, 0, 0);
        }
        acc[t] = a;
        __syncthreads();
      }
    }
  }
  if (!do_sums) return;

  // the four waves in ascending order, then the workgroup's partial [2][M][J]
  for (int w = 0; w < WAVES; ++w) {
    if (wave == w && li < J) {
#pragma unroll
      for (int t = 0; t < MAX_TILES; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = lk + 4 * r, kind = row / TILE_M, m = t * TILE_M + row % TILE_M;
          if (t < tiles && m < M) {
            const double v = acc[t][r];
            sOut[kind][m][li] = w == 0 ? v : sOut[kind][m][li] + v;
          }
        }
    }
    __syncthreads();
  }
  double* out = partial + (sig * ngroups + grp) * partial_doubles(M, J);
  for (int i = tid; i < 2 * M * J; i += THREADS) {
    const int kind = i / (M * J), m = (i / J) % M, j = i % J;
    out[i] = sOut[kind][m][j];
  }
}

// ---- the Q update ------------------------------------------------------------------------------------------------------------------------
// One workgroup per signal: An, Ad = the partials in ascending workgroup order from 0.0; Q[l][j]' = Q[l][j] g(sum_m K[m][l] An[m][j] /
// max(sum_m K[m][l] Ad[m][j], FLOOR)), m ascending; G = K Q'.
constexpr int Q_LOADS = 32;
__global__ __launch_bounds__(THREADS) void k_projet_q(const double* __restrict__ partial, int ngroups, const double* __restrict__ K, int M, int L, int J, int beta,
                                                       double* __restrict__ Q, double* __restrict__ G) {
#pragma clang fp contract(off)
  __shared__ double sA[2 * MAX_M * MAX_J];
  __shared__ double sQ[MAX_L * MAX_J];
  const size_t sig = blockIdx.x;
  const int n = 2 * M * J, MJ = M * J;
  const double* part = partial + sig * ngroups * n;
  for (int i = threadIdx.x; i < n; i += THREADS) {
    double s = 0.0;
    for (int g0 = 0; g0 < ngroups; g0 += Q_LOADS) {           // the loads of Q_LOADS partials in flight, the additions in order
      double v[Q_LOADS];
#pragma unroll
      for (int u = 0; u < Q_LOADS; ++u) v[u] = g0 + u < ngroups ? part[(size_t)(g0 + u) * n + i] : 0.0;
#pragma unroll
      for (int u = 0; u < Q_LOADS; ++u)
        if (g0 + u < ngroups) s += v[u];
    }
    sA[i] = s;
  }
  __syncthreads();
  double* q = Q + sig * L * J;
  for (int i = threadIdx.x; i < L * J; i += THREADS) {
    const int l = i / J, j = i % J;
    double num = K[l] * sA[j], den = K[l] * sA[MJ + j];
    for (int m = 1; m < M; ++m) {
      num += K[(size_t)m * L + l] * sA[m * J + j];
      den += K[(size_t)m * L + l] * sA[MJ + m * J + j];
    }
    const double r = num / (den < FLOOR ? FLOOR : den);
    const double v = q[i] * (beta == 0 ? sqrt(r) : r);
    sQ[i] = v;
    q[i] = v;
  }
  __syncthreads();
  projet_gains_of(K, sQ, M, L, J, G + sig * MJ);
}

// ---- the divergence ----------------------------------------------------------------------------------------------------------------------
__device__ inline double projet_dbeta(double V, double s, int beta) {
#pragma clang fp contract(off)
  if (beta == 2) {
    const double d = V - s;
    return d * d / 2.0;
  }
  if (beta == 1) return (V > 0.0 ? V * log(V / s) : 0.0) - V + s;
  const double q = (V < FLOOR ? FLOOR : V) / s;
  return q - log(q) - 1.0;
}

template <int J>
__global__ __launch_bounds__(THREADS) void k_projet_divergence(const float2* __restrict__ x, const double* __restrict__ P, int64_t cells, const double* __restrict__ U,
                                                                const double* __restrict__ G, int M, int amode, double half_alpha, int beta,
                                                                double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ Tables tb;
  __shared__ double red[THREADS];
  const int ngroups = groups(cells);
  const size_t sig = blockIdx.x / ngroups;
  const int grp = blockIdx.x % ngroups;
  projet_load_tables(tb, U, G + sig * M * J, M, J);
  __syncthreads();
  int64_t c0, c1;
  chunk_of(cells, grp, c0, c1);
  const int steps = chunk_steps(cells);
  const float2* x1p = x + sig * 2 * cells;
  const float2* x2p = x1p + cells;
  const double* Pp = P + sig * J * cells;
  double sum = 0.0;
  for (int step = 0; step < steps; ++step) {
    const int64_t k = c0 + (int64_t)step * THREADS + threadIdx.x;
    if (k >= c1) break;
    const float2 x1 = x1p[k], x2 = x2p[k];
    double p[J];
#pragma unroll
    for (int j = 0; j < J; ++j) p[j] = Pp[(size_t)j * cells + k];
    for (int m = 0; m < M; ++m) {
      const double V = projet_v(projet_c(x1, x2, tb.u[m][0], tb.u[m][1]), amode, half_alpha);
      double raw;
      const double s = projet_sigma<J>(p, tb.g[m], raw);
      sum += projet_dbeta(V, s, beta);
    }
  }
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int h = THREADS / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[sig * ngroups + grp] = red[0];
}

// d[sig] = the partials in ascending order from 0.0; a thread per signal
__global__ __launch_bounds__(THREADS) void k_projet_divergence_sum(const double* __restrict__ partial, int nsig, int ngroups, double* __restrict__ d) {
#pragma clang fp contract(off)
  const int sig = blockIdx.x * THREADS + threadIdx.x;
  if (sig >= nsig) return;
  double s = 0.0;
  for (int g = 0; g < ngroups; ++g) s += partial[(size_t)sig * ngroups + g];
  d[sig] = s;
}

// ---- the separation ----------------------------------------------------------------------------------------------------------------------
// y [nsig][J][2][rows][frames] complex64: Y_j[ch] = sum_m Up[ch][m] w_mj c_m, m ascending, each component rounded once.  Workgroup
// (sig, b) of `blocks` per signal, one thread per cell.
template <int J>
__global__ __launch_bounds__(THREADS) void k_projet_separate(const float2* __restrict__ x, const double* __restrict__ P, int64_t cells, int blocks,
                                                              const double* __restrict__ U, const double* __restrict__ Up, const double* __restrict__ G, int M,
                                                              float2* __restrict__ y) {
#pragma clang fp contract(off)
  __shared__ Tables tb;
  __shared__ double sup[2][MAX_M];
  const size_t sig = blockIdx.x / blocks;
  const int64_t k = (int64_t)(blockIdx.x % blocks) * THREADS + threadIdx.x;
  for (int i = threadIdx.x; i < 2 * M; i += THREADS) sup[i / M][i % M] = Up[i];
  projet_load_tables(tb, U, G + sig * M * J, M, J);
  __syncthreads();
  if (k >= cells) return;
  const float2 x1 = x[sig * 2 * cells + k], x2 = x[sig * 2 * cells + cells + k];
  double p[J], yr[J][2], yi[J][2];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    p[j] = P[(sig * J + j) * cells + k];
    yr[j][0] = yr[j][1] = yi[j][0] = yi[j][1] = 0.0;
  }
  for (int m = 0; m < M; ++m) {
    const Proj cm = projet_c(x1, x2, tb.u[m][0], tb.u[m][1]);
    double raw;
    const double s = projet_sigma<J>(p, tb.g[m], raw);
    const bool even = !(raw >= FLOOR);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const double w = even ? 1.0 / (double)J : p[j] * tb.g[m][j] / s;
#pragma unroll
      for (int ch = 0; ch < 2; ++ch) {
        const double t = sup[ch][m] * w;
        yr[j][ch] += t * cm.re;
        yi[j][ch] += t * cm.im;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < J; ++j)
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      float2 o;
      o.x = (float)yr[j][ch];
      o.y = (float)yi[j][ch];
      y[((sig * J + j) * 2 + ch) * cells + k] = o;
    }
}

}  // namespace glowk_projet
