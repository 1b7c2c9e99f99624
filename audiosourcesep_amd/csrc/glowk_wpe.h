// glowk: WPE dereverberation (Nakatani et al. 2010; Yoshioka & Nakatani 2012; `nara_wpe`) -- the late reverberation of every frequency
// row is predicted from the row's delayed past by a multichannel linear filter and subtracted.  Formulas, ranges and error bounds in
// include/glowk.h, geometry and orders in glowk_wpe_index.h, design and measurements in DESIGN section 30.
//
//   k_wpe_power    Y -> w = 1 / max(p, eps max_t p) with the row's maximum in the same launch; one workgroup per (signal, row)
//   k_wpe_corr     R = sum_t w x~ x~^H and P = sum_t w x~ x^H on v_mfma_f64_16x16x4_f64: the tiles of one triangle, the frames staged
//                  chunk by chunk in LDS with their halo; one workgroup per (signal, row), four real Gram accumulators per element
//   k_wpe_solve    the loading, R = L L^H, G = R^-1 P and the status word; one wave per (signal, row), the triangle in LDS
//   k_wpe_filter   y = x - G^H x~ from the same staging; one workgroup per (signal, row, chunk)
//
// Everything after the float32 load is fp64 without contraction (the matrix-core instruction is the one fused operation); every order
// is fixed by the shapes; no atomics, no spin waits; a workgroup never reads what another one of its launch writes.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "glowk_wpe_index.h"

namespace glowk_wpe {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---- the power and its inverse ---------------------------------------------------------------------------------------------------------
// q(t) = (sum_m re^2 + im^2) / M, m ascending
__device__ inline double wpe_q(const float2* __restrict__ yr, size_t plane, int M, int t) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int m = 0; m < M; ++m) {
    const float2 v = yr[(size_t)m * plane + t];
    const double re = (double)v.x, im = (double)v.y;
    s += re * re + im * im;
  }
  return s / (double)M;
}
// p(t): q(t), or its mean over the frames of [t - context, t + context] that exist, ascending
__device__ inline double wpe_p(const float2* __restrict__ yr, size_t plane, int M, int frames, int context, int t) {
#pragma clang fp contract(off)
  if (context == 0) return wpe_q(yr, plane, M, t);
  const int lo = t - context < 0 ? 0 : t - context, hi = t + context > frames - 1 ? frames - 1 : t + context;
  double s = wpe_q(yr, plane, M, lo);
  for (int u = lo + 1; u <= hi; ++u) s += wpe_q(yr, plane, M, u);
  return s / (double)(hi - lo + 1);
}
// the larger of two, a NaN once seen for good
__device__ inline double wpe_max(double a, double b) { return (b > a || b != b) ? b : a; }

__global__ __launch_bounds__(THREADS) void k_wpe_power(const float2* __restrict__ y, int M, int rows, int frames, int context, double eps, double* __restrict__ w,
                                                        double* __restrict__ pmax) {
#pragma clang fp contract(off)
  __shared__ double smax[THREADS];
  const int64_t sr = blockIdx.x;
  const int64_t sig = sr / rows, row = sr % rows;
  const size_t plane = (size_t)rows * frames;
  const float2* yr = y + ((size_t)sig * M * rows + row) * frames;
  const int tid = threadIdx.x;
  double mx = 0.0;
  for (int t = tid; t < frames; t += THREADS) mx = wpe_max(mx, wpe_p(yr, plane, M, frames, context, t));
  smax[tid] = mx;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) smax[tid] = wpe_max(smax[tid], smax[tid + s]);
    __syncthreads();
  }
  const double pm = smax[0];
  const bool ok = pm > 0.0 && pm < INFINITY;
  const double floor = eps * pm;
  double* wr = w + (size_t)sr * frames;
  for (int t = tid; t < frames; t += THREADS) {
    const double p = wpe_p(yr, plane, M, frames, context, t);
    wr[t] = ok ? 1.0 / (p < floor ? floor : p) : 0.0;
  }
  if (pmax && tid == 0) pmax[sr] = pm;
}

// ---- the staging of a chunk ------------------------------------------------------------------------------------------------------------
struct Stage {
  double a[MAX_M][MAX_COLS];   // real parts: column j is frame c0 - halo + j
  double b[MAX_M][MAX_COLS];   // imaginary parts
  double w[CHUNK];             // the weights of frames c0 .. c0 + CHUNK - 1
};
__device__ inline void wpe_stage(Stage& s, const float2* __restrict__ xr, size_t plane, int M, int frames, int c0, int H, const double* __restrict__ wr) {
  const int cols = CHUNK + H;
  for (int i = threadIdx.x; i < M * cols; i += THREADS) {
    const int m = i / cols, j = i - m * cols, t = stage_frame(c0, H, j, frames);
    float2 v = {0.0f, 0.0f};
    if (t >= 0) v = xr[(size_t)m * plane + t];
    s.a[m][j] = (double)v.x;
    s.b[m][j] = (double)v.y;
  }
  if (wr)
    for (int i = threadIdx.x; i < CHUNK; i += THREADS) s.w[i] = c0 + i < frames ? wr[c0 + i] : 0.0;
}

// ---- the correlations --------------------------------------------------------------------------------------------------------------------
// With z = a + i b, C[i][j] = sum_t w z_i conj(z_j) = (Gaa + Gbb) + i (Gba - Gab), the four real Gram sums Gpq[i][j] = sum_t (w p_i) q_j,
// each in an accumulator of its own (a chain of `frames` products), combined once at the end.  For the four frames 4 s + k of a step,
// operand A is A[i = lane & 15][k = lane >> 4] = w a_i (or w b_i) of the tile's rows, operand B is B[k = lane >> 4][j = lane & 15] = a_j
// (or b_j) of the tile's columns, result register r holds the element [i = (lane >> 4) + 4 r][j = lane & 15].  Rows from D on, columns
// from E on and frames from `frames` on are zeros.
__global__ __launch_bounds__(THREADS) void k_wpe_corr(const float2* __restrict__ x, const double* __restrict__ w, int M, int K, int delay, int rows, int frames,
                                                       double2* __restrict__ R, double2* __restrict__ P) {
#pragma clang fp contract(off)
  __shared__ Stage st;
  const int64_t sr = blockIdx.x;
  const int64_t sig = sr / rows, row = sr % rows;
  const size_t plane = (size_t)rows * frames;
  const float2* xr = x + ((size_t)sig * M * rows + row) * frames;
  const double* wr = w + (size_t)sr * frames;
  const int D = stacked(M, K), E = elements(M, K), H = halo(K, delay), npairs = pairs(M, K);
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int li = lane & 15, lk = lane >> 4;
  const double* sa = &st.a[0][0];
  const double* sb = &st.b[0][0];

  int offA[PAIRS_PER_WAVE], offB[PAIRS_PER_WAVE];     // where the lane's row of A and column of B start in a plane, -1 for a zero
  f64x4 gaa[PAIRS_PER_WAVE], gbb[PAIRS_PER_WAVE], gba[PAIRS_PER_WAVE], gab[PAIRS_PER_WAVE];
#pragma unroll
  for (int q = 0; q < PAIRS_PER_WAVE; ++q) {
    gaa[q] = gbb[q] = gba[q] = gab[q] = f64x4{0.0, 0.0, 0.0, 0.0};
    offA[q] = offB[q] = -1;
    const int p = wave + q * WAVES;
    if (p < npairs) {
      int I, J;
      pair_of(M, K, p, I, J);
      const int eA = I * TILE + li, eB = J * TILE + li;
      if (eA < D) offA[q] = lane_offset(eA, M, K, delay);
      if (eB < E) offB[q] = lane_offset(eB, M, K, delay);
    }
  }

  const int nchunks = frame_chunks(frames);
  for (int c = 0; c < nchunks; ++c) {
    const int c0 = c * CHUNK;
    __syncthreads();
    wpe_stage(st, xr, plane, M, frames, c0, H, wr);
    __syncthreads();
    const int steps = chunk_steps(c0, frames);
    for (int s = 0; s < steps; ++s) {
      const int col = s * MFMA_FRAMES + lk;
      const double wv = st.w[col];
#pragma unroll
      for (int q = 0; q < PAIRS_PER_WAVE; ++q) {
        if (wave + q * WAVES < npairs) {                                // the same in every lane of the wave
          const double ai = offA[q] >= 0 ? sa[offA[q] + col] : 0.0, bi = offA[q] >= 0 ? sb[offA[q] + col] : 0.0;
          const double aj = offB[q] >= 0 ? sa[offB[q] + col] : 0.0, bj = offB[q] >= 0 ? sb[offB[q] + col] : 0.0;
          const double wa = wv * ai, wb = wv * bi;
          gaa[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa, aj, gaa[q], 0, 0, 0);
          gbb[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wb, bj, gbb[q], 0, 0, 0);
          gba[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wb, aj, gba[q], 0, 0, 0);
          gab[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa, bj, gab[q], 0, 0, 0);
        }
      }
    }
  }

  // every element of R and P is stored once, by the lane that holds it (or its conjugate): tile by tile
  double2* Rr = R + (size_t)sr * D * D;
  double2* Pr = P + (size_t)sr * D * M;
#pragma unroll
  for (int q = 0; q < PAIRS_PER_WAVE; ++q) {
    const int p = wave + q * WAVES;
    if (p < npairs) {
      int I, J;
      pair_of(M, K, p, I, J);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = lane_row(I, lane, r), j = lane_col(J, lane);
        const double re = gaa[q][r] + gbb[q][r], im = gba[q][r] - gab[q][r];
        switch (store_target(i, j, D, E)) {
          case STORE_UPPER:
            Rr[(size_t)i * D + j] = make_double2(re, im);
            Rr[(size_t)j * D + i] = make_double2(re, -im);
            break;
          case STORE_DIAG: Rr[(size_t)i * D + i] = make_double2(re, 0.0); break;
          case STORE_P: Pr[(size_t)i * M + (j - D)] = make_double2(re, im); break;
          default: break;
        }
      }
    }
  }
}

// ---- the solve ---------------------------------------------------------------------------------------------------------------------------
// Thread i owns row i.  The loading: tr = sum_i Re R[i][i] ascending, R[i][i] += loading (tr / D).  The factor by columns (Cholesky-Crout):
// s = R[i][j] - sum_{k < j} L[i][k] conj(L[j][k]), k ascending; L[j][j] = sqrt(Re s), L[i][j] = s / L[j][j].  Then L Z = P by columns
// (z_j = b_j / L[j][j], b_i -= L[i][j] z_j) and L^H G = Z from the last column up (g_j = b_j / L[j][j], b_i -= conj(L[j][i]) g_j).
__global__ __launch_bounds__(SOLVE_THREADS) void k_wpe_solve(const double2* __restrict__ R, const double2* __restrict__ P, int D, int M, double loading,
                                                              double2* __restrict__ G, int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ double2 sl[TRI_MAX];
  __shared__ double2 sz[MAX_M];
  __shared__ double sd;
  __shared__ int sbad;
  const size_t sr = blockIdx.x;
  const double2* Rr = R + sr * D * D;
  const double2* Pr = P + sr * D * M;
  const int i = threadIdx.x;
  for (int r = 0; r < D; ++r)
    for (int j = i; j <= r; j += SOLVE_THREADS) sl[tri(r, j)] = Rr[(size_t)r * D + j];
  if (i == 0) sbad = 0;
  __syncthreads();
  double tr = 0.0;
  for (int r = 0; r < D; ++r) tr += sl[tri(r, r)].x;
  const double lam = loading * (tr / (double)D);
  __syncthreads();
  if (i < D) sl[tri(i, i)].x += lam;
  __syncthreads();

  for (int j = 0; j < D; ++j) {
    double2 s = make_double2(0.0, 0.0);
    if (i >= j && i < D) {
      s = sl[tri(i, j)];
      for (int k = 0; k < j; ++k) {
        const double2 a = sl[tri(i, k)], c = sl[tri(j, k)];
        s.x = s.x - a.x * c.x;
        s.x = s.x - a.y * c.y;
        s.y = s.y - a.y * c.x;
        s.y = s.y + a.x * c.y;
      }
    }
    if (i == j) {
      const bool ok = s.x > 0.0 && s.x < INFINITY;
      if (!ok) sbad = 1;
      sd = ok ? sqrt(s.x) : 1.0;
    }
    __syncthreads();
    const double d = sd;
    if (i == j) sl[tri(j, j)] = make_double2(d, 0.0);
    else if (i > j && i < D) sl[tri(i, j)] = make_double2(s.x / d, s.y / d);
    __syncthreads();
  }

  double2 b[MAX_M];
#pragma unroll
  for (int m = 0; m < MAX_M; ++m) b[m] = (i < D && m < M) ? Pr[(size_t)i * M + m] : make_double2(0.0, 0.0);
  for (int j = 0; j < D; ++j) {
    if (i == j) {
      const double d = sl[tri(j, j)].x;
#pragma unroll
      for (int m = 0; m < MAX_M; ++m) {
        b[m] = make_double2(b[m].x / d, b[m].y / d);
        sz[m] = b[m];
      }
    }
    __syncthreads();
    if (i > j && i < D) {
      const double2 l = sl[tri(i, j)];
#pragma unroll
      for (int m = 0; m < MAX_M; ++m) {
        const double2 z = sz[m];
        b[m].x = b[m].x - l.x * z.x;
        b[m].x = b[m].x + l.y * z.y;
        b[m].y = b[m].y - l.x * z.y;
        b[m].y = b[m].y - l.y * z.x;
      }
    }
    __syncthreads();
  }
  for (int j = D - 1; j >= 0; --j) {
    if (i == j) {
      const double d = sl[tri(j, j)].x;
#pragma unroll
      for (int m = 0; m < MAX_M; ++m) {
        b[m] = make_double2(b[m].x / d, b[m].y / d);
        sz[m] = b[m];
      }
    }
    __syncthreads();
    if (i < j) {
      const double2 l = sl[tri(j, i)];
#pragma unroll
      for (int m = 0; m < MAX_M; ++m) {
        const double2 g = sz[m];
        b[m].x = b[m].x - l.x * g.x;
        b[m].x = b[m].x - l.y * g.y;
        b[m].y = b[m].y - l.x * g.y;
        b[m].y = b[m].y + l.y * g.x;
      }
    }
    __syncthreads();
  }
  const bool bad = sbad != 0;
  if (i < D) {
#pragma unroll
    for (int m = 0; m < MAX_M; ++m)
      if (m < M) G[(sr * D + i) * M + m] = bad ? make_double2(0.0, 0.0) : b[m];
  }
  if (i == 0) status[sr] = bad ? STATUS_PIVOT : STATUS_OK;
}

// ---- the filter --------------------------------------------------------------------------------------------------------------------------
// y_m(t) = x_m(t) - sum_e conj(G[e][m]) x~_e(t), e ascending, each component rounded once to float32.  A row whose G is all zeros is
// copied: the pass-through of a flagged row is exact whatever X holds.
__global__ __launch_bounds__(THREADS) void k_wpe_filter(const float2* __restrict__ x, const double2* __restrict__ G, int M, int K, int delay, int rows, int frames,
                                                         float2* __restrict__ y) {
#pragma clang fp contract(off)
  __shared__ Stage st;
  __shared__ double2 sg[MAX_D * MAX_M];
  const int nch = frame_chunks(frames);
  const int64_t sr = blockIdx.x / nch;
  const int c0 = (int)(blockIdx.x % nch) * CHUNK;
  const int64_t sig = sr / rows, row = sr % rows;
  const size_t plane = (size_t)rows * frames;
  const float2* xr = x + ((size_t)sig * M * rows + row) * frames;
  float2* yr = y + ((size_t)sig * M * rows + row) * frames;
  const int D = stacked(M, K), H = halo(K, delay), tid = threadIdx.x;
  int any = 0;
  for (int i = tid; i < D * M; i += THREADS) {
    const double2 g = G[(size_t)sr * D * M + i];
    sg[i] = g;
    any |= (g.x != 0.0 || g.y != 0.0) ? 1 : 0;
  }
  any = __syncthreads_or(any);
  const int t = c0 + tid;
  if (!any) {
    if (t < frames)
      for (int m = 0; m < M; ++m) yr[(size_t)m * plane + t] = xr[(size_t)m * plane + t];
    return;
  }
  wpe_stage(st, xr, plane, M, frames, c0, H, nullptr);
  __syncthreads();
  if (t >= frames) return;
  const int col = tid + H;
  double sre[MAX_M], sim[MAX_M];
#pragma unroll
  for (int m = 0; m < MAX_M; ++m) sre[m] = sim[m] = 0.0;
  for (int k = 0, e = 0; k < K; ++k) {
    for (int mm = 0; mm < M; ++mm, ++e) {
      const int at = stage_col(tid, H, delay + k);
      const double a = st.a[mm][at], bb = st.b[mm][at];
#pragma unroll
      for (int m = 0; m < MAX_M; ++m) {
        if (m < M) {
          const double2 g = sg[e * M + m];
          sre[m] = sre[m] + g.x * a;
          sre[m] = sre[m] + g.y * bb;
          sim[m] = sim[m] + g.x * bb;
          sim[m] = sim[m] - g.y * a;
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MAX_M; ++m)
    if (m < M) yr[(size_t)m * plane + t] = make_float2((float)(st.a[m][col] - sre[m]), (float)(st.b[m][col] - sim[m]));
}

}  // namespace glowk_wpe
