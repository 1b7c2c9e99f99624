// glowk device code: the 2DFT separation (Seetharaman, Pishdadian & Pardo 2017) -- the real 2-D DFT of a spectrogram and its masked
// inverse as twiddle GEMMs on the fp32 matrix cores, the plane's standard deviation, and the wrap-around local max / min peak rule.
// s [nsig][rows][frames] float32, frames contiguous; R = rows, T = frames, fc = T / 2 + 1; spec [nsig][R][fc] interleaved complex64.
//
//   k_dft2_table     (cos, sin)(2 pi m / N) for m in [0, N): sincospi in fp64, rounded to float32 once
//   k_rdft_frames    Y[r][v] = sum_t x[r][t] w_T[(v t) mod T]: M = nsig R (signals batched), N = fc, K = T; x is the A operand, read
//                    straight from s; two accumulators, x cos and x (-sin)
//   k_cdft_rows      F[u][v] = sum_r Y[r][v] w_R[(u r) mod R] (forward) or its conjugate (inverse): M = R, N = fc, K = 2 R real
//                    terms per output, per signal; Y is the B operand, v contiguous; the optional mask is multiplied in as Y is
//                    loaded; the forward epilogue also writes mag = (float) sqrt((double) re re + (double) im im) for its columns
//   k_mag_mirror     mag[u][v] = mag[(R - u) % R][(T - v) % T] for v >= fc, and for 2 u > R in the self-conjugate columns: copies, never
//                    recomputed, so the plane is Hermitian in its bits
//   k_irdft_frames   out[r][t] = (1 / (R T)) sum_v c_v (Zre[r][v] cos - Zim[r][v] sin)(2 pi v t / T), c_v = 1 at v = 0 and v = T / 2,
//                    else 2; Zim of those self-conjugate columns is dropped on load; M = nsig R, N = T, K = 2 fc real terms
//   k_plane_sum / k_plane_std_final   mean and population std in fp64, per-workgroup partials added in index order
//   k_peak_cols / k_peak_rows   the separable wrap-around running max / min and the peak test
//
// The GEMMs.  One wave owns NT 32 x 32 output tiles side by side along N (2 in k_rdft_frames, 1 in k_cdft_rows, 4 in
// k_irdft_frames) for the whole K loop on v_mfma_f32_32x32x2_f32 (operand layout of k_nn_topk / k_beat_gram: lane l holds
// A[l & 31][l >> 5] and B[l >> 5][l & 31]; C column = l & 31, row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)), so every output is one fp32 fma
// chain in K order, whatever NT.  The data operand comes straight from global memory, KS = 8 K steps of loads issued before their
// MFMAs; in the stages along frames it is the A operand (rows 4 T bytes apart: one cache line per row and load, the expensive
// side), loaded once for the wave's NT tiles.  The twiddle operand is gathered from the table at the exact integer index
// (v t) mod T, stepped by a conditional subtraction (tw_step), never a float angle.  The table is staged in LDS where it fits in
// 64 KB (N <= 8192: always for rows <= 4096, for frames up to 4.4 minutes of audio; three workgroups per CU at the 45 KB of 5626
// frames), because a gather of 64 scattered 8-byte entries costs the vector cache one line per lane and LDS a few bank conflicts;
// longer tables (up to 256 KB, more than the 160 KB of LDS) stay in global memory, resident in L2.  In the complex stages the two K
// slots of one MFMA are the real and imaginary part of one term, so one table entry and one 4-byte data load per lane feed two
// MFMAs.  Rows and columns past the edge read a clamped address and are not stored; a K slot past the end multiplies a zero.  One
// barrier (after the table copy), no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glowk_dft2_index.h"
#include "glowk_repet.h"

namespace glowk_dft2 {

using glowk_repet::f32x16;
constexpr int KS = 8;                       // K steps per chunk of a GEMM loop: the loads of a chunk are issued before its MFMAs

__global__ __launch_bounds__(256) void k_dft2_table(float2* __restrict__ tab, int n) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= n) return;
  double s, c;
  sincospi(2.0 * (double)m / (double)n, &s, &c);
  tab[m] = make_float2((float)c, (float)s);
}

// C row of accumulator register r
__device__ __forceinline__ int c_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// LDS: the table is staged in LDS (T <= LDS_TAB_MAX, T * 8 bytes of dynamic LDS) and gathered from there
template <bool LDS>
__global__ __launch_bounds__(256) void k_rdft_frames(const float* __restrict__ x, int64_t M, int T, int fc, int ngroups,
                                                     const float2* __restrict__ tab, float2* __restrict__ Y) {
  extern __shared__ float2 stab[];
  if (LDS) {
    for (int i = threadIdx.x; i < T; i += 256) stab[i] = tab[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  const int64_t mt = blockIdx.x / (unsigned)ngroups;
  const int nt0 = ((int)(blockIdx.x % (unsigned)ngroups) * WAVES + wave) * NT_FWD;
  if (nt0 * TILE >= fc) return;                                   // wave-uniform; no barrier follows
  const int64_t m = mt * TILE + c;
  const float* xr = x + (m < M ? m : M - 1) * T;
  const unsigned n = (unsigned)T;
  int v[NT_FWD];
  unsigned idx[NT_FWD], step[NT_FWD];
  f32x16 re[NT_FWD], im[NT_FWD];
#pragma unroll
  for (int q = 0; q < NT_FWD; ++q) {
    v[q] = (nt0 + q) * TILE + c;
    const unsigned vc = (unsigned)(v[q] < fc ? v[q] : fc - 1);
    idx[q] = half ? vc % n : 0u;                                  // t = half
    step[q] = (2u * vc) % n;
#pragma unroll
    for (int r = 0; r < 16; ++r) re[q][r] = im[q][r] = 0.0f;
  }
  const int pairs = (T + 1) >> 1;
  int p = 0;
  for (; p + KS <= pairs; p += KS) {                              // KS steps: every load issued before the first MFMA; all t < T but
    float a[KS];                                                  // possibly the last, which the clamp and the select cover
    float2 w[NT_FWD][KS];
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int t = 2 * (p + j) + half;
      const float xv = xr[t < T ? t : T - 1];
      a[j] = t < T ? xv : 0.0f;
#pragma unroll
      for (int q = 0; q < NT_FWD; ++q) {
        w[q][j] = LDS ? stab[idx[q]] : tab[idx[q]];
        idx[q] = tw_step(idx[q], step[q], n);
      }
    }
#pragma unroll
    for (int j = 0; j < KS; ++j) {
#pragma unroll
      for (int q = 0; q < NT_FWD; ++q) {
        re[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], w[q][j].x, re[q], 0, 0, 0);
        im[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], -w[q][j].y, im[q], 0, 0, 0);
      }
    }
  }
  for (; p < pairs; ++p) {
    const int t = 2 * p + half;
    const float xv = xr[t < T ? t : T - 1];
    const float a = t < T ? xv : 0.0f;
#pragma unroll
    for (int q = 0; q < NT_FWD; ++q) {
      const float2 w = LDS ? stab[idx[q]] : tab[idx[q]];
      re[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w.x, re[q], 0, 0, 0);
      im[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, -w.y, im[q], 0, 0, 0);
      idx[q] = tw_step(idx[q], step[q], n);
    }
  }
#pragma unroll
  for (int q = 0; q < NT_FWD; ++q) {
    if (v[q] >= fc) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t mm = mt * TILE + c_row(r, half);
      if (mm < M) Y[mm * fc + v[q]] = make_float2(re[q][r], im[q][r]);
    }
  }
}

// sg = +1: times w = cos - i sin (forward); sg = -1: times its conjugate (inverse).  mask (nullable) [nsig][R][T], columns < C read.
// The table (R <= 4096 entries) is always staged in LDS: R * 8 bytes of dynamic LDS.
__global__ __launch_bounds__(256) void k_cdft_rows(const float2* __restrict__ in, const float* __restrict__ mask, int R, int C, int T, int mtiles,
                                                   int ngroups, const float2* __restrict__ tab, float sg, float2* __restrict__ out,
                                                   float* __restrict__ mag) {
  extern __shared__ float2 stab[];
  for (int i = threadIdx.x; i < R; i += 256) stab[i] = tab[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  unsigned b = blockIdx.x;
  const int nt = (int)(b % (unsigned)ngroups) * WAVES + wave;
  b /= (unsigned)ngroups;
  const int mt = (int)(b % (unsigned)mtiles);
  const int64_t sig = b / (unsigned)mtiles;
  if (nt * TILE >= C) return;                                     // wave-uniform; no barrier follows
  const int u = mt * TILE + c;
  const unsigned n = (unsigned)R, step = (unsigned)(u < R ? u : R - 1);   // u < R: already reduced
  const int v = nt * TILE + c, vc = v < C ? v : C - 1;
  const float* src = (const float*)(in + sig * R * C + vc) + half;
  const float* mk = mask ? mask + sig * R * T + vc : nullptr;
  unsigned idx = 0;                                               // r = 0
  f32x16 re, im;
#pragma unroll
  for (int r = 0; r < 16; ++r) re[r] = im[r] = 0.0f;
  int r = 0;
  for (; r + KS <= R; r += KS) {
    float y[KS];
    float2 w[KS];
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      y[j] = src[(int64_t)(r + j) * C * 2];
      if (mk) y[j] *= mk[(int64_t)(r + j) * T];
      w[j] = stab[idx];
      idx = tw_step(idx, step, n);
    }
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const float s = sg * w[j].y;
      re = __builtin_amdgcn_mfma_f32_32x32x2f32(half ? s : w[j].x, y[j], re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f32_32x32x2f32(half ? w[j].x : -s, y[j], im, 0, 0, 0);
    }
  }
  for (; r < R; ++r) {
    float y = src[(int64_t)r * C * 2];
    if (mk) y *= mk[(int64_t)r * T];
    const float2 w = stab[idx];
    const float s = sg * w.y;
    re = __builtin_amdgcn_mfma_f32_32x32x2f32(half ? s : w.x, y, re, 0, 0, 0);
    im = __builtin_amdgcn_mfma_f32_32x32x2f32(half ? w.x : -s, y, im, 0, 0, 0);
    idx = tw_step(idx, step, n);
  }
  if (v < C) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int uu = mt * TILE + c_row(r, half);
      if (uu < R) {
        out[(sig * R + uu) * C + v] = make_float2(re[r], im[r]);
        if (mag) mag[(sig * R + uu) * T + v] = (float)sqrt((double)re[r] * (double)re[r] + (double)im[r] * (double)im[r]);
      }
    }
  }
}

// the cells of the full plane that are copies: the columns v >= fc, and in the self-conjugate columns (v = 0, and v = T / 2 for even
// T, where (R - u, T - v) is again column v) the lower rows 2 u > R.  Sources are cells this kernel never writes.
__global__ __launch_bounds__(256) void k_mag_mirror(float* __restrict__ mag, int64_t total, int R, int T, int fc, int nself) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;     // (signal, u, slot)
  if (e >= total) return;
  const int w = T - fc + nself;
  const int j = (int)(e % w);
  const int64_t su = e / w;
  const int u = (int)(su % R);
  const int64_t sig = su / R;
  int v, vs;
  if (j < T - fc) {
    v = fc + j;
    vs = T - v;
  } else {
    if (2 * u <= R) return;
    v = vs = j == T - fc ? 0 : T / 2;
  }
  mag[(sig * R + u) * T + v] = mag[(sig * R + (u == 0 ? 0 : R - u)) * T + vs];
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_irdft_frames(const float2* __restrict__ Z, int64_t M, int T, int fc, int ngroups,
                                                      const float2* __restrict__ tab, float scale, float* __restrict__ out) {
  extern __shared__ float2 stab[];
  if (LDS) {
    for (int i = threadIdx.x; i < T; i += 256) stab[i] = tab[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  const int64_t mt = blockIdx.x / (unsigned)ngroups;
  const int nt0 = ((int)(blockIdx.x % (unsigned)ngroups) * WAVES + wave) * NT_INV;
  if (nt0 * TILE >= T) return;                                    // wave-uniform; no barrier follows
  const int64_t m = mt * TILE + c;
  const float* zr = (const float*)(Z + (m < M ? m : M - 1) * fc) + half;
  const unsigned n = (unsigned)T;
  const float* tw = (const float*)tab + half;                     // cos for the real parts' K slot, sin for the imaginary parts'
  int t[NT_INV];
  unsigned idx[NT_INV], step[NT_INV];
  f32x16 acc[NT_INV];
#pragma unroll
  for (int q = 0; q < NT_INV; ++q) {
    t[q] = (nt0 + q) * TILE + c;
    step[q] = (unsigned)(t[q] < T ? t[q] : T - 1);                // < T: already reduced
    idx[q] = 0;                                                   // v = 0
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;
  }
  int v = 0;
  for (; v + KS <= fc; v += KS) {
    float a[KS], w[NT_INV][KS];
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const bool self = v + j == 0 || 2 * (v + j) == T;           // a self-conjugate column: weight 1, the imaginary part dropped
      const float z = zr[2 * (v + j)];
      a[j] = half ? (self ? 0.0f : -z) : z;
#pragma unroll
      for (int q = 0; q < NT_INV; ++q) {
        const float tw_j = LDS ? ((const float*)stab)[2 * idx[q] + half] : tw[2 * idx[q]];
        w[q][j] = self ? tw_j : 2.0f * tw_j;
        idx[q] = tw_step(idx[q], step[q], n);
      }
    }
#pragma unroll
    for (int j = 0; j < KS; ++j) {
#pragma unroll
      for (int q = 0; q < NT_INV; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], w[q][j], acc[q], 0, 0, 0);
    }
  }
  for (; v < fc; ++v) {
    const bool self = v == 0 || 2 * v == T;
    const float z = zr[2 * v];
    const float a = half ? (self ? 0.0f : -z) : z;
#pragma unroll
    for (int q = 0; q < NT_INV; ++q) {
      const float w = LDS ? ((const float*)stab)[2 * idx[q] + half] : tw[2 * idx[q]];
      acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, self ? w : 2.0f * w, acc[q], 0, 0, 0);
      idx[q] = tw_step(idx[q], step[q], n);
    }
  }
#pragma unroll
  for (int q = 0; q < NT_INV; ++q) {
    if (t[q] >= T) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t mm = mt * TILE + c_row(r, half);
      if (mm < M) out[mm * T + t[q]] = acc[q][r] * scale;
    }
  }
}

// ---- mean and population standard deviation of a plane, fp64, fixed order -------------------------------------------------------------
// the sum of 256 doubles in a fixed tree; the result in every thread
__device__ __forceinline__ double block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// part[sig][b] = sum over chunk b of (x - mean)^2 (sq) or of x; mean from the first pass's partials, added in index order
__global__ __launch_bounds__(256) void k_plane_sum(const float* __restrict__ x, int64_t n, int nb, const double* __restrict__ sums, int sq,
                                                   double* __restrict__ part) {
  __shared__ double sh[256];
  const int b = blockIdx.x % (unsigned)nb;
  const int64_t sig = blockIdx.x / (unsigned)nb;
  double mean = 0.0;
  if (sq) {
    for (int i = 0; i < nb; ++i) mean += sums[sig * nb + i];
    mean /= (double)n;
  }
  int64_t first, count;
  std_chunk(n, nb, b, first, count);
  const float* p = x + sig * n + first;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) {
    const double d = (double)p[i] - mean;
    acc += sq ? d * d : d;
  }
  const double tot = block_sum(acc, sh);
  if (threadIdx.x == 0) part[sig * nb + b] = tot;
}

__global__ __launch_bounds__(64) void k_plane_std_final(const double* __restrict__ sums, const double* __restrict__ sq, int64_t n, int nb, int nsig,
                                                        double* __restrict__ out) {
  const int sig = blockIdx.x * 64 + threadIdx.x;
  if (sig >= nsig) return;
  double a = 0.0, q = 0.0;
  for (int i = 0; i < nb; ++i) a += sums[(int64_t)sig * nb + i];
  for (int i = 0; i < nb; ++i) q += sq[(int64_t)sig * nb + i];
  out[2 * sig] = a / (double)n;
  out[2 * sig + 1] = sqrt(q / (double)n);
}

// ---- the peak rule: separable wrap-around running max / min -----------------------------------------------------------------------------
__device__ __forceinline__ float sel_max(float a, float b) { return b > a ? b : a; }
__device__ __forceinline__ float sel_min(float a, float b) { return b < a ? b : a; }

// along the columns of one row: hmax / hmin [nsig][rows][cols]
__global__ __launch_bounds__(256) void k_peak_cols(const float* __restrict__ plane, int cols, int nseg, int nb_c, float* __restrict__ hmax,
                                                   float* __restrict__ hmin) {
  __shared__ float seg[PK_SEG + MAX_NB - 1];
  const int64_t row = blockIdx.x / (unsigned)nseg;               // (signal, row)
  const int c0 = (int)(blockIdx.x % (unsigned)nseg) * PK_SEG, hc = nb_c >> 1;
  const float* p = plane + row * cols;
  for (int i = threadIdx.x; i < PK_SEG + nb_c - 1; i += 256) seg[i] = p[wrap_index(c0 - hc + i, cols)];
  __syncthreads();
  const int col = c0 + threadIdx.x;
  if (col >= cols) return;
  float mx = seg[threadIdx.x], mn = mx;
  for (int d = 1; d < nb_c; ++d) {
    const float v = seg[threadIdx.x + d];
    mx = sel_max(mx, v);
    mn = sel_min(mn, v);
  }
  hmax[row * cols + col] = mx;
  hmin[row * cols + col] = mn;
}

// along the rows, then the test: mask = plane == mx && (no thr || mx - mn > thr[sig])
__global__ __launch_bounds__(256) void k_peak_rows(const float* __restrict__ plane, const float* __restrict__ hmax, const float* __restrict__ hmin, int rows,
                                                   int cols, int rtiles, int ctiles, int nb_r, const float* __restrict__ thr, float* __restrict__ mask,
                                                   float* __restrict__ max_out, float* __restrict__ min_out) {
  __shared__ float smax[PK_TR + MAX_NB - 1][PK_TC];
  __shared__ float smin[PK_TR + MAX_NB - 1][PK_TC];
  unsigned b = blockIdx.x;
  const int c0 = (int)(b % (unsigned)ctiles) * PK_TC;
  b /= (unsigned)ctiles;
  const int r0 = (int)(b % (unsigned)rtiles) * PK_TR;
  const int64_t sig = b / (unsigned)rtiles;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, hr = nb_r >> 1;
  const int col = c0 + tx, cc = col < cols ? col : cols - 1;
  const int64_t base = sig * rows * cols;
  for (int i = ty; i < PK_TR + nb_r - 1; i += 8) {
    const int64_t o = base + (int64_t)wrap_index(r0 - hr + i, rows) * cols + cc;
    smax[i][tx] = hmax[o];
    smin[i][tx] = hmin[o];
  }
  __syncthreads();
  if (col >= cols) return;
  for (int k = 0; k < PK_TR / 8; ++k) {
    const int lr = ty * (PK_TR / 8) + k, row = r0 + lr;
    if (row >= rows) break;
    float mx = smax[lr][tx], mn = smin[lr][tx];
    for (int d = 1; d < nb_r; ++d) {
      mx = sel_max(mx, smax[lr + d][tx]);
      mn = sel_min(mn, smin[lr + d][tx]);
    }
    const int64_t o = base + (int64_t)row * cols + col;
    const bool peak = plane[o] == mx && (!thr || (mx - mn) > thr[sig]);
    mask[o] = peak ? 1.0f : 0.0f;
    if (max_out) max_out[o] = mx;
    if (min_out) min_out[o] = mn;
  }
}

}  // namespace glowk_dft2
