// glowk: DUET (Yilmaz & Rickard 2004; `Duet` in nussl) -- blind separation of a two-channel STFT from the weighted histogram of the
// per-cell inter-channel attenuation and delay.  Formulas in include/glowk.h, design and measurements in DESIGN section 21.
//
//   k_duet_features   X -> alpha, delta, w (fp64 planes): the diagnostic and staging form
//   k_duet_wmax       the largest counted weight, one partial per workgroup (an fp64 max does not depend on order)
//   k_duet_hist       counted weights as integers rint(w 2^(s - e)), added into a per-workgroup LDS plane of 64-bit cells with integer
//                     LDS adds, the plane's non-zero cells flushed with 64-bit integer global adds: integer addition commutes, so the plane is the same
//                     bits every run, for every grid.  <true> reads X and computes the features in registers (the production path),
//                     <false> reads the three feature planes; both call duet_feature / the same counting rule, so they agree bit for bit
//   k_duet_peaks      [1 2 1] x [1 2 1] smoothing in int64 and the greedy picks, one workgroup per signal
//   k_duet_table      a_j e^{-i delta_j omega_r} and 1 / (1 + a_j^2) per (signal, source, row), fp64
//   k_duet_assign     every cell to the source with the smallest J; the masks and the masked stereo spectra in one pass
#pragma once
#include <hip/hip_runtime.h>

#include "glowk_duet_index.h"

namespace glowk_duet {

struct Feature {
  double alpha, delta, w;
};

// The features of one cell of row r (omega = omega_of(r, rows)).  fp64 after the load; no contraction, so that every kernel that
// inlines this rounds alike.  |X|^2 of fp32 components neither overflows nor underflows in fp64: m == 0 exactly when it is 0.
__device__ inline Feature duet_feature(float2 x1, float2 x2, int r, double omega, double p, double q) {
#pragma clang fp contract(off)
  Feature f = {0.0, 0.0, 0.0};
  if (r == 0) return f;
  const double a = x1.x, b = x1.y, c = x2.x, d = x2.y;
  const double p1 = a * a + b * b, p2 = c * c + d * d;
  if (p1 == 0.0 || p2 == 0.0) return f;
  const double mm = sqrt(p1) * sqrt(p2);
  f.alpha = (p2 - p1) / mm;
  f.delta = -atan2(d * a - c * b, c * a + d * b) / omega;          // the angle of X2 conj(X1)
  f.w = p == 1.0 ? mm : pow(mm, p);
  if (q != 0.0) f.w *= pow(omega, q);
  return f;
}

struct Ranges {
  double a_lo, a_hi, d_lo, d_hi;
  int n_a, n_d;
};

// The histogram cell of a feature, or -1 when it does not count.
__device__ inline int duet_cell(const Feature& f, const Ranges& g) {
  if (!weight_counts(f.w)) return -1;
  const int i = bin_of(f.alpha, g.a_lo, g.a_hi, g.n_a), j = bin_of(f.delta, g.d_lo, g.d_hi, g.n_d);
  return i < 0 || j < 0 ? -1 : i * g.n_d + j;
}

// x: [nsig, 2, rows, frames] complex64.  One thread per cell.
__global__ __launch_bounds__(256) void k_duet_features(const float2* x, int64_t total, int rows, int frames, double p, double q, double* alpha,
                                                        double* delta, double* w) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= total) return;
  const int64_t cells = (int64_t)rows * frames, sig = (unsigned)c / (unsigned)cells, k = c - sig * cells;   // c < 2^31
  const int r = (int)((unsigned)k / (unsigned)frames);
  const Feature f = duet_feature(x[sig * 2 * cells + k], x[sig * 2 * cells + cells + k], r, omega_of(r, rows), p, q);
  alpha[c] = f.alpha;
  delta[c] = f.delta;
  w[c] = f.w;
}

// What one cell reads: the two channels (fused) or the three stored features (staged).  The loads of HIST_UNROLL cells are issued
// before the first of them is used.
template <bool FUSED>
struct Raw {
  float2 x1, x2;
  double a, d, w;
};
template <bool FUSED>
__device__ inline Raw<FUSED> duet_load(const float2* x, const double* alpha, const double* delta, const double* w, int64_t sig, int64_t cells, int64_t k) {
  Raw<FUSED> raw = {};
  if (FUSED) {
    raw.x1 = x[sig * 2 * cells + k];
    raw.x2 = x[sig * 2 * cells + cells + k];
  } else {
    raw.a = alpha[sig * cells + k];
    raw.d = delta[sig * cells + k];
    raw.w = w[sig * cells + k];
  }
  return raw;
}
template <bool FUSED>
__device__ inline Feature duet_feature_of(const Raw<FUSED>& raw, int64_t k, int rows, int frames, double p, double q) {
  if (FUSED) {
    const int r = (int)((unsigned)k / (unsigned)frames);       // k < rows * frames <= 2^27
    return duet_feature(raw.x1, raw.x2, r, omega_of(r, rows), p, q);
  }
  Feature f = {raw.a, raw.d, raw.w};
  return f;
}

// Workgroup (sig, g) of `groups` strides over the signal's cells; partial[sig * groups + g] = its largest counted weight (0: none).
template <bool FUSED>
__global__ __launch_bounds__(HIST_THREADS) void k_duet_wmax(const float2* x, const double* alpha, const double* delta, const double* w, int64_t cells,
                                                             int rows, int frames, double p, double q, Ranges rg, int groups, double* partial) {
  __shared__ double red[HIST_THREADS];
  const int64_t sig = blockIdx.x / groups, stride = (int64_t)groups * HIST_THREADS;
  const int g = blockIdx.x % groups;
  double m = 0.0;
  for (int64_t k0 = (int64_t)g * HIST_THREADS + threadIdx.x; k0 < cells; k0 += HIST_UNROLL * stride) {
    Raw<FUSED> raw[HIST_UNROLL];
#pragma unroll
    for (int u = 0; u < HIST_UNROLL; ++u)
      if (k0 + u * stride < cells) raw[u] = duet_load<FUSED>(x, alpha, delta, w, sig, cells, k0 + u * stride);
#pragma unroll
    for (int u = 0; u < HIST_UNROLL; ++u)
      if (k0 + u * stride < cells) {
        const Feature f = duet_feature_of<FUSED>(raw[u], k0 + u * stride, rows, frames, p, q);
        if (duet_cell(f, rg) >= 0) m = fmax(m, f.w);
      }
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int h = HIST_THREADS / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// hist: [nsig, n_a n_d] int64, zeroed before the launch.  es: [nsig, 2] = (e, s), (0, s) for a signal without a counted weight.
template <bool FUSED>
__global__ __launch_bounds__(HIST_THREADS) void k_duet_hist(const float2* x, const double* alpha, const double* delta, const double* w, int64_t cells,
                                                             int rows, int frames, double p, double q, Ranges rg, int groups, int shift_s,
                                                             const double* partial, unsigned long long* hist, int* es) {
  extern __shared__ unsigned long long lds_plane[];           // [bins]
  __shared__ double red[HIST_THREADS];
  const int bins = rg.n_a * rg.n_d;
  const int64_t sig = blockIdx.x / groups, stride = (int64_t)groups * HIST_THREADS;
  const int g = blockIdx.x % groups;
  for (int c = threadIdx.x; c < bins; c += HIST_THREADS) lds_plane[c] = 0;
  double m = 0.0;
  for (int k = threadIdx.x; k < groups; k += HIST_THREADS) m = fmax(m, partial[sig * groups + k]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int h = HIST_THREADS / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + h]);
    __syncthreads();
  }
  const double wmax = red[0];
  const int e = wmax > 0.0 ? weight_exponent(wmax) : 0;
  if (g == 0 && threadIdx.x == 0) {
    es[2 * sig] = e;
    es[2 * sig + 1] = shift_s;
  }
  if (!(wmax > 0.0)) return;                                   // silence: the zeroed plane stands (uniform over the workgroup)
  const int shift = shift_s - e;
  for (int64_t k0 = (int64_t)g * HIST_THREADS + threadIdx.x; k0 < cells; k0 += HIST_UNROLL * stride) {
    Raw<FUSED> raw[HIST_UNROLL];
#pragma unroll
    for (int u = 0; u < HIST_UNROLL; ++u)
      if (k0 + u * stride < cells) raw[u] = duet_load<FUSED>(x, alpha, delta, w, sig, cells, k0 + u * stride);
#pragma unroll
    for (int u = 0; u < HIST_UNROLL; ++u)
      if (k0 + u * stride < cells) {
        const Feature f = duet_feature_of<FUSED>(raw[u], k0 + u * stride, rows, frames, p, q);
        const int cell = duet_cell(f, rg);
        if (cell >= 0) {
          const long long v = quantise(f.w, shift);
          if (v > 0) atomicAdd(&lds_plane[cell], (unsigned long long)v);
        }
      }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < bins; c += HIST_THREADS) {
    const unsigned long long sum = lds_plane[c];
    if (sum) atomicAdd(&hist[sig * bins + c], sum);
  }
}

// One workgroup per signal.  work: [nsig, 2, bins] int64.  The plane is assumed non-negative with every smoothed sum below 2^63
// (hist_shift sees to it for a plane of k_duet_hist).  A pick stops at a largest value <= 0.
__global__ __launch_bounds__(PEAK_THREADS) void k_duet_peaks(const long long* plane, int n_a, int n_d, int smooth, int nsrc, int dist_a, int dist_d,
                                                              long long* work, long long* smooth_out, int* peaks, int* n_found) {
  __shared__ long long best_v[PEAK_THREADS];
  __shared__ int best_c[PEAK_THREADS];
  __shared__ int pick_i[MAX_SRC], pick_j[MAX_SRC];
  __shared__ int s_found, s_stop;
  const int bins = n_a * n_d, tid = threadIdx.x;
  const int64_t sig = blockIdx.x;
  long long *A = work + sig * 2 * bins, *B = A + bins;
  for (int c = tid; c < bins; c += PEAK_THREADS) A[c] = plane[sig * bins + c];
  if (tid == 0) s_found = 0, s_stop = 0;
  __syncthreads();
  for (int pass = 0; pass < smooth; ++pass) {
    for (int c = tid; c < bins; c += PEAK_THREADS) B[c] = tap121((const int64_t*)A, c, c % n_d, n_d, 1);
    __syncthreads();
    for (int c = tid; c < bins; c += PEAK_THREADS) A[c] = tap121((const int64_t*)B, c, c / n_d, n_a, n_d);
    __syncthreads();
  }
  if (smooth_out)
    for (int c = tid; c < bins; c += PEAK_THREADS) smooth_out[sig * bins + c] = A[c];
  for (int k = 0; k < nsrc; ++k) {
    const int found = s_found;
    long long bv = 0;
    int bc = -1;
    for (int c = tid; c < bins; c += PEAK_THREADS) {          // ascending c: a strict > keeps the lowest index of a tie
      const long long v = A[c];
      if (v <= bv) continue;
      const int i = c / n_d, j = c % n_d;
      bool ex = false;
      for (int m = 0; m < found; ++m) ex = ex || excluded_by(i, j, pick_i[m], pick_j[m], dist_a, dist_d);
      if (!ex) bv = v, bc = c;
    }
    best_v[tid] = bv;
    best_c[tid] = bc;
    __syncthreads();
    for (int h = PEAK_THREADS / 2; h > 0; h >>= 1) {
      if (tid < h) {
        const long long ov = best_v[tid + h];
        const int oc = best_c[tid + h];
        if (oc >= 0 && (ov > best_v[tid] || (ov == best_v[tid] && (best_c[tid] < 0 || oc < best_c[tid])))) best_v[tid] = ov, best_c[tid] = oc;
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (best_c[0] < 0) {
        s_stop = 1;
      } else {
        pick_i[found] = best_c[0] / n_d;
        pick_j[found] = best_c[0] % n_d;
        s_found = found + 1;
      }
    }
    __syncthreads();
    if (s_stop) break;
  }
  const int found = s_found;
  for (int k = tid; k < nsrc; k += PEAK_THREADS) {
    peaks[(sig * nsrc + k) * 2] = k < found ? pick_i[k] : -1;
    peaks[(sig * nsrc + k) * 2 + 1] = k < found ? pick_j[k] : -1;
  }
  if (tid == 0) n_found[sig] = found;
}

// table: [nsig, nsrc, rows] entries of four doubles.  One thread per entry.
__global__ __launch_bounds__(256) void k_duet_table(const int* peaks, const int* n_found, int64_t total, int nsrc, int rows, Ranges rg, double* table) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= total) return;
  const int r = (int)(c % rows);
  const int64_t sj = c / rows, sig = sj / nsrc;
  const int j = (int)(sj % nsrc);
  double ec = 0.0, esn = 0.0, inv = 0.0;
  if (j < n_found[sig]) {
    const double al = bin_centre(rg.a_lo, rg.a_hi, rg.n_a, peaks[sj * 2]), de = bin_centre(rg.d_lo, rg.d_hi, rg.n_d, peaks[sj * 2 + 1]);
    const double a = (al + sqrt(al * al + 4.0)) / 2.0, ang = de * omega_of(r, rows);
    ec = a * cos(ang);
    esn = -a * sin(ang);
    inv = 1.0 / (1.0 + a * a);
  }
  table[c * 4] = ec;
  table[c * 4 + 1] = esn;
  table[c * 4 + 2] = inv;
  table[c * 4 + 3] = 0.0;
}

// x: [nsig, 2, rows, frames] complex64 -> mask [nsig, nsrc, rows, frames] float32, spec [nsig, nsrc, 2, rows, frames] complex64.
// One thread per cell; frames is the contiguous axis of every load and store.
__global__ __launch_bounds__(256) void k_duet_assign(const float2* x, int64_t total, int rows, int frames, const int* n_found, int nsrc,
                                                      const double* table, float* mask, float2* spec) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= total) return;
  const int64_t cells = (int64_t)rows * frames, sig = (unsigned)c / (unsigned)cells, k = c - sig * cells;   // c < 2^31
  const int r = (int)((unsigned)k / (unsigned)frames);
  const float2 x1 = x[sig * 2 * cells + k], x2 = x[sig * 2 * cells + cells + k];
  int n = n_found[sig];
  n = n < 0 ? 0 : n > nsrc ? nsrc : n;
  int bj = n > 0 ? 0 : -1;
  double best = 0.0;
  for (int j = 0; j < n; ++j) {
    const double* t = table + ((sig * nsrc + j) * rows + r) * 4;
    const double2 rot = *(const double2*)t;
    const double inv = t[2];
    const double re = rot.x * x1.x - rot.y * x1.y - x2.x, im = rot.x * x1.y + rot.y * x1.x - x2.y;
    const double J = (re * re + im * im) * inv;
    if (j == 0 || J < best) best = J, bj = j == 0 ? 0 : j;
  }
  const float2 zero = {0.0f, 0.0f};
  for (int j = 0; j < nsrc; ++j) {
    const int64_t o = (sig * nsrc + j) * cells + k;
    mask[o] = j == bj ? 1.0f : 0.0f;
    spec[2 * (sig * nsrc + j) * cells + k] = j == bj ? x1 : zero;
    spec[2 * (sig * nsrc + j) * cells + cells + k] = j == bj ? x2 : zero;
  }
}

}  // namespace glowk_duet
