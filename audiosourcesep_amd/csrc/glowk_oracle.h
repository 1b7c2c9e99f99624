// glowk device code: the oracle separation systems (oracle_systems.py, from sigsep-mus-oracle) -- the ideal binary and ratio
// masks, the multichannel Wiener filter and the two mel-domain masks -- with an STFT / iSTFT pair in scipy.signal's conventions
// (nperseg 2048: periodic Hann, hop 1024, 1024 zeros on each side, zero-padded to whole frames, scaled by 1 / sum(win)).
//
// Spectra are [sig][1025][T] complex (re/im interleaved, frame fastest), T = ceil(n / 1024) + 1.  One call's signals are the
// mixture's channels (rows 0 .. nchan-1) followed by source j's channels (rows nchan + j nchan + c); the mask and MWF kernels
// overwrite the source rows with the masked or filtered mixture, which k_sp_istft then inverts.
//
//   k_sp_stft       X[s][b][t] = 2^-10 sum_m hann[m] x_s[1024 (t - 1) + m] e^{-2 pi i b m / 2048}: a GEMM on v_mfma_f32_32x32x2_f32
//                   with the DFT basis from the 2048-entry table at the exact integer phase (b m) mod 2048 (as k_stft)
//   k_oracle_mask   IBM: Y_j = X [|Y_j|^a / (eps + |X|^a) >= theta];  IRM: Y_j = X |Y_j|^a / (eps + sum_k |Y_k|^a); fp64
//   k_mwf_stats     R_j(f) = mean_t Y Y^H / (eps + mean_c |Y_c|^2): fp64, one workgroup per (source, bin), a fixed-order tree
//   k_mwf_norm      the reference's normalisation by np.trace of the [F, 2, 2] array (column k of every R_j(f) times
//                   2 / (R_j(0)[0][k] + R_j(1)[1][k])), + eps I, and R_j^-1 (2 x 2, eps added to the determinant)
//   k_mwf_gain      per (f, t): P_j = Re tr(R_j^-1 Y Y^H) / 2, Cxx = sum_j P_j R_j, Y_j = G_j X with G_j = P_j R_j Cxx^-1; fp64,
//                   except that G_j is held in complex64 as the reference holds it (its rounding moves the estimates by ~1e-4)
//   k_sp_istft      irfft x sum(win) as a GEMM on the same MFMA, overlap-add of the 2 frames of each sample (the earlier frame
//                   first), divided by the overlap-added win^2, the 1024-sample trim, cut to the requested length
//   k_oracle_mel    the mel variants, elementwise: the source sum in the input dtype, the rest in fp64, one rounding
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "glowk_audio.h"

namespace glowk_oracle {

using glowk_audio::AudioConsts;
using glowk_audio::f32x16;
constexpr int NFFT = 2048, HOP = 1024, NBIN = NFFT / 2 + 1;
constexpr int MWF_MAX_SRC = 16;
constexpr double EPS = 2.220446049250313e-16;           // np.finfo(np.float64).eps

__host__ __device__ inline int64_t sp_frames(int64_t n) { return (n + HOP - 1) / HOP + 1; }

// ---- STFT: one wave = 32 bins x 32 frames (re and im accumulators), 4 waves = 128 bins; K = 2048 samples in chunks of 256 ---------
constexpr int SP_KC = 256, SP_PITCH = SP_KC + 1;

__global__ __launch_bounds__(256) void k_sp_stft(const float* __restrict__ x, int64_t n, int T, int ftiles, AudioConsts c,
                                                 float2* __restrict__ spec) {
  __shared__ float tab[NFFT];
  __shared__ float fs[32 * SP_PITCH];                // 32 windowed frames x 256 samples of the current chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t sig = blockIdx.x / ftiles;
  const int f0 = (blockIdx.x % ftiles) * 32;
  const int bin0 = blockIdx.y * 128 + wave * 32;
  const float* a = x + sig * n;
  for (int i = tid; i < NFFT; i += 256) tab[i] = c.tab[i];
  f32x16 acc_re = {}, acc_im = {};
  const int bin = bin0 + (lane & 31), half = lane >> 5;
  for (int n0 = 0; n0 < NFFT; n0 += SP_KC) {
    __syncthreads();                                 // the previous chunk has been consumed
    for (int i = tid; i < 32 * SP_KC; i += 256) {
      const int fr = i / SP_KC, nn = i % SP_KC, f = f0 + fr;
      const int64_t idx = (int64_t)(f - 1) * HOP + n0 + nn;   // 1024 zeros of padding in front, zeros past the end
      float v = 0.0f;
      if (f < T && idx >= 0 && idx < n) v = a[idx] * c.win[n0 + nn];
      fs[fr * SP_PITCH + nn] = v;
    }
    __syncthreads();
    if (bin0 < NBIN) {                               // wave-uniform: the last block's spare waves only help stage
#pragma unroll 8
      for (int kk = 0; kk < SP_KC / 2; ++kk) {
        const int nl = 2 * kk + half;
        const int m = (bin * (n0 + nl)) & (NFFT - 1);
        const float b = fs[(lane & 31) * SP_PITCH + nl];
        acc_re = __builtin_amdgcn_mfma_f32_32x32x2f32(tab[m], b, acc_re, 0, 0, 0);
        acc_im = __builtin_amdgcn_mfma_f32_32x32x2f32(tab[(m + 512) & (NFFT - 1)], b, acc_im, 0, 0, 0);
      }
    }
  }
  if (bin0 >= NBIN) return;
  const int f = f0 + (lane & 31);                    // C/D: column = lane & 31 (frame), row = (r & 3) + 8 (r >> 2) + 4 half (bin)
  if (f >= T) return;
  const float scale = 1.0f / 1024.0f;                // 1 / sum(win), a power of two: exact
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int b = bin0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (b >= NBIN) continue;
    spec[(sig * NBIN + b) * T + f] = make_float2(acc_re[r] * scale, acc_im[r] * scale);
  }
}

// ---- IBM / IRM masks, fp64, in place on the source rows; the IBM mask bits optionally to mask [nsrc][nchan][1025][T] ---------------
__device__ __forceinline__ double spec_pow(float2 v, double alpha) {
  const double m = sqrt((double)v.x * v.x + (double)v.y * v.y);
  return alpha == 1.0 ? m : alpha == 2.0 ? m * m : pow(m, alpha);
}

__device__ __forceinline__ double binary_mask(double ratio, double theta) {   // the reference's two assignments, in order
  double m = ratio >= theta ? 1.0 : ratio;
  return m < theta ? 0.0 : m;
}

struct MaskArgs {
  float2* spec = nullptr;
  int64_t plane = 0;                                     // 1025 T
  int nsrc = 0, nchan = 0, irm = 0;
  double alpha = 0.0, theta = 0.0;
  uint8_t* mask = nullptr;                                     // nullable (IBM only)
};
static_assert(sizeof(MaskArgs) == 56 && std::is_trivially_copyable_v<MaskArgs>, "kernel argument size");

__global__ __launch_bounds__(256) void k_oracle_mask(MaskArgs a) {
  const int64_t total = (int64_t)a.nchan * a.plane;  // one thread per (channel, bin, frame): every source of it
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t ch = i / a.plane, o = i % a.plane;
    const float2 X = a.spec[i];
    double model = EPS, px = 0.0;
    if (a.irm) {
      for (int j = 0; j < a.nsrc; ++j) model += spec_pow(a.spec[(a.nchan + (int64_t)j * a.nchan + ch) * a.plane + o], a.alpha);
    } else {
      px = EPS + spec_pow(X, a.alpha);
    }
    for (int j = 0; j < a.nsrc; ++j) {
      const int64_t row = a.nchan + (int64_t)j * a.nchan + ch;
      const double p = spec_pow(a.spec[row * a.plane + o], a.alpha);
      double m;
      if (a.irm) {
        m = p / model;
      } else {
        m = binary_mask(p / px, a.theta);
        if (a.mask) a.mask[((int64_t)j * a.nchan + ch) * a.plane + o] = m != 0.0 ? 1 : 0;
      }
      a.spec[row * a.plane + o] = make_float2((float)(X.x * m), (float)(X.y * m));
    }
  }
}

// ---- MWF (stereo).  Complex fp64 2 x 2 matrices as [a][b] -> double2 ----------------------------------------------------------------
struct c2 { double2 m[2][2]; };

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cscale(double s, double2 a) { return make_double2(s * a.x, s * a.y); }
__device__ __forceinline__ double2 cdiv(double2 a, double2 b) {
  const double d = b.x * b.x + b.y * b.y;
  return make_double2((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}

__device__ __forceinline__ double2 round_c64(double2 a) { return make_double2((double)(float)a.x, (double)(float)a.y); }

__device__ __forceinline__ c2 inv2(const c2& M) {     // the reference's invert: 1 / (eps + m00 m11 - m01 m10) times the adjugate
  const double2 det = csub(cadd(make_double2(EPS, 0.0), cmul(M.m[0][0], M.m[1][1])), cmul(M.m[0][1], M.m[1][0]));
  const double2 inv = cdiv(make_double2(1.0, 0.0), det);
  c2 r;
  r.m[0][0] = cmul(inv, M.m[1][1]);
  r.m[1][0] = cmul(inv, make_double2(-M.m[1][0].x, -M.m[1][0].y));
  r.m[0][1] = cmul(inv, make_double2(-M.m[0][1].x, -M.m[0][1].y));
  r.m[1][1] = cmul(inv, M.m[0][0]);
  return r;
}

__device__ __forceinline__ c2 load_c2(const double2* p) {
  c2 r;
  r.m[0][0] = p[0]; r.m[0][1] = p[1]; r.m[1][0] = p[2]; r.m[1][1] = p[3];
  return r;
}

// stats [nsrc][1025][4] = mean_t of (|Y0|^2, |Y1|^2, Re Y0 conj Y1, Im Y0 conj Y1) / (eps + P)
constexpr int MS_THREADS = 256;

__global__ __launch_bounds__(MS_THREADS) void k_mwf_stats(const float2* __restrict__ spec, int T, double* __restrict__ stats) {
  __shared__ double red[4][MS_THREADS];
  const int tid = threadIdx.x, f = blockIdx.x, j = blockIdx.y;
  const int64_t plane = (int64_t)NBIN * T;
  const float2* y0 = spec + (2 + 2 * (int64_t)j) * plane + (int64_t)f * T;
  const float2* y1 = y0 + plane;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int t = tid; t < T; t += MS_THREADS) {
    const float2 a = y0[t], b = y1[t];
    const double ar = a.x, ai = a.y, br = b.x, bi = b.y;
    const double p0 = ar * ar + ai * ai, p1 = br * br + bi * bi;
    const double den = EPS + (p0 + p1) / 2.0;
    s[0] += p0 / den;
    s[1] += p1 / den;
    s[2] += (ar * br + ai * bi) / den;               // Y0 conj(Y1)
    s[3] += (ai * br - ar * bi) / den;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k][tid] = s[k];
  __syncthreads();
  for (int w = MS_THREADS / 2; w > 0; w >>= 1) {      // fixed-order tree: bitwise reproducible
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + w];
    }
    __syncthreads();
  }
  if (tid < 4) stats[((int64_t)j * NBIN + f) * 4 + tid] = red[tid][0] / T;
}

__device__ __forceinline__ c2 stats_matrix(const double* s) {
  c2 r;
  r.m[0][0] = make_double2(s[0], 0.0);
  r.m[1][1] = make_double2(s[1], 0.0);
  r.m[0][1] = make_double2(s[2], s[3]);
  r.m[1][0] = make_double2(s[2], -s[3]);
  return r;
}

// rmat [nsrc][1025][2][4] double2: R_j(f) (normalised, + eps I), then R_j(f)^-1
__global__ __launch_bounds__(256) void k_mwf_norm(const double* __restrict__ stats, int nsrc, double2* __restrict__ rmat) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nsrc * NBIN) return;
  const int j = i / NBIN;
  const c2 R0 = stats_matrix(stats + (int64_t)j * NBIN * 4), R1 = stats_matrix(stats + ((int64_t)j * NBIN + 1) * 4);
  c2 R = stats_matrix(stats + (int64_t)i * 4);
  for (int k = 0; k < 2; ++k) {                       // np.trace(R[j]) over axes 0 and 1: c[k] = R(0)[0][k] + R(1)[1][k]
    const double2 tr = cadd(R0.m[0][k], R1.m[1][k]);
    for (int a = 0; a < 2; ++a) R.m[a][k] = cdiv(cscale(2.0, R.m[a][k]), tr);
  }
  R.m[0][0].x += EPS;
  R.m[1][1].x += EPS;
  const c2 Ri = inv2(R);
  double2* o = rmat + (int64_t)i * 8;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      o[2 * a + b] = R.m[a][b];
      o[4 + 2 * a + b] = Ri.m[a][b];
    }
}

__device__ __forceinline__ double refined_psd(const c2& Ri, float2 a, float2 b) {   // Re tr(R^-1 Y Y^H) / 2
  const double2 y[2] = {make_double2(a.x, a.y), make_double2(b.x, b.y)};
  double p = 0.0;
  for (int i1 = 0; i1 < 2; ++i1)
    for (int i2 = 0; i2 < 2; ++i2) {
      const double2 r = cmul(y[i2], make_double2(y[i1].x, -y[i1].y));   // Rjj[i2][i1] = Y_i2 conj(Y_i1)
      p += 0.5 * (Ri.m[i1][i2].x * r.x - Ri.m[i1][i2].y * r.y);
    }
  return p;
}

__global__ __launch_bounds__(256) void k_mwf_gain(float2* __restrict__ spec, int nsrc, int T, const double2* __restrict__ rmat) {
  const int64_t plane = (int64_t)NBIN * T;
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < plane; o += (int64_t)gridDim.x * 256) {
    const int f = (int)(o / T);
    const float2 x0 = spec[o], x1 = spec[plane + o];
    c2 C;
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b) C.m[a][b] = make_double2(0.0, 0.0);
    for (int j = 0; j < nsrc; ++j) {
      const int64_t row = 2 + 2 * (int64_t)j;
      const double2* rm = rmat + ((int64_t)j * NBIN + f) * 8;
      const double p = refined_psd(load_c2(rm + 4), spec[row * plane + o], spec[(row + 1) * plane + o]);
      const c2 R = load_c2(rm);
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) C.m[a][b] = cadd(C.m[a][b], cscale(p, R.m[a][b]));
    }
    const c2 Ci = inv2(C);
    const double2 X[2] = {make_double2(x0.x, x0.y), make_double2(x1.x, x1.y)};
    for (int j = 0; j < nsrc; ++j) {                  // recomputes P_j bit for bit, then overwrites this (f, t) of source j
      const int64_t row = 2 + 2 * (int64_t)j;
      const double2* rm = rmat + ((int64_t)j * NBIN + f) * 8;
      const double p = refined_psd(load_c2(rm + 4), spec[row * plane + o], spec[(row + 1) * plane + o]);
      const c2 R = load_c2(rm);
      for (int a = 0; a < 2; ++a) {
        double2 y = make_double2(0.0, 0.0);
        for (int i = 0; i < 2; ++i) {
          double2 g = make_double2(0.0, 0.0);        // G = (P R) Cxx^-1, held in complex64 as the reference's G: each += rounds
          for (int k = 0; k < 2; ++k) g = round_c64(cadd(g, cmul(cscale(p, R.m[a][k]), Ci.m[k][i])));
          y = cadd(y, cmul(g, X[i]));
        }
        spec[(row + a) * plane + o] = make_float2((float)y.x, (float)y.y);
      }
    }
  }
}

// ---- iSTFT.  Output hop block h (padded samples [1024 h, 1024 h + 1024), h = 1 .. T-1) gathers frame h - 1 at offset 1024 + u and
// frame h at offset u: out = (win[1024 + u] C_1 + win[u] C_0) / (win[u]^2 + win[1024 + u]^2), C_q = sum_b Y[b] basis[b][1024 q + u].
// One wave = 32 hop blocks x 32 samples; 4 waves = 128 samples; the spectra of the 33 frames a tile touches are staged in LDS with
// irfft's weights (DC and Nyquist once and real, the others twice; times sum(win) / 2048 = 1/2), 41 bins at a time (1025 = 25 x 41).
constexpr int SI_BC = 41, SI_ROWS = 33, SI_PITCH = 2 * SI_BC + 1;

__global__ __launch_bounds__(256) void k_sp_istft(const float2* __restrict__ spec, int T, int htiles, int64_t length, AudioConsts c,
                                                  float* __restrict__ out) {
  __shared__ float tab[NFFT];
  __shared__ float sp[SI_ROWS * SI_PITCH];           // [frame - fbase][2 (b - b0) + re/im]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, i = lane & 31;
  const int64_t sig = blockIdx.x / htiles;
  const int ht = blockIdx.x % htiles;
  const int u0 = blockIdx.y * 128 + wave * 32;
  const int fbase = ht * 32;                         // hop block h = 1 + 32 ht + i needs frames h - 1, h: rows i, i + 1
  const float2* X = spec + sig * NBIN * (int64_t)T;
  for (int k = tid; k < NFFT; k += 256) tab[k] = c.tab[k];
  f32x16 acc[2] = {{}, {}};
  for (int b0 = 0; b0 < NBIN; b0 += SI_BC) {
    __syncthreads();
    for (int k = tid; k < SI_BC * SI_ROWS; k += 256) {
      const int bl = k / SI_ROWS, ri = k % SI_ROWS, b = b0 + bl, fr = fbase + ri;
      float yr = 0.0f, yi = 0.0f;
      if (fr < T) {
        const float2 v = X[(int64_t)b * T + fr];
        const bool edge = b == 0 || b == NBIN - 1;
        yr = edge ? 0.5f * v.x : v.x;
        yi = edge ? 0.0f : v.y;
      }
      sp[ri * SI_PITCH + 2 * bl] = yr;
      sp[ri * SI_PITCH + 2 * bl + 1] = yi;
    }
    __syncthreads();
    // each chunk's 82 terms in a chain of their own, then added: one chain over all 2050 terms rounds an impulse's 1025 equal
    // terms the same way at every step, and the bias grows to 1.5e-5 of the sample (n = 1); blocked, it stays below 1e-6
    f32x16 part[2] = {{}, {}};
    for (int bl = 0; bl < SI_BC; ++bl) {
      const int b = b0 + bl;
#pragma unroll
      for (int q = 0; q < 2; ++q) {                  // A[i][k]: frame 1 + 32 ht + i - q, k = (bin, re/im); B[k][j]: Re -> cos, Im -> -sin
        const float av = sp[(i + 1 - q) * SI_PITCH + 2 * bl + half];
        const int t = HOP * q + u0 + i;
        const float bvv = tab[(b * t + 512 * half) & (NFFT - 1)];
        part[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bvv, part[q], 0, 0, 0);
      }
    }
    acc[0] += part[0];
    acc[1] += part[1];
  }
  const int u = u0 + i;                              // C/D: column = lane & 31 (sample), row = (r & 3) + 8 (r >> 2) + 4 half (hop block)
  const float w0 = c.win[u], w1 = c.win[HOP + u];
  const float norm = w0 * w0 + w1 * w1;              // >= 1/2: never below scipy's 1e-10 threshold
  float* y = out + sig * length;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int h = 1 + 32 * ht + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (h >= T) continue;
    const int64_t s = (int64_t)(h - 1) * HOP + u;
    if (s >= length) continue;
    const float v = w1 * acc[1][r] + w0 * acc[0][r];  // the earlier frame first
    y[s] = v / norm;
  }
}

// ---- mel variants: mixture (fp64) [n], sources [nsrc][n] in TS -> out [nsrc][n] in TS ------------------------------------------------
template <typename TS>
__global__ __launch_bounds__(256) void k_oracle_mel(const double* __restrict__ mix, const TS* __restrict__ src, int nsrc, int64_t n,
                                                    int irm, double theta, TS* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double x = mix[i];
    double den;
    if (irm) {
      TS tot = src[i];                               // np.sum over sources in their dtype, in source order
      for (int j = 1; j < nsrc; ++j) tot = tot + src[(int64_t)j * n + i];
      den = (double)tot + EPS;
    } else {
      den = EPS + x;
    }
    for (int j = 0; j < nsrc; ++j) {
      const double r = (double)src[(int64_t)j * n + i] / den;
      const double m = irm ? r : binary_mask(r, theta);
      out[(int64_t)j * n + i] = (TS)(x * m);
    }
  }
}

}  // namespace glowk_oracle
