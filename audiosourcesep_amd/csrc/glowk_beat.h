// glowk device code: the front end of REPET and adaptive REPET (Rafii & Pardo 2013; Liutkus et al. 2012) -- the beat spectrum, its
// windowed form the beat spectrogram, the period, and the periodic neighbour lists that glowk_nn_median (glowk_repet.h) filters
// over.  s [nsig][rows][frames] float32, frames contiguous, real and non-negative; P = s * s in fp32.
//
//   k_beat_gram         the diagonal sums of the banded frame Gram matrix of P, per window: acf[l] = sum_r sum_j P[r][j] P[r][j + l]
//                       over the pairs inside the window, for the lags 0 <= l < nlags alone (the upper triangle, lag 0 once).  Each
//                       Gram element is an fp32 fma chain over the rows in row order on v_mfma_f32_32x32x2_f32; everything after
//                       it is fp64.  Partial sums go to the workspace in a fixed order; no frames x frames array exists anywhere
//   k_beat_reduce       beat[t][l] = (acf[l] / (rows (n_t - l))) / (acf[0] / (rows n_t)) from the partial sums, in fp64, rounded to
//                       float32 once; 0 for l >= n_t and for a silent window
//   k_beat_period       per segment the lag in [pmin, pmax] of largest beat value, equal values to the lower lag
//   k_period_neighbors  per frame j the frames j + i p, i = 0, -1, +1, -2, +2, .., inside the signal, the first k of them
//
// k_beat_gram.  The band of a window is cut into units of QT = 32 query frames by UW = 64 candidate frames: unit (t, u) holds the
// products of the window's frames [32 t, 32 t + 32) with the frames D = 64 u further on, [32 t + D, 32 t + D + 64), so every unit of
// column u holds the same NL = 95 lags [D - 31, D + 63], whatever t.  One wave computes one unit at a time: two 32 x 32
// accumulators over all rows, the operands read straight from s as k_nn_topk reads them (lane l reads row 2 p + (l >> 5), frame
// base + (l & 31); KU = 16 row pairs per step, the next step's loads in flight under this step's MFMAs), squared on the way and
// zeroed where the frame lies outside the window (the address is clamped into it), so a unit that sticks out of the window adds
// exact zeros.  The unit goes to the wave's own LDS tile [32][64 + 8]; lane d then adds diagonal d (and d + 64 for d < 31) down the
// 32 queries in fp64 into a register that it keeps across units: 64 LDS reads and fp64 adds per lane against rows MFMAs.  The waves
// of a workgroup never wait for each other inside the loop.  A workgroup of 4 waves owns column u and the query tiles
// [4 tpw ch, 4 tpw (ch + 1)), wave w every fourth of them; at the end the four waves' sums are added in wave order and written to
// part[signal, window][u][ch][96].  tpw (query tiles per wave, 1 .. 16) and the grid follow from (frames or win, nlags) alone --
// not from nsig -- so a batch adds in the order its signals do alone.  k_beat_reduce adds, per lag, the chunks ch in order of the
// one or two columns that hold it (u - 1 first).
// Registers: 32 accumulators, 6 KU = 96 operands.  LDS: 4 tiles of 32 x 72 floats and 4 x 96 doubles, 39 936 bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glowk_beat_index.h"
#include "glowk_repet.h"

namespace glowk_beat {

using glowk_repet::f32x16;
using glowk_repet::KU;
constexpr int MAX_SIG = 65535, MAX_ROWS = 4096, MAX_FRAMES = 32768, MAX_K = 512;
constexpr int QT = 32;                      // query frames per unit: one MFMA tile high
constexpr int UW = 64;                      // candidate frames per unit: two MFMA tiles wide
constexpr int NL = UW + QT - 1;             // lags a unit touches
constexpr int NLP = 96;                     // doubles per partial-sum record
constexpr int PITCH = UW + 8;
constexpr int MAX_TPW = 16;

// How one (signal, window) is cut up; a function of the shapes alone.  nmax: the longest window.
struct BeatPlan {
  int nwin, nmax, nu, tpw, nch;
};
inline BeatPlan beat_plan(int frames, int nlags, int win, int step) {
  BeatPlan p;
  p.nwin = win == 0 ? 1 : (frames + step - 1) / step;
  p.nmax = win == 0 ? frames : win;
  const int leff = nlags < p.nmax ? nlags : p.nmax;             // lags from nmax on are zero by definition
  p.nu = (leff + 30) / UW + 1;                                  // columns u with 64 u - 31 <= leff - 1
  int64_t units = 0;                                            // units of one full window
  for (int u = 0; u < p.nu; ++u)
    if (p.nmax > u * UW) units += (p.nmax - u * UW + QT - 1) / QT;
  int64_t tpw = (units + 4095) / 4096;
  p.tpw = (int)(tpw < 1 ? 1 : tpw > MAX_TPW ? MAX_TPW : tpw);
  const int qtiles = (p.nmax + QT - 1) / QT;
  p.nch = (qtiles + 4 * p.tpw - 1) / (4 * p.tpw);
  return p;
}

__device__ __forceinline__ float beat_sq(float x, bool live) { return live ? x * x : 0.0f; }

__global__ __launch_bounds__(256) void k_beat_gram(const float* __restrict__ s, int rows, int F, int win, int step, int nwin, int nu, int nch, int tpw,
                                                   int nlags, double* __restrict__ part) {
  __shared__ float tile[4][QT][PITCH];
  __shared__ double wsum[4][NLP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  unsigned b = blockIdx.x;
  const int ch = (int)(b % (unsigned)nch);
  b /= (unsigned)nch;
  const int u = (int)(b % (unsigned)nu);
  b /= (unsigned)nu;
  const int w = (int)(b % (unsigned)nwin);
  const int64_t sig = b / (unsigned)nwin;
  int first, n;
  beat_window(w, win, step, F, first, n);
  const int D = u * UW;
  const float* a = s + sig * rows * F;
  const int64_t rstep = 2 * (int64_t)F;
  const int ntiles = n > D ? (n - D + QT - 1) / QT : 0;          // query tiles whose candidates reach into the window
  const int tend = min(ntiles, (ch + 1) * 4 * tpw);
  const int l0 = D - (QT - 1) + lane, l1 = l0 + 64;              // this lane's lags
  const bool use0 = l0 >= 0 && l0 < nlags, use1 = lane < QT - 1 && l1 < nlags;
  double sum0 = 0.0, sum1 = 0.0;
  const int pairs = rows >> 1, chunks = pairs / KU;
  for (int t = ch * 4 * tpw + wave; t < tend; t += 4) {           // wave-uniform
    const int i0 = t * QT;
    const int qr = i0 + c;
    const bool qv = qr < n;
    const int qf = first + min(qr, n - 1);                        // a frame outside the window: the address clamped, the operand zero
    bool jv[2];
    int jf[2];
    unsigned jo[2];
    f32x16 acc[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int jr = i0 + D + m * 32 + c;
      jv[m] = jr < n;
      jf[m] = first + min(jr, n - 1);
      jo[m] = (unsigned)(half * F + jf[m]);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][r] = 0.0f;
    }
    const unsigned qo = (unsigned)(half * F + qf);
    // KU row pairs per chunk, the next chunk's loads issued before this chunk's MFMAs (k_nn_topk's loop); the loaded values are
    // squared, or zeroed, when they move into the operand registers
    float xa[KU], xb[2][KU], ya[KU], yb[2][KU];
    if (chunks > 0) {
      glowk_repet::nn_load<2>(a, rstep, qo, jo, ya, yb);
#pragma unroll
      for (int x = 0; x < KU; ++x) {
        xa[x] = beat_sq(ya[x], qv);
        xb[0][x] = beat_sq(yb[0][x], jv[0]);
        xb[1][x] = beat_sq(yb[1][x], jv[1]);
      }
    }
    for (int k = 0; k < chunks; ++k) {
      glowk_repet::nn_load<2>(a + (int64_t)min(k + 1, chunks - 1) * KU * rstep, rstep, qo, jo, ya, yb);
      __builtin_amdgcn_sched_barrier(0);
      glowk_repet::nn_mma<2>(xa, xb, acc);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int x = 0; x < KU; ++x) {
        xa[x] = beat_sq(ya[x], qv);
        xb[0][x] = beat_sq(yb[0][x], jv[0]);
        xb[1][x] = beat_sq(yb[1][x], jv[1]);
      }
    }
    const float* pa = a + (int64_t)chunks * KU * rstep;
    for (int p = chunks * KU; p < pairs; ++p) {                   // the pairs left over, in row order
      const float av = beat_sq(pa[qo], qv);
#pragma unroll
      for (int m = 0; m < 2; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, beat_sq(pa[jo[m]], jv[m]), acc[m], 0, 0, 0);
      pa += rstep;
    }
    if (rows & 1) {                                               // an odd row count: the last row against a zero row
      const float* pl = a + (int64_t)(rows - 1) * F;
      const float av = beat_sq(pl[qf], qv && !half);
#pragma unroll
      for (int m = 0; m < 2; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, beat_sq(pl[jf[m]], jv[m] && !half), acc[m], 0, 0, 0);
    }
    // C/D: column = lane & 31 (candidate), row = (r & 3) + 8 (r >> 2) + 4 half (query)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
      for (int r = 0; r < 16; ++r) tile[wave][(r & 3) + 8 * (r >> 2) + 4 * half][m * 32 + c] = acc[m][r];
    }
    __builtin_amdgcn_wave_barrier();
    // diagonal d holds tile[q][d - 31 + q], the pairs (query q, candidate q + lag - D)
    if (use0) {
#pragma unroll
      for (int q = 0; q < QT; ++q) {
        const int x = lane - (QT - 1) + q;
        if (x >= 0) sum0 += (double)tile[wave][q][x];             // x <= 63 always
      }
    }
    if (use1) {
#pragma unroll
      for (int q = 0; q < QT - 1; ++q) {
        const int x = lane + 64 - (QT - 1) + q;
        if (x < UW) sum1 += (double)tile[wave][q][x];
      }
    }
    __builtin_amdgcn_wave_barrier();                              // the tile is free again
  }
  wsum[wave][lane] = sum0;
  if (lane < NLP - 64) wsum[wave][64 + lane] = sum1;              // (slot 95 is a zero)
  __syncthreads();
  if (threadIdx.x < NLP) {
    const int d = threadIdx.x;
    part[(int64_t)blockIdx.x * NLP + d] = ((wsum[0][d] + wsum[1][d]) + wsum[2][d]) + wsum[3][d];
  }
}

// the sum of lag l of one (signal, window): the chunks in order, of column u - 1 (where the lag is among its last 31) and then u
__device__ __forceinline__ double beat_lag_sum(const double* p, int nu, int nch, int l) {
  const int u = (l + QT - 1) / UW, d = l + QT - 1 - UW * u;
  double acc = 0.0;
  if (u >= 1 && d < QT - 1)
    for (int ch = 0; ch < nch; ++ch) acc += p[((int64_t)(u - 1) * nch + ch) * NLP + d + UW];
  if (u < nu)
    for (int ch = 0; ch < nch; ++ch) acc += p[((int64_t)u * nch + ch) * NLP + d];
  return acc;
}

__global__ __launch_bounds__(256) void k_beat_reduce(const double* __restrict__ part, int64_t total, int rows, int F, int win, int step, int nwin,
                                                     int nu, int nch, int nlags, float* __restrict__ beat) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;     // (signal, window, lag)
  if (e >= total) return;
  const int l = (int)(e % nlags);
  const int64_t sw = e / nlags;
  int first, n;
  beat_window((int)(sw % nwin), win, step, F, first, n);
  float out = 0.0f;
  if (l < n) {
    const double* p = part + sw * nu * nch * NLP;
    const double raw0 = beat_lag_sum(p, nu, nch, 0) / ((double)rows * (double)n);
    const double raw = beat_lag_sum(p, nu, nch, l) / ((double)rows * (double)(n - l));
    if (raw0 > 0.0) out = (float)(raw / raw0);
  }
  beat[e] = out;
}

// One wave per segment.  The rule is the order of one key: the value's bits as an ordered integer above, ~lag below.
__global__ __launch_bounds__(64) void k_beat_period(const float* __restrict__ beat, int nlags, int pmin, int pmax, int32_t* __restrict__ period) {
  const float* b = beat + (int64_t)blockIdx.x * nlags;
  unsigned long long best = 0;
  for (int l = pmin + (int)threadIdx.x; l <= pmax; l += 64) {
    const unsigned long long key = glowk_repet::nn_key(b[l], l);
    best = key > best ? key : best;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(best, m, 64);
    best = o > best ? o : best;
  }
  if (threadIdx.x == 0) period[blockIdx.x] = glowk_repet::nn_key_frame(best);   // lane 0 always has lag pmin: best is a real key
}

__global__ __launch_bounds__(256) void k_period_neighbors(const int32_t* __restrict__ period, int64_t total, int F, int nper, int step, int k,
                                                          int32_t* __restrict__ idx) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;     // (signal, frame)
  if (e >= total) return;
  const int j = (int)(e % F);
  period_list(j, period_of(period + (e / F) * nper, nper, step, j), F, k, idx + e * k);
}

}  // namespace glowk_beat
