// glowk device code: harmonic / percussive source separation by median filtering (Fitzgerald 2010; librosa.decompose.hpss) --
// the prior-free baseline: no trained flows, no ground-truth stems.  s [nsig][rows][frames] float32, frames contiguous (|STFT| with
// rows = 1025, or the 96 mel rows; nothing here assumes either).
//
//   k_median_frames  harmonic:   the running median of odd length `size` along the frame axis, one (signal, row) line at a time
//   k_median_rows    percussive: the same along the row axis, one (signal, frame) line at a time
//   k_hpss_mask      the two soft masks of librosa.util.softmask from the two filtered spectra, fp32, optionally times s
//
// Edges: scipy.ndimage.median_filter(mode='reflect'), the half-sample symmetric extension d c b a | a b c d | d c b a: sample j of
// an axis of length n reads r = j mod 2 n (mathematical mod), then r if r < n, else 2 n - 1 - r; right for windows many times longer
// than the axis.  Selection: the output is the window element v with #(w < v) <= size / 2 < #(w <= v), found by counting ranks --
// compares only, no arithmetic on the values -- so ties, runs of equal values and zeros give the bits a sort gives.  Of elements
// that compare equal (they differ in bits only as -0 and +0 do) the first in window order is taken.
//
// Both filters stage a tile and a halo of size / 2 on each side in LDS through the reflect map and select from LDS; neighbouring
// lanes sit at neighbouring frames in both, so global loads are coalesced along frames and a wave's LDS reads are 64 consecutive
// floats (conflict-free):
//   frames filter  a wave owns 64 frames of one line (+ halo: 64 + size - 1 floats), a workgroup 4 consecutive lines
//   rows filter    a workgroup owns 64 frames x 64 rows (+ halo: 64 + size - 1 rows of 64 floats, 48 640 bytes at size 127); a wave
//                  takes 4 of the rows, each lane walking down its own column at a stride of 64 floats
// One launch each, no atomics, no allocation; a line depends on nothing outside its signal: bitwise reproducible, and a batch
// gives what its signals give alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace glowk_hpss {

constexpr int MAX_SIZE = 127, MAX_ROWS = 4096, MAX_FRAMES = 1 << 20, MAX_SIG = 65535;
constexpr int TILE_F = 64;                  // frames per tile: one wave wide
constexpr int LINES = 4;                    // frames filter: lines per workgroup, one per wave
constexpr int ROW_CHUNK = 64, ROW_WAVES = 16;   // rows filter: output rows per workgroup, 4 per wave

__host__ __device__ inline int reflect_index(int j, int n) {
  const int m = 2 * n;
  int r = j % m;
  if (r < 0) r += m;
  return r < n ? r : m - 1 - r;
}

// The median of w[0], w[STRIDE], .. w[(size - 1) STRIDE] by rank: the element v with #(w < v) <= size / 2 < #(w <= v).  Only
// #(w < v) is counted: an element below the median m has #(w < v) < #(w < m) (v itself lies below m), one above it has
// #(w < v) >= #(w <= m) > size / 2, so m is the element with the largest count that does not exceed size / 2, and the first such in
// window order is kept.  Four candidates share each read of the window (past the end the last element stands in again: the same
// count, never taken over the first), so a pair costs a quarter of an LDS read, one compare and one add.
template <int STRIDE>
__device__ __forceinline__ float rank_select(const float* w, int size) {
  const int h = size >> 1;
  float best = w[0];
  int best_lt = -1;
  for (int c = 0; c < size; c += 4) {
    float v[4];
    int lt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = w[min(c + j, size - 1) * STRIDE];
    for (int k = 0; k < size; ++k) {
      const float x = w[k * STRIDE];
#pragma unroll
      for (int j = 0; j < 4; ++j) lt[j] += x < v[j] ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lt[j] <= h && lt[j] > best_lt) { best = v[j]; best_lt = lt[j]; }
    if (__all(best_lt == h)) break;         // wave-uniform exit: no count can exceed size / 2 and be taken
  }
  return best;
}

__global__ __launch_bounds__(LINES * 64) void k_median_frames(const float* __restrict__ s, int64_t lines, int F, int ftiles, int size,
                                                              float* __restrict__ out) {
  __shared__ float tile[LINES][TILE_F + MAX_SIZE - 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = size >> 1;
  const int64_t line = ((int64_t)blockIdx.x / ftiles) * LINES + wave;
  const int f0 = (int)(blockIdx.x % ftiles) * TILE_F;
  const bool live = line < lines;           // wave-uniform
  if (live) {
    const float* a = s + line * F;
    for (int i = lane; i < TILE_F + size - 1; i += 64) tile[wave][i] = a[reflect_index(f0 - h + i, F)];
  }
  __syncthreads();
  if (!live || f0 + lane >= F) return;
  out[line * F + f0 + lane] = rank_select<1>(&tile[wave][lane], size);
}

__global__ __launch_bounds__(ROW_WAVES * 64) void k_median_rows(const float* __restrict__ s, int rows, int F, int ftiles, int rchunks, int size,
                                                               float* __restrict__ out) {
  extern __shared__ float col[];            // [ROW_CHUNK + size - 1][TILE_F]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = size >> 1;
  const unsigned per_sig = (unsigned)ftiles * rchunks;          // <= rows * frames
  const int ft = (blockIdx.x % per_sig) % ftiles, rc = (blockIdx.x % per_sig) / ftiles;
  const int64_t sig = blockIdx.x / per_sig;
  const int f = ft * TILE_F + lane, r0 = rc * ROW_CHUNK;
  const float* a = s + sig * rows * F;
  for (int i = wave; i < ROW_CHUNK + size - 1; i += ROW_WAVES)
    col[i * TILE_F + lane] = f < F ? a[(int64_t)reflect_index(r0 - h + i, rows) * F + f] : 0.0f;
  __syncthreads();
  if (f >= F) return;
  float* o = out + sig * rows * F;
  for (int j = 0; j < ROW_CHUNK / ROW_WAVES; ++j) {
    const int i = wave * (ROW_CHUNK / ROW_WAVES) + j;
    if (r0 + i >= rows) break;              // wave-uniform
    o[(int64_t)(r0 + i) * F + f] = rank_select<TILE_F>(col + i * TILE_F + lane, size);
  }
}

// librosa.util.softmask(X, R, power, split_zeros) in fp32; power = +inf: the hard mask X > R
__device__ __forceinline__ float mask_pow(float x, float power) {       // the exponents 1 and 2 (the default) without powf
  return power == 1.0f ? x : power == 2.0f ? x * x : powf(x, power);
}

__device__ __forceinline__ float softmask(float X, float R, float power, bool split_zeros) {
  float Z = fmaxf(X, R);
  const bool bad = Z < 1.17549435e-38f;     // np.finfo(np.float32).tiny
  if (bad) Z = 1.0f;
  const float m = mask_pow(X / Z, power), r = mask_pow(R / Z, power);
  return bad ? (split_zeros ? 0.5f : 0.0f) : m / (m + r);
}

__global__ __launch_bounds__(256) void k_hpss_mask(const float* __restrict__ harm, const float* __restrict__ perc, const float* __restrict__ s,
                                                   size_t n, float power, float margin_h, float margin_p, float* __restrict__ out_h,
                                                   float* __restrict__ out_p) {
  const bool hard = power == INFINITY, split_zeros = margin_h == 1.0f && margin_p == 1.0f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float H = harm[i], P = perc[i];
    float mh, mp;
    if (hard) {                             // the products of two floats are exact in double: H > P margin as written
      mh = (double)H > (double)P * (double)margin_h ? 1.0f : 0.0f;
      mp = (double)P > (double)H * (double)margin_p ? 1.0f : 0.0f;
    } else {
      mh = softmask(H, P * margin_h, power, split_zeros);
      mp = softmask(P, H * margin_p, power, split_zeros);
    }
    const float x = s ? s[i] : 1.0f;
    out_h[i] = s ? x * mh : mh;
    out_p[i] = s ? x * mp : mp;
  }
}

}  // namespace glowk_hpss
