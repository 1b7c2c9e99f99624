// glowk device code, part 9: whole-signal separation -- mel frames of a signal of any length, overlapping tiles cut from them for the
// priors, and the separated tiles cross-faded back into frames.  The reference only ever cuts disjoint 2.04 s extracts
// (datasets/data_loader.py:113-164); this path is the project's own.  The front-end constants of glowk_audio.h stay compiled in.
//
//   k_mel_frames    L[m][f] = clip(10 log10(max(1e-10, sum_b W[m][b] |X[b][f]|^2)), -100, 20) for [96][F] with any F: k_mel_db's
//                   arithmetic, cell by cell, without its per-extract floor (and so without its LDS tile and its F <= 128);
//                   |X|^2 comes from k_stft (glowk_audio.h) launched on the long grid
//   k_tile_cut      tile k = frames [k hop, k hop + width), -100 dB beyond the signal's end; the per-tile top_db floor of
//                   k_mel_db over the padded tile, then the clip.  One workgroup per (signal, tile): a max pass, a write pass
//   k_tile_stitch   out[f] = sum_k w[f - k hop] t_k[f - k hop] / sum_k w[f - k hop], w[j] = sin^2(pi (j + 1/2) / width), k ascending
//                   in fp32; a frame that one tile covers is copied.  One thread per output cell: no atomics, a fixed order
#pragma once
#include "glowk_audio.h"

namespace glowk_long {

using glowk_audio::AudioConsts;
using glowk_audio::NBIN;
using glowk_audio::NMEL;

constexpr int MAX_WIDTH = 128;                       // a tile is at most glowk_audio::MAX_FRAMES wide (mel_to_power's tiles)
constexpr int MAX_FRAMES = 1 << 20;                  // frames of one signal, as glowk_audio::GL_MAX_FRAMES
constexpr float DB_MIN = -100.0f, DB_MAX = 20.0f;

// ---- mel dB frames: one thread per (signal, filter, frame), frames along the threads (coalesced rows of the spectrum).
// grid (signals x fblocks, 96).  The band sum runs over ascending bins with fmaf, as k_mel_db's
__global__ __launch_bounds__(256) void k_mel_frames(const float* __restrict__ power, const float2* __restrict__ X, int F, int fblocks,
                                                    AudioConsts c, float* __restrict__ mel_db) {
  const int n = blockIdx.x / fblocks, f = (blockIdx.x % fblocks) * 256 + threadIdx.x, m = blockIdx.y;
  if (f >= F) return;
  const size_t base = (size_t)n * NBIN * F;
  const int lo = c.mel_lo[m], len = c.mel_len[m];
  const float* w = c.mel_w + c.mel_off[m];
  float s = 0.0f;
  for (int j = 0; j < len; ++j) s = fmaf(w[j], glowk_audio::bin_power(power, X, base + (size_t)(lo + j) * F + f), s);
  const float db = 10.0f * log10f(fmaxf(s, 1e-10f));
  mel_db[((size_t)n * NMEL + m) * F + f] = fminf(fmaxf(db, DB_MIN), DB_MAX);
}

// ---- tile cut: grid (signals x N), 256 threads over the tile's 96 x width cells -----------------------------------------------------
__global__ __launch_bounds__(256) void k_tile_cut(const float* __restrict__ frames, int F, int N, int width, int hop, float top_db,
                                                  float* __restrict__ tiles) {
  __shared__ float red[256];
  const int tid = threadIdx.x, n = blockIdx.x / N, k = blockIdx.x % N;
  const int f0 = k * hop, cells = NMEL * width;      // f0 + width <= 2^20 + 128
  const float* in = frames + (size_t)n * NMEL * F;
  float floor_db = -INFINITY;
  if (top_db > 0.0f) {
    float mx = -INFINITY;
    for (int o = tid; o < cells; o += 256) {
      const int m = o / width, f = f0 + o % width;
      mx = fmaxf(mx, f < F ? in[(size_t)m * F + f] : DB_MIN);
    }
    red[tid] = mx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {              // max is exact in any order: the result is deterministic
      if (tid < h) red[tid] = fmaxf(red[tid], red[tid + h]);
      __syncthreads();
    }
    floor_db = red[0] - top_db;
  }
  float* out = tiles + (size_t)blockIdx.x * cells;
  for (int o = tid; o < cells; o += 256) {
    const int m = o / width, f = f0 + o % width;
    const float v = f < F ? in[(size_t)m * F + f] : DB_MIN;
    out[o] = fminf(fmaxf(fmaxf(v, floor_db), DB_MIN), DB_MAX);
  }
}

// ---- tile stitch: the cross-fade window travels as a kernel argument (built on the host in fp64, rounded once) ---------------------
struct StitchWindow {
  float w[MAX_WIDTH];
};

// The cross-fade of frame f of one row: t points at that row in tile 0 and `tile` floats lie between a tile's row and the next
// tile's; tiles k_lo..k_hi cover the frame.  Shared with k_basis_update_frames (glowk_frames.h), which stitches gradient tiles
__device__ __forceinline__ float stitch_frame(const float* __restrict__ t, size_t tile, int k_lo, int k_hi, int f, int hop,
                                              const StitchWindow& win) {
  if (k_lo == k_hi) return t[(size_t)k_lo * tile + (f - k_lo * hop)];    // one tile covers the frame: its value, bit for bit
  float num = 0.0f, den = 0.0f;
  for (int k = k_lo; k <= k_hi; ++k) {
    const int j = f - k * hop;
    const float w = win.w[j];
    num = fmaf(w, t[(size_t)k * tile + j], num);
    den += w;
  }
  return num / den;
}

// grid (signals x fblocks, 96).  Tiles k with 0 <= f - k hop < width: k from ceil((f - width + 1) / hop) to min(N - 1, f / hop);
// F <= (N - 1) hop + width makes that range non-empty for every f < F
__global__ __launch_bounds__(256) void k_tile_stitch(const float* __restrict__ tiles, int N, int width, int hop, int F, int fblocks,
                                                     StitchWindow win, float* __restrict__ frames) {
  const int n = blockIdx.x / fblocks, f = (blockIdx.x % fblocks) * 256 + threadIdx.x, m = blockIdx.y;
  if (f >= F) return;
  const int k_hi = min(N - 1, f / hop);
  const int k_lo = f < width ? 0 : (f - width) / hop + 1;
  const float* t = tiles + ((size_t)n * N * NMEL + m) * width;           // tile k's row m starts at t + k 96 width
  frames[((size_t)n * NMEL + m) * F + f] = stitch_frame(t, (size_t)NMEL * width, k_lo, k_hi, f, hop, win);
}

}  // namespace glowk_long
