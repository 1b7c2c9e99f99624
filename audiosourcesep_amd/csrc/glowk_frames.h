// glowk device code, part 10: BASIS as ONE chain over a whole signal -- the Langevin state is the signal's frames [S][rows][F], the
// priors still see tiles of their width every `hop` frames, and the prior score of a frame is the cross-fade (k_tile_stitch's window
// and arithmetic) of the scores the tiles that cover it give it.  The weights of a frame sum to one, so the prior pulls on a frame
// as hard as it does in a per-tile chain, and at hop = width the method is the per-tile chain.  The project's own: the reference only
// cuts disjoint extracts.
//
//   k_frames_to_tiles        tile t = frames [t hop, t hop + width), `pad` at and beyond F: a raw gather, no floor and no clip (BASIS
//                            states leave [-100, 20]); run once per noise level
//   k_basis_update_frames<S> one Langevin step of all S sources in one launch: gather and stitch the gradient tiles (stitch_frame),
//                            the update of k_basis_update_n (basis_quad_weights / basis_quad_step: the same roundings), the frames
//                            written in place and scattered into the next step's tiles.  A thread owns four consecutive elements
//                            e = b F + f of the frame layout, which is one Philox call per source: element e draws element e of the
//                            stream (glowk_random_source at offset 0).  Nothing is accumulated across threads: no atomics, one order
#pragma once
#include "glowk_basis.h"
#include "glowk_longform.h"
#include <utility>

namespace glowk_long {

constexpr int MAX_ROWS = 1 << 16;

// one thread per tile cell, the width along the threads
__global__ __launch_bounds__(256) void k_frames_to_tiles(const float* __restrict__ x, int rows, int F, int N, int width, int hop, float pad,
                                                         size_t cells, float* __restrict__ tiles) {
  const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= cells) return;
  const int j = (int)(o % (size_t)width);
  const size_t row = o / (size_t)width;             // (signal N + t) rows + b
  const int b = (int)(row % (size_t)rows);
  const size_t st = row / (size_t)rows;
  const int t = (int)(st % (size_t)N);
  const size_t sig = st / (size_t)N;
  const int f = t * hop + j;                        // <= (2^20 - 1) + 127
  tiles[o] = f < F ? x[(sig * rows + b) * F + f] : pad;
}

struct BasisFramesArgs {
  float* x = nullptr;                               // [S][rows][F], in place
  const float* g[GLOWK_BASIS_MAX_SOURCES] = {};     // [N][rows][width] grad log p_k of the tiles of x_k
  const float* eps[GLOWK_BASIS_MAX_SOURCES] = {};   // optional [rows][F] standard-normal draws of source k; null: device RNG
  const float* mixed = nullptr;                     // [rows][F]
  float* tiles_out = nullptr;                       // optional [S][N][rows][width]: the tiles of the updated states
  int* nonfinite = nullptr;
  size_t n = 0;                                     // rows F
  uint64_t seed = 0, step = 0;
  unsigned qblocks = 0;                             // workgroups that hold frames; the ones behind them write the last tile's pad cells
  int rows = 0, F = 0, N = 0, width = 0, hop = 0;
  int pad_cols = 0;                                 // (N - 1) hop + width - F: only the last tile reaches past the signal
  float eta = 0.0f, lambda_recon = 0.0f, noise_scale = 0.0f, ln_s = 0.0f, inv_s = 1.0f, pad = 0.0f;
  int mixing = 0;
  int vec = 0;                                      // n % 4 == 0 and x, mixed, eps 16-byte aligned: their quads move as float4
  StitchWindow win;
};
static_assert(sizeof(BasisFramesArgs) <= 1024 && std::is_trivially_copyable_v<BasisFramesArgs>, "kernel argument size");

template <class Body, int... K>
__device__ __forceinline__ void each_source(std::integer_sequence<int, K...>, Body&& body) {
  (body(std::integral_constant<int, K>()), ...);
}

template <int S>
__global__ __launch_bounds__(256) void k_basis_update_frames(BasisFramesArgs a) {
  const size_t tile = (size_t)a.rows * a.width, per_source = (size_t)a.N * tile;
  if (blockIdx.x >= a.qblocks) {                    // the cells of the last tile past the signal's end, one thread per (row, column)
    const unsigned p = (blockIdx.x - a.qblocks) * 256u + threadIdx.x;
    if (p >= (unsigned)(a.rows * a.pad_cols)) return;
    const int b = (int)(p / (unsigned)a.pad_cols), j = a.width - a.pad_cols + (int)(p % (unsigned)a.pad_cols);
    float* o = a.tiles_out + ((size_t)(a.N - 1) * a.rows + b) * a.width + j;
#pragma unroll
    for (int k = 0; k < S; ++k) o[k * per_source] = a.pad;
    return;
  }
  const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const size_t e0 = (size_t)q * 4;
  if (e0 >= a.n) return;
  const bool quad = a.vec;                          // (then n is a multiple of 4: there is no partial quad)
  // where the four elements lie: a quad may run over the end of a row
  int row[4], col[4], t_lo[4], t_hi[4];
  bool in[4];
  {
    unsigned b = a.n <= 0xFFFFFFFFull ? (unsigned)e0 / (unsigned)a.F : (unsigned)(e0 / (size_t)a.F);
    unsigned f = (unsigned)(e0 - (size_t)b * a.F);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      while (f >= (unsigned)a.F) { f -= (unsigned)a.F; ++b; }
      in[j] = e0 + j < a.n;                         // elements past n compute on zeros, read no tile and are never stored
      row[j] = (int)b; col[j] = (int)f;
      t_hi[j] = min(a.N - 1, (int)f / a.hop);       // the tiles t with 0 <= f - t hop < width, as k_tile_stitch's
      t_lo[j] = (int)f < a.width ? 0 : ((int)f - a.width) / a.hop + 1;
      ++f;
    }
  }
  float x[S][4], mixed[4];
  if (quad) {
    const float4 t = *reinterpret_cast<const float4*>(a.mixed + e0);
    mixed[0] = t.x; mixed[1] = t.y; mixed[2] = t.z; mixed[3] = t.w;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const float4 u = *reinterpret_cast<const float4*>(a.x + k * a.n + e0);
      x[k][0] = u.x; x[k][1] = u.y; x[k][2] = u.z; x[k][3] = u.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mixed[j] = in[j] ? a.mixed[e0 + j] : 0.0f;
#pragma unroll
      for (int k = 0; k < S; ++k) x[k][j] = in[j] ? a.x[k * a.n + e0 + j] : 0.0f;
    }
  }
  float m[S][4], r[4];
  bool bad = basis_quad_weights<S>(x, mixed, a.mixing, a.ln_s, a.inv_s, a.lambda_recon, m, r);
  // (a fold over k = 0 .. S-1 in place of `#pragma unroll`: from S = 10 on the body is past the size up to which the compiler
  // follows the pragma, and a loop left rolled would index x[k] and m[k] at run time, which puts them into scratch memory)
  each_source(std::make_integer_sequence<int, S>(), [&](auto source) __attribute__((always_inline)) {
    constexpr int k = decltype(source)::value;
    float g[4], z[4], y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      g[j] = in[j] ? stitch_frame(a.g[k] + (size_t)row[j] * a.width, tile, t_lo[j], t_hi[j], col[j], a.hop, a.win) : 0.0f;
    const float* eps = a.eps[k];
    if (!eps) {
      normal4(a.seed, a.step, (uint32_t)(k & 1), q, z, (uint32_t)(k >> 1));
    } else if (quad) {
      const float4 t = *reinterpret_cast<const float4*>(eps + e0);
      z[0] = t.x; z[1] = t.y; z[2] = t.z; z[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) z[j] = in[j] ? eps[e0 + j] : 0.0f;
    }
    bad |= basis_quad_step(x[k], m[k], r, g, z, a.eta, a.noise_scale, y);
    float* xk = a.x + k * a.n + e0;
    if (quad) {
      *reinterpret_cast<float4*>(xk) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (in[j]) xk[j] = y[j];
    }
    if (a.tiles_out) {                              // cell (t, b, f - t hop) of every tile t that covers the frame
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!in[j]) continue;                       // (of the loop over j)
        float* o = a.tiles_out + k * per_source + (size_t)row[j] * a.width + col[j];
        for (int t = t_lo[j]; t <= t_hi[j]; ++t) o[(size_t)t * tile - (size_t)(t * a.hop)] = y[j];
      }
    }
  });
  if (bad && a.nonfinite) *a.nonfinite = 1;
}

}  // namespace glowk_long
