// glowk device code: kernel additive modelling (Liutkus, FitzGerald, Rafii, Pardo & Daudet 2014; KAML 2015) -- every source has a
// proximity kernel, the set of time-frequency neighbours it is locally constant over, and the sources are estimated together by
// back-fitting: median-filter each source's estimate over its own kernel, share the mixture out by the ratio of the results, repeat.
// s [nsig][rows][frames] float32, frames contiguous.
//
//   k_kam_median   out[r][t] = the median over the table's entries e of s[r + d_row_e][t + d_frame_e], those inside the plane
//   k_kam_backfit  the J soft masks of the J filtered estimates and the mixture shared out by them, elementwise in fp32
//
// k_kam_median: gather, then select.  A wave owns 64 consecutive frames of one row (glowk_kam_index.h: the unit).  The table, n int16
// pairs, is a launch argument, so its entries are scalars: per entry the wave does one coalesced 256-byte load, or none where the row
// is outside the plane; a lane whose frame is outside takes no value.  Eight entries' loads are issued before their values are
// stored, so they overlap.  A lane appends its values, in table order, to its own column of the wave's LDS slab [n][64] (lane stride
// 1: no bank conflict) and keeps its own count m; no lane reads another lane's column, so the kernel has no barrier.  A lane with no
// neighbour takes the cell itself (m = 1).  Columns are filled with +inf up to the wave's largest m, so that the counting loop below
// has one bound for the wave and no per-lane test.
// Selection (glowk_hpss.h's rank counting, extended to per-lane m and the two middle elements): the element of sorted position p is
// the v with the largest #(w < v) that does not exceed p, the first such in table order (elements that compare equal differ in bits
// only as -0 and +0 do).  Positions (m - 1) / 2 and m / 2 are tracked together; four candidates share each read of the column (eight
// for n > 28: fewer LDS reads per compare, coarser steps to the early exit); the wave leaves when every lane has both counts at their
// targets.  m odd: the element; m even: (a + b) * 0.5f, the only arithmetic.
// One launch, no atomics, no allocation; a unit depends on nothing outside its signal: bitwise reproducible, and a batch gives what
// its signals give alone.  Signals may be strided (glowk_kam_fit filters source j of [nsig][J][rows][frames] in place).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glowk_kam_index.h"

namespace glowk_kam {

// CAND: the candidates that share each read of a lane's column (glowk_kam_index.h: candidates(n))
template <int CAND>
__global__ __launch_bounds__(MAX_WAVES * 64) void k_kam_median(const float* __restrict__ s, int64_t s_stride, int rows, int F, int64_t nunits,
                                                               const Table tab, int n, float* __restrict__ out, int64_t out_stride) {
  extern __shared__ float slab[];             // [waves][n][TILE_F]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t unit = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (unit >= nunits) return;                 // wave-uniform; the kernel has no barrier
  int64_t sig;
  int r, f0;
  unit_of(unit, rows, F, sig, r, f0);
  const int f = f0 + lane;
  const bool live = f < F;
  const float* a = s + sig * s_stride;
  float* w = slab + (size_t)wave * n * TILE_F + lane;           // this lane's column, stride TILE_F
  int m = 0;
  for (int e0 = 0; e0 < n; e0 += TABLE_STEP) {
    float x[TABLE_STEP];
    bool ok[TABLE_STEP];
#pragma unroll
    for (int u = 0; u < TABLE_STEP; ++u) {
      const int e = e0 + u;                   // < table_reads(n) <= TABLE_ENTRIES
      const int dr = tab.d[e][0], df = tab.d[e][1];
      ok[u] = e < n && live && neighbour(r, f, dr, df, rows, F);
      x[u] = ok[u] ? a[(int64_t)(r + dr) * F + (f + df)] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < TABLE_STEP; ++u)
      if (ok[u]) {
        w[m * TILE_F] = x[u];
        ++m;
      }
  }
  if (m == 0) {                               // no neighbour: the cell itself (a lane past the last frame: a zero, never written out)
    w[0] = live ? a[(int64_t)r * F + f] : 0.0f;
    m = 1;
  }
  int mmax = m;
  for (int o = 32; o; o >>= 1) mmax = max(mmax, __shfl_xor(mmax, o, 64));
  for (int k = m; k < mmax; ++k) w[k * TILE_F] = INFINITY;      // never below a candidate, never a candidate (those end at m - 1)
  const int pa = pos_low(m), pb = pos_high(m);
  float va = w[0], vb = va;
  int la = -1, lb = -1;
  for (int c = 0; c < mmax; c += CAND) {
    float v[CAND];
    int lt[CAND];
#pragma unroll
    for (int j = 0; j < CAND; ++j) {
      v[j] = w[min(c + j, m - 1) * TILE_F];   // past the end the last element again: the same count, never taken over the first
      lt[j] = 0;
    }
    for (int k = 0; k < mmax; ++k) {
      const float y = w[k * TILE_F];
#pragma unroll
      for (int j = 0; j < CAND; ++j) lt[j] += y < v[j] ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < CAND; ++j) {
      if (lt[j] <= pa && lt[j] > la) { va = v[j]; la = lt[j]; }
      if (lt[j] <= pb && lt[j] > lb) { vb = v[j]; lb = lt[j]; }
    }
    if (__all(la == pa && lb == pb)) break;   // wave-uniform exit: no count can exceed its position and be taken
  }
  if (live) out[sig * out_stride + (int64_t)r * F + f] = (m & 1) ? va : (va + vb) * 0.5f;
}

// glowk_hpss.h's softmask arithmetic from 2 to J sources: Z = max_j a_j, bad = Z < FLT_MIN (then Z = 1), r_j = (a_j / Z)^power,
// mask_j = r_j / (r_0 + r_1 + .. ) added in ascending j, 1 / J where bad; p_j = v mask_j.  No contraction: every operation rounds once.
__device__ __forceinline__ float kam_pow(float x, float power) {          // the exponents 1 and 2 (the default) without powf
  return power == 1.0f ? x : power == 2.0f ? __fmul_rn(x, x) : powf(x, power);
}

template <int J>
__global__ __launch_bounds__(256) void k_kam_backfit(const float* __restrict__ v, const float* __restrict__ a, int64_t total, int64_t n, float power,
                                                     float* __restrict__ p, float* __restrict__ mask) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t base = (i / n) * J * n + i % n;
    float x[J];
#pragma unroll
    for (int j = 0; j < J; ++j) x[j] = a[base + j * n];
    float Z = x[0];
#pragma unroll
    for (int j = 1; j < J; ++j) Z = fmaxf(Z, x[j]);
    const bool bad = Z < 1.17549435e-38f;     // FLT_MIN
    if (bad) Z = 1.0f;
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      x[j] = kam_pow(__fdiv_rn(x[j], Z), power);
      sum = j == 0 ? x[0] : __fadd_rn(sum, x[j]);
    }
    const float mix = v[i];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const float mk = bad ? __fdiv_rn(1.0f, (float)J) : __fdiv_rn(x[j], sum);
      p[base + j * n] = __fmul_rn(mix, mk);
      if (mask) mask[base + j * n] = mk;
    }
  }
}

#define GLOWK_KAM_EACH_J(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

}  // namespace glowk_kam
