// glowk: melody separation -- harmonic salience (Salamon & Gomez 2012), a Viterbi f0 track, a harmonic comb mask (Hsu & Jang 2010).
// Formulas in include/glowk.h, design and measurements in DESIGN section 24, the host-side rules in glowk_melody_index.h.
//
//   k_melody_salience  a thread per (bin, frame), the frame fastest: sal[b][t] = sum_h w_h ((1 - a) S[i][t] + a S[i + 1][t]), h
//                      ascending, fp64, rounded once; every gathered read is a wave's contiguous segment of a row, served by the
//                      caches (a slab of frames staged in LDS was 2.7 times slower: DESIGN section 24)
//   k_melody_max       partial maxima of a signal's salience plane; k_melody_emission reduces them again per workgroup (a maximum is
//                      exact in any order) and divides
//   k_melody_track     one workgroup per signal, thread b <-> state b: D double-buffered in LDS, one barrier per frame, the unvoiced
//                      state's maximum over all bins as one (value, earliest index) reduction per wave whose results cross the same
//                      barrier; back pointers uint16 [T][B + 1] to the workspace, traced back out of LDS chunk by chunk
//   k_melody_mask      the comb around the tracked f0: the nearest harmonic alone decides
//
// fp64 with contraction off; no atomics; every order is fixed by the shapes: the bits do not depend on the run or the batch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glowk_melody_index.h"

namespace glowk_melody {

__global__ __launch_bounds__(SAL_THREADS) void k_melody_salience(const float* __restrict__ s, int rows, int frames, const int32_t* __restrict__ idx,
                                                                  const double* __restrict__ frac, const double* __restrict__ w, int B, int H, int blocks,
                                                                  float* __restrict__ sal) {
#pragma clang fp contract(off)
  const int sig = blockIdx.x / blocks;
  const int64_t q = (int64_t)(blockIdx.x - sig * blocks) * SAL_THREADS + threadIdx.x;   // (bin, frame), the frame fastest
  if (q >= (int64_t)B * frames) return;
  const int b = (int)(q / frames), t = (int)(q - (int64_t)b * frames);
  const float* sp = s + (size_t)sig * rows * frames + t;
  double acc = 0.0;
  for (int h = 0; h < H; ++h) {
    const int i = idx[b * H + h];
    if (i < 0 || i > rows - 2) continue;                 // a dead term (a table out of range reads nothing either)
    const double a = frac[b * H + h];
    const double s0 = (double)sp[(size_t)i * frames], s1 = (double)sp[(size_t)(i + 1) * frames];
    const double term = w[h] * ((1.0 - a) * s0 + a * s1);
    acc = acc + term;
  }
  sal[(size_t)sig * B * frames + q] = (float)acc;
}

// the maximum of 256 threads' values; every thread gets it
__device__ inline float block_max_256(float v, float* sh /* [4] */) {
  for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  __syncthreads();                                       // sh may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

__global__ __launch_bounds__(EMI_THREADS) void k_melody_max(const float* __restrict__ sal, int64_t cells, int groups, float* __restrict__ partial) {
  __shared__ float sh[4];
  const int sig = blockIdx.x / groups, g = blockIdx.x - sig * groups;
  int64_t c0, c1;
  emi_chunk(cells, g, c0, c1);
  const float* p = sal + (size_t)sig * cells;
  float v = 0.0f;                                        // the plane is non-negative
  for (int64_t c = c0 + threadIdx.x; c < c1; c += EMI_THREADS) v = fmaxf(v, p[c]);
  v = block_max_256(v, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

__global__ __launch_bounds__(EMI_THREADS) void k_melody_emission(const float* __restrict__ sal, int64_t cells, int groups, int blocks,
                                                                  const float* __restrict__ partial, double* __restrict__ e, float* __restrict__ m_out) {
#pragma clang fp contract(off)
  __shared__ float sh[4];
  const int sig = blockIdx.x / blocks, blk = blockIdx.x - sig * blocks;
  const float m = block_max_256((int)threadIdx.x < groups ? partial[(size_t)sig * groups + threadIdx.x] : 0.0f, sh);
  if (blk == 0 && threadIdx.x == 0) m_out[sig] = m;
  const double den = (double)m > FLOOR ? (double)m : FLOOR;
  const float* p = sal + (size_t)sig * cells;
  double* q = e + (size_t)sig * cells;
  const int64_t c0 = (int64_t)blk * EMI_THREADS * EMI_PER_THREAD;
#pragma unroll
  for (int k = 0; k < EMI_PER_THREAD; ++k) {
    const int64_t c = c0 + k * EMI_THREADS + threadIdx.x;
    if (c < cells) q[c] = (double)p[c] / den;
  }
}

// a candidate of an ordered maximum: the greater value wins, of equal values the earlier index
struct Cand {
  double v;
  int i;
};
__device__ inline Cand cand_best(Cand a, Cand b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ inline Cand wave_best(Cand a) {
  for (int o = 32; o; o >>= 1) {
    Cand b;
    b.v = __shfl_xor(a.v, o);
    b.i = __shfl_xor(a.i, o);
    a = cand_best(a, b);
  }
  return a;
}

// The maximum of a wave's values and the first lane that holds it: the lanes are in index order, so that lane is the earliest
// candidate among equals.
__device__ inline double wave_first_max(double v, int& lane) {
  double m = v;
  for (int o = 32; o; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  lane = __ffsll((long long)__ballot(v == m)) - 1;
  return m;
}

// The barrier of a frame: the LDS writes of the workgroup are visible after it; the global store of the back pointers and the load of
// the next frame's emission stay in flight (__syncthreads would wait for both, a round trip to memory per frame).
__device__ inline void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

__global__ __launch_bounds__(TRK_MAX_THREADS) void k_melody_track(const double* __restrict__ e, int B, int frames, const double* __restrict__ pen, int J,
                                                                   double theta, double nu, uint16_t* __restrict__ bp, int32_t* __restrict__ path,
                                                                   int64_t* __restrict__ ticks) {
#pragma clang fp contract(off)
  __shared__ double D[2][MAX_BINS + 1];
  __shared__ double pens[MAX_JUMP + 1];
  __shared__ double wv[2][TRK_MAX_THREADS / 64];
  __shared__ int wi[2][TRK_MAX_THREADS / 64];
  __shared__ uint16_t chunk[TRK_CHUNK];
  const int sig = blockIdx.x, b = threadIdx.x, nw = blockDim.x >> 6, wave = b >> 6;
  const int ub = trk_unvoiced_thread(B);
  const bool voiced = b < B;
  const double* ep = e + (size_t)sig * B * frames + (size_t)(voiced ? b : 0) * frames;
  uint16_t* bpp = bp + (size_t)sig * (trk_bp_bytes(B, frames) / 2);
  int32_t* pp = path + (size_t)sig * frames;
  const double ninf = -__builtin_huge_val();
  long long tick0 = 0, tick1 = 0;
  if (ticks && b == 0) tick0 = wall_clock64();
  for (int d = b; d <= J; d += blockDim.x) pens[d] = pen[d];
  // frame 0
  {
    double d0 = ninf;
    if (voiced) {
      d0 = ep[0];
      D[0][b] = d0;
    }
    if (b == ub) D[0][B] = theta;
    int lane;
    const double m = wave_first_max(voiced ? d0 - nu : ninf, lane);
    if ((b & 63) == 0) {
      wv[0][wave] = m;
      wi[0][wave] = (wave << 6) + lane;
    }
  }
  double en = voiced && frames > 1 ? ep[1] : 0.0;         // e[b][t] of the next frame, fetched a frame ahead
  lds_barrier();
  for (int t = 1; t < frames; ++t) {
    const int cur = t & 1, prev = cur ^ 1;
    const double et = en;
    if (voiced && t + 1 < frames) en = ep[t + 1];
    uint16_t* row = bpp + (size_t)t * (B + 1);
    double dn = ninf;
    if (voiced) {
      double best = D[prev][B] - nu;
      int arg = B;
      const int lo = b - J > 0 ? b - J : 0, hi = b + J < B - 1 ? b + J : B - 1;
#pragma unroll 4
      for (int c = lo; c <= hi; ++c) {
        const double v = D[prev][c] - pens[c < b ? b - c : c - b];
        if (v > best) {
          best = v;
          arg = c;
        }
      }
      dn = et + best;
      D[cur][b] = dn;
      row[b] = (uint16_t)arg;
    }
    if (b == ub) {
      double best = D[prev][B];
      int arg = B;
      for (int k = 0; k < nw; ++k) {                     // the waves in order: the earliest of equal maxima stays
        const double v = wv[prev][k];
        if (v > best) {
          best = v;
          arg = wi[prev][k];
        }
      }
      D[cur][B] = theta + best;
      row[B] = (uint16_t)arg;
    }
    int lane;
    const double m = wave_first_max(voiced ? dn - nu : ninf, lane);
    if ((b & 63) == 0) {
      wv[cur][wave] = m;
      wi[cur][wave] = (wave << 6) + lane;
    }
    lds_barrier();
  }
  // the end: the first maximum of D[0 .. B] in state order
  const int last = (frames - 1) & 1;
  int state = 0;
  if (wave == 0) {
    Cand c = {ninf, 0x7fffffff};
    for (int k = b; k <= B; k += 64) {
      const Cand x = {D[last][k], k};
      c = cand_best(c, x);
    }
    c = wave_best(c);
    state = c.i;
  }
  if (ticks && b == 0) tick1 = wall_clock64();
  // the back-trace: frames (lo, hi] of back pointers at a time through LDS; thread 0 walks
  const int tc = trk_chunk_frames(B);
  for (int hi = frames - 1; hi > 0; hi -= tc) {
    const int lo = hi - tc > 0 ? hi - tc : 0;
    const int n = (hi - lo) * (B + 1);
    const uint16_t* src = bpp + (size_t)(lo + 1) * (B + 1);
    __syncthreads();                                     // the back pointers are written, the last chunk is walked
    for (int k = b; k < n; k += blockDim.x) chunk[k] = src[k];
    __syncthreads();
    if (b == 0)
      for (int t = hi; t > lo; --t) {
        pp[t] = state;
        state = chunk[(t - lo - 1) * (B + 1) + state];
      }
  }
  if (b == 0) {
    pp[0] = state;
    if (ticks) {
      ticks[2 * sig] = tick1 - tick0;
      ticks[2 * sig + 1] = wall_clock64() - tick1;
    }
  }
}

__global__ __launch_bounds__(MSK_THREADS) void k_melody_mask(const int32_t* __restrict__ path, int frames, const double* __restrict__ f0, int B, int rows,
                                                              int Hm, double width, double bin_hz, int blocks, float* __restrict__ mask) {
#pragma clang fp contract(off)
  const int sig = blockIdx.x / blocks;
  const int64_t cell = (int64_t)(blockIdx.x - sig * blocks) * MSK_THREADS + threadIdx.x;
  if (cell >= (int64_t)rows * frames) return;
  const int f = (int)(cell / frames), t = (int)(cell - (int64_t)f * frames);
  const int p = path[(size_t)sig * frames + t];
  float out = 0.0f;
  if (p >= 0 && p < B) {
    const double g = f0[p], x = (double)f * bin_hz;
    const double r = rint(x / g);
    const int h0 = !(r >= 1.0) ? 1 : (r > (double)Hm ? Hm : (int)r);
    double d = __builtin_huge_val();
    for (int h = h0 - 1; h <= h0 + 1; ++h)               // the nearest harmonic is one of these whichever way x / g rounded
      if (h >= 1 && h <= Hm) {
        const double v = fabs(x - (double)h * g);
        d = v < d ? v : d;
      }
    const double m = 1.0 - d / width;
    out = (float)(m > 0.0 ? m : 0.0);
  }
  mask[(size_t)sig * rows * frames + cell] = out;
}

}  // namespace glowk_melody
