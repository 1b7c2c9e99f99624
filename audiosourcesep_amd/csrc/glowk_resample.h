// glowk device code, part 7: band-limited sample-rate conversion (the resampling inside librosa.core.load, datasets/preprocessing.py:21).
//
// The filter is librosa 0.7's default design (resampy's kaiser_best: a Kaiser-windowed sinc, Z = 64 zero crossings, P = 512 table
// points per zero crossing, beta = 14.769656459379492, roll-off rho = 0.9475937167399596), evaluated at the exact position of
// every tap.  With a = sr_in / gcd, b = sr_out / gcd, d = max(a, b), s = min(1, b / a) and t a = q b + r (64-bit integers):
//
//     y[t] = s sum_m x[m] h(s ((q - m) + r / b)),    h(u) = T[k] + (p - k) (T[k + 1] - T[k]),  p = |u| P,  k = floor(p)
//
// The table position of the tap at distance j = q - m is p = |j b + r| P / d, a ratio of integers: k and the remainder come from
// integer arithmetic (one division per side, then += (b P) div d, += (b P) mod d with a carry per tap), so the position of an output
// never depends on how many came before it.
//
//   k_resample    one workgroup = RS_THREADS threads = `tb` consecutive outputs of one signal (tb <= RS_THREADS, smaller only for
//                 ratios whose input span would not fit the LDS); the input span [q_lo - H, q_hi + H] is staged in LDS, zero outside
//                 the signal; the table, as pairs (T[k], T[k + 1] - T[k]), is gathered from global memory (256 KB: L2-resident).
//                 Summation order of one output, fixed relative to its centre q: the taps m = q, q - 1, ... (outwards) in one fp32
//                 FMA chain, the taps m = q + 1, q + 2, ... in a second one, y = s (right + left).  A tap outside the signal
//                 multiplies a zero, which leaves the chains bit-identical to skipping it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace glowk_rs {

constexpr int RS_Z = 64, RS_P = 512, RS_ZP = RS_Z * RS_P;    // the table holds k = 0 .. Z P
constexpr int RS_THREADS = 256;
constexpr int RS_LDS_FLOATS = 15360;                          // 60 KB: the staged span of the widest supported ratio still holds 111 outputs

struct ResampleArgs {
  const float* x = nullptr;        // [nsig][n_in]
  float* y = nullptr;              // [nsig][n_out]
  const float2* tab = nullptr;     // [Z P + 1] (T[k], T[k + 1] - T[k]); the last difference is 0
  int64_t n_in = 0, n_out = 0, blocks_per_sig = 0;
  uint32_t a = 1, b = 1, d = 1;      // reduced rates, d = max(a, b)
  uint32_t stepk = 0, stepr = 0; // (b P) div d, (b P) mod d: the table advance of one tap
  int H = 0;                 // taps per side at most: floor(Z d / b) + 1
  int tb = 0;                // outputs per workgroup
  float scale = 1.0f, inv_d = 1.0f;    // s = min(1, b / a); 1 / d
};
static_assert(sizeof(ResampleArgs) == 88 && std::is_trivially_copyable_v<ResampleArgs>, "kernel argument size");

__global__ __launch_bounds__(RS_THREADS) void k_resample(ResampleArgs g) {
  extern __shared__ float xs[];                        // x[m0 .. m0 + span)
  const int tid = threadIdx.x;
  const int64_t sig = (int64_t)blockIdx.x / g.blocks_per_sig, blk = (int64_t)blockIdx.x % g.blocks_per_sig;
  const int64_t t0 = blk * g.tb;
  const int64_t t_last = (t0 + g.tb - 1 < g.n_out - 1) ? t0 + g.tb - 1 : g.n_out - 1;
  const int64_t q_lo = (t0 * (int64_t)g.a) / g.b, q_hi = (t_last * (int64_t)g.a) / g.b;
  const int64_t m0 = q_lo - g.H;
  const int span = (int)(q_hi - q_lo) + 2 * g.H + 1;   // <= the host's bound (glowk_resample), which sized the LDS
  const float* __restrict__ x = g.x + sig * g.n_in;
  for (int i = tid; i < span; i += RS_THREADS) {
    const int64_t m = m0 + i;
    xs[i] = (m >= 0 && m < g.n_in) ? x[m] : 0.0f;
  }
  __syncthreads();
  const int64_t t = t0 + tid;
  if (tid >= g.tb || t >= g.n_out) return;
  const int64_t ta = t * (int64_t)g.a, q = ta / g.b;
  const uint32_t r = (uint32_t)(ta - q * g.b);
  const int c = (int)(q - m0);                          // xs[c] = x[q]; c - i >= 1 and c + 1 + i < span for every tap below
  // right side: m = q - i, numerator N = i b + r; left side: m = q + 1 + i, N = (i + 1) b - r.  N P < 2^29 at i = 0.
  uint32_t kr = (r * RS_P) / g.d, rr = (r * RS_P) % g.d;
  uint32_t kl = ((g.b - r) * RS_P) / g.d, rl = ((g.b - r) * RS_P) % g.d;
  float accr = 0.0f, accl = 0.0f;
  // a tap counts while p <= Z P: k < Z P, or k == Z P with no remainder
  bool onr = kr < RS_ZP || (kr == RS_ZP && rr == 0), onl = kl < RS_ZP || (kl == RS_ZP && rl == 0);
  for (int i = 0; onr || onl; ++i) {
    if (onr) {
      const float2 w = g.tab[kr];
      accr = fmaf(xs[c - i], fmaf((float)rr * g.inv_d, w.y, w.x), accr);
      kr += g.stepk; rr += g.stepr;
      if (rr >= g.d) { rr -= g.d; ++kr; }
      onr = kr < RS_ZP || (kr == RS_ZP && rr == 0);
    }
    if (onl) {
      const float2 w = g.tab[kl];
      accl = fmaf(xs[c + 1 + i], fmaf((float)rl * g.inv_d, w.y, w.x), accl);
      kl += g.stepk; rl += g.stepr;
      if (rl >= g.d) { rl -= g.d; ++kl; }
      onl = kl < RS_ZP || (kl == RS_ZP && rl == 0);
    }
  }
  g.y[sig * g.n_out + t] = g.scale * (accr + accl);
}

}  // namespace glowk_rs
