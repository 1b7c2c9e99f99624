// glowk device code, part 3: the BASIS Langevin update (run_basis_sep.py:106-181) for 2..16 sources as ONE elementwise kernel
// with its own counter-based RNG.  HBM-bound and tiny next to the S log_prob_grad calls of a step; what matters at the
// reference's 30 tiles is that it is one launch instead of the dozen elementwise/reduction launches of a tensor library.
// k_basis_update_n<S> is the only update kernel: the two-source entry points (glowk_basis_update, glowk_basis_mix) launch its
// S = 2 instance.  For the dB mixing process (:131-147; the linear mean of :108-116 is the other):
//
//   eps_k  = sqrt(2 eta) N(0, I)                                                 :163-164
//   mix    = 10/ln10 (logsumexp_k(x_k ln10/10) - ln S)                            :133-141  (g, sum in power)
//   m_k    = softmax_k(x_k ln10/10)                                               :143-147  (grad_g)
//   x_k   <- x_k + eta (grad_logprob_k + lambda m_k (mixed - mix)) + eps_k        :180-181
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1) -> 4 x 32 random bits.  Stateless, so element e of
// step t of stream w always gets the same draw whatever the grid.  The counter and the key as normal4 and k_basis_noise build them
// (include/glowk.h states the mapping next to glowk_random; tests/rng_ref.py restates it), for quad q = e / 4:
//   c0 = lo32(q), c1 = hi32(q) ^ (which << 28), c2 = lo32(step), c3 = hi32(step) ^ (pair << 16), key = (lo32(seed), hi32(seed)).
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// four standard normals for elements 4 q .. 4 q + 3 of (seed, step, which, pair): two Box-Muller pairs.  `pair` (the S-source
// update: source k draws which = k & 1, pair = k >> 1) goes into bits 16.. of the word that holds step >> 32, which is zero for
// every step < 2^32 and below bit 16 for step < 2^48; pair = 0 is the two-source stream.
__device__ __forceinline__ void normal4(uint64_t seed, uint64_t step, uint32_t which, uint64_t q, float (&z)[4], uint32_t pair = 0u) {
  uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32) ^ (which << 28), (uint32_t)step, (uint32_t)(step >> 32) ^ (pair << 16)};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = ((float)(c[2 * p] >> 8) + 0.5f) * (1.0f / 16777216.0f);        // (0, 1]: 24 bits, never 0; 1 at the largest word (r = 0)
    const float u2 = ((float)(c[2 * p + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.28318530717958647692f * u2, &sn, &cs);
    z[2 * p] = r * cs;
    z[2 * p + 1] = r * sn;
  }
}

__device__ __forceinline__ bool basis_bad(float v) { return !(fabsf(v) <= 3.0e38f); }

// ---- any number of sources (run_basis_sep.py:106-149: g(*sources), grad_g(*sources) for K = len(sources)) ---------------------
//   GLOWK_MIX_DB   (:131-147)  mix = 10/ln10 (logsumexp_k(x_k ln10/10) - ln S),  m_k = softmax_k(x_k ln10/10)
//   GLOWK_MIX_MEAN (:108-116)  mix = mean_k x_k,                                 m_k = 1/S
//   x_k <- x_k + eta (g_k + lambda m_k (mixed - mix)) + sqrt(2 eta) z_k          for k = 0..S-1
// The pointers travel by value in the kernel arguments.  S is a template parameter so that a thread's 4 S state values stay in
// registers between the reduction over the sources and the update: every x_k, g_k and mixed element is read from HBM once and
// every x_k written once, (3 S + 1) * 4 bytes per element.
#define GLOWK_BASIS_MAX_SOURCES 16

struct BasisNArgs {
  float* x[GLOWK_BASIS_MAX_SOURCES] = {};           // [n] each, in place
  const float* g[GLOWK_BASIS_MAX_SOURCES] = {};     // [n] grad log p_k(x_k)
  const float* eps[GLOWK_BASIS_MAX_SOURCES] = {};   // optional [n] standard-normal draws of source k; null: device RNG (k & 1, pair k >> 1)
  const float* mixed = nullptr;   // [n]
  size_t n = 0;
  float eta = 0.0f, lambda_recon = 0.0f, noise_scale = 0.0f;        // noise_scale = sqrt(2 eta)
  float ln_s = 0.0f, inv_s = 1.0f;    // ln S, 1 / S
  int mixing = 0;           // enum glowk_mixing
  int vec = 0;              // every pointer is 16-byte aligned: whole quads move as float4
  uint64_t seed = 0, step = 0, q0 = 0;
  int* nonfinite = nullptr;
};
static_assert(sizeof(BasisNArgs) == 464 && std::is_trivially_copyable_v<BasisNArgs>, "kernel argument size");

// The mixture and the weights m_k of one element from its S source values: v[k] holds x_k on entry and m_k on return, and
// mix = scale * t with t returned.  Wherever a product meets a sum the rounding is written out (__fmul_rn / fmaf) instead of
// left to the compiler's contraction, here and in the callers: it is the rounding of the two-source kernel this one replaced,
// whose results are pinned bit for bit (tests/golden/basis_two_source.npz).  The maximum is taken over the rounded products
// x_k L10; each difference x_k L10 - mx is one fma; the callers form mixed - mix as fmaf(-scale, t, mixed).
template <int S>
__device__ __forceinline__ float basis_mix_terms(float (&v)[S], int mixing, float ln_s, float inv_s, float& scale) {
  const float L10 = 0.23025850929940457f;   // ln 10 / 10
  if (mixing == 1) {                        // GLOWK_MIX_MEAN
    float sum = v[0];
#pragma unroll
    for (int k = 1; k < S; ++k) sum += v[k];
#pragma unroll
    for (int k = 0; k < S; ++k) v[k] = inv_s;
    scale = inv_s;
    return sum;
  }
  float mx = __fmul_rn(v[0], L10);
#pragma unroll
  for (int k = 1; k < S; ++k) mx = fmaxf(mx, __fmul_rn(v[k], L10));
#pragma unroll
  for (int k = 0; k < S; ++k) v[k] = expf(fmaf(v[k], L10, -mx));
  float den = v[0];
#pragma unroll
  for (int k = 1; k < S; ++k) den += v[k];
#pragma unroll
  for (int k = 0; k < S; ++k) v[k] = v[k] / den;
  scale = 1.0f / L10;
  return mx + logf(den) - ln_s;
}

// The update of one thread's four elements, in two parts that k_basis_update_n and k_basis_update_frames (glowk_frames.h) share.
// First the weights m[k][j] = m_k and r[j] = lambda (mixed - mix) of the elements from their S states; true if a mixture is not finite
template <int S>
__device__ __forceinline__ bool basis_quad_weights(const float (&x)[S][4], const float (&mixed)[4], int mixing, float ln_s, float inv_s,
                                                   float lambda_recon, float (&m)[S][4], float (&r)[4]) {
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float v[S];
#pragma unroll
    for (int k = 0; k < S; ++k) v[k] = x[k][j];
    float scale;
    const float t = basis_mix_terms<S>(v, mixing, ln_s, inv_s, scale);
#pragma unroll
    for (int k = 0; k < S; ++k) m[k][j] = v[k];
    r[j] = lambda_recon * fmaf(-scale, t, mixed[j]);
    bad |= basis_bad(__fmul_rn(scale, t));
  }
  return bad;
}

// then y = x_k + eta (g_k + m_k r) + noise_scale z_k for one source; true if a gradient or a result is not finite
__device__ __forceinline__ bool basis_quad_step(const float (&x)[4], const float (&m)[4], const float (&r)[4], const float (&g)[4],
                                                const float (&z)[4], float eta, float noise_scale, float (&y)[4]) {
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    y[j] = fmaf(noise_scale, z[j], fmaf(eta, fmaf(m[j], r[j], g[j]), x[j]));
    bad |= basis_bad(g[j]) | basis_bad(y[j]);
  }
  return bad;
}

// one thread = four consecutive elements of every source (one Philox call per source)
template <int S>
__global__ __launch_bounds__(256) void k_basis_update_n(BasisNArgs a) {
  const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const size_t e0 = (size_t)q * 4;
  if (e0 >= a.n) return;
  const bool quad = a.vec && e0 + 4 <= a.n;   // the tail quad and unaligned pointers move element by element
  float x[S][4], mixed[4];
  if (quad) {
    const float4 t = *reinterpret_cast<const float4*>(a.mixed + e0);
    mixed[0] = t.x; mixed[1] = t.y; mixed[2] = t.z; mixed[3] = t.w;
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const float4 u = *reinterpret_cast<const float4*>(a.x[k] + e0);
      x[k][0] = u.x; x[k][1] = u.y; x[k][2] = u.z; x[k][3] = u.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = e0 + j < a.n;           // lanes past n compute on zeros and are never stored
      mixed[j] = in ? a.mixed[e0 + j] : 0.0f;
#pragma unroll
      for (int k = 0; k < S; ++k) x[k][j] = in ? a.x[k][e0 + j] : 0.0f;
    }
  }
  float m[S][4], r[4];
  bool bad = basis_quad_weights<S>(x, mixed, a.mixing, a.ln_s, a.inv_s, a.lambda_recon, m, r);
#pragma unroll
  for (int k = 0; k < S; ++k) {
    float g[4], z[4];
    const float* eps = a.eps[k];
    if (quad) {
      const float4 t = *reinterpret_cast<const float4*>(a.g[k] + e0);
      g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = e0 + j < a.n ? a.g[k][e0 + j] : 0.0f;
    }
    if (!eps) {
      normal4(a.seed, a.step, (uint32_t)(k & 1), a.q0 + q, z, (uint32_t)(k >> 1));
    } else if (quad) {
      const float4 t = *reinterpret_cast<const float4*>(eps + e0);
      z[0] = t.x; z[1] = t.y; z[2] = t.z; z[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) z[j] = e0 + j < a.n ? eps[e0 + j] : 0.0f;
    }
    float y[4];
    bad |= basis_quad_step(x[k], m[k], r, g, z, a.eta, a.noise_scale, y);
    if (quad) {
      *reinterpret_cast<float4*>(a.x[k] + e0) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j < a.n) a.x[k][e0 + j] = y[j];
    }
  }
  if (bad && a.nonfinite) *a.nonfinite = 1;
}

struct BasisMixNArgs {
  const float* x[GLOWK_BASIS_MAX_SOURCES] = {};
  float* out = nullptr;
  size_t n = 0;
  float ln_s = 0.0f, inv_s = 1.0f;
  int mixing = 0;
};
static_assert(sizeof(BasisMixNArgs) == 160 && std::is_trivially_copyable_v<BasisMixNArgs>, "kernel argument size");

// g(x_0 .. x_{S-1}) alone
template <int S>
__global__ __launch_bounds__(256) void k_basis_mix_n(BasisMixNArgs a) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.n) return;
  float v[S];
#pragma unroll
  for (int k = 0; k < S; ++k) v[k] = a.x[k][e];
  float scale;
  const float t = basis_mix_terms<S>(v, a.mixing, a.ln_s, a.inv_s, scale);
  a.out[e] = __fmul_rn(scale, t);
}

// the standard-normal draws k_basis_update_n makes for (seed, step, which); also the engine's general device RNG
// (uniform = 1: U(0, 1) instead -- the reference starts the chain from uniform noise, run_basis_sep.py:360-361)
__global__ __launch_bounds__(256) void k_basis_noise(float* __restrict__ out, size_t n, uint64_t seed, uint64_t step, uint32_t which, int uniform,
                                                    uint64_t q0, uint32_t pair) {
  const uint64_t ql = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const size_t e0 = (size_t)ql * 4;
  if (e0 >= n) return;
  const uint64_t q = q0 + ql;     // position in the logical stream: a shard draws what the whole batch would have drawn for its elements
  float z[4];
  if (uniform) {
    uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32) ^ (which << 28), (uint32_t)step, (uint32_t)(step >> 32) ^ (pair << 16)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int j = 0; j < 4; ++j)     // the 25-bit sum rounds to even from 2^23 on, 16777215.5 to 2^24: clamped to the largest float below one
      z[j] = fminf(((float)(c[j] >> 8) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
  } else {
    normal4(seed, step, which, q, z, pair);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (e0 + j < n) out[e0 + j] = z[j];
}

// out = x + sigma N(0, I) with the draws of (seed, step, which) from element 4 q0 on: the noise of train_noisy_glow.py:31 (the
// noise-conditioned priors of BASIS are trained on X + tf.random.normal(X.shape) * noise) without a tensor-library kernel
__global__ __launch_bounds__(256) void k_add_noise(const float* __restrict__ x, float* __restrict__ out, size_t n, float sigma, uint64_t seed,
                                                  uint64_t step, uint32_t which, uint64_t q0) {
  const uint64_t ql = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const size_t e0 = (size_t)ql * 4;
  if (e0 >= n) return;
  float z[4];
  normal4(seed, step, which, q0 + ql, z);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (e0 + j < n) out[e0 + j] = fmaf(sigma, z[j], x[e0 + j]);
}
