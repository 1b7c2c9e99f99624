// glowk device code: non-negative matrix factorisation by multiplicative updates (Lee & Seung 2001; Fevotte & Idier 2011 for the
// beta divergences and the majorise-minimise exponent), the divergence, and ratio masks of component ranges.
// V [nsig][rows][frames] float32 >= 0, frames contiguous; W [nw][rows][K], K contiguous; H [nsig][K][frames]; FLOOR = 2^-40.
//
//   k_nmf_update_h    H' = H g(W^T Q / max(W^T P, FLOOR)): a workgroup owns 32 frames and all K components and walks the rows
//   k_nmf_update_w    partial Q H^T and P H^T of a 32-row tile over one chunk of the frames, to the workspace
//   k_nmf_w_finish    W' = W g(sum of the chunks' Q H^T / max(sum of the chunks' P H^T, FLOOR)), the chunks in order
//   k_nmf_divergence  partial sums of D_beta(V | max(W H, FLOOR)) in fp64, per (row tile, chunk)
//   k_nmf_div_reduce  the partial sums of a signal in a fixed order
//   k_nmf_masks       mask_s = (W_s H_s)^power / sum over the sources, and optionally mask_s X
//
// Every product is on v_mfma_f32_32x32x2_f32 (exact fp32: an fma chain).  Lane l = (c, half) = (l & 31, l >> 5) gives the A operand
// A[c][half] and the B operand B[half][c] of D[32][32] += A[32][2] B[2][32]; accumulator register r of the lane holds
// D[rho(r, half)][c], rho = (r & 3) + 8 (r >> 2) + 4 half.  K is padded to KP = 32 KT with operands that are exact zeros, rows and
// frames past the end read a clamped address, so the loads of a tile are unconditional and all in flight together, and add exact
// zeros: Q = P = 0 there.
//
// k_nmf_update_h.  Wave w of the four takes the row tiles w, w + 4, ..; per tile of 32 rows it
//   1. loads the W tile as the second chain's A operand, a2[kt][r] = W[row rho(r, half)][32 kt + c] (two 128-byte runs per load),
//      and writes it to its own LDS tile [32][KP + 1]; loads V[row rho(r, half)][frame c] the same way;
//   2. Lambda[row][frame] = sum_k W[row][k] H[k][frame]: A from the LDS tile (lane stride KP + 1: no bank conflict), B = the H tile
//      H[2 kk + half][frame c], which the lane holds in KP / 2 registers for the whole kernel; KP / 2 MFMAs;
//   3. Q and P from Lambda and V, register by register -- Lambda's accumulator layout is the B layout of the second chain, row pair
//      (rho(r, 0), rho(r, 1)) in step r -- so they go straight into num[k][frame] += W[row][k] Q[row][frame] and den likewise:
//      2 x 16 KT MFMAs into 2 KT accumulators.  The rows are added in the order rho gives, the same for every element.
// Lambda, Q and P exist in registers alone.  At the end the four waves' accumulators are added in wave order through LDS and the
// workgroup writes H' over its own 32 frames of H (no other workgroup reads them).
//
// k_nmf_update_w is the transpose: the workgroup owns 32 rows (B operand W[row c][2 kk + half], KP / 2 registers) and the frame
// tiles of one chunk, wave w every fourth.  Per tile the H tile is loaded as the first chain's A operand H[2 kk + half][frame c]
// and written to LDS [KP][33] for the second chain's A operand H[32 kt + c][frame rho(r, half)]; V is loaded as in k_nmf_update_h
// and transposed through LDS [32][33], so that V[row c][frame rho(r, half)] meets Lambda^T = H^T W^T in its accumulator layout.
// The partial sums go to part[chunk][num, den][row][k]; the cut into chunks is nmf_plan's, a function of (rows, frames, K) alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glowk_nmf_index.h"
#include "glowk_repet.h"

namespace glowk_nmf {

using glowk_repet::f32x16;
constexpr float FLOOR = 0x1p-40f;

struct NmfBounds {
  int b[MAX_SRC + 1];
};

// A loaded operand or an exact zero.  A product, not a select: a select on a loaded value lets the compiler move the load under the
// condition, one branch and one wait per load; the loads here are unconditional (clamped addresses) and in flight together.  The
// arrays hold finite values, so x * 0 is an exact zero.
__device__ __forceinline__ float nmf_keep(float x, bool live) { return x * (live ? 1.0f : 0.0f); }

// The operands of the outer sums from one cell: beta 2: Q = V, P = Le; beta 1: Q = V / Le, P = 1; beta 0: Q = V / (Le Le), P = 1 / Le
__device__ __forceinline__ void nmf_qp(int beta, float v, float lam, float& q, float& p) {
  const float le = fmaxf(lam, FLOOR);
  if (beta == 2) { q = v; p = le; }
  else if (beta == 1) { q = v / le; p = 1.0f; }
  else { q = v / (le * le); p = 1.0f / le; }
}

__device__ __forceinline__ float nmf_step(int beta, float old, float num, float den) {
  const float x = num / fmaxf(den, FLOOR);
  return old * (beta == 0 ? sqrtf(x) : x);
}

template <int KT>
__global__ __launch_bounds__(256) void k_nmf_update_h(const float* __restrict__ V, const float* __restrict__ W, int64_t wstride, float* __restrict__ H,
                                                      int rows, int F, int K, int ftiles, int beta) {
  constexpr int KP = TILE * KT, PW = KP + 1;
  __shared__ float lds[WAVES * TILE * PW];                       // a W tile per wave; at the end the waves' accumulators [4][KP][32]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  const int64_t sig = blockIdx.x / (unsigned)ftiles;
  const int f0 = (int)(blockIdx.x % (unsigned)ftiles) * TILE;
  const float* v = V + sig * rows * F;
  const float* w = W + sig * wstride;
  float* h = H + sig * K * F;
  const int f = f0 + c, fc = min(f, F - 1);                        // past the end: the address clamped, the operand zero
  const bool fv = f < F;
  float hb[KP / 2];
#pragma unroll
  for (int kk = 0; kk < KP / 2; ++kk) {
    const int k = 2 * kk + half;
    hb[kk] = nmf_keep(h[(int64_t)min(k, K - 1) * F + fc], fv && k < K);
  }
  f32x16 num[KT], den[KT];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) num[kt][r] = den[kt][r] = 0.0f;
  }
  float* ws = lds + wave * TILE * PW;
  const int rtiles = (rows + TILE - 1) / TILE;
  for (int rt = wave; rt < rtiles; rt += WAVES) {                 // wave-uniform
    const int r0 = rt * TILE;
    float a2[KT][16], vv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {                                // every load is issued before the first is used
      const int rc = min(r0 + nmf_rho(r, half), rows - 1);
      vv[r] = v[(int64_t)rc * F + fc];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) a2[kt][r] = w[(int64_t)rc * K + min(kt * TILE + c, K - 1)];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) ws[nmf_rho(r, half) * PW + kt * TILE + c] = a2[kt][r];
    }
    __builtin_amdgcn_wave_barrier();
    f32x16 lam;
#pragma unroll
    for (int r = 0; r < 16; ++r) lam[r] = 0.0f;
#pragma unroll
    for (int kk = 0; kk < KP / 2; ++kk) lam = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[c * PW + 2 * kk + half], hb[kk], lam, 0, 0, 0);
    __builtin_amdgcn_wave_barrier();                              // the tile is free again
    // A row past the end (its operands are a clamped row's, finite) adds exact zeros: Q = P = 0.  Components past K are exact
    // zeros in hb, so Lambda is the sum over K; the accumulator rows past K are never written.  Frames past the end likewise.
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float q, p;
      nmf_qp(beta, vv[r], lam[r], q, p);
      const bool rv = r0 + nmf_rho(r, half) < rows;
      q = rv ? q : 0.0f;
      p = rv ? p : 0.0f;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        num[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[kt][r], q, num[kt], 0, 0, 0);
        den[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[kt][r], p, den[kt], 0, 0, 0);
      }
    }
  }
  // the four waves' sums in wave order, numerators first; thread t owns the elements t + 256 i = (k, frame) = (e >> 5, e & 31)
  float* red = lds;
  float ns[4 * KT];
  __syncthreads();
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave * KP * TILE + (kt * TILE + nmf_rho(r, half)) * TILE + c] = num[kt][r];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4 * KT; ++i) {
    const int e = (int)threadIdx.x + 256 * i;
    ns[i] = ((red[e] + red[KP * TILE + e]) + red[2 * KP * TILE + e]) + red[3 * KP * TILE + e];
  }
  __syncthreads();
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave * KP * TILE + (kt * TILE + nmf_rho(r, half)) * TILE + c] = den[kt][r];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4 * KT; ++i) {
    const int e = (int)threadIdx.x + 256 * i;
    const float ds = ((red[e] + red[KP * TILE + e]) + red[2 * KP * TILE + e]) + red[3 * KP * TILE + e];
    const int k = e >> 5, fo = f0 + (e & 31);
    if (k < K && fo < F) {
      float* o = h + (int64_t)k * F + fo;
      *o = nmf_step(beta, *o, ns[i], ds);
    }
  }
}

template <int KT>
__global__ __launch_bounds__(256) void k_nmf_update_w(const float* __restrict__ V, const float* __restrict__ W, const float* __restrict__ H, int rows, int F,
                                                      int K, NmfPlan plan, int beta, float* __restrict__ part) {
  constexpr int KP = TILE * KT, PT = TILE + 1, PER = (KP + TILE) * PT;
  __shared__ float lds[WAVES * PER];                             // per wave an H tile [KP][33] and a V tile [32][33]; at the end [4][KP][33]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  unsigned b = blockIdx.x;
  const int ch = (int)(b % (unsigned)plan.nch);
  b /= (unsigned)plan.nch;
  const int r0 = (int)(b % (unsigned)plan.rtiles) * TILE;
  const int64_t sig = b / (unsigned)plan.rtiles;
  const float* v = V + sig * rows * F;
  const float* w = W + sig * rows * K;
  const float* h = H + sig * K * F;
  const int wrow = r0 + c;
  float wb[KP / 2];
#pragma unroll
  for (int kk = 0; kk < KP / 2; ++kk) {                           // past the end: the address clamped, the operand zero
    const int k = 2 * kk + half;
    wb[kk] = nmf_keep(w[(int64_t)min(wrow, rows - 1) * K + min(k, K - 1)], wrow < rows && k < K);
  }
  f32x16 num[KT], den[KT];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) num[kt][r] = den[kt][r] = 0.0f;
  }
  float* hs = lds + wave * PER;
  float* vt = hs + KP * PT;
  // offsets into one signal's H, which has fewer than 2^31 elements: the lane's first row, the last row of its parity, two rows
  const unsigned hfirst = (unsigned)min(half, K - 1) * (unsigned)F, hstep = 2u * (unsigned)F;
  const unsigned hlast = (unsigned)(K - 1 >= half ? (K - 1) - ((K - 1 - half) & 1) : 0) * (unsigned)F;
  unsigned vrow[16];                                             // rows * frames of one signal fits 31 bits
#pragma unroll
  for (int r = 0; r < 16; ++r) vrow[r] = (unsigned)min(r0 + nmf_rho(r, half), rows - 1) * (unsigned)F;
  int t0, t1;
  nmf_chunk(plan, ch, t0, t1);
  for (int t = t0 + wave; t < t1; t += WAVES) {                   // wave-uniform
    const int fc = min(t * TILE + c, F - 1);
    float ha[KP / 2], vr[16];
    // Every load before the first use.  Row min(2 kk + half, the lane's last row) of H: the offset moves on by two rows until it
    // meets the last row of the lane's parity, and depends on the tile, so that no address outlives its load (64 addresses or 64
    // lane masks that do not change from tile to tile would be kept in registers otherwise).
    unsigned ho = hfirst + (unsigned)fc;
    const unsigned hend = hlast + (unsigned)fc;
#pragma unroll
    for (int kk = 0; kk < KP / 2; ++kk) {
      ha[kk] = h[ho];
      ho = min(ho + hstep, hend);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) vr[r] = v[(unsigned)(vrow[r] + fc)];
#pragma unroll
    for (int kk = 0; kk < KP / 2; ++kk) hs[(2 * kk + half) * PT + c] = ha[kk];
#pragma unroll
    for (int r = 0; r < 16; ++r) vt[nmf_rho(r, half) * PT + c] = vr[r];
    __builtin_amdgcn_wave_barrier();
    f32x16 lam;                                                   // Lambda^T: register r holds (frame rho(r, half), row c)
#pragma unroll
    for (int r = 0; r < 16; ++r) lam[r] = 0.0f;
#pragma unroll
    for (int kk = 0; kk < KP / 2; ++kk) lam = __builtin_amdgcn_mfma_f32_32x32x2f32(ha[kk], wb[kk], lam, 0, 0, 0);
    // A frame past the end (its operands are the last frame's, finite) adds exact zeros: Q = P = 0.  Components past K are exact
    // zeros in wb; the accumulator rows past K and the rows past the end are never written.
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int fl = nmf_rho(r, half);
      float q, p;
      nmf_qp(beta, vt[c * PT + fl], lam[r], q, p);
      const bool live = t * TILE + fl < F;
      q = live ? q : 0.0f;
      p = live ? p : 0.0f;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const float a = hs[(kt * TILE + c) * PT + fl];
        num[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, q, num[kt], 0, 0, 0);
        den[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, p, den[kt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_wave_barrier();                              // the tiles are free again
  }
  // the four waves' sums in wave order; thread t owns the elements t + 256 i = (row, k) = (e / KP, e % KP)
  float* red = lds;
  float* po = part + sig * nmf_w_part_floats(plan, rows, K);
  for (int which = 0; which < 2; ++which) {
    __syncthreads();
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[wave * KP * PT + (kt * TILE + nmf_rho(r, half)) * PT + c] = which ? den[kt][r] : num[kt][r];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4 * KT; ++i) {
      const int e = (int)threadIdx.x + 256 * i;
      const int rl = e / KP, k = e % KP, x = k * PT + rl;
      const float s = ((red[x] + red[KP * PT + x]) + red[2 * KP * PT + x]) + red[3 * KP * PT + x];
      if (r0 + rl < rows && k < K) po[nmf_w_part_index(ch, which, r0 + rl, k, rows, K)] = s;
    }
  }
}

__global__ __launch_bounds__(256) void k_nmf_w_finish(const float* __restrict__ part, int64_t total, int64_t per_sig, int64_t part_sig, int nch, int beta,
                                                      float* __restrict__ W) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;     // (signal, row, k)
  if (e >= total) return;
  const float* p = part + (e / per_sig) * part_sig + e % per_sig;
  float n = 0.0f, d = 0.0f;
  for (int ch = 0; ch < nch; ++ch) {
    n += p[(int64_t)(2 * ch) * per_sig];
    d += p[(int64_t)(2 * ch + 1) * per_sig];
  }
  W[e] = nmf_step(beta, W[e], n, d);
}

// Lambda of one 32 x 32 tile over the components [lo, hi): register r holds (row r0 + rho(r, half), frame f0 + c)
__device__ __forceinline__ f32x16 nmf_lambda(const float* __restrict__ w, const float* __restrict__ h, int rows, int F, int K, int r0, int f0, int lo, int hi,
                                             int c, int half) {
  f32x16 lam;
#pragma unroll
  for (int r = 0; r < 16; ++r) lam[r] = 0.0f;
  const int row = r0 + c, f = f0 + c;
  const float* wr = w + (int64_t)min(row, rows - 1) * K;           // past the end: the address clamped, the operand zero
  const float* hf = h + min(f, F - 1);
  for (int k0 = lo; k0 < hi; k0 += 2) {
    const int k = k0 + half, kc = min(k, hi - 1);
    const float a = wr[kc], b = hf[(int64_t)kc * F];
    lam = __builtin_amdgcn_mfma_f32_32x32x2f32(nmf_keep(a, row < rows && k < hi), nmf_keep(b, f < F && k < hi), lam, 0, 0, 0);
  }
  return lam;
}

__device__ __forceinline__ double nmf_term(int beta, float v, float lam) {
  const double le = (double)fmaxf(lam, FLOOR), x = (double)v;
  if (beta == 2) return 0.5 * (x - le) * (x - le);
  if (beta == 1) return (v > 0.0f ? x * log(x / le) : 0.0) - x + le;
  const double q = fmax(x, (double)FLOOR) / le;
  return q - log(q) - 1.0;
}

__global__ __launch_bounds__(256) void k_nmf_divergence(const float* __restrict__ V, const float* __restrict__ W, int64_t wstride, const float* __restrict__ H,
                                                        int rows, int F, int K, NmfPlan plan, int beta, double* __restrict__ part) {
  __shared__ double wsum[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  unsigned b = blockIdx.x;
  const int ch = (int)(b % (unsigned)plan.nch);
  b /= (unsigned)plan.nch;
  const int r0 = (int)(b % (unsigned)plan.rtiles) * TILE;
  const int64_t sig = b / (unsigned)plan.rtiles;
  const float* v = V + sig * rows * F;
  const float* w = W + sig * wstride;
  const float* h = H + sig * K * F;
  int t0, t1;
  nmf_chunk(plan, ch, t0, t1);
  double acc = 0.0;
  for (int t = t0 + wave; t < t1; t += WAVES) {
    const int f0 = t * TILE, f = f0 + c;
    const f32x16 lam = nmf_lambda(w, h, rows, F, K, r0, f0, 0, K, c, half);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = r0 + nmf_rho(r, half);
      if (row < rows && f < F) acc += nmf_term(beta, v[(int64_t)row * F + f], lam[r]);
    }
  }
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
  if (lane == 0) wsum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one wave per signal: lane l adds the partial sums l, l + 64, .. in order, then the lanes add up in a fixed tree
__global__ __launch_bounds__(64) void k_nmf_div_reduce(const double* __restrict__ part, int64_t per_sig, double* __restrict__ out) {
  const double* p = part + (int64_t)blockIdx.x * per_sig;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < per_sig; i += 64) acc += p[i];
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

// One wave per 32 x 32 tile, four frame tiles per workgroup.  Two passes over the sources: the sum of the m_s, then every m_s again
// (the same instructions: the same bits) divided by it.  X [nsig][C][rows][frames] complex64 and spec [nsig][S][C][rows][frames] or null.
__global__ __launch_bounds__(256) void k_nmf_masks(const float* __restrict__ W, int64_t wstride, const float* __restrict__ H, int rows, int F, int K,
                                                   int rtiles, int fgroups, NmfBounds bounds, int S, int power, const float2* __restrict__ X, int C,
                                                   float* __restrict__ masks, float2* __restrict__ spec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  unsigned b = blockIdx.x;
  const int f0 = ((int)(b % (unsigned)fgroups) * WAVES + wave) * TILE;
  b /= (unsigned)fgroups;
  const int r0 = (int)(b % (unsigned)rtiles) * TILE;
  const int64_t sig = b / (unsigned)rtiles;
  if (f0 >= F) return;                                            // wave-uniform; no barrier follows
  const float* w = W + sig * wstride;
  const float* h = H + sig * K * F;
  const int f = f0 + c;
  f32x16 tot;
#pragma unroll
  for (int r = 0; r < 16; ++r) tot[r] = 0.0f;
  for (int s = 0; s < S; ++s) {
    const f32x16 lam = nmf_lambda(w, h, rows, F, K, r0, f0, bounds.b[s], bounds.b[s + 1], c, half);
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] += power == 2 ? lam[r] * lam[r] : lam[r];
  }
  const float even = 1.0f / (float)S;
  const int64_t plane = (int64_t)rows * F;
  for (int s = 0; s < S; ++s) {
    const f32x16 lam = nmf_lambda(w, h, rows, F, K, r0, f0, bounds.b[s], bounds.b[s + 1], c, half);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = r0 + nmf_rho(r, half);
      if (row < rows && f < F) {
        const float m = power == 2 ? lam[r] * lam[r] : lam[r];
        const float mk = tot[r] < FLOOR ? even : m / tot[r];
        const int64_t cell = (int64_t)row * F + f;
        masks[(sig * S + s) * plane + cell] = mk;
        if (X) {
          for (int x = 0; x < C; ++x) {
            const float2 z = X[(sig * C + x) * plane + cell];
            spec[((sig * S + s) * C + x) * plane + cell] = make_float2(mk * z.x, mk * z.y);
          }
        }
      }
    }
  }
}

}  // namespace glowk_nmf
