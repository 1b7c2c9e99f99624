// glowk device code: convolutive NMF (Smaragdis 2004, "NMFD"; Schmidt & Morup 2006): every component is a patch of Tw spectra, the
// activations say where the patches start.  V [nsig][rows][frames] float32 >= 0; W [nw][rows][K][Tw], Tw contiguous; H [nsig][K][frames].
//
// It is NMF with K Tw stacked components, s = k Tw + tau, whose activations are tied shifts of each other: Ws [rows][K Tw] is W's own
// memory, Hs[s][t] = H[k][t - tau] (an exact 0 for t < tau), Lambda = Ws Hs.  The kernels are glowk_nmf.h's with two changes: the
// Hs operand is never in memory -- the shift is applied where H is loaded, one clamped unconditional load per element and an exact
// zero in registers where t < tau (nmf_keep, the pattern of the "past the end" handling) -- and the H update adds the shifts up:
//
//   k_nmfd_update_h   the stacked numerators and denominators Ws^T Q and Ws^T P, [2][K Tw][frames], to the workspace; k_nmf_update_h's
//                     tile walk, the same chains in the same order
//   k_nmfd_h_finish   N[k][t] = sum over tau of the stacked numerator [k Tw + tau][t + tau], t + tau < frames, tau ascending; D
//                     likewise; H' = H g(N / max(D, FLOOR))
//   k_nmfd_update_w   k_nmf_update_w on (V, Ws, Hs); k_nmf_w_finish itself finishes it
//   k_nmfd_divergence k_nmf_divergence on (V, Ws, Hs); k_nmf_div_reduce itself reduces it
//   k_nmfd_masks      k_nmf_masks on (Ws, Hs), the bounds in stacked components
//
// The chain order over s, the tiles and the chunk plan (nmf_plan at K Tw components) are the NMF kernels', so the W update, the
// divergence and the masks give the bits glowk_nmf_* give on a materialised Hs, and at Tw = 1 so does the H update (a sum of one
// term).  Lambda, Q and P exist in registers alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glowk_nmf.h"
#include "glowk_nmfd_index.h"

namespace glowk_nmfd {

using glowk_nmf::f32x16;
using glowk_nmf::FLOOR;
using glowk_nmf::nmf_chunk;
using glowk_nmf::nmf_keep;
using glowk_nmf::nmf_qp;
using glowk_nmf::nmf_rho;
using glowk_nmf::nmf_step;
using glowk_nmf::nmf_term;
using glowk_nmf::nmf_w_part_floats;
using glowk_nmf::nmf_w_part_index;
using glowk_nmf::NmfBounds;
using glowk_nmf::TILE;
using glowk_nmf::WAVES;

// KS = K Tw stacked components, padded to KP = 32 KT.  H is read, never written: the workgroups' frames overlap through the shifts.
template <int KT>
__global__ __launch_bounds__(256) void k_nmfd_update_h(const float* __restrict__ V, const float* __restrict__ W, int64_t wstride, const float* __restrict__ H,
                                                       float* __restrict__ plane, int rows, int F, int K, int Tw, int ftiles, int beta) {
  constexpr int KP = TILE * KT, PW = KP + 1;
  __shared__ float lds[WAVES * TILE * PW];                       // a W tile per wave; at the end the waves' accumulators [4][KP][32]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  const int KS = K * Tw;
  const int64_t sig = blockIdx.x / (unsigned)ftiles;
  const int f0 = (int)(blockIdx.x % (unsigned)ftiles) * TILE;
  const float* v = V + sig * rows * F;
  const float* w = W + sig * wstride;
  const float* h = H + sig * K * F;
  const int f = f0 + c, fc = min(f, F - 1);                        // past the end: the address clamped, the operand zero
  const bool fv = f < F;
  float hb[KP / 2];
  {
    int k, tau;                                                   // of min(s, the last stacked component of the lane's parity)
    nmfd_split(min(half, KS - 1), Tw, k, tau);
#pragma unroll
    for (int kk = 0; kk < KP / 2; ++kk) {
      const int s = 2 * kk + half, t = f - tau;                   // Hs[s][f] = H[k][f - tau], an exact zero before the signal starts
      hb[kk] = nmf_keep(h[(int64_t)k * F + min(max(t, 0), F - 1)], fv && s < KS && t >= 0);
      nmfd_advance2(Tw, k, tau, s + 2 < KS);
    }
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
      for (int kt = 0; kt < KT; ++kt) a2[kt][r] = w[(int64_t)rc * KS + min(kt * TILE + c, KS - 1)];
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
    // A row past the end adds exact zeros: Q = P = 0.  Stacked components past KS are exact zeros in hb; frames past the end likewise.
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
  // the four waves' sums in wave order; thread t owns the elements t + 256 i = (s, frame) = (e >> 5, e & 31)
  float* red = lds;
  float* po = plane + sig * nmfd_plane_floats(KS, F);
  for (int which = 0; which < 2; ++which) {
    __syncthreads();
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[wave * KP * TILE + (kt * TILE + nmf_rho(r, half)) * TILE + c] = which ? den[kt][r] : num[kt][r];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4 * KT; ++i) {
      const int e = (int)threadIdx.x + 256 * i;
      const float x = ((red[e] + red[KP * TILE + e]) + red[2 * KP * TILE + e]) + red[3 * KP * TILE + e];
      const int s = e >> 5, fo = f0 + (e & 31);
      if (s < KS && fo < F) po[nmfd_plane_index(which, s, fo, KS, F)] = x;
    }
  }
}

// thread e = (signal, k, t): the shifts of a component in tau order, then the step
__global__ __launch_bounds__(256) void k_nmfd_h_finish(const float* __restrict__ plane, int64_t total, int K, int Tw, int F, int beta, float* __restrict__ H) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int KS = K * Tw, t = (int)(e % F), k = (int)((e / F) % K);
  const float* p = plane + (e / ((int64_t)K * F)) * nmfd_plane_floats(KS, F);
  const int taps = nmfd_taps(Tw, F, t);
  float n = 0.0f, d = 0.0f;
  for (int tau = 0; tau < taps; ++tau) {
    n += p[nmfd_plane_index(0, k * Tw + tau, t + tau, KS, F)];
    d += p[nmfd_plane_index(1, k * Tw + tau, t + tau, KS, F)];
  }
  H[e] = nmf_step(beta, H[e], n, d);
}

template <int KT>
__global__ __launch_bounds__(256) void k_nmfd_update_w(const float* __restrict__ V, const float* __restrict__ W, const float* __restrict__ H, int rows, int F,
                                                       int K, int Tw, NmfPlan plan, int beta, float* __restrict__ part) {
  constexpr int KP = TILE * KT, PT = TILE + 1, PER = (KP + TILE) * PT;
  __shared__ float lds[WAVES * PER];                             // per wave an Hs tile [KP][33] and a V tile [32][33]; at the end [4][KP][33]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  const int KS = K * Tw;
  unsigned b = blockIdx.x;
  const int ch = (int)(b % (unsigned)plan.nch);
  b /= (unsigned)plan.nch;
  const int r0 = (int)(b % (unsigned)plan.rtiles) * TILE;
  const int64_t sig = b / (unsigned)plan.rtiles;
  const float* v = V + sig * rows * F;
  const float* w = W + sig * rows * KS;
  const float* h = H + sig * K * F;
  const int wrow = r0 + c;
  float wb[KP / 2];
#pragma unroll
  for (int kk = 0; kk < KP / 2; ++kk) {                           // past the end: the address clamped, the operand zero
    const int s = 2 * kk + half;
    wb[kk] = nmf_keep(w[(int64_t)min(wrow, rows - 1) * KS + min(s, KS - 1)], wrow < rows && s < KS);
  }
  f32x16 num[KT], den[KT];
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) num[kt][r] = den[kt][r] = 0.0f;
  }
  float* hs = lds + wave * PER;
  float* vt = hs + KP * PT;
  // Hs[min(2 kk + half, the last stacked component of the lane's parity)][f] = H[k][f - tau]: the row offset k F < 2^22 and tau < 32 of
  // every kk in one register, found once without a division
  unsigned hrow[KP / 2];
  {
    int k, tau;
    nmfd_split(min(half, KS - 1), Tw, k, tau);
#pragma unroll
    for (int kk = 0; kk < KP / 2; ++kk) {
      hrow[kk] = ((unsigned)k * (unsigned)F) << 5 | (unsigned)tau;
      nmfd_advance2(Tw, k, tau, 2 * kk + half + 2 < KS);
    }
  }
  unsigned vrow[16];                                             // rows * frames of one signal fits 31 bits
#pragma unroll
  for (int r = 0; r < 16; ++r) vrow[r] = (unsigned)min(r0 + nmf_rho(r, half), rows - 1) * (unsigned)F;
  int t0, t1;
  nmf_chunk(plan, ch, t0, t1);
  for (int t = t0 + wave; t < t1; t += WAVES) {                   // wave-uniform
    const int fc = min(t * TILE + c, F - 1);
    float ha[KP / 2], vr[16];
    // Every load before the first use.  The packed (row offset, tau) goes through a value the compiler cannot see through, once per
    // tile, so that no address or lane mask outlives its load (64 of each, the same for every tile, would be kept in registers
    // beside the 64 packed ones).
#pragma unroll
    for (int kk = 0; kk < KP / 2; ++kk) {
      unsigned pk = hrow[kk];
      asm volatile("" : "+v"(pk));
      ha[kk] = h[(pk >> 5) + (unsigned)max(fc - (int)(pk & 31u), 0)];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) vr[r] = v[(unsigned)(vrow[r] + fc)];
#pragma unroll
    for (int kk = 0; kk < KP / 2; ++kk) {                         // after the last load is issued: volatile statements keep their order
      unsigned pk = hrow[kk];
      asm volatile("" : "+v"(pk));
      ha[kk] = nmf_keep(ha[kk], fc >= (int)(pk & 31u));
      hs[(2 * kk + half) * PT + c] = ha[kk];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) vt[nmf_rho(r, half) * PT + c] = vr[r];
    __builtin_amdgcn_wave_barrier();
    f32x16 lam;                                                   // Lambda^T: register r holds (frame rho(r, half), row c)
#pragma unroll
    for (int r = 0; r < 16; ++r) lam[r] = 0.0f;
#pragma unroll
    for (int kk = 0; kk < KP / 2; ++kk) lam = __builtin_amdgcn_mfma_f32_32x32x2f32(ha[kk], wb[kk], lam, 0, 0, 0);
    // A frame past the end (its operands are the last frame's, finite) adds exact zeros: Q = P = 0.  Stacked components past KS are
    // exact zeros in wb; the accumulator rows past KS and the rows past the end are never written.
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
  // the four waves' sums in wave order; thread t owns the elements t + 256 i = (row, s) = (e / KP, e % KP)
  float* red = lds;
  float* po = part + sig * nmf_w_part_floats(plan, rows, KS);
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
      const int rl = e / KP, s = e % KP, x = s * PT + rl;
      const float sum = ((red[x] + red[KP * PT + x]) + red[2 * KP * PT + x]) + red[3 * KP * PT + x];
      if (r0 + rl < rows && s < KS) po[nmf_w_part_index(ch, which, r0 + rl, s, rows, KS)] = sum;
    }
  }
}

// Lambda of one 32 x 32 tile over the stacked components [lo, hi): register r holds (row r0 + rho(r, half), frame f0 + c).
// nmf_lambda's chain with the Hs operand taken from H.
__device__ __forceinline__ f32x16 nmfd_lambda(const float* __restrict__ w, const float* __restrict__ h, int rows, int F, int KS, int Tw, int r0, int f0, int lo,
                                              int hi, int c, int half) {
  f32x16 lam;
#pragma unroll
  for (int r = 0; r < 16; ++r) lam[r] = 0.0f;
  const int row = r0 + c, f = f0 + c, fc = min(f, F - 1);
  const float* wr = w + (int64_t)min(row, rows - 1) * KS;          // past the end: the address clamped, the operand zero
  int k, tau;                                                     // of min(s, KS - 1): a stacked component that exists
  nmfd_split(min(lo + half, KS - 1), Tw, k, tau);
  for (int s0 = lo; s0 < hi; s0 += 2) {
    const int s = s0 + half, ts = fc - tau;
    const float a = wr[min(s, hi - 1)], b = h[(int64_t)k * F + max(ts, 0)];
    lam = __builtin_amdgcn_mfma_f32_32x32x2f32(nmf_keep(a, row < rows && s < hi), nmf_keep(b, f < F && s < hi && ts >= 0), lam, 0, 0, 0);
    nmfd_advance2(Tw, k, tau, s + 2 < KS);
  }
  return lam;
}

__global__ __launch_bounds__(256) void k_nmfd_divergence(const float* __restrict__ V, const float* __restrict__ W, int64_t wstride, const float* __restrict__ H,
                                                         int rows, int F, int K, int Tw, NmfPlan plan, int beta, double* __restrict__ part) {
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
    const f32x16 lam = nmfd_lambda(w, h, rows, F, K * Tw, Tw, r0, f0, 0, K * Tw, c, half);
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

// k_nmf_masks with the bounds in stacked components: one wave per 32 x 32 tile, four frame tiles per workgroup, two passes over the
// sources.  X [nsig][C][rows][frames] complex64 and spec [nsig][S][C][rows][frames] or null.
__global__ __launch_bounds__(256) void k_nmfd_masks(const float* __restrict__ W, int64_t wstride, const float* __restrict__ H, int rows, int F, int K, int Tw,
                                                    int rtiles, int fgroups, NmfBounds bounds, int S, int power, const float2* __restrict__ X, int C,
                                                    float* __restrict__ masks, float2* __restrict__ spec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  unsigned b = blockIdx.x;
  const int f0 = ((int)(b % (unsigned)fgroups) * WAVES + wave) * TILE;
  b /= (unsigned)fgroups;
  const int r0 = (int)(b % (unsigned)rtiles) * TILE;
  const int64_t sig = b / (unsigned)rtiles;
  if (f0 >= F) return;                                            // wave-uniform; no barrier follows
  const int KS = K * Tw;
  const float* w = W + sig * wstride;
  const float* h = H + sig * K * F;
  const int f = f0 + c;
  f32x16 tot;
#pragma unroll
  for (int r = 0; r < 16; ++r) tot[r] = 0.0f;
  for (int s = 0; s < S; ++s) {
    const f32x16 lam = nmfd_lambda(w, h, rows, F, KS, Tw, r0, f0, bounds.b[s], bounds.b[s + 1], c, half);
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] += power == 2 ? lam[r] * lam[r] : lam[r];
  }
  const float even = 1.0f / (float)S;
  const int64_t pl = (int64_t)rows * F;
  for (int s = 0; s < S; ++s) {
    const f32x16 lam = nmfd_lambda(w, h, rows, F, KS, Tw, r0, f0, bounds.b[s], bounds.b[s + 1], c, half);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = r0 + nmf_rho(r, half);
      if (row < rows && f < F) {
        const float m = power == 2 ? lam[r] * lam[r] : lam[r];
        const float mk = tot[r] < FLOOR ? even : m / tot[r];
        const int64_t cell = (int64_t)row * F + f;
        masks[(sig * S + s) * pl + cell] = mk;
        if (X) {
          for (int x = 0; x < C; ++x) {
            const float2 z = X[(sig * C + x) * pl + cell];
            spec[((sig * S + s) * C + x) * pl + cell] = make_float2(mk * z.x, mk * z.y);
          }
        }
      }
    }
  }
}

}  // namespace glowk_nmfd
