// glowk device code, part 4: the audio ends of the pipeline -- the mel front end (datasets/data_loader.py:146-164) and the
// reuse-phase / Wiener mel inversion (melspec_inversion_basis.py:42-93, the `frame` method).  The constants of
// tile_io.MEL_FRONTEND are compiled in: 16 kHz, n_fft 2048, hop 512, 96 Slaney mels over 125..7600 Hz, -100..20 dB.
//
//   k_stft        X[b][f] = sum_n a[f*512 + n - 1024] hann[n] e^{-2 pi i b n / 2048}    (librosa.stft, center=True, reflect pad)
//                 one GEMM on v_mfma_f32_32x32x2_f32: A = the DFT basis (bins x samples, from a 2048-entry table indexed by the exact
//                 integer phase (b n) mod 2048), B = the windowed frames, gathered from the audio with the reflect indexing
//   k_mel_db      L = clip(max(10 log10(max(1e-10, W P)), max_extract(L) - top_db), -100, 20), one workgroup per extract
//                 (librosa.feature.melspectrogram + power_to_db + np.clip); W band-sparse
//   k_nnls        x = argmin_{x >= 0} |W x - 10^(L/10)|: FISTA from max(0, W+ b), a fixed number of iterations, all on chip
//                 (stands in for the L-BFGS-B NNLS of librosa.feature.inverse.mel_to_stft)
//   k_istft       Y = mask(x) X_mix (reuse phase or single-channel Wiener), y = istft(Y) (librosa.istft): the inverse real DFT as a
//                 GEMM on the same MFMA, overlap-add as a gather of the <= 4 frames of each output sample in a fixed order,
//                 the window-sum-square normalisation and the 1024-sample trim in the epilogue
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace glowk_audio {

constexpr int NFFT = 2048, HOP = 512, PAD = NFFT / 2, NBIN = NFFT / 2 + 1, NMEL = 96;
constexpr int MAX_FRAMES = 128;                      // k_mel_db holds an extract's [96][F] dB tile in LDS (48 KB at F = 128)
constexpr int GL_MAX_FRAMES = 1 << 20;               // Griffin-Lim signals: (F - 1) 512 samples and F 512 + 1024 stay below 2^31
constexpr int EXTRACT = 32640;                       // int(16000 * 2.04) samples (datasets/preprocessing.py:9-26)

typedef float f32x16 __attribute__((ext_vector_type(16)));

// device constants, built on the host in fp64 and rounded once (glowk_aux.hip: audio_consts), one copy per device
struct AudioConsts {
  const float* tab;      // [2048] cos(2 pi m / 2048); -sin(2 pi m / 2048) = tab[(m + 512) & 2047]
  const float* win;      // [2048] periodic Hann
  const int* mel_lo;     // [96] first bin of filter m
  const int* mel_len;    // [96] its number of bins (the filter is zero outside [lo, lo + len))
  const int* mel_off;    // [96] offset of its weights in mel_w
  const float* mel_w;    // packed band weights (Slaney mel scale and area normalisation, float32)
  const int* bin_mel;    // [1025][2] the <= 2 filters that cover a bin (the first slot is 0 with a zero weight if none)
  const float* bin_w;    // [1025][2] their weights
  const float* pinv;     // [1025][96] the pseudo-inverse of W (NNLS start)
  float step;            // 1 / |W|_2^2 (FISTA step)
};

// ---- STFT: one wave = 32 bins x 32 frames (re and im accumulators), 4 waves = 128 bins; K = 2048 samples in chunks of 256 ---------
constexpr int STFT_KC = 256, STFT_PITCH = STFT_KC + 1;

__device__ __forceinline__ int reflect_index(int t, int n) {   // numpy 'reflect' for a pad shorter than n
  t = t < 0 ? -t : t;
  return t >= n ? 2 * (n - 1) - t : t;
}

__global__ __launch_bounds__(256) void k_stft(const float* __restrict__ audio, int n_samples, int F, int ftiles, AudioConsts c,
                                              float* __restrict__ power, float* __restrict__ stft) {
  __shared__ float tab[NFFT];
  __shared__ float fs[32 * STFT_PITCH];              // 32 windowed frames x 256 samples of the current chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x / ftiles, f0 = (blockIdx.x % ftiles) * 32;
  const int bin0 = blockIdx.y * 128 + wave * 32;
  const float* a = audio + (size_t)n * n_samples;
  for (int i = tid; i < NFFT; i += 256) tab[i] = c.tab[i];
  f32x16 acc_re = {}, acc_im = {};
  const int bin = bin0 + (lane & 31), half = lane >> 5;
  for (int n0 = 0; n0 < NFFT; n0 += STFT_KC) {
    __syncthreads();                                 // the previous chunk has been consumed
    for (int i = tid; i < 32 * STFT_KC; i += 256) {
      const int fr = i / STFT_KC, nn = i % STFT_KC, f = f0 + fr;
      float v = 0.0f;
      if (f < F) v = a[reflect_index(f * HOP + n0 + nn - PAD, n_samples)] * c.win[n0 + nn];
      fs[fr * STFT_PITCH + nn] = v;
    }
    __syncthreads();
    if (bin0 < NBIN) {                               // wave-uniform: the last block's spare waves only help stage
#pragma unroll 8
      for (int kk = 0; kk < STFT_KC / 2; ++kk) {
        const int nl = 2 * kk + half;
        const int m = (bin * (n0 + nl)) & (NFFT - 1);
        const float b = fs[(lane & 31) * STFT_PITCH + nl];
        acc_re = __builtin_amdgcn_mfma_f32_32x32x2f32(tab[m], b, acc_re, 0, 0, 0);
        acc_im = __builtin_amdgcn_mfma_f32_32x32x2f32(tab[(m + 512) & (NFFT - 1)], b, acc_im, 0, 0, 0);
      }
    }
  }
  if (bin0 >= NBIN) return;
  const int f = f0 + (lane & 31);                    // C/D: column = lane & 31 (frame), row = (r & 3) + 8 (r >> 2) + 4 half (bin)
  if (f >= F) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int b = bin0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (b >= NBIN) continue;
    const size_t o = ((size_t)n * NBIN + b) * F + f;
    const float re = acc_re[r], im = acc_im[r];
    if (stft) reinterpret_cast<float2*>(stft)[o] = make_float2(re, im);
    else power[o] = re * re + im * im;
  }
}

// ---- mel + dB + per-extract floor: one workgroup per extract, the [96][F] tile in LDS (dynamic).  |X|^2 from the complex STFT when
// the caller takes it (X != null), else from k_stft's power scratch ----------------------------------------------------------------
__device__ __forceinline__ float bin_power(const float* __restrict__ power, const float2* __restrict__ X, size_t o) {
  if (!X) return power[o];
  const float2 v = X[o];
  return v.x * v.x + v.y * v.y;
}

__global__ __launch_bounds__(256) void k_mel_db(const float* __restrict__ power, const float2* __restrict__ X, int F, float top_db, AudioConsts c,
                                                float* __restrict__ mel_db) {
  extern __shared__ float tile[];                    // [96 * F]
  __shared__ float red[256];
  const int tid = threadIdx.x, n = blockIdx.x;
  const size_t base = (size_t)n * NBIN * F;
  float mx = -INFINITY;
  for (int o = tid; o < NMEL * F; o += 256) {
    const int m = o / F, f = o % F;
    const int lo = c.mel_lo[m], len = c.mel_len[m];
    const float* w = c.mel_w + c.mel_off[m];
    float s = 0.0f;
    for (int j = 0; j < len; ++j) s = fmaf(w[j], bin_power(power, X, base + (size_t)(lo + j) * F + f), s);
    const float db = 10.0f * log10f(fmaxf(s, 1e-10f));
    tile[o] = db;
    mx = fmaxf(mx, db);
  }
  red[tid] = mx;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {                // max is exact in any order: the result is deterministic
    if (tid < k) red[tid] = fmaxf(red[tid], red[tid + k]);
    __syncthreads();
  }
  const float floor_db = top_db > 0.0f ? red[0] - top_db : -INFINITY;
  float* out = mel_db + (size_t)n * NMEL * F;
  for (int o = tid; o < NMEL * F; o += 256) out[o] = fminf(fmaxf(fmaxf(tile[o], floor_db), -100.0f), 20.0f);
}

// ---- NNLS by FISTA: 8 frames per workgroup; y (the extrapolated point) in LDS, x in registers, no HBM traffic between iterations ---
constexpr int NNLS_G = 8, NNLS_SLOTS = (NBIN + 255) / 256;   // thread t owns bins t, t + 256, ... of all 8 frames

__global__ __launch_bounds__(256) void k_nnls(const float* __restrict__ mel_db, int F, int total, int iters, AudioConsts c,
                                              float* __restrict__ out) {
  __shared__ float y[NNLS_G][NBIN];
  __shared__ float bv[NNLS_G][NMEL];
  __shared__ float rv[NNLS_G][NMEL];
  const int tid = threadIdx.x, g0 = blockIdx.x * NNLS_G;
  for (int o = tid; o < NNLS_G * NMEL; o += 256) {
    const int fl = o / NMEL, m = o % NMEL, g = g0 + fl;
    float b = 0.0f;
    if (g < total) b = exp10f(0.1f * mel_db[((size_t)(g / F) * NMEL + m) * F + g % F]);   // librosa.db_to_power
    bv[fl][m] = b;
  }
  __syncthreads();
  float x[NNLS_SLOTS][NNLS_G], yr[NNLS_SLOTS][NNLS_G];
#pragma unroll
  for (int j = 0; j < NNLS_SLOTS; ++j) {
    const int b = tid + 256 * j;
#pragma unroll
    for (int fl = 0; fl < NNLS_G; ++fl) x[j][fl] = 0.0f;
    if (b < NBIN) {
      const float* pr = c.pinv + (size_t)b * NMEL;
      for (int m = 0; m < NMEL; ++m) {
        const float w = pr[m];
#pragma unroll
        for (int fl = 0; fl < NNLS_G; ++fl) x[j][fl] = fmaf(w, bv[fl][m], x[j][fl]);
      }
#pragma unroll
      for (int fl = 0; fl < NNLS_G; ++fl) {
        x[j][fl] = fmaxf(x[j][fl], 0.0f);
        y[fl][b] = x[j][fl];
      }
    }
#pragma unroll
    for (int fl = 0; fl < NNLS_G; ++fl) yr[j][fl] = x[j][fl];
  }
  int bm0[NNLS_SLOTS], bm1[NNLS_SLOTS];
  float bw0[NNLS_SLOTS], bw1[NNLS_SLOTS];
#pragma unroll
  for (int j = 0; j < NNLS_SLOTS; ++j) {
    const int b = min(tid + 256 * j, NBIN - 1);
    bm0[j] = c.bin_mel[2 * b]; bm1[j] = c.bin_mel[2 * b + 1];
    bw0[j] = c.bin_w[2 * b]; bw1[j] = c.bin_w[2 * b + 1];
  }
  const float step = c.step;
  double t = 1.0;
  for (int it = 0; it < iters; ++it) {
    __syncthreads();                                 // y complete
    for (int o = tid; o < NNLS_G * NMEL; o += 256) { // r = W y - b, band-sparse
      const int fl = o / NMEL, m = o % NMEL;
      const int lo = c.mel_lo[m], len = c.mel_len[m];
      const float* w = c.mel_w + c.mel_off[m];
      float s = 0.0f;
      for (int j = 0; j < len; ++j) s = fmaf(w[j], y[fl][lo + j], s);
      rv[fl][m] = s - bv[fl][m];
    }
    __syncthreads();                                 // r complete; y is read only from registers below
    const double t1 = 0.5 * (1.0 + sqrt(1.0 + 4.0 * t * t));
    const float mom = (float)((t - 1.0) / t1);
    t = t1;
#pragma unroll
    for (int j = 0; j < NNLS_SLOTS; ++j) {
      const int b = tid + 256 * j;
      if (b >= NBIN) continue;
#pragma unroll
      for (int fl = 0; fl < NNLS_G; ++fl) {
        const float gr = fmaf(bw1[j], rv[fl][bm1[j]], bw0[j] * rv[fl][bm0[j]]);   // (W^T r)_b: <= 2 filters per bin
        const float z = fmaxf(fmaf(-step, gr, yr[j][fl]), 0.0f);
        const float yn = fmaf(mom, z - x[j][fl], z);
        x[j][fl] = z;
        yr[j][fl] = yn;
        y[fl][b] = yn;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NNLS_SLOTS; ++j) {
    const int b = tid + 256 * j;
    if (b >= NBIN) continue;
#pragma unroll
    for (int fl = 0; fl < NNLS_G; ++fl) {
      const int g = g0 + fl;
      if (g < total) out[((size_t)(g / F) * NBIN + b) * F + g % F] = x[j][fl];
    }
  }
}

// ---- spectrum sources of k_istft: the complex bin Y of signal sn at o = b F + frame of its [1025][F] plane, before the irfft weights.
// MaskSource: power [S][N][1025][F] with the mixture STFT [N][1025][F] (signal sn = s N + n) -- reuse the mixture's phase, or the
// single-channel Wiener filter (melspec_inversion_basis.py:42-93).
struct MaskSource {
  const float* power;
  int S;
  const float2* xm;
  int N, wiener;
  __device__ __forceinline__ float2 bin(int sn, size_t plane, size_t o) const {
    const int n = sn % N;
    const float2 X = xm[(size_t)n * plane + o];
    const float x = power[(size_t)sn * plane + o];
    float yr = 0.0f, yi = 0.0f;
    if (wiener) {                                    // single_channel_wiener_filter: x_i / (sum_j x_j + 1e-10) X
      float tot = 0.0f;
      for (int s = 0; s < S; ++s) tot += power[(size_t)(s * N + n) * plane + o];
      const float g = x / (tot + 1e-10f);
      yr = g * X.x; yi = g * X.y;
    } else {                                         // sqrt(x) e^{i angle(X)}, angle(0) = 0
      const float mag = sqrtf(X.x * X.x + X.y * X.y), sx = sqrtf(x);
      if (mag > 0.0f) { yr = sx * (X.x / mag); yi = sx * (X.y / mag); }
      else yr = sx;
    }
    return make_float2(yr, yi);
  }
};

// GriffinSource: magnitudes mag [N][1025][F] and librosa.griffinlim's phase.  Iteration 0 (R == null): mag init (init == null: ones).
// After it: a = R - beta P from the latest rebuilt spectrum R and the one before it P (P == null: the first update, tprev = 0),
// Y = mag a / (|a| + 1e-16) -- a zero stays zero.  R and P are complex [N][1025][F].
struct GriffinSource {
  const float* mag;
  const float2* init;
  const float2* R;
  const float2* P;
  float beta;                                        // momentum / (1 + momentum)
  __device__ __forceinline__ float2 bin(int sn, size_t plane, size_t o) const {
    const size_t e = (size_t)sn * plane + o;
    const float s = mag[e];
    if (!R) {
      if (!init) return make_float2(s, 0.0f);
      const float2 a = init[e];
      return make_float2(s * a.x, s * a.y);
    }
    float2 a = R[e];
    if (P) {
      const float2 p = P[e];
      a.x = fmaf(-beta, p.x, a.x);
      a.y = fmaf(-beta, p.y, a.y);
    }
    const float r = 1.0f / (sqrtf(a.x * a.x + a.y * a.y) + 1e-16f);
    return make_float2(s * (a.x * r), s * (a.y * r));
  }
};

// ---- iSTFT of the spectra a Source gives.  Output hop block h (padded samples [512 h, 512 h + 512)) gathers frames h - q, q = 0..3,
// at offset 512 q:
//   out[h][u] = sum_q hann[512 q + u] C_q[h][u],   C_q[h][u] = frame_{h-q}[512 q + u] = sum_b Y_{h-q}[b] basis[b][512 q + u]
// so each q is a GEMM with its own accumulator (spectra rows shifted by q), summed in the order q = 0, 1, 2, 3 in the epilogue.
// One wave = 32 hop blocks x 32 samples; 4 waves = 128 samples; the spectra of the 35 frames a tile touches are staged in LDS,
// built by the Source and scaled as they are loaded, 41 bins at a time (1025 = 25 x 41).  One block row per signal and hop tile:
// grid (signals x htiles, 4).  Indices into the spectra and the audio are size_t; F < 2^22 keeps the int hop-block index exact.
constexpr int IS_BC = 41, IS_ROWS = 35, IS_PITCH = 2 * IS_BC + 1;

template <class Source>
__global__ __launch_bounds__(256) void k_istft(Source src, int F, int htiles, AudioConsts c, float* __restrict__ audio) {
  __shared__ float tab[NFFT];
  __shared__ float sp[IS_ROWS * IS_PITCH];           // [frame - fbase][2 (b - b0) + re/im]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, i = lane & 31;
  const int sn = blockIdx.x / htiles, ht = blockIdx.x % htiles;
  const int u0 = blockIdx.y * 128 + wave * 32;
  const int fbase = ht * 32 - 1;                     // hop block h = 2 + 32 ht + i needs frames h - 3 .. h
  const size_t plane = (size_t)NBIN * F;
  for (int k = tid; k < NFFT; k += 256) tab[k] = c.tab[k];
  f32x16 acc[4] = {{}, {}, {}, {}};
  for (int b0 = 0; b0 < NBIN; b0 += IS_BC) {
    __syncthreads();
    for (int k = tid; k < IS_BC * IS_ROWS; k += 256) {
      const int bl = k / IS_ROWS, ri = k % IS_ROWS, b = b0 + bl, fr = fbase + ri;
      float yr = 0.0f, yi = 0.0f;
      if (fr >= 0 && fr < F) {
        const float2 y = src.bin(sn, plane, (size_t)b * F + fr);
        yr = y.x; yi = y.y;
        const bool edge = b == 0 || b == NBIN - 1;   // irfft: DC and Nyquist once and real, the other bins twice
        yr *= edge ? (1.0f / NFFT) : (2.0f / NFFT);
        yi = edge ? 0.0f : yi * (2.0f / NFFT);
      }
      sp[ri * IS_PITCH + 2 * bl] = yr;
      sp[ri * IS_PITCH + 2 * bl + 1] = yi;
    }
    __syncthreads();
    const int nb = min(IS_BC, NBIN - b0);
    for (int bl = 0; bl < nb; ++bl) {
      const int b = b0 + bl;
#pragma unroll
      for (int q = 0; q < 4; ++q) {                  // A[i][k]: frame 2 + 32 ht + i - q, k = (bin, re/im); B[k][j]: Re -> cos, Im -> -sin
        const float av = sp[(i + 3 - q) * IS_PITCH + 2 * bl + half];
        const int t = 512 * q + u0 + i;
        const float bvv = tab[(b * t + 512 * half) & (NFFT - 1)];
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bvv, acc[q], 0, 0, 0);
      }
    }
  }
  const int u = u0 + i;                              // C/D: column = lane & 31 (sample), row = (r & 3) + 8 (r >> 2) + 4 half (hop block)
  const size_t len = (size_t)(F - 1) * HOP;
  float* out = audio + (size_t)sn * len;
  const float tiny = 1.17549435e-38f;                // np.finfo(float32).tiny (librosa.istft)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int h = 2 + 32 * ht + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (h > F) continue;
    float v = 0.0f, wss = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int fr = h - q;
      if (fr < 0 || fr >= F) continue;
      const float w = c.win[512 * q + u];
      v = fmaf(w, acc[q][r], v);
      wss = fmaf(w, w, wss);
    }
    out[(size_t)(h - 2) * HOP + u] = wss > tiny ? v / wss : v;
  }
}

}  // namespace glowk_audio
