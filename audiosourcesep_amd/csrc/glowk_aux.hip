// glowk handle-free entry points: the BASIS update kernel and mixture, the Philox device RNG, CRC-32C (run_basis_sep.py:131-181, tile_io / tf_checkpoint),
// the audio front end and mel inversion (glowk_audio.h), the BSS Eval v4 metrics (glowk_bsseval.h), the oracle separation
// systems (glowk_oracle.h), the sample-rate converter (glowk_resample.h), the stereo EM Wiener filter (glowk_stereo.h),
// whole-signal mel frames and overlapping tiles (glowk_longform.h), BASIS as one chain over a whole signal's frames (glowk_frames.h),
// harmonic / percussive separation by median filtering (glowk_hpss.h), REPET-SIM's nearest-neighbour filter (glowk_repet.h),
// REPET's beat spectrum, period and periodic neighbours (glowk_beat.h)
// the 2DFT separation: the 2-D DFT GEMMs, the plane's std and the peak mask (glowk_dft2.h)
// DUET: the attenuation-delay histogram, its peaks and the assignment of a two-channel STFT (glowk_duet.h)
// NMF: fused multiplicative updates, the beta divergence and masks of component ranges (glowk_nmf.h)
// AuxIVA and ILRMA: frame norms, weighted covariances with the iterative projection, demixing and images (glowk_iva.h)
// convolutive NMF: NMF on K Tw stacked components whose activations are tied shifts of each other (glowk_nmfd.h)
// WPE dereverberation: the inverse power, the weighted correlations of the stacked past, the Cholesky solve and the filter (glowk_wpe.h)
#include "glowk_engine.h"
#include "glowk_basis.h"
#include "glowk_audio.h"
#include "glowk_bsseval.h"
#include "glowk_oracle.h"
#include "glowk_resample.h"
#include "glowk_stereo.h"
#include "glowk_longform.h"
#include "glowk_frames.h"
#include "glowk_hpss.h"
#include "glowk_repet.h"
#include "glowk_beat.h"
#include "glowk_dft2.h"
#include "glowk_duet.h"
#include "glowk_nmf.h"
#include "glowk_iva.h"
#include "glowk_melody.h"
#include "glowk_rpca.h"
#include "glowk_projet.h"
#include "glowk_cluster.h"
#include "glowk_kam.h"
#include "glowk_nmfd.h"
#include "glowk_wpe.h"

#include <initializer_list>
#include <mutex>

using namespace glowk_eng;

namespace glowk_eng {
// elements [offset, offset + n) of an RNG stream reach past element 2^62: from there hi32(q) of the quad q = e / 4 runs into
// the bits of the counter word that hold `which`, and the draws would be another stream's
static bool rng_range_bad(uint64_t offset, size_t n) {
  const uint64_t lim = (uint64_t)1 << 62;
  return offset > lim || n > lim - offset;
}
}  // namespace glowk_eng

extern "C" {

int glowk_random(float* out_dev, size_t n, uint64_t seed, uint64_t step, int which, int uniform, uint64_t offset, void* stream) {
  if (!out_dev) return fail("null tensor");
  if (which < 0 || which > 15) return fail("random: stream id must be 0..15");
  if (offset % 4) return fail("random: the stream offset must be a multiple of 4 elements");
  if (rng_range_bad(offset, n)) return fail("random: the stream ends at element 2^62 (offset + n is beyond it)");
  if (n == 0) return 0;
  DeviceGuard dg(ptr_device(out_dev));
  const size_t threads = (n + 3) / 4;
  hipLaunchKernelGGL(k_basis_noise, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out_dev, n, seed, step,
                     (uint32_t)which, uniform, offset / 4, 0u);
  LAUNCHCHK("k_basis_noise");
  return 0;
}

int glowk_random_source(float* out_dev, size_t n, uint64_t seed, uint64_t step, int which, int pair, int uniform, uint64_t offset,
                        void* stream) {
  if (!out_dev) return fail("null tensor");
  if (which < 0 || which > 15) return fail("random_source: stream id must be 0..15");
  if (pair < 0 || pair > 65535) return fail("random_source: the source pair must be 0..65535");
  if (pair && step >= ((uint64_t)1 << 48)) return fail("random_source: step must be below 2^48 (a source pair shares its counter word)");
  if (offset % 4) return fail("random_source: the stream offset must be a multiple of 4 elements");
  if (rng_range_bad(offset, n)) return fail("random_source: the stream ends at element 2^62 (offset + n is beyond it)");
  if (n == 0) return 0;
  DeviceGuard dg(ptr_device(out_dev));
  const size_t threads = (n + 3) / 4;
  hipLaunchKernelGGL(k_basis_noise, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out_dev, n, seed, step,
                     (uint32_t)which, uniform, offset / 4, (uint32_t)pair);
  LAUNCHCHK("k_basis_noise");
  return 0;
}

namespace glowk_eng {
// [a, a + n) and [b, b + n) floats share an element
static bool basis_overlap(const float* a, const float* b, size_t n) {
  const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
  return (p > q ? p - q : q - p) < n * sizeof(float);
}

#define GLOWK_BASIS_EACH_S(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
}  // namespace glowk_eng

int glowk_basis_update_n(float* const* x, const float* const* g, const float* const* eps, int nsrc, const float* mixed_dev, size_t n,
                         int mixing, float eta, float lambda_recon, uint64_t seed, uint64_t step, uint64_t offset,
                         int* nonfinite_dev, void* stream) {
  if (nsrc < 2 || nsrc > GLOWK_BASIS_MAX_SOURCES) return fail("basis_update_n: the number of sources must be 2..16");
  if (mixing != GLOWK_MIX_DB && mixing != GLOWK_MIX_MEAN) return fail("basis_update_n: unknown mixing process");
  if (!x || !g || !mixed_dev) return fail("null tensor");
  for (int k = 0; k < nsrc; ++k)
    if (!x[k] || !g[k]) return fail("null tensor");
  if (offset % 4) return fail("basis_update_n: the stream offset must be a multiple of 4 elements");
  if (rng_range_bad(offset, n)) return fail("basis_update_n: the stream ends at element 2^62 (offset + n is beyond it)");
  if (step >= ((uint64_t)1 << 48)) return fail("basis_update_n: step must be below 2^48 (the source pair shares its counter word)");
  if (n > ((size_t)1 << 40)) return fail("basis_update_n: too many elements");
  if (!(eta >= 0.0f)) return fail("basis_update_n: eta must be non-negative");
  for (int k = 0; k < nsrc; ++k) {
    if (basis_overlap(x[k], mixed_dev, n ? n : 1)) return fail("basis_update_n: a source state aliases the mixture");
    for (int l = 0; l < k; ++l)
      if (basis_overlap(x[k], x[l], n ? n : 1)) return fail("basis_update_n: the source states must be distinct buffers");
  }
  if (n == 0) return 0;
  DeviceGuard dg(ptr_device(x[0]));
  BasisNArgs a;
  uintptr_t bits = (uintptr_t)mixed_dev;
  for (int k = 0; k < nsrc; ++k) {
    a.x[k] = x[k]; a.g[k] = g[k]; a.eps[k] = eps ? eps[k] : nullptr;
    bits |= (uintptr_t)a.x[k] | (uintptr_t)a.g[k] | (uintptr_t)a.eps[k];
  }
  a.mixed = mixed_dev; a.n = n; a.eta = eta; a.lambda_recon = lambda_recon; a.noise_scale = std::sqrt(2.0f * eta);
  a.ln_s = (float)std::log((double)nsrc); a.inv_s = 1.0f / (float)nsrc; a.mixing = mixing; a.vec = (bits & 15) == 0;
  a.seed = seed; a.step = step; a.q0 = offset / 4; a.nonfinite = nonfinite_dev;
  const dim3 grid((unsigned)(((n + 3) / 4 + 255) / 256));
  switch (nsrc) {
#define GLOWK_CASE(s) case s: hipLaunchKernelGGL(k_basis_update_n<s>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    GLOWK_BASIS_EACH_S(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_basis_update_n");
  return 0;
}

int glowk_basis_mix_n(const float* const* x, int nsrc, float* out_dev, size_t n, int mixing, void* stream) {
  if (nsrc < 2 || nsrc > GLOWK_BASIS_MAX_SOURCES) return fail("basis_mix_n: the number of sources must be 2..16");
  if (mixing != GLOWK_MIX_DB && mixing != GLOWK_MIX_MEAN) return fail("basis_mix_n: unknown mixing process");
  if (!x || !out_dev) return fail("null tensor");
  for (int k = 0; k < nsrc; ++k)
    if (!x[k]) return fail("null tensor");
  if (n == 0) return 0;
  DeviceGuard dg(ptr_device(out_dev));
  BasisMixNArgs a;
  for (int k = 0; k < nsrc; ++k) a.x[k] = x[k];
  a.out = out_dev; a.n = n; a.ln_s = (float)std::log((double)nsrc); a.inv_s = 1.0f / (float)nsrc; a.mixing = mixing;
  const dim3 grid((unsigned)((n + 255) / 256));
  switch (nsrc) {
#define GLOWK_CASE(s) case s: hipLaunchKernelGGL(k_basis_mix_n<s>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    GLOWK_BASIS_EACH_S(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_basis_mix_n");
  return 0;
}

// the two-source entry points: the S = 2 instance with dB mixing, checked and launched by the calls above
int glowk_basis_update(float* x1_dev, float* x2_dev, const float* g1_dev, const float* g2_dev, const float* mixed_dev, size_t n,
                       float eta, float lambda_recon, const float* eps1_dev, const float* eps2_dev, uint64_t seed, uint64_t step,
                       uint64_t offset, int* nonfinite_dev, void* stream) {
  float* const x[2] = {x1_dev, x2_dev};
  const float* const g[2] = {g1_dev, g2_dev};
  const float* const eps[2] = {eps1_dev, eps2_dev};
  return glowk_basis_update_n(x, g, eps, 2, mixed_dev, n, GLOWK_MIX_DB, eta, lambda_recon, seed, step, offset, nonfinite_dev, stream);
}

int glowk_basis_mix(const float* x1_dev, const float* x2_dev, float* out_dev, size_t n, void* stream) {
  const float* const x[2] = {x1_dev, x2_dev};
  return glowk_basis_mix_n(x, 2, out_dev, n, GLOWK_MIX_DB, stream);
}

int glowk_add_noise(const float* x_dev, float* out_dev, size_t n, float sigma, uint64_t seed, uint64_t step, int which, uint64_t offset,
                    void* stream) {
  if (!x_dev || !out_dev) return fail("null tensor");
  if (which < 0 || which > 15) return fail("add_noise: stream id must be 0..15");
  if (offset % 4) return fail("add_noise: the stream offset must be a multiple of 4 elements");
  if (rng_range_bad(offset, n)) return fail("add_noise: the stream ends at element 2^62 (offset + n is beyond it)");
  if (n == 0) return 0;
  DeviceGuard dg(ptr_device(out_dev));
  const size_t threads = (n + 3) / 4;
  hipLaunchKernelGGL(k_add_noise, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_dev, out_dev, n, sigma, seed,
                     step, (uint32_t)which, offset / 4);
  LAUNCHCHK("k_add_noise");
  return 0;
}

// ---- the split kernels' activation + hi/lo split, eight values per thread through the very helpers the network kernels inline
namespace glowk_eng {
// mode 0: ReLU, scale, split (h3s_act<NET_FWD>); 1: the two-term mode (NET_FWD2: hi only); 2: scale and split alone (the gather prologues)
__global__ __launch_bounds__(256) void k_split_probe(const float* __restrict__ x, int n, float sc, int mode, unsigned short* __restrict__ hi,
                                                     unsigned short* __restrict__ lo) {
  const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 8;
  if (i0 >= n) return;
  f32x4 r0, r1;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = i0 + j < n ? x[i0 + j] : 0.0f;
    if (j < 4) r0[j] = v[j]; else r1[j - 4] = v[j];
  }
  h8 bh, bl;
  if (mode == 0) h3s_act<NET_FWD, false, true>(r0, r1, sc, 0u, bh, bl);
  else if (mode == 1) h3s_act<NET_FWD2, false, true>(r0, r1, sc, 0u, bh, bl);
  else split8(v, sc, bh, bl);
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (i0 + j < n) {
      hi[i0 + j] = __builtin_bit_cast(unsigned short, (_Float16)bh[j]);
      lo[i0 + j] = __builtin_bit_cast(unsigned short, (_Float16)bl[j]);
    }
}
}  // namespace glowk_eng

int glowk_split_probe(const float* x_dev, int n, float sc, int mode, uint16_t* hi_dev, uint16_t* lo_dev, void* stream) {
  if (!x_dev || !hi_dev || !lo_dev) return fail("null tensor");
  if (n < 0 || n > (1 << 30)) return fail("split_probe: n must be 0..2^30");
  if (mode < 0 || mode > 2) return fail("split_probe: mode must be 0 (ReLU), 1 (two-term) or 2 (no activation)");
  if (!split_scale_ok(sc)) return fail("split_probe: the scale must be a power of two (the kernels' contract, NetArgs::sc1)");
  if (n == 0) return 0;
  DeviceGuard dg(ptr_device(hi_dev));
  hipLaunchKernelGGL(k_split_probe, dim3((unsigned)((n + 2047) / 2048)), dim3(256), 0, (hipStream_t)stream, x_dev, n, sc, mode, hi_dev, lo_dev);
  LAUNCHCHK("k_split_probe");
  return 0;
}

namespace glowk_eng {
struct Crc32cTable {
  uint32_t t[8][256];
  Crc32cTable() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xFF];
  }
};
}  // namespace glowk_eng

uint32_t glowk_crc32c(const void* host_data, size_t n) {
  static const Crc32cTable tbl;            // function-local static: initialised once, thread-safe by the language (C++11 [stmt.dcl])
  const uint32_t (&table)[8][256] = tbl.t;
  const unsigned char* p = static_cast<const unsigned char*>(host_data);
  uint32_t c = 0xFFFFFFFFu;
  while (n >= 8) {                         // slicing-by-8
    uint32_t lo, hi;
    std::memcpy(&lo, p, 4);
    std::memcpy(&hi, p + 4, 4);
    lo ^= c;
    c = table[7][lo & 0xFF] ^ table[6][(lo >> 8) & 0xFF] ^ table[5][(lo >> 16) & 0xFF] ^ table[4][lo >> 24] ^
        table[3][hi & 0xFF] ^ table[2][(hi >> 8) & 0xFF] ^ table[1][(hi >> 16) & 0xFF] ^ table[0][hi >> 24];
    p += 8; n -= 8;
  }
  while (n--) c = table[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}


// ---- audio: device constants (glowk_audio.h AudioConsts), built once on the host in fp64, uploaded once per device --------------
namespace glowk_eng {
struct AudioHost {
  std::vector<float> tab, win, mel_w, bin_w, pinv, dense;   // dense: W [96][1025] (glowk_mel_filterbank)
  std::vector<int> mel_lo, mel_len, mel_off, bin_mel;
  float step = 0.0f;
  std::string err;
  AudioHost();
};

// Slaney mel scale (librosa hz_to_mel / mel_to_hz, htk=False): linear below 1 kHz (200/3 Hz per mel), logarithmic above
static double hz_to_mel(double f) {
  const double logstep = std::log(6.4) / 27.0;
  return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) / logstep : f / (200.0 / 3.0);
}
static double mel_to_hz(double m) {
  const double logstep = std::log(6.4) / 27.0;
  return m >= 15.0 ? 1000.0 * std::exp(logstep * (m - 15.0)) : (200.0 / 3.0) * m;
}

AudioHost::AudioHost() {
  using namespace glowk_audio;
  const double pi = 3.14159265358979323846;
  tab.resize(NFFT);
  win.resize(NFFT);
  for (int m = 0; m < NFFT; ++m) {             // exact at the quarter turns, so DC / Nyquist columns carry no stray sine
    tab[m] = (m % 512 == 0) ? (float)(m == 0 ? 1 : m == 1024 ? -1 : 0) : (float)std::cos(2.0 * pi * m / NFFT);
    win[m] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * m / NFFT));   // scipy.signal.get_window('hann', 2048, fftbins=True)
  }
  // librosa.filters.mel(sr=16000, n_fft=2048, n_mels=96, fmin=125, fmax=7600), Slaney area normalisation
  const double mmin = hz_to_mel(125.0), mmax = hz_to_mel(7600.0);
  std::vector<double> mel_f(NMEL + 2);
  for (int i = 0; i < NMEL + 2; ++i) mel_f[i] = mel_to_hz(i == NMEL + 1 ? mmax : mmin + i * ((mmax - mmin) / (NMEL + 1)));
  std::vector<double> W((size_t)NMEL * NBIN);
  for (int i = 0; i < NMEL; ++i) {
    const double d0 = mel_f[i + 1] - mel_f[i], d1 = mel_f[i + 2] - mel_f[i + 1], enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
    for (int k = 0; k < NBIN; ++k) {
      const double f = k * (16000.0 / NFFT);
      const double lower = -(mel_f[i] - f) / d0, upper = (mel_f[i + 2] - f) / d1;
      W[(size_t)i * NBIN + k] = (double)(float)(std::max(0.0, std::min(lower, upper)) * enorm);
    }
  }
  dense.assign(W.begin(), W.end());
  mel_lo.resize(NMEL); mel_len.resize(NMEL); mel_off.resize(NMEL);
  bin_mel.assign(2 * NBIN, 0); bin_w.assign(2 * NBIN, 0.0f);
  std::vector<int> cover(NBIN, 0);
  for (int i = 0; i < NMEL; ++i) {
    int lo = -1, hi = -1;
    for (int k = 0; k < NBIN; ++k)
      if (W[(size_t)i * NBIN + k] != 0.0) { if (lo < 0) lo = k; hi = k; }
    if (lo < 0) { err = "mel filterbank: an empty filter"; return; }
    mel_lo[i] = lo; mel_len[i] = hi - lo + 1; mel_off[i] = (int)mel_w.size();
    for (int k = lo; k <= hi; ++k) {
      const float w = (float)W[(size_t)i * NBIN + k];
      mel_w.push_back(w);
      if (w == 0.0f) continue;
      if (cover[k] == 2) { err = "mel filterbank: a bin in more than two filters"; return; }
      bin_mel[2 * k + cover[k]] = i;
      bin_w[2 * k + cover[k]] = w;
      ++cover[k];
    }
  }
  // G = W W^T (SPD, 96 x 96): step = 1 / lambda_max(G) by power iteration, W+ = W^T G^-1 by Cholesky
  std::vector<double> G((size_t)NMEL * NMEL, 0.0);
  for (int i = 0; i < NMEL; ++i)
    for (int j = 0; j < NMEL; ++j) {
      double s = 0.0;
      for (int k = 0; k < NBIN; ++k) s += W[(size_t)i * NBIN + k] * W[(size_t)j * NBIN + k];
      G[(size_t)i * NMEL + j] = s;
    }
  std::vector<double> v(NMEL, 1.0), u(NMEL);
  double lam = 0.0;
  for (int it = 0; it < 5000; ++it) {
    double nrm = 0.0;
    for (int i = 0; i < NMEL; ++i) {
      double s = 0.0;
      for (int j = 0; j < NMEL; ++j) s += G[(size_t)i * NMEL + j] * v[j];
      u[i] = s;
      nrm += s * s;
    }
    nrm = std::sqrt(nrm);
    lam = nrm;
    for (int i = 0; i < NMEL; ++i) v[i] = u[i] / nrm;
  }
  step = (float)(1.0 / lam);
  std::vector<double> Lc((size_t)NMEL * NMEL, 0.0);
  for (int j = 0; j < NMEL; ++j) {
    double d = G[(size_t)j * NMEL + j];
    for (int k = 0; k < j; ++k) d -= Lc[(size_t)j * NMEL + k] * Lc[(size_t)j * NMEL + k];
    if (!(d > 0.0)) { err = "mel filterbank: W W^T is not positive definite"; return; }
    Lc[(size_t)j * NMEL + j] = std::sqrt(d);
    for (int i = j + 1; i < NMEL; ++i) {
      double s = G[(size_t)i * NMEL + j];
      for (int k = 0; k < j; ++k) s -= Lc[(size_t)i * NMEL + k] * Lc[(size_t)j * NMEL + k];
      Lc[(size_t)i * NMEL + j] = s / Lc[(size_t)j * NMEL + j];
    }
  }
  pinv.assign((size_t)NBIN * NMEL, 0.0f);
  std::vector<double> z(NMEL);
  for (int k = 0; k < NBIN; ++k) {              // row k of W+ = G^-1 w_k (G symmetric), w_k = column k of W
    if (!cover[k]) continue;                    // exactly zero outside every filter
    for (int i = 0; i < NMEL; ++i) {
      double s = W[(size_t)i * NBIN + k];
      for (int j = 0; j < i; ++j) s -= Lc[(size_t)i * NMEL + j] * z[j];
      z[i] = s / Lc[(size_t)i * NMEL + i];
    }
    for (int i = NMEL - 1; i >= 0; --i) {
      double s = z[i];
      for (int j = i + 1; j < NMEL; ++j) s -= Lc[(size_t)j * NMEL + i] * z[j];
      z[i] = s / Lc[(size_t)i * NMEL + i];
    }
    for (int i = 0; i < NMEL; ++i) pinv[(size_t)k * NMEL + i] = (float)z[i];
  }
}

static const AudioHost& audio_host() {
  static const AudioHost host;                 // function-local static: built once, thread-safe by the language
  return host;
}

// the device every pointer lives on; a host, unregistered or foreign-device pointer is refused (the kernels would fault on it)
static int audio_device(std::initializer_list<const void*> ptrs, int* dev, const char* what = "audio") {
  *dev = -1;
  for (const void* p : ptrs) {
    if (!p) continue;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess || !(a.type == hipMemoryTypeDevice || a.isManaged) || a.device < 0) {
      (void)hipGetLastError();
      return fail(std::string(what) + ": every tensor must be device memory");
    }
    if (*dev >= 0 && a.device != *dev) return fail(std::string(what) + ": the tensors are on different devices");
    *dev = a.device;
  }
  return 0;
}

// one upload per device, kept for the life of the process (allocated under the caller's DeviceGuard)
static int audio_consts(int dev, glowk_audio::AudioConsts* out) {
  const AudioHost& host = audio_host();
  static std::mutex mu;
  static std::vector<std::pair<int, glowk_audio::AudioConsts>> cache;
  if (!host.err.empty()) return fail(host.err);
  std::lock_guard<std::mutex> lock(mu);
  for (auto& e : cache)
    if (e.first == dev) { *out = e.second; return 0; }
  const size_t nf = host.tab.size() + host.win.size() + host.mel_w.size() + host.bin_w.size() + host.pinv.size();
  const size_t ni = host.mel_lo.size() + host.mel_len.size() + host.mel_off.size() + host.bin_mel.size();
  DeviceMem<char> base;
  HIPCHK(dev_alloc(base, (nf + ni) * 4));
  std::vector<char> img((nf + ni) * 4);
  size_t pos = 0;
  auto put = [&](const void* src, size_t n) { std::memcpy(img.data() + pos, src, n * 4); const char* p = base + pos; pos += n * 4; return p; };
  glowk_audio::AudioConsts c;
  c.tab = (const float*)put(host.tab.data(), host.tab.size());
  c.win = (const float*)put(host.win.data(), host.win.size());
  c.mel_w = (const float*)put(host.mel_w.data(), host.mel_w.size());
  c.bin_w = (const float*)put(host.bin_w.data(), host.bin_w.size());
  c.pinv = (const float*)put(host.pinv.data(), host.pinv.size());
  c.mel_lo = (const int*)put(host.mel_lo.data(), host.mel_lo.size());
  c.mel_len = (const int*)put(host.mel_len.data(), host.mel_len.size());
  c.mel_off = (const int*)put(host.mel_off.data(), host.mel_off.size());
  c.bin_mel = (const int*)put(host.bin_mel.data(), host.bin_mel.size());
  c.step = host.step;
  HIPCHK(hipMemcpy(base, img.data(), img.size(), hipMemcpyHostToDevice));
  base.release();              // the cache keeps the raw pointers: no static destructor frees device memory at process exit
  cache.emplace_back(dev, c);
  *out = c;
  return 0;
}
}  // namespace glowk_eng

int glowk_mel_filterbank(float* host_out) {
  if (!host_out) return fail("null buffer");
  const AudioHost& host = audio_host();
  if (!host.err.empty()) return fail(host.err);
  std::memcpy(host_out, host.dense.data(), host.dense.size() * sizeof(float));
  return 0;
}

int glowk_mel_frontend(const float* audio_dev, int N, int n_samples, float top_db, float* mel_db_dev, float* stft_dev, void* stream) {
  using namespace glowk_audio;
  if (!audio_dev || !mel_db_dev) return fail("null tensor");
  if (N < 0 || N > (1 << 20)) return fail("mel_frontend: N must be in [0, 2^20]");
  if (n_samples <= PAD || n_samples >= MAX_FRAMES * HOP)
    return fail("mel_frontend: n_samples must be in (1024, 65536): reflect padding needs more than 1024 samples, the tile at most 128 frames");
  if (!(std::fabs(top_db) < 1e30f)) return fail("mel_frontend: top_db must be finite");
  if (N == 0) return 0;
  int dev;
  if (int rc = audio_device({audio_dev, mel_db_dev, stft_dev}, &dev)) return rc;
  DeviceGuard dg(dev);
  AudioConsts c;
  if (int rc = audio_consts(dev, &c)) return rc;
  const int F = 1 + n_samples / HOP, ftiles = (F + 31) / 32;
  hipStream_t s = (hipStream_t)stream;
  Scratch<float> power(HipFreeAsync{s});       // |X|^2 scratch, only when the caller does not take the complex STFT (k_mel_db squares X)
  if (!stft_dev) HIPCHK(scratch_alloc(power, (size_t)N * NBIN * F * sizeof(float)));
  hipLaunchKernelGGL(k_stft, dim3((unsigned)(N * ftiles), (NBIN + 127) / 128), dim3(256), 0, s, audio_dev, n_samples, F, ftiles, c, power, stft_dev);
  LAUNCHCHK("k_stft");
  hipLaunchKernelGGL(k_mel_db, dim3((unsigned)N), dim3(256), NMEL * F * sizeof(float), s, (const float*)power,
                     (const float2*)stft_dev, F, top_db, c, mel_db_dev);
  LAUNCHCHK("k_mel_db");
  return 0;
}

int glowk_mel_to_power(const float* mel_db_dev, int N, int frames, int iters, float* power_dev, void* stream) {
  using namespace glowk_audio;
  if (!mel_db_dev || !power_dev) return fail("null tensor");
  if (N < 0 || N > (1 << 20)) return fail("mel_to_power: N must be in [0, 2^20]");
  if (frames < 1 || frames > MAX_FRAMES) return fail("mel_to_power: frames must be in [1, 128]");
  if (iters < 0 || iters > 100000) return fail("mel_to_power: iters must be in [0, 100000]");
  if (N == 0) return 0;
  int dev;
  if (int rc = audio_device({mel_db_dev, power_dev}, &dev)) return rc;
  DeviceGuard dg(dev);
  AudioConsts c;
  if (int rc = audio_consts(dev, &c)) return rc;
  const int total = N * frames;
  hipLaunchKernelGGL(k_nnls, dim3((unsigned)((total + NNLS_G - 1) / NNLS_G)), dim3(256), 0, (hipStream_t)stream, mel_db_dev, frames, total, iters, c,
                     power_dev);
  LAUNCHCHK("k_nnls");
  return 0;
}

int glowk_masked_istft(const float* power_dev, int S, const float* stft_mix_dev, int N, int frames, int wiener, float* audio_dev, void* stream) {
  using namespace glowk_audio;
  if (!power_dev || !stft_mix_dev || !audio_dev) return fail("null tensor");
  if (S < 1 || S > 16) return fail("masked_istft: S must be in [1, 16]");
  if (wiener && S < 2) return fail("masked_istft: the Wiener filter needs S >= 2 sources");
  if (N < 0 || N > (1 << 20)) return fail("masked_istft: N must be in [0, 2^20]");
  if (frames < 2 || frames > MAX_FRAMES) return fail("masked_istft: frames must be in [2, 128]");
  if (N == 0) return 0;
  int dev;
  if (int rc = audio_device({power_dev, stft_mix_dev, audio_dev}, &dev)) return rc;
  DeviceGuard dg(dev);
  AudioConsts c;
  if (int rc = audio_consts(dev, &c)) return rc;
  const int htiles = (frames - 1 + 31) / 32;
  const MaskSource src{power_dev, S, reinterpret_cast<const float2*>(stft_mix_dev), N, wiener ? 1 : 0};
  hipLaunchKernelGGL(k_istft<MaskSource>, dim3((unsigned)(S * N * htiles), HOP / 128), dim3(256), 0, (hipStream_t)stream, src, frames, htiles, c,
                     audio_dev);
  LAUNCHCHK("k_istft");
  return 0;
}

// Griffin-Lim: iteration 0 is one iSTFT of mag init; each of the n_iter iterations is k_stft of the latest signal into one of two
// complex spectra, then k_istft with the phase update folded into its staging (GriffinSource).  The STFT of iteration k overwrites
// the spectrum iteration k - 1's iSTFT consumed as P.  The signal between the two launches lives in audio_dev.
int glowk_griffinlim(const float* mag_dev, const float* angles0_dev, int N, int frames, int n_iter, float momentum, float* audio_dev,
                     void* stream) {
  using namespace glowk_audio;
  if (!mag_dev || !audio_dev) return fail("null tensor");
  if (N < 0 || N > (1 << 20)) return fail("griffinlim: N must be in [0, 2^20]");
  if (frames < 4 || frames > GL_MAX_FRAMES)
    return fail("griffinlim: frames must be in [4, 2^20]: the STFT's reflect padding needs (frames - 1) * 512 > 1024 samples");
  if (n_iter < 0 || n_iter > 100000) return fail("griffinlim: n_iter must be in [0, 100000]");
  if (!(momentum >= 0.0f && momentum < INFINITY)) return fail("griffinlim: momentum must be finite and >= 0");
  const int ftiles = (frames + 31) / 32, htiles = (frames - 1 + 31) / 32;
  if ((int64_t)N * ftiles > INT32_MAX) return fail("griffinlim: N x frames too large for one launch");
  if (N == 0) return 0;
  int dev;
  if (int rc = audio_device({mag_dev, angles0_dev, audio_dev}, &dev, "griffinlim")) return rc;
  DeviceGuard dg(dev);
  AudioConsts c;
  if (int rc = audio_consts(dev, &c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const dim3 is_grid((unsigned)(N * htiles), HOP / 128), st_grid((unsigned)(N * ftiles), (NBIN + 127) / 128);
  const int n_samples = (frames - 1) * HOP;
  const size_t spec = (size_t)N * NBIN * frames;   // complex elements of one spectrum
  Scratch<float2> R(HipFreeAsync{s});              // two rebuilt spectra, ping-pong
  if (n_iter > 0) HIPCHK(scratch_alloc(R, (n_iter > 1 ? 2 : 1) * spec * sizeof(float2)));
  const float beta = (float)((double)momentum / (1.0 + (double)momentum));
  GriffinSource src{mag_dev, reinterpret_cast<const float2*>(angles0_dev), nullptr, nullptr, beta};
  hipLaunchKernelGGL(k_istft<GriffinSource>, is_grid, dim3(256), 0, s, src, frames, htiles, c, audio_dev);
  LAUNCHCHK("k_istft");
  for (int it = 1; it <= n_iter; ++it) {
    float2* cur = R + (size_t)((it - 1) & 1) * spec;
    hipLaunchKernelGGL(k_stft, st_grid, dim3(256), 0, s, (const float*)audio_dev, n_samples, frames, ftiles, c, (float*)nullptr, (float*)cur);
    LAUNCHCHK("k_stft");
    src.R = cur;
    src.P = it > 1 ? R + (size_t)(it & 1) * spec : nullptr;
    hipLaunchKernelGGL(k_istft<GriffinSource>, is_grid, dim3(256), 0, s, src, frames, htiles, c, audio_dev);
    LAUNCHCHK("k_istft");
  }
  return 0;
}

// ---- sample-rate conversion (glowk_resample.h) ------------------------------------------------------------------------------------
namespace glowk_eng {
// I0 by its power series sum_k ((x / 2)^k / k!)^2: all terms positive, so fp64 keeps ~1e-16 relative at the beta used here
static double bessel_i0(double x) {
  const double h = 0.5 * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= (h / k) * (h / k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

struct ResampleHost {
  std::vector<double> T;            // [Z P + 1]
  std::vector<float2> pairs;        // (T[k], T[k + 1] - T[k]) rounded once; the last difference is 0
  ResampleHost() {
    using namespace glowk_rs;
    const double pi = 3.14159265358979323846, beta = 14.769656459379492, rolloff = 0.9475937167399596;
    const double i0b = bessel_i0(beta);
    T.resize(RS_ZP + 1);
    for (int k = 0; k <= RS_ZP; ++k) {
      const double u = (double)k / RS_ZP, x = pi * rolloff * k / RS_P;
      const double sinc = k == 0 ? 1.0 : std::sin(x) / x;
      T[k] = rolloff * sinc * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0b;
    }
    pairs.resize(RS_ZP + 1);
    for (int k = 0; k <= RS_ZP; ++k) pairs[k] = make_float2((float)T[k], k < RS_ZP ? (float)(T[k + 1] - T[k]) : 0.0f);
  }
};

static const ResampleHost& resample_host() {
  static const ResampleHost host;              // function-local static: built once, thread-safe by the language
  return host;
}

// one upload per device, kept for the life of the process (allocated under the caller's DeviceGuard), like audio_consts
static int resample_table(int dev, const float2** out) {
  const ResampleHost& host = resample_host();
  static std::mutex mu;
  static std::vector<std::pair<int, const float2*>> cache;
  std::lock_guard<std::mutex> lock(mu);
  for (auto& e : cache)
    if (e.first == dev) { *out = e.second; return 0; }
  DeviceMem<float2> tab;
  HIPCHK(dev_alloc(tab, host.pairs.size() * sizeof(float2)));
  HIPCHK(hipMemcpy(tab, host.pairs.data(), host.pairs.size() * sizeof(float2), hipMemcpyHostToDevice));
  *out = tab.release();
  cache.emplace_back(dev, *out);
  return 0;
}

// the arguments glowk_resample takes: rates, ratio and length; a, b = the rates over their gcd
static int resample_check(int64_t n_in, int sr_in, int sr_out, uint32_t* a, uint32_t* b) {
  if (sr_in < 1000 || sr_in > 768000 || sr_out < 1000 || sr_out > 768000) return fail("resample: sr_in and sr_out must be in [1000, 768000]");
  if ((int64_t)sr_out > 64 * (int64_t)sr_in || (int64_t)sr_in > 64 * (int64_t)sr_out) return fail("resample: sr_out / sr_in must be in [1/64, 64]");
  if (n_in < 0 || n_in > ((int64_t)1 << 32)) return fail("resample: n_in must be in [0, 2^32]");
  uint32_t x = (uint32_t)sr_in, y = (uint32_t)sr_out;
  while (y) { const uint32_t z = x % y; x = y; y = z; }
  *a = (uint32_t)sr_in / x;
  *b = (uint32_t)sr_out / x;
  return 0;
}
}  // namespace glowk_eng

int64_t glowk_resample_length(int64_t n_in, int sr_in, int sr_out) {
  uint32_t a, b;
  if (resample_check(n_in, sr_in, sr_out, &a, &b)) return -1;
  return (n_in * (int64_t)b + a - 1) / a;        // n_in b < 2^52
}

int glowk_resample_filter(double* host_out) {
  if (!host_out) return fail("null buffer");
  const ResampleHost& host = resample_host();
  std::memcpy(host_out, host.T.data(), host.T.size() * sizeof(double));
  return 0;
}

int glowk_resample(const float* x_dev, int nsig, int64_t n_in, int sr_in, int sr_out, float* y_dev, void* stream) {
  using namespace glowk_rs;
  uint32_t a, b;
  if (int rc = resample_check(n_in, sr_in, sr_out, &a, &b)) return rc;
  if (nsig < 0 || nsig > (1 << 20)) return fail("resample: nsig must be in [0, 2^20]");
  if (nsig == 0 || n_in == 0) return 0;          // nothing to read or write: an empty tensor has no storage, its pointer may be null
  if (!x_dev || !y_dev) return fail("null tensor");
  ResampleArgs g;
  g.x = x_dev; g.y = y_dev; g.n_in = n_in; g.n_out = (n_in * (int64_t)b + a - 1) / a;
  g.a = a; g.b = b; g.d = std::max(a, b);
  g.stepk = (uint32_t)(((uint64_t)b * RS_P) / g.d); g.stepr = (uint32_t)(((uint64_t)b * RS_P) % g.d);
  g.H = (int)(((int64_t)RS_Z * g.d) / b) + 1;    // <= 4097 at the ratio 1/64
  g.scale = (float)std::min(1.0, (double)b / (double)a); g.inv_d = 1.0f / (float)g.d;
  // the staged span of tb outputs: their centres cover at most floor((tb - 1) a / b) + 1 steps, plus H samples on each side
  auto span = [&](int tb) { return ((int64_t)(tb - 1) * a) / b + 2 * (int64_t)g.H + 2; };
  g.tb = RS_THREADS;
  if (span(g.tb) > RS_LDS_FLOATS) {
    g.tb = (int)(((RS_LDS_FLOATS - 2 * (int64_t)g.H - 2) * b) / a) + 1;
    while (g.tb > 1 && span(g.tb) > RS_LDS_FLOATS) --g.tb;
  }
  g.blocks_per_sig = (g.n_out + g.tb - 1) / g.tb;
  if (g.blocks_per_sig * nsig > (int64_t)INT32_MAX) return fail("resample: too many signals x outputs for one launch");
  int dev;
  if (int rc = audio_device({x_dev, y_dev}, &dev, "resample")) return rc;
  DeviceGuard dg(dev);
  if (int rc = resample_table(dev, &g.tab)) return rc;
  hipLaunchKernelGGL(k_resample, dim3((unsigned)(g.blocks_per_sig * nsig)), dim3(RS_THREADS), (size_t)span(g.tb) * sizeof(float), (hipStream_t)stream, g);
  LAUNCHCHK("k_resample");
  return 0;
}

// ---- BSS Eval v4 (glowk_bsseval.h) ------------------------------------------------------------------------------------------------
namespace {
constexpr size_t BSS_SCRATCH_CAP = (size_t)256 << 20;   // partial sums of one launch group
constexpr size_t BSS_CHOL_CAP = (size_t)2 << 30;        // Cholesky workspaces in flight (8 MB per system at M = 1024)
}

int glowk_bss_xcorr(const double* sig_dev, int nsig, int64_t nsampl, const int64_t* win_dev, int nwin, int64_t max_len, const int* pairs_dev,
                    int npairs, int filters_len, double* corr_dev, void* stream) {
  using namespace glowk_bss;
  if (!sig_dev || !win_dev || !pairs_dev || !corr_dev) return fail("null tensor");
  if (nsig < 1 || nsampl < 1 || nsampl > ((int64_t)1 << 40)) return fail("bss_xcorr: nsig and nsampl must be positive");
  if (filters_len < 1 || filters_len > LMAX) return fail("bss_xcorr: filters_len must be in [1, 512]");
  if (npairs < 1 || npairs > 65535) return fail("bss_xcorr: npairs must be in [1, 65535]");
  if (nwin < 0 || max_len < 0 || max_len > nsampl) return fail("bss_xcorr: nwin >= 0 and max_len in [0, nsampl] required");
  if (nwin == 0) return 0;
  int dev;
  if (int rc = audio_device({sig_dev, win_dev, pairs_dev, corr_dev}, &dev, "bss_xcorr")) return rc;
  DeviceGuard dg(dev);
  hipStream_t s = (hipStream_t)stream;
  const int64_t nsub = std::max<int64_t>(1, (max_len + XC_SUB - 1) / XC_SUB);
  const int per = (int)((nsub + 1023) / 1024), nblk = (int)((nsub + per - 1) / per);
  const size_t per_win = (size_t)npairs * nblk * filters_len * sizeof(double);
  const int group = (int)std::max<size_t>(1, std::min<size_t>({BSS_SCRATCH_CAP / per_win, (size_t)nwin, (size_t)65535}));
  Scratch<double> part(HipFreeAsync{s});
  HIPCHK(scratch_alloc(part, group * per_win));
  for (int w0 = 0; w0 < nwin; w0 += group) {
    const int g = std::min(group, nwin - w0);
    XcorrArgs a;
    a.sig = sig_dev; a.nsig = nsig; a.nsampl = nsampl; a.win = win_dev + 2 * (int64_t)w0; a.pairs = pairs_dev; a.npairs = npairs;
    a.L = filters_len; a.per = per; a.nblk = nblk; a.part = part;
    hipLaunchKernelGGL(k_bss_xcorr, dim3(nblk, npairs, g), dim3(XC_THREADS), 0, s, a);
    LAUNCHCHK("k_bss_xcorr");
    const int64_t n = (int64_t)g * npairs * filters_len;
    hipLaunchKernelGGL(k_bss_xcorr_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const double*)part, n, filters_len, nblk,
                       corr_dev + (int64_t)w0 * npairs * filters_len);
    LAUNCHCHK("k_bss_xcorr_sum");
  }
  return 0;
}

int glowk_bss_solve(const double* corr_dev, int nwin, int npairs, int nref, int filters_len, int nchan_sys, const int* sys_dev, int nsys,
                    double* coef_dev, int* status_dev, void* stream) {
  using namespace glowk_bss;
  if (!corr_dev || !sys_dev || !coef_dev || !status_dev) return fail("null tensor");
  if (filters_len < 1 || filters_len > LMAX) return fail("bss_solve: filters_len must be in [1, 512]");
  if (nref < 1 || nchan_sys < 1 || nchan_sys > nref) return fail("bss_solve: need 1 <= nchan_sys <= nref");
  if ((int64_t)nchan_sys * filters_len > MMAX) return fail("bss_solve: nchan_sys * filters_len must be <= 2048");
  if (nwin < 1 || (int64_t)npairs < 2 * (int64_t)nref * nref) return fail("bss_solve: nwin >= 1 and npairs >= 2 nref^2 required");
  if (nsys < 0) return fail("bss_solve: nsys must be >= 0");
  if (nsys == 0) return 0;
  int dev;
  if (int rc = audio_device({corr_dev, sys_dev, coef_dev, status_dev}, &dev, "bss_solve")) return rc;
  DeviceGuard dg(dev);
  hipStream_t s = (hipStream_t)stream;
  const int M = nchan_sys * filters_len;
  const size_t per_sys = (size_t)M * M * sizeof(double);
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>(BSS_CHOL_CAP / per_sys, (size_t)nsys));
  Scratch<double> A(HipFreeAsync{s});
  HIPCHK(scratch_alloc(A, chunk * per_sys));
  for (int k0 = 0; k0 < nsys; k0 += chunk) {
    CholArgs a;
    a.corr = corr_dev; a.nwin = nwin; a.npairs = npairs; a.P = nref; a.L = filters_len; a.np = nchan_sys; a.sys = sys_dev; a.sys0 = k0;
    a.A = A; a.X = coef_dev; a.status = status_dev;
    hipLaunchKernelGGL(k_bss_chol, dim3(std::min(chunk, nsys - k0)), dim3(CH_THREADS), 0, s, a);
    LAUNCHCHK("k_bss_chol");
  }
  return 0;
}

int glowk_bss_project(const double* sig_dev, int64_t nsampl, int nsrc, int nchan, int filters_len, const int64_t* items_dev, int nitems,
                      int64_t max_len, const double* coef_c_dev, int nsys_c, const double* coef_j_dev, int nsys_j, double* energy_dev,
                      void* stream) {
  using namespace glowk_bss;
  if (!sig_dev || !items_dev || !coef_c_dev || !coef_j_dev || !energy_dev) return fail("null tensor");
  if (nsampl < 1 || nsampl > ((int64_t)1 << 40)) return fail("bss_project: nsampl must be positive");
  if (filters_len < 1 || filters_len > LMAX) return fail("bss_project: filters_len must be in [1, 512]");
  if (nsrc < 1 || nchan < 1 || (int64_t)nsrc * nchan * filters_len > MMAX) return fail("bss_project: nsrc * nchan * filters_len must be <= 2048");
  if (nitems < 0 || nsys_c < 1 || nsys_j < 1 || max_len < 0 || max_len > nsampl) return fail("bss_project: bad item / system counts or max_len");
  if (nitems == 0) return 0;
  int dev;
  if (int rc = audio_device({sig_dev, items_dev, coef_c_dev, coef_j_dev, energy_dev}, &dev, "bss_project")) return rc;
  DeviceGuard dg(dev);
  hipStream_t s = (hipStream_t)stream;
  const int64_t nchunk = (max_len + filters_len - 1 + PJ_OUT - 1) / PJ_OUT;
  if (nchunk > (1 << 24)) return fail("bss_project: window too long");
  const size_t per_item = (size_t)nchunk * NENERGY * sizeof(double);
  const int group = (int)std::max<size_t>(1, std::min<size_t>({BSS_SCRATCH_CAP / per_item, (size_t)nitems, (size_t)(((int64_t)1 << 30) / nchunk)}));
  Scratch<double> part(HipFreeAsync{s});
  HIPCHK(scratch_alloc(part, group * per_item));
  for (int i0 = 0; i0 < nitems; i0 += group) {
    const int g = std::min(group, nitems - i0);
    ProjArgs a;
    a.sig = sig_dev; a.nsampl = nsampl; a.nsrc = nsrc; a.nchan = nchan; a.L = filters_len; a.items = items_dev + 6 * (int64_t)i0; a.nitems = g;
    a.nchunk = (int)nchunk; a.coefC = coef_c_dev; a.nsysC = nsys_c; a.coefJ = coef_j_dev; a.nsysJ = nsys_j; a.part = part;
    hipLaunchKernelGGL(k_bss_project, dim3((unsigned)(g * nchunk)), dim3(PJ_THREADS), 0, s, a);
    LAUNCHCHK("k_bss_project");
    hipLaunchKernelGGL(k_bss_energy_sum, dim3((unsigned)((g * NENERGY + 255) / 256)), dim3(256), 0, s, (const double*)part, g, (int)nchunk,
                       energy_dev + (int64_t)i0 * NENERGY);
    LAUNCHCHK("k_bss_energy_sum");
  }
  return 0;
}

// ---- oracle separation systems (glowk_oracle.h) -----------------------------------------------------------------------------------
namespace {
constexpr int64_t SP_MAX_SAMPLES = (int64_t)1 << 40;
constexpr int64_t SP_MAX_GRID = ((int64_t)1 << 31) - 1;
unsigned stride_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)1 << 18)); }
}

int glowk_sp_stft(const float* x_dev, int nsig, int64_t n, float* spec_dev, void* stream) {
  using namespace glowk_oracle;
  if (nsig < 0 || n < 1 || n > SP_MAX_SAMPLES) return fail("sp_stft: need nsig >= 0 and 1 <= n <= 2^40");
  if (nsig == 0) return 0;                     // nothing to read or write: an empty tensor has no storage, its pointer may be null
  if (!x_dev || !spec_dev) return fail("null tensor");
  const int64_t T = sp_frames(n), ftiles = (T + 31) / 32;
  if (nsig * ftiles > SP_MAX_GRID) return fail("sp_stft: too many signals x frames for one launch");
  int dev;
  if (int rc = audio_device({x_dev, spec_dev}, &dev, "sp_stft")) return rc;
  DeviceGuard dg(dev);
  AudioConsts c;
  if (int rc = audio_consts(dev, &c)) return rc;
  hipLaunchKernelGGL(k_sp_stft, dim3((unsigned)(nsig * ftiles), (NBIN + 127) / 128), dim3(256), 0, (hipStream_t)stream, x_dev, n, (int)T,
                     (int)ftiles, c, reinterpret_cast<float2*>(spec_dev));
  LAUNCHCHK("k_sp_stft");
  return 0;
}

int glowk_sp_istft(const float* spec_dev, int nsig, int frames, int64_t length, float* out_dev, void* stream) {
  using namespace glowk_oracle;
  if (nsig < 0 || frames < 2 || frames > sp_frames(SP_MAX_SAMPLES)) return fail("sp_istft: need nsig >= 0 and frames >= 2");
  if (length < 0 || length > (int64_t)(frames - 1) * HOP) return fail("sp_istft: length must be in [0, (frames - 1) * 1024]");
  if (nsig == 0 || length == 0) return 0;      // an empty output has no storage: its pointer may be null
  if (!spec_dev || !out_dev) return fail("null tensor");
  const int64_t htiles = ((int64_t)frames - 1 + 31) / 32;
  if (nsig * htiles > SP_MAX_GRID) return fail("sp_istft: too many signals x frames for one launch");
  int dev;
  if (int rc = audio_device({spec_dev, out_dev}, &dev, "sp_istft")) return rc;
  DeviceGuard dg(dev);
  AudioConsts c;
  if (int rc = audio_consts(dev, &c)) return rc;
  hipLaunchKernelGGL(k_sp_istft, dim3((unsigned)(nsig * htiles), HOP / 128), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float2*>(spec_dev), frames, (int)htiles, length, c, out_dev);
  LAUNCHCHK("k_sp_istft");
  return 0;
}

int glowk_oracle_mask(float* spec_dev, int nsrc, int nchan, int frames, int irm, double alpha, double theta, uint8_t* mask_dev, void* stream) {
  using namespace glowk_oracle;
  if (!spec_dev) return fail("null tensor");
  if (nsrc < 1 || nsrc > 1024 || nchan < 1 || nchan > 1024 || frames < 1 || frames > sp_frames(SP_MAX_SAMPLES))
    return fail("oracle_mask: need 1 <= nsrc, nchan <= 1024 and frames >= 1");
  if (!std::isfinite(alpha) || std::isnan(theta)) return fail("oracle_mask: alpha must be finite and theta a number");
  if (irm && mask_dev) return fail("oracle_mask: the mask output is for the binary mask only");
  int dev;
  if (int rc = audio_device({spec_dev, mask_dev}, &dev, "oracle_mask")) return rc;
  DeviceGuard dg(dev);
  MaskArgs a;
  a.spec = reinterpret_cast<float2*>(spec_dev); a.plane = (int64_t)NBIN * frames; a.nsrc = nsrc; a.nchan = nchan; a.irm = irm ? 1 : 0;
  a.alpha = alpha; a.theta = theta; a.mask = mask_dev;
  hipLaunchKernelGGL(k_oracle_mask, dim3(stride_grid(nchan * a.plane)), dim3(256), 0, (hipStream_t)stream, a);
  LAUNCHCHK("k_oracle_mask");
  return 0;
}

int glowk_mwf(float* spec_dev, int nsrc, int frames, void* stream) {
  using namespace glowk_oracle;
  if (!spec_dev) return fail("null tensor");
  if (nsrc < 1 || nsrc > MWF_MAX_SRC) return fail("mwf: nsrc must be in [1, 16]");
  if (frames < 1 || frames > sp_frames(SP_MAX_SAMPLES)) return fail("mwf: frames must be >= 1");
  int dev;
  if (int rc = audio_device({spec_dev}, &dev, "mwf")) return rc;
  DeviceGuard dg(dev);
  hipStream_t s = (hipStream_t)stream;
  Scratch<double> stats(HipFreeAsync{s});      // [nsrc][1025][4] doubles, then the matrices [nsrc][1025][8] double2
  const size_t n_stats = (size_t)nsrc * NBIN * 4, n_mat = (size_t)nsrc * NBIN * 16;
  HIPCHK(scratch_alloc(stats, (n_stats + n_mat) * sizeof(double)));
  double2* rmat = reinterpret_cast<double2*>(stats + n_stats);
  float2* spec = reinterpret_cast<float2*>(spec_dev);
  hipLaunchKernelGGL(k_mwf_stats, dim3(NBIN, nsrc), dim3(MS_THREADS), 0, s, (const float2*)spec, frames, stats);
  LAUNCHCHK("k_mwf_stats");
  hipLaunchKernelGGL(k_mwf_norm, dim3((nsrc * NBIN + 255) / 256), dim3(256), 0, s, (const double*)stats, nsrc, rmat);
  LAUNCHCHK("k_mwf_norm");
  hipLaunchKernelGGL(k_mwf_gain, dim3(stride_grid((int64_t)NBIN * frames)), dim3(256), 0, s, spec, nsrc, frames, (const double2*)rmat);
  LAUNCHCHK("k_mwf_gain");
  return 0;
}

int glowk_oracle_mel(const double* mix_dev, const void* src_dev, int nsrc, int64_t n, int src_f64, int irm, double theta, void* out_dev,
                     void* stream) {
  using namespace glowk_oracle;
  if (nsrc < 1 || n < 0 || n > SP_MAX_SAMPLES) return fail("oracle_mel: need nsrc >= 1 and 0 <= n <= 2^40");
  if (std::isnan(theta)) return fail("oracle_mel: theta must be a number");
  if (n == 0) return 0;                        // empty tensors have no storage: their pointers may be null
  if (!mix_dev || !src_dev || !out_dev) return fail("null tensor");
  int dev;
  if (int rc = audio_device({mix_dev, src_dev, out_dev}, &dev, "oracle_mel")) return rc;
  DeviceGuard dg(dev);
  const unsigned g = stride_grid(n);
  if (src_f64)
    hipLaunchKernelGGL(k_oracle_mel<double>, dim3(g), dim3(256), 0, (hipStream_t)stream, mix_dev, (const double*)src_dev, nsrc, n,
                       irm ? 1 : 0, theta, (double*)out_dev);
  else
    hipLaunchKernelGGL(k_oracle_mel<float>, dim3(g), dim3(256), 0, (hipStream_t)stream, mix_dev, (const float*)src_dev, nsrc, n,
                       irm ? 1 : 0, theta, (float*)out_dev);
  LAUNCHCHK("k_oracle_mel");
  return 0;
}

// ---- stereo separation: the multichannel Wiener filter with EM-fitted spatial covariances (glowk_stereo.h) ------------------------
int glowk_mwf_em(const float* x_dev, float* v_dev, int nsrc, int nprob, int frames, int n_iter, float* y_dev, double* r_dev, void* stream) {
  using namespace glowk_stereo;
  if (nsrc < 1 || nsrc > MAX_SRC) return fail("mwf_em: nsrc must be in [1, 16]");
  if (nprob < 0 || nprob > (1 << 20)) return fail("mwf_em: nprob must be in [0, 2^20]");
  if (frames < 1 || frames > (1 << 20)) return fail("mwf_em: frames must be in [1, 2^20]");
  if (n_iter < 0 || n_iter > 1000) return fail("mwf_em: n_iter must be in [0, 1000]");
  if (nprob == 0) return 0;                    // nothing to read or write: an empty tensor has no storage, its pointer may be null
  if (!x_dev || !v_dev || !y_dev) return fail("null tensor");
  int dev;
  if (int rc = audio_device({x_dev, v_dev, y_dev, r_dev}, &dev, "mwf_em")) return rc;
  DeviceGuard dg(dev);
  EmArgs a;
  a.x = reinterpret_cast<const float2*>(x_dev); a.v = v_dev; a.y = reinterpret_cast<float2*>(y_dev); a.r = r_dev;
  a.S = nsrc; a.P = nprob; a.T = frames; a.n_iter = n_iter;
  const int nt = em_threads(frames);
  const size_t staged = em_stage_bytes(nsrc, frames);
  const bool stage = staged <= STAGE_MAX;
  const size_t lds = em_state_bytes(nt) + (stage ? staged : 0);
  const dim3 grid((unsigned)((int64_t)nprob * NBIN));          // <= 2^20 x 1025 workgroups: within one launch
  hipStream_t s = (hipStream_t)stream;
#define GLOWK_EM_LAUNCH(NT) \
  if (stage) hipLaunchKernelGGL((k_mwf_em<NT, true>), grid, dim3(NT), lds, s, a); \
  else hipLaunchKernelGGL((k_mwf_em<NT, false>), grid, dim3(NT), lds, s, a)
  if (nt == 64) { GLOWK_EM_LAUNCH(64); }
  else if (nt == 128) { GLOWK_EM_LAUNCH(128); }
  else { GLOWK_EM_LAUNCH(256); }
#undef GLOWK_EM_LAUNCH
  LAUNCHCHK("k_mwf_em");
  return 0;
}

// ---- whole-signal separation: mel frames of any length, overlapping tiles out and back (glowk_longform.h) -------------------------
namespace {
// the geometry glowk_tile_cut and glowk_tile_stitch share
int tile_geometry(const char* who, int nsig, int width, int hop) {
  if (nsig < 0 || nsig > (1 << 20)) return fail(std::string(who) + ": nsig must be in [0, 2^20]");
  if (width < 2 || width > glowk_long::MAX_WIDTH) return fail(std::string(who) + ": width must be in [2, 128]");
  if (hop < 1 || hop > width) return fail(std::string(who) + ": hop must be in [1, width]");
  return 0;
}

// sin^2(pi (j + 1/2) / width) in fp64, rounded once; zero past the width (never read)
glowk_long::StitchWindow stitch_window(int width) {
  glowk_long::StitchWindow win;
  for (int j = 0; j < glowk_long::MAX_WIDTH; ++j) {
    const double sn = std::sin(3.14159265358979323846 * (j + 0.5) / width);
    win.w[j] = j < width ? (float)(sn * sn) : 0.0f;
  }
  return win;
}

// [a, a + na) and [b, b + nb) floats share an element
bool floats_overlap(const float* a, size_t na, const float* b, size_t nb) {
  const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
  return p < q + nb * sizeof(float) && q < p + na * sizeof(float);
}
}  // namespace

int glowk_mel_frames(const float* audio_dev, int nsig, int64_t n_samples, float* mel_db_dev, float* stft_dev, void* stream) {
  using namespace glowk_audio;
  if (nsig < 0 || nsig > (1 << 20)) return fail("mel_frames: nsig must be in [0, 2^20]");
  if (n_samples < 3 * HOP || n_samples > (int64_t)(glowk_long::MAX_FRAMES - 1) * HOP || n_samples % HOP)
    return fail("mel_frames: n_samples must be a multiple of 512 in [1536, (2^20 - 1) * 512]");
  const int F = 1 + (int)(n_samples / HOP), ftiles = (F + 31) / 32, fblocks = (F + 255) / 256;
  if ((int64_t)nsig * ftiles > INT32_MAX) return fail("mel_frames: too many signals x frames for one launch");
  if (nsig == 0) return 0;                     // nothing to read or write: an empty tensor has no storage, its pointer may be null
  if (!audio_dev || !mel_db_dev) return fail("null tensor");
  int dev;
  if (int rc = audio_device({audio_dev, mel_db_dev, stft_dev}, &dev, "mel_frames")) return rc;
  DeviceGuard dg(dev);
  AudioConsts c;
  if (int rc = audio_consts(dev, &c)) return rc;
  hipStream_t s = (hipStream_t)stream;
  Scratch<float> power(HipFreeAsync{s});       // |X|^2 scratch, only when the caller does not take the complex STFT
  if (!stft_dev) HIPCHK(scratch_alloc(power, (size_t)nsig * NBIN * F * sizeof(float)));
  hipLaunchKernelGGL(k_stft, dim3((unsigned)(nsig * ftiles), (NBIN + 127) / 128), dim3(256), 0, s, audio_dev, (int)n_samples, F, ftiles, c, power,
                     stft_dev);
  LAUNCHCHK("k_stft");
  hipLaunchKernelGGL(glowk_long::k_mel_frames, dim3((unsigned)(nsig * fblocks), NMEL), dim3(256), 0, s, (const float*)power,
                     (const float2*)stft_dev, F, fblocks, c, mel_db_dev);
  LAUNCHCHK("k_mel_frames");
  return 0;
}

int glowk_tile_cut(const float* frames_dev, int nsig, int frames, int width, int hop, float top_db, float* tiles_dev, void* stream) {
  using namespace glowk_long;
  if (int rc = tile_geometry("tile_cut", nsig, width, hop)) return rc;
  if (frames < 1 || frames > MAX_FRAMES) return fail("tile_cut: frames must be in [1, 2^20]");
  if (!(std::fabs(top_db) < 1e30f)) return fail("tile_cut: top_db must be finite");
  const int N = frames <= width ? 1 : 1 + (frames - width + hop - 1) / hop;
  if ((int64_t)nsig * N > INT32_MAX) return fail("tile_cut: too many signals x tiles for one launch");
  if (nsig == 0) return 0;                     // nothing to read or write: an empty tensor has no storage, its pointer may be null
  if (!frames_dev || !tiles_dev) return fail("null tensor");
  int dev;
  if (int rc = audio_device({frames_dev, tiles_dev}, &dev, "tile_cut")) return rc;
  DeviceGuard dg(dev);
  hipLaunchKernelGGL(k_tile_cut, dim3((unsigned)(nsig * N)), dim3(256), 0, (hipStream_t)stream, frames_dev, frames, N, width, hop, top_db, tiles_dev);
  LAUNCHCHK("k_tile_cut");
  return 0;
}

int glowk_tile_stitch(const float* tiles_dev, int nsig, int N, int width, int hop, int frames, float* frames_dev, void* stream) {
  using namespace glowk_long;
  if (int rc = tile_geometry("tile_stitch", nsig, width, hop)) return rc;
  if (N < 1 || N > MAX_FRAMES) return fail("tile_stitch: N must be in [1, 2^20]");
  if (frames < 1 || frames > MAX_FRAMES || frames > (int64_t)(N - 1) * hop + width)
    return fail("tile_stitch: frames must be in [1, min(2^20, (N - 1) * hop + width)]: every frame needs a tile");
  const int fblocks = (frames + 255) / 256;
  if ((int64_t)nsig * fblocks > INT32_MAX) return fail("tile_stitch: too many signals x frames for one launch");
  if (nsig == 0) return 0;                     // nothing to read or write: an empty tensor has no storage, its pointer may be null
  if (!tiles_dev || !frames_dev) return fail("null tensor");
  int dev;
  if (int rc = audio_device({tiles_dev, frames_dev}, &dev, "tile_stitch")) return rc;
  DeviceGuard dg(dev);
  const StitchWindow win = stitch_window(width);
  hipLaunchKernelGGL(k_tile_stitch, dim3((unsigned)(nsig * fblocks), glowk_audio::NMEL), dim3(256), 0, (hipStream_t)stream, tiles_dev, N, width,
                     hop, frames, fblocks, win, frames_dev);
  LAUNCHCHK("k_tile_stitch");
  return 0;
}

// ---- BASIS as one chain over a whole signal: the state is its frames, the priors see its overlapping tiles (glowk_frames.h) --------
int glowk_frames_to_tiles(const float* x_dev, int nsig, int rows, int frames, int width, int hop, float pad, float* tiles_dev,
                          void* stream) {
  using namespace glowk_long;
  if (int rc = tile_geometry("frames_to_tiles", nsig, width, hop)) return rc;
  if (rows < 1 || rows > MAX_ROWS) return fail("frames_to_tiles: rows must be in [1, 65536]");
  if (frames < 1 || frames > MAX_FRAMES) return fail("frames_to_tiles: frames must be in [1, 2^20]");
  if (!(std::fabs(pad) < 1e30f)) return fail("frames_to_tiles: pad must be finite");
  const int N = frames <= width ? 1 : 1 + (frames - width + hop - 1) / hop;
  if ((double)nsig * N * rows * width > 1e12) return fail("frames_to_tiles: too many tile cells for one launch");
  if (nsig == 0) return 0;                     // nothing to read or write: an empty tensor has no storage, its pointer may be null
  if (!x_dev || !tiles_dev) return fail("null tensor");
  const size_t cells = (size_t)nsig * N * rows * width;
  if (floats_overlap(x_dev, (size_t)nsig * rows * frames, tiles_dev, cells)) return fail("frames_to_tiles: the tiles alias the frames");
  int dev;
  if (int rc = audio_device({x_dev, tiles_dev}, &dev, "frames_to_tiles")) return rc;
  DeviceGuard dg(dev);
  hipLaunchKernelGGL(k_frames_to_tiles, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_dev, rows, frames, N,
                     width, hop, pad, cells, tiles_dev);
  LAUNCHCHK("k_frames_to_tiles");
  return 0;
}

int glowk_basis_update_frames(float* x_dev, const float* const* g, const float* const* eps, int nsrc, const float* mixed_dev, int rows,
                              int frames, int width, int hop, int mixing, float eta, float lambda_recon, uint64_t seed, uint64_t step,
                              float pad, float* tiles_out_dev, int* nonfinite_dev, void* stream) {
  using namespace glowk_long;
  if (nsrc < 2 || nsrc > GLOWK_BASIS_MAX_SOURCES) return fail("basis_update_frames: the number of sources must be 2..16");
  if (mixing != GLOWK_MIX_DB && mixing != GLOWK_MIX_MEAN) return fail("basis_update_frames: unknown mixing process");
  if (int rc = tile_geometry("basis_update_frames", 1, width, hop)) return rc;
  if (rows < 1 || rows > MAX_ROWS) return fail("basis_update_frames: rows must be in [1, 65536]");
  if (frames < 1 || frames > MAX_FRAMES) return fail("basis_update_frames: frames must be in [1, 2^20]");
  if (step >= ((uint64_t)1 << 48)) return fail("basis_update_frames: step must be below 2^48 (the source pair shares its counter word)");
  if (!(eta >= 0.0f)) return fail("basis_update_frames: eta must be non-negative");
  if (!(std::fabs(pad) < 1e30f)) return fail("basis_update_frames: pad must be finite");
  if (!x_dev || !g || !mixed_dev) return fail("null tensor");
  for (int k = 0; k < nsrc; ++k)
    if (!g[k]) return fail("null tensor");
  const int N = frames <= width ? 1 : 1 + (frames - width + hop - 1) / hop;
  const size_t n = (size_t)rows * frames, per_source = (size_t)N * rows * width;
  if (floats_overlap(x_dev, nsrc * n, mixed_dev, n)) return fail("basis_update_frames: the states alias the mixture");
  if (tiles_out_dev && (floats_overlap(tiles_out_dev, nsrc * per_source, x_dev, nsrc * n) || floats_overlap(tiles_out_dev, nsrc * per_source, mixed_dev, n)))
    return fail("basis_update_frames: tiles_out aliases the states or the mixture");
  for (int k = 0; k < nsrc; ++k) {
    if (floats_overlap(g[k], per_source, x_dev, nsrc * n)) return fail("basis_update_frames: a gradient aliases the states");
    if (tiles_out_dev && floats_overlap(g[k], per_source, tiles_out_dev, nsrc * per_source))
      return fail("basis_update_frames: a gradient aliases tiles_out");
    if (eps && eps[k] && (floats_overlap(eps[k], n, x_dev, nsrc * n) || (tiles_out_dev && floats_overlap(eps[k], n, tiles_out_dev, nsrc * per_source))))
      return fail("basis_update_frames: a noise tensor aliases the states or tiles_out");
  }
  int dev;
  if (int rc = audio_device({x_dev, mixed_dev, tiles_out_dev, nonfinite_dev}, &dev, "basis_update_frames")) return rc;
  for (int k = 0; k < nsrc; ++k)
    if (int rc = audio_device({x_dev, g[k], eps ? eps[k] : nullptr}, &dev, "basis_update_frames")) return rc;
  DeviceGuard dg(dev);
  BasisFramesArgs a;
  uintptr_t bits = (uintptr_t)x_dev | (uintptr_t)mixed_dev;
  for (int k = 0; k < nsrc; ++k) {
    a.g[k] = g[k]; a.eps[k] = eps ? eps[k] : nullptr;
    bits |= (uintptr_t)a.eps[k];
  }
  a.x = x_dev; a.mixed = mixed_dev; a.tiles_out = tiles_out_dev; a.nonfinite = nonfinite_dev; a.n = n; a.seed = seed; a.step = step;
  a.rows = rows; a.F = frames; a.N = N; a.width = width; a.hop = hop; a.pad_cols = (N - 1) * hop + width - frames;
  a.eta = eta; a.lambda_recon = lambda_recon; a.noise_scale = std::sqrt(2.0f * eta); a.pad = pad;
  a.ln_s = (float)std::log((double)nsrc); a.inv_s = 1.0f / (float)nsrc; a.mixing = mixing; a.vec = (bits & 15) == 0 && n % 4 == 0;
  a.win = stitch_window(width);
  a.qblocks = (unsigned)(((n + 3) / 4 + 255) / 256);          // <= 2^26
  const unsigned pad_blocks = tiles_out_dev ? (unsigned)(((size_t)rows * a.pad_cols + 255) / 256) : 0u;
  const dim3 grid(a.qblocks + pad_blocks);
  switch (nsrc) {
#define GLOWK_CASE(s) case s: hipLaunchKernelGGL(k_basis_update_frames<s>, grid, dim3(256), 0, (hipStream_t)stream, a); break;
    GLOWK_BASIS_EACH_S(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_basis_update_frames");
  return 0;
}

// ---- harmonic / percussive separation by median filtering (glowk_hpss.h) ----------------------------------------------------------
int glowk_median_filter(const float* s_dev, int nsig, int rows, int frames, int size, int axis, float* out_dev, void* stream) {
  using namespace glowk_hpss;
  if (nsig < 0 || nsig > MAX_SIG) return fail("median_filter: nsig must be in [0, 65535]");
  if (rows < 1 || rows > MAX_ROWS) return fail("median_filter: rows must be in [1, 4096]");
  if (frames < 1 || frames > MAX_FRAMES) return fail("median_filter: frames must be in [1, 2^20]");
  if ((int64_t)nsig * rows * frames > (int64_t)INT32_MAX) return fail("median_filter: nsig * rows * frames must be at most 2^31 - 1");
  if (size < 1 || size > MAX_SIZE || size % 2 == 0) return fail("median_filter: size must be odd and in [1, 127]");
  if (axis != 0 && axis != 1) return fail("median_filter: axis must be 0 (along frames) or 1 (along rows)");
  if (nsig == 0) return 0;                     // nothing to read or write: an empty tensor has no storage, its pointer may be null
  if (!s_dev || !out_dev) return fail("null tensor");
  const size_t n = (size_t)nsig * rows * frames;
  if (floats_overlap(s_dev, n, out_dev, n)) return fail("median_filter: out_dev must not be s_dev (the filter does not run in place)");
  int dev;
  if (int rc = audio_device({s_dev, out_dev}, &dev, "median_filter")) return rc;
  DeviceGuard dg(dev);
  const int ftiles = (frames + TILE_F - 1) / TILE_F;
  if (axis == 0) {
    const int64_t lines = (int64_t)nsig * rows;                  // workgroups: <= lines * ftiles <= nsig * rows * frames < 2^31
    hipLaunchKernelGGL(k_median_frames, dim3((unsigned)(((lines + LINES - 1) / LINES) * ftiles)), dim3(LINES * 64), 0, (hipStream_t)stream,
                       s_dev, lines, frames, ftiles, size, out_dev);
    LAUNCHCHK("k_median_frames");
  } else {
    const int rchunks = (rows + ROW_CHUNK - 1) / ROW_CHUNK;
    const size_t lds = (size_t)(ROW_CHUNK + size - 1) * TILE_F * sizeof(float);   // <= 48 640 bytes
    hipLaunchKernelGGL(k_median_rows, dim3((unsigned)((int64_t)nsig * rchunks * ftiles)), dim3(ROW_WAVES * 64), lds, (hipStream_t)stream, s_dev, rows,
                       frames, ftiles, rchunks, size, out_dev);
    LAUNCHCHK("k_median_rows");
  }
  return 0;
}

int glowk_hpss_mask(const float* harm_dev, const float* perc_dev, const float* s_dev, size_t n, float power, float margin_h,
                    float margin_p, float* out_h_dev, float* out_p_dev, void* stream) {
  using namespace glowk_hpss;
  if (n > ((size_t)1 << 40)) return fail("hpss_mask: n must be at most 2^40");
  if (!(power > 0.0f)) return fail("hpss_mask: power must be > 0 (+inf: the hard mask)");
  if (!(margin_h >= 1.0f && margin_h < INFINITY && margin_p >= 1.0f && margin_p < INFINITY))
    return fail("hpss_mask: both margins must be finite and >= 1");
  if (n == 0) return 0;                        // empty tensors have no storage: their pointers may be null
  if (!harm_dev || !perc_dev || !out_h_dev || !out_p_dev) return fail("null tensor");
  if (floats_overlap(out_h_dev, n, out_p_dev, n)) return fail("hpss_mask: the two outputs must be distinct buffers");
  int dev;
  if (int rc = audio_device({harm_dev, perc_dev, s_dev, out_h_dev, out_p_dev}, &dev, "hpss_mask")) return rc;
  DeviceGuard dg(dev);
  hipLaunchKernelGGL(k_hpss_mask, dim3(stride_grid((int64_t)n)), dim3(256), 0, (hipStream_t)stream, harm_dev, perc_dev, s_dev, n, power,
                     margin_h, margin_p, out_h_dev, out_p_dev);
  LAUNCHCHK("k_hpss_mask");
  return 0;
}


// ---- REPET-SIM: nearest-neighbour median filtering (glowk_repet.h) ------------------------------------------------------------------
namespace {
// the ranges the three entries share; 0 or an error
int nn_ranges(const char* what, int nsig, int rows, int frames, int k) {
  using namespace glowk_repet;
  const std::string w(what);
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (rows < 1 || rows > MAX_ROWS) return fail(w + ": rows must be in [1, 4096]");
  if (frames < 1 || frames > MAX_FRAMES) return fail(w + ": frames must be in [1, 32768]");
  if (k < 1 || k > MAX_K) return fail(w + ": k must be in [1, 512]");
  if ((int64_t)nsig * rows * frames > (int64_t)INT32_MAX) return fail(w + ": nsig * rows * frames must be at most 2^31 - 1");
  if ((int64_t)nsig * frames * k > (int64_t)INT32_MAX) return fail(w + ": nsig * frames * k must be at most 2^31 - 1");
  return 0;
}
// the workspace: the norms [nsig][frames], then the frame-major copy [nsig][frames][rows]
size_t nn_work_floats(int nsig, int rows, int frames) { return (size_t)nsig * frames * ((size_t)rows + 1); }
// in bytes, rounded up to 8 as every other size query is: a caller that allocates its workspaces in 8-byte words gets all of it
size_t nn_work_bytes(int nsig, int rows, int frames) { return (nn_work_floats(nsig, rows, frames) * sizeof(float) + 7) / 8 * 8; }
bool bytes_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
  return p < q + nb && q < p + na;
}
}  // namespace

size_t glowk_nn_workspace_bytes(int nsig, int rows, int frames, int k) {
  if (nn_ranges("nn_workspace_bytes", nsig, rows, frames, k)) return 0;
  return nn_work_bytes(nsig, rows, frames);
}

int glowk_nn_neighbors(const float* s_dev, int nsig, int rows, int frames, int k, int width, int32_t* idx_dev, float* sim_dev,
                       void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_repet;
  if (int rc = nn_ranges("nn_neighbors", nsig, rows, frames, k)) return rc;
  if (width < 1 || width > MAX_WIDTH) return fail("nn_neighbors: width must be in [1, 2^20]");
  if (nsig == 0) return 0;                     // nothing to read or write: an empty tensor has no storage, its pointer may be null
  if (!s_dev || !idx_dev || !work_dev) return fail("null tensor");
  const size_t need = nn_work_bytes(nsig, rows, frames);
  if (work_bytes < need) return fail("nn_neighbors: work_bytes is smaller than glowk_nn_workspace_bytes says");
  const size_t n = (size_t)nsig * rows * frames * 4, nk = (size_t)nsig * frames * k * 4;
  if (bytes_overlap(s_dev, n, idx_dev, nk) || (sim_dev && bytes_overlap(s_dev, n, sim_dev, nk)) || (sim_dev && bytes_overlap(idx_dev, nk, sim_dev, nk)))
    return fail("nn_neighbors: s_dev, idx_dev and sim_dev must not overlap");
  if (bytes_overlap(work_dev, need, s_dev, n) || bytes_overlap(work_dev, need, idx_dev, nk) || (sim_dev && bytes_overlap(work_dev, need, sim_dev, nk)))
    return fail("nn_neighbors: work_dev must not overlap the tensors");
  int dev;
  if (int rc = audio_device({s_dev, idx_dev, sim_dev, work_dev}, &dev, "nn_neighbors")) return rc;
  DeviceGuard dg(dev);
  float* norm = (float*)work_dev;
  const int64_t total = (int64_t)nsig * frames;
  hipLaunchKernelGGL(k_nn_norms, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s_dev, total, rows, frames, norm);
  LAUNCHCHK("k_nn_norms");
  const int qtiles = (frames + QT - 1) / QT;
  const dim3 grid((unsigned)((int64_t)nsig * qtiles));        // <= 65535 * 1024
  if (k <= K_SMALL)
    hipLaunchKernelGGL((k_nn_topk<K_SMALL, 2>), grid, dim3(256), 0, (hipStream_t)stream, s_dev, (const float*)norm, rows, frames, k, width, qtiles,
                       idx_dev, sim_dev);
  else
    hipLaunchKernelGGL((k_nn_topk<MAX_K, 1>), grid, dim3(256), 0, (hipStream_t)stream, s_dev, (const float*)norm, rows, frames, k, width, qtiles,
                       idx_dev, sim_dev);
  LAUNCHCHK("k_nn_topk");
  return 0;
}

int glowk_nn_median(const float* s_dev, const int32_t* idx_dev, int nsig, int rows, int frames, int k, float* out_dev, void* work_dev,
                    size_t work_bytes, void* stream) {
  using namespace glowk_repet;
  if (int rc = nn_ranges("nn_median", nsig, rows, frames, k)) return rc;
  if (nsig == 0) return 0;
  if (!s_dev || !idx_dev || !out_dev || !work_dev) return fail("null tensor");
  const size_t need = nn_work_bytes(nsig, rows, frames);
  if (work_bytes < need) return fail("nn_median: work_bytes is smaller than glowk_nn_workspace_bytes says");
  const size_t n = (size_t)nsig * rows * frames * 4, nk = (size_t)nsig * frames * k * 4;
  if (bytes_overlap(s_dev, n, out_dev, n)) return fail("nn_median: out_dev must not be s_dev (the filter does not run in place)");
  if (bytes_overlap(idx_dev, nk, out_dev, n)) return fail("nn_median: out_dev must not overlap idx_dev");
  if (bytes_overlap(work_dev, need, s_dev, n) || bytes_overlap(work_dev, need, idx_dev, nk) || bytes_overlap(work_dev, need, out_dev, n))
    return fail("nn_median: work_dev must not overlap the tensors");
  int dev;
  if (int rc = audio_device({s_dev, idx_dev, out_dev, work_dev}, &dev, "nn_median")) return rc;
  DeviceGuard dg(dev);
  float* st = (float*)work_dev + (size_t)nsig * frames;
  const int rtiles = (rows + 31) / 32, ftiles = (frames + 31) / 32;    // workgroups: <= nsig * rows * frames < 2^31 in both launches
  hipLaunchKernelGGL(k_nn_transpose, dim3((unsigned)((int64_t)nsig * rtiles * ftiles)), dim3(256), 0, (hipStream_t)stream, s_dev, rows, frames,
                     rtiles, ftiles, st);
  LAUNCHCHK("k_nn_transpose");
  const int ll = k <= 192 ? 0 : k <= 384 ? 1 : 2;                // lanes per output 1 << ll: (k + 1) * (64 >> ll) floats of LDS stay within 49 KiB
  const int no = 64 >> ll, rchunks = (rows + no - 1) / no;
  const size_t lds = ((size_t)k + 1) * no * sizeof(float);       // a spare slot for the entries that are not neighbours
  hipLaunchKernelGGL(k_nn_median, dim3((unsigned)((int64_t)nsig * rchunks * frames)), dim3(64), lds, (hipStream_t)stream, s_dev, (const float*)st,
                     idx_dev, rows, frames, k, rchunks, ll, out_dev);
  LAUNCHCHK("k_nn_median");
  return 0;
}

// ---- REPET and adaptive REPET: beat spectrum, period, periodic neighbours (glowk_beat.h) --------------------------------------------
namespace {
// the ranges glowk_beat_workspace_bytes and glowk_beat_spectrum share; 0 or an error
int beat_ranges(const char* what, int nsig, int rows, int frames, int nlags, int win, int step) {
  using namespace glowk_beat;
  const std::string w(what);
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (rows < 1 || rows > MAX_ROWS) return fail(w + ": rows must be in [1, 4096]");
  if (frames < 1 || frames > MAX_FRAMES) return fail(w + ": frames must be in [1, 32768]");
  if (nlags < 1 || nlags > frames) return fail(w + ": nlags must be in [1, frames]");
  if (win != 0 && (win < 2 || win > frames)) return fail(w + ": win must be 0 (one window, the whole signal) or in [2, frames]");
  if (win != 0 && (step < 1 || step > win)) return fail(w + ": step must be in [1, win]");
  if ((int64_t)nsig * rows * frames > (int64_t)INT32_MAX) return fail(w + ": nsig * rows * frames must be at most 2^31 - 1");
  const BeatPlan p = beat_plan(frames, nlags, win, step);
  if ((int64_t)nsig * p.nwin * nlags > (int64_t)INT32_MAX) return fail(w + ": nsig * nwin * nlags must be at most 2^31 - 1");
  if ((int64_t)nsig * p.nwin * p.nu * p.nch > (int64_t)INT32_MAX) return fail(w + ": nsig * nwin * nu * nch (the workgroups) must be at most 2^31 - 1");
  return 0;
}
size_t beat_work_bytes(int nsig, const glowk_beat::BeatPlan& p) {
  return (size_t)nsig * p.nwin * p.nu * p.nch * glowk_beat::NLP * sizeof(double);
}
}  // namespace

size_t glowk_beat_workspace_bytes(int nsig, int rows, int frames, int nlags, int win, int step) {
  if (beat_ranges("beat_workspace_bytes", nsig, rows, frames, nlags, win, step)) return 0;
  return beat_work_bytes(nsig, glowk_beat::beat_plan(frames, nlags, win, step));
}

int glowk_beat_spectrum(const float* s_dev, int nsig, int rows, int frames, int nlags, int win, int step, float* beat_dev, void* work_dev,
                        size_t work_bytes, void* stream) {
  using namespace glowk_beat;
  if (int rc = beat_ranges("beat_spectrum", nsig, rows, frames, nlags, win, step)) return rc;
  if (nsig == 0) return 0;                     // nothing to read or write: an empty tensor has no storage, its pointer may be null
  if (!s_dev || !beat_dev || !work_dev) return fail("null tensor");
  const BeatPlan p = beat_plan(frames, nlags, win, step);
  const size_t need = beat_work_bytes(nsig, p);
  if (work_bytes < need) return fail("beat_spectrum: work_bytes is smaller than glowk_beat_workspace_bytes says");
  if ((uintptr_t)work_dev % 8) return fail("beat_spectrum: work_dev must be aligned to 8 bytes");
  const size_t n = (size_t)nsig * rows * frames * 4, nb = (size_t)nsig * p.nwin * nlags * 4;
  if (bytes_overlap(s_dev, n, beat_dev, nb)) return fail("beat_spectrum: s_dev and beat_dev must not overlap");
  if (bytes_overlap(work_dev, need, s_dev, n) || bytes_overlap(work_dev, need, beat_dev, nb))
    return fail("beat_spectrum: work_dev must not overlap the tensors");
  int dev;
  if (int rc = audio_device({s_dev, beat_dev, work_dev}, &dev, "beat_spectrum")) return rc;
  DeviceGuard dg(dev);
  double* part = (double*)work_dev;
  hipLaunchKernelGGL(k_beat_gram, dim3((unsigned)((int64_t)nsig * p.nwin * p.nu * p.nch)), dim3(256), 0, (hipStream_t)stream, s_dev, rows, frames, win,
                     step, p.nwin, p.nu, p.nch, p.tpw, nlags, part);
  LAUNCHCHK("k_beat_gram");
  const int64_t total = (int64_t)nsig * p.nwin * nlags;
  hipLaunchKernelGGL(k_beat_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double*)part, total, rows, frames,
                     win, step, p.nwin, p.nu, p.nch, nlags, beat_dev);
  LAUNCHCHK("k_beat_reduce");
  return 0;
}

int glowk_beat_period(const float* beat_dev, int nseg, int nlags, int pmin, int pmax, int32_t* period_dev, void* stream) {
  using namespace glowk_beat;
  if (nseg < 0) return fail("beat_period: nseg must be in [0, 2^31 - 1]");
  if (nlags < 2 || nlags > MAX_FRAMES) return fail("beat_period: nlags must be in [2, 32768]");
  if (pmin < 1 || pmin > pmax || pmax > nlags - 1) return fail("beat_period: 1 <= pmin <= pmax <= nlags - 1 is required");
  if ((int64_t)nseg * nlags > (int64_t)INT32_MAX) return fail("beat_period: nseg * nlags must be at most 2^31 - 1");
  if (nseg == 0) return 0;
  if (!beat_dev || !period_dev) return fail("null tensor");
  if (bytes_overlap(beat_dev, (size_t)nseg * nlags * 4, period_dev, (size_t)nseg * 4)) return fail("beat_period: beat_dev and period_dev must not overlap");
  int dev;
  if (int rc = audio_device({beat_dev, period_dev}, &dev, "beat_period")) return rc;
  DeviceGuard dg(dev);
  hipLaunchKernelGGL(k_beat_period, dim3((unsigned)nseg), dim3(64), 0, (hipStream_t)stream, beat_dev, nlags, pmin, pmax, period_dev);
  LAUNCHCHK("k_beat_period");
  return 0;
}

int glowk_period_neighbors(const int32_t* period_dev, int nsig, int frames, int nper, int step, int k, int32_t* idx_dev, void* stream) {
  using namespace glowk_beat;
  if (nsig < 0 || nsig > MAX_SIG) return fail("period_neighbors: nsig must be in [0, 65535]");
  if (frames < 1 || frames > MAX_FRAMES) return fail("period_neighbors: frames must be in [1, 32768]");
  if (nper < 1 || nper > MAX_FRAMES) return fail("period_neighbors: nper must be in [1, 32768]");
  if (step < 1 || step > MAX_FRAMES) return fail("period_neighbors: step must be in [1, 32768]");
  if (k < 1 || k > MAX_K) return fail("period_neighbors: k must be in [1, 512]");
  if ((int64_t)nsig * frames * k > (int64_t)INT32_MAX) return fail("period_neighbors: nsig * frames * k must be at most 2^31 - 1");
  if (nsig == 0) return 0;
  if (!period_dev || !idx_dev) return fail("null tensor");
  if (bytes_overlap(period_dev, (size_t)nsig * nper * 4, idx_dev, (size_t)nsig * frames * k * 4))
    return fail("period_neighbors: period_dev and idx_dev must not overlap");
  int dev;
  if (int rc = audio_device({period_dev, idx_dev}, &dev, "period_neighbors")) return rc;
  DeviceGuard dg(dev);
  const int64_t total = (int64_t)nsig * frames;
  hipLaunchKernelGGL(k_period_neighbors, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, period_dev, total, frames, nper, step,
                     k, idx_dev);
  LAUNCHCHK("k_period_neighbors");
  return 0;
}

// ---- 2DFT separation: real 2-D DFT and inverse, plane std, peak mask (glowk_dft2.h) --------------------------------------------------
namespace {
int dft2_ranges(const char* what, int nsig, int rows, int frames) {
  using namespace glowk_dft2;
  const std::string w(what);
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (rows < 1 || rows > MAX_ROWS) return fail(w + ": rows must be in [1, 4096]");
  if (frames < 1 || frames > MAX_FRAMES) return fail(w + ": frames must be in [1, 32768]");
  if ((int64_t)nsig * rows * frames > (int64_t)INT32_MAX) return fail(w + ": nsig * rows * frames must be at most 2^31 - 1");
  return 0;
}
// the two twiddle tables filled; 0 or an error.  The launches of both transforms begin with this.
int dft2_tables(const glowk_dft2::Dft2Plan& p, int rows, int frames, void* work_dev, hipStream_t s) {
  using namespace glowk_dft2;
  char* w = (char*)work_dev;
  hipLaunchKernelGGL(k_dft2_table, dim3((unsigned)((frames + 255) / 256)), dim3(256), 0, s, (float2*)(w + p.tab_t_off), frames);
  LAUNCHCHK("k_dft2_table");
  hipLaunchKernelGGL(k_dft2_table, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (float2*)(w + p.tab_r_off), rows);
  LAUNCHCHK("k_dft2_table");
  return 0;
}
}  // namespace

size_t glowk_dft2_workspace_bytes(int nsig, int rows, int frames) {
  if (dft2_ranges("dft2_workspace_bytes", nsig, rows, frames) || nsig == 0) return 0;
  return glowk_dft2::dft2_plan(nsig, rows, frames).bytes;
}

int glowk_rdft2(const float* s_dev, int nsig, int rows, int frames, float* spec_dev, float* mag_dev, void* work_dev, size_t work_bytes,
                void* stream) {
  using namespace glowk_dft2;
  if (int rc = dft2_ranges("rdft2", nsig, rows, frames)) return rc;
  if (nsig == 0) return 0;                     // nothing to read or write: an empty tensor has no storage, its pointer may be null
  if (!s_dev || !spec_dev || !work_dev) return fail("null tensor");
  const Dft2Plan p = dft2_plan(nsig, rows, frames);
  if (work_bytes < p.bytes) return fail("rdft2: work_bytes is smaller than glowk_dft2_workspace_bytes says");
  if ((uintptr_t)work_dev % 8 || (uintptr_t)spec_dev % 8) return fail("rdft2: work_dev and spec_dev must be aligned to 8 bytes");
  const size_t n = (size_t)nsig * rows * frames * 4, ns = (size_t)nsig * rows * p.fc * 8;
  if (bytes_overlap(s_dev, n, spec_dev, ns) || (mag_dev && (bytes_overlap(s_dev, n, mag_dev, n) || bytes_overlap(spec_dev, ns, mag_dev, n))))
    return fail("rdft2: s_dev, spec_dev and mag_dev must not overlap");
  if (bytes_overlap(work_dev, p.bytes, s_dev, n) || bytes_overlap(work_dev, p.bytes, spec_dev, ns) || (mag_dev && bytes_overlap(work_dev, p.bytes, mag_dev, n)))
    return fail("rdft2: work_dev must not overlap the tensors");
  if (p.fwd_frames_blocks > (int64_t)INT32_MAX || p.rows_blocks > (int64_t)INT32_MAX) return fail("rdft2: too many workgroups");
  int dev;
  if (int rc = audio_device({s_dev, spec_dev, mag_dev, work_dev}, &dev, "rdft2")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = dft2_tables(p, rows, frames, work_dev, st)) return rc;
  char* w = (char*)work_dev;
  const float2 *tab_t = (const float2*)(w + p.tab_t_off), *tab_r = (const float2*)(w + p.tab_r_off);
  float2* mid = (float2*)(w + p.mid_off);
  const int ng = (int)groups_of(p.fc, NT_FWD);
  if (frames <= LDS_TAB_MAX)
    hipLaunchKernelGGL(k_rdft_frames<true>, dim3((unsigned)p.fwd_frames_blocks), dim3(256), (size_t)frames * 8, st, s_dev, p.m_frames, frames, p.fc, ng,
                       tab_t, mid);
  else
    hipLaunchKernelGGL(k_rdft_frames<false>, dim3((unsigned)p.fwd_frames_blocks), dim3(256), 0, st, s_dev, p.m_frames, frames, p.fc, ng, tab_t, mid);
  LAUNCHCHK("k_rdft_frames");
  hipLaunchKernelGGL(k_cdft_rows, dim3((unsigned)p.rows_blocks), dim3(256), (size_t)rows * 8, st, (const float2*)mid, (const float*)nullptr, rows, p.fc, frames,
                     (int)ceil_div64(rows, TILE), (int)groups_of(p.fc, NT_ROWS), tab_r, 1.0f, (float2*)spec_dev, mag_dev);
  LAUNCHCHK("k_cdft_rows");
  if (mag_dev) {
    const int nself = frames % 2 == 0 && frames > 1 ? 2 : 1;
    const int64_t total = (int64_t)nsig * rows * (frames - p.fc + nself);
    hipLaunchKernelGGL(k_mag_mirror, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, mag_dev, total, rows, frames, p.fc, nself);
    LAUNCHCHK("k_mag_mirror");
  }
  return 0;
}

int glowk_irdft2(const float* spec_dev, const float* mask_dev, int nsig, int rows, int frames, float* out_dev, void* work_dev,
                 size_t work_bytes, void* stream) {
  using namespace glowk_dft2;
  if (int rc = dft2_ranges("irdft2", nsig, rows, frames)) return rc;
  if (nsig == 0) return 0;
  if (!spec_dev || !out_dev || !work_dev) return fail("null tensor");
  const Dft2Plan p = dft2_plan(nsig, rows, frames);
  if (work_bytes < p.bytes) return fail("irdft2: work_bytes is smaller than glowk_dft2_workspace_bytes says");
  if ((uintptr_t)work_dev % 8 || (uintptr_t)spec_dev % 8) return fail("irdft2: work_dev and spec_dev must be aligned to 8 bytes");
  const size_t n = (size_t)nsig * rows * frames * 4, ns = (size_t)nsig * rows * p.fc * 8;
  if (bytes_overlap(out_dev, n, spec_dev, ns) || (mask_dev && bytes_overlap(out_dev, n, mask_dev, n)))
    return fail("irdft2: out_dev must not overlap spec_dev or mask_dev");
  if (bytes_overlap(work_dev, p.bytes, out_dev, n) || bytes_overlap(work_dev, p.bytes, spec_dev, ns) || (mask_dev && bytes_overlap(work_dev, p.bytes, mask_dev, n)))
    return fail("irdft2: work_dev must not overlap the tensors");
  if (p.inv_frames_blocks > (int64_t)INT32_MAX || p.rows_blocks > (int64_t)INT32_MAX) return fail("irdft2: too many workgroups");
  int dev;
  if (int rc = audio_device({spec_dev, mask_dev, out_dev, work_dev}, &dev, "irdft2")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = dft2_tables(p, rows, frames, work_dev, st)) return rc;
  char* w = (char*)work_dev;
  const float2 *tab_t = (const float2*)(w + p.tab_t_off), *tab_r = (const float2*)(w + p.tab_r_off);
  float2* mid = (float2*)(w + p.mid_off);
  hipLaunchKernelGGL(k_cdft_rows, dim3((unsigned)p.rows_blocks), dim3(256), (size_t)rows * 8, st, (const float2*)spec_dev, mask_dev, rows, p.fc, frames,
                     (int)ceil_div64(rows, TILE), (int)groups_of(p.fc, NT_ROWS), tab_r, -1.0f, mid, (float*)nullptr);
  LAUNCHCHK("k_cdft_rows");
  const float scale = (float)(1.0 / ((double)rows * (double)frames));
  const int ngi = (int)groups_of(frames, NT_INV);
  if (frames <= LDS_TAB_MAX)
    hipLaunchKernelGGL(k_irdft_frames<true>, dim3((unsigned)p.inv_frames_blocks), dim3(256), (size_t)frames * 8, st, (const float2*)mid, p.m_frames,
                       frames, p.fc, ngi, tab_t, scale, out_dev);
  else
    hipLaunchKernelGGL(k_irdft_frames<false>, dim3((unsigned)p.inv_frames_blocks), dim3(256), 0, st, (const float2*)mid, p.m_frames, frames, p.fc, ngi,
                       tab_t, scale, out_dev);
  LAUNCHCHK("k_irdft_frames");
  return 0;
}

size_t glowk_plane_std_workspace_bytes(int nsig, int64_t n) {
  if (nsig < 1 || nsig > glowk_dft2::MAX_SIG || n < 1 || (int64_t)nsig * n > (int64_t)INT32_MAX) return 0;
  return (size_t)nsig * glowk_dft2::std_blocks(n) * 2 * sizeof(double);
}

int glowk_plane_std(const float* plane_dev, int nsig, int64_t n, double* out_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_dft2;
  if (nsig < 0 || nsig > MAX_SIG) return fail("plane_std: nsig must be in [0, 65535]");
  if (n < 1 || n > (int64_t)INT32_MAX) return fail("plane_std: n must be in [1, 2^31 - 1]");
  if ((int64_t)nsig * n > (int64_t)INT32_MAX) return fail("plane_std: nsig * n must be at most 2^31 - 1");
  if (nsig == 0) return 0;
  if (!plane_dev || !out_dev || !work_dev) return fail("null tensor");
  const int nb = std_blocks(n);
  const size_t need = (size_t)nsig * nb * 2 * sizeof(double), np = (size_t)nsig * n * 4, no = (size_t)nsig * 16;
  if (work_bytes < need) return fail("plane_std: work_bytes is smaller than glowk_plane_std_workspace_bytes says");
  if ((uintptr_t)work_dev % 8 || (uintptr_t)out_dev % 8) return fail("plane_std: work_dev and out_dev must be aligned to 8 bytes");
  if (bytes_overlap(plane_dev, np, out_dev, no)) return fail("plane_std: plane_dev and out_dev must not overlap");
  if (bytes_overlap(work_dev, need, plane_dev, np) || bytes_overlap(work_dev, need, out_dev, no)) return fail("plane_std: work_dev must not overlap the tensors");
  int dev;
  if (int rc = audio_device({plane_dev, out_dev, work_dev}, &dev, "plane_std")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  double *sums = (double*)work_dev, *sq = sums + (size_t)nsig * nb;
  hipLaunchKernelGGL(k_plane_sum, dim3((unsigned)(nsig * nb)), dim3(256), 0, st, plane_dev, n, nb, (const double*)sums, 0, sums);
  LAUNCHCHK("k_plane_sum");
  hipLaunchKernelGGL(k_plane_sum, dim3((unsigned)(nsig * nb)), dim3(256), 0, st, plane_dev, n, nb, (const double*)sums, 1, sq);
  LAUNCHCHK("k_plane_sum");
  hipLaunchKernelGGL(k_plane_std_final, dim3((unsigned)((nsig + 63) / 64)), dim3(64), 0, st, (const double*)sums, (const double*)sq, n, nb, nsig, out_dev);
  LAUNCHCHK("k_plane_std_final");
  return 0;
}

namespace {
int peak_ranges(const char* what, int nsig, int rows, int cols, int nb_r, int nb_c) {
  using namespace glowk_dft2;
  const std::string w(what);
  if (int rc = dft2_ranges(what, nsig, rows, cols)) return rc;
  if (nb_r < 1 || nb_r > MAX_NB || !(nb_r & 1)) return fail(w + ": nb_r must be odd and in [1, 127]");
  if (nb_c < 1 || nb_c > MAX_NB || !(nb_c & 1)) return fail(w + ": nb_c must be odd and in [1, 127]");
  return 0;
}
}  // namespace

size_t glowk_peak_workspace_bytes(int nsig, int rows, int cols) {
  if (dft2_ranges("peak_workspace_bytes", nsig, rows, cols)) return 0;
  return (size_t)nsig * rows * cols * 8;
}

int glowk_peak_mask(const float* plane_dev, int nsig, int rows, int cols, int nb_r, int nb_c, const float* thr_dev, float* mask_dev,
                    float* max_dev, float* min_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_dft2;
  if (int rc = peak_ranges("peak_mask", nsig, rows, cols, nb_r, nb_c)) return rc;
  if (nsig == 0) return 0;
  if (!plane_dev || !mask_dev || !work_dev) return fail("null tensor");
  const size_t n = (size_t)nsig * rows * cols * 4, need = 2 * n;
  if (work_bytes < need) return fail("peak_mask: work_bytes is smaller than glowk_peak_workspace_bytes says");
  if ((uintptr_t)work_dev % 4) return fail("peak_mask: work_dev must be aligned to 4 bytes");
  const void* outs[3] = {mask_dev, max_dev, min_dev};
  for (int i = 0; i < 3; ++i) {
    if (!outs[i]) continue;
    if (bytes_overlap(plane_dev, n, outs[i], n) || (thr_dev && bytes_overlap(thr_dev, (size_t)nsig * 4, outs[i], n)))
      return fail("peak_mask: the outputs must not overlap plane_dev or thr_dev");
    if (bytes_overlap(work_dev, need, outs[i], n)) return fail("peak_mask: work_dev must not overlap the tensors");
    for (int j = i + 1; j < 3; ++j)
      if (outs[j] && bytes_overlap(outs[i], n, outs[j], n)) return fail("peak_mask: the outputs must be distinct buffers and not overlap");
  }
  if (bytes_overlap(work_dev, need, plane_dev, n) || (thr_dev && bytes_overlap(work_dev, need, thr_dev, (size_t)nsig * 4)))
    return fail("peak_mask: work_dev must not overlap the tensors");
  int dev;
  if (int rc = audio_device({plane_dev, thr_dev, mask_dev, max_dev, min_dev, work_dev}, &dev, "peak_mask")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  float *hmax = (float*)work_dev, *hmin = hmax + (size_t)nsig * rows * cols;
  const int nseg = (cols + PK_SEG - 1) / PK_SEG, rtiles = (rows + PK_TR - 1) / PK_TR, ctiles = (cols + PK_TC - 1) / PK_TC;
  hipLaunchKernelGGL(k_peak_cols, dim3((unsigned)((int64_t)nsig * rows * nseg)), dim3(256), 0, st, plane_dev, cols, nseg, nb_c, hmax, hmin);
  LAUNCHCHK("k_peak_cols");
  hipLaunchKernelGGL(k_peak_rows, dim3((unsigned)((int64_t)nsig * rtiles * ctiles)), dim3(256), 0, st, plane_dev, (const float*)hmax, (const float*)hmin,
                     rows, cols, rtiles, ctiles, nb_r, thr_dev, mask_dev, max_dev, min_dev);
  LAUNCHCHK("k_peak_rows");
  return 0;
}

// ---- DUET: features, the attenuation-delay histogram, its peaks, the assignment (glowk_duet.h) --------------------------------------
namespace {
int duet_shape(const std::string& w, int nsig, int rows, int frames) {
  using namespace glowk_duet;
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (rows < 1 || rows > MAX_ROWS) return fail(w + ": rows must be in [1, 4096]");
  if (frames < 1 || frames > MAX_FRAMES) return fail(w + ": frames must be in [1, 32768]");
  if ((int64_t)nsig * 2 * rows * frames > (int64_t)INT32_MAX) return fail(w + ": nsig * 2 * rows * frames must be at most 2^31 - 1");
  return 0;
}
int duet_bins(const std::string& w, int n_a, int n_d) {
  if (n_a < 1 || n_d < 1 || (int64_t)n_a * n_d > glowk_duet::MAX_BINS) return fail(w + ": n_a and n_d must be at least 1 and n_a * n_d at most 16384");
  return 0;
}
int duet_grid(const std::string& w, double a_lo, double a_hi, int n_a, double d_lo, double d_hi, int n_d) {
  if (int rc = duet_bins(w, n_a, n_d)) return rc;
  if (!(std::isfinite(a_lo) && std::isfinite(a_hi) && a_lo < a_hi && std::isfinite(a_hi - a_lo)))
    return fail(w + ": the attenuation range must be finite with a_lo < a_hi");
  if (!(std::isfinite(d_lo) && std::isfinite(d_hi) && d_lo < d_hi && std::isfinite(d_hi - d_lo)))
    return fail(w + ": the delay range must be finite with d_lo < d_hi");
  return 0;
}
int duet_exponents(const std::string& w, double p, double q) {
  if (!std::isfinite(p) || !std::isfinite(q)) return fail(w + ": the exponents p and q must be finite");
  return 0;
}
int duet_smooth(const std::string& w, int smooth) {
  if (smooth < 0 || smooth > glowk_duet::MAX_SMOOTH) return fail(w + ": smooth must be in [0, 3]");
  return 0;
}
// the two passes of the histogram, staged (x null) or fused (the planes null)
int duet_hist_launch(const float* x_dev, const double* a_dev, const double* d_dev, const double* w_dev, int nsig, int64_t cells, int rows, int frames,
                     double p, double q, const glowk_duet::Ranges& rg, int smooth, int64_t* hist_dev, int32_t* es_dev, void* work_dev, hipStream_t st) {
  using namespace glowk_duet;
  const HistPlan pl = hist_plan(nsig, cells, rg.n_a, rg.n_d);
  const int shift = hist_shift(cells, smooth);
  double* partial = (double*)work_dev;
  const dim3 grid((unsigned)((int64_t)nsig * pl.groups)), block(HIST_THREADS);
  static std::once_flag lds_once;                              // a plane of more than 64 KB needs the attribute on some runtimes
  std::call_once(lds_once, [] {
    (void)hipFuncSetAttribute((const void*)k_duet_hist<true>, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_BINS * 8);
    (void)hipFuncSetAttribute((const void*)k_duet_hist<false>, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_BINS * 8);
    (void)hipGetLastError();
  });
  if (hipMemsetAsync(hist_dev, 0, (size_t)nsig * rg.n_a * rg.n_d * 8, st) != hipSuccess) return fail("duet_histogram: hipMemsetAsync failed");
  if (x_dev) {
    hipLaunchKernelGGL(k_duet_wmax<true>, grid, block, 0, st, (const float2*)x_dev, a_dev, d_dev, w_dev, cells, rows, frames, p, q, rg, pl.groups, partial);
    LAUNCHCHK("k_duet_wmax");
    hipLaunchKernelGGL(k_duet_hist<true>, grid, block, pl.lds_bytes, st, (const float2*)x_dev, a_dev, d_dev, w_dev, cells, rows, frames, p, q, rg, pl.groups,
                       shift, (const double*)partial, (unsigned long long*)hist_dev, es_dev);
  } else {
    hipLaunchKernelGGL(k_duet_wmax<false>, grid, block, 0, st, (const float2*)x_dev, a_dev, d_dev, w_dev, cells, rows, frames, p, q, rg, pl.groups, partial);
    LAUNCHCHK("k_duet_wmax");
    hipLaunchKernelGGL(k_duet_hist<false>, grid, block, pl.lds_bytes, st, (const float2*)x_dev, a_dev, d_dev, w_dev, cells, rows, frames, p, q, rg, pl.groups,
                       shift, (const double*)partial, (unsigned long long*)hist_dev, es_dev);
  }
  LAUNCHCHK("k_duet_hist");
  return 0;
}
}  // namespace

int glowk_duet_features(const float* x_dev, int nsig, int rows, int frames, double p, double q, double* alpha_dev, double* delta_dev, double* w_dev,
                        void* stream) {
  using namespace glowk_duet;
  if (int rc = duet_shape("duet_features", nsig, rows, frames)) return rc;
  if (int rc = duet_exponents("duet_features", p, q)) return rc;
  if (nsig == 0) return 0;
  if (!x_dev || !alpha_dev || !delta_dev || !w_dev) return fail("null tensor");
  const int64_t total = (int64_t)nsig * rows * frames;
  const size_t nx = (size_t)total * 16, nf = (size_t)total * 8;
  if ((uintptr_t)x_dev % 8 || (uintptr_t)alpha_dev % 8 || (uintptr_t)delta_dev % 8 || (uintptr_t)w_dev % 8)
    return fail("duet_features: the tensors must be aligned to 8 bytes");
  const void* outs[3] = {alpha_dev, delta_dev, w_dev};
  for (int i = 0; i < 3; ++i) {
    if (bytes_overlap(x_dev, nx, outs[i], nf)) return fail("duet_features: the outputs must not overlap x_dev");
    for (int j = i + 1; j < 3; ++j)
      if (bytes_overlap(outs[i], nf, outs[j], nf)) return fail("duet_features: the outputs must be distinct buffers and not overlap");
  }
  int dev;
  if (int rc = audio_device({x_dev, alpha_dev, delta_dev, w_dev}, &dev, "duet_features")) return rc;
  DeviceGuard dg(dev);
  hipLaunchKernelGGL(k_duet_features, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float2*)x_dev, total, rows, frames, p, q,
                     alpha_dev, delta_dev, w_dev);
  LAUNCHCHK("k_duet_features");
  return 0;
}

size_t glowk_duet_hist_workspace_bytes(int nsig, int64_t cells, int n_a, int n_d) {
  using namespace glowk_duet;
  if (nsig < 1 || nsig > MAX_SIG || cells < 1 || cells > (int64_t)MAX_ROWS * MAX_FRAMES || n_a < 1 || n_d < 1 || (int64_t)n_a * n_d > MAX_BINS) return 0;
  return hist_plan(nsig, cells, n_a, n_d).bytes;
}

int glowk_duet_histogram(const double* alpha_dev, const double* delta_dev, const double* w_dev, int nsig, int64_t cells, double a_lo, double a_hi,
                         int n_a, double d_lo, double d_hi, int n_d, int smooth, int64_t* hist_dev, int32_t* es_dev, void* work_dev,
                         size_t work_bytes, void* stream) {
  using namespace glowk_duet;
  const std::string me("duet_histogram");
  if (nsig < 0 || nsig > MAX_SIG) return fail(me + ": nsig must be in [0, 65535]");
  if (cells < 1 || cells > (int64_t)MAX_ROWS * MAX_FRAMES) return fail(me + ": cells must be in [1, 2^27]");
  if ((int64_t)nsig * cells > (int64_t)INT32_MAX) return fail(me + ": nsig * cells must be at most 2^31 - 1");
  if (int rc = duet_grid(me, a_lo, a_hi, n_a, d_lo, d_hi, n_d)) return rc;
  if (int rc = duet_smooth(me, smooth)) return rc;
  if (nsig == 0) return 0;
  if (!alpha_dev || !delta_dev || !w_dev || !hist_dev || !es_dev || !work_dev) return fail("null tensor");
  const HistPlan pl = hist_plan(nsig, cells, n_a, n_d);
  if (work_bytes < pl.bytes) return fail(me + ": work_bytes is smaller than glowk_duet_hist_workspace_bytes says");
  if ((uintptr_t)alpha_dev % 8 || (uintptr_t)delta_dev % 8 || (uintptr_t)w_dev % 8 || (uintptr_t)hist_dev % 8 || (uintptr_t)work_dev % 8 || (uintptr_t)es_dev % 4)
    return fail(me + ": the tensors must be aligned to 8 bytes (es_dev to 4)");
  const size_t nf = (size_t)nsig * cells * 8, nh = (size_t)nsig * n_a * n_d * 8, ne = (size_t)nsig * 8;
  const void* ins[3] = {alpha_dev, delta_dev, w_dev};
  for (int i = 0; i < 3; ++i)
    if (bytes_overlap(ins[i], nf, hist_dev, nh) || bytes_overlap(ins[i], nf, es_dev, ne) || bytes_overlap(ins[i], nf, work_dev, pl.bytes))
      return fail(me + ": hist_dev, es_dev and work_dev must not overlap the features");
  if (bytes_overlap(hist_dev, nh, es_dev, ne) || bytes_overlap(hist_dev, nh, work_dev, pl.bytes) || bytes_overlap(es_dev, ne, work_dev, pl.bytes))
    return fail(me + ": hist_dev, es_dev and work_dev must not overlap");
  int dev;
  if (int rc = audio_device({alpha_dev, delta_dev, w_dev, hist_dev, es_dev, work_dev}, &dev, "duet_histogram")) return rc;
  DeviceGuard dg(dev);
  const Ranges rg = {a_lo, a_hi, d_lo, d_hi, n_a, n_d};
  return duet_hist_launch(nullptr, alpha_dev, delta_dev, w_dev, nsig, cells, 1, 1, 1.0, 0.0, rg, smooth, hist_dev, es_dev, work_dev, (hipStream_t)stream);
}

int glowk_duet_histogram_stft(const float* x_dev, int nsig, int rows, int frames, double p, double q, double a_lo, double a_hi, int n_a, double d_lo,
                              double d_hi, int n_d, int smooth, int64_t* hist_dev, int32_t* es_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_duet;
  const std::string me("duet_histogram_stft");
  if (int rc = duet_shape(me, nsig, rows, frames)) return rc;
  if (int rc = duet_exponents(me, p, q)) return rc;
  if (int rc = duet_grid(me, a_lo, a_hi, n_a, d_lo, d_hi, n_d)) return rc;
  if (int rc = duet_smooth(me, smooth)) return rc;
  if (nsig == 0) return 0;
  if (!x_dev || !hist_dev || !es_dev || !work_dev) return fail("null tensor");
  const int64_t cells = (int64_t)rows * frames;
  const HistPlan pl = hist_plan(nsig, cells, n_a, n_d);
  if (work_bytes < pl.bytes) return fail(me + ": work_bytes is smaller than glowk_duet_hist_workspace_bytes says");
  if ((uintptr_t)x_dev % 8 || (uintptr_t)hist_dev % 8 || (uintptr_t)work_dev % 8 || (uintptr_t)es_dev % 4)
    return fail(me + ": the tensors must be aligned to 8 bytes (es_dev to 4)");
  const size_t nx = (size_t)nsig * cells * 16, nh = (size_t)nsig * n_a * n_d * 8, ne = (size_t)nsig * 8;
  if (bytes_overlap(x_dev, nx, hist_dev, nh) || bytes_overlap(x_dev, nx, es_dev, ne) || bytes_overlap(x_dev, nx, work_dev, pl.bytes))
    return fail(me + ": hist_dev, es_dev and work_dev must not overlap x_dev");
  if (bytes_overlap(hist_dev, nh, es_dev, ne) || bytes_overlap(hist_dev, nh, work_dev, pl.bytes) || bytes_overlap(es_dev, ne, work_dev, pl.bytes))
    return fail(me + ": hist_dev, es_dev and work_dev must not overlap");
  int dev;
  if (int rc = audio_device({x_dev, hist_dev, es_dev, work_dev}, &dev, "duet_histogram_stft")) return rc;
  DeviceGuard dg(dev);
  const Ranges rg = {a_lo, a_hi, d_lo, d_hi, n_a, n_d};
  return duet_hist_launch(x_dev, nullptr, nullptr, nullptr, nsig, cells, rows, frames, p, q, rg, smooth, hist_dev, es_dev, work_dev, (hipStream_t)stream);
}

size_t glowk_duet_peaks_workspace_bytes(int nsig, int n_a, int n_d) {
  using namespace glowk_duet;
  if (nsig < 1 || nsig > MAX_SIG || n_a < 1 || n_d < 1 || (int64_t)n_a * n_d > MAX_BINS) return 0;
  return peaks_bytes(nsig, n_a, n_d);
}

int glowk_duet_peaks(const int64_t* hist_dev, int nsig, int n_a, int n_d, int smooth, int num_sources, int dist_a, int dist_d, int64_t* smooth_dev,
                     int32_t* peaks_dev, int32_t* nfound_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_duet;
  const std::string me("duet_peaks");
  if (nsig < 0 || nsig > MAX_SIG) return fail(me + ": nsig must be in [0, 65535]");
  if (int rc = duet_bins(me, n_a, n_d)) return rc;
  if (int rc = duet_smooth(me, smooth)) return rc;
  if (num_sources < 1 || num_sources > MAX_SRC) return fail(me + ": num_sources must be in [1, 16]");
  if (dist_a < 0 || dist_d < 0) return fail(me + ": min_distance must not be negative");
  if (nsig == 0) return 0;
  if (!hist_dev || !peaks_dev || !nfound_dev || !work_dev) return fail("null tensor");
  const size_t need = peaks_bytes(nsig, n_a, n_d), nh = need / 2, np = (size_t)nsig * num_sources * 8, nn = (size_t)nsig * 4;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_duet_peaks_workspace_bytes says");
  if ((uintptr_t)hist_dev % 8 || (uintptr_t)smooth_dev % 8 || (uintptr_t)work_dev % 8 || (uintptr_t)peaks_dev % 4 || (uintptr_t)nfound_dev % 4)
    return fail(me + ": the planes and work_dev must be aligned to 8 bytes, the peaks to 4");
  const void* outs[4] = {smooth_dev, peaks_dev, nfound_dev, work_dev};
  const size_t sizes[4] = {nh, np, nn, need};
  for (int i = 0; i < 4; ++i) {
    if (!outs[i]) continue;
    if (bytes_overlap(hist_dev, nh, outs[i], sizes[i])) return fail(me + ": the outputs and work_dev must not overlap hist_dev");
    for (int j = i + 1; j < 4; ++j)
      if (outs[j] && bytes_overlap(outs[i], sizes[i], outs[j], sizes[j])) return fail(me + ": the outputs and work_dev must not overlap each other");
  }
  int dev;
  if (int rc = audio_device({hist_dev, smooth_dev, peaks_dev, nfound_dev, work_dev}, &dev, "duet_peaks")) return rc;
  DeviceGuard dg(dev);
  hipLaunchKernelGGL(k_duet_peaks, dim3((unsigned)nsig), dim3(PEAK_THREADS), 0, (hipStream_t)stream, (const long long*)hist_dev, n_a, n_d, smooth, num_sources,
                     dist_a, dist_d, (long long*)work_dev, (long long*)smooth_dev, peaks_dev, nfound_dev);
  LAUNCHCHK("k_duet_peaks");
  return 0;
}

size_t glowk_duet_assign_workspace_bytes(int nsig, int rows, int num_sources) {
  using namespace glowk_duet;
  if (nsig < 1 || nsig > MAX_SIG || rows < 1 || rows > MAX_ROWS || num_sources < 1 || num_sources > MAX_SRC) return 0;
  return assign_bytes(nsig, num_sources, rows);
}

int glowk_duet_assign(const float* x_dev, int nsig, int rows, int frames, const int32_t* peaks_dev, const int32_t* nfound_dev, int num_sources,
                      double a_lo, double a_hi, int n_a, double d_lo, double d_hi, int n_d, float* mask_dev, float* spec_dev, void* work_dev,
                      size_t work_bytes, void* stream) {
  using namespace glowk_duet;
  const std::string me("duet_assign");
  if (int rc = duet_shape(me, nsig, rows, frames)) return rc;
  if (int rc = duet_grid(me, a_lo, a_hi, n_a, d_lo, d_hi, n_d)) return rc;
  if (num_sources < 1 || num_sources > MAX_SRC) return fail(me + ": num_sources must be in [1, 16]");
  if (nsig == 0) return 0;
  if (!x_dev || !peaks_dev || !nfound_dev || !mask_dev || !spec_dev || !work_dev) return fail("null tensor");
  const int64_t cells = (int64_t)rows * frames, total = (int64_t)nsig * cells;
  const size_t need = assign_bytes(nsig, num_sources, rows);
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_duet_assign_workspace_bytes says");
  if ((uintptr_t)x_dev % 8 || (uintptr_t)spec_dev % 8 || (uintptr_t)work_dev % 16 || (uintptr_t)mask_dev % 4 || (uintptr_t)peaks_dev % 4 || (uintptr_t)nfound_dev % 4)
    return fail(me + ": x_dev and spec_dev must be aligned to 8 bytes, work_dev to 16, the others to 4");
  const size_t nx = (size_t)total * 16, nm = (size_t)total * num_sources * 4, ns = (size_t)total * num_sources * 16,
               np = (size_t)nsig * num_sources * 8, nn = (size_t)nsig * 4;
  const void* ins[3] = {x_dev, peaks_dev, nfound_dev};
  const size_t in_sizes[3] = {nx, np, nn};
  const void* outs[3] = {mask_dev, spec_dev, work_dev};
  const size_t out_sizes[3] = {nm, ns, need};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      if (bytes_overlap(ins[j], in_sizes[j], outs[i], out_sizes[i])) return fail(me + ": mask_dev, spec_dev and work_dev must not overlap the inputs");
    for (int j = i + 1; j < 3; ++j)
      if (bytes_overlap(outs[i], out_sizes[i], outs[j], out_sizes[j])) return fail(me + ": mask_dev, spec_dev and work_dev must not overlap each other");
  }
  int dev;
  if (int rc = audio_device({x_dev, peaks_dev, nfound_dev, mask_dev, spec_dev, work_dev}, &dev, "duet_assign")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  const Ranges rg = {a_lo, a_hi, d_lo, d_hi, n_a, n_d};
  const int64_t entries = (int64_t)nsig * num_sources * rows;
  hipLaunchKernelGGL(k_duet_table, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, peaks_dev, nfound_dev, entries, num_sources, rows, rg,
                     (double*)work_dev);
  LAUNCHCHK("k_duet_table");
  hipLaunchKernelGGL(k_duet_assign, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float2*)x_dev, total, rows, frames, nfound_dev, num_sources,
                     (const double*)work_dev, mask_dev, (float2*)spec_dev);
  LAUNCHCHK("k_duet_assign");
  return 0;
}

// ---- NMF: multiplicative updates, divergence, masks of component ranges (glowk_nmf.h) ---------------------------------------------------
namespace {
// the ranges every glowk_nmf_* call shares; 0 or an error
int nmf_ranges(const std::string& w, int nsig, int rows, int frames, int K) {
  using namespace glowk_nmf;
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (rows < 1 || rows > MAX_ROWS) return fail(w + ": rows must be in [1, 4096]");
  if (frames < 1 || frames > MAX_FRAMES) return fail(w + ": frames must be in [1, 32768]");
  if (K < 1 || K > MAX_K) return fail(w + ": K must be in [1, 128]");
  if ((int64_t)nsig * rows * frames > (int64_t)INT32_MAX) return fail(w + ": nsig * rows * frames must be at most 2^31 - 1");
  if ((int64_t)nsig * K * frames > (int64_t)INT32_MAX) return fail(w + ": nsig * K * frames must be at most 2^31 - 1");
  if ((int64_t)nsig * rows * K > (int64_t)INT32_MAX) return fail(w + ": nsig * rows * K must be at most 2^31 - 1");
  const NmfPlan p = nmf_plan(rows, frames, K);
  if ((int64_t)nsig * p.rtiles * p.nch > (int64_t)INT32_MAX || (int64_t)nsig * p.ftiles > (int64_t)INT32_MAX)
    return fail(w + ": the workgroup count must be at most 2^31 - 1");
  return 0;
}
int nmf_model(const std::string& w, int nsig, int nw, int beta) {
  if (nw != 1 && nw != nsig) return fail(w + ": nw must be 1 (one shared dictionary) or nsig");
  if (beta < 0 || beta > 2) return fail(w + ": beta must be 0 (Itakura-Saito), 1 (Kullback-Leibler) or 2 (Euclidean)");
  return 0;
}

#define GLOWK_NMF_EACH_KT(X) X(1) X(2) X(3) X(4)
}  // namespace

size_t glowk_nmf_workspace_bytes(int nsig, int rows, int frames, int K) {
  if (nmf_ranges("nmf_workspace_bytes", nsig, rows, frames, K)) return 0;
  return glowk_nmf::nmf_work_bytes(nsig, rows, frames, K);
}

int glowk_nmf_fit(const float* v_dev, int nsig, int rows, int frames, float* w_dev, int nw, float* h_dev, int K, int beta, int n_iter, int update_w,
                  void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_nmf;
  const std::string me("nmf_fit");
  if (int rc = nmf_ranges(me, nsig, rows, frames, K)) return rc;
  if (int rc = nmf_model(me, nsig, nw, beta)) return rc;
  if (n_iter < 0 || n_iter > MAX_ITER) return fail(me + ": n_iter must be in [0, 100000]");
  if (update_w < 0 || update_w > 2) return fail(me + ": update_w must be 0 (H alone), 1 (W, then H) or 2 (W alone)");
  if (update_w && nw != nsig) return fail(me + ": a dictionary shared by several signals cannot be updated (nw = 1 needs update_w = 0)");
  if (nsig == 0 || n_iter == 0) return 0;
  if (!v_dev || !w_dev || !h_dev || (update_w && !work_dev)) return fail("null tensor");
  const NmfPlan p = nmf_plan(rows, frames, K);
  const size_t need = update_w ? (size_t)nsig * (size_t)nmf_w_part_floats(p, rows, K) * 4 : 0;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_nmf_workspace_bytes says");
  if ((uintptr_t)work_dev % 8) return fail(me + ": work_dev must be aligned to 8 bytes");
  const size_t nv = (size_t)nsig * rows * frames * 4, nww = (size_t)nw * rows * K * 4, nh = (size_t)nsig * K * frames * 4;
  if (bytes_overlap(v_dev, nv, w_dev, nww) || bytes_overlap(v_dev, nv, h_dev, nh) || bytes_overlap(w_dev, nww, h_dev, nh))
    return fail(me + ": V, W and H must not overlap");
  if (need && (bytes_overlap(work_dev, need, v_dev, nv) || bytes_overlap(work_dev, need, w_dev, nww) || bytes_overlap(work_dev, need, h_dev, nh)))
    return fail(me + ": work_dev must not overlap the tensors");
  int dev;
  if (int rc = audio_device({v_dev, w_dev, h_dev, work_dev}, &dev, "nmf_fit")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)work_dev;
  const int64_t wstride = nw == 1 ? 0 : (int64_t)rows * K, per_sig = (int64_t)rows * K, total = (int64_t)nsig * per_sig;
  const dim3 gw((unsigned)((int64_t)nsig * p.rtiles * p.nch)), gh((unsigned)((int64_t)nsig * p.ftiles)), gf((unsigned)((total + 255) / 256));
  for (int it = 0; it < n_iter; ++it) {
    if (update_w) {
      switch (p.kt) {
#define GLOWK_CASE(n) \
  case n: hipLaunchKernelGGL(k_nmf_update_w<n>, gw, dim3(256), 0, st, v_dev, (const float*)w_dev, (const float*)h_dev, rows, frames, K, p, beta, part); break;
        GLOWK_NMF_EACH_KT(GLOWK_CASE)
#undef GLOWK_CASE
      }
      LAUNCHCHK("k_nmf_update_w");
      hipLaunchKernelGGL(k_nmf_w_finish, gf, dim3(256), 0, st, (const float*)part, total, per_sig, nmf_w_part_floats(p, rows, K), p.nch, beta, w_dev);
      LAUNCHCHK("k_nmf_w_finish");
    }
    if (update_w != 2) {
      switch (p.kt) {
#define GLOWK_CASE(n) \
  case n: hipLaunchKernelGGL(k_nmf_update_h<n>, gh, dim3(256), 0, st, v_dev, (const float*)w_dev, wstride, h_dev, rows, frames, K, p.ftiles, beta); break;
        GLOWK_NMF_EACH_KT(GLOWK_CASE)
#undef GLOWK_CASE
      }
      LAUNCHCHK("k_nmf_update_h");
    }
  }
  return 0;
}

int glowk_nmf_divergence(const float* v_dev, int nsig, int rows, int frames, const float* w_dev, int nw, const float* h_dev, int K, int beta,
                         double* out_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_nmf;
  const std::string me("nmf_divergence");
  if (int rc = nmf_ranges(me, nsig, rows, frames, K)) return rc;
  if (int rc = nmf_model(me, nsig, nw, beta)) return rc;
  if (nsig == 0) return 0;
  if (!v_dev || !w_dev || !h_dev || !out_dev || !work_dev) return fail("null tensor");
  const NmfPlan p = nmf_plan(rows, frames, K);
  const size_t need = (size_t)nsig * (size_t)nmf_div_parts(p) * 8;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_nmf_workspace_bytes says");
  if ((uintptr_t)work_dev % 8 || (uintptr_t)out_dev % 8) return fail(me + ": work_dev and out_dev must be aligned to 8 bytes");
  const size_t nv = (size_t)nsig * rows * frames * 4, nww = (size_t)nw * rows * K * 4, nh = (size_t)nsig * K * frames * 4, no = (size_t)nsig * 8;
  const void* ins[3] = {v_dev, w_dev, h_dev};
  const size_t in_sizes[3] = {nv, nww, nh};
  for (int i = 0; i < 3; ++i)
    if (bytes_overlap(ins[i], in_sizes[i], out_dev, no) || bytes_overlap(ins[i], in_sizes[i], work_dev, need))
      return fail(me + ": out_dev and work_dev must not overlap the inputs");
  if (bytes_overlap(out_dev, no, work_dev, need)) return fail(me + ": out_dev and work_dev must not overlap");
  int dev;
  if (int rc = audio_device({v_dev, w_dev, h_dev, out_dev, work_dev}, &dev, "nmf_divergence")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_nmf_divergence, dim3((unsigned)((int64_t)nsig * p.rtiles * p.nch)), dim3(256), 0, st, v_dev, w_dev, nw == 1 ? (int64_t)0 : (int64_t)rows * K,
                     h_dev, rows, frames, K, p, beta, (double*)work_dev);
  LAUNCHCHK("k_nmf_divergence");
  hipLaunchKernelGGL(k_nmf_div_reduce, dim3((unsigned)nsig), dim3(64), 0, st, (const double*)work_dev, nmf_div_parts(p), out_dev);
  LAUNCHCHK("k_nmf_div_reduce");
  return 0;
}

int glowk_nmf_masks(const float* w_dev, int nw, const float* h_dev, int nsig, int rows, int frames, int K, const int32_t* bounds_host, int num_sources,
                    int power, const float* x_dev, int channels, float* mask_dev, float* spec_dev, void* stream) {
  using namespace glowk_nmf;
  const std::string me("nmf_masks");
  if (int rc = nmf_ranges(me, nsig, rows, frames, K)) return rc;
  if (nw != 1 && nw != nsig) return fail(me + ": nw must be 1 (one shared dictionary) or nsig");
  if (num_sources < 1 || num_sources > MAX_SRC) return fail(me + ": the number of sources must be in [1, 16]");
  if (power != 1 && power != 2) return fail(me + ": power must be 1 or 2");
  if (!bounds_host) return fail(me + ": bounds_host is null");
  NmfBounds bd;
  for (int s = 0; s <= MAX_SRC; ++s) bd.b[s] = s <= num_sources ? bounds_host[s] : K;
  if (bd.b[0] != 0 || bd.b[num_sources] != K) return fail(me + ": bounds must start at 0 and end at K");
  for (int s = 0; s < num_sources; ++s)
    if (bd.b[s] >= bd.b[s + 1]) return fail(me + ": bounds must increase strictly (every source owns at least one component)");
  if ((x_dev == nullptr) != (spec_dev == nullptr)) return fail(me + ": x_dev and spec_dev are given together or not at all");
  if (x_dev && channels != 1 && channels != 2) return fail(me + ": the channel count must be 1 or 2");
  const int C = x_dev ? channels : 0;
  const int64_t cells = (int64_t)nsig * rows * frames;
  if (cells * num_sources * (C ? C : 1) > (int64_t)INT32_MAX) return fail(me + ": nsig * S * C * rows * frames must be at most 2^31 - 1");
  if (nsig == 0) return 0;
  if (!w_dev || !h_dev || !mask_dev) return fail("null tensor");
  if ((uintptr_t)x_dev % 8 || (uintptr_t)spec_dev % 8) return fail(me + ": x_dev and spec_dev must be aligned to 8 bytes");
  const size_t nww = (size_t)nw * rows * K * 4, nh = (size_t)nsig * K * frames * 4, nx = (size_t)cells * C * 8,
               nm = (size_t)cells * num_sources * 4, ns = (size_t)cells * num_sources * C * 8;
  const void* ins[3] = {w_dev, h_dev, x_dev};
  const size_t in_sizes[3] = {nww, nh, nx};
  for (int i = 0; i < 3; ++i) {
    if (!ins[i]) continue;
    if (bytes_overlap(ins[i], in_sizes[i], mask_dev, nm) || (spec_dev && bytes_overlap(ins[i], in_sizes[i], spec_dev, ns)))
      return fail(me + ": mask_dev and spec_dev must not overlap the inputs");
  }
  if (spec_dev && bytes_overlap(mask_dev, nm, spec_dev, ns)) return fail(me + ": mask_dev and spec_dev must not overlap");
  int dev;
  if (int rc = audio_device({w_dev, h_dev, x_dev, mask_dev, spec_dev}, &dev, "nmf_masks")) return rc;
  DeviceGuard dg(dev);
  const NmfPlan p = nmf_plan(rows, frames, K);
  const int fgroups = (p.ftiles + WAVES - 1) / WAVES;
  if ((int64_t)nsig * p.rtiles * fgroups > (int64_t)INT32_MAX) return fail(me + ": the workgroup count must be at most 2^31 - 1");
  hipLaunchKernelGGL(k_nmf_masks, dim3((unsigned)((int64_t)nsig * p.rtiles * fgroups)), dim3(256), 0, (hipStream_t)stream, w_dev,
                     nw == 1 ? (int64_t)0 : (int64_t)rows * K, h_dev, rows, frames, K, p.rtiles, fgroups, bd, num_sources, power, (const float2*)x_dev, C, mask_dev,
                     (float2*)spec_dev);
  LAUNCHCHK("k_nmf_masks");
  return 0;
}

// ---- AuxIVA and ILRMA: blind separation by one demixing matrix per row (glowk_iva.h) ---------------------------------------------------
namespace {
struct IvaBuf {
  const void* p;
  size_t n;
};
// 0 when no written buffer overlaps another buffer of the call (the first `nout` entries are written), null entries skipped
int iva_disjoint(const std::string& w, std::initializer_list<IvaBuf> bufs, size_t nout) {
  size_t i = 0;
  for (const IvaBuf& a : bufs) {
    size_t j = 0;
    for (const IvaBuf& b : bufs) {
      if (j > i && i < nout && a.p && b.p && a.n && b.n && bytes_overlap(a.p, a.n, b.p, b.n)) return fail(w + ": a tensor the call writes overlaps another of its tensors");
      ++j;
    }
    ++i;
  }
  return 0;
}
int iva_ranges(const std::string& w, int nsig, int M, int rows, int frames) {
  using namespace glowk_iva;
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (M < 2 || M > MAX_M) return fail(w + ": the channel count M must be in [2, 4]");
  if (rows < 1 || rows > MAX_ROWS) return fail(w + ": rows must be in [1, 4096]");
  if (frames < M || frames > MAX_FRAMES) return fail(w + ": frames must be in [M, 32768] (fewer frames than channels leave the covariances rank-deficient)");
  if ((int64_t)nsig * M * rows * frames > (int64_t)INT32_MAX) return fail(w + ": nsig * M * rows * frames must be at most 2^31 - 1");
  return 0;
}
int iva_rows_only(const std::string& w, int nsig, int M, int rows) {
  using namespace glowk_iva;
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (M < 2 || M > MAX_M) return fail(w + ": the channel count M must be in [2, 4]");
  if (rows < 1 || rows > MAX_ROWS) return fail(w + ": rows must be in [1, 4096]");
  return 0;
}
int iva_factors(const std::string& w, int nsig, int M, int rows, int frames, int K) {
  using namespace glowk_iva;
  if (K < 1 || K > MAX_K) return fail(w + ": K must be in [1, 128]");
  if ((int64_t)nsig * M > MAX_SIG) return fail(w + ": nsig * M must be at most 65535 (the factors are a batch of nsig * M spectrograms)");
  if ((int64_t)nsig * M * rows * K > (int64_t)INT32_MAX || (int64_t)nsig * M * K * frames > (int64_t)INT32_MAX)
    return fail(w + ": the factors must have at most 2^31 - 1 elements each");
  return 0;
}
int iva_aligned(const std::string& w, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if ((uintptr_t)p % 8) return fail(w + ": the tensors must be aligned to 8 bytes");
  return 0;
}
size_t iva_bytes_x(int nsig, int M, int rows, int frames) { return (size_t)nsig * M * rows * frames * 8; }
size_t iva_bytes_w(int nsig, int M, int rows) { return (size_t)nsig * rows * M * M * 16; }
// work_dev of the AuxIVA calls: the partial norms, phi [nsig][M][frames], lambda [nsig][M]; all doubles
size_t iva_work_doubles(int nsig, int M, int rows, int frames) {
  return glowk_iva::partial_doubles(nsig, M, rows, frames) + (size_t)nsig * M * frames + (size_t)nsig * M;
}

#define GLOWK_IVA_EACH_M(X) X(2) X(3) X(4)

int iva_launch_norms(const float* x, const double* w, int nsig, int M, int rows, int frames, double* partial, hipStream_t st) {
  using namespace glowk_iva;
  const RowPlan rp = row_plan(rows);
  const dim3 grid((unsigned)((int64_t)nsig * rp.nrb * frame_chunks(frames)));
  switch (M) {
#define GLOWK_CASE(m) case m: hipLaunchKernelGGL(k_iva_norms<m>, grid, dim3(THREADS), 0, st, (const float2*)x, w, rows, frames, rp, partial); break;
    GLOWK_IVA_EACH_M(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_iva_norms");
  return 0;
}
int iva_launch_phi(const double* partial, int nsig, int M, int rows, int frames, int model, double* phi, hipStream_t st) {
  using namespace glowk_iva;
  const int64_t total = (int64_t)nsig * M * frames;
  hipLaunchKernelGGL(k_iva_phi, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, partial, total, M, rows, frames, row_plan(rows).nrb, model, phi);
  LAUNCHCHK("k_iva_phi");
  return 0;
}
// the covariances with phi (cw.phi) or the factors, followed by the row updates of w (v_out null) or stored to v_out (w null)
int iva_launch_cov(const float* x, const glowk_iva::CovWeights& cw, int nsig, int M, int rows, int frames, double* w, double* v_out, hipStream_t st) {
  using namespace glowk_iva;
  const dim3 grid((unsigned)((int64_t)nsig * rows)), block(THREADS);
  const float2* xc = (const float2*)x;
  const int form = (cw.phi ? 0 : 2) + (v_out ? 0 : 1);
  switch (M * 4 + form) {
#define GLOWK_CASE(m)                                                                                                    \
  case m * 4 + 0: hipLaunchKernelGGL((k_iva_cov<m, 0, false>), grid, block, 0, st, xc, cw, rows, frames, w, v_out); break; \
  case m * 4 + 1: hipLaunchKernelGGL((k_iva_cov<m, 0, true>), grid, block, 0, st, xc, cw, rows, frames, w, v_out); break;  \
  case m * 4 + 2: hipLaunchKernelGGL((k_iva_cov<m, 1, false>), grid, block, 0, st, xc, cw, rows, frames, w, v_out); break; \
  case m * 4 + 3: hipLaunchKernelGGL((k_iva_cov<m, 1, true>), grid, block, 0, st, xc, cw, rows, frames, w, v_out); break;
    GLOWK_IVA_EACH_M(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_iva_cov");
  return 0;
}
int iva_launch_power(const float* x, const double* w, int nsig, int M, int rows, int frames, float* P, hipStream_t st) {
  using namespace glowk_iva;
  const dim3 grid((unsigned)((int64_t)nsig * rows * frame_chunks(frames)));
  switch (M) {
#define GLOWK_CASE(m) case m: hipLaunchKernelGGL(k_iva_power<m>, grid, dim3(THREADS), 0, st, (const float2*)x, w, rows, frames, P); break;
    GLOWK_IVA_EACH_M(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_iva_power");
  return 0;
}
// lambda from the refreshed y, then W's rows and the basis scaled: four launches
int iva_launch_normalize(const float* x, double* w, float* basis, int nsig, int M, int rows, int frames, int K, double* work, hipStream_t st) {
  using namespace glowk_iva;
  double* partial = work;
  double* r = work + partial_doubles(nsig, M, rows, frames);
  double* lam = r + (size_t)nsig * M * frames;
  if (int rc = iva_launch_norms(x, w, nsig, M, rows, frames, partial, st)) return rc;
  if (int rc = iva_launch_phi(partial, nsig, M, rows, frames, MODEL_SUM, r, st)) return rc;
  hipLaunchKernelGGL(k_iva_lambda, dim3((unsigned)(nsig * M)), dim3(THREADS), 0, st, (const double*)r, rows, frames, lam);
  LAUNCHCHK("k_iva_lambda");
  const int64_t nw = (int64_t)nsig * rows * M * M, nb = (int64_t)nsig * M * rows * K;
  hipLaunchKernelGGL(k_iva_scale, dim3((unsigned)((nw + nb + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, (const double*)lam, nw, nb, M, rows, K, w, basis);
  LAUNCHCHK("k_iva_scale");
  return 0;
}
int iva_launch_demix(const float* x, const double* w, const double* winv, int nsig, int M, int rows, int frames, float* y, float* img, hipStream_t st) {
  using namespace glowk_iva;
  const dim3 grid((unsigned)((int64_t)nsig * rows * frame_chunks(frames)));
  switch (M) {
#define GLOWK_CASE(m) \
  case m: hipLaunchKernelGGL(k_iva_demix<m>, grid, dim3(THREADS), 0, st, (const float2*)x, w, winv, rows, frames, (float2*)y, (float2*)img); break;
    GLOWK_IVA_EACH_M(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_iva_demix");
  return 0;
}
}  // namespace

size_t glowk_iva_workspace_bytes(int nsig, int M, int rows, int frames) {
  if (iva_ranges("iva_workspace_bytes", nsig, M, rows, frames)) return 0;
  return iva_work_doubles(nsig, M, rows, frames) * 8;
}

size_t glowk_ilrma_workspace_bytes(int nsig, int M, int rows, int frames, int K) {
  if (iva_ranges("ilrma_workspace_bytes", nsig, M, rows, frames) || iva_factors("ilrma_workspace_bytes", nsig, M, rows, frames, K)) return 0;
  if (nmf_ranges("ilrma_workspace_bytes", nsig * M, rows, frames, K)) return 0;
  const size_t p = ((size_t)nsig * M * rows * frames * 4 + 7) / 8 * 8;
  return iva_work_doubles(nsig, M, rows, frames) * 8 + p + (glowk_nmf::nmf_work_bytes(nsig * M, rows, frames, K) + 7) / 8 * 8;
}

int glowk_iva_weights(const float* x_dev, const double* w_dev, int nsig, int M, int rows, int frames, int model, double* phi_dev, void* work_dev,
                      size_t work_bytes, void* stream) {
  const std::string me("iva_weights");
  if (int rc = iva_ranges(me, nsig, M, rows, frames)) return rc;
  if (model != glowk_iva::MODEL_LAPLACE && model != glowk_iva::MODEL_GAUSS) return fail(me + ": model must be 0 (laplace) or 1 (gauss)");
  if (nsig == 0) return 0;
  if (!x_dev || !w_dev || !phi_dev || !work_dev) return fail("null tensor");
  const size_t need = iva_work_doubles(nsig, M, rows, frames) * 8;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_iva_workspace_bytes says");
  if (int rc = iva_aligned(me, {x_dev, w_dev, phi_dev, work_dev})) return rc;
  if (int rc = iva_disjoint(me, {{phi_dev, (size_t)nsig * M * frames * 8}, {work_dev, need}, {x_dev, iva_bytes_x(nsig, M, rows, frames)}, {w_dev, iva_bytes_w(nsig, M, rows)}}, 2))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, w_dev, phi_dev, work_dev}, &dev, "iva_weights")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = iva_launch_norms(x_dev, w_dev, nsig, M, rows, frames, (double*)work_dev, st)) return rc;
  return iva_launch_phi((const double*)work_dev, nsig, M, rows, frames, model, phi_dev, st);
}

int glowk_iva_covariances(const float* x_dev, int nsig, int M, int rows, int frames, const double* phi_dev, const float* basis_dev, const float* act_dev,
                          int K, double* v_dev, void* stream) {
  const std::string me("iva_covariances");
  if (int rc = iva_ranges(me, nsig, M, rows, frames)) return rc;
  if ((phi_dev != nullptr) == (basis_dev != nullptr || act_dev != nullptr)) return fail(me + ": give either phi_dev or both factors");
  if (!phi_dev && (!basis_dev || !act_dev)) return fail(me + ": the factors are given together");
  if (!phi_dev)
    if (int rc = iva_factors(me, nsig, M, rows, frames, K)) return rc;
  if (nsig == 0) return 0;
  if (!x_dev || !v_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {x_dev, phi_dev, v_dev})) return rc;
  if ((uintptr_t)basis_dev % 4 || (uintptr_t)act_dev % 4) return fail(me + ": the factors must be aligned to 4 bytes");
  const size_t nv = iva_bytes_w(nsig, M, rows) * M;
  if (int rc = iva_disjoint(me, {{v_dev, nv}, {x_dev, iva_bytes_x(nsig, M, rows, frames)}, {phi_dev, (size_t)nsig * M * frames * 8},
                                 {basis_dev, phi_dev ? 0 : (size_t)nsig * M * rows * K * 4}, {act_dev, phi_dev ? 0 : (size_t)nsig * M * K * frames * 4}}, 1))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, phi_dev, basis_dev, act_dev, v_dev}, &dev, "iva_covariances")) return rc;
  DeviceGuard dg(dev);
  const glowk_iva::CovWeights cw = {phi_dev, basis_dev, act_dev, phi_dev ? 0 : K};
  return iva_launch_cov(x_dev, cw, nsig, M, rows, frames, nullptr, v_dev, (hipStream_t)stream);
}

int glowk_iva_ip_update(double* w_dev, const double* v_dev, int nsig, int M, int rows, void* stream) {
  using namespace glowk_iva;
  const std::string me("iva_ip_update");
  if (int rc = iva_rows_only(me, nsig, M, rows)) return rc;
  if (nsig == 0) return 0;
  if (!w_dev || !v_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {w_dev, v_dev})) return rc;
  if (int rc = iva_disjoint(me, {{w_dev, iva_bytes_w(nsig, M, rows)}, {v_dev, iva_bytes_w(nsig, M, rows) * M}}, 1)) return rc;
  int dev;
  if (int rc = audio_device({w_dev, v_dev}, &dev, "iva_ip_update")) return rc;
  DeviceGuard dg(dev);
  const int64_t total = (int64_t)nsig * rows;
  const dim3 grid((unsigned)((total + 63) / 64));
  switch (M) {
#define GLOWK_CASE(m) case m: hipLaunchKernelGGL(k_iva_ip<m>, grid, dim3(64), 0, (hipStream_t)stream, w_dev, v_dev, total); break;
    GLOWK_IVA_EACH_M(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_iva_ip");
  return 0;
}

int glowk_auxiva_fit(const float* x_dev, double* w_dev, int nsig, int M, int rows, int frames, int model, int n_iter, void* work_dev, size_t work_bytes,
                     void* stream) {
  using namespace glowk_iva;
  const std::string me("auxiva_fit");
  if (int rc = iva_ranges(me, nsig, M, rows, frames)) return rc;
  if (model != MODEL_LAPLACE && model != MODEL_GAUSS) return fail(me + ": model must be 0 (laplace) or 1 (gauss)");
  if (n_iter < 0 || n_iter > 100000) return fail(me + ": n_iter must be in [0, 100000]");
  if (nsig == 0 || n_iter == 0) return 0;
  if (!x_dev || !w_dev || !work_dev) return fail("null tensor");
  const size_t need = iva_work_doubles(nsig, M, rows, frames) * 8;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_iva_workspace_bytes says");
  if (int rc = iva_aligned(me, {x_dev, w_dev, work_dev})) return rc;
  if (int rc = iva_disjoint(me, {{w_dev, iva_bytes_w(nsig, M, rows)}, {work_dev, need}, {x_dev, iva_bytes_x(nsig, M, rows, frames)}}, 2)) return rc;
  int dev;
  if (int rc = audio_device({x_dev, w_dev, work_dev}, &dev, "auxiva_fit")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)work_dev;
  double* phi = partial + partial_doubles(nsig, M, rows, frames);
  const CovWeights cw = {phi, nullptr, nullptr, 0};
  for (int it = 0; it < n_iter; ++it) {
    if (int rc = iva_launch_norms(x_dev, w_dev, nsig, M, rows, frames, partial, st)) return rc;
    if (int rc = iva_launch_phi(partial, nsig, M, rows, frames, model, phi, st)) return rc;
    if (int rc = iva_launch_cov(x_dev, cw, nsig, M, rows, frames, w_dev, nullptr, st)) return rc;
  }
  return 0;
}

int glowk_iva_power(const float* x_dev, const double* w_dev, int nsig, int M, int rows, int frames, float* p_dev, void* stream) {
  const std::string me("iva_power");
  if (int rc = iva_ranges(me, nsig, M, rows, frames)) return rc;
  if (nsig == 0) return 0;
  if (!x_dev || !w_dev || !p_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {x_dev, w_dev})) return rc;
  if ((uintptr_t)p_dev % 4) return fail(me + ": p_dev must be aligned to 4 bytes");
  if (int rc = iva_disjoint(me, {{p_dev, iva_bytes_x(nsig, M, rows, frames) / 2}, {x_dev, iva_bytes_x(nsig, M, rows, frames)}, {w_dev, iva_bytes_w(nsig, M, rows)}}, 1))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, w_dev, p_dev}, &dev, "iva_power")) return rc;
  DeviceGuard dg(dev);
  return iva_launch_power(x_dev, w_dev, nsig, M, rows, frames, p_dev, (hipStream_t)stream);
}

int glowk_iva_normalize(const float* x_dev, double* w_dev, float* basis_dev, int nsig, int M, int rows, int frames, int K, void* work_dev, size_t work_bytes,
                        void* stream) {
  const std::string me("iva_normalize");
  if (int rc = iva_ranges(me, nsig, M, rows, frames)) return rc;
  if (int rc = iva_factors(me, nsig, M, rows, frames, K)) return rc;
  if (nsig == 0) return 0;
  if (!x_dev || !w_dev || !basis_dev || !work_dev) return fail("null tensor");
  const size_t need = iva_work_doubles(nsig, M, rows, frames) * 8;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_iva_workspace_bytes says");
  if (int rc = iva_aligned(me, {x_dev, w_dev, work_dev})) return rc;
  if ((uintptr_t)basis_dev % 4) return fail(me + ": basis_dev must be aligned to 4 bytes");
  if (int rc = iva_disjoint(me, {{w_dev, iva_bytes_w(nsig, M, rows)}, {basis_dev, (size_t)nsig * M * rows * K * 4}, {work_dev, need},
                                 {x_dev, iva_bytes_x(nsig, M, rows, frames)}}, 3))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, w_dev, basis_dev, work_dev}, &dev, "iva_normalize")) return rc;
  DeviceGuard dg(dev);
  return iva_launch_normalize(x_dev, w_dev, basis_dev, nsig, M, rows, frames, K, (double*)work_dev, (hipStream_t)stream);
}

int glowk_ilrma_fit(const float* x_dev, double* w_dev, float* basis_dev, float* act_dev, int nsig, int M, int rows, int frames, int K, int n_iter,
                    void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_iva;
  const std::string me("ilrma_fit");
  if (int rc = iva_ranges(me, nsig, M, rows, frames)) return rc;
  if (int rc = iva_factors(me, nsig, M, rows, frames, K)) return rc;
  if (int rc = nmf_ranges(me, nsig * M, rows, frames, K)) return rc;
  if (n_iter < 0 || n_iter > 100000) return fail(me + ": n_iter must be in [0, 100000]");
  if (nsig == 0 || n_iter == 0) return 0;
  if (!x_dev || !w_dev || !basis_dev || !act_dev || !work_dev) return fail("null tensor");
  const size_t iva_b = iva_work_doubles(nsig, M, rows, frames) * 8, p_b = ((size_t)nsig * M * rows * frames * 4 + 7) / 8 * 8;
  const size_t nmf_b = glowk_nmf::nmf_work_bytes(nsig * M, rows, frames, K), need = iva_b + p_b + (nmf_b + 7) / 8 * 8;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_ilrma_workspace_bytes says");
  if (int rc = iva_aligned(me, {x_dev, w_dev, work_dev})) return rc;
  if ((uintptr_t)basis_dev % 4 || (uintptr_t)act_dev % 4) return fail(me + ": the factors must be aligned to 4 bytes");
  if (int rc = iva_disjoint(me, {{w_dev, iva_bytes_w(nsig, M, rows)}, {basis_dev, (size_t)nsig * M * rows * K * 4}, {act_dev, (size_t)nsig * M * K * frames * 4},
                                 {work_dev, need}, {x_dev, iva_bytes_x(nsig, M, rows, frames)}}, 4))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, w_dev, basis_dev, act_dev, work_dev}, &dev, "ilrma_fit")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  double* work = (double*)work_dev;
  float* P = (float*)((char*)work_dev + iva_b);
  void* nmf_work = (char*)work_dev + iva_b + p_b;
  const CovWeights cw = {nullptr, basis_dev, act_dev, K};
  for (int it = 0; it < n_iter; ++it) {
    if (int rc = iva_launch_power(x_dev, w_dev, nsig, M, rows, frames, P, st)) return rc;
    if (int rc = glowk_nmf_fit(P, nsig * M, rows, frames, basis_dev, nsig * M, act_dev, K, 0, 1, 1, nmf_work, nmf_b, stream)) return rc;
    if (int rc = iva_launch_cov(x_dev, cw, nsig, M, rows, frames, w_dev, nullptr, st)) return rc;
    if (int rc = iva_launch_normalize(x_dev, w_dev, basis_dev, nsig, M, rows, frames, K, work, st)) return rc;
  }
  return 0;
}

int glowk_iva_inverse(const double* w_dev, int nsig, int M, int rows, double* winv_dev, void* stream) {
  using namespace glowk_iva;
  const std::string me("iva_inverse");
  if (int rc = iva_rows_only(me, nsig, M, rows)) return rc;
  if (nsig == 0) return 0;
  if (!w_dev || !winv_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {w_dev, winv_dev})) return rc;
  if (int rc = iva_disjoint(me, {{winv_dev, iva_bytes_w(nsig, M, rows)}, {w_dev, iva_bytes_w(nsig, M, rows)}}, 1)) return rc;
  int dev;
  if (int rc = audio_device({w_dev, winv_dev}, &dev, "iva_inverse")) return rc;
  DeviceGuard dg(dev);
  const int64_t total = (int64_t)nsig * rows;
  const dim3 grid((unsigned)((total + 63) / 64));
  switch (M) {
#define GLOWK_CASE(m) case m: hipLaunchKernelGGL(k_iva_inverse<m>, grid, dim3(64), 0, (hipStream_t)stream, w_dev, total, winv_dev); break;
    GLOWK_IVA_EACH_M(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_iva_inverse");
  return 0;
}

int glowk_iva_demix(const float* x_dev, const double* w_dev, int nsig, int M, int rows, int frames, float* y_dev, void* stream) {
  const std::string me("iva_demix");
  if (int rc = iva_ranges(me, nsig, M, rows, frames)) return rc;
  if (nsig == 0) return 0;
  if (!x_dev || !w_dev || !y_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {x_dev, w_dev, y_dev})) return rc;
  const size_t nx = iva_bytes_x(nsig, M, rows, frames);
  if (int rc = iva_disjoint(me, {{y_dev, nx}, {x_dev, nx}, {w_dev, iva_bytes_w(nsig, M, rows)}}, 1)) return rc;
  int dev;
  if (int rc = audio_device({x_dev, w_dev, y_dev}, &dev, "iva_demix")) return rc;
  DeviceGuard dg(dev);
  return iva_launch_demix(x_dev, w_dev, nullptr, nsig, M, rows, frames, y_dev, nullptr, (hipStream_t)stream);
}

int glowk_iva_images(const float* x_dev, const double* w_dev, const double* winv_dev, int nsig, int M, int rows, int frames, float* y_dev, float* img_dev,
                     void* stream) {
  const std::string me("iva_images");
  if (int rc = iva_ranges(me, nsig, M, rows, frames)) return rc;
  if ((int64_t)nsig * M * M * rows * frames > (int64_t)INT32_MAX) return fail(me + ": nsig * M * M * rows * frames must be at most 2^31 - 1");
  if (nsig == 0) return 0;
  if (!x_dev || !w_dev || !winv_dev || !img_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {x_dev, w_dev, winv_dev, y_dev, img_dev})) return rc;
  const size_t nx = iva_bytes_x(nsig, M, rows, frames), nw = iva_bytes_w(nsig, M, rows);
  if (int rc = iva_disjoint(me, {{img_dev, nx * M}, {y_dev, nx}, {x_dev, nx}, {w_dev, nw}, {winv_dev, nw}}, 2)) return rc;
  int dev;
  if (int rc = audio_device({x_dev, w_dev, winv_dev, y_dev, img_dev}, &dev, "iva_images")) return rc;
  DeviceGuard dg(dev);
  return iva_launch_demix(x_dev, w_dev, winv_dev, nsig, M, rows, frames, y_dev, img_dev, (hipStream_t)stream);
}

// ---- melody: harmonic salience, a Viterbi f0 track, a harmonic comb mask (glowk_melody.h) ------------------------------------------------
namespace {
int mel_sizes(const std::string& w, int nsig, int rows, int frames, int B) {
  using namespace glowk_melody;
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (rows < MIN_ROWS || rows > MAX_ROWS) return fail(w + ": rows must be in [2, 4096]");
  if (frames < 1 || frames > MAX_FRAMES) return fail(w + ": frames must be in [1, 32768]");
  if (B < 1 || B > MAX_BINS) return fail(w + ": the number of f0 bins B must be in [1, 1024]");
  if (!sizes_ok(nsig, rows, frames, B)) return fail(w + ": nsig * rows * frames and nsig * (B + 1) * frames must be at most 2^31 - 1");
  return 0;
}
int mel_harm(const std::string& w, int H) {
  if (H < 1 || H > glowk_melody::MAX_HARM) return fail(w + ": the number of harmonics H must be in [1, 32]");
  return 0;
}
int mel_track_params(const std::string& w, int J, double theta, double nu) {
  if (J < 0 || J > glowk_melody::MAX_JUMP) return fail(w + ": max_jump J must be in [0, 1023]");
  if (!std::isfinite(theta) || !std::isfinite(nu)) return fail(w + ": threshold and voicing_penalty must be finite");
  return 0;
}
int mel_mask_params(const std::string& w, int Hm, double width, double bin_hz) {
  if (Hm < 1 || Hm > glowk_melody::MAX_MASK_HARM) return fail(w + ": n_harmonics Hm must be in [1, 1024]");
  if (!(std::isfinite(width) && width > 0)) return fail(w + ": width must be finite and positive");
  if (!(std::isfinite(bin_hz) && bin_hz > 0)) return fail(w + ": bin_hz must be finite and positive");
  return 0;
}
size_t mel_bytes_s(int nsig, int rows, int frames) { return (size_t)nsig * rows * frames * 4; }

int mel_launch_salience(const float* s, int nsig, int rows, int frames, const int32_t* idx, const double* frac, const double* w, int B, int H, float* sal,
                        hipStream_t st) {
  using namespace glowk_melody;
  const int blocks = sal_blocks(B, frames);
  hipLaunchKernelGGL(k_melody_salience, dim3((unsigned)((int64_t)nsig * blocks)), dim3(SAL_THREADS), 0, st, s, rows, frames, idx, frac, w, B, H, blocks, sal);
  LAUNCHCHK("k_melody_salience");
  return 0;
}
int mel_launch_emission(const float* sal, int nsig, int B, int frames, double* e, float* m, float* partial, hipStream_t st) {
  using namespace glowk_melody;
  const int64_t cells = (int64_t)B * frames;
  const int groups = emi_groups(cells), blocks = emi_blocks(cells);
  hipLaunchKernelGGL(k_melody_max, dim3((unsigned)((int64_t)nsig * groups)), dim3(EMI_THREADS), 0, st, sal, cells, groups, partial);
  LAUNCHCHK("k_melody_max");
  hipLaunchKernelGGL(k_melody_emission, dim3((unsigned)((int64_t)nsig * blocks)), dim3(EMI_THREADS), 0, st, sal, cells, groups, blocks,
                     (const float*)partial, e, m);
  LAUNCHCHK("k_melody_emission");
  return 0;
}
int mel_launch_track(const double* e, int nsig, int B, int frames, const double* pen, int J, double theta, double nu, void* bp, int32_t* path, int64_t* ticks,
                     hipStream_t st) {
  using namespace glowk_melody;
  hipLaunchKernelGGL(k_melody_track, dim3((unsigned)nsig), dim3(trk_threads(B)), 0, st, e, B, frames, pen, J, theta, nu, (uint16_t*)bp, path, ticks);
  LAUNCHCHK("k_melody_track");
  return 0;
}
int mel_launch_mask(const int32_t* path, int nsig, int frames, const double* f0, int B, int rows, int Hm, double width, double bin_hz, float* mask,
                    hipStream_t st) {
  using namespace glowk_melody;
  const int blocks = msk_blocks(rows, frames);
  hipLaunchKernelGGL(k_melody_mask, dim3((unsigned)((int64_t)nsig * blocks)), dim3(MSK_THREADS), 0, st, path, frames, f0, B, rows, Hm, width, bin_hz, blocks,
                     mask);
  LAUNCHCHK("k_melody_mask");
  return 0;
}
}  // namespace

int glowk_melody_positions(const double* f0_host, int B, int H, double bin_hz, int rows, int32_t* idx_host, double* frac_host) {
  using namespace glowk_melody;
  const std::string me("melody_positions");
  if (B < 1 || B > MAX_BINS) return fail(me + ": the number of f0 bins B must be in [1, 1024]");
  if (int rc = mel_harm(me, H)) return rc;
  if (rows < MIN_ROWS || rows > MAX_ROWS) return fail(me + ": rows must be in [2, 4096]");
  if (!f0_host || !idx_host || !frac_host) return fail("null tensor");
  if (!grid_ok(f0_host, B, bin_hz)) return fail(me + ": f0 must be finite, positive and strictly ascending, bin_hz finite and positive");
  positions(f0_host, B, H, bin_hz, rows, idx_host, frac_host);
  return 0;
}

size_t glowk_melody_emission_workspace_bytes(int nsig, int B, int frames) {
  if (nsig < 1 || !glowk_melody::sizes_ok(nsig, glowk_melody::MIN_ROWS, frames, B)) return 0;
  return glowk_melody::emi_work_bytes(nsig, B, frames);
}
size_t glowk_melody_track_workspace_bytes(int nsig, int B, int frames) {
  if (nsig < 1 || !glowk_melody::sizes_ok(nsig, glowk_melody::MIN_ROWS, frames, B)) return 0;
  return glowk_melody::trk_work_bytes(nsig, B, frames);
}
size_t glowk_melody_workspace_bytes(int nsig, int B, int frames) {
  if (nsig < 1 || !glowk_melody::sizes_ok(nsig, glowk_melody::MIN_ROWS, frames, B)) return 0;
  return glowk_melody::fit_plan(nsig, B, frames).bytes;
}

int glowk_melody_salience(const float* s_dev, int nsig, int rows, int frames, const int32_t* idx_dev, const double* frac_dev, const double* w_dev, int B, int H,
                          float* sal_dev, void* stream) {
  const std::string me("melody_salience");
  if (int rc = mel_sizes(me, nsig, rows, frames, B)) return rc;
  if (int rc = mel_harm(me, H)) return rc;
  if (nsig == 0) return 0;
  if (!s_dev || !idx_dev || !frac_dev || !w_dev || !sal_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {frac_dev, w_dev})) return rc;
  if ((uintptr_t)s_dev % 4 || (uintptr_t)idx_dev % 4 || (uintptr_t)sal_dev % 4) return fail(me + ": the float32 and int32 tensors must be aligned to 4 bytes");
  if (int rc = iva_disjoint(me, {{sal_dev, (size_t)nsig * B * frames * 4}, {s_dev, mel_bytes_s(nsig, rows, frames)}, {idx_dev, (size_t)B * H * 4},
                                 {frac_dev, (size_t)B * H * 8}, {w_dev, (size_t)H * 8}}, 1))
    return rc;
  int dev;
  if (int rc = audio_device({s_dev, idx_dev, frac_dev, w_dev, sal_dev}, &dev, "melody_salience")) return rc;
  DeviceGuard dg(dev);
  return mel_launch_salience(s_dev, nsig, rows, frames, idx_dev, frac_dev, w_dev, B, H, sal_dev, (hipStream_t)stream);
}

int glowk_melody_emission(const float* sal_dev, int nsig, int B, int frames, double* e_dev, float* m_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_melody;
  const std::string me("melody_emission");
  if (int rc = mel_sizes(me, nsig, MIN_ROWS, frames, B)) return rc;
  if (nsig == 0) return 0;
  if (!sal_dev || !e_dev || !m_dev || !work_dev) return fail("null tensor");
  const size_t need = emi_work_bytes(nsig, B, frames), cells = (size_t)nsig * B * frames;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_melody_emission_workspace_bytes says");
  if (int rc = iva_aligned(me, {e_dev, work_dev})) return rc;
  if ((uintptr_t)sal_dev % 4 || (uintptr_t)m_dev % 4) return fail(me + ": the float32 tensors must be aligned to 4 bytes");
  if (int rc = iva_disjoint(me, {{e_dev, cells * 8}, {m_dev, (size_t)nsig * 4}, {work_dev, need}, {sal_dev, cells * 4}}, 3)) return rc;
  int dev;
  if (int rc = audio_device({sal_dev, e_dev, m_dev, work_dev}, &dev, "melody_emission")) return rc;
  DeviceGuard dg(dev);
  return mel_launch_emission(sal_dev, nsig, B, frames, e_dev, m_dev, (float*)work_dev, (hipStream_t)stream);
}

int glowk_melody_track(const double* e_dev, int nsig, int B, int frames, const double* pen_dev, int J, double theta, double nu, int32_t* path_dev,
                       int64_t* ticks_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_melody;
  const std::string me("melody_track");
  if (int rc = mel_sizes(me, nsig, MIN_ROWS, frames, B)) return rc;
  if (int rc = mel_track_params(me, J, theta, nu)) return rc;
  if (nsig == 0) return 0;
  if (!e_dev || !pen_dev || !path_dev || !work_dev) return fail("null tensor");
  const size_t need = trk_work_bytes(nsig, B, frames);
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_melody_track_workspace_bytes says");
  if (int rc = iva_aligned(me, {e_dev, pen_dev, ticks_dev, work_dev})) return rc;
  if ((uintptr_t)path_dev % 4) return fail(me + ": path_dev must be aligned to 4 bytes");
  if (int rc = iva_disjoint(me, {{path_dev, (size_t)nsig * frames * 4}, {work_dev, need}, {ticks_dev, (size_t)nsig * 16},
                                 {e_dev, (size_t)nsig * B * frames * 8}, {pen_dev, (size_t)(J + 1) * 8}}, 3))
    return rc;
  int dev;
  if (int rc = audio_device({e_dev, pen_dev, path_dev, ticks_dev, work_dev}, &dev, "melody_track")) return rc;
  DeviceGuard dg(dev);
  return mel_launch_track(e_dev, nsig, B, frames, pen_dev, J, theta, nu, work_dev, path_dev, ticks_dev, (hipStream_t)stream);
}

int glowk_melody_mask(const int32_t* path_dev, int nsig, int frames, const double* f0_dev, int B, int rows, int Hm, double width, double bin_hz, float* mask_dev,
                      void* stream) {
  const std::string me("melody_mask");
  if (int rc = mel_sizes(me, nsig, rows, frames, B)) return rc;
  if (int rc = mel_mask_params(me, Hm, width, bin_hz)) return rc;
  if (nsig == 0) return 0;
  if (!path_dev || !f0_dev || !mask_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {f0_dev})) return rc;
  if ((uintptr_t)path_dev % 4 || (uintptr_t)mask_dev % 4) return fail(me + ": the float32 and int32 tensors must be aligned to 4 bytes");
  if (int rc = iva_disjoint(me, {{mask_dev, mel_bytes_s(nsig, rows, frames)}, {path_dev, (size_t)nsig * frames * 4}, {f0_dev, (size_t)B * 8}}, 1)) return rc;
  int dev;
  if (int rc = audio_device({path_dev, f0_dev, mask_dev}, &dev, "melody_mask")) return rc;
  DeviceGuard dg(dev);
  return mel_launch_mask(path_dev, nsig, frames, f0_dev, B, rows, Hm, width, bin_hz, mask_dev, (hipStream_t)stream);
}

int glowk_melody_fit(const float* s_dev, int nsig, int rows, int frames, const int32_t* idx_dev, const double* frac_dev, const double* w_dev,
                     const double* f0_dev, int B, int H, const double* pen_dev, int J, double theta, double nu, int Hm, double width, double bin_hz,
                     int32_t* path_dev, float* mask_dev, float* m_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_melody;
  const std::string me("melody_fit");
  if (int rc = mel_sizes(me, nsig, rows, frames, B)) return rc;
  if (int rc = mel_harm(me, H)) return rc;
  if (int rc = mel_track_params(me, J, theta, nu)) return rc;
  if (int rc = mel_mask_params(me, Hm, width, bin_hz)) return rc;
  if (nsig == 0) return 0;
  if (!s_dev || !idx_dev || !frac_dev || !w_dev || !f0_dev || !pen_dev || !path_dev || !mask_dev || !m_dev || !work_dev) return fail("null tensor");
  const FitPlan pl = fit_plan(nsig, B, frames);
  if (work_bytes < pl.bytes) return fail(me + ": work_bytes is smaller than glowk_melody_workspace_bytes says");
  if (int rc = iva_aligned(me, {frac_dev, w_dev, f0_dev, pen_dev, work_dev})) return rc;
  if ((uintptr_t)s_dev % 4 || (uintptr_t)idx_dev % 4 || (uintptr_t)path_dev % 4 || (uintptr_t)mask_dev % 4 || (uintptr_t)m_dev % 4)
    return fail(me + ": the float32 and int32 tensors must be aligned to 4 bytes");
  if (int rc = iva_disjoint(me, {{path_dev, (size_t)nsig * frames * 4}, {mask_dev, mel_bytes_s(nsig, rows, frames)}, {m_dev, (size_t)nsig * 4},
                                 {work_dev, pl.bytes}, {s_dev, mel_bytes_s(nsig, rows, frames)}, {idx_dev, (size_t)B * H * 4}, {frac_dev, (size_t)B * H * 8},
                                 {w_dev, (size_t)H * 8}, {f0_dev, (size_t)B * 8}, {pen_dev, (size_t)(J + 1) * 8}}, 4))
    return rc;
  int dev;
  if (int rc = audio_device({s_dev, idx_dev, frac_dev, w_dev, f0_dev, pen_dev, path_dev, mask_dev, m_dev, work_dev}, &dev, "melody_fit")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  char* wk = (char*)work_dev;
  float* sal = (float*)(wk + pl.sal);
  double* e = (double*)(wk + pl.emi);
  if (int rc = mel_launch_salience(s_dev, nsig, rows, frames, idx_dev, frac_dev, w_dev, B, H, sal, st)) return rc;
  if (int rc = mel_launch_emission(sal, nsig, B, frames, e, m_dev, (float*)(wk + pl.part), st)) return rc;
  if (int rc = mel_launch_track(e, nsig, B, frames, pen_dev, J, theta, nu, wk + pl.bp, path_dev, nullptr, st)) return rc;
  return mel_launch_mask(path_dev, nsig, frames, f0_dev, B, rows, Hm, width, bin_hz, mask_dev, st);
}


// ---- RPCA: low-rank plus sparse by inexact ALM; fp64 GEMM on the matrix cores, Jacobi eigensolver (glowk_rpca.h) ------------------------------
namespace {
enum { RPCA_GRAM = 0, RPCA_SCALED = 1, RPCA_APPLY = 2 };

int rpca_sizes(const std::string& w, int nsig, int rows, int frames) {
  using namespace glowk_rpca;
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (rows < 1 || rows > MAX_ROWS) return fail(w + ": rows must be in [1, 2049]");
  if (frames < 1 || frames > MAX_FRAMES) return fail(w + ": frames must be in [1, 65535]");
  if (!sizes_ok(nsig, rows, frames)) return fail(w + ": nsig * rows * frames and nsig * rows * rows must be at most 2^31 - 1");
  return 0;
}
bool rpca_gemm_ok(int nsig, int M, int N, int K, int form) {
  using namespace glowk_rpca;
  if (form < RPCA_GRAM || form > RPCA_APPLY) return false;
  if (nsig < 0 || nsig > MAX_SIG || M < 1 || M > MAX_ROWS || N < 1 || N > MAX_FRAMES || K < 1 || K > MAX_FRAMES) return false;
  if (form != RPCA_APPLY && N != M) return false;
  return (int64_t)nsig * M * N <= MAX_ELEMENTS && (int64_t)nsig * M * K <= MAX_ELEMENTS && (int64_t)nsig * N * K <= MAX_ELEMENTS;
}
int rpca_blocks(int64_t cells) { return (int)((cells + glowk_rpca::EW_THREADS - 1) / glowk_rpca::EW_THREADS); }

// C = A A^T (GRAM, K split by the index header's rule), A diag(scale) A^T (SCALED) or A B (APPLY)
int rpca_launch_gemm(int form, const double* A, const double* B, const double* scale, int nsig, int M, int N, int K, const int* active, double* C,
                     double* partial, hipStream_t st) {
  using namespace glowk_rpca;
  const int nsplit = form == RPCA_GRAM ? gemm_splits(K) : 1;
  const int len = nsplit == 1 ? K : gemm_split_len(K);
  if (form == RPCA_APPLY) {
    const dim3 grid((unsigned)(gemm_tiles(M) * gemm_tiles(N)), 1, (unsigned)nsig);
    hipLaunchKernelGGL((k_rpca_gemm<false, false>), grid, dim3(GEMM_THREADS), 0, st, A, B, scale, M, N, K, 1, len, active, C, partial);
    LAUNCHCHK("k_rpca_gemm");
    return 0;
  }
  const dim3 grid((unsigned)gemm_upper_count(gemm_tiles(M)), (unsigned)nsplit, (unsigned)nsig);
  hipLaunchKernelGGL((k_rpca_gemm<true, true>), grid, dim3(GEMM_THREADS), 0, st, A, A, scale, M, M, K, nsplit, len, active, C, partial);
  LAUNCHCHK("k_rpca_gemm");
  if (nsplit > 1) {
    const int blocks = rpca_blocks((int64_t)M * M);
    hipLaunchKernelGGL((k_rpca_gemm_reduce<true>), dim3((unsigned)((int64_t)nsig * blocks)), dim3(EW_THREADS), 0, st, (const double*)partial, M, M, nsplit,
                       blocks, active, C);
    LAUNCHCHK("k_rpca_gemm_reduce");
  }
  return 0;
}

// G -> diag(l) in place, V; two launches per round, the sweep flags read by the host after every sweep (the one synchronisation)
int rpca_launch_eigh(double* G, int nsig, int n, const int* active, double* l, double* V, int32_t* sweeps, int32_t* status, void* work, hipStream_t st) {
  using namespace glowk_rpca;
  const EighPlan pl = eigh_plan(nsig, n);
  double* cs = (double*)((char*)work + pl.cs);
  double* floor = (double*)((char*)work + pl.floor);
  int* flags = (int*)((char*)work + pl.flags);
  const int blocks = rpca_blocks((int64_t)n * n), rounds = rr_rounds(n), pairs = rr_pairs(n);
  hipLaunchKernelGGL(k_rpca_eye, dim3((unsigned)((int64_t)nsig * blocks)), dim3(EW_THREADS), 0, st, V, n, blocks, nsig, active, flags);
  LAUNCHCHK("k_rpca_eye");
  hipLaunchKernelGGL(k_rpca_jacobi_floor, dim3((unsigned)nsig), dim3(EW_THREADS), 0, st, (const double*)G, n, active, floor);
  LAUNCHCHK("k_rpca_jacobi_floor");
  int swept = 1;
  if (rounds > 0) {
    std::vector<int> host((size_t)nsig);
    for (int sweep = 0; sweep < MAX_SWEEPS; ++sweep) {
      for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_rpca_jacobi_rows, dim3((unsigned)pairs, (unsigned)nsig), dim3(JAC_THREADS), 0, st, G, n, nsig, sweep, r, active, (const double*)floor, cs, flags);
        LAUNCHCHK("k_rpca_jacobi_rows");
        hipLaunchKernelGGL(k_rpca_jacobi_cols, dim3((unsigned)n, (unsigned)nsig), dim3(JAC_THREADS), 0, st, G, V, n, nsig, sweep, r, active,
                           (const double*)cs, (const int*)flags);
        LAUNCHCHK("k_rpca_jacobi_cols");
      }
      swept = sweep + 1;
      HIPCHK(hipMemcpyAsync(host.data(), flags + (size_t)sweep * nsig, (size_t)nsig * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      bool any = false;
      for (int v : host) any = any || v != 0;
      if (!any) break;
    }
  }
  hipLaunchKernelGGL(k_rpca_eigh_finish, dim3((unsigned)nsig), dim3(EW_THREADS), 0, st, (const double*)G, n, nsig, swept, active, (const int*)flags, l, sweeps,
                     status);
  LAUNCHCHK("k_rpca_eigh_finish");
  return 0;
}

// L = V diag(g) V^T A from the eigendecomposition of A A^T
int rpca_launch_svt(const double* A, int nsig, int rows, int frames, const double* tau, const int* active, double* L, int32_t* sweeps, int32_t* status,
                    void* work, hipStream_t st) {
  using namespace glowk_rpca;
  const SvtPlan pl = svt_plan(nsig, rows, frames);
  char* wk = (char*)work;
  double *G = (double*)(wk + pl.g), *V = (double*)(wk + pl.v), *P = (double*)(wk + pl.p), *l = (double*)(wk + pl.l), *gain = (double*)(wk + pl.gain);
  if (int rc = rpca_launch_gemm(RPCA_GRAM, A, nullptr, nullptr, nsig, rows, rows, frames, active, G, (double*)(wk + pl.gemm), st)) return rc;
  if (int rc = rpca_launch_eigh(G, nsig, rows, active, l, V, sweeps ? sweeps : (int32_t*)(wk + pl.sweeps), status, wk + pl.eigh, st)) return rc;
  const int blocks = rpca_blocks(rows);
  hipLaunchKernelGGL(k_rpca_gains, dim3((unsigned)((int64_t)nsig * blocks)), dim3(EW_THREADS), 0, st, (const double*)l, tau, rows, blocks, active, gain);
  LAUNCHCHK("k_rpca_gains");
  if (int rc = rpca_launch_gemm(RPCA_SCALED, V, nullptr, gain, nsig, rows, rows, rows, active, P, nullptr, st)) return rc;
  return rpca_launch_gemm(RPCA_APPLY, P, A, nullptr, nsig, rows, frames, rows, active, L, nullptr, st);
}
}  // namespace

size_t glowk_rpca_gemm_workspace_bytes(int nsig, int M, int N, int K, int form) {
  if (nsig < 1 || !rpca_gemm_ok(nsig, M, N, K, form) || form != RPCA_GRAM) return 0;
  return glowk_rpca::gemm_work_bytes(nsig, M, M, K);
}
size_t glowk_rpca_eigh_workspace_bytes(int nsig, int n) {
  if (nsig < 1 || !glowk_rpca::sizes_ok(nsig, n, 1)) return 0;
  return glowk_rpca::eigh_plan(nsig, n).bytes;
}
size_t glowk_rpca_svt_workspace_bytes(int nsig, int rows, int frames) {
  if (nsig < 1 || !glowk_rpca::sizes_ok(nsig, rows, frames)) return 0;
  return glowk_rpca::svt_plan(nsig, rows, frames).bytes;
}
size_t glowk_rpca_workspace_bytes(int nsig, int rows, int frames) {
  if (nsig < 1 || !glowk_rpca::sizes_ok(nsig, rows, frames)) return 0;
  return glowk_rpca::fit_plan(nsig, rows, frames).bytes;
}

int glowk_rpca_gemm(const double* a_dev, const double* b_dev, const double* scale_dev, int nsig, int M, int N, int K, int form, double* c_dev, void* work_dev,
                    size_t work_bytes, void* stream) {
  using namespace glowk_rpca;
  const std::string me("rpca_gemm");
  if (form < RPCA_GRAM || form > RPCA_APPLY) return fail(me + ": form must be 0 (A A^T), 1 (A diag(scale) A^T) or 2 (A B)");
  if (nsig < 0 || nsig > MAX_SIG) return fail(me + ": nsig must be in [0, 65535]");
  if (M < 1 || M > MAX_ROWS) return fail(me + ": M must be in [1, 2049]");
  if (N < 1 || N > MAX_FRAMES || K < 1 || K > MAX_FRAMES) return fail(me + ": N and K must be in [1, 65535]");
  if (form != RPCA_APPLY && N != M) return fail(me + ": the symmetric forms need N == M");
  if (!rpca_gemm_ok(nsig, M, N, K, form)) return fail(me + ": every operand must have at most 2^31 - 1 elements");
  if (nsig == 0) return 0;
  const size_t need = form == RPCA_GRAM ? gemm_work_bytes(nsig, M, M, K) : 0;
  if (!a_dev || !c_dev || (form == RPCA_APPLY && !b_dev) || (form == RPCA_SCALED && !scale_dev) || (need && !work_dev)) return fail("null tensor");
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_rpca_gemm_workspace_bytes says");
  if (int rc = iva_aligned(me, {a_dev, b_dev, scale_dev, c_dev, work_dev})) return rc;
  const double* b = form == RPCA_APPLY ? b_dev : nullptr;
  const double* sc = form == RPCA_SCALED ? scale_dev : nullptr;
  if (int rc = iva_disjoint(me, {{c_dev, (size_t)nsig * M * N * 8}, {need ? work_dev : nullptr, need}, {a_dev, (size_t)nsig * M * K * 8},
                                 {b, (size_t)nsig * K * N * 8}, {sc, (size_t)nsig * K * 8}}, 2))
    return rc;
  int dev;
  if (int rc = audio_device({a_dev, b, sc, c_dev, need ? work_dev : nullptr}, &dev, "rpca_gemm")) return rc;
  DeviceGuard dg(dev);
  return rpca_launch_gemm(form, a_dev, b, sc, nsig, M, N, K, nullptr, c_dev, (double*)work_dev, (hipStream_t)stream);
}

int glowk_rpca_eigh(double* g_dev, int nsig, int n, double* l_dev, double* v_dev, int32_t* sweeps_dev, int32_t* status_dev, void* work_dev, size_t work_bytes,
                    void* stream) {
  using namespace glowk_rpca;
  const std::string me("rpca_eigh");
  if (nsig < 0 || nsig > MAX_SIG) return fail(me + ": nsig must be in [0, 65535]");
  if (n < 1 || n > MAX_ROWS) return fail(me + ": n must be in [1, 2049]");
  if (!sizes_ok(nsig, n, 1)) return fail(me + ": nsig * n * n must be at most 2^31 - 1");
  if (nsig == 0) return 0;
  if (!g_dev || !l_dev || !v_dev || !sweeps_dev || !status_dev || !work_dev) return fail("null tensor");
  const size_t need = eigh_plan(nsig, n).bytes, nn = (size_t)nsig * n * n * 8;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_rpca_eigh_workspace_bytes says");
  if (int rc = iva_aligned(me, {g_dev, l_dev, v_dev, work_dev})) return rc;
  if ((uintptr_t)sweeps_dev % 4 || (uintptr_t)status_dev % 4) return fail(me + ": the int32 tensors must be aligned to 4 bytes");
  if (int rc = iva_disjoint(me, {{g_dev, nn}, {v_dev, nn}, {l_dev, (size_t)nsig * n * 8}, {sweeps_dev, (size_t)nsig * 4}, {status_dev, (size_t)nsig * 4},
                                 {work_dev, need}}, 6))
    return rc;
  int dev;
  if (int rc = audio_device({g_dev, l_dev, v_dev, sweeps_dev, status_dev, work_dev}, &dev, "rpca_eigh")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(status_dev, 0, (size_t)nsig * 4, st));
  return rpca_launch_eigh(g_dev, nsig, n, nullptr, l_dev, v_dev, sweeps_dev, status_dev, work_dev, st);
}

int glowk_rpca_shrink(const double* t_dev, size_t count, double thr, double* out_dev, void* stream) {
  const std::string me("rpca_shrink");
  if (count > (size_t)glowk_rpca::MAX_ELEMENTS) return fail(me + ": count must be at most 2^31 - 1");
  if (!(std::isfinite(thr) && thr >= 0)) return fail(me + ": thr must be finite and not negative");
  if (count == 0) return 0;
  if (!t_dev || !out_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {t_dev, out_dev})) return rc;
  if (t_dev != out_dev && bytes_overlap(t_dev, count * 8, out_dev, count * 8)) return fail(me + ": out_dev must be t_dev itself or not overlap it");
  int dev;
  if (int rc = audio_device({t_dev, out_dev}, &dev, "rpca_shrink")) return rc;
  DeviceGuard dg(dev);
  hipLaunchKernelGGL(glowk_rpca::k_rpca_shrink, dim3((unsigned)rpca_blocks((int64_t)count)), dim3(glowk_rpca::EW_THREADS), 0, (hipStream_t)stream, t_dev,
                     (int64_t)count, thr, out_dev);
  LAUNCHCHK("k_rpca_shrink");
  return 0;
}

int glowk_rpca_svt(const double* a_dev, int nsig, int rows, int frames, const double* tau_dev, double* l_dev, int32_t* sweeps_dev, int32_t* status_dev,
                   void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_rpca;
  const std::string me("rpca_svt");
  if (int rc = rpca_sizes(me, nsig, rows, frames)) return rc;
  if (nsig == 0) return 0;
  if (!a_dev || !tau_dev || !l_dev || !sweeps_dev || !status_dev || !work_dev) return fail("null tensor");
  const size_t need = svt_plan(nsig, rows, frames).bytes, cells = (size_t)nsig * rows * frames * 8;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_rpca_svt_workspace_bytes says");
  if (int rc = iva_aligned(me, {a_dev, tau_dev, l_dev, work_dev})) return rc;
  if ((uintptr_t)sweeps_dev % 4 || (uintptr_t)status_dev % 4) return fail(me + ": the int32 tensors must be aligned to 4 bytes");
  if (int rc = iva_disjoint(me, {{l_dev, cells}, {sweeps_dev, (size_t)nsig * 4}, {status_dev, (size_t)nsig * 4}, {work_dev, need}, {a_dev, cells},
                                 {tau_dev, (size_t)nsig * 8}}, 4))
    return rc;
  int dev;
  if (int rc = audio_device({a_dev, tau_dev, l_dev, sweeps_dev, status_dev, work_dev}, &dev, "rpca_svt")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(status_dev, 0, (size_t)nsig * 4, st));
  return rpca_launch_svt(a_dev, nsig, rows, frames, tau_dev, nullptr, l_dev, sweeps_dev, status_dev, work_dev, st);
}

int glowk_rpca_fit(const float* m_dev, int nsig, int rows, int frames, double gain, double tol, int n_iter, double* l_dev, double* s_dev, int32_t* iters_dev,
                   int32_t* status_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_rpca;
  const std::string me("rpca_fit");
  if (int rc = rpca_sizes(me, nsig, rows, frames)) return rc;
  if (!(std::isfinite(gain) && gain > 0)) return fail(me + ": gain must be finite and positive");
  if (!(std::isfinite(tol) && tol >= 0)) return fail(me + ": tol must be finite and not negative");
  if (n_iter < 0 || n_iter > MAX_ITER) return fail(me + ": n_iter must be in [0, 100000]");
  if (nsig == 0) return 0;
  if (!m_dev || !l_dev || !s_dev || !iters_dev || !status_dev || !work_dev) return fail("null tensor");
  const FitPlan pl = fit_plan(nsig, rows, frames);
  const size_t cells8 = (size_t)nsig * rows * frames * 8;
  if (work_bytes < pl.bytes) return fail(me + ": work_bytes is smaller than glowk_rpca_workspace_bytes says");
  if (int rc = iva_aligned(me, {l_dev, s_dev, work_dev})) return rc;
  if ((uintptr_t)m_dev % 4 || (uintptr_t)iters_dev % 4 || (uintptr_t)status_dev % 4) return fail(me + ": the float32 and int32 tensors must be aligned to 4 bytes");
  if (int rc = iva_disjoint(me, {{l_dev, cells8}, {s_dev, cells8}, {iters_dev, (size_t)nsig * 4}, {status_dev, (size_t)nsig * 4}, {work_dev, pl.bytes},
                                 {m_dev, cells8 / 2}}, 5))
    return rc;
  int dev;
  if (int rc = audio_device({m_dev, l_dev, s_dev, iters_dev, status_dev, work_dev}, &dev, "rpca_fit")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  char* wk = (char*)work_dev;
  const SvtPlan sp = svt_plan(nsig, rows, frames);
  double *Y = (double*)(wk + pl.y), *A = (double*)(wk + pl.a), *state = (double*)(wk + pl.state), *tau = (double*)(wk + pl.tau), *sums = (double*)(wk + pl.sums);
  float* maxes = (float*)(wk + pl.maxes);
  int* active = (int*)(wk + pl.active);
  char* svt = wk + pl.svt;
  double *G = (double*)(svt + sp.g), *V = (double*)(svt + sp.v), *l = (double*)(svt + sp.l);
  int32_t *sweeps = (int32_t*)(svt + sp.sweeps), *solve_status = (int32_t*)(svt + sp.status);
  const int64_t cells = (int64_t)rows * frames;
  const int groups = ew_groups(cells), blocks = rpca_blocks(cells);
  const double lam = gain / std::sqrt((double)(rows > frames ? rows : frames));

  // the start: ||M||_2 from the Gram matrix of M itself (A holds M as float64 for the product), max |M|, then Y, L, S and the state
  HIPCHK(hipMemsetAsync(status_dev, 0, (size_t)nsig * 4, st));
  HIPCHK(hipMemsetAsync(solve_status, 0, (size_t)nsig * 4, st));
  hipLaunchKernelGGL(k_rpca_widen, dim3((unsigned)rpca_blocks((int64_t)nsig * cells)), dim3(EW_THREADS), 0, st, m_dev, (int64_t)nsig * cells, A);
  LAUNCHCHK("k_rpca_widen");
  if (int rc = rpca_launch_gemm(RPCA_GRAM, A, nullptr, nullptr, nsig, rows, rows, frames, nullptr, G, (double*)(svt + sp.gemm), st)) return rc;
  if (int rc = rpca_launch_eigh(G, nsig, rows, nullptr, l, V, sweeps, solve_status, svt + sp.eigh, st)) return rc;
  hipLaunchKernelGGL(k_rpca_absmax, dim3((unsigned)((int64_t)nsig * groups)), dim3(EW_THREADS), 0, st, m_dev, cells, groups, maxes);
  LAUNCHCHK("k_rpca_absmax");
  hipLaunchKernelGGL(k_rpca_init, dim3((unsigned)nsig), dim3(64), 0, st, (const double*)l, rows, (const float*)maxes, groups, lam, state, tau, active, iters_dev,
                     (const int*)solve_status, status_dev);
  LAUNCHCHK("k_rpca_init");
  hipLaunchKernelGGL(k_rpca_start, dim3((unsigned)((int64_t)nsig * blocks)), dim3(EW_THREADS), 0, st, m_dev, cells, blocks, (const double*)state, (const int*)active,
                     l_dev, s_dev, Y);
  LAUNCHCHK("k_rpca_start");

  std::vector<int> host((size_t)nsig);
  for (int it = 0; it < n_iter; ++it) {
    HIPCHK(hipMemcpyAsync(host.data(), active, (size_t)nsig * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    bool any = false;
    for (int v : host) any = any || v != 0;
    if (!any) break;
    hipLaunchKernelGGL(k_rpca_sparse, dim3((unsigned)((int64_t)nsig * blocks)), dim3(EW_THREADS), 0, st, m_dev, (const double*)l_dev, (const double*)Y, cells, blocks,
                       (const double*)state, (const int*)active, s_dev, A);
    LAUNCHCHK("k_rpca_sparse");
    if (int rc = rpca_launch_svt(A, nsig, rows, frames, tau, active, l_dev, nullptr, solve_status, svt, st)) return rc;
    hipLaunchKernelGGL(k_rpca_residual, dim3((unsigned)((int64_t)nsig * groups)), dim3(EW_THREADS), 0, st, m_dev, (const double*)l_dev, (const double*)s_dev, cells,
                       groups, (const double*)state, (const int*)active, Y, sums);
    LAUNCHCHK("k_rpca_residual");
    hipLaunchKernelGGL(k_rpca_finish, dim3((unsigned)nsig), dim3(64), 0, st, (const double*)sums, groups, tol, state, tau, active, iters_dev,
                       (const int*)solve_status, status_dev);
    LAUNCHCHK("k_rpca_finish");
  }
  return 0;
}

int glowk_rpca_binary_mask(const double* l_dev, const double* s_dev, const float* x_dev, size_t count, double gain_mask, float* mask_dev, float* bg_dev,
                           float* fg_dev, void* stream) {
  const std::string me("rpca_binary_mask");
  if (count > (size_t)glowk_rpca::MAX_ELEMENTS) return fail(me + ": count must be at most 2^31 - 1");
  if (!(std::isfinite(gain_mask) && gain_mask >= 0)) return fail(me + ": gain_mask must be finite and not negative");
  if (count == 0) return 0;
  if (!l_dev || !s_dev || !mask_dev || (x_dev && (!bg_dev || !fg_dev))) return fail("null tensor");
  if (int rc = iva_aligned(me, {l_dev, s_dev, x_dev, bg_dev, fg_dev})) return rc;
  if ((uintptr_t)mask_dev % 4) return fail(me + ": mask_dev must be aligned to 4 bytes");
  const float* bg = x_dev ? bg_dev : nullptr;
  const float* fg = x_dev ? fg_dev : nullptr;
  if (int rc = iva_disjoint(me, {{mask_dev, count * 4}, {bg, count * 8}, {fg, count * 8}, {l_dev, count * 8}, {s_dev, count * 8}, {x_dev, count * 8}}, 3)) return rc;
  int dev;
  if (int rc = audio_device({l_dev, s_dev, x_dev, mask_dev, bg, fg}, &dev, "rpca_binary_mask")) return rc;
  DeviceGuard dg(dev);
  hipLaunchKernelGGL(glowk_rpca::k_rpca_binary_mask, dim3((unsigned)rpca_blocks((int64_t)count)), dim3(glowk_rpca::EW_THREADS), 0, (hipStream_t)stream, l_dev, s_dev,
                     (const float2*)x_dev, (int64_t)count, gain_mask, mask_dev, (float2*)bg, (float2*)fg);
  LAUNCHCHK("k_rpca_binary_mask");
  return 0;
}

// ---- PROJET: panned sources from two channels by projections; the outer sums on the fp64 matrix cores (glowk_projet.h) -------------------------
namespace {
int projet_sizes(const std::string& w, int nsig, int rows, int frames, int J) {
  using namespace glowk_projet;
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (rows < 1 || rows > MAX_ROWS) return fail(w + ": rows must be in [1, 4096]");
  if (frames < 1 || frames > MAX_FRAMES) return fail(w + ": frames must be in [1, 32768]");
  if (J < 1 || J > MAX_J) return fail(w + ": the source count J must be in [1, 8]");
  if (!sizes_ok(nsig, rows, frames, J)) return fail(w + ": nsig * J * rows * frames must be at most 2^31 - 1");
  return 0;
}
int projet_model(const std::string& w, int nsig, int M, int L, int J) {
  using namespace glowk_projet;
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (M < MIN_M || M > MAX_M) return fail(w + ": the projection count M must be in [2, 32]");
  if (L < 1 || L > MAX_L) return fail(w + ": the pan count L must be in [1, 128]");
  if (J < 1 || J > MAX_J) return fail(w + ": the source count J must be in [1, 8]");
  return 0;
}
int projet_powers(const std::string& w, double alpha, int beta) {
  if (!(alpha >= 1.0 && alpha <= 2.0)) return fail(w + ": alpha must be in [1, 2]");
  if (beta < 0 || beta > 2) return fail(w + ": beta must be 0, 1 or 2");
  return 0;
}
int projet_amode(double alpha) {
  return alpha == 1.0 ? glowk_projet::ALPHA_ONE : alpha == 2.0 ? glowk_projet::ALPHA_TWO : glowk_projet::ALPHA_POW;
}
size_t projet_bytes_x(int nsig, int rows, int frames) { return (size_t)nsig * 2 * rows * frames * 8; }
size_t projet_bytes_p(int nsig, int J, int rows, int frames) { return (size_t)nsig * J * rows * frames * 8; }

#define GLOWK_PROJET_EACH_J(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

int projet_launch_gains(const double* K, const double* Q, int nsig, int M, int L, int J, double* G, hipStream_t st) {
  using namespace glowk_projet;
  hipLaunchKernelGGL(k_projet_gains, dim3((unsigned)nsig), dim3(THREADS), 0, st, K, Q, M, L, J, G);
  LAUNCHCHK("k_projet_gains");
  return 0;
}
// the fused pass: the P update (do_p), the partial outer sums (do_sums), or both
int projet_launch_iterate(const float* x, double* P, int nsig, int rows, int frames, const double* U, const double* G, int M, int J, double alpha, int beta,
                          int do_p, int do_sums, double* partial, hipStream_t st) {
  using namespace glowk_projet;
  const int64_t cells = (int64_t)rows * frames;
  const dim3 grid((unsigned)((int64_t)nsig * groups(cells)));
  switch (J) {
#define GLOWK_CASE(j)                                                                                                                        \
  case j:                                                                                                                                    \
    hipLaunchKernelGGL(k_projet_iterate<j>, grid, dim3(THREADS), 0, st, (const float2*)x, P, cells, U, G, M, projet_amode(alpha), alpha / 2.0, beta, do_p, do_sums, \
                       partial);                                                                                                             \
    break;
    GLOWK_PROJET_EACH_J(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_projet_iterate");
  return 0;
}
int projet_launch_q(const double* partial, int nsig, int rows, int frames, const double* K, int M, int L, int J, int beta, double* Q, double* G, hipStream_t st) {
  using namespace glowk_projet;
  hipLaunchKernelGGL(k_projet_q, dim3((unsigned)nsig), dim3(THREADS), 0, st, partial, groups((int64_t)rows * frames), K, M, L, J, beta, Q, G);
  LAUNCHCHK("k_projet_q");
  return 0;
}
}  // namespace

size_t glowk_projet_workspace_bytes(int nsig, int M, int J, int rows, int frames) {
  using namespace glowk_projet;
  if (nsig < 1 || !sizes_ok(nsig, rows, frames, J) || !model_ok(M, 1, J)) return 0;
  return work_bytes(nsig, M, J, rows, frames);
}

int glowk_projet_projections(const float* x_dev, int nsig, int rows, int frames, const double* u_dev, int M, double alpha, double* v_dev, void* stream) {
  using namespace glowk_projet;
  const std::string me("projet_projections");
  if (int rc = projet_sizes(me, nsig, rows, frames, 1)) return rc;
  if (int rc = projet_model(me, nsig, M, 1, 1)) return rc;
  if (int rc = projet_powers(me, alpha, 1)) return rc;
  if ((int64_t)nsig * M * rows * frames > MAX_ELEMENTS) return fail(me + ": nsig * M * rows * frames must be at most 2^31 - 1");
  if (nsig == 0) return 0;
  if (!x_dev || !u_dev || !v_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {x_dev, u_dev, v_dev})) return rc;
  if (int rc = iva_disjoint(me, {{v_dev, (size_t)nsig * M * rows * frames * 8}, {x_dev, projet_bytes_x(nsig, rows, frames)}, {u_dev, (size_t)M * 16}}, 1)) return rc;
  int dev;
  if (int rc = audio_device({x_dev, u_dev, v_dev}, &dev, "projet_projections")) return rc;
  DeviceGuard dg(dev);
  const int64_t cells = (int64_t)rows * frames, total = cells * nsig;
  hipLaunchKernelGGL(k_projet_projections, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, (const float2*)x_dev, total, cells,
                     u_dev, M, projet_amode(alpha), alpha / 2.0, v_dev);
  LAUNCHCHK("k_projet_projections");
  return 0;
}

int glowk_projet_gains(const double* k_dev, const double* q_dev, int nsig, int M, int L, int J, double* g_dev, void* stream) {
  const std::string me("projet_gains");
  if (int rc = projet_model(me, nsig, M, L, J)) return rc;
  if (nsig == 0) return 0;
  if (!k_dev || !q_dev || !g_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {k_dev, q_dev, g_dev})) return rc;
  if (int rc = iva_disjoint(me, {{g_dev, (size_t)nsig * M * J * 8}, {k_dev, (size_t)M * L * 8}, {q_dev, (size_t)nsig * L * J * 8}}, 1)) return rc;
  int dev;
  if (int rc = audio_device({k_dev, q_dev, g_dev}, &dev, "projet_gains")) return rc;
  DeviceGuard dg(dev);
  return projet_launch_gains(k_dev, q_dev, nsig, M, L, J, g_dev, (hipStream_t)stream);
}

int glowk_projet_update_p(const float* x_dev, int nsig, int rows, int frames, const double* u_dev, const double* g_dev, int M, int J, double alpha, int beta,
                          double* p_dev, void* stream) {
  const std::string me("projet_update_p");
  if (int rc = projet_sizes(me, nsig, rows, frames, J)) return rc;
  if (int rc = projet_model(me, nsig, M, 1, J)) return rc;
  if (int rc = projet_powers(me, alpha, beta)) return rc;
  if (nsig == 0) return 0;
  if (!x_dev || !u_dev || !g_dev || !p_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {x_dev, u_dev, g_dev, p_dev})) return rc;
  if (int rc = iva_disjoint(me, {{p_dev, projet_bytes_p(nsig, J, rows, frames)}, {x_dev, projet_bytes_x(nsig, rows, frames)}, {u_dev, (size_t)M * 16},
                                 {g_dev, (size_t)nsig * M * J * 8}}, 1))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, u_dev, g_dev, p_dev}, &dev, "projet_update_p")) return rc;
  DeviceGuard dg(dev);
  return projet_launch_iterate(x_dev, p_dev, nsig, rows, frames, u_dev, g_dev, M, J, alpha, beta, 1, 0, nullptr, (hipStream_t)stream);
}

int glowk_projet_update_q(const float* x_dev, const double* p_dev, int nsig, int rows, int frames, const double* u_dev, const double* k_dev, int M, int L, int J,
                          double alpha, int beta, double* q_dev, double* g_dev, void* work_dev, size_t work_bytes, void* stream) {
  const std::string me("projet_update_q");
  if (int rc = projet_sizes(me, nsig, rows, frames, J)) return rc;
  if (int rc = projet_model(me, nsig, M, L, J)) return rc;
  if (int rc = projet_powers(me, alpha, beta)) return rc;
  if (nsig == 0) return 0;
  if (!x_dev || !p_dev || !u_dev || !k_dev || !q_dev || !g_dev || !work_dev) return fail("null tensor");
  const size_t need = glowk_projet::work_bytes(nsig, M, J, rows, frames);
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_projet_workspace_bytes says");
  if (int rc = iva_aligned(me, {x_dev, p_dev, u_dev, k_dev, q_dev, g_dev, work_dev})) return rc;
  if (int rc = iva_disjoint(me, {{q_dev, (size_t)nsig * L * J * 8}, {g_dev, (size_t)nsig * M * J * 8}, {work_dev, need}, {p_dev, projet_bytes_p(nsig, J, rows, frames)},
                                 {x_dev, projet_bytes_x(nsig, rows, frames)}, {u_dev, (size_t)M * 16}, {k_dev, (size_t)M * L * 8}}, 3))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, p_dev, u_dev, k_dev, q_dev, g_dev, work_dev}, &dev, "projet_update_q")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = projet_launch_iterate(x_dev, const_cast<double*>(p_dev), nsig, rows, frames, u_dev, g_dev, M, J, alpha, beta, 0, 1, (double*)work_dev, st)) return rc;
  return projet_launch_q((const double*)work_dev, nsig, rows, frames, k_dev, M, L, J, beta, q_dev, g_dev, st);
}

int glowk_projet_fit(const float* x_dev, int nsig, int rows, int frames, const double* u_dev, const double* k_dev, int M, int L, int J, double alpha, int beta,
                     int n_iter, double* p_dev, double* q_dev, double* g_dev, void* work_dev, size_t work_bytes, void* stream) {
  const std::string me("projet_fit");
  if (int rc = projet_sizes(me, nsig, rows, frames, J)) return rc;
  if (int rc = projet_model(me, nsig, M, L, J)) return rc;
  if (int rc = projet_powers(me, alpha, beta)) return rc;
  if (n_iter < 0 || n_iter > glowk_projet::MAX_ITER) return fail(me + ": n_iter must be in [0, 100000]");
  if (nsig == 0) return 0;
  if (!x_dev || !u_dev || !k_dev || !p_dev || !q_dev || !g_dev || !work_dev) return fail("null tensor");
  const size_t need = glowk_projet::work_bytes(nsig, M, J, rows, frames);
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_projet_workspace_bytes says");
  if (int rc = iva_aligned(me, {x_dev, u_dev, k_dev, p_dev, q_dev, g_dev, work_dev})) return rc;
  if (int rc = iva_disjoint(me, {{p_dev, projet_bytes_p(nsig, J, rows, frames)}, {q_dev, (size_t)nsig * L * J * 8}, {g_dev, (size_t)nsig * M * J * 8}, {work_dev, need},
                                 {x_dev, projet_bytes_x(nsig, rows, frames)}, {u_dev, (size_t)M * 16}, {k_dev, (size_t)M * L * 8}}, 4))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, u_dev, k_dev, p_dev, q_dev, g_dev, work_dev}, &dev, "projet_fit")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = projet_launch_gains(k_dev, q_dev, nsig, M, L, J, g_dev, st)) return rc;
  for (int it = 0; it < n_iter; ++it) {
    if (int rc = projet_launch_iterate(x_dev, p_dev, nsig, rows, frames, u_dev, g_dev, M, J, alpha, beta, 1, 1, (double*)work_dev, st)) return rc;
    if (int rc = projet_launch_q((const double*)work_dev, nsig, rows, frames, k_dev, M, L, J, beta, q_dev, g_dev, st)) return rc;
  }
  return 0;
}

int glowk_projet_divergence(const float* x_dev, const double* p_dev, int nsig, int rows, int frames, const double* u_dev, const double* g_dev, int M, int J,
                            double alpha, int beta, double* d_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_projet;
  const std::string me("projet_divergence");
  if (int rc = projet_sizes(me, nsig, rows, frames, J)) return rc;
  if (int rc = projet_model(me, nsig, M, 1, J)) return rc;
  if (int rc = projet_powers(me, alpha, beta)) return rc;
  if (nsig == 0) return 0;
  if (!x_dev || !p_dev || !u_dev || !g_dev || !d_dev || !work_dev) return fail("null tensor");
  const size_t need = glowk_projet::work_bytes(nsig, M, J, rows, frames);
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_projet_workspace_bytes says");
  if (int rc = iva_aligned(me, {x_dev, p_dev, u_dev, g_dev, d_dev, work_dev})) return rc;
  if (int rc = iva_disjoint(me, {{d_dev, (size_t)nsig * 8}, {work_dev, need}, {p_dev, projet_bytes_p(nsig, J, rows, frames)}, {x_dev, projet_bytes_x(nsig, rows, frames)},
                                 {u_dev, (size_t)M * 16}, {g_dev, (size_t)nsig * M * J * 8}}, 2))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, p_dev, u_dev, g_dev, d_dev, work_dev}, &dev, "projet_divergence")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  const int64_t cells = (int64_t)rows * frames;
  const int ng = groups(cells);
  const dim3 grid((unsigned)((int64_t)nsig * ng));
  switch (J) {
#define GLOWK_CASE(j)                                                                                                                              \
  case j:                                                                                                                                          \
    hipLaunchKernelGGL(k_projet_divergence<j>, grid, dim3(THREADS), 0, st, (const float2*)x_dev, p_dev, cells, u_dev, g_dev, M, projet_amode(alpha), alpha / 2.0, beta, \
                       (double*)work_dev);                                                                                                         \
    break;
    GLOWK_PROJET_EACH_J(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_projet_divergence");
  hipLaunchKernelGGL(k_projet_divergence_sum, dim3((unsigned)((nsig + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, (const double*)work_dev, nsig, ng, d_dev);
  LAUNCHCHK("k_projet_divergence_sum");
  return 0;
}

int glowk_projet_separate(const float* x_dev, const double* p_dev, int nsig, int rows, int frames, const double* u_dev, const double* up_dev, const double* g_dev,
                          int M, int J, float* y_dev, void* stream) {
  using namespace glowk_projet;
  const std::string me("projet_separate");
  if (int rc = projet_sizes(me, nsig, rows, frames, J)) return rc;
  if (int rc = projet_model(me, nsig, M, 1, J)) return rc;
  if (nsig == 0) return 0;
  if (!x_dev || !p_dev || !u_dev || !up_dev || !g_dev || !y_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {x_dev, p_dev, u_dev, up_dev, g_dev, y_dev})) return rc;
  if (int rc = iva_disjoint(me, {{y_dev, projet_bytes_p(nsig, J, rows, frames) * 2}, {x_dev, projet_bytes_x(nsig, rows, frames)}, {p_dev, projet_bytes_p(nsig, J, rows, frames)},
                                 {u_dev, (size_t)M * 16}, {up_dev, (size_t)M * 16}, {g_dev, (size_t)nsig * M * J * 8}}, 1))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, p_dev, u_dev, up_dev, g_dev, y_dev}, &dev, "projet_separate")) return rc;
  DeviceGuard dg(dev);
  const int64_t cells = (int64_t)rows * frames;
  const int blocks = (int)((cells + THREADS - 1) / THREADS);
  const dim3 grid((unsigned)((int64_t)nsig * blocks));
  switch (J) {
#define GLOWK_CASE(j)                                                                                                                                   \
  case j:                                                                                                                                               \
    hipLaunchKernelGGL(k_projet_separate<j>, grid, dim3(THREADS), 0, (hipStream_t)stream, (const float2*)x_dev, p_dev, cells, blocks, u_dev, up_dev, g_dev, M, \
                       (float2*)y_dev);                                                                                                                 \
    break;
    GLOWK_PROJET_EACH_J(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_projet_separate");
  return 0;
}

// ---- clustering: a weighted Gaussian mixture over time-frequency cells; the moments on the fp64 matrix cores (glowk_cluster.h) ---------------
namespace {
int cluster_sizes(const std::string& w, int nsig, int D, int J, int rows, int frames) {
  using namespace glowk_cluster;
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (rows < 1 || rows > MAX_ROWS) return fail(w + ": rows must be in [1, 4096]");
  if (frames < 1 || frames > MAX_FRAMES) return fail(w + ": frames must be in [1, 32768]");
  if (D < 1 || D > MAX_D) return fail(w + ": the feature count D must be in [1, 8]");
  if (J < 1 || J > MAX_J) return fail(w + ": the cluster count J must be in [1, 8]");
  if (!sizes_ok(nsig, D, J, rows, frames)) return fail(w + ": nsig * max(D, J) * rows * frames must be at most 2^31 - 1");
  return 0;
}
int cluster_reg(const std::string& w, double reg) {
  if (!(reg >= glowk_cluster::MIN_REG) || !std::isfinite(reg)) return fail(w + ": reg_covar must be finite and at least 2^-40");
  return 0;
}
int cluster_aligned(const std::string& w, std::initializer_list<const void*> f64, std::initializer_list<const void*> f32) {
  for (const void* p : f64)
    if ((uintptr_t)p % 8) return fail(w + ": the float64 tensors and the workspace must be aligned to 8 bytes");
  for (const void* p : f32)
    if ((uintptr_t)p % 4) return fail(w + ": the float32 and int32 tensors must be aligned to 4 bytes");
  return 0;
}
// the parts of work_dev
struct ClusterWork {
  double *partial, *stats, *cons, *ctl;
};
ClusterWork cluster_work(void* work, int nsig, int D, int J, int rows, int frames) {
  using namespace glowk_cluster;
  ClusterWork cw;
  cw.partial = (double*)work;
  cw.stats = cw.partial + work_partials(nsig, D, J, rows, frames);
  cw.cons = cw.stats + (size_t)nsig * partial_doubles(D, J);
  cw.ctl = cw.cons + (size_t)nsig * cons_doubles(D, J);
  return cw;
}
size_t cluster_bytes_f(int nsig, int D, int rows, int frames) { return (size_t)nsig * D * rows * frames * 4; }
size_t cluster_bytes_state(int nsig, int D, int J) { return (size_t)nsig * J * D * D * 8; }

#define GLOWK_CLUSTER_EACH_D(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

// the statistics pass: J clusters from the constants (MODE_EM), or one cluster with r = 1 about the constants' origin or about 0
int cluster_launch_stats(const float* f, const float* w, int nsig, int D, int J, int rows, int frames, int mode, const double* cons, int cons_stride, double* partial,
                         hipStream_t st) {
  using namespace glowk_cluster;
  const int64_t cells = (int64_t)rows * frames;
  const dim3 grid((unsigned)((int64_t)nsig * groups(cells)));
  switch (D) {
#define GLOWK_CASE(d)                                                                                                          \
  case d:                                                                                                                      \
    hipLaunchKernelGGL(k_cluster_stats<d>, grid, dim3(THREADS), 0, st, f, w, cells, J, mode, cons, cons_stride, partial);      \
    break;
    GLOWK_CLUSTER_EACH_D(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_cluster_stats");
  return 0;
}
// pass 0: W and o (and the origin of the constants)
int cluster_launch_pass0(const float* f, const float* w, int nsig, int D, int J, int rows, int frames, double* origin, double* total, int32_t* status,
                         const ClusterWork& cw, hipStream_t st) {
  using namespace glowk_cluster;
  const int ng = groups((int64_t)rows * frames);
  if (int rc = cluster_launch_stats(f, w, nsig, D, 1, rows, frames, MODE_UNIT_ZERO, cw.cons, cons_doubles(D, J), cw.partial, st)) return rc;
  hipLaunchKernelGGL(k_cluster_origin, dim3((unsigned)nsig), dim3(THREADS), 0, st, (const double*)cw.partial, ng, D, J, origin, total, status, cw.cons);
  LAUNCHCHK("k_cluster_origin");
  return 0;
}
// the start from the moments about o
int cluster_launch_start(const float* f, const float* w, int nsig, int D, int J, int rows, int frames, const double* z, double reg, const double* total, double* pi,
                         double* mu, double* sigma, int32_t* status, const ClusterWork& cw, hipStream_t st) {
  using namespace glowk_cluster;
  const int ng = groups((int64_t)rows * frames);
  if (int rc = cluster_launch_stats(f, w, nsig, D, 1, rows, frames, MODE_UNIT, cw.cons, cons_doubles(D, J), cw.partial, st)) return rc;
  hipLaunchKernelGGL(k_cluster_start, dim3((unsigned)nsig), dim3(THREADS), 0, st, (const double*)cw.partial, ng, D, J, z, reg, total, pi, mu, sigma, status, cw.cons);
  LAUNCHCHK("k_cluster_start");
  return 0;
}
int cluster_launch_prepare(int nsig, int D, int J, const double* pi, const double* mu, const double* sigma, const double* origin, const double* total,
                           int32_t* status, double* cons, hipStream_t st) {
  using namespace glowk_cluster;
  hipLaunchKernelGGL(k_cluster_prepare, dim3((unsigned)nsig), dim3(THREADS), 0, st, D, J, pi, mu, sigma, origin, total, status, cons);
  LAUNCHCHK("k_cluster_prepare");
  return 0;
}
int cluster_launch_update(const double* partial, int ngroups, int nsig, int D, int J, double reg, double tol, int it, double* pi, double* mu, double* sigma,
                          const double* origin, const double* total, int32_t* status, double* cons, double* ctl, double* ll, int ll_stride, int32_t* iters,
                          hipStream_t st) {
  using namespace glowk_cluster;
  hipLaunchKernelGGL(k_cluster_update, dim3((unsigned)nsig), dim3(THREADS), 0, st, partial, ngroups, D, J, reg, tol, it, pi, mu, sigma, origin, total, status, cons,
                     ctl, ll, ll_stride, iters);
  LAUNCHCHK("k_cluster_update");
  return 0;
}
}  // namespace

size_t glowk_cluster_work_bytes(int nsig, int D, int J, int rows, int frames) {
  using namespace glowk_cluster;
  if (nsig < 1 || !sizes_ok(nsig, D, J, rows, frames)) return 0;
  return work_bytes(nsig, D, J, rows, frames);
}

int glowk_cluster_init(const float* f_dev, const float* w_dev, int nsig, int D, int J, int rows, int frames, const double* z_dev, double reg_covar, double* pi_dev,
                       double* mu_dev, double* sigma_dev, double* origin_dev, double* total_dev, int32_t* status_dev, void* work_dev, size_t work_bytes,
                       void* stream) {
  const std::string me("cluster_init");
  if (int rc = cluster_sizes(me, nsig, D, J, rows, frames)) return rc;
  if (int rc = cluster_reg(me, reg_covar)) return rc;
  if (nsig == 0) return 0;
  if (!f_dev || !w_dev || !z_dev || !pi_dev || !mu_dev || !sigma_dev || !origin_dev || !total_dev || !status_dev || !work_dev) return fail("null tensor");
  const size_t need = glowk_cluster::work_bytes(nsig, D, J, rows, frames);
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_cluster_work_bytes says");
  if (int rc = cluster_aligned(me, {z_dev, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, work_dev}, {f_dev, w_dev, status_dev})) return rc;
  if (int rc = iva_disjoint(me, {{pi_dev, (size_t)nsig * J * 8}, {mu_dev, (size_t)nsig * J * D * 8}, {sigma_dev, cluster_bytes_state(nsig, D, J)},
                                 {origin_dev, (size_t)nsig * D * 8}, {total_dev, (size_t)nsig * 8}, {status_dev, (size_t)nsig * 4}, {work_dev, need},
                                 {f_dev, cluster_bytes_f(nsig, D, rows, frames)}, {w_dev, cluster_bytes_f(nsig, 1, rows, frames)}, {z_dev, (size_t)J * 8}}, 7))
    return rc;
  int dev;
  if (int rc = audio_device({f_dev, w_dev, z_dev, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, status_dev, work_dev}, &dev, "cluster_init")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  const ClusterWork cw = cluster_work(work_dev, nsig, D, J, rows, frames);
  if (int rc = cluster_launch_pass0(f_dev, w_dev, nsig, D, J, rows, frames, origin_dev, total_dev, status_dev, cw, st)) return rc;
  return cluster_launch_start(f_dev, w_dev, nsig, D, J, rows, frames, z_dev, reg_covar, total_dev, pi_dev, mu_dev, sigma_dev, status_dev, cw, st);
}

int glowk_cluster_stats(const float* f_dev, const float* w_dev, int nsig, int D, int J, int rows, int frames, const double* pi_dev, const double* mu_dev,
                        const double* sigma_dev, const double* origin_dev, const double* total_dev, double* stats_dev, int32_t* status_dev, void* work_dev,
                        size_t work_bytes, void* stream) {
  using namespace glowk_cluster;
  const std::string me("cluster_stats");
  if (int rc = cluster_sizes(me, nsig, D, J, rows, frames)) return rc;
  if (nsig == 0) return 0;
  if (!f_dev || !w_dev || !pi_dev || !mu_dev || !sigma_dev || !origin_dev || !total_dev || !stats_dev || !status_dev || !work_dev) return fail("null tensor");
  const size_t need = glowk_cluster::work_bytes(nsig, D, J, rows, frames);
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_cluster_work_bytes says");
  if (int rc = cluster_aligned(me, {pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, stats_dev, work_dev}, {f_dev, w_dev, status_dev})) return rc;
  if (int rc = iva_disjoint(me, {{stats_dev, (size_t)nsig * partial_doubles(D, J) * 8}, {status_dev, (size_t)nsig * 4}, {work_dev, need}, {pi_dev, (size_t)nsig * J * 8},
                                 {mu_dev, (size_t)nsig * J * D * 8}, {sigma_dev, cluster_bytes_state(nsig, D, J)}, {origin_dev, (size_t)nsig * D * 8},
                                 {total_dev, (size_t)nsig * 8}, {f_dev, cluster_bytes_f(nsig, D, rows, frames)}, {w_dev, cluster_bytes_f(nsig, 1, rows, frames)}}, 3))
    return rc;
  int dev;
  if (int rc = audio_device({f_dev, w_dev, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, stats_dev, status_dev, work_dev}, &dev, "cluster_stats")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  const ClusterWork cw = cluster_work(work_dev, nsig, D, J, rows, frames);
  if (int rc = cluster_launch_prepare(nsig, D, J, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, status_dev, cw.cons, st)) return rc;
  if (int rc = cluster_launch_stats(f_dev, w_dev, nsig, D, J, rows, frames, MODE_EM, cw.cons, cons_doubles(D, J), cw.partial, st)) return rc;
  hipLaunchKernelGGL(k_cluster_sum, dim3((unsigned)nsig), dim3(THREADS), 0, st, (const double*)cw.partial, groups((int64_t)rows * frames), (int)partial_doubles(D, J),
                     stats_dev);
  LAUNCHCHK("k_cluster_sum");
  return 0;
}

int glowk_cluster_update(const double* stats_dev, int nsig, int D, int J, double reg_covar, double* pi_dev, double* mu_dev, double* sigma_dev,
                         const double* origin_dev, const double* total_dev, double* ll_dev, int32_t* status_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_cluster;
  const std::string me("cluster_update");
  if (int rc = cluster_sizes(me, nsig, D, J, 1, 1)) return rc;
  if (int rc = cluster_reg(me, reg_covar)) return rc;
  if (nsig == 0) return 0;
  if (!stats_dev || !pi_dev || !mu_dev || !sigma_dev || !origin_dev || !total_dev || !ll_dev || !status_dev || !work_dev) return fail("null tensor");
  const size_t need = (size_t)nsig * cons_doubles(D, J) * 8;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than 8 nsig (D + J (1 + D + D D))");
  if (int rc = cluster_aligned(me, {stats_dev, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, ll_dev, work_dev}, {status_dev})) return rc;
  if (int rc = iva_disjoint(me, {{pi_dev, (size_t)nsig * J * 8}, {mu_dev, (size_t)nsig * J * D * 8}, {sigma_dev, cluster_bytes_state(nsig, D, J)},
                                 {ll_dev, (size_t)nsig * 8}, {status_dev, (size_t)nsig * 4}, {work_dev, need}, {stats_dev, (size_t)nsig * partial_doubles(D, J) * 8},
                                 {origin_dev, (size_t)nsig * D * 8}, {total_dev, (size_t)nsig * 8}}, 6))
    return rc;
  int dev;
  if (int rc = audio_device({stats_dev, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, ll_dev, status_dev, work_dev}, &dev, "cluster_update")) return rc;
  DeviceGuard dg(dev);
  return cluster_launch_update(stats_dev, 1, nsig, D, J, reg_covar, 0.0, 0, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, status_dev, (double*)work_dev, nullptr,
                               ll_dev, 1, nullptr, (hipStream_t)stream);
}

int glowk_cluster_fit(const float* f_dev, const float* w_dev, int nsig, int D, int J, int rows, int frames, const double* z_dev, double reg_covar, int n_iter,
                      double tol, double* pi_dev, double* mu_dev, double* sigma_dev, double* origin_dev, double* total_dev, double* ll_dev, int32_t* iters_dev,
                      int32_t* status_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_cluster;
  const std::string me("cluster_fit");
  if (int rc = cluster_sizes(me, nsig, D, J, rows, frames)) return rc;
  if (int rc = cluster_reg(me, reg_covar)) return rc;
  if (n_iter < 0 || n_iter > MAX_ITER) return fail(me + ": n_iter must be in [0, 100000]");
  if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(me + ": tol must be finite and at least 0");
  if (nsig == 0) return 0;
  if (!f_dev || !w_dev || !pi_dev || !mu_dev || !sigma_dev || !origin_dev || !total_dev || !iters_dev || !status_dev || !work_dev || (n_iter > 0 && !ll_dev))
    return fail("null tensor");
  const size_t need = glowk_cluster::work_bytes(nsig, D, J, rows, frames);
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_cluster_work_bytes says");
  if (int rc = cluster_aligned(me, {z_dev, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, ll_dev, work_dev}, {f_dev, w_dev, iters_dev, status_dev})) return rc;
  if (int rc = iva_disjoint(me, {{pi_dev, (size_t)nsig * J * 8}, {mu_dev, (size_t)nsig * J * D * 8}, {sigma_dev, cluster_bytes_state(nsig, D, J)},
                                 {origin_dev, (size_t)nsig * D * 8}, {total_dev, (size_t)nsig * 8}, {ll_dev, (size_t)nsig * n_iter * 8}, {iters_dev, (size_t)nsig * 4},
                                 {status_dev, (size_t)nsig * 4}, {work_dev, need}, {f_dev, cluster_bytes_f(nsig, D, rows, frames)},
                                 {w_dev, cluster_bytes_f(nsig, 1, rows, frames)}, {z_dev, (size_t)J * 8}}, 9))
    return rc;
  int dev;
  if (int rc = audio_device({f_dev, w_dev, z_dev, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, ll_dev, iters_dev, status_dev, work_dev}, &dev, "cluster_fit")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  const ClusterWork cw = cluster_work(work_dev, nsig, D, J, rows, frames);
  const int ng = groups((int64_t)rows * frames);
  if (int rc = cluster_launch_pass0(f_dev, w_dev, nsig, D, J, rows, frames, origin_dev, total_dev, status_dev, cw, st)) return rc;
  if (z_dev) {
    if (int rc = cluster_launch_start(f_dev, w_dev, nsig, D, J, rows, frames, z_dev, reg_covar, total_dev, pi_dev, mu_dev, sigma_dev, status_dev, cw, st)) return rc;
  } else {
    if (int rc = cluster_launch_prepare(nsig, D, J, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, status_dev, cw.cons, st)) return rc;
  }
  hipLaunchKernelGGL(k_cluster_reset, dim3((unsigned)((nsig + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, nsig, cw.ctl, iters_dev);
  LAUNCHCHK("k_cluster_reset");
  for (int it = 0; it < n_iter; ++it) {
    if (int rc = cluster_launch_stats(f_dev, w_dev, nsig, D, J, rows, frames, MODE_EM, cw.cons, cons_doubles(D, J), cw.partial, st)) return rc;
    if (int rc = cluster_launch_update(cw.partial, ng, nsig, D, J, reg_covar, tol, it, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, status_dev, cw.cons, cw.ctl,
                                       ll_dev, n_iter, iters_dev, st))
      return rc;
  }
  return 0;
}

int glowk_cluster_posteriors(const float* f_dev, int nsig, int D, int J, int rows, int frames, const double* pi_dev, const double* mu_dev, const double* sigma_dev,
                             const double* origin_dev, const double* total_dev, const float* x_dev, int C, float* mask_dev, float* y_dev, int32_t* status_dev,
                             void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_cluster;
  const std::string me("cluster_posteriors");
  if (int rc = cluster_sizes(me, nsig, D, J, rows, frames)) return rc;
  if (x_dev && (C < 1 || C > 2)) return fail(me + ": the channel count C must be 1 or 2");
  if (x_dev && (int64_t)nsig * J * C * rows * frames > MAX_ELEMENTS) return fail(me + ": nsig * J * C * rows * frames must be at most 2^31 - 1");
  if ((x_dev == nullptr) != (y_dev == nullptr)) return fail(me + ": x_dev and y_dev go together");
  if (nsig == 0) return 0;
  if (!f_dev || !pi_dev || !mu_dev || !sigma_dev || !origin_dev || !total_dev || !mask_dev || !status_dev || !work_dev) return fail("null tensor");
  const size_t need = (size_t)nsig * cons_doubles(D, J) * 8;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than 8 nsig (D + J (1 + D + D D))");
  if (int rc = cluster_aligned(me, {pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, work_dev, x_dev, y_dev}, {f_dev, mask_dev, status_dev})) return rc;
  const size_t cells = (size_t)rows * frames;
  if (int rc = iva_disjoint(me, {{mask_dev, (size_t)nsig * J * cells * 4}, {y_dev, y_dev ? (size_t)nsig * J * C * cells * 8 : 0}, {status_dev, (size_t)nsig * 4},
                                 {work_dev, need}, {f_dev, cluster_bytes_f(nsig, D, rows, frames)}, {x_dev, x_dev ? (size_t)nsig * C * cells * 8 : 0},
                                 {pi_dev, (size_t)nsig * J * 8}, {mu_dev, (size_t)nsig * J * D * 8}, {sigma_dev, cluster_bytes_state(nsig, D, J)},
                                 {origin_dev, (size_t)nsig * D * 8}, {total_dev, (size_t)nsig * 8}}, 4))
    return rc;
  int dev;
  if (int rc = audio_device({f_dev, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, x_dev, mask_dev, y_dev, status_dev, work_dev}, &dev, "cluster_posteriors")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = cluster_launch_prepare(nsig, D, J, pi_dev, mu_dev, sigma_dev, origin_dev, total_dev, status_dev, (double*)work_dev, st)) return rc;
  const int blocks = (int)((cells + THREADS - 1) / THREADS);
  const dim3 grid((unsigned)((int64_t)nsig * blocks));
  switch (D) {
#define GLOWK_CASE(d)                                                                                                                                       \
  case d:                                                                                                                                                   \
    hipLaunchKernelGGL(k_cluster_posteriors<d>, grid, dim3(THREADS), 0, st, f_dev, (int64_t)cells, blocks, J, (const double*)work_dev, (const float2*)x_dev, C, \
                       mask_dev, (float2*)y_dev);                                                                                                           \
    break;
    GLOWK_CLUSTER_EACH_D(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_cluster_posteriors");
  return 0;
}

int glowk_cluster_spatial_features(const float* x_dev, int nsig, int rows, int frames, int delay, double max_delay, double p, float* feat_dev, float* w_dev,
                                   void* stream) {
  using namespace glowk_cluster;
  const std::string me("cluster_spatial_features");
  if (int rc = cluster_sizes(me, nsig, 2, 1, rows, frames)) return rc;
  if (delay != 0 && delay != 1) return fail(me + ": delay must be 0 or 1");
  if (!(max_delay > 0.0) || !std::isfinite(max_delay)) return fail(me + ": max_delay must be finite and positive");
  if (!(p > 0.0) || !std::isfinite(p)) return fail(me + ": p must be finite and positive");
  if (nsig == 0) return 0;
  if (!x_dev || !feat_dev || !w_dev) return fail("null tensor");
  if (int rc = cluster_aligned(me, {x_dev}, {feat_dev, w_dev})) return rc;
  const size_t cells = (size_t)rows * frames;
  if (int rc = iva_disjoint(me, {{feat_dev, (size_t)nsig * (1 + delay) * cells * 4}, {w_dev, (size_t)nsig * cells * 4}, {x_dev, (size_t)nsig * 2 * cells * 8}}, 2)) return rc;
  int dev;
  if (int rc = audio_device({x_dev, feat_dev, w_dev}, &dev, "cluster_spatial_features")) return rc;
  DeviceGuard dg(dev);
  const int64_t total = (int64_t)cells * nsig;
  hipLaunchKernelGGL(k_cluster_spatial, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, (const float2*)x_dev, total, rows,
                     frames, delay, max_delay, p, feat_dev, w_dev);
  LAUNCHCHK("k_cluster_spatial");
  return 0;
}

// ---- kernel additive modelling: sparse-kernel medians with back-fitting (glowk_kam.h) ------------------------------------------------------
namespace {
int kam_sizes(const std::string& w, int nsig, int rows, int frames, int J) {
  using namespace glowk_kam;
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (rows < 1 || rows > MAX_ROWS) return fail(w + ": rows must be in [1, 4096]");
  if (frames < 1 || frames > MAX_FRAMES) return fail(w + ": frames must be in [1, 32768]");
  if (J < 1 || J > MAX_J) return fail(w + ": J must be in [1, 8]");
  if (!sizes_ok(nsig, rows, frames, J)) return fail(w + ": nsig * J * rows * frames must be at most 2^31 - 1");
  return 0;
}
int kam_offsets(const std::string& w, const int32_t* offsets, int n) {
  using namespace glowk_kam;
  if (n < 1 || n > MAX_N) return fail(w + ": n, the number of offsets, must be in [1, 127]");
  if (!offsets) return fail(w + ": the offset table is null");
  if (!offsets_ok(offsets, n)) return fail(w + ": every offset needs |d_row| <= 4095 and |d_frame| <= 32767");
  return 0;
}
int kam_power(const std::string& w, float power) {
  if (!(power > 0.0f) || !std::isfinite(power)) return fail(w + ": power must be finite and > 0");
  return 0;
}
// one filter over an offset table; signals s_stride / out_stride floats apart
int kam_launch_median(const float* s, int64_t s_stride, int nsig, int rows, int frames, const int32_t* offsets, int n, float* out, int64_t out_stride,
                      hipStream_t st) {
  using namespace glowk_kam;
  const dim3 grid((unsigned)blocks(nsig, rows, frames, n)), block(waves(n) * 64);
  if (candidates(n) == 8)
    hipLaunchKernelGGL(k_kam_median<8>, grid, block, lds_bytes(n), st, s, s_stride, rows, frames, units(nsig, rows, frames), pack(offsets, n), n, out, out_stride);
  else
    hipLaunchKernelGGL(k_kam_median<4>, grid, block, lds_bytes(n), st, s, s_stride, rows, frames, units(nsig, rows, frames), pack(offsets, n), n, out, out_stride);
  LAUNCHCHK("k_kam_median");
  return 0;
}
int kam_launch_backfit(const float* v, const float* a, int nsig, int J, int64_t n, float power, float* p, float* mask, hipStream_t st) {
  using namespace glowk_kam;
  const int64_t total = (int64_t)nsig * n;
  switch (J) {
#define GLOWK_CASE(j) case j: hipLaunchKernelGGL(k_kam_backfit<j>, dim3(stride_grid(total)), dim3(256), 0, st, v, a, total, n, power, p, mask); break;
    GLOWK_KAM_EACH_J(GLOWK_CASE)
#undef GLOWK_CASE
  }
  LAUNCHCHK("k_kam_backfit");
  return 0;
}
// the models of glowk_kam_fit: 0 or an error; has_idx: a source has a frame-neighbour model
int kam_models(const std::string& w, int nsig, int frames, int J, const int32_t* model_n, const int32_t* offsets, const int32_t* model_k, bool* has_idx) {
  *has_idx = false;
  if (!model_n || !model_k) return fail(w + ": model_n and model_k are null");
  size_t at = 0;
  for (int j = 0; j < J; ++j) {
    if ((model_n[j] != 0) == (model_k[j] != 0)) return fail(w + ": every source needs exactly one of model_n (an offset table) and model_k (a frame-neighbour tensor)");
    if (model_n[j]) {
      if (int rc = kam_offsets(w, offsets ? offsets + 2 * at : nullptr, model_n[j])) return rc;
      at += (size_t)model_n[j];
    } else {
      if (int rc = nn_ranges(w.c_str(), nsig, 1, frames, model_k[j])) return rc;
      *has_idx = true;
    }
  }
  return 0;
}
}  // namespace

int glowk_kam_median(const float* s_dev, int nsig, int rows, int frames, const int32_t* offsets, int n, float* out_dev, void* stream) {
  const std::string me("kam_median");
  if (int rc = kam_sizes(me, nsig, rows, frames, 1)) return rc;
  if (int rc = kam_offsets(me, offsets, n)) return rc;
  if (nsig == 0) return 0;                     // nothing to read or write: an empty tensor has no storage, its pointer may be null
  if (!s_dev || !out_dev) return fail("null tensor");
  const size_t cells = (size_t)nsig * rows * frames;
  if (floats_overlap(s_dev, cells, out_dev, cells)) return fail(me + ": out_dev must not be s_dev (the filter does not run in place)");
  int dev;
  if (int rc = audio_device({s_dev, out_dev}, &dev, "kam_median")) return rc;
  DeviceGuard dg(dev);
  const int64_t plane = (int64_t)rows * frames;
  return kam_launch_median(s_dev, plane, nsig, rows, frames, offsets, n, out_dev, plane, (hipStream_t)stream);
}

int glowk_kam_backfit(const float* v_dev, const float* a_dev, int nsig, int J, size_t n, float power, float* p_dev, float* mask_dev, void* stream) {
  using namespace glowk_kam;
  const std::string me("kam_backfit");
  if (nsig < 0 || nsig > MAX_SIG) return fail(me + ": nsig must be in [0, 65535]");
  if (J < 1 || J > MAX_J) return fail(me + ": J must be in [1, 8]");
  if (n > (size_t)MAX_ELEMENTS || (uint64_t)nsig * J * n > (uint64_t)MAX_ELEMENTS) return fail(me + ": nsig * J * n must be at most 2^31 - 1");
  if (int rc = kam_power(me, power)) return rc;
  if (nsig == 0 || n == 0) return 0;
  if (!v_dev || !a_dev || !p_dev) return fail("null tensor");
  const size_t all = (size_t)nsig * J * n * 4;
  if (int rc = iva_disjoint(me, {{p_dev, all}, {mask_dev, mask_dev ? all : 0}, {a_dev, all}, {v_dev, (size_t)nsig * n * 4}}, 2)) return rc;
  int dev;
  if (int rc = audio_device({v_dev, a_dev, p_dev, mask_dev}, &dev, "kam_backfit")) return rc;
  DeviceGuard dg(dev);
  return kam_launch_backfit(v_dev, a_dev, nsig, J, (int64_t)n, power, p_dev, mask_dev, (hipStream_t)stream);
}

size_t glowk_kam_work_bytes(int nsig, int rows, int frames, int J, const int32_t* model_k) {
  using namespace glowk_kam;
  if (nsig < 1 || !sizes_ok(nsig, rows, frames, J) || !model_k) return 0;
  bool has_idx = false;
  for (int j = 0; j < J; ++j) {
    if (model_k[j] < 0 || model_k[j] > glowk_repet::MAX_K) return 0;
    has_idx = has_idx || model_k[j] > 0;
  }
  return work_bytes(nsig, rows, frames, J, has_idx ? nn_work_bytes(1, rows, frames) : 0);
}

int glowk_kam_fit(const float* v_dev, int nsig, int rows, int frames, int J, const int32_t* model_n, const int32_t* offsets, const int32_t* model_k,
                  const int32_t* const* idx_dev, int n_iter, float power, float* p_dev, float* mask_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_kam;
  const std::string me("kam_fit");
  if (int rc = kam_sizes(me, nsig, rows, frames, J)) return rc;
  bool has_idx;
  if (int rc = kam_models(me, nsig, frames, J, model_n, offsets, model_k, &has_idx)) return rc;
  if (n_iter < 1 || n_iter > MAX_ITER) return fail(me + ": n_iter must be in [1, 100]");
  if (int rc = kam_power(me, power)) return rc;
  if (nsig == 0) return 0;
  if (!v_dev || !p_dev || !work_dev) return fail("null tensor");
  if (has_idx && !idx_dev) return fail(me + ": idx_dev is null");
  const size_t nn_bytes = has_idx ? nn_work_bytes(1, rows, frames) : 0, need = glowk_kam::work_bytes(nsig, rows, frames, J, nn_bytes);
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_kam_work_bytes says");
  const size_t cells = (size_t)rows * frames, all = (size_t)nsig * J * cells * 4;
  if (int rc = iva_disjoint(me, {{p_dev, all}, {mask_dev, mask_dev ? all : 0}, {work_dev, need}, {v_dev, (size_t)nsig * cells * 4}}, 3)) return rc;
  for (int j = 0; j < J; ++j)
    if (model_k[j]) {
      if (!idx_dev[j]) return fail(me + ": a frame-neighbour model's tensor is null");
      const size_t nk = (size_t)nsig * frames * model_k[j] * 4;
      if (bytes_overlap(idx_dev[j], nk, p_dev, all) || bytes_overlap(idx_dev[j], nk, work_dev, need) || (mask_dev && bytes_overlap(idx_dev[j], nk, mask_dev, all)))
        return fail(me + ": a tensor the call writes overlaps another of its tensors");
    }
  int dev;
  if (int rc = audio_device({v_dev, p_dev, mask_dev, work_dev}, &dev, "kam_fit")) return rc;
  for (int j = 0; j < J; ++j) {
    int dj;
    if (!model_k[j]) continue;
    if (int rc = audio_device({idx_dev[j]}, &dj, "kam_fit")) return rc;
    if (dj != dev) return fail(me + ": the tensors are on different devices");
  }
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  float* a = (float*)work_dev;
  void* nn_work = (char*)work_dev + work_a_bytes(nsig, rows, frames, J);
  const int64_t plane = (int64_t)cells, group = (int64_t)J * plane;
  for (int it = 0; it < n_iter; ++it) {
    // iteration 0 filters the mixture itself (P_j = V for every j), later ones source j of p_dev; A_j goes to source j of the workspace
    const float* src = it == 0 ? v_dev : p_dev;
    const int64_t src_stride = it == 0 ? plane : group;
    size_t at = 0;
    for (int j = 0; j < J; ++j) {
      const int64_t src_off = it == 0 ? 0 : j * plane;
      if (model_n[j]) {
        if (int rc = kam_launch_median(src + src_off, src_stride, nsig, rows, frames, offsets + 2 * at, model_n[j], a + j * plane, group, st)) return rc;
        at += (size_t)model_n[j];
      } else {
        for (int sg = 0; sg < nsig; ++sg)      // glowk_nn_median wants contiguous signals: one signal at a time
          if (int rc = glowk_nn_median(src + src_off + sg * src_stride, idx_dev[j] + (size_t)sg * frames * model_k[j], 1, rows, frames, model_k[j],
                                       a + sg * group + j * plane, nn_work, nn_bytes, stream))
            return rc;
      }
    }
    if (int rc = kam_launch_backfit(v_dev, a, nsig, J, plane, power, p_dev, it == n_iter - 1 ? mask_dev : nullptr, st)) return rc;
  }
  return 0;
}

// ---- convolutive NMF: K patches of Tw spectra, NMF on K Tw stacked components with tied shifts (glowk_nmfd.h) ------------------------------
namespace {
// the ranges every glowk_nmfd_* call shares; 0 or an error.  The stacked problem (rows, frames, K Tw) is held to the NMF ranges.
int nmfd_ranges(const std::string& w, int nsig, int rows, int frames, int K, int Tw) {
  using namespace glowk_nmfd;
  if (K < 1 || K > glowk_nmf::MAX_K) return fail(w + ": K must be in [1, 128]");
  if (Tw < 1 || Tw > MAX_TW) return fail(w + ": Tw must be in [1, 32]");
  if (K * Tw > MAX_STACK) return fail(w + ": K * Tw must be at most 128");
  return nmf_ranges(w, nsig, rows, frames, K * Tw);
}
}  // namespace

size_t glowk_nmfd_workspace_bytes(int nsig, int rows, int frames, int K, int Tw) {
  if (nmfd_ranges("nmfd_workspace_bytes", nsig, rows, frames, K, Tw)) return 0;
  return glowk_nmfd::nmfd_work_bytes(nsig, rows, frames, K, Tw);
}

int glowk_nmfd_fit(const float* v_dev, int nsig, int rows, int frames, float* w_dev, int nw, float* h_dev, int K, int Tw, int beta, int n_iter, int update_w,
                   void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_nmfd;
  const std::string me("nmfd_fit");
  if (int rc = nmfd_ranges(me, nsig, rows, frames, K, Tw)) return rc;
  if (int rc = nmf_model(me, nsig, nw, beta)) return rc;
  if (n_iter < 0 || n_iter > glowk_nmf::MAX_ITER) return fail(me + ": n_iter must be in [0, 100000]");
  if (update_w < 0 || update_w > 2) return fail(me + ": update_w must be 0 (H alone), 1 (W, then H) or 2 (W alone)");
  if (update_w && nw != nsig) return fail(me + ": a dictionary shared by several signals cannot be updated (nw = 1 needs update_w = 0)");
  if (nsig == 0 || n_iter == 0) return 0;
  if (!v_dev || !w_dev || !h_dev || !work_dev) return fail("null tensor");
  const int KS = K * Tw;
  const NmfPlan p = nmf_plan(rows, frames, KS);
  const size_t need_w = update_w ? (size_t)nmf_w_part_floats(p, rows, KS) * 4 : 0, need_h = update_w != 2 ? (size_t)nmfd_plane_floats(KS, frames) * 4 : 0;
  const size_t need = (size_t)nsig * (need_w > need_h ? need_w : need_h);
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_nmfd_workspace_bytes says");
  if ((uintptr_t)work_dev % 8) return fail(me + ": work_dev must be aligned to 8 bytes");
  const size_t nv = (size_t)nsig * rows * frames * 4, nww = (size_t)nw * rows * KS * 4, nh = (size_t)nsig * K * frames * 4;
  if (bytes_overlap(v_dev, nv, w_dev, nww) || bytes_overlap(v_dev, nv, h_dev, nh) || bytes_overlap(w_dev, nww, h_dev, nh))
    return fail(me + ": V, W and H must not overlap");
  if (bytes_overlap(work_dev, need, v_dev, nv) || bytes_overlap(work_dev, need, w_dev, nww) || bytes_overlap(work_dev, need, h_dev, nh))
    return fail(me + ": work_dev must not overlap the tensors");
  int dev;
  if (int rc = audio_device({v_dev, w_dev, h_dev, work_dev}, &dev, "nmfd_fit")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)work_dev;
  const int64_t wstride = nw == 1 ? 0 : (int64_t)rows * KS, per_sig = (int64_t)rows * KS, total = (int64_t)nsig * per_sig, htotal = (int64_t)nsig * K * frames;
  const dim3 gw((unsigned)((int64_t)nsig * p.rtiles * p.nch)), gh((unsigned)((int64_t)nsig * p.ftiles)), gf((unsigned)((total + 255) / 256)),
      ghf((unsigned)((htotal + 255) / 256));
  for (int it = 0; it < n_iter; ++it) {
    if (update_w) {
      switch (p.kt) {
#define GLOWK_CASE(n) \
  case n: hipLaunchKernelGGL(k_nmfd_update_w<n>, gw, dim3(256), 0, st, v_dev, (const float*)w_dev, (const float*)h_dev, rows, frames, K, Tw, p, beta, part); break;
        GLOWK_NMF_EACH_KT(GLOWK_CASE)
#undef GLOWK_CASE
      }
      LAUNCHCHK("k_nmfd_update_w");
      hipLaunchKernelGGL(glowk_nmf::k_nmf_w_finish, gf, dim3(256), 0, st, (const float*)part, total, per_sig, nmf_w_part_floats(p, rows, KS), p.nch, beta, w_dev);
      LAUNCHCHK("k_nmf_w_finish");
    }
    if (update_w != 2) {
      switch (p.kt) {
#define GLOWK_CASE(n) \
  case n: hipLaunchKernelGGL(k_nmfd_update_h<n>, gh, dim3(256), 0, st, v_dev, (const float*)w_dev, wstride, (const float*)h_dev, part, rows, frames, K, Tw, p.ftiles, beta); break;
        GLOWK_NMF_EACH_KT(GLOWK_CASE)
#undef GLOWK_CASE
      }
      LAUNCHCHK("k_nmfd_update_h");
      hipLaunchKernelGGL(k_nmfd_h_finish, ghf, dim3(256), 0, st, (const float*)part, htotal, K, Tw, frames, beta, h_dev);
      LAUNCHCHK("k_nmfd_h_finish");
    }
  }
  return 0;
}

int glowk_nmfd_divergence(const float* v_dev, int nsig, int rows, int frames, const float* w_dev, int nw, const float* h_dev, int K, int Tw, int beta,
                          double* out_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_nmfd;
  const std::string me("nmfd_divergence");
  if (int rc = nmfd_ranges(me, nsig, rows, frames, K, Tw)) return rc;
  if (int rc = nmf_model(me, nsig, nw, beta)) return rc;
  if (nsig == 0) return 0;
  if (!v_dev || !w_dev || !h_dev || !out_dev || !work_dev) return fail("null tensor");
  const int KS = K * Tw;
  const NmfPlan p = nmf_plan(rows, frames, KS);
  const size_t need = (size_t)nsig * (size_t)glowk_nmf::nmf_div_parts(p) * 8;
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_nmfd_workspace_bytes says");
  if ((uintptr_t)work_dev % 8 || (uintptr_t)out_dev % 8) return fail(me + ": work_dev and out_dev must be aligned to 8 bytes");
  const size_t nv = (size_t)nsig * rows * frames * 4, nww = (size_t)nw * rows * KS * 4, nh = (size_t)nsig * K * frames * 4, no = (size_t)nsig * 8;
  const void* ins[3] = {v_dev, w_dev, h_dev};
  const size_t in_sizes[3] = {nv, nww, nh};
  for (int i = 0; i < 3; ++i)
    if (bytes_overlap(ins[i], in_sizes[i], out_dev, no) || bytes_overlap(ins[i], in_sizes[i], work_dev, need))
      return fail(me + ": out_dev and work_dev must not overlap the inputs");
  if (bytes_overlap(out_dev, no, work_dev, need)) return fail(me + ": out_dev and work_dev must not overlap");
  int dev;
  if (int rc = audio_device({v_dev, w_dev, h_dev, out_dev, work_dev}, &dev, "nmfd_divergence")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_nmfd_divergence, dim3((unsigned)((int64_t)nsig * p.rtiles * p.nch)), dim3(256), 0, st, v_dev, w_dev,
                     nw == 1 ? (int64_t)0 : (int64_t)rows * KS, h_dev, rows, frames, K, Tw, p, beta, (double*)work_dev);
  LAUNCHCHK("k_nmfd_divergence");
  hipLaunchKernelGGL(glowk_nmf::k_nmf_div_reduce, dim3((unsigned)nsig), dim3(64), 0, st, (const double*)work_dev, glowk_nmf::nmf_div_parts(p), out_dev);
  LAUNCHCHK("k_nmf_div_reduce");
  return 0;
}

int glowk_nmfd_masks(const float* w_dev, int nw, const float* h_dev, int nsig, int rows, int frames, int K, int Tw, const int32_t* bounds_host,
                     int num_sources, int power, const float* x_dev, int channels, float* mask_dev, float* spec_dev, void* stream) {
  using namespace glowk_nmfd;
  const std::string me("nmfd_masks");
  if (int rc = nmfd_ranges(me, nsig, rows, frames, K, Tw)) return rc;
  if (nw != 1 && nw != nsig) return fail(me + ": nw must be 1 (one shared dictionary) or nsig");
  if (num_sources < 1 || num_sources > glowk_nmf::MAX_SRC) return fail(me + ": the number of sources must be in [1, 16]");
  if (power != 1 && power != 2) return fail(me + ": power must be 1 or 2");
  if (!bounds_host) return fail(me + ": bounds_host is null");
  const int KS = K * Tw;
  int bc[glowk_nmf::MAX_SRC + 1];                                // in components, as the caller gives them
  for (int s = 0; s <= glowk_nmf::MAX_SRC; ++s) bc[s] = s <= num_sources ? bounds_host[s] : K;
  if (bc[0] != 0 || bc[num_sources] != K) return fail(me + ": bounds must start at 0 and end at K");
  for (int s = 0; s < num_sources; ++s)
    if (bc[s] >= bc[s + 1]) return fail(me + ": bounds must increase strictly (every source owns at least one component)");
  glowk_nmf::NmfBounds bd;                                       // in stacked components: k-major, so a range stays a range
  for (int s = 0; s <= glowk_nmf::MAX_SRC; ++s) bd.b[s] = bc[s] * Tw;
  if ((x_dev == nullptr) != (spec_dev == nullptr)) return fail(me + ": x_dev and spec_dev are given together or not at all");
  if (x_dev && channels != 1 && channels != 2) return fail(me + ": the channel count must be 1 or 2");
  const int C = x_dev ? channels : 0;
  const int64_t cells = (int64_t)nsig * rows * frames;
  if (cells * num_sources * (C ? C : 1) > (int64_t)INT32_MAX) return fail(me + ": nsig * S * C * rows * frames must be at most 2^31 - 1");
  if (nsig == 0) return 0;
  if (!w_dev || !h_dev || !mask_dev) return fail("null tensor");
  if ((uintptr_t)x_dev % 8 || (uintptr_t)spec_dev % 8) return fail(me + ": x_dev and spec_dev must be aligned to 8 bytes");
  const size_t nww = (size_t)nw * rows * KS * 4, nh = (size_t)nsig * K * frames * 4, nx = (size_t)cells * C * 8,
               nm = (size_t)cells * num_sources * 4, ns = (size_t)cells * num_sources * C * 8;
  const void* ins[3] = {w_dev, h_dev, x_dev};
  const size_t in_sizes[3] = {nww, nh, nx};
  for (int i = 0; i < 3; ++i) {
    if (!ins[i]) continue;
    if (bytes_overlap(ins[i], in_sizes[i], mask_dev, nm) || (spec_dev && bytes_overlap(ins[i], in_sizes[i], spec_dev, ns)))
      return fail(me + ": mask_dev and spec_dev must not overlap the inputs");
  }
  if (spec_dev && bytes_overlap(mask_dev, nm, spec_dev, ns)) return fail(me + ": mask_dev and spec_dev must not overlap");
  int dev;
  if (int rc = audio_device({w_dev, h_dev, x_dev, mask_dev, spec_dev}, &dev, "nmfd_masks")) return rc;
  DeviceGuard dg(dev);
  const NmfPlan p = nmf_plan(rows, frames, KS);
  const int fgroups = (p.ftiles + glowk_nmf::WAVES - 1) / glowk_nmf::WAVES;
  if ((int64_t)nsig * p.rtiles * fgroups > (int64_t)INT32_MAX) return fail(me + ": the workgroup count must be at most 2^31 - 1");
  hipLaunchKernelGGL(k_nmfd_masks, dim3((unsigned)((int64_t)nsig * p.rtiles * fgroups)), dim3(256), 0, (hipStream_t)stream, w_dev,
                     nw == 1 ? (int64_t)0 : (int64_t)rows * KS, h_dev, rows, frames, K, Tw, p.rtiles, fgroups, bd, num_sources, power, (const float2*)x_dev, C, mask_dev,
                     (float2*)spec_dev);
  LAUNCHCHK("k_nmfd_masks");
  return 0;
}

// ---- WPE dereverberation: delayed linear prediction, the correlations on the fp64 matrix cores (glowk_wpe.h) ---------------------------------
namespace {
int wpe_sizes(const std::string& w, int nsig, int M, int rows, int frames) {
  using namespace glowk_wpe;
  if (nsig < 0 || nsig > MAX_SIG) return fail(w + ": nsig must be in [0, 65535]");
  if (M < 1 || M > MAX_M) return fail(w + ": the channel count M must be in [1, 4]");
  if (rows < 1 || rows > MAX_ROWS) return fail(w + ": rows must be in [1, 4096]");
  if (frames < 1 || frames > MAX_FRAMES) return fail(w + ": frames must be in [1, 32768]");
  if (!sizes_ok(nsig, M, rows, frames)) return fail(w + ": nsig * M * rows * frames must be at most 2^31 - 1");
  return 0;
}
int wpe_model(const std::string& w, int M, int K, int delay) {
  using namespace glowk_wpe;
  if (K < 1 || K > MAX_K) return fail(w + ": the tap count K must be in [1, 32]");
  if (M * K > MAX_D) return fail(w + ": M * K must be at most 64");
  if (delay < 1 || delay > MAX_DELAY) return fail(w + ": delay must be in [1, 16]");
  return 0;
}
int wpe_power_args(const std::string& w, int context, double eps) {
  if (context < 0 || context > glowk_wpe::MAX_CONTEXT) return fail(w + ": context must be in [0, 8]");
  if (!(eps > 0.0 && eps <= 1.0)) return fail(w + ": eps must be in (0, 1]");
  return 0;
}
int wpe_loading(const std::string& w, double loading) {
  if (!(loading >= 0.0 && loading <= 1.0)) return fail(w + ": loading must be in [0, 1]");
  return 0;
}
int wpe_launch_power(const float* y, int nsig, int M, int rows, int frames, int context, double eps, double* w, double* pmax, hipStream_t st) {
  using namespace glowk_wpe;
  hipLaunchKernelGGL(k_wpe_power, dim3((unsigned)row_grid(nsig, rows)), dim3(THREADS), 0, st, (const float2*)y, M, rows, frames, context, eps, w, pmax);
  LAUNCHCHK("k_wpe_power");
  return 0;
}
int wpe_launch_corr(const float* x, const double* w, int nsig, int M, int rows, int frames, int K, int delay, double* r, double* p, hipStream_t st) {
  using namespace glowk_wpe;
  hipLaunchKernelGGL(k_wpe_corr, dim3((unsigned)row_grid(nsig, rows)), dim3(THREADS), 0, st, (const float2*)x, w, M, K, delay, rows, frames, (double2*)r, (double2*)p);
  LAUNCHCHK("k_wpe_corr");
  return 0;
}
int wpe_launch_solve(const double* r, const double* p, int nsig, int rows, int D, int M, double loading, double* g, int* status, hipStream_t st) {
  using namespace glowk_wpe;
  hipLaunchKernelGGL(k_wpe_solve, dim3((unsigned)row_grid(nsig, rows)), dim3(SOLVE_THREADS), 0, st, (const double2*)r, (const double2*)p, D, M, loading, (double2*)g,
                     status);
  LAUNCHCHK("k_wpe_solve");
  return 0;
}
int wpe_launch_filter(const float* x, const double* g, int nsig, int M, int rows, int frames, int K, int delay, float* y, hipStream_t st) {
  using namespace glowk_wpe;
  hipLaunchKernelGGL(k_wpe_filter, dim3((unsigned)filter_grid(nsig, rows, frames)), dim3(THREADS), 0, st, (const float2*)x, (const double2*)g, M, K, delay, rows, frames,
                     (float2*)y);
  LAUNCHCHK("k_wpe_filter");
  return 0;
}
}  // namespace

size_t glowk_wpe_workspace_bytes(int nsig, int M, int K, int rows, int frames) {
  if (wpe_sizes("wpe_workspace_bytes", nsig, M, rows, frames) || K < 1 || K > glowk_wpe::MAX_K || M * K > glowk_wpe::MAX_D) return 0;
  return glowk_wpe::work_bytes(nsig, M, K, rows, frames);
}

int glowk_wpe_power(const float* y_dev, int nsig, int M, int rows, int frames, int context, double eps, double* w_dev, double* max_dev, void* stream) {
  using namespace glowk_wpe;
  const std::string me("wpe_power");
  if (int rc = wpe_sizes(me, nsig, M, rows, frames)) return rc;
  if (int rc = wpe_power_args(me, context, eps)) return rc;
  if (nsig == 0) return 0;
  if (!y_dev || !w_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {y_dev, w_dev, max_dev})) return rc;
  if (int rc = iva_disjoint(me, {{w_dev, w_bytes(nsig, rows, frames)}, {max_dev, (size_t)nsig * rows * 8}, {y_dev, x_bytes(nsig, M, rows, frames)}}, 2)) return rc;
  int dev;
  if (int rc = audio_device({y_dev, w_dev, max_dev}, &dev, "wpe_power")) return rc;
  DeviceGuard dg(dev);
  return wpe_launch_power(y_dev, nsig, M, rows, frames, context, eps, w_dev, max_dev, (hipStream_t)stream);
}

int glowk_wpe_correlations(const float* x_dev, const double* w_dev, int nsig, int M, int rows, int frames, int K, int delay, double* r_dev, double* p_dev,
                           void* stream) {
  using namespace glowk_wpe;
  const std::string me("wpe_correlations");
  if (int rc = wpe_sizes(me, nsig, M, rows, frames)) return rc;
  if (int rc = wpe_model(me, M, K, delay)) return rc;
  if (nsig == 0) return 0;
  if (!x_dev || !w_dev || !r_dev || !p_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {x_dev, w_dev, r_dev, p_dev})) return rc;
  const int D = stacked(M, K);
  if (int rc = iva_disjoint(me, {{r_dev, r_bytes(nsig, rows, D)}, {p_dev, p_bytes(nsig, rows, D, M)}, {x_dev, x_bytes(nsig, M, rows, frames)},
                                 {w_dev, w_bytes(nsig, rows, frames)}}, 2))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, w_dev, r_dev, p_dev}, &dev, "wpe_correlations")) return rc;
  DeviceGuard dg(dev);
  return wpe_launch_corr(x_dev, w_dev, nsig, M, rows, frames, K, delay, r_dev, p_dev, (hipStream_t)stream);
}

int glowk_wpe_solve(const double* r_dev, const double* p_dev, int nsig, int rows, int D, int M, double loading, double* g_dev, int32_t* status_dev, void* stream) {
  using namespace glowk_wpe;
  const std::string me("wpe_solve");
  if (nsig < 0 || nsig > MAX_SIG) return fail(me + ": nsig must be in [0, 65535]");
  if (rows < 1 || rows > MAX_ROWS) return fail(me + ": rows must be in [1, 4096]");
  if (M < 1 || M > MAX_M) return fail(me + ": the channel count M must be in [1, 4]");
  if (D < 1 || D > MAX_D) return fail(me + ": the system size D must be in [1, 64]");
  if (int rc = wpe_loading(me, loading)) return rc;
  if (nsig == 0) return 0;
  if (!r_dev || !p_dev || !g_dev || !status_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {r_dev, p_dev, g_dev})) return rc;
  if ((uintptr_t)status_dev % 4) return fail(me + ": status_dev must be aligned to 4 bytes");
  if (int rc = iva_disjoint(me, {{g_dev, p_bytes(nsig, rows, D, M)}, {status_dev, (size_t)nsig * rows * 4}, {r_dev, r_bytes(nsig, rows, D)},
                                 {p_dev, p_bytes(nsig, rows, D, M)}}, 2))
    return rc;
  int dev;
  if (int rc = audio_device({r_dev, p_dev, g_dev, status_dev}, &dev, "wpe_solve")) return rc;
  DeviceGuard dg(dev);
  return wpe_launch_solve(r_dev, p_dev, nsig, rows, D, M, loading, g_dev, status_dev, (hipStream_t)stream);
}

int glowk_wpe_filter(const float* x_dev, const double* g_dev, int nsig, int M, int rows, int frames, int K, int delay, float* y_dev, void* stream) {
  using namespace glowk_wpe;
  const std::string me("wpe_filter");
  if (int rc = wpe_sizes(me, nsig, M, rows, frames)) return rc;
  if (int rc = wpe_model(me, M, K, delay)) return rc;
  if (nsig == 0) return 0;
  if (!x_dev || !g_dev || !y_dev) return fail("null tensor");
  if (int rc = iva_aligned(me, {x_dev, g_dev, y_dev})) return rc;
  if (int rc = iva_disjoint(me, {{y_dev, x_bytes(nsig, M, rows, frames)}, {x_dev, x_bytes(nsig, M, rows, frames)}, {g_dev, p_bytes(nsig, rows, stacked(M, K), M)}}, 1))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, g_dev, y_dev}, &dev, "wpe_filter")) return rc;
  DeviceGuard dg(dev);
  return wpe_launch_filter(x_dev, g_dev, nsig, M, rows, frames, K, delay, y_dev, (hipStream_t)stream);
}

int glowk_wpe_fit(const float* x_dev, int nsig, int M, int rows, int frames, int K, int delay, int iterations, int context, double eps, double loading,
                  float* y_dev, double* g_dev, int32_t* status_dev, void* work_dev, size_t work_bytes, void* stream) {
  using namespace glowk_wpe;
  const std::string me("wpe_fit");
  if (int rc = wpe_sizes(me, nsig, M, rows, frames)) return rc;
  if (int rc = wpe_model(me, M, K, delay)) return rc;
  if (int rc = wpe_power_args(me, context, eps)) return rc;
  if (int rc = wpe_loading(me, loading)) return rc;
  if (iterations < 0 || iterations > MAX_ITER) return fail(me + ": iterations must be in [0, 1000]");
  if (nsig == 0 || iterations == 0) return 0;
  if (!x_dev || !y_dev || !g_dev || !status_dev || !work_dev) return fail("null tensor");
  const size_t need = glowk_wpe::work_bytes(nsig, M, K, rows, frames);
  if (work_bytes < need) return fail(me + ": work_bytes is smaller than glowk_wpe_workspace_bytes says");
  if (int rc = iva_aligned(me, {x_dev, y_dev, g_dev, work_dev})) return rc;
  if ((uintptr_t)status_dev % 4) return fail(me + ": status_dev must be aligned to 4 bytes");
  const int D = stacked(M, K);
  if (int rc = iva_disjoint(me, {{y_dev, x_bytes(nsig, M, rows, frames)}, {g_dev, p_bytes(nsig, rows, D, M)}, {status_dev, (size_t)nsig * rows * 4}, {work_dev, need},
                                 {x_dev, x_bytes(nsig, M, rows, frames)}}, 4))
    return rc;
  int dev;
  if (int rc = audio_device({x_dev, y_dev, g_dev, status_dev, work_dev}, &dev, "wpe_fit")) return rc;
  DeviceGuard dg(dev);
  hipStream_t st = (hipStream_t)stream;
  double* w = (double*)work_dev;
  double* r = w + (size_t)nsig * rows * frames;
  double* p = r + (size_t)nsig * rows * D * D * 2;
  for (int it = 0; it < iterations; ++it) {
    if (int rc = wpe_launch_power(it ? y_dev : x_dev, nsig, M, rows, frames, context, eps, w, nullptr, st)) return rc;
    if (int rc = wpe_launch_corr(x_dev, w, nsig, M, rows, frames, K, delay, r, p, st)) return rc;
    if (int rc = wpe_launch_solve(r, p, nsig, rows, D, M, loading, g_dev, status_dev, st)) return rc;
    if (int rc = wpe_launch_filter(x_dev, g_dev, nsig, M, rows, frames, K, delay, y_dev, st)) return rc;
  }
  return 0;
}

}  // extern "C"
