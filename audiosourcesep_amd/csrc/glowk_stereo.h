// glowk device code: stereo separation -- the multichannel Wiener filter under the local Gaussian model, its spatial covariances
// fitted by EM (Duong, Vincent, Gribonval 2010), in the front end's STFT convention ([.., 1025, T], frame fastest).
//
// A problem is one mixture STFT x(f,t) in C^2 with S source PSDs v_j(f,t) >= 0; R_j(f) is 2 x 2 Hermitian, R_j = I at the start.
// One iteration, the old v, R on every right-hand side (eps = 1e-10):
//   Cx = sum_k v_k R_k + eps I,  W_j = v_j R_j Cx^-1,  y_j = W_j x,  C_j = y_j y_j^H + (I - W_j) v_j R_j,
//   v_j' = max(0, Re tr(R_j^-1 C_j) / 2),  R_j' = (1/T) sum_t C_j / (v_j' + eps) + eps I;   after n_iter of them Y_j = W_j x.
//
//   k_mwf_em   one workgroup owns one (problem, bin) and runs the whole loop: every (problem, bin) is independent of every other, so
//              the call is one launch with no atomics and nothing shared between workgroups.  Lane = frame (coalesced rows); a
//              thread walks the frames t = tid, tid + NT, ..; per frame one pass over the sources builds Cx, a second updates
//              source after source (v_j is overwritten once Cx holds its old value, so the update is in place).  fp64 in
//              registers, v stored as fp32 between iterations.  The time sums: per NT-frame chunk one exchange tree over the 64
//              lanes (wave_sum4), added chunk after chunk into the wave's running sum, the waves' sums added in wave order -- one
//              fixed order that depends on T alone (NT = 64, 128 or 256 from T), so the result is bitwise reproducible and
//              independent of the batch.
//              The workgroup's S T PSDs and 2 T mixture values are staged in LDS when they fit (STAGE), else streamed in place.
//
// Determinants: a 2 x 2 Hermitian M + eps I with M positive semi-definite has det = det M + eps tr M + eps^2; det M is clamped at 0,
// so rounding never makes the ridged matrix singular (det >= eps^2 = 1e-20, a normal fp64 number).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace glowk_stereo {

constexpr int NBIN = 1025;
constexpr int MAX_SRC = 16;
constexpr double EM_EPS = 1e-10;
constexpr int R_WORDS = 5;                                   // r00, r11, Re r01, Im r01, 1 / det R
constexpr size_t STAGE_MAX = 61440;                          // staged bytes; with the state below the workgroup stays within 64 KiB

__host__ __device__ inline int em_threads(int T) { return T <= 64 ? 64 : T <= 128 ? 128 : 256; }
__host__ __device__ inline size_t em_state_bytes(int nt) { return (size_t)(MAX_SRC * R_WORDS + (nt / 64) * MAX_SRC * 4) * sizeof(double); }
__host__ __device__ inline size_t em_stage_bytes(int S, int T) { return (size_t)T * ((size_t)S * sizeof(float) + 2 * sizeof(float2)); }

struct EmArgs {
  const float2* x = nullptr;    // [P][2][1025][T]
  float* v = nullptr;           // [S][P][1025][T]
  float2* y = nullptr;          // [S][P][2][1025][T]
  double* r = nullptr;          // nullable [S][P][1025][4]
  int S = 0, P = 0, T = 0, n_iter = 0;
};
static_assert(sizeof(EmArgs) == 48 && std::is_trivially_copyable_v<EmArgs>, "kernel argument size");

// The four time sums of one source over the wave's 64 lanes in 7 exchanges instead of 24: lanes 32 apart split the four values
// between them (the lower half keeps s0, s1), lanes 16 apart split the two, then a butterfly over each 16-lane group.  Every lane
// of group k = lane >> 4 ends with the total of s_k: one fixed order of additions.
__device__ __forceinline__ double wave_sum4(double s0, double s1, double s2, double s3, int lane) {
  const bool up = (lane & 32) != 0;
  double k0 = up ? s2 : s0, k1 = up ? s3 : s1;
  k0 += __shfl_xor(up ? s0 : s2, 32, 64);
  k1 += __shfl_xor(up ? s1 : s3, 32, 64);
  const bool odd = (lane & 16) != 0;
  double k = odd ? k1 : k0;
  k += __shfl_xor(odd ? k0 : k1, 16, 64);
#pragma unroll
  for (int m = 8; m > 0; m >>= 1) k += __shfl_xor(k, m, 64);
  return k;
}

// Cx^-1 = [[ib, -ic], [-conj ic, ia]] of Cx = sum_k v_k R_k + eps I at one frame
struct CxInv { double ia, ib, icr, ici; };

template <typename VP>
__device__ __forceinline__ CxInv cx_inverse(const double* Rs, VP v, int64_t vstride, int S, int t, bool act) {
  double a0 = 0.0, b0 = 0.0, cr = 0.0, ci = 0.0;
  for (int k = 0; k < S; ++k) {
    const double vk = act ? (double)v[k * vstride + t] : 0.0;
    const double* R = Rs + k * R_WORDS;
    a0 += vk * R[0]; b0 += vk * R[1]; cr += vk * R[2]; ci += vk * R[3];
  }
  const double d0 = a0 * b0 - (cr * cr + ci * ci);
  const double det = (d0 > 0.0 ? d0 : 0.0) + EM_EPS * (a0 + b0) + EM_EPS * EM_EPS;
  const double inv = 1.0 / det;
  CxInv c;
  c.ia = (a0 + EM_EPS) * inv; c.ib = (b0 + EM_EPS) * inv; c.icr = cr * inv; c.ici = ci * inv;
  return c;
}

// W = G Cx^-1 for the Hermitian G = v_j R_j = [[g0, g], [conj g, g1]]: rows (w00, w01), (w10, w11), complex
struct Gain { double w00r, w00i, w01r, w01i, w10r, w10i, w11r, w11i; };

__device__ __forceinline__ Gain wiener_gain(double g0, double g1, double gr, double gi, const CxInv& c) {
  Gain w;
  w.w00r = g0 * c.ib - (gr * c.icr + gi * c.ici);            // g0 ib - g conj(ic)
  w.w00i = -(gi * c.icr - gr * c.ici);
  w.w01r = gr * c.ia - g0 * c.icr;                           // g ia - g0 ic
  w.w01i = gi * c.ia - g0 * c.ici;
  w.w10r = gr * c.ib - g1 * c.icr;                           // conj(g) ib - g1 conj(ic)
  w.w10i = -gi * c.ib + g1 * c.ici;
  w.w11r = g1 * c.ia - (gr * c.icr + gi * c.ici);            // g1 ia - conj(g) ic
  w.w11i = -(gr * c.ici - gi * c.icr);
  return w;
}

template <int NT, bool STAGE>
__global__ __launch_bounds__(NT) void k_mwf_em(EmArgs a) {
  extern __shared__ __attribute__((aligned(16))) double em_lds[];
  double* Rs = em_lds;                                       // [16][5]
  double* wsum = Rs + MAX_SRC * R_WORDS;                     // [NT / 64][16][4]
  float2* xs = reinterpret_cast<float2*>(wsum + (NT / 64) * MAX_SRC * 4);   // STAGE: [2][T], then v [S][T]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = a.S, T = a.T;
  const int64_t p = blockIdx.x / NBIN, f = blockIdx.x % NBIN;
  const int64_t plane = (int64_t)NBIN * T;
  const float2* gx0 = a.x + (p * 2 * NBIN + f) * T;
  const float2* gx1 = gx0 + plane;
  float* gv = a.v + (p * NBIN + f) * T;                      // source j at gv + j gstride
  const int64_t gstride = (int64_t)a.P * plane;
  float* sv = reinterpret_cast<float*>(xs + 2 * (size_t)T);
  if (STAGE) {
    for (int t = tid; t < T; t += NT) {
      xs[t] = gx0[t];
      xs[T + t] = gx1[t];
      for (int j = 0; j < S; ++j) sv[j * T + t] = gv[j * gstride + t];
    }
  }
  if (tid < S) {
    double* R = Rs + tid * R_WORDS;
    R[0] = 1.0; R[1] = 1.0; R[2] = 0.0; R[3] = 0.0; R[4] = 1.0;
  }
  __syncthreads();
  // one view of the rows for both forms: the frames of a thread are its own, so reads and writes need no barrier
  const float2* x0 = STAGE ? xs : gx0;
  const float2* x1 = STAGE ? xs + T : gx1;
  float* v = STAGE ? sv : gv;
  const int64_t vstride = STAGE ? (int64_t)T : gstride;
  const int chunks = (T + NT - 1) / NT;

  for (int it = 0; it < a.n_iter; ++it) {
    wsum[wave * MAX_SRC * 4 + lane] = 0.0;                   // the wave's own 16 x 4 sums
    __syncthreads();
    for (int c = 0; c < chunks; ++c) {
      const int t = c * NT + tid;
      const bool act = t < T;
      const CxInv ci = cx_inverse(Rs, v, vstride, S, t, act);   // idle lanes run on v = 0, x = 0 and add exact zeros
      const float2 xa = act ? x0[t] : make_float2(0.0f, 0.0f), xb = act ? x1[t] : make_float2(0.0f, 0.0f);
      const double x0r = xa.x, x0i = xa.y, x1r = xb.x, x1i = xb.y;
      for (int j = 0; j < S; ++j) {
        const double* R = Rs + j * R_WORDS;
        const double vj = act ? (double)v[j * vstride + t] : 0.0;
        const double g0 = vj * R[0], g1 = vj * R[1], gr = vj * R[2], gi = vj * R[3];
        const Gain w = wiener_gain(g0, g1, gr, gi, ci);
        const double y0r = w.w00r * x0r - w.w00i * x0i + w.w01r * x1r - w.w01i * x1i;
        const double y0i = w.w00r * x0i + w.w00i * x0r + w.w01r * x1i + w.w01i * x1r;
        const double y1r = w.w10r * x0r - w.w10i * x0i + w.w11r * x1r - w.w11i * x1i;
        const double y1i = w.w10r * x0i + w.w10i * x0r + w.w11r * x1i + w.w11i * x1r;
        // C = y y^H + G - W G: the diagonal's real parts, c01 complex
        const double c00 = y0r * y0r + y0i * y0i + g0 - (w.w00r * g0 + (w.w01r * gr + w.w01i * gi));      // w01 conj(g)
        const double c11 = y1r * y1r + y1i * y1i + g1 - ((w.w10r * gr - w.w10i * gi) + w.w11r * g1);      // w10 g
        const double c01r = y0r * y1r + y0i * y1i + gr - ((w.w00r * gr - w.w00i * gi) + w.w01r * g1);     // y0 conj(y1), w00 g + w01 g1
        const double c01i = y0i * y1r - y0r * y1i + gi - ((w.w00r * gi + w.w00i * gr) + w.w01i * g1);
        const double tr = (R[1] * c00 + R[0] * c11 - 2.0 * (R[2] * c01r + R[3] * c01i)) * R[4];             // Re tr(R^-1 C)
        double vn = 0.5 * tr;
        vn = vn > 0.0 ? vn : 0.0;                            // also turns a NaN into 0
        const float vf = (float)vn;
        if (act) v[j * vstride + t] = vf;
        const double q = 1.0 / (vn + EM_EPS);
        const double sk = wave_sum4(c00 * q, c11 * q, c01r * q, c01i * q, lane);
        if ((lane & 15) == 0) wsum[(wave * MAX_SRC + j) * 4 + (lane >> 4)] += sk;
      }
    }
    __syncthreads();
    if (tid < S) {
      double m[4];
      for (int k = 0; k < 4; ++k) {
        double s = wsum[tid * 4 + k];
        for (int w = 1; w < NT / 64; ++w) s += wsum[(w * MAX_SRC + tid) * 4 + k];
        m[k] = s / (double)T;
      }
      const double d0 = m[0] * m[1] - (m[2] * m[2] + m[3] * m[3]);
      double* R = Rs + tid * R_WORDS;
      R[0] = m[0] + EM_EPS; R[1] = m[1] + EM_EPS; R[2] = m[2]; R[3] = m[3];
      R[4] = 1.0 / ((d0 > 0.0 ? d0 : 0.0) + EM_EPS * (m[0] + m[1]) + EM_EPS * EM_EPS);
    }
    __syncthreads();
  }

  // Y_j = v_j R_j Cx^-1 x with the final v, R
  const int64_t ystride = 2 * gstride;
  float2* y0 = a.y + (p * 2 * NBIN + f) * T;
  for (int t = tid; t < T; t += NT) {
    const CxInv ci = cx_inverse(Rs, v, vstride, S, t, true);
    const float2 xa = x0[t], xb = x1[t];
    const double x0r = xa.x, x0i = xa.y, x1r = xb.x, x1i = xb.y;
    for (int j = 0; j < S; ++j) {
      const double* R = Rs + j * R_WORDS;
      const float vf = v[j * vstride + t];
      const double vj = (double)vf;
      const Gain w = wiener_gain(vj * R[0], vj * R[1], vj * R[2], vj * R[3], ci);
      const double y0r = w.w00r * x0r - w.w00i * x0i + w.w01r * x1r - w.w01i * x1i;
      const double y0i = w.w00r * x0i + w.w00i * x0r + w.w01r * x1i + w.w01i * x1r;
      const double y1r = w.w10r * x0r - w.w10i * x0i + w.w11r * x1r - w.w11i * x1i;
      const double y1i = w.w10r * x0i + w.w10i * x0r + w.w11r * x1i + w.w11i * x1r;
      float2* yj = y0 + j * ystride;
      yj[t] = make_float2((float)y0r, (float)y0i);
      yj[plane + t] = make_float2((float)y1r, (float)y1i);
      if (STAGE && a.n_iter > 0) gv[j * gstride + t] = vf;
    }
  }
  if (a.r && tid < S) {
    double* o = a.r + (((int64_t)tid * a.P + p) * NBIN + f) * 4;
    const double* R = Rs + tid * R_WORDS;
    o[0] = R[0]; o[1] = R[1]; o[2] = R[2]; o[3] = R[3];
  }
}

}  // namespace glowk_stereo
