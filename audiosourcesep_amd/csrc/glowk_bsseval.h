// glowk device code, part 5: BSS Eval v4 separation metrics (bsseval_v4.py, sigsep's v4 with the v3 wrappers), all in fp64.
// Signals are one array sig[2P][nsampl], P = nsrc * nchan: reference channel p = j * nchan + c first, then estimate channel
// P + jest * nchan + c.  A window is a half-open sample range [start, stop); a slice is zero outside it.
//
//   k_bss_xcorr     R_uv(d) = sum_m u[m] v[m + d], d = 0..L-1, over one window, for a list of signal pairs (u, v): the
//                   reference x reference pairs give the block-Toeplitz G (G[(p,a),(q,b)] = R_pq(a-b), or R_qp(b-a)), the
//                   reference x estimate pairs the right-hand sides D[(p,a), e] = R_pe(a) (_compute_reference_correlations,
//                   :465-498, and the correlations of _compute_projection_filters, :520-534: linear, not circular, correlations).
//                   One workgroup per (window, pair, run of 1024-sample chunks) writes partial sums; k_bss_xcorr_sum adds them
//                   in a fixed order (no atomics: bitwise reproducible)
//   k_bss_chol      (G + eps I) C = D per system (np.linalg.solve, :541-544): G assembled from the correlations while loading,
//                   a blocked right-looking Cholesky (32-column panels, 64 x 64 trailing tiles) in a global workspace, the
//                   two triangular solves in place on the right-hand sides; one workgroup per system.  A non-positive or
//                   non-finite pivot stops the system with status 1 (the host redoes it by least squares, :545-548)
//   k_bss_project   for one (window, jtrue, jest): proj_j = Cj * s_jtrue and proj_all = C * s over len + L - 1 samples
//                   (_project, :557-581) and the eight energy sums both forms of _bss_crit (:584-608) need; partial sums per
//                   512-sample chunk, added in a fixed order by k_bss_energy_sum
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace glowk_bss {

constexpr int LMAX = 512;                 // filters_len bound
constexpr int MMAX = 2048;                // nsrc * nchan * filters_len bound of one system
constexpr int XC_THREADS = 128, XC_SUB = 1024, XC_LAGS = LMAX / XC_THREADS;
constexpr int CH_THREADS = 256, CH_NB = 32, CH_TB = 64;
constexpr int PJ_THREADS = 256, PJ_OUT = 2 * PJ_THREADS;
constexpr int NENERGY = 8;

// ---- correlations ---------------------------------------------------------------------------------------------------------------
struct XcorrArgs {
  const double* sig = nullptr;
  int nsig = 0;
  int64_t nsampl = 0;
  const int64_t* win = nullptr;   // [nwin][2] start, stop
  const int* pairs = nullptr;     // [npairs][2] u, v
  int npairs = 0, L = 0;
  int per = 0, nblk = 0;        // chunks per workgroup, workgroups per (window, pair)
  double* part = nullptr;         // [nwin][npairs][nblk][L]
};
static_assert(sizeof(XcorrArgs) == 64 && std::is_trivially_copyable_v<XcorrArgs>, "kernel argument size");

__global__ __launch_bounds__(XC_THREADS) void k_bss_xcorr(XcorrArgs a) {
  __shared__ double su[XC_SUB];
  __shared__ double sv[XC_SUB + LMAX];
  const int t = threadIdx.x, blk = blockIdx.x, pr = blockIdx.y, w = blockIdx.z;
  const int64_t s = max(a.win[2 * w], (int64_t)0), e = min(a.win[2 * w + 1], a.nsampl);
  const int iu = a.pairs[2 * pr], iv = a.pairs[2 * pr + 1];
  const bool ok = iu >= 0 && iu < a.nsig && iv >= 0 && iv < a.nsig;
  const double* u = a.sig + (int64_t)(ok ? iu : 0) * a.nsampl;
  const double* v = a.sig + (int64_t)(ok ? iv : 0) * a.nsampl;
  double acc[XC_LAGS] = {};
  for (int k = 0; ok && k < a.per; ++k) {
    const int64_t m0 = s + ((int64_t)blk * a.per + k) * XC_SUB;
    if (m0 >= e) break;
    __syncthreads();
    for (int i = t; i < XC_SUB; i += XC_THREADS) su[i] = m0 + i < e ? u[m0 + i] : 0.0;
    for (int i = t; i < XC_SUB + a.L - 1; i += XC_THREADS) sv[i] = m0 + i < e ? v[m0 + i] : 0.0;
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < XC_SUB; ++i) {
      const double x = su[i];
#pragma unroll
      for (int l = 0; l < XC_LAGS; ++l)
        if (t + l * XC_THREADS < a.L) acc[l] = fma(x, sv[i + t + l * XC_THREADS], acc[l]);
    }
  }
  double* out = a.part + (((int64_t)w * a.npairs + pr) * a.nblk + blk) * a.L;
#pragma unroll
  for (int l = 0; l < XC_LAGS; ++l)
    if (t + l * XC_THREADS < a.L) out[t + l * XC_THREADS] = acc[l];
}

// corr[w][pair][d] = sum over the workgroups' partials in order
__global__ __launch_bounds__(256) void k_bss_xcorr_sum(const double* __restrict__ part, int64_t n, int L, int nblk, double* __restrict__ corr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t wp = i / L, d = i % L;
  const double* p = part + wp * nblk * L + d;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += p[(int64_t)b * L];
  corr[i] = s;
}

// ---- batched Cholesky solve -----------------------------------------------------------------------------------------------------
struct CholArgs {
  const double* corr = nullptr;   // [nwin][npairs][L]
  int nwin = 0, npairs = 0, P = 0, L = 0, np = 0;   // system: np reference channels from p0, M = np * L; right-hand sides: the P estimate channels
  const int* sys = nullptr;       // [nsys][2] correlation window, p0
  int sys0 = 0;             // first system of this launch (workspace slot = blockIdx.x)
  double* A = nullptr;            // [launch systems][M][M] workspace (lower triangle used)
  double* X = nullptr;            // [nsys][P][M] solutions
  int* status = nullptr;          // [nsys]
};
static_assert(sizeof(CholArgs) == 72 && std::is_trivially_copyable_v<CholArgs>, "kernel argument size");

__global__ __launch_bounds__(CH_THREADS) void k_bss_chol(CholArgs a) {
  __shared__ double Ld[CH_NB][CH_NB + 1];
  __shared__ double T1[CH_TB][CH_NB + 1], T2[CH_TB][CH_NB + 1];
  __shared__ double Y[CH_NB * 8];
  __shared__ int fail;
  const int tid = threadIdx.x, k = a.sys0 + blockIdx.x, L = a.L, P = a.P, M = a.np * L;
  const int w = a.sys[2 * k], p0 = a.sys[2 * k + 1];
  if (w < 0 || w >= a.nwin || p0 < 0 || p0 + a.np > P || a.npairs < 2 * P * P) {
    if (tid == 0) a.status[k] = 2;
    return;
  }
  const double* corr = a.corr + (int64_t)w * a.npairs * L;
  double* A = a.A + (int64_t)blockIdx.x * M * M;
  double* X = a.X + (int64_t)k * P * M;
  const double eps = 2.220446049250313e-16;   // np.finfo(np.float64).eps
  // assemble: lower triangle of G + eps I, and D
  for (int64_t idx = tid; idx < (int64_t)M * M; idx += CH_THREADS) {
    const int r = (int)(idx / M), c = (int)(idx % M);
    if (c > r) continue;
    const int p = p0 + r / L, q = p0 + c / L, d = r % L - c % L;
    double g = d >= 0 ? corr[(int64_t)(p * P + q) * L + d] : corr[(int64_t)(q * P + p) * L - d];
    A[idx] = r == c ? g + eps : g;
  }
  for (int idx = tid; idx < P * M; idx += CH_THREADS) {
    const int e = idx / M, r = idx % M;
    X[idx] = corr[(int64_t)(P * P + (p0 + r / L) * P + e) * L + r % L];
  }
  if (tid == 0) fail = 0;
  __syncthreads();

  // factorisation: A = L L^T, L in the lower triangle
  for (int k0 = 0; k0 < M; k0 += CH_NB) {
    const int kn = min(CH_NB, M - k0);
    for (int i = tid; i < CH_NB * CH_NB; i += CH_THREADS) {
      const int r = i / CH_NB, c = i % CH_NB;
      Ld[r][c] = (r < kn && c <= r) ? A[(int64_t)(k0 + r) * M + k0 + c] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < kn; ++j) {
      if (tid == 0) {
        const double dj = Ld[j][j];
        if (!(dj > 0.0) || !(dj < INFINITY)) fail = 1;
        Ld[j][j] = fail ? 1.0 : sqrt(dj);
      }
      __syncthreads();
      if (fail) break;
      if (tid > j && tid < kn) Ld[tid][j] /= Ld[j][j];
      __syncthreads();
      for (int i = tid; i < CH_NB * CH_NB; i += CH_THREADS) {
        const int r = i / CH_NB, c = i % CH_NB;
        if (r < kn && c > j && c <= r) Ld[r][c] -= Ld[r][j] * Ld[c][j];
      }
      __syncthreads();
    }
    if (fail) break;
    for (int i = tid; i < CH_NB * CH_NB; i += CH_THREADS) {
      const int r = i / CH_NB, c = i % CH_NB;
      if (r < kn && c <= r) A[(int64_t)(k0 + r) * M + k0 + c] = Ld[r][c];
    }
    const int k1 = k0 + CH_NB;
    if (k1 >= M) break;                     // then kn == M - k0: the last panel
    // panel: rows below, L_i = A_i Ld^-T (kn == CH_NB here)
    for (int r = k1 + tid; r < M; r += CH_THREADS) {
      asm volatile("" ::: "memory");        // keeps the Ld loads inside the row loop (hoisted, 528 of them spill)
      double x[CH_NB];
      double* row = A + (int64_t)r * M + k0;
#pragma unroll
      for (int j = 0; j < CH_NB; ++j) x[j] = row[j];
#pragma unroll
      for (int j = 0; j < CH_NB; ++j) {
        double s = x[j];
#pragma unroll
        for (int t = 0; t < j; ++t) s -= x[t] * Ld[j][t];
        x[j] = s / Ld[j][j];
      }
#pragma unroll
      for (int j = 0; j < CH_NB; ++j) row[j] = x[j];
    }
    __syncthreads();
    // trailing update of the lower triangle: A[r][c] -= sum_t L[r][t] L[c][t], in 64 x 64 tiles
    const int nt = (M - k1 + CH_TB - 1) / CH_TB, ty = tid / 16, tx = tid % 16;
    for (int I = 0; I < nt; ++I) {
      const int r0 = k1 + I * CH_TB;
      for (int J = 0; J <= I; ++J) {
        const int c0 = k1 + J * CH_TB;
        for (int i = tid; i < CH_TB * CH_NB; i += CH_THREADS) {
          const int r = i / CH_NB, c = i % CH_NB;
          T1[r][c] = r0 + r < M ? A[(int64_t)(r0 + r) * M + k0 + c] : 0.0;
          T2[r][c] = c0 + r < M ? A[(int64_t)(c0 + r) * M + k0 + c] : 0.0;
        }
        __syncthreads();
        double acc[4][4] = {};
#pragma unroll 4
        for (int t = 0; t < CH_NB; ++t) {
          double l1[4], l2[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) { l1[q] = T1[ty + 16 * q][t]; l2[q] = T2[tx + 16 * q][t]; }
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int o = 0; o < 4; ++o) acc[q][o] = fma(l1[q], l2[o], acc[q][o]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int o = 0; o < 4; ++o) {
            const int r = r0 + ty + 16 * q, c = c0 + tx + 16 * o;
            if (r < M && c <= r) A[(int64_t)r * M + c] -= acc[q][o];
          }
        __syncthreads();
      }
    }
  }
  if (fail) {
    if (tid == 0) a.status[k] = 1;
    return;
  }

  // forward substitution L Y = D, then L^T C = Y, on the P right-hand sides in place (blocks of CH_NB rows; P <= 8 per pass)
  for (int e0 = 0; e0 < P; e0 += 8) {
    const int ne = min(8, P - e0);
    for (int k0 = 0; k0 < M; k0 += CH_NB) {
      const int kn = min(CH_NB, M - k0);
      for (int i = tid; i < CH_NB * CH_NB; i += CH_THREADS) {
        const int r = i / CH_NB, c = i % CH_NB;
        Ld[r][c] = (r < kn && c <= r) ? A[(int64_t)(k0 + r) * M + k0 + c] : 0.0;
      }
      __syncthreads();
      if (tid < ne) {
        double* x = X + (int64_t)(e0 + tid) * M + k0;
        for (int j = 0; j < kn; ++j) {
          double s = x[j];
          for (int t = 0; t < j; ++t) s -= Ld[j][t] * Y[t * 8 + tid];
          Y[j * 8 + tid] = s / Ld[j][j];
          x[j] = Y[j * 8 + tid];
        }
      }
      __syncthreads();
      for (int i = k0 + kn + tid; i < M; i += CH_THREADS) {
        const double* row = A + (int64_t)i * M + k0;
        double s[8] = {};
        for (int t = 0; t < kn; ++t) {
          const double l = row[t];
#pragma unroll
          for (int q = 0; q < 8; ++q) s[q] = fma(l, Y[t * 8 + q], s[q]);
        }
        for (int q = 0; q < ne; ++q) X[(int64_t)(e0 + q) * M + i] -= s[q];
      }
      __syncthreads();
    }
    for (int k0 = ((M - 1) / CH_NB) * CH_NB; k0 >= 0; k0 -= CH_NB) {
      const int kn = min(CH_NB, M - k0);
      for (int i = tid; i < CH_NB * CH_NB; i += CH_THREADS) {
        const int r = i / CH_NB, c = i % CH_NB;
        Ld[r][c] = (r < kn && c <= r) ? A[(int64_t)(k0 + r) * M + k0 + c] : 0.0;
      }
      __syncthreads();
      if (tid < ne) {
        double* x = X + (int64_t)(e0 + tid) * M + k0;
        for (int j = kn - 1; j >= 0; --j) {
          double s = x[j];
          for (int t = j + 1; t < kn; ++t) s -= Ld[t][j] * Y[t * 8 + tid];
          Y[j * 8 + tid] = s / Ld[j][j];
          x[j] = Y[j * 8 + tid];
        }
      }
      __syncthreads();
      for (int i = tid; i < k0; i += CH_THREADS) {
        double s[8] = {};
        for (int t = 0; t < kn; ++t) {
          const double l = A[(int64_t)(k0 + t) * M + i];
#pragma unroll
          for (int q = 0; q < 8; ++q) s[q] = fma(l, Y[t * 8 + q], s[q]);
        }
        for (int q = 0; q < ne; ++q) X[(int64_t)(e0 + q) * M + i] -= s[q];
      }
      __syncthreads();
    }
  }
  if (tid == 0) a.status[k] = 0;
}

// ---- projections and energies ---------------------------------------------------------------------------------------------------
struct ProjArgs {
  const double* sig = nullptr;    // [2P][nsampl]
  int64_t nsampl = 0;
  int nsrc = 0, nchan = 0, L = 0;
  const int64_t* items = nullptr; // [nitems][6] start, stop, jtrue, jest, C system, Cj system
  int nitems = 0, nchunk = 0;
  const double* coefC = nullptr;  // [nsysC][P][P * L]
  int nsysC = 0;
  const double* coefJ = nullptr;  // [nsysJ][P][nchan * L]
  int nsysJ = 0;
  double* part = nullptr;         // [nitems][nchunk][NENERGY]
};
static_assert(sizeof(ProjArgs) == 88 && std::is_trivially_copyable_v<ProjArgs>, "kernel argument size");

// energies: 0 |s_true|^2, 1 |est - s_true|^2, 2 |e_spat|^2 = |proj_j - s_true|^2, 3 |proj_j|^2, 4 |e_interf|^2 = |proj_all - proj_j|^2,
// 5 |proj_all|^2, 6 |e_artif|^2 = |est - proj_all|^2, 7 |est - proj_j|^2, each over len + L - 1 samples and every channel
__global__ __launch_bounds__(PJ_THREADS) void k_bss_project(ProjArgs a) {
  __shared__ double xs[PJ_OUT + LMAX];
  __shared__ double cC[LMAX], cJ[LMAX];
  __shared__ double red[NENERGY][PJ_THREADS];
  const int tid = threadIdx.x, item = blockIdx.x / a.nchunk, chunk = blockIdx.x % a.nchunk;
  const int L = a.L, nchan = a.nchan, P = a.nsrc * nchan;
  const int64_t* it = a.items + (int64_t)item * 6;
  const int64_t s = max(it[0], (int64_t)0), e = min(it[1], a.nsampl);
  const int64_t len = e > s ? e - s : 0;
  // range-checked as the 64-bit words they are: narrowed first, 2^32 would pass for 0
  const bool ok = it[2] >= 0 && it[2] < a.nsrc && it[3] >= 0 && it[3] < a.nsrc && it[4] >= 0 && it[4] < a.nsysC && it[5] >= 0 && it[5] < a.nsysJ;
  const int jtrue = ok ? (int)it[2] : 0, jest = ok ? (int)it[3] : 0, sc = ok ? (int)it[4] : 0, sj = ok ? (int)it[5] : 0;
  const int64_t n0 = (int64_t)chunk * PJ_OUT, nout = len + L - 1;
  double en[NENERGY] = {};
  if (ok && n0 < nout) {
    for (int c = 0; c < nchan; ++c) {
      const int ecol = jest * nchan + c;
      double accA[2] = {}, accJ[2] = {};
      for (int p = 0; p < P; ++p) {
        const bool isj = p / nchan == jtrue;
        const double* x = a.sig + (int64_t)p * a.nsampl;
        __syncthreads();
        for (int i = tid; i < PJ_OUT + L - 1; i += PJ_THREADS) {
          const int64_t m = n0 - (L - 1) + i;       // offset in the window
          xs[i] = m >= 0 && m < len ? x[s + m] : 0.0;
        }
        const double* hc = a.coefC + ((int64_t)sc * P + ecol) * P * L + (int64_t)p * L;
        for (int i = tid; i < L; i += PJ_THREADS) cC[i] = hc[i];
        if (isj) {
          const double* hj = a.coefJ + ((int64_t)sj * P + ecol) * nchan * L + (int64_t)(p - jtrue * nchan) * L;
          for (int i = tid; i < L; i += PJ_THREADS) cJ[i] = hj[i];
        }
        __syncthreads();
        const double* xa = xs + tid + L - 1;
        if (isj) {
          for (int d = 0; d < L; ++d) {
            const double h = cC[d], g = cJ[d], x0 = xa[-d], x1 = xa[PJ_THREADS - d];
            accA[0] = fma(h, x0, accA[0]); accA[1] = fma(h, x1, accA[1]);
            accJ[0] = fma(g, x0, accJ[0]); accJ[1] = fma(g, x1, accJ[1]);
          }
        } else {
          for (int d = 0; d < L; ++d) {
            const double h = cC[d];
            accA[0] = fma(h, xa[-d], accA[0]); accA[1] = fma(h, xa[PJ_THREADS - d], accA[1]);
          }
        }
      }
      const double* st = a.sig + (int64_t)(jtrue * nchan + c) * a.nsampl + s;
      const double* es = a.sig + (int64_t)(P + ecol) * a.nsampl + s;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int64_t n = n0 + tid + q * PJ_THREADS;
        if (n >= nout) continue;
        const double t = n < len ? st[n] : 0.0, y = n < len ? es[n] : 0.0, pj = accJ[q], pa = accA[q];
        en[0] = fma(t, t, en[0]);
        en[1] = fma(y - t, y - t, en[1]);
        en[2] = fma(pj - t, pj - t, en[2]);
        en[3] = fma(pj, pj, en[3]);
        en[4] = fma(pa - pj, pa - pj, en[4]);
        en[5] = fma(pa, pa, en[5]);
        en[6] = fma(y - pa, y - pa, en[6]);
        en[7] = fma(y - pj, y - pj, en[7]);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NENERGY; ++q) red[q][tid] = en[q];
  __syncthreads();
  for (int h = PJ_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h)
#pragma unroll
      for (int q = 0; q < NENERGY; ++q) red[q][tid] += red[q][tid + h];
    __syncthreads();
  }
  if (tid < NENERGY) a.part[((int64_t)item * a.nchunk + chunk) * NENERGY + tid] = red[tid][0];
}

// energy[item][q] = sum over the chunks' partials in order
__global__ __launch_bounds__(256) void k_bss_energy_sum(const double* __restrict__ part, int nitems, int nchunk, double* __restrict__ energy) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nitems * NENERGY) return;
  const int item = i / NENERGY, q = i % NENERGY;
  const double* p = part + (int64_t)item * nchunk * NENERGY + q;
  double s = 0.0;
  for (int c = 0; c < nchunk; ++c) s += p[(int64_t)c * NENERGY];
  energy[i] = s;
}

}  // namespace glowk_bss
