// glowk: AuxIVA (Ono 2011) and ILRMA (Kitamura et al. 2016) -- blind separation of an M-channel STFT by one M x M demixing matrix per
// frequency row, updated by iterative projection.  Formulas in include/glowk.h, design and measurements in DESIGN section 23.
//
//   k_iva_norms     partial[sig][rb][k][t] = sum over the rows of row block rb of |y_k(f, t)|^2, y = W_f x in registers (never stored);
//                   compensated, as are the sums over the row blocks and lambda's sum per thread
//   k_iva_phi       r_k(t) = the partials added in row-block order; phi_k(t) from r by the source model
//   k_iva_cov       one workgroup per (signal, row): V_k(f) = (1/T) sum_t phi_k x x^H for every k, the frames in an order that T alone
//                   fixes, then (IP) the M sequential row updates of W_f by one thread.  <MODE 0> reads phi [M][T]; <MODE 1> evaluates
//                   the low-rank model sum_l basis_k(f, l) act_k(l, t) in registers.  Without IP it stores V (the diagnostic stage)
//   k_iva_ip        the same row updates from a stored V: iva_ip_row is the one function both call, so the stages give the fused bits
//   k_iva_power     P_k = |y_k|^2 rounded once to float32 (ILRMA's NMF input)
//   k_iva_lambda    lambda_k = sqrt(mean |y_k|^2) from r_k(t) (k_iva_norms, k_iva_phi); k_iva_scale divides W's rows and the basis by it
//   k_iva_inverse   W_f^-1 by Gauss-Jordan with partial pivoting, all zero where it is not finite
//   k_iva_demix     Y = W X and the images W^-1[m][k] y_k in one pass over X
//
// Everything after the load of X is fp64 with contraction off, every sum has an order that the shapes alone fix, and no kernel uses
// an atomic: the bits do not depend on the run, the grid or the batch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace glowk_iva {

constexpr int MAX_M = 4, MAX_ROWS = 4096, MAX_FRAMES = 32768, MAX_SIG = 65535, MAX_K = 128;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_ROW_BLOCKS = 32, MIN_BLOCK_ROWS = 32;
constexpr double FLOOR = 0x1p-40;
enum { MODEL_LAPLACE = 0, MODEL_GAUSS = 1, MODEL_SUM = 2 };   // MODEL_SUM (internal): k_iva_phi stores r_k(t) itself, for lambda

// The rows are cut into nrb <= 32 blocks of rpc >= 32 rows (the last may be shorter): a function of `rows` alone.
struct RowPlan {
  int rpc, nrb;
};
inline RowPlan row_plan(int rows) {
  const int want = (rows + MIN_BLOCK_ROWS - 1) / MIN_BLOCK_ROWS;
  const int n0 = want < MAX_ROW_BLOCKS ? want : MAX_ROW_BLOCKS;
  RowPlan p;
  p.rpc = (rows + n0 - 1) / n0;
  p.nrb = (rows + p.rpc - 1) / p.rpc;
  return p;
}
__host__ __device__ inline int frame_chunks(int frames) { return (frames + THREADS - 1) / THREADS; }
// doubles: the partial norms [nsig][nrb][M][frames]
inline size_t partial_doubles(int nsig, int M, int rows, int frames) { return (size_t)nsig * row_plan(rows).nrb * M * frames; }

struct cd {
  double re, im;
};
__device__ inline cd cmul(cd a, cd b) {
#pragma clang fp contract(off)
  cd r = {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
  return r;
}
// a conj(b)
__device__ inline cd cmulc(cd a, cd b) {
#pragma clang fp contract(off)
  cd r = {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im};
  return r;
}
__device__ inline cd cdiv(cd a, cd b) {
#pragma clang fp contract(off)
  const double den = b.re * b.re + b.im * b.im;
  cd r = {(a.re * b.re + a.im * b.im) / den, (a.im * b.re - a.re * b.im) / den};
  return r;
}
__device__ inline cd csub(cd a, cd b) {
#pragma clang fp contract(off)
  cd r = {a.re - b.re, a.im - b.im};
  return r;
}
__device__ inline cd cadd(cd a, cd b) {
#pragma clang fp contract(off)
  cd r = {a.re + b.re, a.im + b.im};
  return r;
}
__device__ inline double cmag2(cd a) {
#pragma clang fp contract(off)
  return a.re * a.re + a.im * a.im;
}
__device__ inline void cswap_if(bool c, cd& a, cd& b) {
  const cd t = a;
  a.re = c ? b.re : a.re; a.im = c ? b.im : a.im;
  b.re = c ? t.re : b.re; b.im = c ? t.im : b.im;
}
__device__ inline cd cload(const double* p, int i) {
  cd r = {p[2 * i], p[2 * i + 1]};
  return r;
}

// Neumaier's compensated sum: s + c carries the sum of its terms to about one rounding, whatever their number.  The frame norms and
// lambda are sums of up to 2^27 non-negative terms, and lambda's error is every scaled entry's error.
struct KSum {
  double s, c;
};
__device__ inline void ksum_add(KSum& a, double x) {
#pragma clang fp contract(off)
  const double t = a.s + x;
  a.c += fabs(a.s) >= fabs(x) ? (a.s - t) + x : (x - t) + a.s;
  a.s = t;
}
__device__ inline double ksum_value(const KSum& a) { return a.s + a.c; }

// y_k = sum_m W[k][m] x_m, m ascending; w: M x M complex128 row-major, x: the M channels of one cell
template <int M>
__device__ inline void demix_cell(const cd (&w)[M][M], const float2 (&x)[M], cd (&y)[M]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < M; ++k) {
    cd xm = {(double)x[0].x, (double)x[0].y};
    cd acc = cmul(w[k][0], xm);
#pragma unroll
    for (int m = 1; m < M; ++m) {
      cd xv = {(double)x[m].x, (double)x[m].y};
      acc = cadd(acc, cmul(w[k][m], xv));
    }
    y[k] = acc;
  }
}
template <int M>
__device__ inline void load_matrix(const double* p, cd (&w)[M][M]) {
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) w[i][j] = cload(p, i * M + j);
}
// the M channels of cell (f, t) of signal sig; x: [nsig][M][rows][frames]
template <int M>
__device__ inline void load_cell(const float2* x, int64_t sig, int rows, int frames, int f, int t, float2 (&v)[M]) {
  const int64_t plane = (int64_t)rows * frames;
#pragma unroll
  for (int m = 0; m < M; ++m) v[m] = x[(sig * M + m) * plane + (int64_t)f * frames + t];
}

// Workgroup (sig, rb, tc): thread t of frame chunk tc walks the rows of row block rb in order.
template <int M>
__global__ __launch_bounds__(THREADS) void k_iva_norms(const float2* __restrict__ x, const double* __restrict__ w, int rows, int frames, RowPlan rp,
                                                        double* __restrict__ partial) {
#pragma clang fp contract(off)
  const int tcs = frame_chunks(frames);
  const int64_t b = blockIdx.x;
  const int tc = (int)(b % tcs), rb = (int)((b / tcs) % rp.nrb);
  const int64_t sig = b / ((int64_t)tcs * rp.nrb);
  const int t = tc * THREADS + (int)threadIdx.x;
  if (t >= frames) return;
  const int f0 = rb * rp.rpc, f1 = f0 + rp.rpc < rows ? f0 + rp.rpc : rows;
  KSum acc[M];
#pragma unroll
  for (int k = 0; k < M; ++k) acc[k].s = acc[k].c = 0.0;
  for (int f = f0; f < f1; ++f) {
    cd wf[M][M], y[M];
    float2 xv[M];
    load_matrix<M>(w + (sig * rows + f) * (2 * M * M), wf);
    load_cell<M>(x, sig, rows, frames, f, t, xv);
    demix_cell<M>(wf, xv, y);
#pragma unroll
    for (int k = 0; k < M; ++k) ksum_add(acc[k], cmag2(y[k]));
  }
#pragma unroll
  for (int k = 0; k < M; ++k) partial[((sig * rp.nrb + rb) * M + k) * frames + t] = ksum_value(acc[k]);
}

// r_k(t): the row blocks in order
__device__ inline double norm_of(const double* partial, int64_t sig, int k, int t, int M, int nrb, int frames) {
  KSum r = {0.0, 0.0};
  for (int rb = 0; rb < nrb; ++rb) ksum_add(r, partial[((sig * nrb + rb) * M + k) * frames + t]);
  return ksum_value(r);
}

// one thread per (sig, k, t)
__global__ __launch_bounds__(THREADS) void k_iva_phi(const double* __restrict__ partial, int64_t total, int M, int rows, int frames, int nrb, int model,
                                                      double* __restrict__ phi) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= total) return;
  const int t = (int)(i % frames), k = (int)((i / frames) % M);
  const int64_t sig = i / ((int64_t)frames * M);
  const double r = norm_of(partial, sig, k, t, M, nrb, frames);
  phi[i] = model == MODEL_SUM ? r : 1.0 / fmax(model == MODEL_GAUSS ? r / (double)rows : sqrt(r), FLOOR);
}

// ---- iterative projection ------------------------------------------------------------------------------------------------------------
// The M sequential updates of one row's W (M x M complex128 at wp, in place) from its covariances v: [M(k)][M][M] complex128, Hermitian,
// both triangles stored.  For k ascending: A = W V_k, u = A^-1 e_k by Gaussian elimination with partial pivoting, d = Re(u^H V_k u);
// row k becomes conj(u) / sqrt(d) when every component of u and d is finite and d > 0, else it stays.  v may be LDS or global memory.
template <int M>
__device__ inline void iva_ip_row(double* wp, const double* v) {
#pragma clang fp contract(off)
  // one source at a time, W re-read from memory: unrolling the sources would hold M copies of the elimination in registers
#pragma unroll 1
  for (int k = 0; k < M; ++k) {
    cd a[M][M], b[M], u[M];
    const double* vk = v + k * 2 * M * M;
#pragma unroll
    for (int i = 0; i < M; ++i) {
#pragma unroll
      for (int j = 0; j < M; ++j) {
        cd s = cmul(cload(wp, i * M), cload(vk, j));
#pragma unroll
        for (int m = 1; m < M; ++m) s = cadd(s, cmul(cload(wp, i * M + m), cload(vk, m * M + j)));
        a[i][j] = s;
      }
      b[i].re = i == k ? 1.0 : 0.0;
      b[i].im = 0.0;
    }
#pragma unroll
    for (int c = 0; c < M; ++c) {
#pragma unroll
      for (int r = c + 1; r < M; ++r) {
        const bool sw = cmag2(a[r][c]) > cmag2(a[c][c]);
#pragma unroll
        for (int j = 0; j < M; ++j) cswap_if(sw, a[r][j], a[c][j]);
        cswap_if(sw, b[r], b[c]);
      }
#pragma unroll
      for (int r = c + 1; r < M; ++r) {
        const cd g = cdiv(a[r][c], a[c][c]);
#pragma unroll
        for (int j = c + 1; j < M; ++j) a[r][j] = csub(a[r][j], cmul(g, a[c][j]));
        b[r] = csub(b[r], cmul(g, b[c]));
      }
    }
#pragma unroll
    for (int c = M - 1; c >= 0; --c) {
      cd s = b[c];
#pragma unroll
      for (int j = c + 1; j < M; ++j) s = csub(s, cmul(a[c][j], u[j]));
      u[c] = cdiv(s, a[c][c]);
    }
    // d = sum_i conj(u_i) (V_k u)_i; V_k is Hermitian, so the exact value is real
    double d = 0.0;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      cd s = cmul(cload(vk, i * M), u[0]);
#pragma unroll
      for (int j = 1; j < M; ++j) s = cadd(s, cmul(cload(vk, i * M + j), u[j]));
      d += cmulc(s, u[i]).re;
      ok = ok && isfinite(u[i].re) && isfinite(u[i].im);
    }
    ok = ok && isfinite(d) && d > 0.0;
    const double sd = sqrt(d);
    if (ok) {
#pragma unroll
      for (int m = 0; m < M; ++m) {
        wp[2 * (k * M + m)] = u[m].re / sd;
        wp[2 * (k * M + m) + 1] = -u[m].im / sd;
      }
    }
  }
}

// The weights one cell's covariance terms take: phi [nsig][M][frames] (AuxIVA) or the low-rank model (ILRMA).
struct CovWeights {
  const double* phi;
  const float* basis;   // [nsig][M][rows][K]
  const float* act;     // [nsig][M][K][frames]
  int K;
};

// Workgroup (sig, f).  Thread i adds the frames i, i + 256, .. in order; a wave adds its lanes by halving (32, 16, .. 1); the four
// waves are added in order: the order depends on T alone.  acc[k] holds V_k's M diagonal entries, then (re, im) of the entries
// (i, j), i < j, in row-major order.
template <int M, int MODE, bool IP>
__global__ __launch_bounds__(THREADS) void k_iva_cov(const float2* __restrict__ x, CovWeights cw, int rows, int frames, double* w, double* __restrict__ v_out) {
#pragma clang fp contract(off)
  constexpr int NV = M * M, NALL = M * NV;
  __shared__ double red[WAVES][NALL];
  __shared__ double vfull[2 * NALL];
  __shared__ float bas[MODE == 1 ? M * MAX_K : 1];
  const int64_t sig = blockIdx.x / rows;
  const int f = (int)(blockIdx.x % rows);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (MODE == 1) {
    for (int i = tid; i < M * cw.K; i += THREADS) bas[i] = cw.basis[((sig * M + i / cw.K) * rows + f) * cw.K + i % cw.K];
    __syncthreads();
  }
  double acc[M][NV];
#pragma unroll
  for (int k = 0; k < M; ++k)
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[k][q] = 0.0;
  for (int t = tid; t < frames; t += THREADS) {
    float2 xv[M];
    load_cell<M>(x, sig, rows, frames, f, t, xv);
    double ph[M];
#pragma unroll
    for (int k = 0; k < M; ++k) {
      if (MODE == 0) {
        ph[k] = cw.phi[(sig * M + k) * frames + t];
      } else {
        double rho = 0.0;
        for (int l = 0; l < cw.K; ++l) rho += (double)bas[k * cw.K + l] * (double)cw.act[((sig * M + k) * cw.K + l) * (int64_t)frames + t];
        ph[k] = 1.0 / fmax(rho, FLOOR);
      }
    }
    double p[NV];
#pragma unroll
    for (int i = 0; i < M; ++i) p[i] = (double)xv[i].x * (double)xv[i].x + (double)xv[i].y * (double)xv[i].y;
    {
      int q = M;
#pragma unroll
      for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = i + 1; j < M; ++j) {
          const cd a = {(double)xv[i].x, (double)xv[i].y}, b = {(double)xv[j].x, (double)xv[j].y};
          const cd c = cmulc(a, b);
          p[q++] = c.re;
          p[q++] = c.im;
        }
    }
#pragma unroll
    for (int k = 0; k < M; ++k)
#pragma unroll
      for (int q = 0; q < NV; ++q) acc[k][q] += ph[k] * p[q];
  }
#pragma unroll
  for (int k = 0; k < M; ++k)
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      double s = acc[k][q];
#pragma unroll
      for (int h = 32; h > 0; h >>= 1) s += __shfl_down(s, h, 64);
      if (lane == 0) red[wave][k * NV + q] = s;
    }
  __syncthreads();
  if (tid < NALL) {
    double s = red[0][tid];
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) s += red[wv][tid];
    s = s / (double)frames;
    const int k = tid / NV, e = tid % NV;
    double* vk = vfull + k * 2 * NV;
    if (e < M) {
      vk[2 * (e * M + e)] = s;
      vk[2 * (e * M + e) + 1] = 0.0;
    } else {
      const int pr = (e - M) >> 1, im = (e - M) & 1;
      int i = 0, j = 1, c = 0;
      for (int a = 0; a < M; ++a)
        for (int b = a + 1; b < M; ++b, ++c)
          if (c == pr) { i = a; j = b; }
      vk[2 * (i * M + j) + im] = s;
      vk[2 * (j * M + i) + im] = im ? -s : s;
    }
  }
  __syncthreads();
  if (IP) {
    if (tid == 0) iva_ip_row<M>(w + (sig * rows + f) * (2 * NV), vfull);
  } else {
    if (tid < 2 * NALL) v_out[(sig * rows + f) * (2 * NALL) + tid] = vfull[tid];
  }
}

// one thread per (sig, f): the staged form of the row updates
template <int M>
__global__ __launch_bounds__(64) void k_iva_ip(double* w, const double* __restrict__ v, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= total) return;
  iva_ip_row<M>(w + i * (2 * M * M), v + i * (2 * M * M * M));
}

// ---- ILRMA's power planes and normalisation ----------------------------------------------------------------------------------------------
// Workgroup (sig, f, tc); P [nsig][M][rows][frames] float32
template <int M>
__global__ __launch_bounds__(THREADS) void k_iva_power(const float2* __restrict__ x, const double* __restrict__ w, int rows, int frames, float* __restrict__ P) {
  const int tcs = frame_chunks(frames);
  const int64_t b = blockIdx.x;
  const int tc = (int)(b % tcs), f = (int)((b / tcs) % rows);
  const int64_t sig = b / ((int64_t)tcs * rows);
  const int t = tc * THREADS + (int)threadIdx.x;
  if (t >= frames) return;
  cd wf[M][M], y[M];
  float2 xv[M];
  load_matrix<M>(w + (sig * rows + f) * (2 * M * M), wf);
  load_cell<M>(x, sig, rows, frames, f, t, xv);
  demix_cell<M>(wf, xv, y);
  const int64_t plane = (int64_t)rows * frames;
#pragma unroll
  for (int k = 0; k < M; ++k) P[(sig * M + k) * plane + (int64_t)f * frames + t] = (float)cmag2(y[k]);
}

// Workgroup (sig, k): lambda = sqrt(sum_t r_k(t) / (rows frames)) from r [nsig][M][frames] (k_iva_phi with MODEL_SUM), the frames in
// k_iva_cov's order, each thread's share compensated
__global__ __launch_bounds__(THREADS) void k_iva_lambda(const double* __restrict__ r, int rows, int frames, double* __restrict__ lam) {
  __shared__ double red[WAVES];
  const int tid = (int)threadIdx.x;
  KSum ks = {0.0, 0.0};
  for (int t = tid; t < frames; t += THREADS) ksum_add(ks, r[(int64_t)blockIdx.x * frames + t]);
  double s = ksum_value(ks);
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) s += __shfl_down(s, h, 64);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double tot = red[0];
#pragma unroll
    for (int wv = 1; wv < WAVES; ++wv) tot += red[wv];
    lam[blockIdx.x] = sqrt(tot / ((double)rows * (double)frames));
  }
}

// Elements [0, nw) are W's complex entries [nsig][rows][M][M], divided by lambda of their row k; the rest are the basis entries
// [nsig][M][rows][K], divided by lambda_k^2 and rounded once.  A lambda that is not finite and positive leaves its source as it is.
__global__ __launch_bounds__(THREADS) void k_iva_scale(const double* __restrict__ lam, int64_t nw, int64_t nb, int M, int rows, int K, double* w, float* basis) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i < nw) {
    const int k = (int)((i / M) % M);
    const int64_t sig = i / ((int64_t)rows * M * M);
    const double l = lam[sig * M + k];
    if (isfinite(l) && l > 0.0) {
      w[2 * i] = w[2 * i] / l;
      w[2 * i + 1] = w[2 * i + 1] / l;
    }
  } else if (i < nw + nb) {
    const int64_t j = i - nw, per = (int64_t)rows * K;
    const double l = lam[j / per];
    if (isfinite(l) && l > 0.0) basis[j] = (float)((double)basis[j] / (l * l));
  }
}

// ---- output ------------------------------------------------------------------------------------------------------------------------------
// one thread per (sig, f): Gauss-Jordan on [W | I] with partial pivoting; all zero where an entry of the inverse is not finite
template <int M>
__global__ __launch_bounds__(64) void k_iva_inverse(const double* __restrict__ w, int64_t total, double* __restrict__ winv) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (idx >= total) return;
  cd a[M][M], b[M][M];
  load_matrix<M>(w + idx * (2 * M * M), a);
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      b[i][j].re = i == j ? 1.0 : 0.0;
      b[i][j].im = 0.0;
    }
#pragma unroll
  for (int c = 0; c < M; ++c) {
#pragma unroll
    for (int r = c + 1; r < M; ++r) {
      const bool sw = cmag2(a[r][c]) > cmag2(a[c][c]);
#pragma unroll
      for (int j = 0; j < M; ++j) {
        cswap_if(sw, a[r][j], a[c][j]);
        cswap_if(sw, b[r][j], b[c][j]);
      }
    }
    const cd piv = a[c][c];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      a[c][j] = cdiv(a[c][j], piv);
      b[c][j] = cdiv(b[c][j], piv);
    }
#pragma unroll
    for (int r = 0; r < M; ++r) {
      if (r == c) continue;
      const cd g = a[r][c];
#pragma unroll
      for (int j = 0; j < M; ++j) {
        a[r][j] = csub(a[r][j], cmul(g, a[c][j]));
        b[r][j] = csub(b[r][j], cmul(g, b[c][j]));
      }
    }
  }
  bool ok = true;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) ok = ok && isfinite(b[i][j].re) && isfinite(b[i][j].im);
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      winv[idx * (2 * M * M) + 2 * (i * M + j)] = ok ? b[i][j].re : 0.0;
      winv[idx * (2 * M * M) + 2 * (i * M + j) + 1] = ok ? b[i][j].im : 0.0;
    }
}

// Workgroup (sig, f, tc).  y_k is rounded to complex64 once; the image of source k in channel m is W^-1[m][k] times that rounded
// y_k, in fp64, rounded once: demix followed by the formula gives the same bits.  y_out [nsig][M][rows][frames] and img_out
// [nsig][M(k)][M(m)][rows][frames] complex64; either may be null (winv is read only with img_out).
template <int M>
__global__ __launch_bounds__(THREADS) void k_iva_demix(const float2* __restrict__ x, const double* __restrict__ w, const double* __restrict__ winv, int rows,
                                                        int frames, float2* __restrict__ y_out, float2* __restrict__ img_out) {
  const int tcs = frame_chunks(frames);
  const int64_t b = blockIdx.x;
  const int tc = (int)(b % tcs), f = (int)((b / tcs) % rows);
  const int64_t sig = b / ((int64_t)tcs * rows);
  const int t = tc * THREADS + (int)threadIdx.x;
  if (t >= frames) return;
  cd wf[M][M], y[M];
  float2 xv[M];
  load_matrix<M>(w + (sig * rows + f) * (2 * M * M), wf);
  load_cell<M>(x, sig, rows, frames, f, t, xv);
  demix_cell<M>(wf, xv, y);
  const int64_t plane = (int64_t)rows * frames, cell = (int64_t)f * frames + t;
  float2 yq[M];
#pragma unroll
  for (int k = 0; k < M; ++k) {
    yq[k] = make_float2((float)y[k].re, (float)y[k].im);
    if (y_out) y_out[(sig * M + k) * plane + cell] = yq[k];
  }
  if (img_out) {
    cd wi[M][M];
    load_matrix<M>(winv + (sig * rows + f) * (2 * M * M), wi);
#pragma unroll
    for (int k = 0; k < M; ++k) {
      const cd yk = {(double)yq[k].x, (double)yq[k].y};
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const cd z = cmul(wi[m][k], yk);
        img_out[((sig * M + k) * M + m) * plane + cell] = make_float2((float)z.re, (float)z.im);
      }
    }
  }
}

}  // namespace glowk_iva
