// glowk device code: REPET-SIM (Rafii & Pardo 2012; librosa's nn_filter "vocal separation" recipe) -- the prior-free baseline for a
// foreground over a repeating accompaniment.  s [nsig][rows][frames] float32, frames contiguous, real and non-negative.
//
//   k_nn_norms      n[f] = sqrt(sum_r s[r][f]^2), an fmaf chain down the rows in row order, one thread per frame
//   k_nn_topk       sim(i, j) = <s[:, i], s[:, j]> / max(n[i] n[j], FLT_MIN) for |i - j| >= width, and per frame i the k largest in
//                   decreasing order, equal similarities to the lower index: the Gram matrix on v_mfma_f32_32x32x2_f32 (exact fp32:
//                   an fmaf chain over the rows in row order, so sim(i, j) and sim(j, i) have the same bits), the norm scaling and
//                   the selection in the same pass; no frames x frames matrix exists anywhere
//   k_nn_transpose  st[f][r] = s[r][f]: the frame-major copy the median gathers from
//   k_nn_median     out[r][i] = the median over the neighbours j of frame i of s[r][j], selected by compares
//
// k_nn_topk: a workgroup of 4 waves owns QT = 32 consecutive query frames of one signal and walks all candidate frames in tiles of
// JT = 128 NACC.  Wave w accumulates the 32 x 32 NACC products of the queries with candidates [32 NACC w, 32 NACC (w + 1)) of the
// tile over all rows: both operands are read straight from s (lane l reads row 2 t + (l >> 5), frame base + (l & 31): two
// 128-byte runs per load), one A and NACC B loads per NACC MFMAs, KU = 16 row pairs per step with the next step's loads in flight
// under this step's MFMAs.  The scaled tile goes to LDS [QT][JT + 8] (the two lane halves of a store land 4 rows = 32 banks
// apart), then wave w selects for queries w, w + 4, ..: 64 candidates per step in increasing frame order, a ballot of those that
// are candidates and beat the list's last entry, and one insertion per set bit into the query's sorted list in LDS.  A list entry
// is one 64-bit key, the similarity's bits as an ordered integer above and ~frame below, so key order is the rule (larger
// similarity first, of equal ones the lower frame) and no two entries are equal; an insertion walks the list from its end, 64
// entries per step, moving those below the new key up by one until it meets a larger one.  Registers: 16 NACC accumulators and
// 2 (1 + NACC) KU operands; LDS: the lists QT KCAP 8 bytes, the tile, the norms and list states -- 75 264 bytes at (KCAP, NACC) =
// (160, 2), 148 992 at (512, 1).  The number of insertions depends on the data, the launches and the result do not.
//
// k_nn_median: a workgroup is one wave and owns one frame and 64 >> ll rows, 1 << ll lanes per output (ll = 0, 1, 2 for k <= 192,
// <= 384, above, so that (k + 1) (64 >> ll) floats stay within 49 KiB of LDS).  It walks the frame's entries 64 at a time, keeps
// those in [0, frames) in order (any other entry is skipped, never read through), and gathers st[j][r0 .. r0 + 64 >> ll) -- a run
// of consecutive floats per neighbour, 16 loads in flight -- into LDS as ordered integers.  The element of sorted position p is
// the largest x with #(w < x) <= p; its 32 bits are fixed from the top down, one count over the neighbours per bit: compares
// only, so the result is an input element's bits.  Odd n: p = n / 2; even n: p = n / 2 - 1, then one more pass gives the element
// above it (the same value if #(w <= x) > p + 1, else the smallest larger one), and (a + b) * 0.5f is the only arithmetic on the
// values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace glowk_repet {

constexpr int MAX_SIG = 65535, MAX_ROWS = 4096, MAX_FRAMES = 32768, MAX_K = 512, MAX_WIDTH = 1 << 20;
constexpr int QT = 32;                      // query frames per workgroup: one MFMA tile high
constexpr int KU = 16;                      // row pairs per step of the Gram loop
constexpr int K_SMALL = 160;               // list capacity of the two-accumulator instance
constexpr float TINY = 1.17549435e-38f;     // FLT_MIN

using f32x16 = __attribute__((ext_vector_type(16))) float;

__global__ __launch_bounds__(256) void k_nn_norms(const float* __restrict__ s, int64_t total, int rows, int F, float* __restrict__ norm) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;    // (signal, frame)
  if (e >= total) return;
  const float* a = s + (e / F) * rows * F + e % F;
  float acc = 0.0f;
  for (int r = 0; r < rows; ++r) {
    const float x = a[(int64_t)r * F];
    acc = fmaf(x, x, acc);
  }
  norm[e] = sqrtf(acc);
}

// A list entry is one 64-bit key: the similarity as an order-preserving integer above, ~frame below, so a larger key is a larger
// similarity or, of equal ones, the lower frame: no two candidates of a query share a key, and the list is the keys in decreasing
// order.  (-0 counts as +0.)
__device__ __forceinline__ unsigned long long nn_key(float v, int j) {
  const uint32_t u = __float_as_uint(v + 0.0f);
  return ((unsigned long long)(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u)) << 32) | (uint32_t)~j;
}
__device__ __forceinline__ float nn_key_sim(unsigned long long key) {
  const uint32_t u = (uint32_t)(key >> 32);
  return __uint_as_float((u >> 31) ? u ^ 0x80000000u : ~u);
}
__device__ __forceinline__ int nn_key_frame(unsigned long long key) { return (int)~(uint32_t)key; }

// one key into the list lk of n entries, capacity k; the whole wave calls it with the same arguments.  Needs n < k or key > lk[k - 1].
// From the top down, 64 slots per step: slot d takes entry d - 1 where that is below the key; the first step that meets a larger
// entry ends the walk, and the key goes into the slot under it.  At capacity the last entry has no slot and drops out.
__device__ __forceinline__ void nn_insert(unsigned long long* lk, int& n, unsigned long long& thr, int k, unsigned long long key, int lane) {
  const int n1 = min(n + 1, k);
  int p = 0;
  for (int base = n1 - 1; base >= 1; base -= 64) {
    const int d = base - lane;
    const bool has = d >= 1;
    unsigned long long x = 0;
    if (has) x = lk[d - 1];
    const bool mv = has && x < key;
    __builtin_amdgcn_wave_barrier();                          // every lane has read before any lane writes
    if (mv) lk[d] = x;
    const unsigned long long keep = __ballot(has && !mv);     // entries above the key: from some lane on, the list is sorted
    if (keep) { p = base - (__ffsll(keep) - 1); break; }
  }
  if (lane == 0) lk[p] = key;
  __builtin_amdgcn_wave_barrier();
  n = n1;
  if (n == k) thr = lk[k - 1];
}

// one chunk of the Gram loop: lane l's A and B operands of row pairs 0 .. KU - 1 from `row` on (row 2 u + (l >> 5), frame of l & 31)
template <int NACC>
__device__ __forceinline__ void nn_load(const float* row, int64_t step, unsigned qo, const unsigned (&jo)[NACC], float (&va)[KU],
                                        float (&vb)[NACC][KU]) {
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    const float* p = row + u * step;
    va[u] = p[qo];
#pragma unroll
    for (int n = 0; n < NACC; ++n) vb[n][u] = p[jo[n]];
  }
}

template <int NACC>
__device__ __forceinline__ void nn_mma(const float (&va)[KU], const float (&vb)[NACC][KU], f32x16 (&acc)[NACC]) {
#pragma unroll
  for (int u = 0; u < KU; ++u) {
#pragma unroll
    for (int n = 0; n < NACC; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[u], vb[n][u], acc[n], 0, 0, 0);
  }
}

template <int KCAP, int NACC>
__global__ __launch_bounds__(256) void k_nn_topk(const float* __restrict__ s, const float* __restrict__ norm, int rows, int F, int k, int width,
                                                 int qtiles, int32_t* __restrict__ idx, float* __restrict__ sim) {
  constexpr int JT = 128 * NACC, PITCH = JT + 8, WJ = 32 * NACC;
  __shared__ unsigned long long lk[QT][KCAP], qthr[QT];         // the lists; a query's last entry and length: its wave's alone
  __shared__ float tile[QT][PITCH];
  __shared__ float qn[QT];
  __shared__ int qcnt[QT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, half = lane >> 5;
  const int64_t sig = blockIdx.x / qtiles;
  const int i0 = (int)(blockIdx.x % qtiles) * QT;
  const float* a = s + sig * rows * F;
  const float* nrm = norm + sig * F;
  if (threadIdx.x < QT) {
    qn[threadIdx.x] = nrm[min(i0 + (int)threadIdx.x, F - 1)];
    qcnt[threadIdx.x] = 0;
    qthr[threadIdx.x] = 0;
  }
  __syncthreads();
  const int64_t step = 2 * (int64_t)F;
  const int qf = min(i0 + c, F - 1);                            // frames past the end read the last one; never selected or written
  const unsigned qo = (unsigned)(half * F + qf);
  for (int j0 = 0; j0 < F; j0 += JT) {
    f32x16 acc[NACC];
    int jf[NACC];
#pragma unroll
    for (int n = 0; n < NACC; ++n) {
      jf[n] = min(j0 + wave * WJ + n * 32 + c, F - 1);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[n][r] = 0.0f;
    }
    unsigned jo[NACC];                                          // a lane's offsets within a row pair: row half, its frame
#pragma unroll
    for (int n = 0; n < NACC; ++n) jo[n] = (unsigned)(half * F + jf[n]);
    // KU row pairs per chunk: the next chunk's loads are issued before this chunk's MFMAs and land under them (the scheduling
    // barriers keep them there).  Chunk c covers rows 2 KU c .. 2 KU (c + 1) - 1; past the last chunk the last is read again.
    const int pairs = rows >> 1, chunks = pairs / KU;
    float xa[KU], xb[NACC][KU], ya[KU], yb[NACC][KU];
    if (chunks > 0) nn_load<NACC>(a, step, qo, jo, xa, xb);
    for (int ch = 0; ch < chunks; ++ch) {
      nn_load<NACC>(a + (int64_t)min(ch + 1, chunks - 1) * KU * step, step, qo, jo, ya, yb);
      __builtin_amdgcn_sched_barrier(0);
      nn_mma<NACC>(xa, xb, acc);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        xa[u] = ya[u];
#pragma unroll
        for (int n = 0; n < NACC; ++n) xb[n][u] = yb[n][u];
      }
    }
    const float* pa = a + (int64_t)chunks * KU * step;
    for (int t = chunks * KU; t < pairs; ++t) {                 // the pairs left over, in row order
      const float av = pa[qo];
#pragma unroll
      for (int n = 0; n < NACC; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, pa[jo[n]], acc[n], 0, 0, 0);
      pa += step;
    }
    if (rows & 1) {                                             // an odd row count: the last row against a zero row
      const float* pl = a + (int64_t)(rows - 1) * F;
      const float av = half ? 0.0f : pl[qf];
#pragma unroll
      for (int n = 0; n < NACC; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, half ? 0.0f : pl[jf[n]], acc[n], 0, 0, 0);
    }
    // C/D: column = lane & 31 (candidate), row = (r & 3) + 8 (r >> 2) + 4 half (query)
#pragma unroll
    for (int n = 0; n < NACC; ++n) {
      const float nj = nrm[jf[n]];
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const int q = (rr & 3) + 8 * (rr >> 2) + 4 * half;
        tile[q][wave * WJ + n * 32 + c] = acc[n][rr] / fmaxf(qn[q] * nj, TINY);
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int q = wave; q < QT; q += 4) {
      const int i = i0 + q;
      if (i >= F) break;                                        // wave-uniform
      int cnt = qcnt[q];
      unsigned long long thr = qthr[q];
      for (int cb = 0; cb < JT; cb += 64) {
        const int j = j0 + cb + lane;
        const unsigned long long key = nn_key(tile[q][cb + lane], j);
        const bool cand = j < F && (j - i >= width || i - j >= width);
        unsigned long long m = __ballot(cand && (cnt < k || key > thr));
        while (m) {
          const int b = __ffsll(m) - 1;
          nn_insert(lk[q], cnt, thr, k, __shfl(key, b, 64), lane);
          m = __ballot(lane > b && cand && (cnt < k || key > thr));
        }
      }
      if (lane == 0) { qcnt[q] = cnt; qthr[q] = thr; }
    }
    __syncthreads();                                            // the tile is free again
  }
  for (int q = wave; q < QT; q += 4) {
    const int i = i0 + q;
    if (i >= F) break;
    const int cnt = qcnt[q];
    const int64_t o = (sig * F + i) * k;
    for (int t = lane; t < k; t += 64) {
      const bool live = t < cnt;
      const unsigned long long key = live ? lk[q][t] : 0;
      idx[o + t] = live ? nn_key_frame(key) : -1;
      if (sim) sim[o + t] = live ? nn_key_sim(key) : 0.0f;
    }
  }
}

__global__ __launch_bounds__(256) void k_nn_transpose(const float* __restrict__ s, int rows, int F, int rtiles, int ftiles, float* __restrict__ st) {
  __shared__ float t[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
  const unsigned per_sig = (unsigned)rtiles * ftiles;
  const int64_t sig = blockIdx.x / per_sig;
  const int r0 = (int)((blockIdx.x % per_sig) / ftiles) * 32, f0 = (int)((blockIdx.x % per_sig) % ftiles) * 32;
  const float* a = s + sig * rows * F;
  float* o = st + sig * rows * F;
  for (int y = ty; y < 32; y += 8)
    if (r0 + y < rows && f0 + tx < F) t[y][tx] = a[(int64_t)(r0 + y) * F + f0 + tx];
  __syncthreads();
  for (int y = ty; y < 32; y += 8)
    if (f0 + y < F && r0 + tx < rows) o[(int64_t)(f0 + y) * rows + r0 + tx] = t[tx][y];
}

// floats as integers of the same order (the bits stay recoverable; -0 sorts just below +0)
__device__ __forceinline__ uint32_t nn_ord(float v) {
  const uint32_t u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float nn_unord(uint32_t u) { return __uint_as_float((u >> 31) ? u ^ 0x80000000u : ~u); }

// One wave per workgroup: one frame, no = 64 >> ll rows, 1 << ll lanes per output (lane = l * no + o); dynamic LDS: [k + 1][no] uint32.
__global__ __launch_bounds__(64) void k_nn_median(const float* __restrict__ s, const float* __restrict__ st, const int32_t* __restrict__ idx, int rows, int F,
                                                  int k, int rchunks, int ll, float* __restrict__ out) {
  extern __shared__ uint32_t vals[];
  const int lane = threadIdx.x, no = 64 >> ll, L = 1 << ll, o = lane & (no - 1), l = lane >> (6 - ll);
  const int i = blockIdx.x % F;                                 // frames fastest: neighbouring workgroups write neighbouring floats
  const int rc = (blockIdx.x / F) % rchunks;
  const int64_t sig = (blockIdx.x / F) / rchunks;
  const int r = rc * no + o;
  const bool live = r < rows;
  const int32_t* li = idx + (sig * F + i) * k;
  const float* base = st + sig * rows * F + r;
  // The valid entries in order, each one's no rows side by side.  A lane packs its entry's slot and frame; an invalid entry (or a
  // lane past k) reads frame 0 into the spare slot k.  16 independent loads per step, so they overlap.
  int n = 0;
  for (int t0 = 0; t0 < k; t0 += 64) {
    const int t = t0 + lane;
    const int32_t j = t < k ? li[t] : -1;
    const bool ok = j >= 0 && j < F;
    const unsigned long long m = __ballot(ok);
    const int mine = ok ? ((n + __popcll(m & ((1ull << lane) - 1))) << 16) | j : k << 16;
    const int span = min(64, k - t0);
    for (int b0 = 0; b0 < span; b0 += 16) {
      uint32_t slot[16];
      float x[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int e = __shfl(mine, min(b0 + u, 63), 64);        // (past the span: a lane beyond k, invalid)
        slot[u] = (uint32_t)e >> 16;
        x[u] = live ? base[(int64_t)(e & 0xffff) * rows] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (l == 0 && b0 + u < 64) vals[slot[u] * no + o] = nn_ord(x[u]);
    }
    n += __popcll(m);
  }
  const int64_t oo = (sig * rows + r) * F + i;
  if (n == 0) {                                                 // no neighbours: the frame stays
    if (live && l == 0) out[oo] = s[oo];
    return;
  }
  __syncthreads();
  // The element of sorted position p is the largest x with #(w < x) <= p: its 32 bits from the top down, one count over the
  // neighbours per bit.  Lanes of one output count every L-th neighbour and add up.
  const int p = (n - 1) >> 1;                                   // n odd: the middle; n even: the lower of the two middle ones
  const uint32_t* w = vals + o;
  uint32_t res = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t piv = res | (1u << bit);
    int c = 0;
#pragma unroll 8
    for (int x = l; x < n; x += L) c += w[x * no] < piv ? 1 : 0;
    for (int m = no; m < 64; m <<= 1) c += __shfl_xor(c, m, 64);
    if (c <= p) res = piv;
  }
  float v = nn_unord(res);
  if (!(n & 1)) {                                               // the upper middle one: res again if #(w <= res) > p + 1, else the next above
    int c = 0;
    uint32_t up = 0xffffffffu;
#pragma unroll 8
    for (int x = l; x < n; x += L) {
      const uint32_t y = w[x * no];
      c += y <= res ? 1 : 0;
      up = y > res ? min(up, y) : up;
    }
    for (int m = no; m < 64; m <<= 1) {
      c += __shfl_xor(c, m, 64);
      up = min(up, (uint32_t)__shfl_xor((int)up, m, 64));
    }
    v = (v + (c > p + 1 ? v : nn_unord(up))) * 0.5f;
  }
  if (live && l == 0) out[oo] = v;
}

}  // namespace glowk_repet
