// glowk: the index rules of the convolutive NMF kernels (glowk_nmfd.h), in plain C++ so that a host program can run them without
// HIP (tests/nmfd_index_sanitize_main.cpp sweeps them under AddressSanitizer + UBSan against straightforward loops).  The kernels
// and the entry points call the same functions.
//
// The stacked view: component k at template frame tau is the stacked component s = k Tw + tau (k-major, so that W [rows][K][Tw] read
// as [rows][K Tw] is the stacked dictionary and a source's component range is one stacked range); Hs[s][t] = H[k][t - tau], an exact
// zero for t < tau.  The cut into tiles and chunks is nmf_plan's at K Tw components.
#pragma once
#include "glowk_nmf_index.h"

namespace glowk_nmfd {

using glowk_nmf::NmfPlan;
using glowk_nmf::nmf_plan;

constexpr int MAX_TW = 32;                  // template frames
constexpr int MAX_STACK = 128;              // K Tw: the stacked components one pass over the accumulators holds

// s = k Tw + tau, 0 <= tau < Tw
GLOWK_NMF_HD void nmfd_split(int s, int Tw, int& k, int& tau) {
  k = s / Tw;
  tau = s - k * Tw;
}

// (k, tau) of s + 2 from (k, tau) of s where `go`, else unchanged; without a division and without a branch (the kernels call it
// between loads that are to be in flight together): two carries, tau + 2 < 3 Tw
GLOWK_NMF_HD void nmfd_advance2(int Tw, int& k, int& tau, bool go = true) {
  const int t2 = tau + 2, c1 = t2 >= Tw ? 1 : 0, c2 = t2 >= 2 * Tw ? 1 : 0;
  const int kn = k + c1 + c2, tn = t2 - (c1 + c2) * Tw;
  k = go ? kn : k;
  tau = go ? tn : tau;
}

// The H update's stacked numerators and denominators of one signal, [2][K Tw][frames]: the first launch writes every (which, s, t)
// with t < frames, the second adds the Tw shifted rows of a component.
GLOWK_NMF_HD int64_t nmfd_plane_floats(int KS, int frames) { return (int64_t)2 * KS * frames; }
GLOWK_NMF_HD int64_t nmfd_plane_index(int which, int s, int t, int KS, int frames) { return ((int64_t)which * KS + s) * frames + t; }

// The template frames of component k that frame t of H meets: tau < nmfd_taps(Tw, frames, t) keeps t + tau inside the signal.
GLOWK_NMF_HD int nmfd_taps(int Tw, int frames, int t) { return frames - t < Tw ? frames - t : Tw; }

// The bytes of workspace per call: the largest of the W update's partial sums, the divergence's partial sums and the H update's plane.
GLOWK_NMF_HD size_t nmfd_work_bytes(int nsig, int rows, int frames, int K, int Tw) {
  const int KS = K * Tw;
  const NmfPlan p = nmf_plan(rows, frames, KS);
  int64_t m = glowk_nmf::nmf_w_part_floats(p, rows, KS) * 4;
  const int64_t b = glowk_nmf::nmf_div_parts(p) * 8, c = nmfd_plane_floats(KS, frames) * 4;
  if (b > m) m = b;
  if (c > m) m = c;
  return (size_t)nsig * (size_t)m;
}

}  // namespace glowk_nmfd
