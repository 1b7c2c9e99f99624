// Activation scale before the fp16 split, shared by the kernels (glowk_kernels.h: gathered inputs are scaled by it) and the host
// packer (glowk_pack.h: folded into the split scales and range limits).  Overflow (a hidden activation above 65504 / scale) turns
// into inf/NaN, underflow only costs the low bits of activations below ~6e-5 / scale * 2^11: 4 leaves |activation| < 16 376 with
// activations down to 0.03 fully split; log_prob accuracy measured identical for 1, 4 and 32 (scripts/act_scale_probe.py).
#pragma once
#define GLOWK_ACT_SCALE 4.0f

// conv1 of the forward 16x16x32 kernels (RingS; K1 = 9 * input channels, one more row carries the bias): the three split terms
// w_hi x_hi + w_hi x_lo + w_lo x_hi are three dot products over the same output tile, so they can be ONE contraction over a
// stacked K of 3 K1 + 2 slots, A = [w_hi | w_hi | w_lo | b_hi b_lo], B = [x_hi | x_lo | x_hi | c c] (c: the bias constant,
// whose lo half is zero), at one MFMA per k-step of 32 instead of three.  A level shape takes the stacked layout when it needs
// no more operand pieces (LDS, DMA) and no more fragment registers than the three-term one: 2 stacked k-steps cost what one
// three-term k-step costs (a hi and a lo piece per row block; 16 fragment registers).  K1 = 18, 36 (c = 4, 8): 2 and 4 stacked
// k-steps for 1 and 2; K1 = 72, 144: 7 > 6 and 14 > 10, they keep the three-term layout.  The packer writes the image and the
// kernels read it by this one rule.
constexpr int glowk_conv1_ks(int K1) { return (K1 + 1 + 31) / 32; }
constexpr int glowk_conv1_ks_stacked(int K1) { return (3 * K1 + 2 + 31) / 32; }
constexpr bool glowk_conv1_stacked(int K1) { return glowk_conv1_ks_stacked(K1) <= 2 * glowk_conv1_ks(K1); }

// conv3 of the forward 16x16x32 kernels (RingS; M = 9 c output rows in 16-row tiles): row order of the A image at c = 8 and 16.
// A lane of group kq = lane >> 4 holds, per 16-pixel half, register r of row tile mt = row 16 mt + 4 kq + r; the tiles of one
// accumulator group (<= 6 tiles: mt = 6 gi + ml) are live together, s = 4 ml + r numbers the group's registers of a lane.  The
// rows are ordered so that registers 3 u, 3 u + 1, 3 u + 2 of a lane group are the taps dx = -1, 0, +1 of ONE (dy, channel): the
// kernels can then add the three horizontal taps in registers (two DPP row shifts: the neighbour pixels sit in the neighbour
// lanes) and store P with 3 c rows instead of 9 c.  Triplet u of lane group kq in accumulator group gi is row
//     T = 32 gi + 4 u + kq = (dy + 1) c + channel
// of that pre-summed P (a full group of six tiles holds 4 x 8 triplets); c = 8: one group of five tiles, six triplets per lane
// group and two spare registers (zero rows); c = 16: groups of six and three tiles, 8 + 4 triplets, no padding.  Every other c keeps
// the natural order (row m = tap c + channel).  The packer writes the image, the kernels decode their store rows and the
// per-row constants (which stay in natural order) by this one rule.
constexpr bool glowk_conv3_permuted(int c) { return c == 8 || c == 16; }
// row T of the pre-summed P that image row m belongs to, times 3, plus its tap dx + 1; -1: a padding row
constexpr int glowk_conv3_triplet(int c, int m) {
  const int nmt = (9 * c + 15) / 16;
  const int mt = m / 16, kq = (m % 16) / 4, r = m % 4;
  const int gi = mt / 6, ml = mt % 6;
  const int gn = nmt - 6 * gi < 6 ? nmt - 6 * gi : 6;
  const int s = 4 * ml + r, u = s / 3;
  if (mt >= nmt || u >= 4 * gn / 3) return -1;
  return 3 * (32 * gi + 4 * u + kq) + s % 3;
}
// natural row tap * c + channel (tap = 3 (dy + 1) + dx + 1) held by image row m; 9 c: a padding row.  Within a lane's register the
// natural row of lane group kq is that of lane group 0 plus kq (4 u is a multiple of 4, c a multiple of 8).
constexpr int glowk_conv3_row(int c, int m) {
  if (!glowk_conv3_permuted(c)) return m < 9 * c ? m : 9 * c;
  const int t = glowk_conv3_triplet(c, m);
  if (t < 0) return 9 * c;
  const int T = t / 3, dxi = t % 3;
  return (3 * (T / c) + dxi) * c + T % c;
}
