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
