// Activation scale before the fp16 split, shared by the kernels (glowk_kernels.h: gathered inputs are scaled by it) and the host
// packer (glowk_pack.h: folded into the split scales and range limits).  Overflow (a hidden activation above 65504 / scale) turns
// into inf/NaN, underflow only costs the low bits of activations below ~6e-5 / scale * 2^11: 4 leaves |activation| < 16 376 with
// activations down to 0.03 fully split; log_prob accuracy measured identical for 1, 4 and 32 (scripts/act_scale_probe.py).
#pragma once
#define GLOWK_ACT_SCALE 4.0f
