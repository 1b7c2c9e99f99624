"""GPU tests of the training sweep off the power-of-two shapes it was written against: image sides that are multiples of 2^L only
(12 x 12, 12 x 20, 24 x 8, 48 x 16, the shipped 96 x 64), odd pixel counts per level (3 x 1 and 1 x 1 images at the last level),
n_filters = 384, C > 1.  Every gradient tensor of glowk_param_grad against the fp64 autograd of the torch oracle, in both
arithmetics, with the bar of tests/test_gpu_training.py; the case list is checked to reach all nine instantiations of the
weight-gradient GEMM (launch_wgrad, csrc/glowk_training.hip).

Measured on an MI355X, worst |g - fp64| / max|g| over all tensors of a case (bar: 2e-4), float32 oracle | f32 sweep | f16x3 sweep:
  12x12_F128_n7   3.4e-6 | 2.1e-6 | 2.2e-6      12x12_F128_n1        1.1e-6 | 1.3e-6 | 1.3e-6      12x20_F512_n29   1.8e-6 | 1.3e-6 | 1.4e-6
  24x8_F384_n33   2.4e-6 | 7.1e-7 | 7.2e-7      8x8_F384_n5          1.7e-6 | 7.2e-7 | 1.5e-6      8x16_C4_F256_n3  1.3e-6 | 9.3e-7 | 9.1e-7
  96x64_F512_n2   1.7e-6 | 5.7e-7 | 4.0e-7      12x12_C2_F256_notop  9.1e-7 | 6.3e-7 | 5.3e-7      48x16_L4_F512_n3 1.5e-6 | 7.6e-7 | 7.6e-7
  24 x 8, K = 3, the three batching paths: 8.9e-7 (f32), 9.0e-7 (f16x3); between paths 4.6e-9 (f32), 0 / 1.4e-7 (f16x3) of the vector's norm.
Every f16x3 sweep stayed on the split kernels (no k_net_f32 launch, no range trip): the 32x32x16 family at n_filters 128, the
half-wave 16x16x32 form elsewhere.  No kernel was found wrong at these shapes.  What the first runs did find is in the comment at
the seeds: single ReLU inputs within float32 rounding of zero, worth 1e-3 of a tensor each."""
import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib
from audiosourcesep_amd.config import GlowConfig
from audiosourcesep_amd.engine import GlowEngine
from audiosourcesep_amd.flow_models.flow_glow import GlowFlow
from audiosourcesep_amd.synthetic import synthetic_mel_tiles, synthetic_params
from oracle import glowref_torch as RT
from tests.test_gpu_training import FROZEN_IN_VECTOR, dev, engine_grads, oracle_param_grads

pytestmark = pytest.mark.gpu

# id: (config, tiles, input seed) -- pixels per level Q = tiles * h * w in the comment
CASES = {
    "12x12_F128_n7": (GlowConfig(H=12, W=12, C=1, L=2, K=2, F=128), 7, 17),                            # 252, 63
    "12x12_F128_n1": (GlowConfig(H=12, W=12, C=1, L=2, K=2, F=128), 1, 17),                            # 36, 9
    "12x20_F512_n29": (GlowConfig(H=12, W=20, C=1, L=2, K=2, F=512), 29, 242),                          # 1740, 435
    "24x8_F384_n33": (GlowConfig(H=24, W=8, C=1, L=3, K=2, F=384), 33, 204),                            # 1584, 396, 99
    "8x8_F384_n5": (GlowConfig(H=8, W=8, C=1, L=3, K=2, F=384), 5, 17),                                # 80, 20, 5
    "12x12_C2_F256_notop": (GlowConfig(H=12, W=12, C=2, L=2, K=2, F=256, learntop=False), 5, 17),      # 180, 45
    "8x16_C4_F256_n3": (GlowConfig(H=8, W=16, C=4, L=2, K=2, F=256), 3, 17),                           # 96, 24
    "48x16_L4_F512_n3": (GlowConfig(H=48, W=16, C=1, L=4, K=1, F=512), 3, 24),                         # 576, 144, 36, 9
    "96x64_F512_n2": (GlowConfig(H=96, W=64, C=1, L=3, K=1, F=512), 2, 247),                            # 3072, 768, 192
}
# Seeds: 17 as in tests/test_gpu_training.py, but for the four cases with 0.8 to 4.5 million ReLU inputs.  Among that many one or
# two land within float32 rounding of zero with most seeds, and an isolated ReLU decision that falls the other way
# moves a tensor of the deeper levels by 1e-3 or more of its largest entry: with the ActNorm tensors the GPU initialises, the
# nearest input is 0.22 roundings from zero for 12 x 20 with seed 17 and 0.48 with 19, 0.08 / 0.45 for 24 x 8, 0.24 for 96 x 64 and
# 2.84 for 48 x 16 with 17 (relu_margin below).  Those four take the first seed from 17 upwards whose margin in the fp64 oracle
# (the engine is not consulted) is RELU_MARGIN or more: 4.08, 6.80, 4.23 and 6.24; 17 itself has 13 or more in the other cases.
PATHS_SEED = 496                       # likewise for the K = 3 flow of the batching-path test (margin 5.08)

PRECISIONS = {"f32": _lib.PREC_F32, "f16x3": _lib.PREC_F16X3}
GRAD_ATOL, GRAD_RTOL = 2e-4, 2e-3      # the bar of tests/test_gpu_training.py: atol = 2e-4 max|ref|, rtol = 2e-3
INPUT_BAR = 2e-5                       # precondition on a case's input: the float32 oracle within this of fp64 on every tensor
# ... and no ReLU input of the fp64 oracle nearer to zero than this many float32 roundings of its own sum.  One rounding is what a
# single partial sum of exact inputs loses; the inputs of a deeper network carry the roundings of everything before them.  Seen to
# fall the other way: a unit at 0.24 (96 x 64, seed 17: the f32 sweep and the float32 oracle), one at 1.65 (12 x 20, seed 19: both
# sweeps) and one at 3.07 (24 x 8 with K = 3, seed 28: the f16x3 sweep, whose products drop the lo x lo term and are exact to 2^-22,
# four roundings).  Not a bound on the engine: a distance the inputs keep from where a float32-class sum cannot decide.
RELU_MARGIN = 4.0

WGRAD_INSTANCES = ("k_wgrad_nt<1,true>", "k_wgrad_nt<1,false>", "k_wgrad_h3<2,2,4,4,true>", "k_wgrad_h3<2,2,4,2,true>",
                   "k_wgrad_h3<2,2,4,2,false>", "k_wgrad_h3<2,2,2,2,true>", "k_wgrad_h3<2,2,2,2,false>", "k_wgrad_h3<1,2,4,1,true>",
                   "k_wgrad_h3<1,2,4,1,false>")
UNTESTED_BEFORE = ("k_wgrad_nt<1,false>", "k_wgrad_h3<2,2,4,2,false>", "k_wgrad_h3<2,2,2,2,true>", "k_wgrad_h3<2,2,2,2,false>",
                   "k_wgrad_h3<1,2,4,1,false>")


def wgrad_instance(split, M, N, Q):
    """launch_wgrad's choice (csrc/glowk_training.hip) for C[M][N] = A . B^T over Q pixels, restated."""
    vec = "true" if Q % 4 == 0 else "false"
    if not split:
        return "k_wgrad_nt<1,%s>" % vec
    big = N >= 256
    big8 = big and M % 256 == 0
    if big8 and N % 256 == 0 and Q % 4 == 0:
        return "k_wgrad_h3<2,2,4,4,true>"
    return "k_wgrad_h3<%s,%s>" % ("2,2,4,2" if big8 else "2,2,2,2" if big else "1,2,4,1", vec)


def case_instances(cfg, n):
    """{(instance, split)} over the three GEMMs of every level: conv3 (N = 9 c), conv2 (N = F), conv1 (N = 9 c / 2 + 1); M = F."""
    return {wgrad_instance(split, cfg.F, N, n * h * w) for (h, w, c) in cfg.level_shapes() for N in (9 * c, cfg.F, 9 * (c // 2) + 1)
            for split in (False, True)}


def test_the_case_list_reaches_every_weight_gradient_instance():
    reached = {name: case_instances(cfg, n) for name, (cfg, n, _) in CASES.items()}
    union = set().union(*reached.values())
    assert union == set(WGRAD_INSTANCES), sorted(set(WGRAD_INSTANCES) ^ union)
    for inst in UNTESTED_BEFORE:
        by = [name for name, r in reached.items() if inst in r]
        assert len(by) >= 2, (inst, by)


def mel_tiles(n, cfg, seed):
    """synthetic_mel_tiles; for C > 1 (it repeats one channel) plus Gaussian noise of 3 dB, so that the channels differ."""
    x = synthetic_mel_tiles(n, cfg, seed=seed)
    if cfg.C > 1:
        x = np.clip(x + np.random.default_rng(seed + 1).normal(0.0, 3.0, x.shape), cfg.minval, cfg.maxval)
    return np.ascontiguousarray(x, dtype=np.float32)


def engine_for(cfg, init_tiles=8, seed=2024, init_seed=77):
    """synthetic.calibrated_engine, with the data-init minibatch from mel_tiles (channels that differ for C > 1)."""
    params = synthetic_params(cfg, seed=seed)
    eng = GlowEngine(cfg, device=0)
    eng.load_params(params)
    eng.actnorm_data_init(mel_tiles(init_tiles, cfg, init_seed), runtime_order=True, raw_minibatch_quirk=False)
    params.update(eng.actnorm_params())
    return eng, params


def tensor_errors(got, ref):
    return {k: float(np.abs(got[k] - r).max() / max(np.abs(r).max(), 1e-12)) for k, r in ref.items()}


def relu_margin(x, params, cfg):
    """How far the nearest ReLU input of the fp64 oracle is from zero, in units of what float32 can resolve there:
    min over every output of conv1 / conv2 of |conv + b| / (2^-24 (|x| * |kernel| + |b|)), with where it is.  A float32 evaluation
    rounds each partial sum to 2^-24 of its size, so below ~1 the sign of such a unit -- its ReLU mask, and with it a whole pixel's
    contribution to one channel's gradients -- depends on the order of the sum, not on the arithmetic being right."""
    worst = [np.inf, ""]
    calls = [0]
    conv = RT._conv_same

    def spy(xx, kernel, bias):
        y = conv(xx, kernel, bias)
        if calls[0] % 3 != 2:                                   # conv1, conv2 feed a ReLU; conv3 does not
            r = (y.abs() / (2.0 ** -24 * conv(xx.abs(), kernel.abs(), bias.abs()))).min().item()
            if r < worst[0]:
                worst[:] = [r, "network %d (in the order the oracle runs them), conv%d" % (calls[0] // 3, calls[0] % 3 + 1)]
        calls[0] += 1
        return y

    RT._conv_same = spy
    try:
        with torch.no_grad():
            RT.log_prob(torch.from_numpy(x).double(), RT.to_torch(params, torch.float64), cfg.as_dict())
    finally:
        RT._conv_same = conv
    return tuple(worst)


def reference(name, x, params, cfg, scale):
    """fp64 autograd of the oracle, after two preconditions on the INPUT (tiles and the ActNorm tensors the GPU initialised) -- not
    checks of the engine, and never a reason to widen its bar: if one fails, change the case's seed.
    (1) the oracle evaluated in float32 is within INPUT_BAR of fp64 on every tensor;
    (2) no ReLU input of the fp64 oracle is within float32 rounding of zero (relu_margin >= RELU_MARGIN).  (1) alone does not hold a case
        still: it depends on the host's float32 convolution (12 x 20 with seed 19: 2.5e-6 on one host, 1.7e-3 on another), and
        the engine sums in another order again -- with that seed both of its arithmetics were 1.7e-3 off at b1/s1/nn/conv1/kernel
        and 1.2e-3 at its bias, everything else <= 7e-6: exactly what flipping ONE unit of the oracle does (channel 102 of that
        conv1 at one pixel, fp64 input 6.0e-8, margin 1.65)."""
    lp_ref, ref = oracle_param_grads(x, params, cfg, scale)
    _, ref32 = oracle_param_grads(x, params, cfg, scale, dtype=torch.float32)
    yard = tensor_errors(ref32, ref)
    margin, where = relu_margin(x, params, cfg)
    print(name, "input: float32 oracle worst |g - fp64| / max|g| %.1e (%s); nearest ReLU input %.2f float32 roundings from zero (%s)"
          % (max(yard.values()), max(yard, key=yard.get), margin, where))
    assert max(yard.values()) <= INPUT_BAR, "precondition on the input of %s (not on the engine): the float32 oracle is %.1e from fp64 at %s" % (
        name, max(yard.values()), max(yard, key=yard.get))
    assert margin >= RELU_MARGIN, "precondition on the input of %s (not on the engine): a ReLU input of the fp64 oracle lies %.2f float32 roundings from zero, %s" % (
        name, margin, where)
    return lp_ref, ref


def check_grads(got, ref, tag):
    for k, r in ref.items():
        np.testing.assert_allclose(got[k], r, atol=GRAD_ATOL * max(np.abs(r).max(), 1e-12), rtol=GRAD_RTOL, err_msg="%s %s" % (tag, k))


def worst_per_kind(errs):
    worst = {}
    for k, e in errs.items():
        kind = k.split("/", 2)[-1] if k[0] == "b" else k
        worst[kind] = max(worst.get(kind, 0.0), e)
    return {k: "%.1e" % v for k, v in sorted(worst.items())}


@pytest.mark.parametrize("name", list(CASES))
def test_parameter_gradients_off_the_power_of_two_shapes(name):
    """log_prob and every gradient tensor against the fp64 autograd, the untrained entries of the vector exactly zero, a second call
    bit for bit -- in f32 and in f16x3, where the sweep must stay on the split kernels (no k_net_f32 launch, no range trip)."""
    cfg, n, seed = CASES[name]
    eng, params = engine_for(cfg)
    x = mel_tiles(n, cfg, seed)
    scale = -1.0 / 32.0
    lp_ref, ref = reference(name, x, params, cfg, scale)
    for prec in ("f32", "f16x3"):
        eng.set_precision(PRECISIONS[prec])
        eng.set_range_policy("error")
        before = eng.kernel_families()
        lp, got, flat = engine_grads(eng, params, x, scale)
        after = eng.kernel_families()
        errs = tensor_errors(got, ref)
        print(name, prec, "worst |g - fp64| / max|g| %.1e; per tensor kind:" % max(errs.values()), worst_per_kind(errs),
              "; launches by family", {k: after[k] - before[k] for k in after if after[k] != before[k]})
        np.testing.assert_allclose(lp, lp_ref, rtol=1e-6 if prec == "f32" else 2e-6, err_msg=prec)
        check_grads(got, ref, prec)
        # non-trainable entries of the vector and its padding carry exactly zero
        used = np.zeros(flat.shape, bool)
        for k in params:
            if k.endswith(("inv1x1/P", "inv1x1/P_inv", "inv1x1/sign_S")):
                continue
            off, cnt = eng.param_slice(k)
            if k.split("/", 2)[-1] in FROZEN_IN_VECTOR or (not cfg.learntop and k.startswith("prior/")):
                assert not flat[off:off + cnt].any(), (prec, k)
            used[off:off + cnt] = True
        assert not flat[~used].any(), prec
        _, _, flat2 = engine_grads(eng, params, x, scale)
        assert np.array_equal(flat, flat2), prec                 # repeatable bit for bit (fixed-order split-K sums, no atomics)
        if prec == "f16x3":
            # the sweep ran the split kernels at every level: glowk_param_grad takes the exact ones for the WHOLE sweep when one level
            # has no storing split instance, and a case that does so has not run k_wgrad_h3 at all
            assert eng.kernel_families()["f32"] == before["f32"], (before, eng.kernel_families())
            assert eng.range_status() == (False, 0)
    eng.close()


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_step_by_step_and_recompute_paths_at_an_odd_shape(prec, monkeypatch):
    """The three ways through the weight-gradient work (tests/test_gpu_training.py: the level batch, GLOWK_TRAIN_PERSTEP,
    GLOWK_TRAIN_RECOMPUTE) on 24 x 8 tiles, n_filters 384, K = 3, 33 tiles: 396 and 99 pixels at the deeper levels, 3 x 1 images."""
    cfg, n, _ = CASES["24x8_F384_n33"]
    cfg = GlowConfig(H=cfg.H, W=cfg.W, C=cfg.C, L=cfg.L, K=3, F=cfg.F)
    x = mel_tiles(n, cfg, PATHS_SEED)
    scale = -1.0 / n
    flats = {}
    try:
        for mode in ("batch", "GLOWK_TRAIN_PERSTEP", "GLOWK_TRAIN_RECOMPUTE"):
            if mode != "batch":
                monkeypatch.setenv(mode, "1")
                _lib.load().glowk_reload_env()       # (the engine reads its switches when the library loads)
            eng, params = engine_for(cfg)
            if prec == "f16x3":
                eng.set_precision(_lib.PREC_F16X3)
                eng.set_range_policy("error")
            lp, got, flat = engine_grads(eng, params, x, scale)
            flats[mode] = flat.astype(np.float64)
            if mode == "batch":
                lp_ref, ref = reference("24x8_F384_n33 with K = 3", x, params, cfg, scale)
            print(prec, mode, "worst |g - fp64| / max|g| %.1e" % max(tensor_errors(got, ref).values()))
            check_grads(got, ref, mode)
            eng.close()
            if mode != "batch":
                monkeypatch.delenv(mode)
                _lib.load().glowk_reload_env()
    finally:
        monkeypatch.undo()
        _lib.load().glowk_reload_env()
    ref_norm = np.linalg.norm(flats["batch"])
    for mode in ("GLOWK_TRAIN_PERSTEP", "GLOWK_TRAIN_RECOMPUTE"):
        rel = np.linalg.norm(flats[mode] - flats["batch"]) / ref_norm
        print(prec, mode, "against the level batch: relative l2 difference %.1e" % rel)
        assert rel < 2e-6, mode


@pytest.mark.parametrize("name", ["24x8_F384_n33", "12x12_C2_F256_notop"])
def test_split_training_steps_refresh_the_f16_images_at_odd_shapes(name):
    """Four Adamax steps in f16x3 on 24 tiles, the fp16 hi / lo images rebuilt on the device after each (k_f16_*, k_repack_f16) at
    n_filters 384 and at C = 2: a fresh engine that loads the trained variables -- the host packs its images -- gives bitwise the same
    log_prob, latent and input gradient in f16x3 and the same log_prob in f16x2, and log_prob matches the fp64 oracle on them."""
    cfg = CASES[name][0]
    eng, _ = engine_for(cfg, init_tiles=16)
    flow = GlowFlow(eng)
    eng.set_precision(_lib.PREC_F16X3)
    eng.set_range_policy("error")
    x_host = mel_tiles(24, cfg, 41)
    x = dev(x_host)
    losses = []
    for it in range(4):
        lp, g = eng.param_grad(x, -1.0 / 24.0)
        losses.append(float(-lp.mean()))
        eng.apply_gradients(g, optimizer="adamax", lr=5e-4)
    assert np.isfinite(losses).all() and losses[-1] != losses[0]
    lp_dev, z_dev = eng.log_prob(x, return_latent=True)          # images refreshed by the device
    lpg_dev, gx_dev = eng.log_prob_grad(x)
    sd = flow.state_dict()
    other, _ = engine_for(cfg, init_tiles=16)
    GlowFlow(other).load_state_dict(sd)                            # images packed by the host
    other.set_precision(_lib.PREC_F16X3)
    other.set_range_policy("error")
    lp_host, z_host = other.log_prob(x, return_latent=True)
    lpg_host, gx_host = other.log_prob_grad(x)
    assert torch.equal(lp_dev, lp_host) and torch.equal(z_dev, z_host) and torch.equal(gx_dev, gx_host) and torch.equal(lpg_dev, lpg_host)
    for e in (eng, other):
        e.set_precision(_lib.PREC_F16X2)
    assert torch.equal(eng.log_prob(x), other.log_prob(x))
    lp_ref = RT.log_prob(torch.from_numpy(x_host.astype(np.float64)), RT.to_torch(sd, torch.float64), cfg.as_dict())[0].numpy()
    np.testing.assert_allclose(lp_dev.cpu().numpy(), lp_ref, rtol=2e-6)
    assert eng.range_status() == (False, 0) and other.range_status() == (False, 0)
    eng.close()
    other.close()
