"""GPU tests of the training step (train_glow.py:29-44): every parameter gradient of the mean negative
log-likelihood against the fp64 autograd of the torch oracle, the optimizer step against the Keras Adamax / Adam formulas, the
device-side refresh of the packed kernel images against the oracle evaluated on the updated variables, and a short loop."""
import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib
from audiosourcesep_amd.config import GlowConfig
from audiosourcesep_amd.flow_models.flow_glow import GlowFlow
from audiosourcesep_amd.synthetic import synthetic_mel_tiles, calibrated_engine
from oracle import glowref as R
from oracle import glowref_torch as RT

pytestmark = pytest.mark.gpu
PRIMARY_FAMILIES = ("f32", "h3_32x32x16", "h3s_16x16x32", "h3s_half", "fused")   # (co_resident / small_grid_q count subsets of these)

TRAINABLE = ("actnorm/log_scale", "actnorm/shift", "inv1x1/L", "inv1x1/log_S", "inv1x1/U", "nn/conv1/kernel", "nn/conv1/bias",
             "nn/bn1/gamma", "nn/bn1/beta", "nn/conv2/kernel", "nn/conv2/bias", "nn/bn2/gamma", "nn/bn2/beta", "nn/conv3/kernel",
             "nn/conv3/bias", "prior/loc", "prior/log_scale")
FROZEN_IN_VECTOR = ("nn/bn1/mean", "nn/bn1/var", "nn/bn2/mean", "nn/bn2/var")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def oracle_param_grads(x, params, cfg, scale, dtype=torch.float64):
    """d (scale * sum_n log_prob(x_n)) / d theta for every trainable tensor, fp64 reverse mode over oracle/glowref_torch.py
    (dtype=torch.float32: the same oracle in float32, the yardstick of what a plain fp32 implementation delivers)."""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=k.split("/", 2)[-1] in TRAINABLE or k in TRAINABLE)
         for k, v in params.items()}
    lp, _ = RT.log_prob(torch.from_numpy(x).to(dtype), p, cfg.as_dict())
    names = [k for k, v in p.items() if v.requires_grad]
    grads = torch.autograd.grad(scale * lp.sum(), [p[k] for k in names], allow_unused=True)
    return lp.detach().numpy(), {k: (g.numpy() if g is not None else np.zeros_like(params[k], dtype=np.float64)) for k, g in zip(names, grads)}


def engine_grads(eng, params, x, scale):
    lp, g = eng.param_grad(dev(x), scale)
    g = g.cpu().numpy()
    out = {}
    for name in params:
        if name.endswith(("inv1x1/P", "inv1x1/P_inv", "inv1x1/sign_S")):
            continue
        off, cnt = eng.param_slice(name)
        out[name] = g[off:off + cnt].reshape(np.asarray(params[name]).shape)
    return lp.cpu().numpy(), out, g


CASES = {
    "L2_K2_F128": (GlowConfig(H=16, W=16, C=1, L=2, K=2, F=128), 5),
    "L3_K2_F128_rect": (GlowConfig(H=16, W=32, C=1, L=3, K=2, F=128), 3),
    "L2_K3_F256_notop": (GlowConfig(H=16, W=16, C=1, L=2, K=3, F=256, learntop=False), 4),
    "L4_K1_F128": (GlowConfig(H=16, W=16, C=1, L=4, K=1, F=128), 3),
    "configB_shape_K2": (GlowConfig(H=64, W=64, C=1, L=3, K=2, F=512), 3),
    "L3_K2_F256": (GlowConfig(H=32, W=32, C=1, L=3, K=2, F=256), 6),
}


@pytest.mark.parametrize("name", list(CASES))
def test_parameter_gradients_match_fp64_autograd(name):
    cfg, n = CASES[name]
    eng, params = calibrated_engine(cfg, device=0, init_tiles=8)
    x = synthetic_mel_tiles(n, cfg, seed=17)
    scale = -1.0 / 32.0                                     # loss = sum(-log_prob) / global batch (train_glow.py:29-31), global batch 32
    lp_ref, ref = oracle_param_grads(x, params, cfg, scale)
    lp, got, flat = engine_grads(eng, params, x, scale)
    np.testing.assert_allclose(lp, lp_ref, rtol=1e-6)
    worst = {}
    for k, r in ref.items():
        g = got[k]
        denom = max(np.abs(r).max(), 1e-12)
        worst[k.split("/", 2)[-1] if k[0] == "b" else k] = max(worst.get(k, 0.0), float(np.abs(g - r).max() / denom))
        # fp32 kernels, sums over up to 12 288 pixels: a few 1e-5 of the tensor's largest entry; 2e-4 asserted
        np.testing.assert_allclose(g, r, atol=2e-4 * denom, rtol=2e-3, err_msg=k)
    print(name, "worst |g - fp64| / max|g| per tensor kind:", {k: "%.1e" % v for k, v in sorted(worst.items())})
    # non-trainable entries of the vector carry zero gradient; nothing else is in it
    used = np.zeros(flat.shape, bool)
    for k in params:
        if k.endswith(("inv1x1/P", "inv1x1/P_inv", "inv1x1/sign_S")):
            continue
        off, cnt = eng.param_slice(k)
        if k.split("/", 2)[-1] in FROZEN_IN_VECTOR or (not cfg.learntop and k.startswith("prior/")):
            assert not flat[off:off + cnt].any(), k
        used[off:off + cnt] = True
    assert not flat[~used].any()
    # repeatable bit for bit (fixed-order split-K sums, no atomics)
    _, _, flat2 = engine_grads(eng, params, x, scale)
    assert np.array_equal(flat, flat2)


def keras_update(opt, p, g, m, v, t, lr):
    b1, b2, eps = 0.9, 0.999, 1e-7
    m = b1 * m + (1 - b1) * g
    if opt == "adamax":
        v = np.maximum(b2 * v, np.abs(g))
        p = p - lr / (1 - b1 ** t) * m / (v + eps)
    else:
        v = b2 * v + (1 - b2) * g * g
        p = p - lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (np.sqrt(v) + eps)
    return p, m, v


@pytest.mark.parametrize("name", ["L2_K2_F128", "L2_K3_F256_notop", "configB_shape_K2", "L3_K2_F256"])
def test_parameter_gradients_in_the_split_arithmetic(name):
    """glowk_param_grad with the handle in f16x3: the sweep runs the fp16-split kernels (k_net_h3 with hidden stores, planar arrays
    in scaled units, undone in the assembly) -- fp32-class, so the same bar against the fp64 autograd; and it is a different
    code path from the exact one (not bitwise equal), with no range-guard fallback on a normalised flow."""
    cfg, n = CASES[name]
    eng, params = calibrated_engine(cfg, device=0, init_tiles=8)
    x = synthetic_mel_tiles(n, cfg, seed=17)
    scale = -1.0 / 32.0
    lp_ref, ref = oracle_param_grads(x, params, cfg, scale)
    _, _, flat32 = engine_grads(eng, params, x, scale)
    eng.set_precision(_lib.PREC_F16X3)
    eng.set_range_policy("error")
    lp, got, flat = engine_grads(eng, params, x, scale)
    np.testing.assert_allclose(lp, lp_ref, rtol=2e-6)
    worst = 0.0
    for k, r in ref.items():
        denom = max(np.abs(r).max(), 1e-12)
        worst = max(worst, float(np.abs(got[k] - r).max() / denom))
        np.testing.assert_allclose(got[k], r, atol=2e-4 * denom, rtol=2e-3, err_msg=k)
    print(name, "f16x3 sweep: worst |g - fp64| / max|g| over all tensors %.1e" % worst)
    assert not np.array_equal(flat, flat32) and eng.range_status() == (False, 0)
    _, _, flat2 = engine_grads(eng, params, x, scale)
    assert np.array_equal(flat, flat2)                     # repeatable bit for bit


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_step_by_step_and_recompute_paths_agree_with_the_level_batches(prec, monkeypatch):
    """Three ways through the weight-gradient work, chosen by free memory (forced here by the environment switches the engine reads
    when it sizes its training buffers): a level's steps as one batch of launches (default), step by step (GLOWK_TRAIN_PERSTEP), and
    step by step with every step's forward network re-run instead of its hiddens kept (GLOWK_TRAIN_RECOMPUTE).  Same sums in a
    different split-K order: equal to fp32 rounding, all three within the bar of the fp64 autograd."""
    cfg, n = GlowConfig(H=32, W=32, C=1, L=3, K=3, F=256), 5
    x = synthetic_mel_tiles(n, cfg, seed=23)
    scale = -1.0 / n
    flats = {}
    try:
        for mode in ("batch", "GLOWK_TRAIN_PERSTEP", "GLOWK_TRAIN_RECOMPUTE"):
            if mode != "batch":
                monkeypatch.setenv(mode, "1")
                _lib.load().glowk_reload_env()       # (the engine reads its switches when the library loads)
            eng, params = calibrated_engine(cfg, device=0, init_tiles=8)
            if prec == "f16x3":
                eng.set_precision(_lib.PREC_F16X3)
                eng.set_range_policy("error")
            lp, got, flat = engine_grads(eng, params, x, scale)
            flats[mode] = flat.astype(np.float64)
            if mode == "batch":
                lp_ref, ref = oracle_param_grads(x, params, cfg, scale)
            for k, r in ref.items():
                np.testing.assert_allclose(got[k], r, atol=2e-4 * max(np.abs(r).max(), 1e-12), rtol=2e-3, err_msg="%s %s" % (mode, k))
            eng.close()
            if mode != "batch":
                monkeypatch.delenv(mode)
                _lib.load().glowk_reload_env()
    finally:
        monkeypatch.undo()
        _lib.load().glowk_reload_env()
    ref_norm = np.linalg.norm(flats["batch"])
    for mode in ("GLOWK_TRAIN_PERSTEP", "GLOWK_TRAIN_RECOMPUTE"):
        assert np.linalg.norm(flats[mode] - flats["batch"]) < 2e-6 * ref_norm, mode


@pytest.mark.parametrize("opt", ["adamax", "adam"])
def test_optimizer_step_and_image_refresh(opt):
    """Two optimizer steps: the variables follow the Keras formulas on the engine's own gradients, and -- the part that
    exercises the device-side re-packing of the kernel images and the re-folded ActNorm + 1x1 -- log_prob / inverse / the input
    gradient of the updated flow equal the fp64 oracle evaluated on the variables the flow reports, in every arithmetic."""
    cfg = GlowConfig(H=16, W=32, C=1, L=3, K=2, F=128)
    eng, params = calibrated_engine(cfg, device=0, init_tiles=8)
    flow = GlowFlow(eng)
    x = synthetic_mel_tiles(6, cfg, seed=23)
    lr = 2e-3
    state = {k: (np.zeros_like(v, dtype=np.float64), np.zeros_like(v, dtype=np.float64)) for k, v in params.items()}
    cur = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    with pytest.raises(ValueError):
        eng.apply_gradients(torch.zeros(eng.param_vector_size, device="cuda"), optimizer="sgd")
    for t in (1, 2):
        _, got, flat = engine_grads(eng, cur, x, -1.0 / 6.0)
        eng.apply_gradients(dev(flat), optimizer=opt, lr=lr)
        sd = flow.state_dict()
        for k, g in got.items():
            m, v = state[k]
            cur[k], m, v = keras_update(opt, cur[k], g.astype(np.float64), m, v, t, lr)
            state[k] = (m, v)
            np.testing.assert_allclose(sd[k], cur[k], rtol=2e-5, atol=2e-6, err_msg="%s step %d" % (k, t))
        for k in params:
            if k.endswith(("inv1x1/P", "inv1x1/sign_S", "bn1/mean", "bn1/var", "bn2/mean", "bn2/var")):
                np.testing.assert_array_equal(sd[k], np.asarray(params[k], dtype=np.float32), err_msg=k)   # frozen
        assert np.abs(sd["b0/s0/nn/conv2/kernel"] - params["b0/s0/nn/conv2/kernel"]).max() > 1e-4          # it did move
        cur = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}     # continue from the fp32 values the engine holds
    p64 = R.cast_params(flow.state_dict(), np.float64)
    lp_ref, g_ref = RT.log_prob_and_grad(x.astype(np.float64), flow.state_dict(), cfg.as_dict())
    lp32, z = eng.log_prob(dev(x), return_latent=True)
    np.testing.assert_allclose(lp32.cpu().numpy(), lp_ref, rtol=1e-6)
    np.testing.assert_allclose(eng.inverse(z).cpu().numpy(), x, atol=5e-3)
    _, gx = eng.log_prob_grad(dev(x))
    np.testing.assert_allclose(gx.cpu().numpy(), g_ref, atol=2e-4 * np.abs(g_ref).max(), rtol=2e-3)
    # the split kernels' images are re-packed (host) on demand
    eng.set_range_policy("error")
    for prec, tol in ((_lib.PREC_F16X3, 2e-6), (_lib.PREC_F16X2, 5e-5)):
        eng.set_precision(prec)
        np.testing.assert_allclose(eng.log_prob(dev(x)).cpu().numpy(), lp_ref, rtol=tol)
    # and training continues from there (the sweep itself always runs the exact kernels)
    lp_t, _, _ = engine_grads(eng, cur, x, -1.0 / 6.0)
    np.testing.assert_allclose(lp_t, lp_ref, rtol=1e-6)
    assert R.log_prob(x.astype(np.float64), p64, cfg.as_dict()).shape == (6,)


def test_short_training_loop_lowers_the_loss():
    """train_glow.py's loop in miniature: the mean negative log-likelihood of a fixed batch falls under Adamax, set_tensor
    between steps is honoured (the device master copy is re-uploaded), and the result survives a save / restore."""
    cfg = GlowConfig(H=16, W=16, C=1, L=2, K=4, F=128)
    eng, params = calibrated_engine(cfg, device=0, init_tiles=16)
    flow = GlowFlow(eng)
    x = dev(synthetic_mel_tiles(32, cfg, seed=31))
    losses = []
    for it in range(12):
        lp, g = eng.param_grad(x, -1.0 / 32.0)
        losses.append(float(-lp.mean()))
        eng.apply_gradients(g, optimizer="adamax", lr=1e-3)
    assert np.isfinite(losses).all() and losses[-1] < losses[0] - 1.0, losses
    assert all(b < a + 0.5 for a, b in zip(losses, losses[1:])), losses
    lp_after = flow.log_prob(x)
    assert abs(float(-lp_after.mean()) - losses[-1]) < abs(losses[-1] - losses[-2]) + 5.0
    sd = flow.state_dict()
    other = GlowFlow(calibrated_engine(cfg, device=0, init_tiles=16)[0])
    other.load_state_dict(sd)
    assert torch.equal(other.log_prob(x), lp_after)
    # a variable assigned by hand between steps is what the next step differentiates
    v = [v for v in flow.variables if v.name == "b1/s0/nn/conv3/bias"][0]
    v.assign(v.numpy() + 0.25)
    lp2, _ = eng.param_grad(x, -1.0 / 32.0)
    assert torch.equal(lp2, flow.log_prob(x)) and not torch.equal(lp2, lp_after)


@pytest.mark.parametrize("cfg", [GlowConfig(H=16, W=32, C=1, L=3, K=2, F=256), GlowConfig(H=32, W=32, C=1, L=2, K=3, F=512),
                                 GlowConfig(H=32, W=32, C=1, L=4, K=2, F=128)], ids=["L3_F256", "L2_F512", "L4_F128"])
def test_split_training_steps_refresh_the_f16_images_on_the_device(cfg):
    """Training with the handle in f16x3: sweep on the split kernels, Adamax, and the fp16 hi/lo images (BatchNorm folds,
    per-layer power-of-two scales, epilogue constants, range-guard limits) rebuilt ON THE DEVICE after every step.  The rebuilt
    images must be the host packer's, bit for bit: a fresh engine that loads the trained variables (host packing) gives
    bitwise the same log_prob / gradient in f16x3 and f16x2, and both match the fp64 oracle on those variables."""
    eng, params = calibrated_engine(cfg, device=0, init_tiles=16)
    flow = GlowFlow(eng)
    eng.set_precision(_lib.PREC_F16X3)
    eng.set_range_policy("error")
    x = dev(synthetic_mel_tiles(24, cfg, seed=41))
    losses = []
    for it in range(4):
        lp, g = eng.param_grad(x, -1.0 / 24.0)
        losses.append(float(-lp.mean()))
        eng.apply_gradients(g, optimizer="adamax", lr=5e-4)
    assert np.isfinite(losses).all() and losses[-1] != losses[0]
    lp_dev, z_dev = eng.log_prob(x, return_latent=True)          # images refreshed by the device
    lpg_dev, gx_dev = eng.log_prob_grad(x)
    sd = flow.state_dict()
    other, _ = calibrated_engine(cfg, device=0, init_tiles=16)
    oflow = GlowFlow(other)
    oflow.load_state_dict(sd)                                      # images packed by the host
    other.set_precision(_lib.PREC_F16X3)
    other.set_range_policy("error")
    lp_host, z_host = other.log_prob(x, return_latent=True)
    lpg_host, gx_host = other.log_prob_grad(x)
    assert torch.equal(lp_dev, lp_host) and torch.equal(z_dev, z_host) and torch.equal(gx_dev, gx_host) and torch.equal(lpg_dev, lpg_host)
    for e in (eng, other):
        e.set_precision(_lib.PREC_F16X2)
    assert torch.equal(eng.log_prob(x), other.log_prob(x))
    lp_ref = RT.log_prob(torch.from_numpy(x.cpu().numpy().astype(np.float64)), RT.to_torch(sd, torch.float64), cfg.as_dict())[0].numpy()
    np.testing.assert_allclose(lp_dev.cpu().numpy(), lp_ref, rtol=2e-6)
    assert eng.range_status() == (False, 0) and other.range_status() == (False, 0)
    # one more step from the device-refreshed images equals one more step from the host-packed ones
    eng.set_precision(_lib.PREC_F16X3)
    other.set_precision(_lib.PREC_F16X3)
    # (to fp32 rounding, not bit for bit: since round 3 the split sweep carries g_o times a power of two sized on the PREVIOUS
    #  sweep's gradient magnitudes -- dynamic gradient scaling, DESIGN section 8a -- and `eng` has a history that `other` lacks;
    #  a power-of-two scale moves which low bits of the small values fall into fp16's subnormal range)
    _, g1 = eng.param_grad(x, -1.0 / 24.0)
    _, g2 = other.param_grad(x, -1.0 / 24.0)
    assert float((g1 - g2).abs().max()) <= 2e-6 * float(g2.abs().max())
    _, g3 = other.param_grad(x, -1.0 / 24.0)                       # with the same history: bit for bit
    _, g4 = other.param_grad(x, -1.0 / 24.0)
    assert torch.equal(g3, g4)


def test_four_level_training_sweep_runs_entirely_on_the_split_kernels():
    """Round-2 verdict #7: the 32-channel level of 4-level flows (flow_glow.py:228-329; thesis table 3.4 trained an L = 4 flow) used to
    send the WHOLE parameter-gradient sweep to the exact fp32 kernels -- its K = 288 backward network had no split instance.  Now
    its saving forward and backward launches (with hidden stores) run the half-wave form of the 16x16x32 family: every gradient
    tensor against the fp64 autograd of the oracle in f16x3, and not one launch of k_net_f32 (glowk_kernel_families)."""
    cfg = GlowConfig(H=32, W=32, C=1, L=4, K=2, F=512)
    eng, params = calibrated_engine(cfg, device=0, init_tiles=8)
    x = synthetic_mel_tiles(5, cfg, seed=23)
    scale = -1.0 / 32.0
    lp_ref, ref = oracle_param_grads(x, params, cfg, scale)
    eng.set_precision(_lib.PREC_F16X3)
    eng.set_range_policy("error")
    before = eng.kernel_families()
    lp, got, flat = engine_grads(eng, params, x, scale)
    fam = {k: v - before[k] for k, v in eng.kernel_families().items()}
    assert fam["f32"] == 0 and sum(fam[k] for k in PRIMARY_FAMILIES) == 4 * 2 * 2 and fam["h3s_half"] >= 4, fam
    np.testing.assert_allclose(lp, lp_ref, rtol=1e-6)
    worst = 0.0
    for k, r in ref.items():
        denom = max(np.abs(r).max(), 1e-12)
        worst = max(worst, float(np.abs(got[k] - r).max() / denom))
        np.testing.assert_allclose(got[k], r, atol=2e-4 * denom, rtol=2e-3, err_msg=k)
    print("L4 f16x3 sweep: worst |g - fp64| / max|g| over all tensors %.1e; launches by family %s" % (worst, fam))
    # a few optimizer steps: the loss goes down, nothing falls back
    flow = GlowFlow(eng)
    xd = dev(x)
    losses = [float(flow.train_step(xd, lr=2e-4)) for _ in range(6)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert eng.kernel_families()["f32"] == before["f32"] and eng.range_status() == (False, 0)


def test_parameter_gradients_of_the_full_depth_flow():
    """Config B at its real depth (L = 3, K = 32, n_filters = 512: 96 flow steps, 31.9 M parameters) -- the bench's training workload --
    against the fp64 autograd of the oracle, in both arithmetics, on two tiles (the oracle's reverse mode is ~150 GFLOP in fp64).
    Through 96 coupling steps and ~200 ReLU layers fp32 rounding is amplified by the flow itself (and isolated ReLU decisions fall
    differently): the yardstick is the SAME oracle evaluated in float32 -- what a plain fp32 implementation of the
    reference delivers -- and the engine has to be as close to fp64 as that, in both arithmetics."""
    cfg = GlowConfig(H=64, W=64, C=1, L=3, K=32, F=512)
    eng, params = calibrated_engine(cfg, device=0, init_tiles=16)
    x = synthetic_mel_tiles(2, cfg, seed=23)
    scale = -1.0 / 32.0
    lp_ref, ref = oracle_param_grads(x, params, cfg, scale)

    def errors(got):
        errs = np.array([float(np.abs(got[k] - r).max() / max(np.abs(r).max(), 1e-12)) for k, r in ref.items()])
        num = np.sqrt(sum(float(((got[k] - r) ** 2).sum()) for k, r in ref.items()))
        den = np.sqrt(sum(float((r ** 2).sum()) for r in ref.values()))
        return errs, num / den

    # the yardstick: the oracle's own reverse mode in float32
    p32 = {k: torch.tensor(np.asarray(v), dtype=torch.float32, requires_grad=k.split("/", 2)[-1] in TRAINABLE or k in TRAINABLE)
           for k, v in params.items()}
    lp32, _ = RT.log_prob(torch.from_numpy(x.astype(np.float32)), p32, cfg.as_dict())
    names = [k for k, v in p32.items() if v.requires_grad]
    g32 = torch.autograd.grad(scale * lp32.sum(), [p32[k] for k in names], allow_unused=True)
    yard, yard_vec = errors({k: (g.double().numpy() if g is not None else np.zeros_like(ref[k])) for k, g in zip(names, g32)})
    print("K = 32, float32 oracle: |g - fp64| / max|g| median %.1e, 95th percentile %.1e, worst %.1e; whole vector %.1e"
          % (np.median(yard), np.percentile(yard, 95), yard.max(), yard_vec))
    for prec in ("f32", "f16x3"):
        eng.set_precision({"f32": _lib.PREC_F32, "f16x3": _lib.PREC_F16X3}[prec])
        eng.set_range_policy("error")
        lp, got, flat = engine_grads(eng, params, x, scale)
        np.testing.assert_allclose(lp, lp_ref, rtol=2e-6)
        errs, vec = errors(got)
        print("K = 32, %s: %d tensors, |g - fp64| / max|g| median %.1e, 95th percentile %.1e, worst %.1e; whole vector %.1e; fallbacks %s"
              % (prec, len(errs), np.median(errs), np.percentile(errs, 95), errs.max(), vec, eng.range_status()))
        assert np.isfinite(flat).all() and eng.range_status() == (False, 0)
        assert np.median(errs) < 3 * np.median(yard) + 1e-6 and np.percentile(errs, 95) < 3 * np.percentile(yard, 95) + 1e-5
        assert vec < 3 * yard_vec + 1e-6 and errs.max() < max(3 * yard.max(), 2e-2)


@pytest.mark.parametrize("n", [16, 128])
def test_training_sweep_in_the_co_resident_form(n, monkeypatch):
    """Level 0 of the split training sweep runs k_net_h3c<..., MODE | 8> (four-wave workgroups two to a CU, adjacent pixels per lane,
    hidden tensors stored as 8-byte pairs) where every workgroup is full: one pass per workgroup on small grids (n = 16; below that the half-wave form takes the level), both passes
    in a workgroup on grids that fill the chip (n = 128).  Against the 32x32x16 family (GLOWK_CO_TRAIN_OFF: same split arithmetic,
    other summation order) and against itself, bit for bit."""
    cfg = GlowConfig(H=64, W=64, C=1, L=3, K=2, F=512)
    eng, params = calibrated_engine(cfg, device=0, init_tiles=8)
    eng.set_precision(_lib.PREC_F16X3)
    eng.set_range_policy("error")
    x = dev(synthetic_mel_tiles(n, cfg, seed=23))
    lib = _lib.load()
    try:
        monkeypatch.setenv("GLOWK_CO_TRAIN_OFF", "1")
        lib.glowk_reload_env()
        before = eng.kernel_families()
        lp0, g0 = eng.param_grad(x, -1.0 / n)
        mid = eng.kernel_families()
        assert mid["co_resident"] == before["co_resident"]
        monkeypatch.delenv("GLOWK_CO_TRAIN_OFF")
        lib.glowk_reload_env()
        lp1, g1 = eng.param_grad(x, -1.0 / n)
        after = eng.kernel_families()
        assert after["co_resident"] - mid["co_resident"] == 2 * cfg.K        # level 0: K saving forward + K backward launches
        lp2, g2 = eng.param_grad(x, -1.0 / n)
    finally:
        monkeypatch.undo()
        lib.glowk_reload_env()
    assert torch.equal(g1, g2) and torch.equal(lp1, lp2)
    rel = ((g1.double() - g0.double()).norm() / g0.double().norm()).item()
    print("n = %d: co-resident training sweep vs the 32x32x16 family: relative l2 difference of the gradient vector %.1e" % (n, rel))
    assert rel < 2e-4
    np.testing.assert_allclose(lp1.cpu().numpy(), lp0.cpu().numpy(), rtol=2e-6)
    assert eng.range_status() == (False, 0)
    eng.close()


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_training_steps_without_a_host_join_equal_joined_ones(prec, monkeypatch):
    """glowk_param_grad does not join the caller's stream: the host's ActNorm / 1x1 chain rule runs beside the last level's
    weight-gradient GEMMs (sums down / results up on a side stream the caller's stream waits for by event), and
    glowk_apply_gradients folds ActNorm + 1x1 on the host while the device refreshes the images.  Eight back-to-back steps with no
    synchronisation in between against the same steps with the host joining the stream inside every sweep (GLOWK_PG_JOIN=1) and a
    device synchronisation after every call: parameters, losses and the final log_prob bit for bit."""
    cfg = GlowConfig(H=32, W=32, C=1, L=3, K=3, F=256)
    x = dev(synthetic_mel_tiles(24, cfg, seed=41))
    out = {}
    try:
        for joined in (False, True):
            if joined:
                monkeypatch.setenv("GLOWK_PG_JOIN", "1")
            else:
                monkeypatch.delenv("GLOWK_PG_JOIN", raising=False)
            _lib.load().glowk_reload_env()           # (the engine reads its switches when the library loads)
            eng, _ = calibrated_engine(cfg, device=0, init_tiles=16)
            if prec == "f16x3":
                eng.set_precision(_lib.PREC_F16X3)
            g = torch.zeros(eng.param_vector_size, device="cuda")
            lps = []
            for it in range(8):
                lp, _ = eng.param_grad(x, -1.0 / 24.0, g)
                if joined:
                    torch.cuda.synchronize()
                lps.append(lp)
                eng.apply_gradients(g, optimizer="adamax", lr=1e-3)
                if joined:
                    torch.cuda.synchronize()
            final = eng.log_prob(x)
            torch.cuda.synchronize()
            out[joined] = (torch.stack(lps).cpu(), final.cpu(), {k: np.asarray(v) for k, v in GlowFlow(eng).state_dict().items()}, g.cpu())
            eng.close()
    finally:
        monkeypatch.undo()
        _lib.load().glowk_reload_env()
    a, b = out[False], out[True]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k
    assert float(-a[0][-1].mean()) < float(-a[0][0].mean())
