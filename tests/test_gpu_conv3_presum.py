"""conv3's horizontal taps added in registers at the 8- and 16-channel levels (glowk_kernels.h: c3_presum_store): the
forward 16x16x32 kernels write P as [3 c][Q] -- one row per (dy, channel) -- where the level's width is a power of two in [4, 16], and
per-tap P through the permuted rows everywhere else.  Checked against the exact fp32 kernels of the same build (which still write
per-tap P: every border pixel goes through an independent path), against the same build with GLOWK_NO_PRESUM=1, against the fp64
oracle, across batch sizes (every launch form of a level shape writes the same layout and adds in the same order) and for
repeatability."""
import os

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib
from audiosourcesep_amd.config import GlowConfig
from audiosourcesep_amd.synthetic import synthetic_mel_tiles, calibrated_engine
from oracle import glowref as R

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _engine(H, W, F, K):
    key = (H, W, F, K)
    if key not in _ENGINES:
        cfg = GlowConfig(H=H, W=W, C=1, L=3, K=K, F=F)
        eng, params = calibrated_engine(cfg, device=0, init_tiles=32)
        eng.set_range_policy("error")
        _ENGINES[key] = (cfg, eng, params)
    cfg, eng, params = _ENGINES[key]
    eng.set_precision(_lib.PREC_F16X3)
    return cfg, eng, params


def _setenv(name, on):
    """The engine reads its diagnostic switches at load time: change one and have them read again (glowk_reload_env)."""
    if on:
        os.environ[name] = "1"
    else:
        os.environ.pop(name, None)
    _lib.load().glowk_reload_env()


# (H, W, tiles, F): levels 1 / 2 are (H/4, W/4, 8) / (H/8, W/8, 16)
NET_CASES = [
    (64, 64, 3, 128),      # 16 x 16 x 8 (a half = one image row), 8 x 8 x 16 (two rows); small-grid forms, a ragged last workgroup
    (64, 64, 160, 128),    # ... the co-resident form at level 1
    (32, 32, 3, 128),      # 8 x 8 x 8, 4 x 4 x 16 (four rows per half)
    (32, 128, 3, 128),     # level 1: w = 32, per-tap P through the permuted rows; level 2: 4 x 16 x 16
    (32, 96, 3, 128),      # w = 24 and 12: both per-tap
    (96, 64, 3, 128),      # level 1: 24 x 16; level 2: 12 x 8
    (64, 64, 3, 512),
    (64, 64, 160, 512),    # the headline's instances
]


@pytest.mark.parametrize("H,W,n,F", NET_CASES)
def test_network_outputs_against_the_exact_fp32_kernels(H, W, n, F):
    cfg, eng, _ = _engine(H, W, F, 1)
    for level in (1, 2):
        h, w, c = cfg.level_shapes()[level]
        xb = torch.from_numpy(np.random.default_rng(31 + level).standard_normal((n, h, w, c // 2)).astype(np.float32)).cuda()
        before = eng.kernel_families()
        ls, t = eng.coupling_net(level, 0, xb)
        torch.cuda.synchronize()
        fam = {k: v - before[k] for k, v in eng.kernel_families().items()}
        assert fam["f32"] == 0 and fam["h3s_16x16x32"] + fam["h3s_half"] == 1, fam      # the split call ran a 16x16x32 kernel
        eng.set_precision(_lib.PREC_F32)
        try:
            ls32, t32 = eng.coupling_net(level, 0, xb)
        finally:
            eng.set_precision(_lib.PREC_F16X3)
        print("%dx%d level %d (%dx%dx%d) %d tiles F=%d: max |d log_s| %.2e, max |d t| %.2e" %
              (H, W, level, h, w, c, n, F, float((ls - ls32).abs().max()), float((t - t32).abs().max())), fam)
        np.testing.assert_allclose(ls.cpu().numpy(), ls32.cpu().numpy(), atol=2e-5, rtol=1e-4)
        np.testing.assert_allclose(t.cpu().numpy(), t32.cpu().numpy(), atol=2e-5, rtol=1e-4)
    assert eng.range_status() == (False, 0)


def _run(eng, x, presum):
    _setenv("GLOWK_NO_PRESUM", not presum)
    try:
        lp, z = eng.log_prob(x, return_latent=True)
        xr = eng.inverse(z)
        torch.cuda.synchronize()
        return lp, z, xr
    finally:
        _setenv("GLOWK_NO_PRESUM", False)


@pytest.fixture(scope="module")
def batch160():
    """160 tiles of 64 x 64 at K = 2, F = 128, and their log_prob / latent / round trip with the pre-sum: shared, never modified."""
    cfg, eng, params = _engine(64, 64, 128, 2)
    x = torch.from_numpy(synthetic_mel_tiles(160, cfg, seed=17)).cuda()
    lp, z, xr = _run(eng, x, True)
    return cfg, eng, params, x, lp, z, xr


@pytest.mark.parametrize("n", [3, 160])
def test_presum_against_per_tap_layout_of_the_same_build(batch160, n):
    cfg, eng, params, x160, lp160, z160, xr160 = batch160
    x = x160[:n].contiguous()
    lp_a, z_a, xr_a = (lp160, z160, xr160) if n == 160 else _run(eng, x, True)
    lp_b, z_b, xr_b = _run(eng, x, False)
    rel = float(((lp_a - lp_b).abs() / lp_b.abs()).max())
    dz = float((z_a - z_b).abs().max())
    print("%d tiles, pre-sum vs per-tap: log_prob rel %.1e, |dz| %.1e; round trip %.1e / %.1e dB" %
          (n, rel, dz, float((xr_a - x).abs().max()), float((xr_b - x).abs().max())))
    assert torch.isfinite(lp_a).all() and torch.isfinite(lp_b).all()
    assert rel < 2e-6 and dz < 2e-4
    assert float((xr_a - x).abs().max()) < 2e-2 and float((xr_b - x).abs().max()) < 2e-2
    ref = R.log_prob(x[:2].cpu().numpy().astype(np.float64), R.cast_params(params, np.float64), cfg.as_dict())
    np.testing.assert_allclose(lp_a[:2].cpu().numpy(), ref, rtol=2e-6)
    np.testing.assert_allclose(lp_b[:2].cpu().numpy(), ref, rtol=2e-6)
    assert eng.range_status() == (False, 0)


def test_a_tile_alone_against_the_tile_inside_the_batch(batch160):
    cfg, eng, _, x160, lp160, _, _ = batch160
    for i in (0, 77, 159):
        lp1 = eng.log_prob(x160[i:i + 1].contiguous())
        rel = float(((lp1 - lp160[i:i + 1]).abs() / lp160[i:i + 1].abs()).max())
        print("tile %d alone vs in the batch of 160: log_prob rel %.1e" % (i, rel))
        assert rel < 2e-6


@pytest.mark.parametrize("n", [160, 3])
def test_log_prob_repeats_bit_for_bit(batch160, n):
    cfg, eng, _, x160, lp160, _, _ = batch160
    x = x160[:n].contiguous()
    first = lp160 if n == 160 else eng.log_prob(x)
    same = torch.ones((), dtype=torch.bool, device=x.device)
    for _ in range(200):
        same &= (eng.log_prob(x) == first).all()
    assert bool(same)
