"""The operand prefetch across op boundaries in the double-buffered level-0 kernel (glowk_co.h: co_Xdb / co_Ydb -- the next block's conv1
operands are read under the end of Y, the block's barrier sits in front of the activation, Y's first A group is read behind it, and the
units' DMA pieces all leave in the first half of Y) against references that share none of that schedule:

- the eight-wave form k_net_h3s (GLOWK_CO_OFF=1), which has no ring code in common.  On 16 x 16 tiles a 128- or 256-pixel workgroup of
  the 4-channel level holds whole 8 x 8 images, so neither form leaves edge rows to k_couple_edge, the log-det partials are per 32-pixel
  wave in both, and log_prob and latent are bit for bit equal;
- the tile itself: a batch that repeats one tile gives every entry the result of entry 0, whatever its workgroup's position, partner and
  timing -- a K slot or a pair read too early shows as entries that differ;
- the first of 200 calls, at the shortest ring (F = 128: two hidden blocks per pass, so the prefetch across the wrap of the K slots and
  the hand-over to conv3 follow each other directly).

Every case launches more than 2 x CUs workgroups of 128 pixels at the 4-channel level, so workgroups start beside a running partner;
the odd tile counts leave the last workgroup two idle waves, which must still reach the moved barrier."""
import functools
import os

import pytest
import torch

from audiosourcesep_amd import _lib
from audiosourcesep_amd.config import GlowConfig
from audiosourcesep_amd.synthetic import synthetic_mel_tiles, calibrated_engine

pytestmark = pytest.mark.gpu

# F -> tiles: NG = F / 128 MFMA groups per half of Y.  16 x 16 tiles are 64 pixels at the 4-channel level: two tiles per workgroup.
# F = 512 and F = 128 ragged (odd count: the last workgroup has two idle waves), F = 256 ragged too (NG = 2: the first shape where
# "the last group" and "the first half" of Y differ by one group), F = 384 whole.
TILES = {128: 1031, 256: 1033, 384: 1040, 512: 1031}
PREC = {"f16x3": _lib.PREC_F16X3, "f16x2": _lib.PREC_F16X2}


def _setenv(name, on):
    """The engine reads its diagnostic switches at load time: change one and have them read again (glowk_reload_env)."""
    if on:
        os.environ[name] = "1"
    else:
        os.environ.pop(name, None)
    _lib.load().glowk_reload_env()


@functools.lru_cache(maxsize=None)
def _engine(F):
    cfg = GlowConfig(H=16, W=16, C=1, L=2, K=2, F=F)
    eng, _ = calibrated_engine(cfg, device=0, init_tiles=32)
    eng.set_range_policy("error")
    return cfg, eng


def _fills_the_grid(cfg, n):
    # 128-pixel workgroups of a 4-channel-level launch (the squeeze halves H and W): more than two per CU
    wgs = -(-(n * (cfg.H // 2) * (cfg.W // 2)) // 128)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert wgs > 2 * cus, (wgs, cus)


def _families(eng, before):
    return {k: v - before[k] for k, v in eng.kernel_families().items()}


@pytest.mark.parametrize("precision", list(PREC))
@pytest.mark.parametrize("F", list(TILES))
def test_prefetching_ring_equals_the_eight_wave_form(F, precision):
    cfg, eng = _engine(F)
    n = TILES[F]
    _fills_the_grid(cfg, n)
    eng.set_precision(PREC[precision])
    x = torch.from_numpy(synthetic_mel_tiles(n, cfg, seed=11)).cuda()
    out = {}
    try:
        for co in (False, True):
            _setenv("GLOWK_CO_OFF", not co)
            before = eng.kernel_families()
            lp, z = eng.log_prob(x, return_latent=True)
            torch.cuda.synchronize()
            out[co] = (lp.clone(), z.clone(), _families(eng, before))
    finally:
        _setenv("GLOWK_CO_OFF", False)
    fam = out[True][2]
    assert fam["fused"] == cfg.K and fam["co_resident"] >= cfg.K, fam       # every step of the 4-channel level ran fused and co-resident
    assert out[False][2]["fused"] == cfg.K and out[False][2]["co_resident"] == 0, out[False][2]
    print("F=%d %s: max |d log_prob| %.3e, max |d latent| %.3e" % (F, precision, float((out[True][0] - out[False][0]).abs().max()),
                                                                  float((out[True][1] - out[False][1]).abs().max())))
    assert torch.isfinite(out[True][0]).all()
    assert torch.equal(out[True][0], out[False][0]), (F, precision, "log_prob")
    assert torch.equal(out[True][1], out[False][1]), (F, precision, "latent")
    assert eng.range_status() == (False, 0)


@pytest.mark.parametrize("F", [512, 128])
def test_results_do_not_depend_on_the_partner_workgroup(F):
    cfg, eng = _engine(F)
    n = TILES[F]
    _fills_the_grid(cfg, n)
    eng.set_precision(_lib.PREC_F16X3)
    one = torch.from_numpy(synthetic_mel_tiles(1, cfg, seed=12))
    x = one.repeat(n, *([1] * (one.dim() - 1))).contiguous().cuda()
    before = eng.kernel_families()
    lp, z = eng.log_prob(x, return_latent=True)
    torch.cuda.synchronize()
    fam = _families(eng, before)
    assert fam["fused"] == cfg.K and fam["co_resident"] >= cfg.K, fam
    z = z.reshape(n, -1)
    print("F=%d: entries that differ from entry 0: log_prob %d, latent rows %d" % (F, int((lp != lp[0]).sum()), int((z != z[0]).any(dim=1).sum())))
    assert torch.isfinite(lp).all()
    assert torch.equal(lp, lp[0].expand_as(lp))
    assert torch.equal(z, z[0].expand_as(z))
    assert eng.range_status() == (False, 0)


def test_prefetching_ring_repeats_bit_for_bit_at_the_shortest_ring():
    """200 log_prob calls over the same resident batch at F = 128 (NF = 4): every result is bit for bit the first."""
    cfg, eng = _engine(128)
    n = TILES[128]
    _fills_the_grid(cfg, n)
    eng.set_precision(_lib.PREC_F16X3)
    x = torch.from_numpy(synthetic_mel_tiles(n, cfg, seed=13)).cuda()
    before = eng.kernel_families()
    first = eng.log_prob(x).clone()
    fam = _families(eng, before)
    assert fam["fused"] == cfg.K and fam["co_resident"] >= cfg.K, fam
    differ = torch.zeros((), dtype=torch.int64, device=x.device)
    for _ in range(199):
        differ += (eng.log_prob(x) != first).sum()
    assert int(differ) == 0
    assert torch.isfinite(first).all()
    assert eng.range_status() == (False, 0)
