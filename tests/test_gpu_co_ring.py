"""The double-buffered weight ring of the fused co-resident network kernel (glowk_co.h, RingC::DB: four unit slots read as two pairs,
one barrier per hidden block, P in slots that are dead by then) against the three-slot ring of the same build (GLOWK_CO_RING3=1, the
instance k_net_h3c<..., RING3 = true>).  The per-wave MFMA order, the epilogues and fused_couple are the same, so every result is bit for
bit equal; a difference is a race in the ring (a slot refilled under a reader, a slot read before its pieces landed, P written into a
slot still in use).  Every case launches more than 2 x CUs workgroups of 128 pixels at the 4-channel level: the fused co-resident form
is taken, and workgroups start beside a partner that is already running."""
import os

import pytest
import torch

from audiosourcesep_amd import _lib
from audiosourcesep_amd.config import GlowConfig
from audiosourcesep_amd.synthetic import synthetic_mel_tiles, calibrated_engine

pytestmark = pytest.mark.gpu

CASES = {
    # name: (cfg, tiles)
    "64x64_F512_edge_rows_8_wgs_per_tile": (GlowConfig(H=64, W=64, C=1, L=3, K=2, F=512), 160),
    "32x32_F512_ragged": (GlowConfig(H=32, W=32, C=1, L=2, K=3, F=512), 555),
    "64x32_F384_NF12": (GlowConfig(H=64, W=32, C=1, L=3, K=2, F=384), 301),
    # the shortest ring, two hidden blocks per pass: block 0 / 1 start-up, the hand-over to conv3 and the wrap of the conv1 slots follow
    # each other directly; two tiles per workgroup, ragged last workgroup
    "16x16_F128_NF4_two_tiles_per_wg_ragged": (GlowConfig(H=16, W=16, C=1, L=2, K=2, F=128), 1031),
}
PREC = {"f16x3": _lib.PREC_F16X3, "f16x2": _lib.PREC_F16X2}


def _setenv(name, on):
    """The engine reads its diagnostic switches at load time: change one and have them read again (glowk_reload_env)."""
    if on:
        os.environ[name] = "1"
    else:
        os.environ.pop(name, None)
    _lib.load().glowk_reload_env()


def _engine(name, precision):
    cfg, n = CASES[name]
    eng, _ = calibrated_engine(cfg, device=0, init_tiles=32)
    eng.set_precision(PREC[precision])
    eng.set_range_policy("error")
    x = torch.from_numpy(synthetic_mel_tiles(n, cfg, seed=9)).cuda()
    # 128-pixel workgroups of a 4-channel-level launch (the squeeze halves H and W): more than two per CU
    wgs = -(-(n * (cfg.H // 2) * (cfg.W // 2)) // 128)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert wgs > 2 * cus, (wgs, cus)
    return cfg, eng, x


def _families(eng, before):
    return {k: v - before[k] for k, v in eng.kernel_families().items()}


@pytest.mark.parametrize("precision", list(PREC))
@pytest.mark.parametrize("name", list(CASES))
def test_double_buffered_ring_equals_three_slot_ring(name, precision):
    cfg, eng, x = _engine(name, precision)
    out = {}
    try:
        for ring3 in (True, False):
            _setenv("GLOWK_CO_RING3", ring3)
            before = eng.kernel_families()
            lp, z = eng.log_prob(x, return_latent=True)
            xr = eng.inverse(z)
            torch.cuda.synchronize()
            fam = _families(eng, before)
            # every step of the 4-channel level, forward and inverse, ran fused and co-resident (the 8-channel level may add
            # co-resident launches of its own; it is never fused)
            assert fam["fused"] == 2 * cfg.K and fam["co_resident"] >= 2 * cfg.K, (ring3, fam)
            out[ring3] = (lp, z, xr)
    finally:
        _setenv("GLOWK_CO_RING3", False)
    assert torch.isfinite(out[False][0]).all()
    for i, what in enumerate(("log_prob", "latent", "inverse")):
        assert torch.equal(out[False][i], out[True][i]), (name, precision, what)
    assert eng.range_status() == (False, 0)


def test_double_buffered_ring_repeats_bit_for_bit():
    """200 log_prob calls over the same resident batch: a race in the ring shows as a result that differs from the first."""
    cfg, eng, x = _engine("64x64_F512_edge_rows_8_wgs_per_tile", "f16x3")
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
