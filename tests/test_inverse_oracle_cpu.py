"""Conditioning of the inputs of tests/test_gpu_inverse_oracle.py, checked without a GPU: the bars of that module are multiples of
each case's yardstick y = max |float32 restatement - fp64 restatement| of the latent -> data direction, so a case is only worth
keeping if y is small and the direction is well conditioned at its inputs.  For every case of tests/inverse_cases.py, on the tiles
the GPU test compares (the subset for 256 compute units), with ActNorm calibrated by the oracle's own data-dependent init:
  * y <= 1e-4 dB for inverse(z) and for sample_from_eps(eps)   (so that no bar of the GPU module exceeds 16 * 1e-4 = 1.6e-3 dB);
  * the fp64 restatement returns x from its own latent to <= 1e-5 dB.
A case that fails either is replaced, not kept with a wider bar.  Also here: the restated launch rule reaches every coupling launch
form of the direction on 256 compute units, and the tile subsets are what the rule says."""
import numpy as np
import pytest

from audiosourcesep_amd.synthetic import synthetic_mel_tiles
from oracle import glowref as R
from tests import inverse_cases as IC

YARDSTICK_CAP = 1e-4      # dB
ROUND_TRIP_CAP = 1e-5     # dB
CUS = 256                 # the MI355X; the GPU module asks the device


@pytest.mark.parametrize("name", list(IC.CASES))
def test_case_is_well_conditioned(name):
    case = IC.CASES[name]
    cfg, d = case.cfg, case.cfg.as_dict()
    params = IC.cpu_calibrated_params(case)
    idx = IC.tile_subset(case, CUS)
    x = synthetic_mel_tiles(case.n, cfg, seed=case.seed)[idx]
    p64 = R.cast_params(params, np.float64)
    z64, _ = R.bijector_forward(x.astype(np.float64), p64, d)
    back = float(np.abs(R.bijector_inverse(z64, p64, d) - x).max())
    ref = IC.references(params, cfg, z64.astype(np.float32), IC.latent_noise(case)[idx])
    print("%-24s tiles %s: yardstick inverse %.1e dB, sample %.1e dB; fp64 round trip %.1e dB" % (
        name, idx, ref["y_inverse"], ref["y_sample"], back))
    assert np.isfinite(ref["inverse"]).all() and np.isfinite(ref["sample"]).all()
    assert 0 < ref["y_inverse"] <= YARDSTICK_CAP and 0 < ref["y_sample"] <= YARDSTICK_CAP
    assert back <= ROUND_TRIP_CAP
    # the samples are spectrogram-like: inside the dB range the preprocessing maps from, not saturated garbage
    assert np.abs(ref["sample"]).max() < 1e3


def test_table_reaches_every_launch_form_on_256_compute_units():
    seen = set()
    for case in IC.CASES.values():
        for arith in IC.ARITHMETICS:
            seen |= IC.forms_of(case, arith, CUS)
        if case.co_off:
            seen |= IC.forms_of(case, "f16x3", CUS, co_off=True)
    assert seen == set(IC.ALL_FORMS), sorted(set(IC.ALL_FORMS) ^ seen)


def test_launch_rule_restatement_on_known_cases():
    """The rows of the issue's table, as the rule answers them for 256 compute units."""
    C, f = IC.CASES, lambda name, arith, **kw: IC.forms_of(IC.CASES[name], arith, CUS, **kw)
    assert f("16x16_L2_n3", "f32") == {"k_couple_flat<.,4>", "k_couple<.,true>@256"}
    assert "k_couple_flat<.,16>" in f("32x32_L3_n5", "f32")
    assert f("24x24_L2_F256_n7", "f16x3") == {"k_couple<.,true>@512", "k_couple<.,true>@256"}       # width 12: never fused
    assert f("40x40_L2_n3", "f32") == {"k_couple<.,true>@1024", "k_couple<.,true>@512"}
    assert f("8x8_L2_n515", "f16x2") == {"k_couple<.,false>"}
    assert f("24x24_L2_F384_n515", "f32") == {"k_couple<.,false>"}
    assert f("16x16_C2_L3_n7", "f16x3") == f("16x16_C2_L3_n7", "f32")                               # c = 8 at level 0: never fused
    assert f("64x64_L3_F512_n160", "f32") == {"k_couple_flat<.,4>", "k_couple_flat<.,16>"}
    assert f("64x64_L3_F512_n160", "f16x3") == {"fused_co_resident", "k_couple_edge", "k_couple_flat<.,4>", "k_couple_flat<.,16>"}
    assert f("96x64_L3_F512_n30", "f16x2") >= {"fused_co_resident", "k_couple_edge"}
    assert f("32x32_L2_K3_F512_n300", "f16x3", co_off=True) == {"fused_256", "k_couple_flat<.,16>"}
    assert f("16x16_L2_n1031", "f16x3", co_off=True) == {"fused_256", "k_couple<.,false>"}
    assert f("16x16_L2_n1031", "f16x3") == {"fused_co_resident", "k_couple<.,false>"}
    # the subsets: first and last tile, and the tiles at the first and the last level-0 workgroup boundary
    assert IC.tile_subset(C["16x16_L2_n1031"], CUS) == [0, 3, 4, 1027, 1028, 1030]      # 256-pixel workgroups, 64 pixels a tile
    assert IC.tile_subset(C["64x64_L3_F512_n160"], CUS) == [0, 159]                     # boundaries inside the tiles
    assert IC.tile_subset(C["8x8_L2_n515"], CUS) == [0, 1, 513, 514]                    # a workgroup per tile
    assert IC.tile_subset(C["16x16_L2_n3"], CUS) == [0, 1, 2]
    assert all(len(IC.tile_subset(c, CUS)) <= 6 for c in C.values())
