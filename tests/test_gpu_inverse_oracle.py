"""The latent -> data direction (glowk_inverse, glowk_sample: k_unsplit, the inverse branches of k_couple / k_couple_flat /
k_couple_edge and of the fused kernels, the folded inverse affine applied after the coupling, k_out's inverse preprocessing,
k_prior_sample) against the fp64 oracle DIRECTLY, in every arithmetic and through every launch form of the coupling, with a bar
that comes from the reference and not from the kernels.  Elsewhere this direction is only held to a round trip or to another launch
form of itself, at bars of 2e-3 ... 5e-2 dB.

Per case (tests/inverse_cases.py): z = forward(x) once in exact fp32 and a seeded eps; inverse(z) and sample_from_eps(eps) of the
WHOLE batch (that selects the launch form) in f32, f16x3 and f16x2; the oracle on a subset of at most six tiles -- the first, the
last, and those at the first and the last workgroup boundary of the level-0 grid of the case's split-arithmetic form (the form
is named in inverse_cases.tile_subset; the boundaries of a case's other runs are covered by the first and last tile) -- from the
same float32 z / eps.
Yardstick y: max |float32 restatement - fp64 restatement| on those tiles (tests/test_inverse_oracle_cpu.py holds it to 1e-4 dB).
Bars: f32 <= 8 y (one decimal order for what the restatement does not model: MFMA summation order over up to 9 * 512 terms,
ActNorm + 1x1 folded into one matrix); f16x3 <= 16 y (the factor 2 the suite grants that mode over exact fp32 on log_prob); f16x2
rounds activations to fp16 by design and is held to the 0.3 dB its round trip is held to elsewhere -- it is here to catch a gross
error in the two-term launches.  The launch forms are asserted from the engine's counters where it has one (fused steps,
co-resident launches) and from the restated launch rule otherwise; one test checks that the table reaches every form on the device
it runs on.

Measured on an MI355X (256 compute units), max |gpu - fp64| in dB, inverse / sample:
  case                    yardstick y      f32              f16x3            f16x2          
  16x16_L2_n3             2.1e-5 / 3.5e-5  9.0e-6 / 9.0e-6  1.2e-5 / 1.1e-5  6.3e-4 / 6.7e-4
  16x16_L3_n4             3.0e-5 / 3.3e-5  9.7e-6 / 1.1e-5  1.0e-5 / 1.1e-5  7.2e-4 / 5.8e-4
  32x32_L3_n5             2.1e-5 / 2.2e-5  1.3e-5 / 1.3e-5  1.0e-5 / 1.1e-5  8.2e-4 / 7.1e-4
  24x24_L2_F256_n7        3.6e-5 / 3.8e-5  1.1e-5 / 1.3e-5  1.1e-5 / 1.3e-5  1.6e-3 / 1.1e-3
  40x40_L2_n3             2.0e-5 / 2.2e-5  1.2e-5 / 1.3e-5  1.2e-5 / 1.3e-5  7.4e-4 / 6.1e-4
  8x8_L2_n515             1.4e-5 / 1.5e-5  9.3e-6 / 1.0e-5  9.6e-6 / 1.0e-5  2.3e-4 / 2.8e-4
  24x24_L2_F384_n515      3.5e-5 / 4.0e-5  1.2e-5 / 1.4e-5  2.0e-5 / 1.6e-5  1.8e-3 / 2.4e-3
  32x16_L4_n3             2.3e-5 / 2.4e-5  1.4e-5 / 1.8e-5  1.4e-5 / 1.8e-5  5.6e-4 / 7.1e-4
  16x16_C2_L3_n7          3.8e-5 / 2.7e-5  1.8e-5 / 2.3e-5  1.8e-5 / 2.3e-5  1.1e-3 / 6.2e-4
  8x16_C4_L2_n7           3.1e-5 / 2.8e-5  1.4e-5 / 1.6e-5  1.4e-5 / 1.6e-5  1.4e-3 / 6.1e-4
  8x8_logit_notop_n3      1.6e-5 / 1.6e-5  1.6e-5 / 1.4e-5  1.6e-5 / 1.4e-5  2.0e-4 / 4.3e-4
  16x16_L2_K8_n4          4.1e-5 / 4.4e-5  2.1e-5 / 2.1e-5  1.7e-5 / 1.8e-5  1.1e-3 / 8.4e-4
  32x32_L2_K3_F512_n300   2.6e-5 / 2.7e-5  1.5e-5 / 1.4e-5  1.8e-5 / 1.5e-5  3.2e-3 / 2.9e-3
    with GLOWK_CO_OFF                                       1.4e-5 / 1.5e-5  3.2e-3 / 2.9e-3
  16x16_L2_n1031          2.4e-5 / 2.7e-5  8.7e-6 / 1.1e-5  8.3e-6 / 1.1e-5  4.1e-4 / 5.6e-4
    with GLOWK_CO_OFF                                       8.3e-6 / 1.1e-5  4.1e-4 / 5.6e-4
  64x64_L3_F512_n160      4.3e-5 / 4.9e-5  2.4e-5 / 2.2e-5  2.3e-5 / 2.3e-5  6.1e-3 / 5.5e-3
  96x64_L3_F512_n30       4.4e-5 / 5.5e-5  2.1e-5 / 2.9e-5  1.8e-5 / 2.9e-5  5.7e-3 / 5.5e-3
Every error is two to six roundings of the float32 output itself (3.8e-6 dB between -64 and -32 dB) and at most 1.1 y: no kernel was
found wrong in this direction.  The fused forms were taken where the table says (counters), the window of 3/4 of a fused batch agrees
with the batch to <= 2.9e-5 dB (f32-class modes) and <= 2.3e-3 dB (f16x2); inverse() and sample_from_eps() repeat bit for bit and
follow a permutation of the batch bit for bit.  One check found something: see test_a_tile_inverts_alone_as_in_its_batch.
On this device the grid rule of launch_h3s prefers the co-resident fused kernel wherever the eight-wave 256-pixel one could run
(2 * ceil(Q / 256) > CUs implies ceil(Q / 128) > CUs), so the latter is reached with GLOWK_CO_OFF=1, as tests/test_gpu_fused_coupling.py
does; both forms of those two cases are held to the oracle.
"""
import os

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib
from audiosourcesep_amd.synthetic import calibrated_engine, synthetic_mel_tiles
from tests import inverse_cases as IC

pytestmark = pytest.mark.gpu

PREC = {"f32": _lib.PREC_F32, "f16x3": _lib.PREC_F16X3, "f16x2": _lib.PREC_F16X2}
FACTOR = {"f32": 8.0, "f16x3": 16.0}     # multiples of the case's yardstick
F16X2_BAR = 0.3                          # dB
YARDSTICK_CAP = 1e-4                     # dB: no bar above 1.6e-3 dB


@pytest.fixture(scope="module")
def cus():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return IC.device_cus()


def _setenv(name, on):
    """The engine reads its diagnostic switches at load time: change one and have them read again (glowk_reload_env)."""
    if on:
        os.environ[name] = "1"
    else:
        os.environ.pop(name, None)
    _lib.load().glowk_reload_env()


def _set_arith(eng, arith):
    eng.set_precision(PREC[arith])
    if arith != "f32":
        eng.set_range_policy("error")


def _bar(arith, y):
    return F16X2_BAR if arith == "f16x2" else FACTOR[arith] * y


def _counted(eng, call):
    """call() and what it added to the engine's launch counters."""
    before, fused = eng.kernel_families(), eng.fused_steps
    out = call()
    torch.cuda.synchronize()
    fam = {k: v - before[k] for k, v in eng.kernel_families().items()}
    fam["fused_steps"] = eng.fused_steps - fused
    return out, fam


def _check_form(case, arith, cus, co_off, fam):
    """The counters of one inverse() call say what the restated rule says: K fused level-0 steps or none, co-resident or not."""
    cfg = case.cfg
    h, w, c = cfg.level_shapes()[0]
    px = IC.fused_px(case.n, h, w, c, cfg.F, arith != "f32", cus, co_off)
    assert fam["fused_steps"] == fam["fused"] == (cfg.K if px else 0), (arith, co_off, px, fam)
    if arith == "f32":
        assert fam["f32"] == cfg.K * cfg.L and sum(fam[k] for k in ("h3_32x32x16", "h3s_16x16x32", "h3s_half", "fused")) == 0, fam
    else:
        # (a split request falls back to k_net_f32 only where the shape has no split instance: the 32-channel level at n_filters 128)
        assert fam["f32"] == cfg.K * sum(1 for (_, _, lc) in cfg.level_shapes() if lc == 32 and cfg.F == 128), fam
    if px == 128:
        assert fam["co_resident"] in (cfg.K, 2 * cfg.K), fam      # (the 8-channel level too where its grid is large enough)
    if co_off:
        assert fam["co_resident"] == 0, fam


@pytest.mark.parametrize("name", list(IC.CASES))
def test_inverse_and_sample_against_the_fp64_oracle(name, cus):
    case = IC.CASES[name]
    cfg, n = case.cfg, case.n
    eng, params = calibrated_engine(cfg, device=0, init_tiles=case.init_tiles)
    x = torch.from_numpy(synthetic_mel_tiles(n, cfg, seed=case.seed)).cuda()
    z = eng.forward(x, with_logdet=False)                               # exact fp32: the common input of both sides
    eps = torch.from_numpy(IC.latent_noise(case)).cuda()
    idx = IC.tile_subset(case, cus)
    ref = IC.references(params, cfg, z[idx].cpu().numpy(), eps[idx].cpu().numpy())
    y_i, y_s = ref["y_inverse"], ref["y_sample"]
    print("\n%s tiles %s: yardstick inverse %.1e dB, sample %.1e dB" % (name, idx, y_i, y_s))
    assert 0 < y_i <= YARDSTICK_CAP and 0 < y_s <= YARDSTICK_CAP         # (the inputs' condition: tests/test_inverse_oracle_cpu.py)
    x_ref, s_ref = torch.from_numpy(ref["inverse"]), torch.from_numpy(ref["sample"])
    h0, w0, c0 = cfg.level_shapes()[0]
    failures = []
    for arith in IC.ARITHMETICS:
        _set_arith(eng, arith)
        for co_off in ((False, True) if (case.co_off and arith != "f32") else (False,)):
            _setenv("GLOWK_CO_OFF", co_off)
            try:
                xr, fam = _counted(eng, lambda: eng.inverse(z))
                _check_form(case, arith, cus, co_off, fam)
                xs = eng.sample_from_eps(eps)
                assert torch.equal(eng.inverse(z), xr) and torch.equal(eng.sample_from_eps(eps), xs)     # repeatable bit for bit
                e_i = float((xr[idx].cpu().double() - x_ref).abs().max())
                e_s = float((xs[idx].cpu().double() - s_ref).abs().max())
                tag = arith + (" (GLOWK_CO_OFF)" if co_off else "")
                print("   %-22s inverse %.1e dB (bar %.1e), sample %.1e dB (bar %.1e); round trip of the batch %.1e dB" % (
                    tag, e_i, _bar(arith, y_i), e_s, _bar(arith, y_s), float((xr - x).abs().max())))
                assert torch.isfinite(xr).all() and torch.isfinite(xs).all()
                if not e_i <= _bar(arith, y_i):
                    failures.append((tag, "inverse", e_i, _bar(arith, y_i)))
                if not e_s <= _bar(arith, y_s):
                    failures.append((tag, "sample", e_s, _bar(arith, y_s)))
                if IC.fused_px(n, h0, w0, c0, cfg.F, arith != "f32", cus, co_off):
                    # batch independence through the fused kernels: a window of the batch moves the workgroup boundaries (and may
                    # change the deeper levels' forms), so the tiles agree within the arithmetic's bar, not bit for bit
                    m = max(n * 3 // 4, 1)
                    xw, famw = _counted(eng, lambda: eng.inverse(z[:m].contiguous()))
                    assert famw["fused_steps"] == cfg.K, famw
                    d = float((xw - xr[:m]).abs().max())
                    print("   %-22s window of %d tiles against the batch: %.1e dB" % ("", m, d))
                    if not d <= _bar(arith, y_i):
                        failures.append((tag, "window", d, _bar(arith, y_i)))
                if arith != "f32":
                    assert eng.range_status() == (False, 0)
            finally:
                _setenv("GLOWK_CO_OFF", False)
    assert not failures, failures


@pytest.mark.parametrize("arith", IC.ARITHMETICS)
@pytest.mark.parametrize("name", ["16x16_L2_n3", "8x8_L2_n515"])
def test_a_tile_inverts_alone_as_in_its_batch(name, arith):
    """Batch independence in this direction, as tests/test_gpu_parity.py::test_config_B_full_size_properties claims it for log_prob:
    inverse() of the batch twice is one result, a permuted batch gives the permuted result, and a tile's inverse() inside the batch
    is, bit for bit, its inverse() alone.

    The invariant behind the last claim: the one-lane k_couple<., false> (batches of >= 2 x compute units tiles) and the four-lane
    k_couple<., true> / k_couple_flat<., 4> add the nine taps of every partial P buffer in the same order (couple_pixel,
    csrc/glowk_light.h), and the network launch of these shapes is the same for one tile and for the batch.  The sixteen-lane
    k_couple_flat<., 16> adds in an order of its own and is not part of the claim: neither case reaches it at either batch size."""
    case = IC.CASES[name]
    cfg, n = case.cfg, case.n
    eng, _ = calibrated_engine(cfg, device=0, init_tiles=case.init_tiles)
    x = torch.from_numpy(synthetic_mel_tiles(n, cfg, seed=case.seed)).cuda()
    z = eng.forward(x, with_logdet=False)
    _set_arith(eng, arith)
    xr = eng.inverse(z)
    assert torch.equal(eng.inverse(z), xr)
    perm = torch.from_numpy(np.random.default_rng(0).permutation(n)).cuda()
    assert torch.equal(eng.inverse(z[perm].contiguous()), xr[perm])
    worst = {}
    for t in sorted({0, n // 2, n - 1}):
        alone = eng.inverse(z[t:t + 1].contiguous())
        worst[t] = float((alone - xr[t:t + 1]).abs().max()) if not torch.equal(alone, xr[t:t + 1]) else None
        print(name, arith, "tile %d alone against the batch: %s" % (t, "equal" if worst[t] is None else "%.1e dB" % worst[t]))
    assert all(v is None for v in worst.values()), worst


def test_table_reaches_every_launch_form_on_this_device(cus):
    """The forms the cases above go through, by the restated launch rule with this device's compute-unit count (the fused ones are
    also asserted from the engine's counters, case by case).  A device with another count fails HERE instead of testing less."""
    seen = {}
    for name, case in IC.CASES.items():
        for arith in IC.ARITHMETICS:
            for co_off in ((False, True) if (case.co_off and arith != "f32") else (False,)):
                for form in IC.forms_of(case, arith, cus, co_off):
                    seen.setdefault(form, []).append("%s/%s%s" % (name, arith, "/co_off" if co_off else ""))
    for form in IC.ALL_FORMS:
        print("%-24s %s" % (form, ", ".join(seen.get(form, ["-- not reached --"])[:4])))
    assert set(seen) == set(IC.ALL_FORMS), sorted(set(IC.ALL_FORMS) ^ set(seen))
