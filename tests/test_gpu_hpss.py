"""Harmonic / percussive separation on the GPU (csrc/glowk_hpss.h through ``audiosourcesep_amd.hpss``) against the restatement of
tests/hpss_ref.py.

Bars.  Filters: bitwise -- the median is a selection, no arithmetic touches the values.  Masks: 1e-6 absolute against the fp64
restatement fed the device's own medians: a mask lies in [0, 1] and is a quotient of two powers, each with relative error at most
about (p / 2 + 2) 2^-23, <= 4e-7 for p <= 10 (numpy's own fp32 evaluation: 0.7 - 1.3e-7).  Components: 1 ulp of S mask.  Audio: 1e-5
of the mixture's peak over every sample, the bar of the whole-file inversion of tests/test_gpu_longform.py, whose path this is."""
import functools
import wave

import numpy as np
import pytest
import torch

from audiosourcesep_amd import audio, hpss
from tests import hpss_ref as R

pytestmark = pytest.mark.gpu

# (nsig, rows, F, size).  The frames filter gives a wave 64 frames of one line and a workgroup 4 lines; the rows filter gives a
# workgroup 64 frames x 64 rows: sizes on either side of each.
FILTER_CASES = [
    (1, 7, 4, 31),                          # the window far longer than both axes: several reflections
    (1, 9, 1, 5),                           # a single frame
    (1, 1, 40, 31),                         # a single row
    (1, 12, 30, 1),                         # the identity
    (3, 33, 63, 31), (3, 33, 64, 31), (3, 33, 65, 31), (3, 33, 129, 31),     # either side of a 64-frame tile edge; the signal stride
    (2, 1025, 5, 17),                       # the real row count: 17 row chunks, the last with one row
    (1, 130, 70, 127),                      # the largest halo
    (1, 63, 5, 17), (1, 64, 5, 17), (1, 65, 5, 17),                          # the 64-row chunk and one off it
    (1, 3, 70, 5), (1, 4, 70, 5), (1, 5, 70, 5),                             # the frames filter's 4 lines per workgroup and one off it
    (2, 96, 64, 31),                        # the mel rows, one extract wide
]


def quantised(rng, shape):
    """|N(0, 1)| quantised to 8 levels (multiples of 1/2, so a margin of 2.5 or 3 multiplies them exactly), 30 % exact zeros."""
    x = np.minimum(np.floor(np.abs(rng.standard_normal(shape)) * 2.0), 7.0) / 2.0
    x[rng.random(shape) < 0.3] = 0.0
    return x.astype(np.float32)


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("nsig,rows,F,size", FILTER_CASES)
def test_median_filter_bitwise(nsig, rows, F, size, axis):
    S = quantised(np.random.default_rng(1000 * rows + 10 * F + size), (nsig, rows, F))
    want = R.median_filter(S, size, axis)
    got = hpss.median_filter(S, size, axis)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == S.shape
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    again = hpss.median_filter(torch.from_numpy(S).cuda(), size, ("frames", "rows")[axis])       # a second run, from the device
    assert torch.equal(got, again)
    for i in range(nsig):                                                          # a batch gives what its signals give alone
        assert torch.equal(hpss.median_filter(S[i], size, axis), got[i])


def test_median_filter_of_continuous_values_and_negative_ones():
    S = np.random.default_rng(3).standard_normal((2, 70, 131)).astype(np.float32)
    for axis, size in ((0, 31), (1, 31), (0, 127), (1, 5)):
        np.testing.assert_array_equal(hpss.median_filter(S, size, axis).cpu().numpy(), R.median_filter(S, size, axis))
    assert tuple(hpss.median_filter(np.zeros((0, 5, 7), np.float32), 3, 0).shape) == (0, 5, 7)


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
POWERS = [0.5, 1.0, 2.0, 10.0, float("inf")]
MARGINS = [(1.0, 1.0), (2.5, 1.0), (1.0, 3.0)]


@functools.lru_cache(maxsize=None)
def filtered():
    """A quantised [2, 40, 70] spectrum with an all-zero block and the device's own medians of it (size 5).  Never modified."""
    S = quantised(np.random.default_rng(11), (2, 40, 70))
    S[:, :, 20:40] = 0.0
    harm, perc = hpss.median_filter(S, 5, 0).cpu().numpy(), hpss.median_filter(S, 5, 1).cpu().numpy()
    for a in (S, harm, perc):
        a.setflags(write=False)
    return S, harm, perc


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("power", POWERS)
def test_masks_against_the_restatement(power, margin):
    S, harm, perc = filtered()
    zero = (harm == 0) & (perc == 0)
    assert zero[:, :, 22:38].all() and not zero.all()
    mh, mp = (m.cpu().numpy() for m in hpss.hpss(S.copy(), kernel_size=5, power=power, mask=True, margin=margin))
    wh, wp = R.masks(harm, perc, power, margin)
    err = max(float(np.abs(mh - wh).max()), float(np.abs(mp - wp).max()))
    print("masks power = %g, margins %s: max abs error %.3e" % (power, margin, err))
    assert err <= 1e-6
    assert mh.min() >= 0.0 and mh.max() <= 1.0 and mp.min() >= 0.0 and mp.max() <= 1.0
    if np.isinf(power):                                                            # the hard mask, the zero block included
        assert np.array_equal(mh, (harm.astype(np.float64) > perc.astype(np.float64) * margin[0]).astype(np.float32))
        assert np.array_equal(mp, (perc.astype(np.float64) > harm.astype(np.float64) * margin[1]).astype(np.float32))
        return
    split = 0.5 if margin == (1.0, 1.0) else 0.0
    assert (mh[zero] == split).all() and (mp[zero] == split).all()
    if margin == (1.0, 1.0):                                                       # a / (a + b) + b / (b + a): two roundings of 2^-25
        assert np.abs(mh[~zero].astype(np.float64) + mp[~zero] - 1.0).max() <= 2.0 ** -22


def test_masks_of_continuous_spectra():
    """Values that are no multiples of 1/2: every power and quotient rounds."""
    S = np.abs(np.random.default_rng(5).standard_normal((33, 65))).astype(np.float32) ** 3
    harm, perc = hpss.median_filter(S, 7, 0).cpu().numpy(), hpss.median_filter(S, 7, 1).cpu().numpy()
    for power in POWERS[:4]:
        for margin in MARGINS:
            mh, mp = (m.cpu().numpy() for m in hpss.hpss(S, kernel_size=7, power=power, mask=True, margin=margin))
            wh, wp = R.masks(harm, perc, power, margin)
            err = max(float(np.abs(mh - wh).max()), float(np.abs(mp - wp).max()))
            print("continuous spectra, power = %g, margins %s: max abs error %.3e" % (power, margin, err))
            assert err <= 1e-6


# ---- hpss ----------------------------------------------------------------------------------------------------------------------------
def test_hpss_components_are_the_masked_spectrum():
    rng = np.random.default_rng(21)
    S = np.abs(rng.standard_normal((2, 33, 65))).astype(np.float32)
    S[rng.random(S.shape) < 0.1] = 0.0
    for margin in (1.0, (2.0, 1.5)):
        comps = hpss.hpss(S, margin=margin)
        masks = hpss.hpss(S, mask=True, margin=margin)
        for c, m in zip(comps, masks):
            assert c.dtype == torch.float32 and tuple(c.shape) == S.shape
            want = S.astype(np.float64) * m.cpu().numpy().astype(np.float64)
            assert (np.abs(c.cpu().numpy() - want) <= np.spacing(np.abs(want).astype(np.float32))).all()       # 1 ulp
    assert torch.equal(hpss.hpss(S[0])[0], hpss.hpss(S)[0][0])                     # [rows, F] is the batch of one
    # complex input: the components carry the input's phase.  exp(i angle(S)) in fp32: the angle within an ulp of pi (2.4e-7), its
    # cosine and sine within an ulp (6e-8), the product's rounding (6e-8) -- below 4e-7 together; the bar is 1e-6
    phi = rng.uniform(-np.pi, np.pi, S.shape)
    Sc = (S * np.exp(1j * phi)).astype(np.complex64)
    Hc, Pc = hpss.hpss(Sc)
    mag = np.abs(Sc)
    Hr, Pr = hpss.hpss(mag)
    for c, r in ((Hc, Hr), (Pc, Pr)):
        assert c.dtype == torch.complex64 and tuple(c.shape) == S.shape
        c, r = c.cpu().numpy(), r.cpu().numpy()
        live = r > 0
        assert live.any() and np.abs(c[live] / np.abs(c[live]) - Sc[live] / mag[live]).max() <= 1e-6
        assert np.abs(np.abs(c) - r).max() <= 1e-6 * r.max() and not c[~live].any()


def test_a_kernel_size_pair_changes_the_percussive_filter_only():
    S = quantised(np.random.default_rng(31), (40, 70))
    scalar, same, pair = hpss.hpss(S, 31, mask=True), hpss.hpss(S, (31, 31), mask=True), hpss.hpss(S, (31, 17), mask=True)
    assert torch.equal(scalar[0], same[0]) and torch.equal(scalar[1], same[1])
    assert not torch.equal(pair[0], scalar[0]) and not torch.equal(pair[1], scalar[1])
    harm, perc17 = hpss.median_filter(S, 31, "frames").cpu().numpy(), hpss.median_filter(S, 17, "rows").cpu().numpy()
    for got, want in zip(pair, R.masks(harm, perc17, 2.0, 1.0)):                   # the harmonic filter kept 31 frames, the percussive took 17 rows
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-6
    flipped = hpss.hpss(S, (17, 31), mask=True)
    harm17, perc = hpss.median_filter(S, 17, "frames").cpu().numpy(), hpss.median_filter(S, 31, "rows").cpu().numpy()
    for got, want in zip(flipped, R.masks(harm17, perc, 2.0, 1.0)):
        assert np.abs(got.cpu().numpy() - want).max() <= 1e-6


# ---- audio ---------------------------------------------------------------------------------------------------------------------------
N_AUDIO = 24576
AUDIO_BAR = 1e-5


@functools.lru_cache(maxsize=None)
def mixture():
    """(sines, clicks, y) as float32, y their sum: two sines and a click train, 24 576 samples at 16 kHz.  Never modified."""
    sines, clicks = (c.astype(np.float32) for c in R.sines_and_clicks(N_AUDIO))
    out = (sines, clicks, sines + clicks)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_stems(kernel_size, margin):
    return R.hpss_audio(mixture()[2].astype(np.float64), kernel_size=kernel_size, margin=margin, residual=True)


@pytest.mark.parametrize("kernel_size", [31, 17])
def test_hpss_audio_against_the_restatement(kernel_size):
    sines, clicks, y = mixture()
    peak = float(np.abs(y).max())
    h, p = hpss.hpss_audio(y.copy(), kernel_size=kernel_size)
    assert h.is_cuda and tuple(h.shape) == tuple(p.shape) == (N_AUDIO,) and h.dtype == torch.float32
    h, p = h.cpu().numpy(), p.cpu().numpy()
    wh, wp, _ = reference_stems(kernel_size, 1.0)
    e_h, e_p = float(np.abs(h - wh).max() / peak), float(np.abs(p - wp).max() / peak)
    e_sum = float(np.abs(h.astype(np.float64) + p - y).max() / peak)
    print("hpss_audio kernel_size = %d: harmonic %.2e, percussive %.2e, harmonic + percussive - y %.2e of the peak" % (kernel_size, e_h, e_p, e_sum))
    assert e_h <= AUDIO_BAR and e_p <= AUDIO_BAR and e_sum <= AUDIO_BAR
    # the device's masks of the mixture on each component's own STFT: the sines belong to the harmonic stem, the clicks to the other
    _, X = audio.mel_frames(np.stack([y, sines, clicks]), return_stft=True)
    mask_h, mask_p = hpss.hpss(X[0].abs(), kernel_size=kernel_size, mask=True)
    in_h = float(((mask_h * X[1].abs()) ** 2).sum() / (X[1].abs() ** 2).sum())
    in_p = float(((mask_p * X[2].abs()) ** 2).sum() / (X[2].abs() ** 2).sum())
    print("kernel_size = %d: %.4f of the sines' energy in the harmonic stem, %.4f of the clicks' in the percussive" % (kernel_size, in_h, in_p))
    assert in_h >= 0.9 and in_p >= 0.9


def test_hpss_audio_channels_and_residual():
    y = mixture()[2]
    two = np.stack([y, 0.5 * y[::-1]]).astype(np.float32)
    h2, p2 = hpss.hpss_audio(two)
    assert tuple(h2.shape) == tuple(p2.shape) == (2, N_AUDIO)
    for c in range(2):                                                             # a channel's stems depend on that channel alone
        h, p = hpss.hpss_audio(two[c])
        assert torch.equal(h2[c], h) and torch.equal(p2[c], p)
    assert len(hpss.hpss_audio(y.copy(), residual=False)) == 2
    yt = torch.from_numpy(y.copy()).cuda()
    h, p, r = hpss.hpss_audio(yt, margin=2.0, residual=True)
    assert tuple(r.shape) == (N_AUDIO,) and float(r.abs().max()) > 1e-3              # a margin above 1 leaves a residual
    assert torch.equal(r, yt - h - p)                                              # the residual is y minus the other two
    # summed back in fp32, (h + p) + r returns y up to the roundings of the two subtractions and the two additions: 4 x 2^-24 of
    # the largest magnitude on the way
    top = float(max(yt.abs().max(), h.abs().max(), p.abs().max(), (h + p).abs().max()))
    assert float(((h + p) + r - yt).abs().max()) <= 4 * 2.0 ** -24 * top
    wh, wp, wr = reference_stems(31, 2.0)
    peak = float(np.abs(y).max())
    errs = [float(np.abs(a.cpu().numpy() - w).max() / peak) for a, w in ((h, wh), (p, wp), (r, wr))]
    print("hpss_audio margin = 2: harmonic %.2e, percussive %.2e, residual %.2e of the peak" % tuple(errs))
    assert max(errs[:2]) <= AUDIO_BAR and errs[2] <= 2 * AUDIO_BAR                  # the residual carries both stems' errors


def test_separate_wav_hpss_returns_the_files_rate_and_length(tmp_path):
    rate = 22050
    sines, clicks = R.sines_and_clicks(N_AUDIO, rate)
    y = sines + clicks
    q = np.rint(np.clip(np.stack([y, 0.5 * y]), -1.0, 1.0) * 32767.0).astype("<i2")
    mono, stereo = tmp_path / "mono.wav", tmp_path / "stereo.wav"
    for path, data in ((mono, q[:1]), (stereo, q)):
        with wave.open(str(path), "wb") as w:
            w.setnchannels(data.shape[0])
            w.setsampwidth(2)
            w.setframerate(rate)
            w.writeframes(np.ascontiguousarray(data.T).tobytes())
    stems, out_rate = hpss.separate_wav_hpss(str(mono))
    assert out_rate == rate and tuple(stems.shape) == (2, N_AUDIO) and bool(torch.isfinite(stems).all()) and float(stems.abs().max()) > 0.1
    n16 = -(-N_AUDIO * 16000 // rate)                                              # 24 576 samples at 22 050 Hz are 17 833 at 16 kHz
    stems, out_rate = hpss.separate_wav_hpss(str(mono), out_rate=None, margin=2.0, residual=True)
    assert out_rate == 16000 and tuple(stems.shape) == (3, n16)
    stems, out_rate = hpss.separate_wav_hpss(str(stereo), kernel_size=(31, 17))
    assert out_rate == rate and tuple(stems.shape) == (2, 2, N_AUDIO) and bool(torch.isfinite(stems).all())
    stems, out_rate = hpss.separate_wav_hpss(str(stereo), out_rate=8000, mono=True)
    assert out_rate == 8000 and tuple(stems.shape) == (2, -(-n16 * 8000 // 16000))
