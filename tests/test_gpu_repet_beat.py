"""REPET's front end and REPET itself on the GPU (csrc/glowk_beat.h through ``audiosourcesep_amd.repet``) against the fp64
restatement of tests/repet_beat_ref.py.

Bars.  Beat values: per element ``|dev - ref| <= 2 (rows + 8) 2^-24 ref`` -- derived, not measured: numerator and denominator each
carry at most (rows + 2) 2^-24 relative error (one fp32 square per operand, then an fp32 chain of ``rows`` non-negative terms), the
fp64 part and the final rounding are below the slack; where the restatement is zero the device is zero.  Period and neighbours:
exact, they are integer rules.  Filter: bitwise (a selection, at an even count one fp32 (a + b) * 0.5).  Masks: 1e-6 absolute
against fp64 fed the device's filter; audio: 1e-5 of the mixture's peak -- the bars of tests/test_gpu_repet.py for the same kernels
on the same path.

Measured on an MI355X (largest |dev - ref| / (bar ref) per shape, all nlags): see the table in DESIGN section 19."""
import functools
import wave

import numpy as np
import pytest
import torch

from audiosourcesep_amd import audio, repet
from tests import audio_ref as A
from tests import repet_beat_ref as B
from tests import repet_ref as R

pytestmark = pytest.mark.gpu

# (nsig, rows, F): odd and single rows, frame counts on both sides of a tile edge (32 query frames, 64 candidate frames), bands that
# end inside a tile, several chunks of query tiles per column (F > 128), and at 4500 frames two query tiles per wave
SHAPES = [(1, 1, 1), (1, 1, 33), (1, 2, 31), (3, 33, 95), (1, 1025, 257), (2, 96, 600), (1, 4096, 66), (1, 2, 4500)]
WINDOWS = [(2, 1), (7, 3), (32, 16), (33, 33), (95, 1), (95, 95)]                   # (win, step) on F = 95


def continuous(rng, shape):
    """|N(0, 1)|^2 with about 5 % all-zero frames (none in a signal of fewer than 8 frames)."""
    x = (np.abs(rng.standard_normal(shape)) ** 2).astype(np.float32)
    silent = (rng.random(shape[-1]) < 0.05) & (shape[-1] >= 8)
    if shape[-1] >= 8:
        silent[shape[-1] // 2] = True
    x[..., silent] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def spectra(shape):
    S = continuous(np.random.default_rng(1000 * shape[1] + shape[2]), shape)
    S.setflags(write=False)
    return S


def lag_counts(F):
    return sorted({n for n in (1, 2, 31, 32, 33, F - 1, F) if 1 <= n <= F})


def worst_ratio(dev, ref, rows):
    """The largest |dev - ref| / (bar ref); where ref is 0 the device must be 0."""
    assert dev.shape == ref.shape and dev.dtype == np.float32
    zero = ref == 0
    assert not dev[zero].any()
    if zero.all():
        return 0.0
    return float((np.abs(dev[~zero].astype(np.float64) - ref[~zero]) / (B.bar(rows) * ref[~zero])).max())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_beat_spectrum_against_the_restatement(shape):
    nsig, rows, F = shape
    S = spectra(shape)
    ref = B.beat_spectrum(S, F)                                                     # [nsig, F]; fewer lags are its first ones
    worst = 0.0
    for nlags in lag_counts(F):
        got = repet.beat_spectrum(S.copy(), nlags)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (nsig, nlags)
        got = got.cpu().numpy()
        assert (got[:, 0] == 1.0).all()
        worst = max(worst, worst_ratio(got, ref[:, :nlags], rows))
        again = repet.beat_spectrum(torch.from_numpy(S.copy()).cuda(), nlags)       # a second run, from the device
        assert np.array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32))
        if nsig > 1:                                                                # a batch gives what its signals give alone
            for n in range(nsig):
                alone = repet.beat_spectrum(S[n].copy(), nlags)
                assert tuple(alone.shape) == (nlags,) and np.array_equal(alone.cpu().numpy().view(np.uint32), got[n].view(np.uint32))
    print("beat spectrum %s: largest |dev - ref| / (bar ref) = %.4f, bar %.3e" % (shape, worst, B.bar(rows)))
    assert worst <= 1.0


@pytest.mark.parametrize("win,step", WINDOWS)
def test_beat_spectrogram_against_the_restatement(win, step):
    nsig, rows, F = 3, 33, 95
    S = spectra((nsig, rows, F)).copy()
    S[1] = 0.0                                                                      # a silent signal
    S[2, :, 40:] = 0.0                                                              # silent windows in a signal that is not
    nwin = -(-F // step)
    worst = 0.0
    for nlags in sorted({1, min(win, 31), win, min(F, win + 5), F}):
        ref = B.beat_spectrogram(S, nlags, win, step)
        got = repet.beat_spectrogram(S.copy(), win, step, nlags)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (nsig, nwin, nlags) == ref.shape
        got = got.cpu().numpy()
        worst = max(worst, worst_ratio(got, ref, rows))
        assert not got[1].any() and (got[0, :, 0] == 1.0).all()
        for t, (a, n) in enumerate(B.windows(F, win, step)):
            assert not got[:, t, n:].any()                                          # no pair of frames that far apart in the window
            if a >= 40:
                assert not got[2, t].any()                                          # a silent window
        again = repet.beat_spectrogram(torch.from_numpy(S.copy()).cuda(), win, step, nlags)
        assert np.array_equal(again.cpu().numpy().view(np.uint32), got.view(np.uint32))
        for n in (0, 2):
            alone = repet.beat_spectrogram(S[n].copy(), win, step, nlags).cpu().numpy()
            assert np.array_equal(alone.view(np.uint32), got[n].view(np.uint32))
    clipped = B.windows(F, win, step)
    # the first window is cut short, and the last one too where it sticks out ((2, 1) and (33, 33) end inside the signal)
    assert clipped[0][1] == win - win // 2 and (clipped[-1][1] < win) == ((win, step) not in ((2, 1), (33, 33)))
    print("beat spectrogram (win, step) = (%d, %d): largest |dev - ref| / (bar ref) = %.4f" % (win, step, worst))
    assert worst <= 1.0


def test_defaults_the_whole_signal_window_and_empty_batches():
    S = spectra((3, 33, 95))
    F = 95
    full = repet.beat_spectrum(S.copy())                                            # nlags = F
    assert tuple(full.shape) == (3, F) and torch.equal(full, repet.beat_spectrum(S.copy(), F))
    spec = repet.beat_spectrogram(S.copy(), 32)                                     # step = 16, nlags = 32
    assert tuple(spec.shape) == (3, 6, 32) and torch.equal(spec, repet.beat_spectrogram(S.copy(), 32, 16, 32))
    # window t of (win, step) = (F, 1) covers [t - F // 2, t - F // 2 + F): at t = F // 2 the whole signal, cut up as the beat
    # spectrum cuts it, so the bits are the same.  (win = F, step = F has the one window [0, F - F // 2): held to the bar above.)
    for nlags in (33, F):
        whole = repet.beat_spectrogram(S.copy(), F, 1, nlags)[:, F // 2]
        assert torch.equal(whole, repet.beat_spectrum(S.copy(), nlags))
    assert tuple(repet.beat_spectrum(np.zeros((0, 5, 7), np.float32), 3).shape) == (0, 3)
    assert tuple(repet.beat_spectrogram(np.zeros((0, 5, 7), np.float32), 4, 2).shape) == (0, 4, 4)
    assert tuple(repet.find_period(np.zeros((0, 9), np.float32), 2, 5).shape) == (0,)
    assert tuple(repet.period_neighbors(np.zeros((0,), np.int32), 7, 3).shape) == (0, 7, 3)


def test_find_period_is_the_restatements_rule_on_the_devices_own_values():
    for shape, pmin, pmax in [((3, 33, 95), 2, 31), ((2, 96, 600), 1, 599), ((1, 1025, 257), 5, 200), ((1, 2, 31), 30, 30), ((1, 1, 33), 1, 1)]:
        beat = repet.beat_spectrum(spectra(shape).copy())
        got = repet.find_period(beat, pmin, pmax)
        assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (shape[0],)
        assert np.array_equal(got.cpu().numpy(), B.find_period(beat.cpu().numpy(), pmin, pmax))
    spec = repet.beat_spectrogram(spectra((3, 33, 95)).copy(), 32, 16)
    got = repet.find_period(spec, 2, 10)
    assert tuple(got.shape) == (3, 6) and np.array_equal(got.cpu().numpy(), B.find_period(spec.cpu().numpy(), 2, 10))
    # values from the host, ties included: quantised to 4 levels, so most maxima are shared
    rng = np.random.default_rng(8)
    q = (np.floor(rng.random((50, 300)) * 4) / 4).astype(np.float32)
    for pmin, pmax in [(1, 299), (7, 7), (64, 128), (65, 299)]:
        assert np.array_equal(repet.find_period(q, pmin, pmax).cpu().numpy(), B.find_period(q, pmin, pmax))
    assert repet.find_period(np.zeros(9, np.float32), 3, 8).item() == 3            # all zeros give pmin


def test_ties_give_the_lowest_lag():
    """One row of constants: P = 2.25, every product 5.0625 and every sum of them exact, so every normalised lag is exactly 1."""
    S = np.full((1, 95), 1.5, np.float32)
    beat = repet.beat_spectrum(S)
    assert (beat == 1.0).all()
    for pmin, pmax in [(2, 31), (1, 94), (40, 90), (94, 94)]:
        assert repet.find_period(beat, pmin, pmax).item() == pmin
        assert repet.repet(S, period_range=(pmin, pmax), return_period=True)[2] == pmin


@pytest.mark.parametrize("case", B.PLANTED, ids=lambda c: "-".join(map(str, c)))
def test_the_planted_period_is_found(case):
    S, pmin, pmax = B.planted_case(case)
    beat = repet.beat_spectrum(S.copy(), pmax + 1)
    assert repet.find_period(beat, pmin, pmax).item() == case[1]
    assert repet.repet(S.copy(), period_range=(pmin, pmax), return_period=True)[2] == case[1]


def test_period_neighbors_equal_the_restatement():
    for p, frames, k in [(3, 10, 4), (3, 10, 3), (3, 10, 2), (1, 70, 512), (16, 95, 6), (16, 95, 5), (95, 95, 3), (1000, 95, 3), (0, 20, 5), (-7, 20, 5),
                         (7, 1, 1), (2, 300, 150), (2, 300, 149), (1, 600, 512)]:
        got = repet.period_neighbors(p, frames, k)
        assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (frames, k)
        assert np.array_equal(got.cpu().numpy(), B.period_neighbors(np.asarray(p), frames, k)), (p, frames, k)
    per = np.array([[3, 0], [17, 2 ** 31 - 1]], np.int64)                          # a batch, one period per signal
    assert np.array_equal(repet.period_neighbors(per, 40, 7).cpu().numpy(), B.period_neighbors(per, 40, 7))
    rng = np.random.default_rng(4)
    for frames, step, nper, k in [(95, 7, 14, 5), (95, 7, 3, 5), (95, 16, 6, 4), (33, 33, 1, 9), (257, 10, 26, 3), (64, 1, 64, 2)]:
        per = rng.integers(-2, 20, (3, nper)).astype(np.int32)                      # a step that does not divide F; too few periods
        got = repet.period_neighbors(torch.from_numpy(per).cuda(), frames, k, step)
        assert tuple(got.shape) == (3, frames, k)
        assert np.array_equal(got.cpu().numpy(), B.period_neighbors(per, frames, k, step)), (frames, step, nper, k)
        assert np.array_equal(repet.period_neighbors(per[1], frames, k, step).cpu().numpy(), got[1].cpu().numpy())


# ---- the filter and the masks ----------------------------------------------------------------------------------------------------------
def check_filter_and_masks(S, idx, mb, mf, power, margin):
    """idx: the device's neighbours; the device's median over them is bitwise gather_median's, the masks within 1e-6 of fp64."""
    x = torch.from_numpy(S.copy()).cuda()
    filt = repet._median(x, idx)                                                    # glowk_nn_median, as repet() calls it
    want = R.gather_median(S, idx.cpu().numpy())
    np.testing.assert_array_equal(filt.cpu().numpy().view(np.uint32), want.view(np.uint32))
    wb, wf = R.masks(S, want, power, margin)
    err = max(float(np.abs(mb.cpu().numpy() - wb).max()), float(np.abs(mf.cpu().numpy() - wf).max()))
    assert err <= 1e-6
    return err


@pytest.mark.parametrize("power,margin", [(1.0, (1.0, 1.0)), (2.0, (2.0, 10.0))])
def test_repet_filter_and_masks(power, margin):
    S = np.stack([B.planted_case(B.PLANTED[1])[0], spectra((3, 33, 95))[0, :, :60]])    # planted with 30 % noise, and no period at all
    _, pmin, pmax = B.planted_case(B.PLANTED[1])
    mb, mf, period = repet.repet(S.copy(), period_range=(pmin, pmax), power=power, margin=margin, mask=True, return_period=True)
    assert period.dtype == np.int32 and period.shape == (2,) and period[0] == 12 and pmin <= period[1] <= pmax
    k = -(-60 // pmin)
    idx = repet.period_neighbors(period, 60, k)
    assert np.array_equal(idx.cpu().numpy(), B.period_neighbors(period, 60, k))
    assert ((idx[0] >= 0).sum(-1) == 5).all()                                       # every congruent frame, the frame itself included
    err = check_filter_and_masks(S, idx, mb, mf, power, margin)
    print("repet masks power = %g, margins %s: max abs error %.3e" % (power, margin, err))
    b, f = (c.cpu().numpy() for c in repet.repet(S.copy(), period_range=(pmin, pmax), power=power, margin=margin))
    for c, m in ((b, mb), (f, mf)):                                                 # the components are the masked spectrum: 1 ulp
        want = S.astype(np.float64) * m.cpu().numpy().astype(np.float64)
        assert c.dtype == np.float32 and (np.abs(c - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    # a given period, one per signal or one for all; [rows, F] is the batch of one
    gb, gf = repet.repet(S.copy(), period=period, k=k, power=power, margin=margin, mask=True)
    assert torch.equal(gb, mb) and torch.equal(gf, mf)
    ob, of = repet.repet(S[0].copy(), period=12, power=power, margin=margin, mask=True)
    assert torch.equal(ob, mb[0]) and torch.equal(of, mf[0])
    if margin == (1.0, 1.0):
        one = repet.repet(S.copy(), period_range=(pmin, pmax), mask=True)           # the defaults are the ratio mask
        assert torch.equal(one[0], mb) and torch.equal(one[1], mf)
        rep = np.minimum(S, R.gather_median(S, idx.cpu().numpy())).astype(np.float64)
        live = S > 0
        assert np.abs(mb.cpu().numpy()[live] - rep[live] / S[live]).max() <= 1e-6  # W / V


@pytest.mark.parametrize("win,step,order", [(24, 12, 5), (30, 7, 3), (60, 60, 1)])
def test_repet_adaptive_filter_and_masks(win, step, order):
    S = np.stack([B.planted_case(B.PLANTED[1])[0], spectra((3, 33, 95))[0, :, :60]])
    F = 60
    mb, mf, period = repet.repet_adaptive(S.copy(), win, step, order=order, mask=True, return_period=True)
    nwin = -(-F // step)
    assert period.dtype == np.int32 and period.shape == (2, nwin) and (period >= 2).all() and (period <= win // 3).all()
    spec = repet.beat_spectrogram(S.copy(), win, step, win // 3 + 1)
    assert np.array_equal(period, B.find_period(spec.cpu().numpy(), 2, win // 3))
    idx = repet.period_neighbors(period, F, order, step)
    assert np.array_equal(idx.cpu().numpy(), B.period_neighbors(period, F, order, step))
    err = check_filter_and_masks(S, idx, mb, mf, 1.0, (1.0, 1.0))
    print("repet_adaptive (win, step, order) = (%d, %d, %d): max abs mask error %.3e" % (win, step, order, err))
    if order == 1:
        assert (mb == 1.0)[torch.from_numpy(S > 0).cuda()].all()                    # only the frame itself: everything repeats
    ob, of = repet.repet_adaptive(S[1].copy(), win, step, order=order, mask=True)
    assert torch.equal(ob, mb[1]) and torch.equal(of, mf[1])


def test_repet_of_complex_spectra_keeps_the_phase():
    rng = np.random.default_rng(21)
    S = continuous(rng, (2, 33, 65))
    phi = rng.uniform(-np.pi, np.pi, S.shape)
    Sc = (S * np.exp(1j * phi)).astype(np.complex64)
    mag = np.abs(Sc)
    for complex_out, real_out in ((repet.repet(Sc, period=7), repet.repet(mag, period=7)),
                                  (repet.repet_adaptive(Sc, 30, order=3), repet.repet_adaptive(mag, 30, order=3))):
        # exp(i angle(S)) in fp32 and one product: below 4e-7 together; the bar is 1e-6 (tests/test_gpu_repet.py)
        for c, r in zip(complex_out, real_out):
            assert c.dtype == torch.complex64 and tuple(c.shape) == S.shape and r.dtype == torch.float32
            c, r = c.cpu().numpy(), r.cpu().numpy()
            live = r > 0
            assert live.any() and np.abs(c[live] / np.abs(c[live]) - Sc[live] / mag[live]).max() <= 1e-6
            assert np.abs(np.abs(c) - r).max() <= 1e-6 * r.max() and not c[~live].any()


# ---- audio ---------------------------------------------------------------------------------------------------------------------------
N_AUDIO = 48000
PERIOD_SEC = (0.3, 0.8)                     # 10 .. 25 frames: of the multiples of the phrase's 16 frames only 16 itself
AUDIO_BAR = 1e-5
CUT_ROWS = 13                               # rows r with r 16000 / 2048 <= 100 Hz: 0 .. 12


@functools.lru_cache(maxsize=None)
def mixture():
    """(pattern, chirp, y) as float32, y their sum: 3 s at 16 kHz of a phrase of four 2048-sample notes -- 8192 samples, 16 frames
    exactly -- repeated, and tests/repet_ref.py's chirp, which never repeats.  Never modified."""
    sr, note = 16000, 2048
    t = np.arange(note) / sr
    fade = np.sin(np.pi * (np.arange(note) + 0.5) / note) ** 0.5
    phrase = np.concatenate([(0.25 * np.sin(2 * np.pi * f * t) + 0.15 * np.sin(2 * np.pi * 2.5 * f * t)) * fade
                             for f in (330.0, 440.0, 587.0, 392.0)])
    assert len(phrase) == 16 * audio.HOP
    pattern = np.tile(phrase, -(-N_AUDIO // len(phrase)))[:N_AUDIO]
    chirp = R.pattern_and_chirp(N_AUDIO)[1]
    out = tuple(c.astype(np.float32) for c in (pattern, chirp, pattern + chirp))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("adaptive", [False, True], ids=["repet", "adaptive"])
def test_repet_audio_against_the_restatement(adaptive):
    pattern, chirp, y = mixture()
    peak = float(np.abs(y).max())
    kw = dict(adaptive=True, win_sec=2.0, step_sec=1.0, order=5) if adaptive else {}
    b, f = repet.repet_audio(y.copy(), period_sec=PERIOD_SEC, **kw)
    assert b.is_cuda and tuple(b.shape) == tuple(f.shape) == (N_AUDIO,) and b.dtype == torch.float32
    b, f = b.cpu().numpy(), f.cpu().numpy()
    # the restatement's path: the fp64 rules on the device's |X| and beat values, the same inverse STFT
    _, X = audio.mel_frames(np.stack([y, chirp]), return_stft=True)
    mag = X[0].abs()
    F = mag.shape[1]
    assert F == 95
    pmin, pmax = 10, 25
    if adaptive:
        win, step = 62, 31                                                          # int(2 s 31.25), int(1 s 31.25); win // 3 = 20
        pmax = min(pmax, win // 3)
        spec = repet.beat_spectrogram(mag, win, step, pmax + 1)
        period = B.find_period(spec.cpu().numpy(), pmin, pmax)
        idx = B.period_neighbors(period, F, 5, step)
    else:
        period = B.find_period(repet.beat_spectrum(mag, pmax + 1).cpu().numpy(), pmin, pmax)
        idx = B.period_neighbors(period, F, -(-F // pmin))
    print("repet_audio (%s): period %s frames" % ("adaptive" if adaptive else "whole signal", period.tolist()))
    assert [m for m in range(pmin, pmax + 1) if m % 16 == 0] == [16] and (np.asarray(period) == 16).all()
    mag = mag.cpu().numpy()
    wb, wf = R.masks(mag, R.gather_median(mag, idx), 1.0, (1.0, 1.0))
    wb[:CUT_ROWS], wf[:CUT_ROWS] = 1.0, 0.0                                         # at most 100 Hz: wholly background
    X0 = X[0].cpu().numpy().astype(np.complex128)
    want_b, want_f = (A.istft(X0 * m)[:N_AUDIO] for m in (wb, wf))
    e_b, e_f = float(np.abs(b - want_b).max() / peak), float(np.abs(f - want_f).max() / peak)
    e_sum = float(np.abs(b.astype(np.float64) + f - y).max() / peak)
    print("repet_audio: background %.2e, foreground %.2e, background + foreground - y %.2e of the peak" % (e_b, e_f, e_sum))
    assert e_b <= AUDIO_BAR and e_f <= AUDIO_BAR and e_sum <= AUDIO_BAR            # unit margins: the stems sum to the mixture
    # the device's foreground mask of the mixture on the chirp's own STFT: what does not repeat is foreground
    if adaptive:
        _, mask_f = repet.repet_adaptive(X[0].abs(), 62, 31, (pmin, pmax), 5, mask=True)
    else:
        _, mask_f = repet.repet(X[0].abs(), period_range=(pmin, pmax), mask=True)
    in_f = float(((mask_f * X[1].abs()) ** 2).sum() / (X[1].abs() ** 2).sum())
    print("repet_audio (%s): %.4f of the chirp's energy in the foreground stem" % ("adaptive" if adaptive else "whole signal", in_f))
    assert in_f >= 0.9


def test_repet_audio_cutoff_channels_and_residual(monkeypatch):
    y = mixture()[2]
    two = np.stack([y, 0.5 * y[::-1]]).astype(np.float32)
    seen = []
    inverse = audio.griffinlim

    def spy(S, **kw):
        seen.append(S.clone())
        return inverse(S, **kw)

    monkeypatch.setattr(audio, "griffinlim", spy)
    b2, f2 = repet.repet_audio(two, period_sec=PERIOD_SEC)
    assert tuple(b2.shape) == tuple(f2.shape) == (2, N_AUDIO)
    _, X = audio.mel_frames(two, return_stft=True)
    mags = seen.pop()                                                               # [background of 2 channels, foreground of 2 channels]
    assert tuple(mags.shape) == (4, 1025, 95)
    assert not mags[2:, :CUT_ROWS].any() and mags[2:, CUT_ROWS].any()               # the foreground's rows 0 .. 12 are zero ...
    assert torch.equal(mags[:2, :CUT_ROWS], X.abs()[:, :CUT_ROWS])                  # ... and the background has all of them
    repet.repet_audio(two, period_sec=PERIOD_SEC, cutoff_hz=0.0)
    assert seen.pop()[2:, :CUT_ROWS].any()                                          # 0 switches it off
    repet.repet_audio(two, period_sec=PERIOD_SEC, cutoff_hz=7.0)
    mags = seen.pop()
    assert not mags[2:, :1].any() and mags[2:, 1].any()                             # below one row's spacing: row 0 alone
    for c in range(2):                                                              # a channel's stems depend on that channel alone
        b, f = repet.repet_audio(two[c], period_sec=PERIOD_SEC)
        assert torch.equal(b2[c], b) and torch.equal(f2[c], f)
    yt = torch.from_numpy(y.copy()).cuda()
    b, f, r = repet.repet_audio(yt, period_sec=PERIOD_SEC, margin=(2.0, 10.0), power=2.0, residual=True)
    assert tuple(r.shape) == (N_AUDIO,) and torch.equal(r, yt - b - f) and float(r.abs().max()) > 1e-3   # margins above 1 leave a residual


def test_separate_wav_repet_periodic_returns_the_files_rate_and_length(tmp_path):
    rate = 22050
    pattern, chirp = R.pattern_and_chirp(N_AUDIO, rate)
    y = pattern + chirp
    q = np.rint(np.clip(np.stack([y, 0.5 * y]), -1.0, 1.0) * 32767.0).astype("<i2")
    stereo = tmp_path / "stereo.wav"
    with wave.open(str(stereo), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(q.T).tobytes())
    stems, out_rate = repet.separate_wav_repet_periodic(str(stereo), period_sec=(0.3, 0.8))
    assert out_rate == rate and tuple(stems.shape) == (2, 2, N_AUDIO) and bool(torch.isfinite(stems).all()) and float(stems.abs().max()) > 0.1
    n16 = -(-N_AUDIO * 16000 // rate)
    stems, out_rate = repet.separate_wav_repet_periodic(str(stereo), out_rate=None, mono=True, adaptive=True, win_sec=1.5, step_sec=0.5,
                                                        period_sec=(0.2, 0.5), residual=True)
    assert out_rate == 16000 and tuple(stems.shape) == (3, n16) and bool(torch.isfinite(stems).all())
