"""REPET's front end without a GPU: the restatement of tests/repet_beat_ref.py against an independent FFT autocorrelation, the
planted periods, the neighbour order on hand-checked cases, the Python argument checks of ``audiosourcesep_amd.repet`` (refused
with ValueError before the library is loaded), the boundary of the C entries (declared, exported, bound; every refusal before any
device call), and the index rule the kernel shares with the host under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, repet
from tests import repet_beat_ref as B

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def test_the_restatement_against_an_fft_autocorrelation():
    """Wiener-Khinchin with zero padding to 2 F: irfft(|rfft(P)|^2)[l] is the lag-l autocorrelation of every row."""
    rng = np.random.default_rng(3)
    S = (np.abs(rng.standard_normal((17, 75))) ** 2).astype(np.float32)
    rows, F = S.shape
    P = S.astype(np.float64) ** 2
    acf = np.fft.irfft(np.abs(np.fft.rfft(P, 2 * F, axis=1)) ** 2, 2 * F, axis=1)[:, :F].sum(0)
    raw = acf / (rows * (F - np.arange(F)))
    want = raw / raw[0]
    got = B.beat_spectrum(S, F)
    # the FFT's error is relative to lag 0 (about 2e-16 F log F of acf[0]); the late lags average few pairs of comparable size
    assert got.shape == (F,) and got[0] == 1.0 and np.abs(got - want).max() <= 1e-12 * want.max()
    assert np.array_equal(B.beat_spectrum(S, 20), got[:20])
    assert np.array_equal(B.beat_spectrum(np.stack([S, 2 * S]), 9)[1], B.beat_spectrum(2 * S, 9))
    assert not B.beat_spectrum(np.zeros((3, 8), np.float32), 8).any()              # a silent signal: all zeros
    # one window that covers the signal is the beat spectrum; windows are clipped at both ends
    assert B.windows(10, 0, 0) == [(0, 10)]
    assert B.windows(10, 4, 3) == [(0, 2), (1, 4), (4, 4), (7, 3)]
    assert B.windows(7, 7, 1)[3] == (0, 7) and B.windows(7, 7, 1)[0] == (0, 4) and B.windows(7, 7, 1)[6] == (3, 4)
    assert np.array_equal(B.beat_spectrogram(S, 30, F, 1)[F // 2], B.beat_spectrum(S, 30))
    short = B.beat_spectrogram(S, 6, 4, 3)
    assert short.shape == (25, 6) and not short[:, 4:].any() and not short[0, 2:].any() and short[0, 1] > 0


@pytest.mark.parametrize("case", B.PLANTED, ids=lambda c: "-".join(map(str, c)))
def test_the_planted_period_is_found(case):
    rows, patterns = case[0], case[1]
    S, pmin, pmax = B.planted_case(case)
    assert [m for m in range(pmin, pmax + 1) if m % patterns == 0] == [patterns]   # exactly one multiple: b[p] and b[2 p] nearly tie
    beat = B.beat_spectrum(S, pmax + 1)
    best, margin = B.best_and_second(beat, pmin, pmax)
    print("planted %s: range [%d, %d], best lag %d, %.3f above the second; 100 bars = %.3e" % (case, pmin, pmax, best, margin, 100 * B.bar(rows)))
    assert best == patterns == int(B.find_period(beat, pmin, pmax))
    assert margin >= 0.5 and margin > 100 * B.bar(rows) * beat[best]


def test_the_period_rule_on_ties():
    assert int(B.find_period(np.ones(9), 2, 7)) == 2 and int(B.find_period(np.zeros(9), 3, 8)) == 3
    assert int(B.find_period(np.array([1.0, 0.0, 0.5, 0.7, 0.7, 0.2]), 1, 5)) == 3
    assert B.find_period(np.array([[0.0, 1.0, 2.0, 2.0], [0.0, 3.0, 1.0, 3.0]]), 1, 3).tolist() == [2, 1]
    assert int(B.find_period(np.array([1.0, 0.9, 0.1, 0.9]), 2, 3)) == 3          # lag 1 is outside the range


def test_the_neighbour_order_on_hand_checked_cases():
    nb = lambda p, frames, k, step=None: B.period_neighbors(np.asarray(p), frames, k, step)
    idx = nb(3, 10, 4)                                                             # 10 frames, period 3: 4, 3, 3 congruent frames
    assert idx[4].tolist() == [4, 1, 7, -1] and idx[0].tolist() == [0, 3, 6, 9] and idx[9].tolist() == [9, 6, 3, 0]
    assert idx[5].tolist() == [5, 2, 8, -1] and idx[3].tolist() == [3, 0, 6, 9]
    idx = nb(3, 10, 3)                                                             # k at the congruent count of classes 1 and 2
    assert idx[4].tolist() == [4, 1, 7] and idx[0].tolist() == [0, 3, 6] and idx[9].tolist() == [9, 6, 3] and idx[6].tolist() == [6, 3, 9]
    idx = nb(3, 10, 2)                                                             # below it: the nearest, the earlier of two first
    assert idx[4].tolist() == [4, 1] and idx[0].tolist() == [0, 3] and idx[9].tolist() == [9, 6]
    assert nb(3, 10, 1)[:, 0].tolist() == list(range(10))
    for p in (10, 11, 1000):                                                       # p >= frames: only the frame itself
        idx = nb(p, 10, 3)
        assert idx[:, 0].tolist() == list(range(10)) and (idx[:, 1:] == -1).all()
    for p in (0, -5):                                                              # clamped to 1
        assert np.array_equal(nb(p, 6, 4), nb(1, 6, 4))
    assert nb(1, 6, 4)[2].tolist() == [2, 1, 3, 0] and nb(1, 6, 4)[5].tolist() == [5, 4, 3, 2]
    # one period per window: frame j uses entry min((j + step // 2) // step, nper - 1)
    idx = nb([2, 3, 0], 11, 3, 4)                                                  # frames 0-1: 2; 2-5: 3; 6-10: max(1, 0) = 1
    assert idx[1].tolist() == [1, 3, 5] and idx[2].tolist() == [2, 5, 8] and idx[5].tolist() == [5, 2, 8]
    assert idx[6].tolist() == [6, 5, 7] and idx[10].tolist() == [10, 9, 8]
    idx = nb([[2, 5], [4, 1]], 9, 2, 7)                                            # a batch; the last entry serves the frames past it
    assert idx.shape == (2, 9, 2) and idx[0, 3].tolist() == [3, 1] and idx[0, 4].tolist() == [4, -1] and idx[0, 8].tolist() == [8, 3]
    assert idx[1, 3].tolist() == [3, 7] and idx[1, 4].tolist() == [4, 3]


def test_bad_arguments_are_refused_before_the_library_loads(monkeypatch, tmp_path):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "_lib", None)
    S, y = np.zeros((12, 30), np.float32), np.zeros(4096, np.float32)
    beat = np.zeros((3, 16), np.float32)
    wav = tmp_path / "none.wav"                                                     # never opened: the arguments are checked first
    bad = [
        lambda: repet.beat_spectrum(S, nlags=0),
        lambda: repet.beat_spectrum(S, nlags=31),
        lambda: repet.beat_spectrum(S, nlags=4.0),
        lambda: repet.beat_spectrum(S, nlags=True),
        lambda: repet.beat_spectrum(S[0]),
        lambda: repet.beat_spectrum(S.astype(np.complex64)),
        lambda: repet.beat_spectrum(np.zeros((4097, 2), np.float32)),
        lambda: repet.beat_spectrum(torch.zeros(1, 32769)),
        lambda: repet.beat_spectrogram(S, 0),
        lambda: repet.beat_spectrogram(S, 1),
        lambda: repet.beat_spectrogram(S, 31),
        lambda: repet.beat_spectrogram(S, 8.0),
        lambda: repet.beat_spectrogram(S, True),
        lambda: repet.beat_spectrogram(S, None),
        lambda: repet.beat_spectrogram(S, 8, step=0),
        lambda: repet.beat_spectrogram(S, 8, step=9),
        lambda: repet.beat_spectrogram(S, 8, step=2.0),
        lambda: repet.beat_spectrogram(S, 8, nlags=0),
        lambda: repet.beat_spectrogram(S, 8, nlags=31),
        lambda: repet.beat_spectrogram(S.astype(np.complex64), 8),
        lambda: repet.beat_spectrogram(np.zeros((3, 1), np.float32), 2),
        lambda: repet.find_period(beat, 0, 5),
        lambda: repet.find_period(beat, 6, 5),
        lambda: repet.find_period(beat, 1, 16),
        lambda: repet.find_period(beat, 1.0, 5),
        lambda: repet.find_period(beat, True, 5),
        lambda: repet.find_period(beat[:, :1], 1, 1),
        lambda: repet.find_period(np.zeros((), np.float32), 1, 1),
        lambda: repet.find_period(beat.astype(np.int32), 1, 5),
        lambda: repet.find_period(beat.astype(np.complex64), 1, 5),
        lambda: repet.period_neighbors(3, 0, 4),
        lambda: repet.period_neighbors(3, 32769, 4),
        lambda: repet.period_neighbors(3, 10, 0),
        lambda: repet.period_neighbors(3, 10, 513),
        lambda: repet.period_neighbors(3, 10, 4.0),
        lambda: repet.period_neighbors(3.0, 10, 4),
        lambda: repet.period_neighbors(True, 10, 4),
        lambda: repet.period_neighbors(np.array([2.0, 3.0]), 10, 4),
        lambda: repet.period_neighbors(3, 10, 4, step=0),
        lambda: repet.period_neighbors(3, 10, 4, step=2),                           # with step the periods are [.., nper]
        lambda: repet.period_neighbors(np.array([3, 4]), 10, 4, step=2.0),
        lambda: repet.period_neighbors(np.zeros((65536,), np.int32), 10, 4),
        lambda: repet.period_neighbors(np.zeros((2, 0), np.int32), 10, 4, step=2),
    ]
    for f in (repet.repet, lambda S, **kw: repet.repet_adaptive(S, 12, **kw)):
        bad += [
            lambda f=f: f(S, margin=0.5),
            lambda f=f: f(S, margin=(1.0, 0.99)),
            lambda f=f: f(S, margin=(2.0,)),
            lambda f=f: f(S, margin="2"),
            lambda f=f: f(S, power=0),
            lambda f=f: f(S, power=None),
            lambda f=f: f(S, mask=1),
            lambda f=f: f(S, return_period="yes"),
            lambda f=f: f(S, period_range=(0, 5)),
            lambda f=f: f(S, period_range=(6, 5)),
            lambda f=f: f(S, period_range=(2, 30)),
            lambda f=f: f(S, period_range=(2.0, 5)),
            lambda f=f: f(S, period_range=(2, True)),
            lambda f=f: f(S, period_range=5),
            lambda f=f: f(S, period_range=(2, 5, 7)),
            lambda f=f: f(S[0]),
            lambda f=f: f(np.zeros((4097, 40), np.float32)),
        ]
    bad += [
        lambda: repet.repet(S[:, :5]),                                             # the default range (2, F // 3) is empty
        lambda: repet.repet(S, k=0),
        lambda: repet.repet(S, k=513),
        lambda: repet.repet(S, k=4.0),
        lambda: repet.repet(S, period=0),
        lambda: repet.repet(S, period=2.5),
        lambda: repet.repet(S, period=True),
        lambda: repet.repet(S, period=np.array([3, 4])),                           # one signal, two periods
        lambda: repet.repet(S, period=5, period_range=(2, 9)),
        lambda: repet.repet_adaptive(S, 1),
        lambda: repet.repet_adaptive(S, 31),
        lambda: repet.repet_adaptive(S, 8.0),
        lambda: repet.repet_adaptive(S, 5),                                        # the default range (2, win // 3) is empty
        lambda: repet.repet_adaptive(S, 12, step=0),
        lambda: repet.repet_adaptive(S, 12, step=13),
        lambda: repet.repet_adaptive(S, 12, order=0),
        lambda: repet.repet_adaptive(S, 12, order=513),
        lambda: repet.repet_adaptive(S, 12, order=True),
        lambda: repet.repet_adaptive(S, 12, period_range=(2, 12)),                 # pmax <= win - 1
        lambda: repet.repet_audio(y[:1024]),
        lambda: repet.repet_audio(np.zeros((2, 3, 4096), np.float32)),
        lambda: repet.repet_audio(y.astype(np.complex64)),
        lambda: repet.repet_audio(y),                                              # 9 frames: 0.8 s is more than a third of them
        lambda: repet.repet_audio(y, adaptive=1),
        lambda: repet.repet_audio(y, period_sec=0.5),
        lambda: repet.repet_audio(y, period_sec=(0.0, 1.0)),
        lambda: repet.repet_audio(y, period_sec=(1.0, 0.5)),
        lambda: repet.repet_audio(y, period_sec=(0.5, float("nan"))),
        lambda: repet.repet_audio(y, period_sec=(0.07, 0.09)),                     # no whole frame count in between
        lambda: repet.repet_audio(y, period_sec=(0.05, 1e6)),
        lambda: repet.repet_audio(y, period_sec=(0.05, 0.1), adaptive=True, win_sec=0.0),
        lambda: repet.repet_audio(y, period_sec=(0.05, 0.1), adaptive=True, win_sec=1.0, step_sec=2.0),
        lambda: repet.repet_audio(y, period_sec=(0.05, 0.1), adaptive=True, step_sec=-1.0),
        lambda: repet.repet_audio(y, period_sec=(0.05, 0.1), win_sec="10"),
        lambda: repet.repet_audio(y, period_sec=(0.05, 0.1), order=0),
        lambda: repet.repet_audio(y, period_sec=(0.05, 0.1), cutoff_hz=-1.0),
        lambda: repet.repet_audio(y, period_sec=(0.05, 0.1), cutoff_hz=9000.0),
        lambda: repet.repet_audio(y, period_sec=(0.05, 0.1), cutoff_hz=None),
        lambda: repet.repet_audio(y, period_sec=(0.05, 0.1), margin=0.0),
        lambda: repet.repet_audio(y, period_sec=(0.05, 0.1), power=0.0),
        lambda: repet.repet_audio(y, period_sec=(0.05, 0.1), residual="yes"),
        lambda: repet.separate_wav_repet_periodic(str(wav), out_rate="native"),
        lambda: repet.separate_wav_repet_periodic(str(wav), out_rate=10),
        lambda: repet.separate_wav_repet_periodic(str(wav), mono="yes"),
        lambda: repet.separate_wav_repet_periodic(str(wav), order=0),
        lambda: repet.separate_wav_repet_periodic(str(wav), margin=0.5),
        lambda: repet.separate_wav_repet_periodic(str(wav), period_sec=(2.0, 1.0)),
        lambda: repet.separate_wav_repet_periodic(str(wav), width_sec=2.0),        # repet_sim_audio's, not repet_audio's
        lambda: repet.separate_wav_repet_periodic(str(wav), k=8),
        lambda: repet.separate_wav_repet_periodic(str(wav), kernel_size=31),
    ]
    for n, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % n)
    with pytest.raises(TypeError):
        repet.repet(S, kernel_size=31)                                            # an unknown keyword of a plain function


PROTOTYPES = (
    "size_t glowk_beat_workspace_bytes(int nsig, int rows, int frames, int nlags, int win, int step);",
    "int glowk_beat_spectrum(const float* s_dev, int nsig, int rows, int frames, int nlags, int win, int step,\n"
    "                        float* beat_dev /* [nsig][nwin][nlags] */, void* work_dev, size_t work_bytes, void* stream);",
    "int glowk_beat_period(const float* beat_dev /* [nseg][nlags] */, int nseg, int nlags, int pmin, int pmax,\n"
    "                      int32_t* period_dev /* [nseg] */, void* stream);",
    "int glowk_period_neighbors(const int32_t* period_dev /* [nsig][nper] */, int nsig, int frames, int nper, int step, int k,\n"
    "                           int32_t* idx_dev /* [nsig][frames][k] */, void* stream);",
)


def test_the_entries_are_declared_exported_and_bound(lib, repo_root):
    text = open(os.path.join(repo_root, "include", "glowk.h")).read()
    for proto in PROTOTYPES:
        assert proto in text, proto
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert _lib.SYMBOLS["glowk_beat_workspace_bytes"] == (sz, [i, i, i, i, i, i])
    assert _lib.SYMBOLS["glowk_beat_spectrum"] == (i, [vp, i, i, i, i, i, i, vp, vp, sz, vp])
    assert _lib.SYMBOLS["glowk_beat_period"] == (i, [vp, i, i, i, i, vp, vp])
    assert _lib.SYMBOLS["glowk_period_neighbors"] == (i, [vp, i, i, i, i, i, vp, vp])
    for name in ("glowk_beat_workspace_bytes", "glowk_beat_spectrum", "glowk_beat_period", "glowk_period_neighbors"):
        assert getattr(lib, name) is not None
    version = int(re.search(r"#define GLOWK_VERSION (\d+)", text).group(1))
    assert lib.glowk_version() == version >= 530                                  # (the version that introduced them)
    assert "Since version 530" in text


def _err(lib):
    return lib.glowk_last_error().decode()


def test_the_workspace_stays_far_below_a_gram_matrix(lib):
    ws = lib.glowk_beat_workspace_bytes
    for nsig, rows, F, nlags, win, step in [(1, 1, 1, 1, 0, 0), (1, 1025, 5626, 251, 0, 0), (1, 1025, 5626, 5626, 0, 0), (3, 33, 95, 95, 0, 0),
                                            (1, 1025, 5626, 105, 312, 156), (2, 96, 32768, 32768, 0, 0), (1, 4096, 66, 66, 33, 33)]:
        got = ws(nsig, rows, F, nlags, win, step)
        assert got > 0 and got % 768 == 0, (nsig, rows, F, nlags, win, step)
        assert ws(2 * nsig, rows, F, nlags, win, step) == 2 * got                   # a batch is its signals side by side
    full = 4 * 5626 * 5626                                                          # the fp32 Gram matrix of 180 s of audio
    assert ws(1, 1025, 5626, 5626, 0, 0) <= full // 32 and ws(1, 1025, 5626, 251, 0, 0) <= full // 512
    assert ws(1, 96, 32768, 32768, 0, 0) <= 4 * 32768 * 32768 // 256
    for args in [(-1, 12, 30, 8, 0, 0), (65536, 12, 30, 8, 0, 0), (1, 0, 30, 8, 0, 0), (1, 4097, 30, 8, 0, 0), (1, 12, 0, 1, 0, 0),
                 (1, 12, 32769, 8, 0, 0), (1, 12, 30, 0, 0, 0), (1, 12, 30, 31, 0, 0), (1, 12, 30, 8, 1, 1), (1, 12, 30, 8, 31, 1),
                 (1, 12, 30, 8, -2, 1), (1, 12, 30, 8, 8, 0), (1, 12, 30, 8, 8, 9), (16, 4096, 32768, 8, 0, 0),
                 (65535, 1, 32768, 2, 2, 1)]:
        assert ws(*args) == 0, args
    assert ws(0, 12, 30, 8, 0, 0) == 0                                              # no signals need no workspace


def test_the_entries_refuse_bad_arguments_before_touching_a_device(lib):
    z, a, b, c, w = (ctypes.c_void_p(v) for v in (0, 1 << 20, 1 << 30, 1 << 31, 1 << 32))   # never dereferenced: refused first
    big = 1 << 40

    def bs(nsig=1, rows=12, F=30, nlags=8, win=0, step=0, s=a, beat=b, work=w, nbytes=big):
        return lib.glowk_beat_spectrum(s, nsig, rows, F, nlags, win, step, beat, work, nbytes, z)

    def bp(nseg=3, nlags=16, pmin=2, pmax=9, beat=a, period=b):
        return lib.glowk_beat_period(beat, nseg, nlags, pmin, pmax, period, z)

    def pn(nsig=1, F=30, nper=1, step=1, k=4, period=a, idx=b):
        return lib.glowk_period_neighbors(period, nsig, F, nper, step, k, idx, z)

    for kw, word in [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(rows=0), "rows"), (dict(rows=4097), "rows"), (dict(F=0), "frames"),
                     (dict(F=32769), "frames"), (dict(nlags=0), "nlags"), (dict(nlags=31), "nlags"), (dict(nlags=-3), "nlags"),
                     (dict(win=1, step=1), "win"), (dict(win=31, step=1), "win"), (dict(win=-8, step=1), "win"), (dict(win=8, step=0), "step"),
                     (dict(win=8, step=9), "step"), (dict(win=8, step=-1), "step"), (dict(nsig=16, rows=4096, F=32768), "2^31"),
                     (dict(nsig=65535, rows=1, F=32768, nlags=2, win=2, step=1), "2^31")]:
        assert bs(**kw) == _lib.ERR and word in _err(lib), kw
    assert bs() == _lib.ERR and "device memory" in _err(lib)                       # valid ranges reach the pointer check
    assert bs(nlags=30, win=30, step=30) == _lib.ERR and "device memory" in _err(lib)
    assert bs(nlags=1, win=2, step=1) == _lib.ERR and "device memory" in _err(lib)
    assert bs(nsig=0, s=z, beat=z, work=z, nbytes=0) == _lib.OK                     # no signals: a successful no-op ...
    assert bs(nsig=0, nlags=0, s=z, beat=z, work=z, nbytes=0) == _lib.ERR           # ... of valid arguments only
    assert bs(nsig=0, win=8, step=0, s=z, beat=z, work=z, nbytes=0) == _lib.ERR
    for kw in (dict(s=z), dict(beat=z), dict(work=z)):
        assert bs(**kw) == _lib.ERR and "null" in _err(lib), kw
    need = lib.glowk_beat_workspace_bytes(1, 12, 30, 8, 0, 0)
    assert need > 0
    assert bs(nbytes=need - 1) == _lib.ERR and "work_bytes" in _err(lib)
    assert bs(nbytes=0) == _lib.ERR and "work_bytes" in _err(lib)
    assert bs(nbytes=need) == _lib.ERR and "device memory" in _err(lib)            # exactly enough passes this check
    assert bs(work=ctypes.c_void_p((1 << 32) + 4)) == _lib.ERR and "aligned" in _err(lib)
    assert bs(beat=a) == _lib.ERR and "overlap" in _err(lib)
    assert bs(beat=ctypes.c_void_p((1 << 20) + 4 * 359)) == _lib.ERR and "overlap" in _err(lib)
    assert bs(beat=ctypes.c_void_p((1 << 20) - 4 * 7)) == _lib.ERR and "overlap" in _err(lib)
    assert bs(work=a) == _lib.ERR and "work_dev" in _err(lib)
    assert bs(work=b) == _lib.ERR and "work_dev" in _err(lib)

    for kw, word in [(dict(nseg=-1), "nseg"), (dict(nlags=1, pmin=1, pmax=1), "nlags"), (dict(nlags=32769), "nlags"), (dict(pmin=0), "pmin"),
                     (dict(pmin=10), "pmin"), (dict(pmax=16), "pmax"), (dict(nseg=1 << 20, nlags=4096), "2^31")]:
        assert bp(**kw) == _lib.ERR and word in _err(lib), kw
    assert bp() == _lib.ERR and "device memory" in _err(lib)
    assert bp(nlags=2, pmin=1, pmax=1) == _lib.ERR and "device memory" in _err(lib)
    assert bp(nseg=0, beat=z, period=z) == _lib.OK and bp(nseg=0, pmin=0, beat=z, period=z) == _lib.ERR
    for kw in (dict(beat=z), dict(period=z)):
        assert bp(**kw) == _lib.ERR and "null" in _err(lib), kw
    assert bp(period=ctypes.c_void_p((1 << 20) + 64)) == _lib.ERR and "overlap" in _err(lib)

    for kw, word in [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(F=0), "frames"), (dict(F=32769), "frames"), (dict(nper=0), "nper"),
                     (dict(nper=32769), "nper"), (dict(step=0), "step"), (dict(step=32769), "step"), (dict(k=0), "k must"), (dict(k=513), "k must"),
                     (dict(nsig=4096, F=32768, k=512), "2^31")]:
        assert pn(**kw) == _lib.ERR and word in _err(lib), kw
    assert pn() == _lib.ERR and "device memory" in _err(lib)
    assert pn(nper=32768, step=32768, k=512, F=32768) == _lib.ERR and "device memory" in _err(lib)
    assert pn(nsig=0, period=z, idx=z) == _lib.OK and pn(nsig=0, k=0, period=z, idx=z) == _lib.ERR
    for kw in (dict(period=z), dict(idx=z)):
        assert pn(**kw) == _lib.ERR and "null" in _err(lib), kw
    assert pn(idx=a) == _lib.ERR and "overlap" in _err(lib)
    # a host pointer is refused (where there is no device at all, every pointer is one)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    host, beat, work = np.zeros(12 * 30, np.float32), np.zeros(16 * 3, np.float32), np.zeros(need // 8 + 1, np.float64)
    per, idx = np.zeros(3, np.int32), np.zeros(30 * 4, np.int32)
    assert bs(s=p(host), beat=p(beat), work=p(work), nbytes=work.nbytes) == _lib.ERR and "device memory" in _err(lib)
    assert bp(beat=p(beat), period=p(per)) == _lib.ERR and "device memory" in _err(lib)
    assert pn(period=p(per), idx=p(idx)) == _lib.ERR and "device memory" in _err(lib)


def test_the_index_rule_under_address_and_ub_sanitizers(tmp_path):
    """glowk_beat_index.h -- the functions k_period_neighbors, k_beat_gram and k_beat_reduce call -- compiled without HIP into a
    stand-alone program with its own main (tests/beat_index_sanitize_main.cpp) and swept against straightforward loops."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "beat_index_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "beat_index_sanitize_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "BEAT_INDEX_SANITIZE_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
