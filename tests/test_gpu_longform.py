"""The whole-signal path on the GPU (csrc/glowk_longform.h through ``audio.mel_frames`` / ``frame_tiles`` / ``stitch_tiles`` /
``mask_istft_long`` / ``invert_frames`` / ``separate_long`` / ``separate_wav_long``) against the restatement of tests/longform_ref.py.

Bars.  Front end: mel 2e-3 dB and STFT 1e-5 of max|X|, the bars of the per-extract front end (tests/test_gpu_audio_shapes.py),
whose arithmetic this is.  Cut: bitwise against the float32 restatement (a gather, a max, one subtraction, a clip: all exact).
Stitch: an fp32 weighted mean of K <= 64 terms with a weight table rounded to fp32 is within (2 K + 4) 2^-24 max|t| = 7.9e-6 max|t|
of the fp64 one; the bar is 2^-15 max|t| = 3.05e-5 max|t|, about four times that.  Length and alignment: 1e-5 of the peak over
every one of the n samples, the bar of the iSTFT round trips of tests/test_gpu_audio_shapes.py."""
import functools
import os
import wave

import numpy as np
import pytest
import torch

from audiosourcesep_amd import audio
from audiosourcesep_amd.config import GlowConfig
from tests import longform_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(5, 32), (64, 32), (65, 32), (100, 32), (138, 32), (138, 48), (70, 1), (138, 64)]      # (F, hop) at width 64
STITCH_BAR = 2.0 ** -15
N_LONG = 70001                                                                                   # 138 frames, 143 samples of padding


@functools.lru_cache(maxsize=None)
def track():
    """Six real extracts end to end: 195 840 samples of 16 kHz audio in [-1, 1).  Never modified."""
    y = np.load(os.path.join(GOLDEN, "real_audio_excerpt.npz"))["pcm"].astype(np.float32).reshape(-1) / 32768.0
    y.setflags(write=False)
    return y


def signals(nsig, n):
    return np.stack([track()[i * 50000:i * 50000 + n] for i in range(nsig)]).copy()


@functools.lru_cache(maxsize=None)
def reference_frames(n):
    """The restatement's (mel, STFT) of ``signals(2, n)``: computed once per length, never modified."""
    return [R.mel_frames(y, return_stft=True) for y in signals(2, n)]


# ---- mel_frames ----------------------------------------------------------------------------------------------------------------------
# F = 4 (the shortest signal), 35 (a second 32-frame STFT tile with 3 frames), 132 (past the per-extract limit of 128 frames),
# 138 from a length that is no hop multiple (zero-padded by 143 samples)
@pytest.mark.parametrize("n,F", [(1536, 4), (17408, 35), (67072, 132), (N_LONG, 138)])
def test_mel_frames_against_the_restatement(n, F):
    y = signals(2, n)
    mel, X = audio.mel_frames(y, return_stft=True)
    assert tuple(mel.shape) == (2, 96, F) and tuple(X.shape) == (2, 1025, F) and X.dtype == torch.complex64 and mel.is_cuda
    plain = audio.mel_frames(torch.from_numpy(y).cuda())                           # |X|^2 through the scratch
    mel, X, plain = mel.cpu().numpy(), X.cpu().numpy(), plain.cpu().numpy()
    for i, (L, Xr) in enumerate(reference_frames(n)):
        e_db, e_plain = float(np.abs(mel[i] - L).max()), float(np.abs(plain[i] - L).max())
        e_x = float(np.abs(X[i] - Xr).max() / np.abs(Xr).max())
        print("mel_frames n = %d (F = %d), signal %d: mel %.2e dB (%.2e without the STFT), STFT %.2e of max|X|" % (n, F, i, e_db, e_plain, e_x))
        assert e_db <= 2e-3 and e_plain <= 2e-3 and e_x <= 1e-5
    again = audio.mel_frames(y, return_stft=True)
    assert np.array_equal(again[0].cpu().numpy(), mel) and np.array_equal(again[1].cpu().numpy(), X)
    assert tuple(audio.mel_frames(y[0]).shape) == (1, 96, F)


def test_mel_frames_of_silence_and_of_one_extract():
    mel, X = audio.mel_frames(np.zeros((2, 2000), np.float32), return_stft=True)
    assert tuple(mel.shape) == (2, 96, 5) and bool((mel == -100.0).all()) and not bool(torch.view_as_real(X).any())
    y = signals(2, 32768)
    mel, X = audio.mel_frames(y, return_stft=True)
    tm, tX = audio.mel_tiles(y, top_db=None, return_stft=True)
    e_db = float((mel - tm[..., 0]).abs().max())
    e_x = float((X - tX).abs().max() / tX.abs().max())
    print("mel_frames against mel_tiles(top_db=None) at n = 32768: mel %.2e dB, STFT %.2e of max|X|" % (e_db, e_x))
    assert e_db <= 2e-3 and e_x <= 1e-5


# ---- frame_tiles ---------------------------------------------------------------------------------------------------------------------
def check_cut(F, width, hop, top_db):
    rng = np.random.default_rng(1000 * F + 10 * hop + width)
    L = rng.uniform(-110.0, 30.0, (2, 96, F)).astype(np.float32)                   # past the clip on both sides
    L[1] -= 60.0                                                                   # a quiet signal: its floor lies below -100
    tiles = audio.frame_tiles(L, width, hop, top_db)
    N = R.tile_count(F, width, hop)
    assert tuple(tiles.shape) == (2, N, 96, width, 1) and tiles.dtype == torch.float32
    tiles = tiles[..., 0].cpu().numpy()
    for i in range(2):
        want = R.cut(L[i], width, hop, top_db, dtype=np.float32)
        assert want.dtype == np.float32 and np.array_equal(tiles[i], want), (i, F, hop, top_db)
        pad = tiles[i, -1][:, F - (N - 1) * hop:]                                  # the cells past the signal's end
        floor = -100.0 if not top_db else max(np.float32(-100.0), np.maximum(L[i][:, (N - 1) * hop:].max(), np.float32(-100.0)) - np.float32(top_db))
        assert (pad == np.float32(floor)).all()
    return tiles


@pytest.mark.parametrize("top_db", [80.0, None])
@pytest.mark.parametrize("F,hop", CASES)
def test_frame_tiles_bitwise(F, hop, top_db):
    check_cut(F, 64, hop, top_db)


def test_frame_tiles_at_another_width():
    for top_db in (80.0, None):
        check_cut(100, 32, 16, top_db)
        check_cut(300, 128, 100, top_db)
    assert tuple(audio.frame_tiles(torch.zeros(96, 10)).shape) == (1, 1, 96, 64, 1)


# ---- stitch_tiles --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,hop", CASES)
def test_stitch_tiles_against_the_restatement(F, hop):
    rng = np.random.default_rng(7000 + 10 * F + hop)
    N = R.tile_count(F, 64, hop)
    t = rng.uniform(-150.0, 50.0, (3, N, 96, 64)).astype(np.float32)
    out = audio.stitch_tiles(torch.from_numpy(t).cuda()[..., None], F, hop)
    assert tuple(out.shape) == (3, 96, F)
    again = audio.stitch_tiles(t, F, hop)                                          # a second run, from the host and without the last axis
    assert torch.equal(out, again)
    out = out.cpu().numpy()
    single = R.coverage(F, N, 64, hop) == 1
    worst = 0.0
    for i in range(3):
        want = R.stitch(t[i], F, hop)
        worst = max(worst, float(np.abs(out[i] - want).max() / np.abs(t).max()))
        assert np.array_equal(out[i][:, single], want[:, single].astype(np.float32))          # copies of the one tile's value
    print("stitch F = %d, hop = %d, N = %d: %.2e of max|t| (%d frames under one tile)" % (F, hop, N, worst, int(single.sum())))
    assert worst <= STITCH_BAR
    L = rng.uniform(-100.0, 20.0, (3, 96, F)).astype(np.float32)
    back = audio.stitch_tiles(audio.frame_tiles(L, 64, hop, top_db=None), F, hop).cpu().numpy()
    err = float(np.abs(back - L).max() / np.abs(L).max())
    print("stitch(cut(L)) - L: %.2e of max|L|" % err)
    assert err <= STITCH_BAR


def test_stitch_tiles_shorter_than_the_tiles_reach():
    """F below (N - 1) hop + width: the frames past F are dropped, whatever the tiles hold there."""
    rng = np.random.default_rng(5)
    t = rng.uniform(-150.0, 50.0, (1, 4, 96, 64)).astype(np.float32)
    full = audio.stitch_tiles(t, 160, 32)
    assert torch.equal(audio.stitch_tiles(t, 138, 32), full[:, :, :138].contiguous())


# ---- length and alignment ------------------------------------------------------------------------------------------------------------
def test_the_mixtures_own_power_gives_the_signal_back_sample_for_sample():
    y = signals(2, N_LONG)
    _, X = audio.mel_frames(y, return_stft=True)
    mono = audio.mask_istft_long((X[0].abs() ** 2)[None], X[0], N_LONG)
    assert tuple(mono.shape) == (1, N_LONG)
    mono = mono.cpu().numpy()[0]
    peak = float(np.abs(y[0]).max())
    err = float(np.abs(mono - y[0]).max() / peak)
    slipped = float(np.abs(mono[1:] - y[0][:-1]).max() / peak)
    print("mono reuse-phase at n = %d: %.2e of the peak over all samples (one sample late: %.2e)" % (N_LONG, err, slipped))
    assert err <= 1e-5 and slipped > 1e-3                                          # a displaced output could not pass
    stereo = audio.mask_istft_long((X.abs() ** 2).mean(0)[None], X, N_LONG, em_iter=0)
    assert tuple(stereo.shape) == (1, 2, N_LONG)
    err = float(np.abs(stereo.cpu().numpy()[0] - y).max() / np.abs(y).max())
    print("stereo, em_iter = 0, one source: %.2e of the peak" % err)
    assert err <= 1e-5


def test_wiener_inversion_against_the_restatement():
    rng = np.random.default_rng(11)
    _, Xr = reference_frames(N_LONG)[0]
    X = Xr.astype(np.complex64)
    m = rng.uniform(0.0, 1.0, Xr.shape)
    p = np.stack([m * np.abs(X) ** 2, (1.0 - m) * np.abs(X) ** 2]).astype(np.float32)
    for wiener in (True, False):
        got = audio.mask_istft_long(p, X, N_LONG, wiener=wiener).cpu().numpy()
        want = R.mask_istft(p, X.astype(np.complex128), N_LONG, wiener)
        assert got.shape == want.shape == (2, N_LONG)
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print("mask_istft_long, wiener = %s: %.2e of max|ref|" % (wiener, err))
        assert err <= 1e-5
    # invert_frames is mel_to_power on tiles of <= 128 frames, then the same last stage: F = 138 goes through as 2 tiles of 69
    L = torch.from_numpy(np.stack([reference_frames(N_LONG)[i][0] for i in range(2)]).astype(np.float32))
    ys = audio.invert_frames(L, X, N_LONG, wiener=True, iters=20)
    pw = torch.cat([audio.mel_to_power(L[:, :, :69], 20), audio.mel_to_power(L[:, :, 69:], 20)], dim=2)
    assert tuple(ys.shape) == (2, N_LONG) and torch.equal(ys, audio.mask_istft_long(pw, X, N_LONG, wiener=True))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flows():
    """Two tiny calibrated K = 1 priors of tile shape [96, 64, 1], as tests/test_gpu_stereo.py builds its own."""
    from audiosourcesep_amd.flow_models.flow_glow import GlowFlow
    from audiosourcesep_amd.synthetic import calibrated_engine
    cfg = GlowConfig(H=96, W=64, C=1, L=2, K=1, F=128)
    return [GlowFlow(calibrated_engine(cfg, device=0, init_tiles=8, seed=50 + k)[0]) for k in range(2)]


SIGMAS = np.array([20.0, 5.0], np.float32)
KW = dict(T=2, delta=1e-4, seed=9, iters=20)


def test_separate_long_end_to_end(flows):
    y = signals(2, N_LONG)
    ys, mixed, src = audio.separate_long(y[0], flows, SIGMAS, **KW)
    assert tuple(ys.shape) == (2, N_LONG) and tuple(mixed.shape) == (96, 138) and tuple(src.shape) == (2, 96, 138)
    assert bool(torch.isfinite(ys).all()) and bool(torch.isfinite(src).all()) and float(ys.abs().max()) > 0
    assert torch.equal(mixed, audio.mel_frames(y[0], return_stft=True)[0][0])
    ys2, mixed2, src2 = audio.separate_long(torch.from_numpy(y[0]), flows, SIGMAS, **KW)
    assert torch.equal(ys, ys2) and torch.equal(src, src2) and torch.equal(mixed, mixed2)
    ys3, _, src3 = audio.separate_long(y[0], flows, SIGMAS, tile_hop=64, **KW)          # disjoint tiles: every frame under one tile
    assert tuple(ys3.shape) == (2, N_LONG) and tuple(src3.shape) == (2, 96, 138) and bool(torch.isfinite(ys3).all())
    assert not torch.equal(src3, src)
    st, smixed, ssrc = audio.separate_long(y, flows, SIGMAS, **KW)
    assert tuple(st.shape) == (2, 2, N_LONG) and bool(torch.isfinite(st).all()) and tuple(ssrc.shape) == (2, 96, 138)
    down = (torch.from_numpy(y[0]) + torch.from_numpy(y[1])) / 2
    assert torch.equal(smixed, audio.mel_frames(down, return_stft=True)[0][0])                  # the priors see the downmix


def write_wav16(path, y, rate):
    q = np.rint(np.clip(np.atleast_2d(y), -1.0, 1.0) * 32767.0).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(q.shape[0])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(q.T).tobytes())


def test_separate_wav_long_returns_the_files_length(flows, tmp_path):
    n, rate = 37485, 22050
    rng = np.random.default_rng(3)
    t = np.arange(n) / rate
    a, b = 0.3 * np.sin(2 * np.pi * 440.0 * t), 0.2 * np.sin(2 * np.pi * (200.0 * t + 900.0 * t * t))
    y = np.stack([0.9 * a + 0.2 * b, 0.3 * a + 0.8 * b]) + 0.01 * rng.standard_normal((2, n))
    mono, stereo = tmp_path / "mono.wav", tmp_path / "stereo.wav"
    write_wav16(mono, y[0], rate)
    write_wav16(stereo, y, rate)
    ys, mixed, src, out_rate = audio.separate_wav_long(str(mono), flows, SIGMAS, **KW)
    F = 1 + -(-27200 // 512)                                                       # 37 485 samples at 22 050 Hz are 27 200 at 16 kHz
    assert out_rate == rate and tuple(ys.shape) == (2, n) and bool(torch.isfinite(ys).all())
    assert tuple(mixed.shape) == (96, F) and tuple(src.shape) == (2, 96, F)
    ys2, _, _, out_rate = audio.separate_wav_long(str(stereo), flows, SIGMAS, **KW)
    assert out_rate == rate and tuple(ys2.shape) == (2, 2, n) and bool(torch.isfinite(ys2).all())
    ym, _, _, out_rate = audio.separate_wav_long(str(stereo), flows, SIGMAS, out_rate=None, mono=True, **KW)
    assert out_rate == 16000 and tuple(ym.shape) == (2, 27200)
