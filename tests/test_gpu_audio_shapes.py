"""The audio ends on the GPU (csrc/glowk_audio.h through audiosourcesep_amd/audio.py) at frame counts other than the F = 64 of an
extract, over the ranges include/glowk.h documents: 1024 < n_samples < 65536 (F = 3 .. 128) for the front end, F in [1, 128] for
the NNLS, F in [2, 128] and S in [1, 16] for the masked iSTFT.  tests/test_gpu_audio.py runs all three at F = 64 only.  The audio
and the tiles are real material (tests/golden/real_audio_excerpt.npz, real_mel_tiles.npz, basis_real_tiles.npz), sliced.

Bounds and where each number comes from (all are those of tests/test_gpu_audio.py, whose header derives them as 5-10x the fp32
error of a CPU emulation of the kernels' arithmetic; none depends on F, because every STFT element is one fp32 sum of 2048 terms,
every mel band one of at most 80 and every iSTFT sample one of at most 4 x 2050, whatever the number of frames):
* front end: mel 2e-3 dB, STFT 1e-5 of max |X|, and the top_db floor exactly (test_front_end_against_the_oracle);
* NNLS against the fp64 iterate: 1e-3 per-frame relative L2 (test_nnls_against_the_oracle_iterate);
* masked iSTFT against the oracle, and reuse phase of |X|^2 against the signal: 1e-5 of the peak
  (test_istft_reuse_phase_wiener_and_length);
* bitwise: STFT frames against those of a prefix and of a shifted copy (each element is its own k-ordered MFMA chain); the NNLS
  of a slice of the frames against the slice of the NNLS (every frame's FISTA chain lives in its own registers and LDS row, so
  neither its workgroup, its slot there nor its neighbours can change a bit of it); ``invert`` against its stages."""
import os

import numpy as np
import pytest
import torch

from audiosourcesep_amd import audio
from tests import audio_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOP = 512

# n_samples -> F = 1 + n // 512: 3, 4, 4, 33, 33, 64, 65, 128, 128.  F = 33 and 65 put one frame in the last 32-frame tile of
# k_stft (f < F guards the other 31); F = 128 is the 48 KB dynamic LDS tile of k_mel_db
FRONT_LENGTHS = [1025, 1536, 2047, 16384, 16895, 32640, 33000, 65024, 65535]


def track():
    """The six real extracts end to end: 195 840 samples of 16 kHz audio in [-1, 1)."""
    return np.load(os.path.join(GOLDEN, "real_audio_excerpt.npz"))["pcm"].astype(np.float32).reshape(-1) / 32768.0


def slices(N, n):
    y = track()
    return np.stack([y[i * 26000:i * 26000 + n] for i in range(N)]).copy()


def real_tiles(N):
    """[N, 96, 64] float32 dB tiles: BASIS iterates and mixtures of real audio."""
    f = np.load(os.path.join(GOLDEN, "basis_real_tiles.npz"))
    g = np.load(os.path.join(GOLDEN, "real_mel_tiles.npz"))
    t = np.concatenate([f["x1"][[0, 7]], f["mixed"][[3]], g["gt1"][:1], f["x2"][[11, 19]]]).astype(np.float32)
    return torch.from_numpy(t[:N]).cuda()


def check_front_end(y, mel, X, top_db):
    worst_db, worst_x = 0.0, 0.0
    for i in range(len(y)):
        L, Xr = R.mel_db(y[i].astype(np.float64), top_db=top_db, return_stft=True)
        assert mel[i].shape == L.shape
        worst_db = max(worst_db, float(np.abs(mel[i] - L).max()))
        if X is not None:
            worst_x = max(worst_x, float(np.abs(X[i] - Xr).max() / max(np.abs(Xr).max(), 1e-30)))
        if top_db and mel[i].max() < 20.0:
            floor = mel[i].max() - np.float32(80.0)
            assert mel[i].min() >= floor
            active = L < L.max() - 80.0 - 0.01
            assert (mel[i][active] == floor).all()
    return worst_db, worst_x


@pytest.mark.parametrize("top_db", [80.0, None])
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("n", FRONT_LENGTHS)
def test_front_end_at_every_frame_count(n, N, top_db):
    y = slices(N, n)
    F = 1 + n // HOP
    mel, X = audio.mel_tiles(torch.from_numpy(y).cuda(), top_db=top_db, return_stft=True)
    assert tuple(mel.shape) == (N, 96, F, 1) and tuple(X.shape) == (N, 1025, F) and X.dtype == torch.complex64
    worst_db, worst_x = check_front_end(y, mel[..., 0].cpu().numpy(), X.cpu().numpy(), top_db)
    print("front end n %d (F %d), N %d, top_db %s: mel %.2e dB, STFT %.2e of max |X|" % (n, F, N, top_db, worst_db, worst_x))
    assert worst_db <= 2e-3 and worst_x <= 1e-5
    again = audio.mel_tiles(torch.from_numpy(y).cuda(), top_db=top_db, return_stft=True)
    assert torch.equal(again[0], mel) and torch.equal(torch.view_as_real(again[1]), torch.view_as_real(X))


@pytest.mark.parametrize("n", [1025, 16895, 65535])
def test_front_end_without_the_complex_stft(n):
    """Without ``return_stft`` k_stft writes |X|^2 to a scratch and k_mel_db reads that instead of squaring X."""
    y = slices(5, n)
    for top_db in (80.0, None):
        mel = audio.mel_tiles(torch.from_numpy(y).cuda(), top_db=top_db)
        worst_db, _ = check_front_end(y, mel[..., 0].cpu().numpy(), None, top_db)
        print("front end through the power scratch, n %d, top_db %s: mel %.2e dB" % (n, top_db, worst_db))
        assert worst_db <= 2e-3


def test_silence_at_128_frames_is_the_floor():
    y = np.zeros((3, 65535), np.float32)
    y[1] = slices(1, 65535)[0]
    for top_db in (80.0, None):
        mel = audio.mel_tiles(torch.from_numpy(y).cuda(), top_db=top_db)[..., 0].cpu().numpy()
        assert mel.shape == (3, 96, 128)
        assert (mel[0] == -100.0).all() and (mel[2] == -100.0).all() and mel[1].max() > -60.0


def test_stft_frames_do_not_depend_on_their_tile():
    """Frame f reads samples [512 f - 1024, 512 f + 1024) of the reflect-padded signal.  Frames whose samples lie inside both a
    signal and a prefix of it, away from the reflected ends, are the same sums in the same order: bit-identical, in whichever
    tile and column they fall.  Likewise frame f of a copy shifted by k hops and frame f + k of the signal."""
    n, m, k = 65535, 20000, 3
    y = slices(2, n)
    X = torch.view_as_real(audio.mel_tiles(torch.from_numpy(y).cuda(), return_stft=True)[1])
    P = torch.view_as_real(audio.mel_tiles(torch.from_numpy(y[:, :m].copy()).cuda(), return_stft=True)[1])
    last = (m - 1024) // HOP                                     # 37: in the second tile of both
    assert last > 32 and torch.equal(X[:, :, 2:last + 1], P[:, :, 2:last + 1])
    S = torch.view_as_real(audio.mel_tiles(torch.from_numpy(y[:, k * HOP:].copy()).cuda(), return_stft=True)[1])
    hi = (n - k * HOP - 1024) // HOP                             # the last frame of the shifted copy with no reflected sample
    assert hi > 96 and torch.equal(S[:, :, 2:hi + 1], X[:, :, 2 + k:hi + 1 + k])


@pytest.mark.parametrize("iters", [0, 1, 200])
@pytest.mark.parametrize("N", [1, 3])
def test_nnls_of_a_slice_is_the_slice_of_the_nnls(N, iters):
    """k_nnls puts 8 consecutive frames of the flattened [N * F] list in a workgroup and finds each one's tile as g / F.  With
    N = 3, F = 5 the 15 frames fill two workgroups: the first holds tile 0 and three frames of tile 1, the second is ragged
    (g < total).  F = 7 and 9 straddle likewise; at F = 8 and 64 no workgroup straddles."""
    t = real_tiles(N)
    full = audio.mel_to_power(t, iters)
    assert tuple(full.shape) == (N, 1025, 64)
    for F in (1, 5, 7, 8, 9, 63, 64):
        part = audio.mel_to_power(t[:, :, :F].contiguous(), iters)
        assert tuple(part.shape) == (N, 1025, F)
        assert torch.equal(part, full[:, :, :F]), F
    wide = torch.cat([t, real_tiles(6)[-N:]], dim=2)            # F = 128: two tiles side by side
    both = audio.mel_to_power(wide, iters)
    assert tuple(both.shape) == (N, 1025, 128)
    assert torch.equal(both[:, :, :64], full) and torch.equal(both[:, :, 64:], audio.mel_to_power(real_tiles(6)[-N:], iters))


@pytest.mark.parametrize("F", [5, 128])
def test_nnls_against_the_oracle_iterate_off_the_extract(F):
    t = real_tiles(3)
    t = torch.cat([t, real_tiles(6)[-3:]], dim=2)[:, :, :F].contiguous()
    p = audio.mel_to_power(t, iters=200).cpu().numpy()
    assert p.shape == (3, 1025, F)
    setup = R.nnls_setup()
    outside = (R.mel_filterbank() > 0).sum(axis=0) == 0
    worst = 0.0
    for i in range(3):
        ref = R.mel_to_power(t[i].cpu().numpy(), 200, setup)
        worst = max(worst, float((np.linalg.norm(p[i] - ref, axis=0) / np.linalg.norm(ref, axis=0)).max()))
    print("NNLS at F %d vs fp64 oracle: worst per-frame relative L2 %.2e" % (F, worst))
    assert worst <= 1e-3
    assert (p >= 0).all() and (p[:, outside, :] == 0).all() and outside.sum() > 0


def mixture_stft(N, F, zero_prefix=0):
    """(audio [N, n], its STFT [N, 1025, F] from the front end) at a length that gives F frames; F = 2 has none (n > 1024 gives
    F >= 3): two frames of the F = 8 spectrum."""
    n = (max(F, 3) if F > 2 else 8) * HOP - HOP + 100
    y = slices(N, n)
    y[:, :zero_prefix] = 0.0
    X = audio.mel_tiles(torch.from_numpy(y).cuda(), return_stft=True)[1]
    if F == 2:
        X = X[:, :, 3:5].contiguous()
    assert X.shape[2] == F
    return y, X


def check_masked_istft(pw, X, wiener):
    """audio.masked_istft against the oracle fed the same spectra and powers -> the worst error, relative to each signal's peak."""
    got = audio.masked_istft(pw, X, wiener=wiener)
    S, N, _, F = pw.shape
    assert tuple(got.shape) == (S, N, (F - 1) * HOP) and got.dtype == torch.float32
    assert torch.equal(got, audio.masked_istft(pw, X, wiener=wiener))
    got = got.cpu().numpy()
    Xn, pn = X.cpu().numpy().astype(np.complex128), pw.cpu().numpy().astype(np.float64)
    worst = 0.0
    for i in range(N):
        ref = R.masked_istft(list(pn[:, i]), Xn[i], wiener=wiener)
        for s in range(S):
            worst = max(worst, float(np.abs(got[s, i] - ref[s]).max() / np.abs(ref[s]).max()))
    return worst


@pytest.mark.parametrize("N", [1, 4])
@pytest.mark.parametrize("F", [2, 3, 31, 32, 33, 34, 65, 66, 127, 128])
def test_masked_istft_at_every_frame_count(F, N):
    """k_istft tiles the F - 1 hop blocks by 32: F = 34 is the first with a second tile, whose staged rows start at the frame
    before it.  S = 1 reuses the phase; S = 3 and S = 16 (the header's bound) take the Wiener sum over S planes and reuse the
    phase of every plane."""
    y, X = mixture_stft(N, F)
    p1 = (X.abs() ** 2)[None].contiguous()
    rng = np.random.default_rng(1000 * F + N)
    for S in (1, 3, 16):
        u = torch.from_numpy(rng.uniform(0.0, 1.0, (S,) + tuple(p1.shape[1:])).astype(np.float32)).cuda()
        pw = (u * p1).contiguous()
        err = check_masked_istft(pw, X, False)
        print("masked iSTFT F %d, N %d, S %d: reuse phase %.2e" % (F, N, S, err))
        assert err <= 1e-5
        if S >= 2:
            err = check_masked_istft(pw, X, True)
            print("masked iSTFT F %d, N %d, S %d: Wiener %.2e" % (F, N, S, err))
            assert err <= 1e-5
    assert check_masked_istft(p1, X, False) <= 1e-5
    if F >= 5:                                                   # below, the ends are not fully overlapped: the oracle only
        back = audio.masked_istft(p1, X).cpu().numpy()[0]
        assert np.abs(back - y[:, :(F - 1) * HOP]).max() / np.abs(y).max() <= 1e-5


def test_masked_istft_where_the_mixture_is_exactly_zero():
    """A zero prefix makes whole frames of the mixture exactly zero; with a positive power there the reused phase is
    angle(0) = 0, i.e. sqrt(x) itself (numpy's np.angle(0) = 0)."""
    y, X = mixture_stft(2, 34, zero_prefix=4096)
    assert bool((torch.view_as_real(X)[:, :, :3] == 0).all())   # frames 0 .. 2 read only zeros (and their reflection)
    rng = np.random.default_rng(8)
    u = torch.from_numpy(rng.uniform(0.0, 1.0, (3, 2, 1025, 34)).astype(np.float32)).cuda()
    pw = (u * (X.abs() ** 2)[None] + 1e-3 * u).contiguous()     # positive where X == 0
    assert check_masked_istft(pw, X, False) <= 1e-5
    assert check_masked_istft(pw, X, True) <= 1e-5


def test_invert_by_frame_is_the_composition_of_its_stages():
    y, X = mixture_stft(4, 34)
    mel = audio.mel_tiles(torch.from_numpy(y).cuda())
    t1, t2 = mel, torch.clamp(mel - 6.0, min=-100.0)
    for wiener in (False, True):
        got = audio.invert([t1, t2], X, wiener=wiener, iters=20)
        assert tuple(got.shape) == (2, 4 * 33 * HOP)
        p = audio.mel_to_power(torch.cat([t1, t2])[..., 0], 20).reshape(2, 4, 1025, 34)
        assert torch.equal(got, audio.masked_istft(p, X, wiener).reshape(2, -1))
