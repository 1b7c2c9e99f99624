"""CPU checks of the audio ends (audiosourcesep_amd/audio.py, csrc/glowk_audio.h): the fp64 oracle against known values and
against scipy, the committed tiles' per-extract floor, extracts and wav I/O, and the argument validation of the three entry
points (no GPU: every call here is refused before any device call)."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, audio
from tests import audio_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_mel_scale_known_values():
    assert abs(float(R.hz_to_mel(1000.0)) - 15.0) < 1e-12
    assert abs(float(R.hz_to_mel(125.0)) - 1.875) < 1e-12
    for f in (60.0, 125.0, 999.0, 1000.0, 4000.0, 7600.0):
        assert abs(float(R.mel_to_hz(R.hz_to_mel(f))) - f) < 1e-9 * f


def test_oracle_istft_inverts_stft():
    rng = np.random.default_rng(0)
    y = rng.standard_normal(R.EXTRACT)
    X = R.stft(y)
    assert X.shape == (1025, 64)
    z = R.istft(X)
    assert z.shape == (32256,)
    assert np.abs(z - y[:32256]).max() < 1e-12


def test_oracle_fista_against_scipy_nnls():
    scipy_opt = pytest.importorskip("scipy.optimize")
    f = np.load(os.path.join(GOLDEN, "basis_real_tiles.npz"))
    setup = R.nnls_setup()
    A = setup[0]
    excess = []
    for key in ("x1", "x2", "mixed"):
        for i in range(6):
            b = 10.0 ** (f[key][5 * i].astype(np.float64) / 10.0)
            x = R.fista_nnls(b, 200, setup)
            assert (x >= 0).all()
            for j in range(0, 64, 8):
                xs, _ = scipy_opt.nnls(A, b[:, j], maxiter=50 * 1025)
                nb = np.linalg.norm(b[:, j])
                excess.append((np.linalg.norm(A @ x[:, j] - b[:, j]) - np.linalg.norm(A @ xs - b[:, j])) / nb)
    excess = np.array(excess)
    assert np.median(excess) <= 1e-4 and excess.max() <= 2e-2, (np.median(excess), excess.max())


def test_golden_tiles_carry_the_per_extract_floor():
    """power_to_db(top_db=80) per extract: min == max - 80 in every gt tile (exact in the reference's float32; the committed
    tiles are float16, 0.06 dB resolution at these magnitudes)."""
    f = np.load(os.path.join(GOLDEN, "basis_real_tiles.npz"))
    for key in ("gt1", "gt2"):
        t = f[key].astype(np.float64)
        gap = t.max(axis=(1, 2)) - t.min(axis=(1, 2))
        assert np.abs(gap - 80.0).max() <= 0.07, (key, gap)


def test_extracts_drop_the_remainder_and_skip():
    y = np.arange(5 * audio.EXTRACT + 100, dtype=np.float32)
    e = audio.extracts(y)
    assert tuple(e.shape) == (5, 32640) and float(e[1, 0]) == 32640.0
    e = audio.extracts(y, skip=2)
    assert tuple(e.shape) == (3, 32640) and float(e[0, 0]) == 2 * 32640.0
    e = audio.extracts(y, skip=2, n=2)
    assert tuple(e.shape) == (2, 32640) and float(e[-1, -1]) == 4 * 32640.0 - 1
    assert tuple(audio.extracts(y, skip=7).shape) == (0, 32640)


def test_wav_round_trip_and_rate(tmp_path):
    rng = np.random.default_rng(1)
    y = (rng.uniform(-0.5, 0.5, 20000)).astype(np.float32)
    p = tmp_path / "a.wav"
    audio.write_wav(p, y)
    z = audio.read_wav(p)
    assert z.dtype == np.float32 and z.shape == y.shape
    assert np.abs(z - y).max() <= 1.0 / 32768
    st = tmp_path / "st.wav"                         # stereo is averaged to mono
    with wave.open(str(st), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.array([[1000, 3000], [-2000, 0]], dtype="<i2").tobytes())
    np.testing.assert_array_equal(audio.read_wav(st), np.array([2000, -1000], np.float32) / 32768)
    q = tmp_path / "b.wav"
    with wave.open(str(q), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(44100)
        w.writeframes(np.zeros(10, "<i2").tobytes())
    with pytest.raises(ValueError, match="44100"):
        audio.read_wav(q)
    with pytest.raises(ValueError):
        audio.write_wav(q, y, sr=44100)


def test_golden_excerpt_and_shipped_length():
    g = np.load(os.path.join(GOLDEN, "real_audio_excerpt.npz"))
    assert g["pcm"].shape == (6, 32640) and g["pcm"].dtype == np.int16
    assert int(g["source_frames"]) == 967680 == 30 * 32256        # 30 tiles, (64 - 1) * 512 samples each


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def _err(lib):
    return lib.glowk_last_error().decode()


def test_audio_entry_points_validate_before_any_device_call(lib):
    d = ctypes.c_void_p(16)                           # never dereferenced: every call below fails validation or returns first
    z = ctypes.c_void_p(0)
    assert lib.glowk_mel_frontend(z, 1, 32640, 80.0, d, z, z) != 0 and "null" in _err(lib)
    assert lib.glowk_mel_frontend(d, 1, 32640, 80.0, z, z, z) != 0 and "null" in _err(lib)
    assert lib.glowk_mel_frontend(d, 1, 1024, 80.0, d, z, z) != 0 and "n_samples" in _err(lib)
    assert lib.glowk_mel_frontend(d, 1, 65536, 80.0, d, z, z) != 0 and "n_samples" in _err(lib)
    assert lib.glowk_mel_frontend(d, -1, 32640, 80.0, d, z, z) != 0 and "N must" in _err(lib)
    assert lib.glowk_mel_frontend(d, 1, 32640, float("nan"), d, z, z) != 0 and "top_db" in _err(lib)
    assert lib.glowk_mel_frontend(d, 0, 32640, 80.0, d, z, z) == 0
    assert lib.glowk_mel_to_power(z, 1, 64, 200, d, z) != 0 and "null" in _err(lib)
    assert lib.glowk_mel_to_power(d, 1, 0, 200, d, z) != 0 and "frames" in _err(lib)
    assert lib.glowk_mel_to_power(d, 1, 129, 200, d, z) != 0 and "frames" in _err(lib)
    assert lib.glowk_mel_to_power(d, 1, 64, -1, d, z) != 0 and "iters" in _err(lib)
    assert lib.glowk_mel_to_power(d, 1, 64, 100001, d, z) != 0 and "iters" in _err(lib)
    assert lib.glowk_mel_to_power(d, 0, 64, 200, d, z) == 0
    assert lib.glowk_masked_istft(d, 2, z, 1, 64, 0, d, z) != 0 and "null" in _err(lib)
    assert lib.glowk_masked_istft(d, 1, d, 1, 64, 1, d, z) != 0 and "Wiener" in _err(lib)
    assert lib.glowk_masked_istft(d, 0, d, 1, 64, 0, d, z) != 0 and "S must" in _err(lib)
    assert lib.glowk_masked_istft(d, 2, d, 1, 1, 0, d, z) != 0 and "frames" in _err(lib)
    assert lib.glowk_masked_istft(d, 2, d, 0, 64, 1, d, z) == 0


def test_separate_audio_refuses_other_rates(tmp_path):
    q = tmp_path / "c.wav"
    with wave.open(str(q), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(22050)
        w.writeframes(np.zeros(10, "<i2").tobytes())
    with pytest.raises(ValueError, match="22050"):
        audio.separate_audio(str(q), None, None, [1.0])


def test_kernel_filterbank_shape_support_and_oracle(lib):
    """The table the kernels use (built in C++, read back through glowk_mel_filterbank) against the oracle's."""
    W = audio.mel_filterbank()
    assert W.shape == (96, 1025) and W.dtype == np.float32
    freqs = np.arange(1025) * 16000.0 / 2048
    assert not W[:, (freqs <= 125.0) | (freqs >= 7600.0)].any()
    assert (W.sum(axis=0)[(freqs > 140.0) & (freqs < 7500.0)] > 0).all()
    assert ((W > 0).sum(axis=0) <= 2).all()                          # the band-sparse kernels rely on it
    np.testing.assert_allclose(W, R.mel_filterbank(), rtol=1e-6, atol=0)
    # Slaney normalisation: every triangle has area 1 on the Hz axis (up to the bin grid)
    area = W.astype(np.float64).sum(axis=1) * (16000.0 / 2048)
    assert np.all(np.abs(area - 1.0) < 0.1), area
    assert lib.glowk_mel_filterbank(None) != 0 and "null" in _err(lib)


def test_mismatched_shapes_are_refused_before_the_kernels():
    """Host-side checks of audio.py: a wrong shape never reaches a kernel (all of these raise before any device work)."""
    tiles = np.zeros((2, 96, 64), np.float32)
    X = torch.zeros((2, 1025, 64), dtype=torch.complex64)
    with pytest.raises(ValueError, match="96"):
        audio.mel_to_power(np.zeros((2, 64, 96), np.float32))               # mel and frame axes swapped
    with pytest.raises(ValueError):
        audio.mel_to_power(np.zeros((2, 96, 200), np.float32))              # more frames than the kernels take
    with pytest.raises(ValueError, match="do not match"):
        audio.invert([tiles, np.zeros((3, 96, 64), np.float32)], X)         # N differs from the mixture's
    with pytest.raises(ValueError, match="do not match"):
        audio.invert([np.zeros((2, 96, 63), np.float32)], X)                # F differs
    with pytest.raises(ValueError, match="match the powers"):
        audio.masked_istft(torch.zeros((2, 3, 1025, 64)), X)
    with pytest.raises(ValueError, match="1025"):
        audio.masked_istft(torch.zeros((2, 2, 1024, 64)), X)
    with pytest.raises(ValueError, match="2 sources"):
        audio.masked_istft(torch.zeros((1, 2, 1025, 64)), X, wiener=True)
    with pytest.raises(ValueError, match="complex"):
        audio.masked_istft(torch.zeros((2, 2, 1025, 64)), torch.zeros((2, 1025, 64)))
    with pytest.raises(ValueError, match="1024 < n"):
        audio.mel_tiles(np.zeros((2, 1024), np.float32))
