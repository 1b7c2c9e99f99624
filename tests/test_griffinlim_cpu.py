"""CPU checks of Griffin-Lim and the `whole` inversion (audiosourcesep_amd/audio.py, glowk_griffinlim): the fp64 oracle on known
cases and the argument validation (no GPU: every call here is refused before any device call)."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, audio
from tests import audio_ref as R
from tests import griffinlim_ref as G


def test_oracle_keeps_a_consistent_spectrum_and_converges():
    rng = np.random.default_rng(0)
    y = rng.standard_normal(20 * 512)
    X = R.stft(y)
    assert X.shape == (1025, 21)
    # n_iter = 0 with the true phases is the plain iSTFT
    assert np.abs(G.griffinlim(np.abs(X), n_iter=0, init=np.exp(1j * np.angle(X))) - y[:20 * 512]).max() < 1e-12
    init = np.exp(2j * np.pi * rng.uniform(0.0, 1.0, X.shape))
    sc = [G.spectral_convergence(G.griffinlim(np.abs(X), n_iter=n, init=init), np.abs(X)) for n in (0, 8, 32)]
    assert sc[0] > sc[1] > sc[2]
    assert G.whole(np.arange(12).reshape(2, 2, 3)).tolist() == [[0, 1, 2, 6, 7, 8], [3, 4, 5, 9, 10, 11]]


def test_griffinlim_arguments_are_validated():
    S = torch.zeros((2, 1025, 8))
    for bad in (torch.zeros((1025, 8)), torch.zeros((2, 1024, 8)), torch.zeros((2, 1025, 3)), torch.zeros((1, 1025, (1 << 20) + 1))):
        with pytest.raises(ValueError, match="S: expected"):
            audio.griffinlim(bad)
    with pytest.raises(ValueError, match="real"):
        audio.griffinlim(torch.zeros((2, 1025, 8), dtype=torch.complex64))
    for n_iter in (-1, 1.5, 100001, True):
        with pytest.raises(ValueError, match="n_iter"):
            audio.griffinlim(S, n_iter=n_iter)
    for momentum in (-0.1, float("nan"), float("inf"), "0.99"):
        with pytest.raises(ValueError, match="momentum"):
            audio.griffinlim(S, momentum=momentum)
    with pytest.raises(ValueError, match="init"):
        audio.griffinlim(S, init="zeros")
    with pytest.raises(ValueError, match="init"):
        audio.griffinlim(S, init=torch.ones((2, 1025, 8)))                       # real phases
    with pytest.raises(ValueError, match="init"):
        audio.griffinlim(S, init=torch.ones((2, 1025, 9), dtype=torch.complex64))
    with pytest.warns(UserWarning, match="momentum"):                           # librosa warns above 1 and goes on
        with pytest.raises(ValueError, match="init"):
            audio.griffinlim(S, momentum=1.5, init="zeros")


def test_mel_to_audio_and_invert_arguments_are_validated():
    tiles = np.zeros((2, 96, 64), np.float32)
    X = torch.zeros((2, 1025, 64), dtype=torch.complex64)
    with pytest.raises(ValueError, match="method"):
        audio.mel_to_audio(tiles, method="tile")
    with pytest.raises(ValueError, match="4 <= frames"):
        audio.mel_to_audio(np.zeros((5, 96, 3), np.float32))                   # 'frame': 3 frames per signal
    with pytest.raises(ValueError, match="4 <= frames"):
        audio.mel_to_audio(np.zeros((1, 96, 3), np.float32), method="whole")   # 'whole': 3 frames in all
    with pytest.raises(ValueError, match="96"):
        audio.mel_to_audio(np.zeros((2, 64, 96), np.float32))
    with pytest.raises(ValueError, match="n_iter"):
        audio.mel_to_audio(tiles, n_iter=-1)
    with pytest.raises(ValueError, match="momentum"):
        audio.mel_to_audio(tiles, momentum=-1.0)
    with pytest.raises(ValueError, match="init"):
        audio.mel_to_audio(tiles, init=torch.ones((1, 1025, 128), dtype=torch.complex64), method="whole")   # init is per tile
    with pytest.raises(ValueError, match="algorithm"):
        audio.invert([tiles], X, algorithm="griffinlim")
    with pytest.raises(ValueError, match="method"):
        audio.invert([tiles], X, method="frames")
    with pytest.raises(ValueError, match="stft_mixture"):
        audio.invert([tiles, tiles])                                              # reuse phase needs the mixture
    with pytest.raises(ValueError, match="wiener"):
        audio.invert([tiles, tiles], algorithm="griffin", wiener=True)
    with pytest.raises(ValueError, match="do not match"):
        audio.invert([tiles, np.zeros((3, 96, 64), np.float32)], algorithm="griffin")
    with pytest.raises(ValueError, match="4 <= frames"):
        audio.invert([np.zeros((2, 96, 3), np.float32)], algorithm="griffin")
    with pytest.raises(ValueError, match="n_iter"):
        audio.invert([tiles], algorithm="griffin", n_iter=-2)
    with pytest.raises(ValueError, match="4 <= frames"):
        audio.invert([np.zeros((1, 96, 3), np.float32)], torch.zeros((1, 1025, 3), dtype=torch.complex64), method="whole")
    with pytest.raises(ValueError, match="2 sources"):
        audio.invert([tiles], X, wiener=True, method="whole")
    with pytest.raises(ValueError, match="do not match"):
        audio.invert([np.zeros((2, 96, 63), np.float32)], X, method="whole")
    with pytest.raises(ValueError, match="algorithm"):
        audio.separate_audio("no-such-file.wav", None, None, [1.0], algorithm="Griffin")
    with pytest.raises(ValueError, match="method"):
        audio.separate_audio("no-such-file.wav", None, None, [1.0], method="all")
    with pytest.raises(ValueError, match="momentum"):
        audio.separate_audio("no-such-file.wav", None, None, [1.0], algorithm="griffin", momentum=-1)


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def test_griffinlim_entry_point_validates_before_any_device_call(lib):
    d = ctypes.c_void_p(16)                           # never dereferenced: every call below fails validation or returns first
    z = ctypes.c_void_p(0)
    err = lambda: lib.glowk_last_error().decode()     # noqa: E731
    assert lib.glowk_griffinlim(z, z, 1, 64, 32, 0.99, d, z) != 0 and "null" in err()
    assert lib.glowk_griffinlim(d, z, 1, 64, 32, 0.99, z, z) != 0 and "null" in err()
    assert lib.glowk_griffinlim(d, z, -1, 64, 32, 0.99, d, z) != 0 and "N must" in err()
    assert lib.glowk_griffinlim(d, z, 1, 3, 32, 0.99, d, z) != 0 and "frames" in err()
    assert lib.glowk_griffinlim(d, z, 1, (1 << 20) + 1, 32, 0.99, d, z) != 0 and "frames" in err()
    assert lib.glowk_griffinlim(d, z, 1, 64, -1, 0.99, d, z) != 0 and "n_iter" in err()
    assert lib.glowk_griffinlim(d, z, 1, 64, 100001, 0.99, d, z) != 0 and "n_iter" in err()
    for m in (-0.5, float("nan"), float("inf")):
        assert lib.glowk_griffinlim(d, z, 1, 64, 32, m, d, z) != 0 and "momentum" in err()
    assert lib.glowk_griffinlim(d, z, 1 << 20, 1 << 20, 32, 0.99, d, z) != 0 and "too large" in err()
    assert lib.glowk_griffinlim(d, d, 0, 64, 32, 0.99, d, z) == 0
