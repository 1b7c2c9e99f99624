"""fp64 NumPy oracle of Griffin-Lim (a helper of the Griffin-Lim tests, not a test module).

Restates librosa.griffinlim (0.7.2, momentum form) and librosa.feature.inverse.mel_to_audio from the formulas, on the STFT and
iSTFT of tests/audio_ref.py (n_fft 2048, hop 512, periodic Hann, center=True, reflect padding).  The random start is an input:
librosa draws it from NumPy's global RNG, which no other implementation reproduces.
"""
import numpy as np

from tests import audio_ref as R


def griffinlim(S, n_iter=32, momentum=0.99, init=None):
    """S [1025, F] magnitudes, init [1025, F] complex (None: ones) -> (F - 1) * 512 samples."""
    S = np.asarray(S, dtype=np.float64)
    angles = np.ones(S.shape, np.complex128) if init is None else np.asarray(init, dtype=np.complex128).copy()
    beta = momentum / (1.0 + momentum)
    rebuilt = 0.0
    for _ in range(n_iter):
        tprev = rebuilt
        inverse = R.istft(S * angles)
        rebuilt = R.stft(inverse)
        angles = rebuilt - beta * tprev
        angles /= np.abs(angles) + 1e-16
    return R.istft(S * angles)


def spectral_convergence(y, S):
    """|| |STFT(y)| - S || / ||S|| (Frobenius)."""
    S = np.asarray(S, dtype=np.float64)
    return float(np.linalg.norm(np.abs(R.stft(np.asarray(y, dtype=np.float64))) - S) / np.linalg.norm(S))


def whole(x):
    """[N, ..., F] -> [..., N F]: the tiles side by side along the frame axis."""
    return np.concatenate(list(x), axis=-1)
