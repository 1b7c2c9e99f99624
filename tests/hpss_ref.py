"""NumPy restatement of harmonic / percussive separation by median filtering (a helper of the HPSS tests, not a test module): the
reflect index map, the median by sorting gathered windows, librosa.util.softmask step by step in fp64, and ``hpss`` / ``hpss_audio``
on the STFT pair of tests/audio_ref.py.  Written from the formulas of include/glowk.h and the documented semantics of
scipy.ndimage.median_filter(mode='reflect') and librosa.decompose.hpss, with no code of the package.  No scipy at module level."""
import numpy as np

from tests import audio_ref as A
from tests import longform_ref as L

TINY = float(np.finfo(np.float32).tiny)                  # 1.17549435e-38: librosa.util.tiny of float32 input


def reflect_index(j, n):
    """Half-sample symmetric extension d c b a | a b c d | d c b a: index j (any integer array) of an axis of length n."""
    r = np.mod(np.asarray(j, dtype=np.int64), 2 * n)     # numpy's mod is the mathematical one: r in [0, 2 n)
    return np.where(r < n, r, 2 * n - 1 - r)


def median_filter(S, size, axis):
    """The running median of odd length ``size`` of S [..., rows, F] along the frames (axis = 0, the last array axis) or the rows
    (axis = 1, the one before it): gather each window through the reflect map, sort it, take the middle.  Keeps S's dtype: a
    selection, so float32 in gives the input's own bits out."""
    S = np.asarray(S)
    assert size % 2 == 1 and axis in (0, 1)
    ax = S.ndim - 1 - axis
    n = S.shape[ax]
    idx = reflect_index(np.arange(n)[:, None] + np.arange(-(size // 2), size // 2 + 1)[None, :], n)      # [n, size]
    win = np.take(S, idx.reshape(-1), axis=ax).reshape(S.shape[:ax] + (n, size) + S.shape[ax + 1:])
    return np.sort(win, axis=ax + 1).take(size // 2, axis=ax + 1)


def softmask(X, R, power=1.0, split_zeros=False):
    """librosa.util.softmask(X, X_ref, power, split_zeros) in fp64, with float32's tiny as the threshold (the spectra are float32)."""
    X, R = np.asarray(X, dtype=np.float64), np.asarray(R, dtype=np.float64)
    if np.isinf(power):
        return (X > R).astype(np.float64)
    Z = np.maximum(X, R)
    bad = Z < TINY
    Z = np.where(bad, 1.0, Z)
    m, r = (X / Z) ** power, (R / Z) ** power
    mask = m / np.where(bad, 1.0, m + r)
    return np.where(bad, 0.5 if split_zeros else 0.0, mask)


def pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def masks(harm, perc, power=2.0, margin=1.0):
    """The two masks of librosa.decompose.hpss from the two filtered spectra."""
    mh, mp = pair(margin)
    split = mh == 1 and mp == 1
    harm, perc = np.asarray(harm, dtype=np.float64), np.asarray(perc, dtype=np.float64)
    return softmask(harm, perc * mh, power, split), softmask(perc, harm * mp, power, split)


def hpss(S, kernel_size=31, power=2.0, mask=False, margin=1.0):
    """librosa.decompose.hpss of S [..., rows, F] (real magnitudes, or complex: split into magnitude and phase)."""
    S = np.asarray(S)
    mag, phase = (np.abs(S), np.exp(1j * np.angle(S))) if np.iscomplexobj(S) else (S, 1.0)
    kh, kp = pair(kernel_size)
    mask_h, mask_p = masks(median_filter(mag, kh, 0), median_filter(mag, kp, 1), power, margin)
    if mask:
        return mask_h, mask_p
    return mag * mask_h * phase, mag * mask_p * phase


def hpss_audio(y, kernel_size=31, power=2.0, margin=1.0, residual=False):
    """One signal [n] at 16 kHz -> (harmonic, percussive[, residual]), each [n]: zero-pad to a hop multiple, STFT, ``hpss`` on |X|
    (rounded to float32, as the device holds it), the masked magnitudes with the mixture's phase, iSTFT, the first n samples."""
    y = np.asarray(y, dtype=np.float64)
    X = A.stft(L.pad_hop(y))
    mag = np.abs(X).astype(np.float32)
    mask_h, mask_p = hpss(mag, kernel_size, power, True, margin)
    phase = np.exp(1j * np.angle(X))
    h, p = (A.istft(mag * m * phase)[:len(y)] for m in (mask_h, mask_p))
    return (h, p, y - h - p) if residual else (h, p)


def sines_and_clicks(n=24576, sr=16000):
    """(sines, clicks): 0.3 sin(2 pi 440 t) + 0.2 sin(2 pi 1320 t), and 0.8 Hann(32) clicks of alternating sign every 4000 samples
    from sample 2000.  The mixture is their sum."""
    t = np.arange(n) / sr
    sines = 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 1320.0 * t)
    clicks = np.zeros(n)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(32) / 32)
    for k, at in enumerate(range(2000, n - 32, 4000)):
        clicks[at:at + 32] += (0.8 if k % 2 == 0 else -0.8) * hann
    return sines, clicks
