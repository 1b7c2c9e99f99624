"""fp64 NumPy oracle of the audio ends of the pipeline (a helper of the audio tests, not a test module).

Restates the reference's front end (datasets/data_loader.py:146-164: librosa.stft center=True, |X|^2, librosa.filters.mel,
power_to_db, np.clip) and its `frame` inversion (melspec_inversion_basis.py:42-93: db_to_power, mel_to_stft's NNLS, reuse-phase
or single-channel Wiener mask, librosa.istft) from the formulas, with numpy.fft.  The NNLS is the project's definition (FISTA from
max(0, W+ b), step 1/|W|_2^2, a fixed iteration count), not librosa's L-BFGS-B, whose particular minimiser no other solver reproduces.
"""
import numpy as np

SR, NFFT, HOP, NMEL, FMIN, FMAX = 16000, 2048, 512, 96, 125.0, 7600.0
NBIN = NFFT // 2 + 1
EXTRACT = int(SR * 2.04)
_LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(f):
    """Slaney mel scale (librosa htk=False): 3 mels per 200 Hz below 1 kHz, logarithmic above."""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / _LOGSTEP, f / (200.0 / 3.0))


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp(_LOGSTEP * (m - 15.0)), (200.0 / 3.0) * m)


def mel_filterbank():
    """[96, 1025] float32: triangles between consecutive points of 98 mel-spaced frequencies, area-normalised (Slaney)."""
    mel_f = mel_to_hz(np.linspace(hz_to_mel(FMIN), hz_to_mel(FMAX), NMEL + 2))
    fft_f = np.arange(NBIN) * (SR / NFFT)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    enorm = 2.0 / (mel_f[2:] - mel_f[:-2])
    return (np.maximum(0.0, np.minimum(lower, upper)) * enorm[:, None]).astype(np.float32)


def hann():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)


def stft(y):
    """[n] -> [1025, 1 + n // 512] complex128 (center=True, reflect padding, periodic Hann)."""
    y = np.asarray(y, dtype=np.float64)
    p = np.pad(y, NFFT // 2, mode="reflect")
    F = 1 + len(y) // HOP
    idx = np.arange(F)[:, None] * HOP + np.arange(NFFT)[None, :]
    return np.fft.rfft(p[idx] * hann(), axis=1).T


def mel_db(y, top_db=80.0, return_stft=False):
    """One extract -> [96, F] dB: power_to_db(W |X|^2) with the per-extract top_db floor (None or <= 0: none), clipped to [-100, 20]."""
    X = stft(y)
    M = mel_filterbank().astype(np.float64) @ (np.abs(X) ** 2)
    L = 10.0 * np.log10(np.maximum(1e-10, M))
    if top_db is not None and top_db > 0:
        L = np.maximum(L, L.max() - top_db)
    L = np.clip(L, -100.0, 20.0)
    return (L, X) if return_stft else L


def nnls_setup():
    A = mel_filterbank().astype(np.float64)
    return A, np.linalg.pinv(A), 1.0 / np.linalg.norm(A, 2) ** 2


def fista_nnls(b, iters=200, setup=None):
    """min_{x >= 0} |A x - b| for every column of b [96, F] -> [1025, F]: FISTA from max(0, A+ b)."""
    A, Ap, step = setup or nnls_setup()
    x = np.maximum(0.0, Ap @ b)
    y = x.copy()
    t = 1.0
    for _ in range(iters):
        z = np.maximum(0.0, y - step * (A.T @ (A @ y - b)))
        t1 = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        y = z + ((t - 1.0) / t1) * (z - x)
        x, t = z, t1
    return x


def mel_to_power(L, iters=200, setup=None):
    """[96, F] dB -> [1025, F] linear power: db_to_power, then the NNLS per frame."""
    return fista_nnls(10.0 ** (np.asarray(L, dtype=np.float64) / 10.0), iters, setup)


def istft(Y):
    """[1025, F] complex -> (F - 1) * 512 samples (librosa.istft, center=True)."""
    F = Y.shape[1]
    frames = np.fft.irfft(Y.T, n=NFFT, axis=1) * hann()
    n = NFFT + HOP * (F - 1)
    y = np.zeros(n)
    wss = np.zeros(n)
    for f in range(F):
        y[f * HOP:f * HOP + NFFT] += frames[f]
        wss[f * HOP:f * HOP + NFFT] += hann() ** 2
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    return y[NFFT // 2:-(NFFT // 2)]


def masked_istft(powers, X_mix, wiener=False):
    """powers: S arrays [1025, F] of one extract, X_mix [1025, F] -> S signals of (F - 1) * 512 samples."""
    powers = [np.asarray(p, dtype=np.float64) for p in powers]
    if wiener:
        tot = np.sum(powers, axis=0) + 1e-10
        return [istft(p / tot * X_mix) for p in powers]
    phase = np.exp(1j * np.angle(X_mix))
    return [istft(np.sqrt(p) * phase) for p in powers]
