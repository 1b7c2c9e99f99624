"""Audio in, audio out: wav I/O, the mel front end and the mel-to-audio inversion around the BASIS loop.

Replaces the reference's ``get_song_extract`` (datasets/data_loader.py:113-164) and the ``frame`` method of
``melspec_inversion_basis.py`` (:42-93, ``run_basis_sep.py --inverse``) without librosa, soundfile or TensorFlow.  The constants
are those of ``tile_io.MEL_FRONTEND`` (16 kHz, n_fft 2048, hop 512, 96 Slaney mels over 125..7600 Hz, -100..20 dB, 2.04 s
extracts), compiled into the HIP kernels of ``csrc/glowk_audio.h``:

* ``mel_tiles``: STFT (a GEMM on the exact-fp32 MFMA), |X|^2, mel, dB with the per-extract ``top_db`` floor, clip;
* ``mel_to_power``: 10^(L/10), then mel -> linear power by NNLS per frame.  librosa solves it with L-BFGS-B, whose particular
  minimiser of the underdetermined problem (96 equations, 1025 unknowns) no other solver reproduces; here it is FISTA from
  max(0, W+ b) with step 1/|W|_2^2 and a fixed iteration count (200 by default);
* ``invert``: reuse the mixture's phase (or a single-channel Wiener filter over the sources) and the inverse STFT.

Not covered: resampling (input must be 16 kHz), Griffin-Lim, the ``whole`` inversion method, the power-scale flows
(``scale='power'``) and stereo output.
"""
import ctypes
import wave

import numpy as np
import torch

from . import _lib, basis
from .tile_io import MEL_FRONTEND

SR = MEL_FRONTEND["sampling_rate"]
HOP = MEL_FRONTEND["hop_length"]
NBIN = MEL_FRONTEND["n_fft"] // 2 + 1
NMEL = MEL_FRONTEND["n_mels"]
EXTRACT = int(SR * MEL_FRONTEND["length_sec"])          # 32 640 samples (datasets/preprocessing.py:9-26)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _s(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def read_wav(path):
    """16-bit PCM wav -> float32 mono in [-1, 1) (int / 32768; channels averaged).  Raises ValueError on any rate but 16 kHz."""
    with wave.open(str(path), "rb") as w:
        rate, ch, width, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
        if width != 2:
            raise ValueError("%s: only 16-bit PCM is supported (sample width %d bytes)" % (path, width))
        if rate != SR:
            raise ValueError("%s: sampling rate %d Hz, the front end needs %d Hz (no resampling)" % (path, rate, SR))
        data = np.frombuffer(w.readframes(n), dtype="<i2").astype(np.float32) / 32768.0
    return data.reshape(-1, ch).mean(axis=1, dtype=np.float32) if ch > 1 else data


def write_wav(path, y, sr=SR):
    """float mono -> 16-bit PCM wav (round(y * 32767), clipped to [-1, 1] first)."""
    if sr != SR:
        raise ValueError("sampling rate %d Hz: only %d Hz is supported" % (sr, SR))
    y = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
    q = np.rint(np.clip(y.astype(np.float64).reshape(-1), -1.0, 1.0) * 32767.0).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(q.tobytes())


def extracts(y, skip=0, n=None):
    """[samples] -> [N, 32640]: consecutive 2.04 s extracts, the trailing partial one dropped, the first ``skip`` skipped
    (``get_song_extract`` skips 2), at most ``n``."""
    y = y if torch.is_tensor(y) else torch.as_tensor(np.asarray(y, dtype=np.float32))
    total = y.shape[-1] // EXTRACT
    stop = total if n is None else min(total, skip + n)
    return y[skip * EXTRACT:max(stop, skip) * EXTRACT].reshape(-1, EXTRACT)


def mel_filterbank():
    """The front end's [96, 1025] float32 mel weights as the kernels use them (librosa.filters.mel defaults: Slaney scale and
    area normalisation, built in fp64 and rounded; ``glowk_mel_filterbank``)."""
    W = np.empty((NMEL, NBIN), dtype=np.float32)
    _lib.check(_lib.load().glowk_mel_filterbank(W.ctypes.data_as(_lib._fp)))
    return W


def _tensor(x, what):
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x))
    if x.is_complex() != (what == "stft_mixture"):
        raise ValueError("%s: expected a %s tensor, got %s" % (what, "complex" if what == "stft_mixture" else "real", x.dtype))
    return x


def _device(*tensors):
    """The CUDA device of the inputs (the current one if they are all on the host); inputs on two GPUs are refused."""
    devs = {t.device for t in tensors if t.is_cuda}
    if len(devs) > 1:
        raise ValueError("inputs on different devices: %s" % sorted(str(d) for d in devs))
    return devs.pop() if devs else torch.device("cuda", torch.cuda.current_device())


def _check_tiles(t, what="tiles"):
    if not (t.dim() == 3 or (t.dim() == 4 and t.shape[3] == 1)) or t.shape[1] != NMEL or not 1 <= t.shape[2] <= 128:
        raise ValueError("%s: expected [N, 96, F] or [N, 96, F, 1] dB tiles with 1 <= F <= 128, got %s" % (what, tuple(t.shape)))


def mel_tiles(extracts, top_db=80.0, return_stft=False):
    """[N, n] 16 kHz audio -> dB mel tiles [N, 96, F, 1] on the GPU (F = 1 + n // 512: 64 for an extract); with
    ``return_stft`` also the complex STFT [N, 1025, F] (complex64), the ``stft_mixture`` of the inversion.
    ``top_db`` (power_to_db's 80 in ``get_song_extract``; None or 0 for the dataset path): per-extract floor at max - top_db."""
    x = _tensor(extracts, "extracts")
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2 or not 1024 < x.shape[1] < 65536:
        raise ValueError("extracts: expected [N, n] audio with 1024 < n < 65536, got %s" % (tuple(x.shape),))
    x = x.to(device=_device(x), dtype=torch.float32).contiguous()
    N, n = x.shape
    F = 1 + n // HOP
    mel = torch.empty((N, NMEL, F, 1), device=x.device, dtype=torch.float32)
    X = torch.empty((N, NBIN, F, 2), device=x.device, dtype=torch.float32)    # also the kernels' |X|^2 source: no scratch outside torch
    _lib.check(_lib.load().glowk_mel_frontend(_p(x), N, n, float(top_db or 0.0), _p(mel), _p(X), _s(x)))
    return (mel, torch.view_as_complex(X)) if return_stft else mel


def mel_to_power(tiles, iters=200):
    """dB mel tiles [N, 96, F(, 1)] -> linear power spectra [N, 1025, F] (NNLS by FISTA, ``iters`` iterations)."""
    t = _tensor(tiles, "tiles")
    _check_tiles(t)
    t = t.to(device=_device(t), dtype=torch.float32).contiguous()
    N, F = t.shape[0], t.shape[2]
    out = torch.empty((N, NBIN, F), device=t.device, dtype=torch.float32)
    _lib.check(_lib.load().glowk_mel_to_power(_p(t), N, F, int(iters), _p(out), _s(t)))
    return out


def masked_istft(powers, stft_mixture, wiener=False):
    """powers [S, N, 1025, F] + mixture STFT [N, 1025, F] (complex64) -> audio [S, N, (F - 1) * 512]."""
    p, X = _tensor(powers, "powers"), _tensor(stft_mixture, "stft_mixture")
    if p.dim() != 4 or p.shape[2] != NBIN or not 2 <= p.shape[3] <= 128:
        raise ValueError("powers: expected [S, N, 1025, F] with 2 <= F <= 128, got %s" % (tuple(p.shape),))
    if tuple(X.shape) != (p.shape[1], NBIN, p.shape[3]):
        raise ValueError("stft_mixture: expected [N, 1025, F] = %s to match the powers, got %s" % ((p.shape[1], NBIN, p.shape[3]), tuple(X.shape)))
    if wiener and p.shape[0] < 2:
        raise ValueError("the Wiener filter needs at least 2 sources, got %d" % p.shape[0])
    dev = _device(p, X)
    p = p.to(device=dev, dtype=torch.float32).contiguous()
    X = torch.view_as_real(X.to(device=dev, dtype=torch.complex64)).contiguous()
    S, N, _, F = p.shape
    out = torch.empty((S, N, (F - 1) * HOP), device=dev, dtype=torch.float32)
    _lib.check(_lib.load().glowk_masked_istft(_p(p), S, _p(X), N, F, 1 if wiener else 0, _p(out), _s(p)))
    return out


def invert(tile_batches, stft_mixture, wiener=False, iters=200):
    """The ``frame`` inversion of melspec_inversion_basis.py: S batches of dB tiles [N, 96, F(, 1)] of one mixture and its STFT
    [N, 1025, F] -> [S, N * (F - 1) * 512] (the extracts' signals concatenated).  ``wiener`` needs S >= 2.  One NNLS launch
    covers the frames of all S batches."""
    tiles = [_tensor(t, "tiles") for t in tile_batches]
    X = _tensor(stft_mixture, "stft_mixture")
    for t in tiles:
        _check_tiles(t)
        if tuple(t.shape[:3]) != (X.shape[0], NMEL, X.shape[-1]):
            raise ValueError("tiles %s do not match stft_mixture %s: expected [N, 96, F] = %s"
                             % (tuple(t.shape), tuple(X.shape), (X.shape[0], NMEL, X.shape[-1])))
    dev = _device(X, *tiles)
    batch = torch.cat([t.to(device=dev, dtype=torch.float32).reshape(t.shape[0], NMEL, -1) for t in tiles])
    powers = mel_to_power(batch, iters).reshape(len(tiles), -1, NBIN, batch.shape[2])
    y = masked_istft(powers, X, wiener)
    return y.reshape(y.shape[0], -1)


def separate_audio(mix, flow1, flow2, sigmas, restore_1=None, restore_2=None, T=100, delta=2e-5, seed=0, skip=0, n=None, wiener=False,
                   top_db=80.0, iters=200):
    """A mixture (wav path or 16 kHz samples) -> two separated signals: front end, ``basis.basis_outer_loop`` from the reference's
    uniform start over [-100, 20] dB (run_basis_sep.py:360-361; device RNG streams 14 / 15 of ``seed``, apart from the Langevin
    noise's 0 / 1), inversion.  Returns ``(y1, y2, mixed, x1, x2)``: the signals [N * 32256] and the tiles [N, 96, 64, 1]."""
    y = read_wav(mix) if isinstance(mix, (str, bytes)) or hasattr(mix, "__fspath__") else mix
    mixed, X = mel_tiles(extracts(y, skip, n), top_db=top_db, return_stft=True)
    x1 = -100.0 + 120.0 * basis.device_randn(tuple(mixed.shape), mixed.device, seed=seed, which=14, uniform=True)
    x2 = -100.0 + 120.0 * basis.device_randn(tuple(mixed.shape), mixed.device, seed=seed, which=15, uniform=True)
    x1, x2, _ = basis.basis_outer_loop(mixed, x1, x2, flow1, flow2, sigmas, restore_1=restore_1, restore_2=restore_2, T=T, delta=delta,
                                       seed=seed)
    out = invert([x1, x2], X, wiener=wiener, iters=iters)
    return out[0], out[1], mixed, x1, x2
