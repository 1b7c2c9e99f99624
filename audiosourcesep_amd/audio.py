"""Audio in, audio out: wav I/O, the mel front end and the mel-to-audio inversion around the BASIS loop.

Replaces the reference's ``get_song_extract`` (datasets/data_loader.py:113-164) and ``melspec_inversion_basis.py`` (:21-93,
``run_basis_sep.py --inverse``) without librosa, soundfile or TensorFlow.  The constants are those of ``tile_io.MEL_FRONTEND``
(16 kHz, n_fft 2048, hop 512, 96 Slaney mels over 125..7600 Hz, -100..20 dB, 2.04 s extracts), compiled into the HIP kernels of
``csrc/glowk_audio.h``:

* ``mel_tiles``: STFT (a GEMM on the exact-fp32 MFMA), |X|^2, mel, dB with the per-extract ``top_db`` floor, clip;
* ``mel_to_power``: 10^(L/10), then mel -> linear power by NNLS per frame.  librosa solves it with L-BFGS-B, whose particular
  minimiser of the underdetermined problem (96 equations, 1025 unknowns) no other solver reproduces; here it is FISTA from
  max(0, W+ b) with step 1/|W|_2^2 and a fixed iteration count (200 by default);
* ``griffinlim`` / ``mel_to_audio``: librosa.griffinlim and librosa.feature.inverse.mel_to_audio (NNLS, square root, 32
  Griffin-Lim iterations with momentum 0.99).  Each iteration is one STFT and one iSTFT with the phase update folded into its
  spectrum staging; the whole loop is one C call.  ``init='random'`` draws its phases from the device RNG (stream
  ``GRIFFINLIM_STREAM`` of ``seed``), not from NumPy's global RNG, so librosa's own random start is not reproduced;
* ``invert``: reuse the mixture's phase (or a single-channel Wiener filter over the sources) or Griffin-Lim, per tile
  (``method='frame'``) or on the tiles concatenated along time (``'whole'``);
* ``separate_sources`` / ``separate_wav_sources``: ``separate_audio`` / ``separate_wav`` for a list of 2..16 priors;
* ``resample`` / ``load_audio`` / ``save_audio`` / ``separate_wav``: PCM wavs of 8 to 32 bits at any rate in, 16-bit wavs at any
  rate out, around a band-limited sample-rate converter on the GPU (``csrc/glowk_resample.h``) -- what ``librosa.core.load(path,
  sr=16000)`` does for the reference (datasets/preprocessing.py:21).  The filter is the same design as librosa 0.7's default
  (resampy's ``kaiser_best``), evaluated at the exact position of every tap; it is not bit-compatible with resampy, whose samples
  cannot be observed here (derived, not observed).  ``read_wav`` / ``write_wav`` / ``separate_audio`` keep to 16 kHz.
* ``multichannel_wiener`` / ``istft`` / ``separate_stereo`` / ``separate_wav_stereo``: stereo in, stereo stems out.  The priors
  stay mono (they see the downmix); the stems come from a multichannel Wiener filter under the local Gaussian model whose
  spatial covariances are fitted by EM from the priors' PSDs (Duong, Vincent, Gribonval 2010; ``csrc/glowk_stereo.h``, one launch).
* ``separate_long`` / ``separate_wav_long``: a whole file in, stems exactly as long as it and aligned with it out (mono or
  stereo).  The per-extract paths above follow the reference, which only ever cuts disjoint 2.04 s extracts: they drop the trailing
  partial extract and shift extract k by 384 k ('frame') or 128 k ('whole') samples.  Here one STFT covers the whole signal
  (``mel_frames``), the priors see tiles cut every ``tile_hop`` frames (``frame_tiles``), their estimates are cross-faded back into
  frames (``stitch_tiles``: sin^2 weights, a weighted mean in dB) and one inversion of the whole signal is trimmed to the input's
  length (``invert_frames``, ``mask_istft_long``).  Kernels in ``csrc/glowk_longform.h``; not in the reference.

Not covered: IEEE-float and WAVE_FORMAT_EXTENSIBLE wavs and the power-scale flows (``scale='power'``).
"""
import ctypes
import math
import struct
import warnings
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
GRIFFINLIM_STREAM = 13      # device RNG stream of init='random' (stream ids are 0..15; 0-3 serve the flows, 11 nmfd, 12 nmf, 14 / 15 separate_audio)
GRIFFINLIM_MAX_FRAMES = 1 << 20                          # glowk_griffinlim's cap: 9.3 h of 16 kHz audio in one signal
MWF_EM_MAX_ITER = 1000                                   # glowk_mwf_em's cap on its EM iterations
MIN_RATE, MAX_RATE = 1000, 768000                        # glowk_resample's sampling rates, at most a factor 64 apart
ALGORITHMS = ("reuse_phase", "griffin")
METHODS = ("frame", "whole")


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


def _check_rate(sr, what):
    if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or not MIN_RATE <= sr <= MAX_RATE:
        raise ValueError("%s: expected an integer sampling rate in [%d, %d] Hz, got %r" % (what, MIN_RATE, MAX_RATE, sr))
    return int(sr)


def resample(y, orig_sr, target_sr):
    """librosa.resample(y, orig_sr, target_sr) on the GPU: [n] or [..., n] (numpy or torch, any device) -> float32 CUDA tensor
    [..., ceil(n * target_sr / orig_sr)] (``glowk_resample``: one launch for all signals, bitwise reproducible).

    Same filter design as librosa 0.7's default (resampy's ``kaiser_best``: Kaiser-windowed sinc, 64 zero crossings), evaluated at
    the exact tap positions; not bit-compatible with it; derived, not observed.  Rates are integers in [1000, 768000] Hz, at most
    a factor 64 apart.  Equal rates return the input as a float32 tensor where it is, without a launch (as librosa does)."""
    orig_sr, target_sr = _check_rate(orig_sr, "orig_sr"), _check_rate(target_sr, "target_sr")
    if max(orig_sr, target_sr) > 64 * min(orig_sr, target_sr):
        raise ValueError("target_sr: expected within a factor 64 of orig_sr = %d Hz, got %d" % (orig_sr, target_sr))
    x = _tensor(y, "y")
    if x.dim() < 1:
        raise ValueError("y: expected [n] or [..., n] audio, got a scalar")
    if orig_sr == target_sr:
        return x.to(torch.float32)
    x = x.to(device=_device(x), dtype=torch.float32).contiguous()
    lib = _lib.load()
    n, nsig = x.shape[-1], x.numel() // max(x.shape[-1], 1)
    if nsig > 1 << 20:
        raise ValueError("y: expected at most 2^20 signals, got %d" % nsig)
    out = torch.empty(tuple(x.shape[:-1]) + (lib.glowk_resample_length(n, orig_sr, target_sr),), device=x.device, dtype=torch.float32)
    _lib.check(lib.glowk_resample(_p(x), nsig, n, orig_sr, target_sr, _p(out), _s(x)))
    return out


def _wav_format_tag(path):
    """wFormatTag of a RIFF/WAVE file's fmt chunk (1 = PCM, 3 = IEEE float, 0xFFFE = WAVE_FORMAT_EXTENSIBLE)."""
    with open(str(path), "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:] != b"WAVE":
            raise ValueError("%s: not a RIFF/WAVE file" % (path,))
        while True:
            ck = f.read(8)
            if len(ck) < 8:
                raise ValueError("%s: no fmt chunk" % (path,))
            size = struct.unpack("<I", ck[4:])[0]
            if ck[:4] == b"fmt ":
                body = f.read(2)
                if len(body) < 2:
                    raise ValueError("%s: truncated fmt chunk" % (path,))
                return struct.unpack("<H", body)[0]
            f.seek(size + (size & 1), 1)


def load_audio(path, sr=SR, mono=True):
    """librosa.core.load(path, sr=sr, mono=mono) for PCM wavs: 8 (unsigned), 16, 24 or 32 bits at any rate -> ``(y, native_rate)``.
    Samples are scaled to [-1, 1) by 2^(bits - 1); ``mono`` averages the channels (librosa.to_mono), else y is [channels, n].
    ``sr``: the rate y is resampled to on the GPU (``resample``; a float32 CUDA tensor); ``None`` or the file's own rate: no
    resampling, no GPU, a float32 host tensor.  IEEE-float and WAVE_FORMAT_EXTENSIBLE files raise ValueError."""
    if sr is not None:
        sr = _check_rate(sr, "sr")
    tag = _wav_format_tag(path)
    if tag != 1:
        kind = {3: "IEEE float", 0xFFFE: "WAVE_FORMAT_EXTENSIBLE"}.get(tag, "format tag 0x%04x" % tag)
        raise ValueError("%s: only plain PCM wavs are supported (format tag 1), this file is %s" % (path, kind))
    try:
        with wave.open(str(path), "rb") as w:
            rate, ch, width = w.getframerate(), w.getnchannels(), w.getsampwidth()
            raw = w.readframes(w.getnframes())
    except wave.Error as e:
        raise ValueError("%s: not a readable PCM wav (%s)" % (path, e))
    if width not in (1, 2, 3, 4):
        raise ValueError("%s: expected 8, 16, 24 or 32-bit PCM, got a sample width of %d bytes" % (path, width))
    raw = raw[:len(raw) - len(raw) % (width * ch)]
    if width == 1:
        v = np.frombuffer(raw, dtype=np.uint8).astype(np.int64) - 128
    elif width == 3:
        b3 = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
        v = ((b3[:, 0] | (b3[:, 1] << 8) | (b3[:, 2] << 16)) ^ 0x800000) - 0x800000
    else:
        v = np.frombuffer(raw, dtype="<i2" if width == 2 else "<i4").astype(np.int64)
    y = (v.astype(np.float64) / float(1 << (8 * width - 1))).reshape(-1, ch).T          # [channels, n]
    y = torch.from_numpy((y.mean(axis=0) if mono else y).astype(np.float32))
    if sr is not None and sr != rate:
        _check_rate(rate, "%s: sampling rate" % (path,))
        y = resample(y, rate, sr)
    return y, rate


def save_audio(path, y, sr):
    """float [n] or [channels, n] -> 16-bit PCM wav at ``sr`` Hz (round(y * 32767), clipped to [-1, 1] first, like ``write_wav``)."""
    sr = _check_rate(sr, "sr")
    y = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
    if y.ndim not in (1, 2) or (y.ndim == 2 and not 1 <= y.shape[0] <= 65535):
        raise ValueError("y: expected [n] or [channels, n] audio, got %s" % (tuple(y.shape),))
    q = np.rint(np.clip(y.astype(np.float64), -1.0, 1.0) * 32767.0).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if y.ndim == 1 else y.shape[0])
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(q.T).tobytes())              # frames interleave the channels


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


def _check_griffin(n_iter, momentum):
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or not 0 <= n_iter <= 100000:
        raise ValueError("n_iter: expected an integer in [0, 100000], got %r" % (n_iter,))
    if not (isinstance(momentum, (int, float, np.integer, np.floating)) and math.isfinite(momentum) and momentum >= 0):
        raise ValueError("momentum: expected a finite number >= 0, got %r" % (momentum,))
    if momentum > 1:
        warnings.warn("Griffin-Lim with momentum=%g > 1 can be unstable. Proceed with caution!" % momentum)


def _check_init(init, shape):
    """init: 'random', None or a complex tensor of ``shape``; returns the tensor form (or the string / None)."""
    if init is None or (isinstance(init, str) and init == "random"):
        return init
    if isinstance(init, str):
        raise ValueError("init: expected 'random', None or a complex tensor, got %r" % init)
    a = init if torch.is_tensor(init) else torch.as_tensor(np.asarray(init))
    if not a.is_complex() or tuple(a.shape) != tuple(shape):
        raise ValueError("init: expected a complex tensor of shape %s, got %s %s" % (tuple(shape), a.dtype, tuple(a.shape)))
    return a


def griffinlim(S, n_iter=32, momentum=0.99, init="random", seed=0):
    """librosa.griffinlim (center=True, the front end's window and hop): magnitudes [N, 1025, F] -> audio [N, (F - 1) * 512].

    ``init``: 'random' (phases exp(2 pi i U), U ~ U(0, 1) from the device RNG stream ``GRIFFINLIM_STREAM`` of ``seed``, drawn
    over [N, 1025, F]), None (all ones) or a complex [N, 1025, F] tensor used as iteration 0's phases as given.  ``n_iter`` = 0
    is the plain iSTFT of S init.  Needs 4 <= F <= 2^20.  One C call: 2 n_iter + 1 kernels on the current stream."""
    m = _tensor(S, "S")
    if m.dim() != 3 or m.shape[1] != NBIN or not 4 <= m.shape[2] <= GRIFFINLIM_MAX_FRAMES:
        raise ValueError("S: expected [N, 1025, F] magnitudes with 4 <= F <= %d, got %s" % (GRIFFINLIM_MAX_FRAMES, tuple(m.shape)))
    _check_griffin(n_iter, momentum)
    a = _check_init(init, m.shape)
    dev = _device(m, *([a] if torch.is_tensor(a) else []))
    m = m.to(device=dev, dtype=torch.float32).contiguous()
    N, _, F = m.shape
    if isinstance(a, str):
        u = basis.device_randn(tuple(m.shape), dev, seed=seed, which=GRIFFINLIM_STREAM, uniform=True)
        a = torch.exp((2j * math.pi) * u.double()).to(torch.complex64)          # the phases rounded once
    if a is not None:
        a = torch.view_as_real(a.to(device=dev, dtype=torch.complex64)).contiguous()
    out = torch.empty((N, (F - 1) * HOP), device=dev, dtype=torch.float32)
    _lib.check(_lib.load().glowk_griffinlim(_p(m), _p(a), N, F, int(n_iter), float(momentum), _p(out), _s(m)))
    return out


def _whole(x):
    """[N, ..., F] -> [1, ..., N F]: the tiles side by side along the frame axis (np.concatenate(list(x), axis=-1))."""
    return torch.cat(list(x), dim=-1)[None]


def _check_method(method):
    if method not in METHODS:
        raise ValueError("method: expected one of %s, got %r" % (METHODS, method))


def _check_frames(N, F, method):
    """Frames of each signal the iSTFT / Griffin-Lim inverts: F per tile ('frame') or N F ('whole'); 4 .. 2^20 of them."""
    frames = N * F if method == "whole" else F
    if not 4 <= frames <= GRIFFINLIM_MAX_FRAMES:
        raise ValueError("tiles: the %r inversion of %d tiles of %d frames gives signals of %d frames, expected 4 <= frames <= %d"
                         % (method, N, F, frames, GRIFFINLIM_MAX_FRAMES))


def mel_to_audio(tiles, n_iter=32, momentum=0.99, init="random", seed=0, iters=200, method="frame"):
    """librosa.feature.inverse.mel_to_audio of the dB tiles [N, 96, F(, 1)]: NNLS (``iters`` FISTA iterations), square root,
    ``griffinlim``.  ``method='frame'`` inverts each tile on its own -> [N * (F - 1) * 512]; ``'whole'`` inverts the tiles laid side
    by side along time as one signal -> [(N F - 1) * 512].  ``init`` as for ``griffinlim``, of the spectra it inverts: a tensor is
    [N, 1025, F] (concatenated like the tiles for 'whole'); 'random' draws over [N, 1025, F] ('frame') or [1, 1025, N F] ('whole')."""
    t = _tensor(tiles, "tiles")
    _check_tiles(t)
    _check_method(method)
    _check_frames(t.shape[0], t.shape[2], method)
    _check_griffin(n_iter, momentum)
    a = _check_init(init, (t.shape[0], NBIN, t.shape[2]))
    S = torch.sqrt(mel_to_power(t, iters))
    if torch.is_tensor(a) and method == "whole":
        a = _whole(a)
    if method == "whole":
        S = _whole(S)
    return griffinlim(S, n_iter=n_iter, momentum=momentum, init=a, seed=seed).reshape(-1)


def invert(tile_batches, stft_mixture=None, wiener=False, iters=200, algorithm="reuse_phase", method="frame", n_iter=32, momentum=0.99,
           seed=0):
    """melspec_inversion_basis.py: S batches of dB tiles [N, 96, F(, 1)] of one mixture -> S signals.  ``method='frame'`` inverts
    each tile and concatenates the signals -> [S, N * (F - 1) * 512]; ``'whole'`` concatenates the tiles (and the mixture STFTs)
    along time and inverts one signal per source -> [S, (N F - 1) * 512].  One NNLS launch covers the frames of all S batches.

    ``algorithm='reuse_phase'`` needs the mixture's STFT [N, 1025, F] and reuses its phase, or with ``wiener`` (S >= 2) applies
    the single-channel Wiener filter.  ``'griffin'`` needs no mixture: ``mel_to_audio``'s Griffin-Lim (``n_iter``, ``momentum``,
    random phases from ``seed``).  The reuse-phase and Wiener 'whole' inversions are ``griffinlim(n_iter=0)`` of the
    concatenated spectra with init = exp(i angle(X))."""
    if algorithm not in ALGORITHMS:
        raise ValueError("algorithm: expected one of %s, got %r" % (ALGORITHMS, algorithm))
    _check_method(method)
    griffin = algorithm == "griffin"
    if griffin and wiener:
        raise ValueError("wiener: the Wiener filter applies to algorithm='reuse_phase' only")
    if not griffin and stft_mixture is None:
        raise ValueError("stft_mixture: algorithm='reuse_phase' needs the mixture's STFT [N, 1025, F]")
    tiles = [_tensor(t, "tiles") for t in tile_batches]
    if not tiles:
        raise ValueError("tile_batches: expected at least one batch of tiles")
    for t in tiles:
        _check_tiles(t)
    if griffin:
        for t in tiles[1:]:
            if tuple(t.shape[:3]) != tuple(tiles[0].shape[:3]):
                raise ValueError("tiles %s do not match the first batch %s" % (tuple(t.shape), tuple(tiles[0].shape)))
        _check_frames(tiles[0].shape[0], tiles[0].shape[2], method)
        _check_griffin(n_iter, momentum)
        dev = _device(*tiles)
    else:
        X = _tensor(stft_mixture, "stft_mixture")
        for t in tiles:
            if tuple(t.shape[:3]) != (X.shape[0], NMEL, X.shape[-1]):
                raise ValueError("tiles %s do not match stft_mixture %s: expected [N, 96, F] = %s"
                                 % (tuple(t.shape), tuple(X.shape), (X.shape[0], NMEL, X.shape[-1])))
        if wiener and len(tiles) < 2:
            raise ValueError("the Wiener filter needs at least 2 sources, got %d" % len(tiles))
        if method == "whole":
            _check_frames(X.shape[0], X.shape[-1], method)
        dev = _device(X, *tiles)
    batch = torch.cat([t.to(device=dev, dtype=torch.float32).reshape(t.shape[0], NMEL, -1) for t in tiles])
    powers = mel_to_power(batch, iters).reshape(len(tiles), -1, NBIN, batch.shape[2])
    if griffin:
        S = torch.sqrt(powers)
        S = torch.cat([_whole(s) for s in S]) if method == "whole" else S.reshape(-1, NBIN, S.shape[-1])
        y = griffinlim(S, n_iter=n_iter, momentum=momentum, init="random", seed=seed)
    elif method == "frame":
        y = masked_istft(powers, X, wiener)
    else:
        Xw = _whole(X.to(device=dev, dtype=torch.complex64))[0]                   # [1025, N F]
        P = torch.cat([_whole(p) for p in powers])                                  # [S, 1025, N F]
        S = P / (P.sum(0) + 1e-10) * Xw.abs() if wiener else torch.sqrt(P)
        phase = torch.polar(torch.ones_like(Xw.real), Xw.angle())                  # exp(i angle(X)), angle(0) = 0
        y = griffinlim(S, n_iter=0, init=phase.expand(S.shape))
    return y.reshape(len(tiles), -1)


def separate_audio(mix, flow1, flow2, sigmas, restore_1=None, restore_2=None, T=100, delta=2e-5, seed=0, skip=0, n=None, wiener=False,
                   top_db=80.0, iters=200, algorithm="reuse_phase", method="frame", n_iter=32, momentum=0.99):
    """A mixture (wav path or 16 kHz samples) -> two separated signals: ``separate_sources`` with the two flows and the dB mixture
    (start states from device RNG streams 14 / 15 of ``seed``).  Returns ``(y1, y2, mixed, x1, x2)``: the signals ([N * 32256]
    per tile, [(64 N - 1) * 512] for 'whole') and the tiles [N, 96, 64, 1].  ``run_basis_sep.py --inverse`` is
    ``algorithm='griffin', method='whole'``."""
    ys, mixed, xs = separate_sources(mix, [flow1, flow2], sigmas, restores=[restore_1, restore_2], T=T, delta=delta, seed=seed, skip=skip,
                                     n=n, wiener=wiener, top_db=top_db, iters=iters, algorithm=algorithm, method=method, n_iter=n_iter,
                                     momentum=momentum)
    return ys[0], ys[1], mixed, xs[0], xs[1]


def separate_wav(path, flow1, flow2, sigmas, out_rate="input", **kwargs):
    """A PCM wav at any rate -> two separated signals at ``out_rate``: ``load_audio(path, sr=16000)`` (channels averaged, resampled
    on the GPU), ``separate_audio`` on the 16 kHz samples (``kwargs`` are its keyword arguments), the two signals resampled in
    one launch.  ``out_rate``: 'input' (the file's rate), an integer rate, or None (left at 16 kHz).  Returns what
    ``separate_audio`` returns plus the output rate: ``(y1, y2, mixed, x1, x2, rate)``."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = _check_rate(out_rate, "out_rate")
    y, native = load_audio(path, sr=SR, mono=True)
    rate = SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    y1, y2, mixed, x1, x2 = separate_audio(y, flow1, flow2, sigmas, **kwargs)
    y1, y2 = resample(torch.stack([y1, y2]), SR, rate)
    return y1, y2, mixed, x1, x2, rate


def separate_sources(mix, flows, sigmas, restores=None, T=100, delta=2e-5, seed=0, skip=0, n=None, wiener=False, top_db=80.0, iters=200,
                     algorithm="reuse_phase", method="frame", n_iter=32, momentum=0.99, mixing="db"):
    """A mixture (wav path or 16 kHz samples) -> S = len(flows) separated signals, S in [2, 16]: front end,
    ``basis.basis_outer_loop_n`` from the reference's uniform start over [-100, 20] dB (run_basis_sep.py:360-361; source k: device
    RNG stream 14 + (k & 1) of source pair k >> 1 of ``seed``, apart from the Langevin noise's 0 / 1), ``invert`` of the S tile
    batches (its ``algorithm``, ``method``, ``n_iter`` and ``momentum``; Griffin-Lim's phases from ``seed``).  ``restores``: as
    for ``basis_outer_loop_n``.  Returns ``(ys, mixed, xs)``: the signals [S, N * 32256] ([S, (64 N - 1) * 512] for 'whole'), the
    mixture tiles [N, 96, 64, 1] and the separated tiles [S, N, 96, 64, 1]."""
    if algorithm not in ALGORITHMS:
        raise ValueError("algorithm: expected one of %s, got %r" % (ALGORITHMS, algorithm))
    _check_method(method)
    if algorithm == "griffin":
        _check_griffin(n_iter, momentum)
    flows = list(flows)
    if not 2 <= len(flows) <= basis.MAX_SOURCES:
        raise ValueError("flows: expected 2..%d priors, got %d" % (basis.MAX_SOURCES, len(flows)))
    y = read_wav(mix) if isinstance(mix, (str, bytes)) or hasattr(mix, "__fspath__") else mix
    mixed, X = mel_tiles(extracts(y, skip, n), top_db=top_db, return_stft=True)
    xs = [-100.0 + 120.0 * basis.device_randn(tuple(mixed.shape), mixed.device, seed=seed, which=14 + (k & 1), uniform=True, pair=k >> 1)
          for k in range(len(flows))]
    xs, _ = basis.basis_outer_loop_n(mixed, xs, flows, sigmas, restores=restores, T=T, delta=delta, seed=seed, mixing=mixing)
    out = invert(xs, X, wiener=wiener, iters=iters, algorithm=algorithm, method=method, n_iter=n_iter, momentum=momentum, seed=seed)
    return out, mixed, torch.stack(xs)


def separate_wav_sources(path, flows, sigmas, out_rate="input", **kwargs):
    """``separate_wav`` for S priors: a PCM wav at any rate -> S separated signals at ``out_rate`` ('input', an integer rate, or
    None for 16 kHz), all S resampled in one launch.  ``kwargs`` are ``separate_sources``' keyword arguments.  Returns
    ``(ys [S, n'], mixed, xs, rate)``."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = _check_rate(out_rate, "out_rate")
    y, native = load_audio(path, sr=SR, mono=True)
    rate = SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    ys, mixed, xs = separate_sources(y, flows, sigmas, **kwargs)
    return resample(ys, SR, rate), mixed, xs, rate


# ---- stereo: multichannel Wiener filter with EM-fitted spatial covariances ----------------------------------------------------------
def _check_em_iter(n_iter, what="n_iter"):
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or not 0 <= n_iter <= MWF_EM_MAX_ITER:
        raise ValueError("%s: expected an integer in [0, %d], got %r" % (what, MWF_EM_MAX_ITER, n_iter))


def multichannel_wiener(powers, stft_mixture, n_iter=2, return_model=False):
    """Source PSDs [S, N, 1025, F] (>= 0) + stereo mixture STFTs [N, 2, 1025, F] (complex) -> the sources' stereo STFTs
    [S, N, 2, 1025, F] (complex64): the multichannel Wiener filter Y_j = v_j R_j (sum_k v_k R_k + eps I)^-1 x under the local
    Gaussian model, after ``n_iter`` EM iterations on the PSDs v_j(f, t) and the 2 x 2 spatial covariances R_j(f) from R_j = I
    (``glowk_mwf_em``: one launch, one model per problem n, fp64 arithmetic, bitwise reproducible; formulas in include/glowk.h).
    ``n_iter`` = 0 is the single-channel Wiener mask v_j / (sum_k v_k + 1e-10) on each channel.  S in [1, 16], F in [1, 2^20].
    With ``return_model`` also the fitted v [S, N, 1025, F] (float32) and R [S, N, 1025, 2, 2] (complex128).  ``powers`` is not
    modified."""
    p, X = _tensor(powers, "powers"), _tensor(stft_mixture, "stft_mixture")
    if p.dim() != 4 or p.shape[2] != NBIN or not 1 <= p.shape[0] <= basis.MAX_SOURCES or not 1 <= p.shape[3] <= GRIFFINLIM_MAX_FRAMES:
        raise ValueError("powers: expected [S, N, 1025, F] with 1 <= S <= %d and 1 <= F <= %d, got %s"
                         % (basis.MAX_SOURCES, GRIFFINLIM_MAX_FRAMES, tuple(p.shape)))
    if tuple(X.shape) != (p.shape[1], 2, NBIN, p.shape[3]):
        raise ValueError("stft_mixture: expected [N, 2, 1025, F] = %s to match the powers, got %s"
                         % ((p.shape[1], 2, NBIN, p.shape[3]), tuple(X.shape)))
    if p.shape[1] > 1 << 20:
        raise ValueError("powers: expected at most 2^20 problems, got %d" % p.shape[1])
    _check_em_iter(n_iter)
    dev = _device(p, X)
    v = p.to(device=dev, dtype=torch.float32).contiguous()
    if v.data_ptr() == p.data_ptr():
        v = v.clone()                                               # the kernel fits the PSDs in place
    X = torch.view_as_real(X.to(device=dev, dtype=torch.complex64)).contiguous()
    S, N, _, F = v.shape
    Y = torch.empty((S, N, 2, NBIN, F, 2), device=dev, dtype=torch.float32)
    r = torch.empty((S, N, NBIN, 4), device=dev, dtype=torch.float64) if return_model else None
    _lib.check(_lib.load().glowk_mwf_em(_p(X), _p(v), S, N, F, int(n_iter), _p(Y), _p(r), _s(v)))
    Y = torch.view_as_complex(Y)
    if not return_model:
        return Y
    c = torch.complex(r[..., 2], r[..., 3])
    R = torch.stack([torch.complex(r[..., 0], torch.zeros_like(r[..., 0])), c, c.conj(),
                     torch.complex(r[..., 1], torch.zeros_like(r[..., 1]))], dim=-1).reshape(S, N, NBIN, 2, 2)
    return Y, v, R


def istft(Y):
    """Complex STFTs [..., 1025, F] in the front end's convention -> audio [..., (F - 1) * 512] (librosa.istft, center=True),
    through ``griffinlim(|Y|, n_iter=0, init=exp(i angle(Y)))`` as ``invert``'s 'whole' branch.  Needs 4 <= F <= 2^20."""
    if not torch.is_tensor(Y):
        Y = torch.as_tensor(np.asarray(Y))
    if not Y.is_complex() or Y.dim() < 2 or Y.shape[-2] != NBIN or not 4 <= Y.shape[-1] <= GRIFFINLIM_MAX_FRAMES:
        raise ValueError("Y: expected [..., 1025, F] complex STFTs with 4 <= F <= %d, got %s %s" % (GRIFFINLIM_MAX_FRAMES, Y.dtype, tuple(Y.shape)))
    Y = Y.to(device=_device(Y), dtype=torch.complex64)
    lead, F = tuple(Y.shape[:-2]), Y.shape[-1]
    Y = Y.reshape(-1, NBIN, F)
    phase = torch.polar(torch.ones_like(Y.real), Y.angle())                         # exp(i angle(Y)), angle(0) = 0
    return griffinlim(Y.abs(), n_iter=0, init=phase).reshape(lead + ((F - 1) * HOP,))


def _basis_tiles(y, flows, sigmas, restores, T, delta, seed, skip, n, top_db, mixing):
    """The tiles ``separate_sources`` finds for the mono signal y: its front end, start states, RNG streams and loop."""
    mixed, _ = mel_tiles(extracts(y, skip, n), top_db=top_db, return_stft=True)
    xs = [-100.0 + 120.0 * basis.device_randn(tuple(mixed.shape), mixed.device, seed=seed, which=14 + (k & 1), uniform=True, pair=k >> 1)
          for k in range(len(flows))]
    xs, _ = basis.basis_outer_loop_n(mixed, xs, flows, sigmas, restores=restores, T=T, delta=delta, seed=seed, mixing=mixing)
    return mixed, xs


def separate_stereo(mix, flows, sigmas, restores=None, em_iter=2, method="frame", T=100, delta=2e-5, seed=0, skip=0, n=None, top_db=80.0,
                    iters=200, mixing="db"):
    """A stereo mixture (wav path, read by ``load_audio(path, sr=16000, mono=False)``, or [2, n] 16 kHz samples) -> S =
    len(flows) stereo stems.  The priors see the downmix (L + R) / 2: the tiles are those ``separate_sources`` returns for it (same
    start states, RNG streams and ``basis_outer_loop_n``; ``restores``, ``T``, ``delta``, ``seed``, ``skip``, ``n``, ``top_db``,
    ``iters`` and ``mixing`` as there).  Their ``mel_to_power`` spectra are the PSDs ``multichannel_wiener`` starts from, with
    ``em_iter`` EM iterations on the two channels' STFTs, and ``istft`` gives the signals.  ``method='frame'`` fits one model per
    extract and concatenates the signals -> [S, 2, N * 32256]; ``'whole'`` lays tiles and STFTs side by side along time and fits
    one model for the signal -> [S, 2, (64 N - 1) * 512].  Returns ``(ys, mixed, xs)`` with the mixture tiles [N, 96, 64, 1] and
    the separated tiles [S, N, 96, 64, 1] of the downmix."""
    _check_method(method)
    _check_em_iter(em_iter, "em_iter")
    flows = list(flows)
    if not 2 <= len(flows) <= basis.MAX_SOURCES:
        raise ValueError("flows: expected 2..%d priors, got %d" % (basis.MAX_SOURCES, len(flows)))
    y = load_audio(mix, sr=SR, mono=False)[0] if isinstance(mix, (str, bytes)) or hasattr(mix, "__fspath__") else _tensor(mix, "mix")
    if y.dim() != 2 or y.shape[0] != 2:
        raise ValueError("mix: expected [2, n] stereo audio, got %s" % (tuple(y.shape),))
    y = y.to(torch.float32)
    mixed, xs = _basis_tiles((y[0] + y[1]) / 2, flows, sigmas, restores, T, delta, seed, skip, n, top_db, mixing)
    S, N = len(xs), mixed.shape[0]
    _check_frames(N, mixed.shape[2], method)
    powers = mel_to_power(torch.cat([x.reshape(N, NMEL, -1) for x in xs]), iters).reshape(S, N, NBIN, -1)
    _, X = mel_tiles(torch.cat([extracts(y[0], skip, n), extracts(y[1], skip, n)]), top_db=top_db, return_stft=True)
    X = X.reshape(2, N, NBIN, -1).permute(1, 0, 2, 3)                                # [N, 2, 1025, F]
    if method == "whole":
        powers = torch.cat([_whole(p) for p in powers])[:, None]                    # [S, 1, 1025, N F]
        X = _whole(X)                                                                # [1, 2, 1025, N F]
    out = istft(multichannel_wiener(powers, X, n_iter=em_iter))                    # [S, N or 1, 2, samples]
    return out.permute(0, 2, 1, 3).reshape(S, 2, -1), mixed, torch.stack(xs)


def separate_wav_stereo(path, flows, sigmas, out_rate="input", **kwargs):
    """``separate_wav_sources`` for a two-channel PCM wav at any rate -> S stereo stems at ``out_rate`` ('input', an integer rate,
    or None for 16 kHz), all 2 S signals resampled in one launch.  ``kwargs`` are ``separate_stereo``'s keyword arguments.
    Returns ``(ys [S, 2, n'], mixed, xs, rate)``."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = _check_rate(out_rate, "out_rate")
    y, native = load_audio(path, sr=None, mono=False)
    if y.shape[0] != 2:
        raise ValueError("%s: expected a two-channel wav, got %d channel(s); separate_wav_sources takes any channel count and "
                         "averages the channels" % (path, y.shape[0]))
    if native != SR:
        y = resample(y, _check_rate(native, "%s: sampling rate" % (path,)), SR)
    rate = SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    ys, mixed, xs = separate_stereo(y, flows, sigmas, **kwargs)
    return resample(ys, SR, rate), mixed, xs, rate


# ---- whole signals: one STFT, overlapping tiles for the priors, stems as long as the input ------------------------------------------
LONG_MAX_SAMPLES = (GRIFFINLIM_MAX_FRAMES - 1) * HOP     # glowk_mel_frames' cap: 2^20 frames
MAX_TILE_WIDTH = 128                                     # glowk_tile_cut / glowk_tile_stitch: a tile is at most mel_to_power's 128 frames


def _long_audio(y, what="y"):
    """[n] or [C, n] audio with 1024 < n <= LONG_MAX_SAMPLES as a [C, n] tensor where it is."""
    x = _tensor(y, what)
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2 or not 1 <= x.shape[0] <= 1 << 20 or not 1024 < x.shape[1] <= LONG_MAX_SAMPLES:
        raise ValueError("%s: expected [n] or [C, n] audio with 1024 < n <= %d, got %s" % (what, LONG_MAX_SAMPLES, tuple(x.shape)))
    return x


def _check_tiling(width, tile_hop):
    for name, v in (("width", width), ("tile_hop", tile_hop)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s: expected an integer, got %r" % (name, v))
    if not 2 <= width <= MAX_TILE_WIDTH:
        raise ValueError("width: expected a tile width in [2, %d], got %d" % (MAX_TILE_WIDTH, width))
    if not 1 <= tile_hop <= width:
        raise ValueError("tile_hop: expected an integer in [1, width = %d], got %d" % (width, tile_hop))


def _check_long_frames(f, what):
    if f.dim() != 3 or f.shape[1] != NMEL or not 1 <= f.shape[2] <= GRIFFINLIM_MAX_FRAMES:
        raise ValueError("%s: expected [C, 96, F] dB frames with 1 <= F <= %d, got %s" % (what, GRIFFINLIM_MAX_FRAMES, tuple(f.shape)))


def _check_top_db(top_db):
    if not (top_db is None or (isinstance(top_db, (int, float, np.integer, np.floating)) and math.isfinite(top_db))):
        raise ValueError("top_db: expected None or a finite number, got %r" % (top_db,))


def tile_count(n_frames, width=64, tile_hop=32):
    """Tiles of ``width`` frames every ``tile_hop`` frames that cover ``n_frames``: 1 if they fit one tile, else
    1 + ceil((n_frames - width) / tile_hop)."""
    return basis.tile_count(n_frames, width, tile_hop)


def mel_frames(y, return_stft=False):
    """[n] or [C, n] 16 kHz audio of any length n > 1024 -> dB mel frames [C, 96, F] of the whole signal, zero-padded to
    n' = ceil(n / 512) * 512 samples (F = 1 + n' / 512); with ``return_stft`` also its complex STFT [C, 1025, F] (complex64).
    ``mel_tiles``' convention and arithmetic without the per-extract ``top_db`` floor and without its 128-frame limit
    (``glowk_mel_frames``); frame f is centred on sample 512 f of the signal."""
    x = _long_audio(y)
    x = x.to(device=_device(x), dtype=torch.float32)
    C, n = x.shape
    x = torch.nn.functional.pad(x, (0, -n % HOP)).contiguous()
    F = 1 + x.shape[1] // HOP
    mel = torch.empty((C, NMEL, F), device=x.device, dtype=torch.float32)
    X = torch.empty((C, NBIN, F, 2), device=x.device, dtype=torch.float32) if return_stft else None
    _lib.check(_lib.load().glowk_mel_frames(_p(x), C, x.shape[1], _p(mel), _p(X), _s(x)))
    return (mel, torch.view_as_complex(X)) if return_stft else mel


def frame_tiles(frames, width=64, tile_hop=32, top_db=80.0):
    """dB frames [C, 96, F] (or [96, F]) -> overlapping tiles [C, N, 96, width, 1], N = ``tile_count(F, width, tile_hop)``: tile k
    holds frames [k tile_hop, k tile_hop + width), -100 dB past the end.  ``top_db`` (None or 0: none): ``mel_tiles``' floor per
    tile, max over the padded tile - top_db; every cell is clipped to [-100, 20] (``glowk_tile_cut``)."""
    f = _tensor(frames, "frames")
    if f.dim() == 2:
        f = f[None]
    _check_long_frames(f, "frames")
    _check_tiling(width, tile_hop)
    _check_top_db(top_db)
    f = f.to(device=_device(f), dtype=torch.float32).contiguous()
    C, _, F = f.shape
    out = torch.empty((C, tile_count(F, width, tile_hop), NMEL, width, 1), device=f.device, dtype=torch.float32)
    _lib.check(_lib.load().glowk_tile_cut(_p(f), C, F, int(width), int(tile_hop), float(top_db or 0.0), _p(out), _s(f)))
    return out


def stitch_tiles(tiles, n_frames, tile_hop=32):
    """Overlapping tiles [C, N, 96, width(, 1)] -> frames [C, 96, n_frames]: each frame the mean, in dB, of the tiles that cover
    it, weighted by w[j] = sin^2(pi (j + 1/2) / width) at its position j in each (``glowk_tile_stitch``; the weights of a frame sum
    to 1 at tile_hop = width / 2).  A frame one tile covers is that tile's value, bit for bit.  n_frames <= (N - 1) tile_hop +
    width.  Inverse of ``frame_tiles(..., top_db=None)`` on frames within [-100, 20]."""
    t = _tensor(tiles, "tiles")
    if t.dim() == 5 and t.shape[4] == 1:
        t = t[..., 0]
    if t.dim() != 4 or t.shape[2] != NMEL or not 1 <= t.shape[1] <= GRIFFINLIM_MAX_FRAMES:
        raise ValueError("tiles: expected [C, N, 96, width] or [C, N, 96, width, 1] dB tiles, got %s" % (tuple(tiles.shape),))
    C, N, _, width = t.shape
    _check_tiling(width, tile_hop)
    if isinstance(n_frames, bool) or not isinstance(n_frames, (int, np.integer)) or not 1 <= n_frames <= min(GRIFFINLIM_MAX_FRAMES, (N - 1) * tile_hop + width):
        raise ValueError("n_frames: expected an integer in [1, (N - 1) tile_hop + width = %d], got %r" % ((N - 1) * tile_hop + width, n_frames))
    t = t.to(device=_device(t), dtype=torch.float32).contiguous()
    out = torch.empty((C, NMEL, int(n_frames)), device=t.device, dtype=torch.float32)
    _lib.check(_lib.load().glowk_tile_stitch(_p(t), C, N, width, int(tile_hop), int(n_frames), _p(out), _s(t)))
    return out


def _check_long_inversion(S, F, X, n, wiener, what):
    """The mixture STFT [1025, F] (mono) or [2, 1025, F] (stereo) of S sources' F frames and the output length n; True if stereo."""
    if tuple(X.shape) not in ((NBIN, F), (2, NBIN, F)):
        raise ValueError("stft_mixture: expected [1025, F] or [2, 1025, F] with F = %d to match the %s, got %s" % (F, what, tuple(X.shape)))
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= (F - 1) * HOP:
        raise ValueError("n: expected an integer in [1, (F - 1) * 512 = %d], got %r" % ((F - 1) * HOP, n))
    if X.dim() == 2 and wiener and S < 2:
        raise ValueError("the Wiener filter needs at least 2 sources, got %d" % S)
    return X.dim() == 3


def mask_istft_long(powers, stft_mixture, n, wiener=False, em_iter=2):
    """Power spectra [S, 1025, F] of S sources + the whole mixture's STFT -> their signals, trimmed to the first n samples.
    Mono, ``stft_mixture`` [1025, F]: the mixture's phase reused, or with ``wiener`` (S >= 2) the single-channel Wiener filter, as
    ``invert``'s 'whole' branch -> [S, n].  Stereo, [2, 1025, F]: ``multichannel_wiener(..., n_iter=em_iter)`` as one problem, then
    ``istft`` -> [S, 2, n] (always a Wiener filter; ``wiener`` is not consulted).  4 <= F <= 2^20, n <= (F - 1) * 512."""
    p, X = _tensor(powers, "powers"), _tensor(stft_mixture, "stft_mixture")
    if p.dim() != 3 or p.shape[1] != NBIN or not 1 <= p.shape[0] <= basis.MAX_SOURCES or not 4 <= p.shape[2] <= GRIFFINLIM_MAX_FRAMES:
        raise ValueError("powers: expected [S, 1025, F] with 1 <= S <= %d and 4 <= F <= %d, got %s"
                         % (basis.MAX_SOURCES, GRIFFINLIM_MAX_FRAMES, tuple(p.shape)))
    stereo = _check_long_inversion(p.shape[0], p.shape[2], X, n, wiener, "powers")
    _check_em_iter(em_iter, "em_iter")
    dev = _device(p, X)
    P, Xw = p.to(device=dev, dtype=torch.float32), X.to(device=dev, dtype=torch.complex64)
    if stereo:
        y = istft(multichannel_wiener(P[:, None], Xw[None], n_iter=em_iter)[:, 0])       # [S, 2, (F - 1) * 512]
    else:
        S = P / (P.sum(0) + 1e-10) * Xw.abs() if wiener else torch.sqrt(P)
        phase = torch.polar(torch.ones_like(Xw.real), Xw.angle())                       # exp(i angle(X)), angle(0) = 0
        y = griffinlim(S, n_iter=0, init=phase.expand(S.shape))
    return y[..., :int(n)].contiguous()


def invert_frames(frames, stft_mixture, n, wiener=False, iters=200, em_iter=2):
    """dB frames [S, 96, F] of S sources of one signal + the mixture's STFT ([1025, F], or [2, 1025, F] for stereo) -> their
    signals [S, n] ([S, 2, n]): ``mel_to_power`` (per frame; the frames go through it as tiles of at most 128), then
    ``mask_istft_long``.  n <= (F - 1) * 512: the samples ``mel_frames`` padded are trimmed."""
    f, X = _tensor(frames, "frames"), _tensor(stft_mixture, "stft_mixture")
    _check_long_frames(f, "frames")
    if not 1 <= f.shape[0] <= basis.MAX_SOURCES or f.shape[2] < 4:
        raise ValueError("frames: expected [S, 96, F] with 1 <= S <= %d and F >= 4, got %s" % (basis.MAX_SOURCES, tuple(f.shape)))
    _check_long_inversion(f.shape[0], f.shape[2], X, n, wiener, "frames")
    _check_em_iter(em_iter, "em_iter")
    f = f.to(device=_device(f, X), dtype=torch.float32)
    S, _, F = f.shape
    nt = -(-F // MAX_TILE_WIDTH)
    w = -(-F // nt)                                                                       # nt tiles of w <= 128 frames hold F
    t = torch.nn.functional.pad(f, (0, nt * w - F), value=-100.0).reshape(S, NMEL, nt, w).permute(0, 2, 1, 3).reshape(S * nt, NMEL, w)
    p = mel_to_power(t, iters).reshape(S, nt, NBIN, w).permute(0, 2, 1, 3).reshape(S, NBIN, nt * w)[:, :, :F]
    return mask_istft_long(p, X, n, wiener=wiener, em_iter=em_iter)


def _tile_width(flows):
    """The tile width W the priors share: every flow's data shape must be [96, W, 1] with 2 <= W <= 128."""
    shapes = [tuple(int(d) for d in getattr(fl, "event_shape", ())) for fl in flows]
    s0 = shapes[0]
    if len(s0) != 3 or s0[0] != NMEL or s0[2] != 1 or not 2 <= s0[1] <= MAX_TILE_WIDTH or any(s != s0 for s in shapes):
        raise ValueError("flows: expected priors of one data shape [96, W, 1] with 2 <= W <= %d, got %s" % (MAX_TILE_WIDTH, shapes))
    return s0[1]


def separate_long(mix, flows, sigmas, restores=None, tile_hop=32, T=100, delta=2e-5, seed=0, top_db=80.0, iters=200, wiener=True,
                  em_iter=2, mixing="db", coupled=False):
    """A whole mixture (wav path, [n] mono or [2, n] stereo 16 kHz samples, n > 1024) -> S = len(flows) stems exactly as long as
    it and aligned with it, S in [2, 16].  One STFT of the signal (``mel_frames``; stereo: of both channels and of the downmix
    (L + R) / 2, which is what the priors see); tiles of the priors' width W every ``tile_hop`` frames with the per-tile ``top_db``
    floor (``frame_tiles``); ``basis.basis_outer_loop_n`` on them from ``separate_sources``' start states and RNG streams;
    the separated tiles cross-faded into frames (``stitch_tiles``); ``invert_frames`` (``wiener``, ``iters``; stereo: ``em_iter``
    EM iterations of the multichannel Wiener filter, one model for the signal).  The priors see independent tiles: only their
    estimates are cross-faded.
    ``coupled=True`` runs ONE chain over the whole signal instead (``basis.basis_outer_loop_frames``): the state is the signal's
    frames, the priors see its overlapping tiles, and a frame's prior score is the cross-fade of the scores of the tiles that
    cover it, so the tiles are coupled inside the Langevin loop and nothing is stitched afterwards.  The mixture's frames are
    floored once over the whole signal (max - ``top_db``, clipped to [-100, 20]; None or 0: no floor), the start states are
    -100 + 120 U in the frame layout from the streams of ``separate_sources``, and ``source_frames`` is the chain's result.
    Returns ``(ys, mixed_frames, source_frames)``: [S, n] (stereo [S, 2, n]), the mixture's (downmix's) unfloored frames [96, F]
    and the separated frames [S, 96, F], F = 1 + ceil(n / 512)."""
    flows = list(flows)
    if not 2 <= len(flows) <= basis.MAX_SOURCES:
        raise ValueError("flows: expected 2..%d priors, got %d" % (basis.MAX_SOURCES, len(flows)))
    W = _tile_width(flows)
    _check_tiling(W, tile_hop)
    _check_em_iter(em_iter, "em_iter")
    if not isinstance(coupled, bool):
        raise ValueError("coupled: expected True or False, got %r" % (coupled,))
    if isinstance(mix, (str, bytes)) or hasattr(mix, "__fspath__"):
        y = load_audio(mix, sr=SR, mono=False)[0]
        y = y[0] if y.shape[0] == 1 else y
    else:
        y = _tensor(mix, "mix")
    if not (y.dim() == 1 or (y.dim() == 2 and y.shape[0] == 2)) or not 1024 < y.shape[-1] <= LONG_MAX_SAMPLES:
        raise ValueError("mix: expected [n] mono or [2, n] stereo audio with 1024 < n <= %d, got %s" % (LONG_MAX_SAMPLES, tuple(y.shape)))
    stereo, n = y.dim() == 2, y.shape[-1]
    y = y.to(device=_device(y), dtype=torch.float32)
    mel, X = mel_frames(torch.stack([y[0], y[1], (y[0] + y[1]) / 2]) if stereo else y, return_stft=True)
    mixed_frames = mel[-1]
    if coupled:
        _check_top_db(top_db)
        floored = torch.maximum(mixed_frames, mixed_frames.max() - float(top_db)) if top_db else mixed_frames
        xs = torch.stack([-100.0 + 120.0 * basis.device_randn(tuple(mixed_frames.shape), mixed_frames.device, seed=seed, which=14 + (k & 1),
                                                              uniform=True, pair=k >> 1) for k in range(len(flows))])
        source_frames, _ = basis.basis_outer_loop_frames(floored.clamp(-100.0, 20.0), xs, flows, sigmas, W, tile_hop, restores=restores,
                                                         T=T, delta=delta, seed=seed, mixing=mixing)
        ys = invert_frames(source_frames, X[:2] if stereo else X[0], n, wiener=wiener, iters=iters, em_iter=em_iter)
        return ys, mixed_frames, source_frames
    mixed = frame_tiles(mixed_frames, W, tile_hop, top_db)[0]                             # [N, 96, W, 1]
    xs = [-100.0 + 120.0 * basis.device_randn(tuple(mixed.shape), mixed.device, seed=seed, which=14 + (k & 1), uniform=True, pair=k >> 1)
          for k in range(len(flows))]
    xs, _ = basis.basis_outer_loop_n(mixed, xs, flows, sigmas, restores=restores, T=T, delta=delta, seed=seed, mixing=mixing)
    source_frames = stitch_tiles(torch.stack(xs), mixed_frames.shape[1], tile_hop)
    ys = invert_frames(source_frames, X[:2] if stereo else X[0], n, wiener=wiener, iters=iters, em_iter=em_iter)
    return ys, mixed_frames, source_frames


def separate_wav_long(path, flows, sigmas, out_rate="input", mono=False, **kwargs):
    """``separate_long`` for a PCM wav at any rate -> S stems at ``out_rate`` ('input', an integer rate, or None for 16 kHz), all
    resampled in one launch.  A two-channel file gives stereo stems unless ``mono``; any other channel count is averaged.  With
    ``out_rate='input'`` the stems have exactly the file's sample count (the round trip through 16 kHz gives at least as many;
    the excess is trimmed).  ``kwargs`` are ``separate_long``'s keyword arguments.  Returns ``(ys [S, n'] or [S, 2, n'],
    mixed_frames, source_frames, rate)``."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = _check_rate(out_rate, "out_rate")
    y, native = load_audio(path, sr=None, mono=False)
    n_file = y.shape[1]
    if y.shape[0] != 2 or mono:
        y = y.mean(0)
    if native != SR:
        y = resample(y, _check_rate(native, "%s: sampling rate" % (path,)), SR)
    rate = SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    ys, mixed_frames, source_frames = separate_long(y, flows, sigmas, **kwargs)
    ys = resample(ys, SR, rate)
    if isinstance(out_rate, str):
        ys = ys[..., :n_file].contiguous()
    return ys, mixed_frames, source_frames, rate
