"""Harmonic / percussive source separation by median filtering (Fitzgerald 2010), with the surface and semantics of
``librosa.decompose.hpss`` / ``librosa.effects.hpss``: the prior-free baseline.  It needs no trained flows and no ground-truth stems
-- a wav in, two stems out -- and gives the BASIS figures a lower bound, as the oracle systems of ``oracle_systems.py`` give them
upper ones.  Not in the reference.

Kernels in ``csrc/glowk_hpss.h`` (``glowk_median_filter``, ``glowk_hpss_mask``; formulas in include/glowk.h):

* ``median_filter``: the running median of odd length along the frames or the rows of [rows, F] spectra, edges as
  ``scipy.ndimage.median_filter(mode='reflect')``.  The median is a selection, so the result equals a sort's bit for bit;
* ``hpss``: ``librosa.decompose.hpss`` -- the harmonic filter along the frames, the percussive one along the rows, the two soft
  masks of ``librosa.util.softmask`` (fp32), the masked spectra (complex input keeps its phase);
* ``hpss_audio``: 16 kHz audio in, stems as long as it out: ``audio.mel_frames``' STFT, ``hpss`` on |X| per channel, the masked
  magnitudes with the mixture's phase through ``audio.griffinlim(n_iter=0)`` -- ``audio.mask_istft_long``'s mono branch;
* ``separate_wav_hpss``: a PCM wav at any rate in, the stems at the file's rate and length out, like ``audio.separate_wav_long``.

Conventions as in ``audio.py``: numpy or torch in, a float32 tensor on the GPU the input lives on (the current one for host input)
out, ValueError for bad arguments before the library is loaded.  Even kernel sizes are not supported.
"""
import math

import numpy as np
import torch

from . import _lib, audio
from .audio import _p, _s

MAX_SIZE = 127                                           # glowk_median_filter: size odd in [1, 127]
MAX_ROWS, MAX_FRAMES, MAX_SIGNALS = 4096, 1 << 20, 65535
MAX_ELEMENTS = (1 << 31) - 1
AXES = {0: 0, 1: 1, "frames": 0, "rows": 1}              # the C ABI's axis: 0 along the frames (harmonic), 1 along the rows


def _check_size(size, what="size"):
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 1 <= size <= MAX_SIZE or size % 2 == 0:
        raise ValueError("%s: expected an odd integer in [1, %d], got %r" % (what, MAX_SIZE, size))
    return int(size)


def _pair(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError("%s: expected a scalar or a (harmonic, percussive) pair, got %r" % (what, v))
        return v[0], v[1]
    return v, v


def _check_params(kernel_size, power, margin):
    """(size_h, size_p), power, (margin_h, margin_p) of ``hpss``, checked."""
    kh, kp = _pair(kernel_size, "kernel_size")
    sizes = _check_size(kh, "kernel_size"), _check_size(kp, "kernel_size")
    margins = _pair(margin, "margin")
    for m in margins:
        if isinstance(m, bool) or not isinstance(m, (int, float, np.integer, np.floating)) or not (math.isfinite(m) and m >= 1):
            raise ValueError("margin: expected finite numbers >= 1, got %r" % (margin,))
    if isinstance(power, bool) or not isinstance(power, (int, float, np.integer, np.floating)) or not power > 0:
        raise ValueError("power: expected a number > 0 (inf: the hard mask), got %r" % (power,))
    return sizes, float(power), (float(margins[0]), float(margins[1]))


def _spectra(S, what="S"):
    """[rows, F] or [N, rows, F] within glowk_median_filter's ranges, as a tensor where it is."""
    x = S if torch.is_tensor(S) else torch.as_tensor(np.asarray(S))
    if x.dim() not in (2, 3) or not 1 <= x.shape[-2] <= MAX_ROWS or not 1 <= x.shape[-1] <= MAX_FRAMES \
            or (x.dim() == 3 and x.shape[0] > MAX_SIGNALS) or x.numel() > MAX_ELEMENTS:
        raise ValueError("%s: expected [rows, F] or [N, rows, F] with N <= %d, 1 <= rows <= %d, 1 <= F <= %d and at most 2^31 - 1 "
                         "elements, got %s" % (what, MAX_SIGNALS, MAX_ROWS, MAX_FRAMES, tuple(x.shape)))
    return x


def _median(x, size, axis):
    """x: float32 contiguous [.., rows, F] on the GPU."""
    out = torch.empty_like(x)
    nsig = x.numel() // (x.shape[-2] * x.shape[-1])
    _lib.check(_lib.load().glowk_median_filter(_p(x), nsig, x.shape[-2], x.shape[-1], size, axis, _p(out), _s(x)))
    return out


def median_filter(S, size, axis):
    """The running median of odd length ``size`` in [1, 127] of real spectra [rows, F] or [N, rows, F] along ``axis``: 'frames' or
    0 (the harmonic filter; the last array axis), 'rows' or 1 (the percussive filter; the axis before it) -- the C ABI's numbering.
    Edges as ``scipy.ndimage.median_filter(mode='reflect')``; the result equals a sort's bit for bit (``glowk_median_filter``: one
    launch, bitwise reproducible, a batch gives what its signals give alone).  float32 out, shaped like S."""
    size = _check_size(size)
    if isinstance(axis, bool) or not isinstance(axis, (int, str, np.integer)) or axis not in AXES:
        raise ValueError("axis: expected 'frames' (0) or 'rows' (1), got %r" % (axis,))
    x = _spectra(S)
    if x.is_complex():
        raise ValueError("S: expected real spectra, got %s" % x.dtype)
    x = x.to(device=audio._device(x), dtype=torch.float32).contiguous()
    return _median(x, size, AXES[axis])


def hpss(S, kernel_size=31, power=2.0, mask=False, margin=1.0):
    """``librosa.decompose.hpss``: spectra [rows, F] or [N, rows, F] -> ``(harmonic, percussive)`` shaped like S.

    The harmonic filter is the median of ``kernel_size`` frames along time, the percussive one of ``kernel_size`` rows along
    frequency; the masks are ``librosa.util.softmask`` of each against the other times its ``margin`` with exponent ``power``
    (inf: the hard mask), in fp32 (``glowk_hpss_mask``).  ``kernel_size`` (odd, in [1, 127]) and ``margin`` (>= 1) are a scalar or
    a (harmonic, percussive) pair.  Complex S is split into magnitude and phase, and the components come back complex64 with S's
    phase; real S gives float32 magnitudes.  ``mask=True`` returns the two masks instead.  With a margin above 1 the components no
    longer sum to S.  Three launches."""
    (kh, kp), power, (mh, mp) = _check_params(kernel_size, power, margin)
    if not isinstance(mask, (bool, np.bool_)):
        raise ValueError("mask: expected True or False, got %r" % (mask,))
    x = _spectra(S)
    dev = audio._device(x)
    phase = None
    if x.is_complex():
        x = x.to(device=dev, dtype=torch.complex64)
        phase = torch.polar(torch.ones_like(x.real), x.angle())                          # exp(i angle(S)), angle(0) = 0
        x = x.abs()
    x = x.to(device=dev, dtype=torch.float32).contiguous()
    harm, perc = _median(x, kh, 0), _median(x, kp, 1)
    out_h, out_p = torch.empty_like(x), torch.empty_like(x)
    _lib.check(_lib.load().glowk_hpss_mask(_p(harm), _p(perc), None if mask else _p(x), x.numel(), power, mh, mp, _p(out_h), _p(out_p),
                                           _s(x)))
    if mask or phase is None:
        return out_h, out_p
    return out_h * phase, out_p * phase


def hpss_audio(y, kernel_size=31, power=2.0, margin=1.0, residual=False):
    """``librosa.effects.hpss`` for 16 kHz audio [n] or [C, n], n > 1024 -> ``(harmonic, percussive)``, each shaped like y and
    aligned with it; with ``residual`` also ``y - harmonic - percussive`` (non-trivial only with a margin above 1).  One STFT of
    the whole signal (``audio.mel_frames``), ``hpss`` on |X| per channel, the masked magnitudes with the mixture's phase through
    one ``audio.griffinlim(n_iter=0)`` of all 2 C spectra, trimmed to n samples.  A channel's stems depend on that channel alone."""
    _check_params(kernel_size, power, margin)
    if not isinstance(residual, (bool, np.bool_)):
        raise ValueError("residual: expected True or False, got %r" % (residual,))
    t = audio._tensor(y, "y")
    x = audio._long_audio(t)
    if x.shape[0] > MAX_SIGNALS:
        raise ValueError("y: expected at most %d channels, got %d" % (MAX_SIGNALS, x.shape[0]))
    lead, n = tuple(t.shape[:-1]), x.shape[1]
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [C, 1025, F]
    mags = torch.cat(hpss(X.abs(), kernel_size=kernel_size, power=power, margin=margin))  # [2 C, 1025, F]
    phase = torch.polar(torch.ones_like(X.real), X.angle())
    stems = audio.griffinlim(mags, n_iter=0, init=torch.cat([phase, phase]))[:, :n].reshape((2,) + lead + (n,))
    h, p = stems[0].contiguous(), stems[1].contiguous()
    return (h, p, x.reshape(lead + (n,)) - h - p) if residual else (h, p)


def separate_wav_hpss(path, out_rate="input", mono=False, **kwargs):
    """``hpss_audio`` for a PCM wav at any rate -> ``(stems, rate)``: stems [2, n'] (harmonic, percussive; [3, n'] with
    ``residual=True``) of a one-channel file or with ``mono`` (the channels averaged), else [2 or 3, C, n'] with the file's C
    channels, at ``out_rate``: 'input' (the file's rate), an integer rate, or None (left at 16 kHz).  The file is resampled to 16 kHz
    on the GPU, the stems back in one launch; with ``out_rate='input'`` they have exactly the file's sample count (the round trip
    through 16 kHz gives at least as many; the excess is trimmed).  ``kwargs`` are ``hpss_audio``'s keyword arguments."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    unknown = set(kwargs) - {"kernel_size", "power", "margin", "residual"}
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected hpss_audio's" % sorted(unknown))
    _check_params(kwargs.get("kernel_size", 31), kwargs.get("power", 2.0), kwargs.get("margin", 1.0))
    y, native = audio.load_audio(path, sr=None, mono=False)
    n_file = y.shape[1]
    y = y.mean(0) if mono or y.shape[0] == 1 else y
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    stems = audio.resample(torch.stack(hpss_audio(y, **kwargs)), audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate
