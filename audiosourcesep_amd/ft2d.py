"""2DFT separation (Seetharaman, Pishdadian & Pardo, WASPAA 2017; ``FT2D`` in nussl, "original" filter approach): a repeating
background as the peaks of the 2-D Fourier transform of the magnitude spectrogram.  Anything that repeats along time -- at any
period, several periods at once -- collapses into isolated peaks of that plane; the background is the inverse transform of the
peaks, the foreground the rest.  Unlike ``repet`` it needs no period range, window or step: it is the prior-free baseline for a
file whose tempo nobody knows.  Not in the reference.

Kernels in ``csrc/glowk_dft2.h`` (formulas and error bounds in include/glowk.h); the masks are ``glowk_hpss_mask``:

* ``rfft2`` / ``irfft2``: ``numpy.fft.rfft2`` and ``irfft2`` of real planes as two twiddle GEMMs each on the fp32 matrix cores
  (no FFT: 1025 = 5^2 41 and 5626 = 2 29 97), the inverse with an optional mask multiplied in on load;
* ``plane_std``: mean and population standard deviation in fp64, fixed order;
* ``peak_mask``: 1 where a cell is the maximum of its periodic neighbourhood and the neighbourhood's range exceeds a threshold --
  ``scipy.ndimage.maximum_filter`` / ``minimum_filter(mode='wrap')``, bit for bit.  nussl filters the shifted plane with scipy's
  ``reflect`` edge and then symmetrises by flips; the plane is periodic, so wrap is the edge that needs no repair;
* ``ft2d``: ``F = rfft2(|S|)``, ``thr = threshold_scale std(|F|)``, ``M = peaks``, ``B = irfft2(F M)``, ``rep = |B|``,
  ``res = ||S| - B|`` (the foreground's own inverse, by linearity), the two soft masks of ``repet``;
* ``ft2d_audio`` / ``separate_wav_ft2d``: the audio and wav paths, line for line those of ``repet.repet_audio``.

Conventions as in ``repet.py``: numpy or torch in, float32 tensors on the GPU the input lives on out, ValueError for bad arguments
before the library is loaded.
"""
import math

import numpy as np
import torch

from . import _lib, audio
from .audio import _p, _s
from .repet import MAX_FRAMES, MAX_SIGNALS, _check_flag, _check_mask_params, _magnitude, _nsig, _real32, _spectra

MAX_NEIGHBORHOOD = 127


def _check_neighborhood(neighborhood):
    """(nb_r, nb_c): two odd integers in [1, 127]."""
    if not isinstance(neighborhood, (tuple, list)) or len(neighborhood) != 2:
        raise ValueError("neighborhood: expected a (rows, frames) pair of odd integers in [1, %d], got %r" % (MAX_NEIGHBORHOOD, neighborhood))
    for v in neighborhood:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_NEIGHBORHOOD or v % 2 == 0:
            raise ValueError("neighborhood: expected a (rows, frames) pair of odd integers in [1, %d], got %r"
                             % (MAX_NEIGHBORHOOD, tuple(neighborhood)))
    return int(neighborhood[0]), int(neighborhood[1])


def _check_scale(threshold_scale):
    if isinstance(threshold_scale, (bool, np.bool_)) or not isinstance(threshold_scale, (int, float, np.integer, np.floating)) \
            or not (math.isfinite(threshold_scale) and threshold_scale >= 0):
        raise ValueError("threshold_scale: expected a finite number >= 0, got %r" % (threshold_scale,))
    return float(threshold_scale)


def _work(nbytes, dev):
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)


def _rdft2(x, want_mag):
    """x: float32 contiguous [.., rows, T] on the GPU -> (spec complex64 [.., rows, fc], mag float32 like x or None)."""
    lib = _lib.load()
    rows, T = x.shape[-2], x.shape[-1]
    nsig = _nsig(x)
    spec = torch.empty(tuple(x.shape[:-1]) + (T // 2 + 1,), dtype=torch.complex64, device=x.device)
    mag = torch.empty_like(x) if want_mag else None
    nbytes = lib.glowk_dft2_workspace_bytes(nsig, rows, T)
    work = _work(nbytes, x.device)
    _lib.check(lib.glowk_rdft2(_p(x), nsig, rows, T, _p(spec), None if mag is None else _p(mag), _p(work), nbytes, _s(x)))
    return spec, mag


def _irdft2(spec, mask, T):
    lib = _lib.load()
    rows = spec.shape[-2]
    nsig = spec.numel() // (rows * spec.shape[-1])
    out = torch.empty(tuple(spec.shape[:-1]) + (T,), dtype=torch.float32, device=spec.device)
    nbytes = lib.glowk_dft2_workspace_bytes(nsig, rows, T)
    work = _work(nbytes, spec.device)
    _lib.check(lib.glowk_irdft2(_p(spec), None if mask is None else _p(mask), nsig, rows, T, _p(out), _p(work), nbytes, _s(spec)))
    return out


def _plane_std(x):
    """x: float32 contiguous [.., rows, T] on the GPU -> float64 [.., 2]: mean and population std of each plane."""
    lib = _lib.load()
    n = x.shape[-2] * x.shape[-1]
    nsig = _nsig(x)
    out = torch.empty(tuple(x.shape[:-2]) + (2,), dtype=torch.float64, device=x.device)
    nbytes = lib.glowk_plane_std_workspace_bytes(nsig, n)
    work = _work(nbytes, x.device)
    _lib.check(lib.glowk_plane_std(_p(x), nsig, n, _p(out), _p(work), nbytes, _s(x)))
    return out


def _peak_mask(x, nb, thr, want_extrema=False):
    """x: float32 contiguous [.., rows, cols] on the GPU, thr float32 [..] on it or None -> mask (, max, min)."""
    lib = _lib.load()
    rows, cols = x.shape[-2], x.shape[-1]
    nsig = _nsig(x)
    mask = torch.empty_like(x)
    mx, mn = (torch.empty_like(x), torch.empty_like(x)) if want_extrema else (None, None)
    nbytes = lib.glowk_peak_workspace_bytes(nsig, rows, cols)
    work = _work(nbytes, x.device)
    _lib.check(lib.glowk_peak_mask(_p(x), nsig, rows, cols, nb[0], nb[1], None if thr is None else _p(thr), _p(mask),
                                   None if mx is None else _p(mx), None if mn is None else _p(mn), _p(work), nbytes, _s(x)))
    return (mask, mx, mn) if want_extrema else mask


def rfft2(S, return_magnitude=False):
    """``numpy.fft.rfft2`` of real planes [rows, T] or [N, rows, T] -> complex64 [.., rows, T // 2 + 1]; with
    ``return_magnitude`` also the full Hermitian plane of magnitudes, float32 shaped like S (its mirrored columns are bitwise
    copies).  ``glowk_rdft2``: four or five launches, bitwise reproducible, a batch gives what its signals give alone."""
    want = _check_flag(return_magnitude, "return_magnitude")
    spec, mag = _rdft2(_real32(S), want)
    return (spec, mag) if want else spec


def irfft2(F, frames, mask=None):
    """``numpy.fft.irfft2(F * mask[..., :fc], s=(rows, frames))`` of half spectra [rows, fc] or [N, rows, fc], fc = frames // 2 + 1
    -> float32 [.., rows, frames].  ``mask`` (optional) is a full real plane [.., rows, frames] of which the first fc columns are
    used; it is multiplied in as F is loaded.  ``glowk_irdft2``: four launches."""
    if isinstance(frames, (bool, np.bool_)) or not isinstance(frames, (int, np.integer)) or not 1 <= frames <= MAX_FRAMES:
        raise ValueError("frames: expected an integer in [1, %d], got %r" % (MAX_FRAMES, frames))
    frames = int(frames)
    f = F if torch.is_tensor(F) else torch.as_tensor(np.asarray(F))
    if f.dim() not in (2, 3) or f.shape[-1] != frames // 2 + 1:
        raise ValueError("F: expected [rows, %d] or [N, rows, %d] for frames = %d, got %s" % (frames // 2 + 1, frames // 2 + 1, frames, tuple(f.shape)))
    shape = tuple(f.shape[:-1]) + (frames,)
    _spectra(torch.empty(shape, device="meta"), "F")                                    # the ranges of the full plane
    m = None
    if mask is not None:
        m = mask if torch.is_tensor(mask) else torch.as_tensor(np.asarray(mask))
        if tuple(m.shape) != shape or m.is_complex():
            raise ValueError("mask: expected a real plane shaped %s, got %s %s" % (shape, m.dtype, tuple(m.shape)))
    dev = audio._device(f)
    f = f.to(device=dev, dtype=torch.complex64).contiguous()
    if m is not None:
        m = m.to(device=dev, dtype=torch.float32).contiguous()
    return _irdft2(f, m, frames)


def peak_mask(P, neighborhood=(1, 25), threshold=None, return_extrema=False):
    """The peaks of real planes [rows, cols] or [N, rows, cols] -> float32 0 / 1 shaped like P: 1 where the cell equals the maximum
    ``mx`` of its periodic ``neighborhood`` (rows, cols; odd, at most 127; indices wrap) and ``mx - mn > threshold`` with ``mn`` the
    minimum -- ``scipy.ndimage.maximum_filter`` / ``minimum_filter(size=neighborhood, mode='wrap')``.  ``threshold``: None (no
    test), a number, or one number per plane [N].  With ``return_extrema`` also ``mx`` and ``mn``, which carry P's bits.
    ``glowk_peak_mask``: two launches."""
    nb = _check_neighborhood(neighborhood)
    want = _check_flag(return_extrema, "return_extrema")
    x0 = _spectra(P, "P")
    lead = tuple(x0.shape[:-2])
    thr = None
    if threshold is not None:
        if isinstance(threshold, (bool, np.bool_)):
            raise ValueError("threshold: expected None, a number or one number per plane, got %r" % (threshold,))
        thr = threshold if torch.is_tensor(threshold) else torch.as_tensor(np.asarray(threshold))
        if thr.is_complex() or tuple(thr.shape) not in ((), lead):
            raise ValueError("threshold: expected None, a number or numbers shaped %s, got %s" % (lead, tuple(thr.shape)))
    if x0.is_complex():
        raise ValueError("P: expected real planes, got %s" % x0.dtype)
    x = _real32(x0)
    if thr is not None:
        thr = thr.to(device=x.device, dtype=torch.float32).expand(lead).contiguous()
    return _peak_mask(x, nb, thr, want)


def ft2d(S, neighborhood=(1, 25), threshold_scale=1.0, power=1.0, margin=1.0, mask=False, return_peaks=False):
    """2DFT separation of spectra [rows, T] or [N, rows, T] -> ``(background, foreground)`` shaped like S.

    ``F, mag = rfft2(|S|)``; ``thr = float32(threshold_scale * std(mag))`` (population std in fp64); ``M = peak_mask(mag,
    neighborhood, thr)`` (symmetric, because ``mag``'s bits are, so the masked inverse is real); ``B = irfft2(F M)``;
    ``rep = |B|``, ``res = ||S| - B|``; the masks are ``librosa.util.softmask`` of each against the other times its ``margin`` with
    exponent ``power`` (``glowk_hpss_mask``; the defaults give the ratio mask ``rep / (rep + res)``).  Complex S keeps its phase;
    ``mask=True`` returns the two masks; ``return_peaks`` adds ``M`` as a third result.  No host synchronisation."""
    nb = _check_neighborhood(neighborhood)
    scale = _check_scale(threshold_scale)
    power, (mb, mf) = _check_mask_params(power, margin)
    mask, return_peaks = _check_flag(mask, "mask"), _check_flag(return_peaks, "return_peaks")
    x, phase = _magnitude(_spectra(S))
    spec, mag = _rdft2(x, True)
    thr = (_plane_std(mag)[..., 1] * scale).to(torch.float32).contiguous()
    peaks = _peak_mask(mag, nb, thr)
    back = _irdft2(spec, peaks, x.shape[-1])
    rep, res = back.abs(), (x - back).abs()
    out_b, out_f = torch.empty_like(x), torch.empty_like(x)
    _lib.check(_lib.load().glowk_hpss_mask(_p(rep), _p(res), None if mask else _p(x), x.numel(), power, mb, mf, _p(out_b), _p(out_f),
                                           _s(x)))
    if not (mask or phase is None):
        out_b, out_f = out_b * phase, out_f * phase
    return (out_b, out_f, peaks) if return_peaks else (out_b, out_f)


_FT2D_AUDIO_DEFAULTS = dict(neighborhood=(1, 25), threshold_scale=1.0, cutoff_hz=100.0, power=1.0, margin=1.0, residual=False)


def _check_ft2d_audio_params(neighborhood, threshold_scale, cutoff_hz, power, margin, residual):
    """The arguments of ``ft2d_audio``, checked -> the number of STFT rows that go wholly to the background."""
    _check_neighborhood(neighborhood)
    _check_scale(threshold_scale)
    _check_mask_params(power, margin)
    _check_flag(residual, "residual")
    if isinstance(cutoff_hz, (bool, np.bool_)) or not isinstance(cutoff_hz, (int, float, np.integer, np.floating)) \
            or not (math.isfinite(cutoff_hz) and 0 <= cutoff_hz <= audio.SR / 2):
        raise ValueError("cutoff_hz: expected a frequency in [0, %g] (0: no cutoff), got %r" % (audio.SR / 2, cutoff_hz))
    n_fft = 2 * (audio.NBIN - 1)
    return 0 if cutoff_hz == 0 else min(audio.NBIN, math.floor(cutoff_hz * n_fft / audio.SR) + 1)


def ft2d_audio(y, neighborhood=(1, 25), threshold_scale=1.0, cutoff_hz=100.0, power=1.0, margin=1.0, residual=False):
    """2DFT separation for 16 kHz audio [n] or [C, n], n > 1024 -> ``(background, foreground)``, each shaped like y and aligned
    with it; with ``residual`` also ``y - background - foreground``.  The path of ``repet.repet_audio``: one STFT of the whole
    signal, ``ft2d`` on |X| per channel, the masked magnitudes with the mixture's phase through one ``audio.griffinlim(n_iter=0)``,
    trimmed to n samples.  The STFT rows r with ``r SR / n_fft <= cutoff_hz`` go wholly to the background (0: none do).  At most
    32 768 frames: about 17 minutes."""
    cut = _check_ft2d_audio_params(neighborhood, threshold_scale, cutoff_hz, power, margin, residual)
    t = audio._tensor(y, "y")
    x = audio._long_audio(t)
    if x.shape[0] > MAX_SIGNALS:
        raise ValueError("y: expected at most %d channels, got %d" % (MAX_SIGNALS, x.shape[0]))
    lead, n = tuple(t.shape[:-1]), x.shape[1]
    if 1 + -(-n // audio.HOP) > MAX_FRAMES:
        raise ValueError("y: expected at most %d frames (%d samples), got %d samples" % (MAX_FRAMES, (MAX_FRAMES - 2) * audio.HOP, n))
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [C, 1025, F]
    mag = X.abs()
    b, f = ft2d(mag, neighborhood, threshold_scale, power, margin)
    if cut:
        b[:, :cut], f[:, :cut] = mag[:, :cut], 0.0
    phase = torch.polar(torch.ones_like(X.real), X.angle())
    stems = audio.griffinlim(torch.cat([b, f]), n_iter=0, init=torch.cat([phase, phase]))[:, :n].reshape((2,) + lead + (n,))
    b, f = stems[0].contiguous(), stems[1].contiguous()
    return (b, f, x.reshape(lead + (n,)) - b - f) if residual else (b, f)


def separate_wav_ft2d(path, out_rate="input", mono=False, **kwargs):
    """``ft2d_audio`` for a PCM wav at any rate -> ``(stems, rate)``, the wrapper ``repet.separate_wav_repet_periodic`` is around
    ``repet_audio``: stems [2, n'] (background, foreground; [3, n'] with ``residual=True``) of a one-channel file or with ``mono``,
    else [2 or 3, C, n'], at ``out_rate``: 'input' (the file's rate and exactly its sample count), an integer rate, or None (16 kHz).
    ``kwargs`` are ``ft2d_audio``'s keyword arguments; any other is refused before the file is opened."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    _check_flag(mono, "mono")
    unknown = set(kwargs) - set(_FT2D_AUDIO_DEFAULTS)
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected ft2d_audio's" % sorted(unknown))
    _check_ft2d_audio_params(**dict(_FT2D_AUDIO_DEFAULTS, **kwargs))
    y, native = audio.load_audio(path, sr=None, mono=False)
    n_file = y.shape[1]
    y = y.mean(0) if mono or y.shape[0] == 1 else y
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    stems = audio.resample(torch.stack(ft2d_audio(y, **kwargs)), audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate
