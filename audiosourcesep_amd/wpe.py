"""WPE (weighted prediction error) dereverberation (Nakatani et al. 2010; Yoshioka & Nakatani 2012; the ``nara_wpe`` package): the late
reverberation of every frequency row is predicted from the row's own delayed past by a multichannel linear filter and subtracted.  Blind;
it keeps the channel count and the phase, so its output is a drop-in ``X`` for ``iva.auxiva``, ``duet.duet``, ``projet.projet`` and
``audio.separate_stereo``: the front end for material recorded in a room, where the instantaneous-mixture model of those separators
breaks first.  Not in the reference.

Per row, with taps K, delay and D = M K, the stacked past is ``x~[k M + m](t) = x_m(t - delay - k)`` (zero before the signal).  One
iteration (kernels in ``csrc/glowk_wpe.h``, formulas and error bounds in include/glowk.h, design in DESIGN 30):

* ``power_inverse``: ``w(t) = 1 / max(p(t), eps max_t p)`` with ``p`` the channel-mean power of the current estimate, optionally
  averaged over ``psd_context`` frames on each side;
* ``correlations``: ``R = sum_t w x~ x~^H`` and ``P = sum_t w x~ x^H`` on the fp64 matrix cores;
* ``solve``: ``R += loading (tr R / D) I``, ``R = L L^H``, ``G = R^-1 P``, and a status word per row;
* ``filter``: ``y = x - G^H x~``, rounded once to complex64;
* ``wpe``: the loop, one C call (``glowk_wpe_fit``, four launches per iteration), bit for bit the staged calls iterated by hand;
* ``wpe_audio`` / ``dereverb_wav``: the audio and wav paths, the latter optionally straight into ``iva.auxiva`` / ``iva.ilrma``.

X is ``[M, R, T]`` or ``[N, M, R, T]`` complex, ``1 <= M <= 4``, ``1 <= K <= 32``, ``M K <= 64``, ``1 <= delay <= 16``,
``1 <= T <= 32768``, ``R <= 4096``.  A row whose power is zero or not finite is passed through (``y = x``, ``G = 0``) with status 1,
as is a row whose Cholesky factor meets a pivot that is not finite or not positive.  Everything after the load of X is fp64 in a
fixed order: results are bitwise reproducible and a batch gives what its signals give alone.

Conventions as in ``iva.py``: numpy or torch in, tensors on the GPU the input lives on out, ValueError for bad arguments before the
library is loaded, no host synchronisation.
"""
import math
import os

import numpy as np
import torch

from . import _lib, audio
from .audio import _p, _s
from .repet import MAX_ELEMENTS, MAX_FRAMES, MAX_ROWS, MAX_SIGNALS, _check_flag, _check_range_int

MIN_CHANNELS, MAX_CHANNELS, MAX_TAPS, MAX_STACKED, MAX_DELAY, MAX_CONTEXT, MAX_ITER = 1, 4, 32, 64, 16, 8, 1000
STATUS_OK, STATUS_PIVOT = 0, 1
SEPARATORS = ("auxiva", "ilrma")


def _check_mix(X, what="X"):
    """[M, R, T] or [N, M, R, T] complex within the kernels' ranges, as a tensor where it is."""
    x = X if torch.is_tensor(X) else torch.as_tensor(np.asarray(X))
    if x.dim() not in (3, 4) or not MIN_CHANNELS <= x.shape[-3] <= MAX_CHANNELS or not 1 <= x.shape[-2] <= MAX_ROWS \
            or not 1 <= x.shape[-1] <= MAX_FRAMES or (x.dim() == 4 and x.shape[0] > MAX_SIGNALS) or x.numel() > MAX_ELEMENTS:
        raise ValueError("%s: expected [M, rows, T] or [N, M, rows, T] with N <= %d, 1 <= M <= 4, 1 <= rows <= %d, 1 <= T <= %d and at most "
                         "2^31 - 1 elements, got %s" % (what, MAX_SIGNALS, MAX_ROWS, MAX_FRAMES, tuple(x.shape)))
    if not x.is_complex():
        raise ValueError("%s: expected the complex STFT of M channels, got %s" % (what, x.dtype))
    return x


def _dims(x):
    """x [.., M, R, T] -> (lead, nsig, M, R, T)."""
    M, R, T = x.shape[-3:]
    return tuple(x.shape[:-3]), (x.shape[0] if x.dim() == 4 else 1), M, R, T


def _check_model(M, taps, delay):
    K = _check_range_int(taps, "taps", 1, MAX_TAPS)
    if M * K > MAX_STACKED:
        raise ValueError("taps: expected M * taps <= %d, got M = %d, taps = %d" % (MAX_STACKED, M, K))
    return K, _check_range_int(delay, "delay", 1, MAX_DELAY)


def _check_unit(v, what, open_zero):
    """A float in (0, 1] (open_zero) or [0, 1]."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) \
            or not (0.0 < v if open_zero else 0.0 <= v) or v > 1.0:
        raise ValueError("%s: expected a number in %s0, 1], got %r" % (what, "(" if open_zero else "[", v))
    return float(v)


def _real_like(t, shape, what):
    r = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
    if r.is_complex() or tuple(r.shape) != shape:
        raise ValueError("%s: expected real %s, got %s %s" % (what, shape, r.dtype, tuple(r.shape)))
    return r


def _complex_like(t, shape, what):
    r = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
    if not r.is_complex() or tuple(r.shape) != shape:
        raise ValueError("%s: expected complex %s, got %s %s" % (what, shape, r.dtype, tuple(r.shape)))
    return r


def _work(nbytes, dev):
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)


def power_inverse(Y, psd_context=0, eps=1e-10, return_max=False):
    """The weights ``w`` [.., R, T] float64 of the estimate Y: ``q(t) = (sum_m |y_m(t)|^2) / M``; ``p(t) = q(t)``, or with
    ``psd_context = c > 0`` the mean of q over the frames of ``[t - c, t + c]`` that exist; ``w(t) = 1 / max(p(t), eps max_t p)``.  A row
    whose maximum is zero or not finite gets ``w = 0``: the later stages pass it through and flag it.  ``return_max`` adds the row maxima
    [.., R].  ``glowk_wpe_power``: one launch, the maximum in it."""
    c = _check_range_int(psd_context, "psd_context", 0, MAX_CONTEXT)
    eps = _check_unit(eps, "eps", True)
    want = _check_flag(return_max, "return_max")
    y = _check_mix(Y, "Y")
    lead, nsig, M, R, T = _dims(y)
    y = y.to(device=audio._device(y), dtype=torch.complex64).contiguous()
    w = torch.empty(lead + (R, T), dtype=torch.float64, device=y.device)
    mx = torch.empty(lead + (R,), dtype=torch.float64, device=y.device) if want else None
    if nsig:
        _lib.check(_lib.load().glowk_wpe_power(_p(y), nsig, M, R, T, c, eps, _p(w), _p(mx), _s(y)))
    return (w, mx) if want else w


def correlations(X, inv_power, taps, delay):
    """``(Rm, P)``: ``Rm = sum_t w(t) x~ x~^H`` complex128 [.., R, D, D] (Hermitian bit for bit, both triangles stored, a real diagonal)
    and ``P = sum_t w(t) x~ x^H`` [.., R, D, M], with ``inv_power`` the weights w [.., R, T].  ``glowk_wpe_correlations``: one launch on
    the fp64 matrix cores, frames in ascending order."""
    x = _check_mix(X)
    lead, nsig, M, R, T = _dims(x)
    K, delay = _check_model(M, taps, delay)
    w = _real_like(inv_power, lead + (R, T), "inv_power")
    dev = audio._device(x, w)
    x = x.to(device=dev, dtype=torch.complex64).contiguous()
    w = w.to(device=dev, dtype=torch.float64).contiguous()
    D = M * K
    Rm = torch.empty(lead + (R, D, D), dtype=torch.complex128, device=dev)
    P = torch.empty(lead + (R, D, M), dtype=torch.complex128, device=dev)
    if nsig:
        _lib.check(_lib.load().glowk_wpe_correlations(_p(x), _p(w), nsig, M, R, T, K, delay, _p(Rm), _p(P), _s(x)))
    return Rm, P


def solve(Rm, P, loading=1e-10):
    """``(G, status)``: per row ``Rm += loading (tr Rm / D) I``, ``Rm = L L^H`` and ``G = Rm^-1 P`` complex128 [.., R, D, M] by the two
    triangular solves; status [.., R] int32 is 0, or 1 where a pivot was not finite or not > 0, and then ``G = 0``.  Only the lower
    triangle of Rm is read.  ``glowk_wpe_solve``: one launch, one wave per row."""
    loading = _check_unit(loading, "loading", False)
    r = Rm if torch.is_tensor(Rm) else torch.as_tensor(np.asarray(Rm))
    if not r.is_complex() or r.dim() not in (3, 4) or r.shape[-1] != r.shape[-2] or not 1 <= r.shape[-1] <= MAX_STACKED \
            or not 1 <= r.shape[-3] <= MAX_ROWS or (r.dim() == 4 and r.shape[0] > MAX_SIGNALS):
        raise ValueError("Rm: expected complex [rows, D, D] or [N, rows, D, D] with 1 <= D <= 64, got %s %s" % (r.dtype, tuple(r.shape)))
    D = r.shape[-1]
    p = P if torch.is_tensor(P) else torch.as_tensor(np.asarray(P))
    if not p.is_complex() or p.dim() != r.dim() or tuple(p.shape[:-1]) != tuple(r.shape[:-1]) or not MIN_CHANNELS <= p.shape[-1] <= MAX_CHANNELS:
        raise ValueError("P: expected complex %s + (M,) with 1 <= M <= 4, got %s %s" % (tuple(r.shape[:-1]), p.dtype, tuple(p.shape)))
    dev = audio._device(r, p)
    r = r.to(device=dev, dtype=torch.complex128).contiguous()
    p = p.to(device=dev, dtype=torch.complex128).contiguous()
    G = torch.empty_like(p)
    status = torch.empty(tuple(r.shape[:-2]), dtype=torch.int32, device=dev)
    nsig = r.shape[0] if r.dim() == 4 else 1
    if nsig:
        _lib.check(_lib.load().glowk_wpe_solve(_p(r), _p(p), nsig, r.shape[-3], D, p.shape[-1], loading, _p(G), _p(status), _s(r)))
    return G, status


def filter(X, G, taps, delay):
    """``y(t) = x(t) - G^H x~(t)`` in fp64, each component rounded once -> complex64 like X.  G is [.., R, D, M]; a row whose G is all
    zeros is copied.  ``glowk_wpe_filter``: one pass over X."""
    x = _check_mix(X)
    lead, nsig, M, R, T = _dims(x)
    K, delay = _check_model(M, taps, delay)
    g = _complex_like(G, lead + (R, M * K, M), "G")
    dev = audio._device(x, g)
    x = x.to(device=dev, dtype=torch.complex64).contiguous()
    g = g.to(device=dev, dtype=torch.complex128).contiguous()
    y = torch.empty_like(x)
    if nsig:
        _lib.check(_lib.load().glowk_wpe_filter(_p(x), _p(g), nsig, M, R, T, K, delay, _p(y), _s(x)))
    return y


def _check_wpe_args(M, taps, delay, iterations, psd_context, eps, loading):
    K, delay = _check_model(M, taps, delay)
    return (K, delay, _check_range_int(iterations, "iterations", 0, MAX_ITER), _check_range_int(psd_context, "psd_context", 0, MAX_CONTEXT),
            _check_unit(eps, "eps", True), _check_unit(loading, "loading", False))


def wpe(X, taps=10, delay=3, iterations=3, psd_context=0, eps=1e-10, loading=1e-10, return_filters=False, return_status=False):
    """WPE on X [M, R, T] or [N, M, R, T] -> the dereverberated STFT, complex64 like X.  ``iterations`` times: ``power_inverse`` of the
    current estimate (X at first, then the complex64 estimate of the iteration before), ``correlations``, ``solve``, ``filter`` -- four
    launches each, all in one C call (``glowk_wpe_fit``), bit for bit the staged calls iterated by hand.  Zero iterations return X.
    ``return_filters`` adds the last iteration's G [.., R, D, M] complex128 (zeros for zero iterations), ``return_status`` its status
    words [.., R] int32."""
    want_g = _check_flag(return_filters, "return_filters")
    want_s = _check_flag(return_status, "return_status")
    x = _check_mix(X)
    lead, nsig, M, R, T = _dims(x)
    K, delay, iterations, c, eps, loading = _check_wpe_args(M, taps, delay, iterations, psd_context, eps, loading)
    x = x.to(device=audio._device(x), dtype=torch.complex64).contiguous()
    D = M * K
    if nsig and iterations:
        y = torch.empty_like(x)
        G = torch.empty(lead + (R, D, M), dtype=torch.complex128, device=x.device)
        status = torch.empty(lead + (R,), dtype=torch.int32, device=x.device)
        lib = _lib.load()
        nbytes = lib.glowk_wpe_workspace_bytes(nsig, M, K, R, T)
        work = _work(nbytes, x.device)
        _lib.check(lib.glowk_wpe_fit(_p(x), nsig, M, R, T, K, delay, iterations, c, eps, loading, _p(y), _p(G), _p(status), _p(work), nbytes, _s(x)))
    else:
        y = x
        G = torch.zeros(lead + (R, D, M), dtype=torch.complex128, device=x.device) if want_g else None
        status = torch.zeros(lead + (R,), dtype=torch.int32, device=x.device) if want_s else None
    out = (y,) + ((G,) if want_g else ()) + ((status,) if want_s else ())
    return out if len(out) > 1 else y


_WPE_DEFAULTS = dict(taps=10, delay=3, iterations=3, psd_context=0, eps=1e-10, loading=1e-10)


def _check_wpe_kwargs(M, kwargs, what):
    unknown = set(kwargs) - set(_WPE_DEFAULTS)
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected %s" % (sorted(unknown), what))
    args = dict(_WPE_DEFAULTS, **kwargs)
    _check_wpe_args(M, **args)
    return args


def _stft(t):
    """[M, n] float32 on its GPU -> the complex STFT [M, 1025, F] of the whole signal."""
    return audio.mel_frames(t, return_stft=True)[1]


def _audio_in(y):
    t = audio._tensor(y, "y")
    if t.dim() not in (1, 2) or (t.dim() == 2 and not MIN_CHANNELS <= t.shape[0] <= MAX_CHANNELS):
        raise ValueError("y: expected [n] or one to four channels [M, n], got %s" % (tuple(t.shape),))
    x = audio._long_audio(t)
    if 1 + -(-x.shape[1] // audio.HOP) > MAX_FRAMES:
        raise ValueError("y: expected at most %d frames (%d samples), got %d samples" % (MAX_FRAMES, (MAX_FRAMES - 2) * audio.HOP, x.shape[1]))
    return t.dim() == 1, x


def wpe_audio(y, **wpe_args):
    """Dereverberation of 16 kHz audio [M, n] or [n], 1 <= M <= 4, n > 1024 -> audio of the same shape and length.  One STFT of the
    whole signal (``audio.mel_frames(return_stft=True)``), ``wpe`` on it with ``wpe_args`` (taps, delay, iterations, psd_context, eps,
    loading), one ``audio.istft``, trimmed to n samples.  The STFT is the package's one pair: 16 kHz, a 2048-sample window every 512
    samples, so a frame is 32 ms and the defaults (delay 3, taps 10) leave 96 ms untouched and predict from the 320 ms before that --
    not the 512 / 128 geometry customary for WPE, which the package has no transform for; there are no ``sr``, ``n_fft`` or
    ``hop_length`` arguments because they could take one value only.  At most 32 768 frames."""
    mono, x = _audio_in(y)
    M, n = x.shape
    args = _check_wpe_kwargs(M, wpe_args, "wpe's taps, delay, iterations, psd_context, eps and loading")
    x = x.to(device=audio._device(x), dtype=torch.float32)
    out = audio.istft(wpe(_stft(x), **args))[..., :n].contiguous()
    return out[0] if mono else out


def dereverb_wav(path_or_array, out=None, sr=None, separate=None, n_iter=None, **wpe_args):
    """``wpe_audio`` for a PCM wav at any rate (or an array of samples at rate ``sr``, 16 kHz by default) -> ``(audio, rate)`` at the
    input's rate and exactly its length, [M, n] or [n] as the input; ``out`` names a wav file to write it to.  With
    ``separate = 'auxiva'`` or ``'ilrma'`` (two to four channels) the dereverberated STFT goes straight into ``iva.auxiva`` /
    ``iva.ilrma`` (``n_iter`` iterations, their defaults when None) and the result is the stems [M, M, n] that
    ``iva.separate_wav_iva`` returns; ``out`` is then refused.  ``wpe_args`` as in ``wpe_audio``; bad arguments are refused before the
    file is opened."""
    from . import iva
    if separate is not None and (not isinstance(separate, str) or separate not in SEPARATORS):
        raise ValueError("separate: expected None, 'auxiva' or 'ilrma', got %r" % (separate,))
    if n_iter is not None:
        _check_range_int(n_iter, "n_iter", 0, iva.MAX_ITER)
    if separate is not None and out is not None:
        raise ValueError("out: stems are returned, not written; expected None with separate, got %r" % (out,))
    if out is not None and not isinstance(out, (str, os.PathLike)):
        raise ValueError("out: expected None or a path, got %r" % (out,))
    _check_wpe_kwargs(1, wpe_args, "wpe_audio's")
    if isinstance(path_or_array, (str, os.PathLike)):
        if sr is not None:
            raise ValueError("sr: a file carries its own rate; expected None, got %r" % (sr,))
        y, native = audio.load_audio(path_or_array, sr=None, mono=False)
    else:
        native = audio.SR if sr is None else audio._check_rate(sr, "sr")
        y = audio._tensor(path_or_array, "y")
    if y.dim() not in (1, 2) or (y.dim() == 2 and not MIN_CHANNELS <= y.shape[0] <= MAX_CHANNELS):
        raise ValueError("expected one to four channels, got %s" % (tuple(y.shape),))
    M = 1 if y.dim() == 1 else y.shape[0]
    args = _check_wpe_kwargs(M, wpe_args, "wpe_audio's")
    if separate is not None and M < iva.MIN_CHANNELS:
        raise ValueError("separate: needs two to four channels, got %d" % M)
    n_file = y.shape[-1]
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "sampling rate"), audio.SR)
    if separate is None:
        res = wpe_audio(y, **args)
    else:
        _, x = _audio_in(y)
        n = x.shape[1]
        x = x.to(device=audio._device(x), dtype=torch.float32)
        Y = wpe(_stft(x), **args)
        img = iva.auxiva(Y, 20 if n_iter is None else n_iter) if separate == "auxiva" else iva.ilrma(Y, n_iter=50 if n_iter is None else n_iter)
        res = audio.istft(img)[..., :n].contiguous()
    res = audio.resample(res, audio.SR, native)[..., :n_file].contiguous()
    if out is not None:
        audio.save_audio(out, res, native)
    return res, native
