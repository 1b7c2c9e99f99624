"""DUET (Yilmaz & Rickard 2004; Rickard, "The DUET blind source separation algorithm", 2007; ``Duet`` in nussl): blind separation of
a stereo mixture from where its sources sit between the two channels.  Every time-frequency cell gets a symmetric attenuation
``alpha = a - 1/a`` and a delay ``delta`` between the channels; a weighted 2-D histogram of the two has one peak per source; every
cell goes to the nearest peak.  Any number of sources from two channels, no priors, no training.  Not in the reference.

Kernels in ``csrc/glowk_duet.h`` (formulas in include/glowk.h, design in DESIGN 21):

* ``features``: alpha, delta and the weight ``(|X1| |X2|)^p omega^q`` per cell, fp64 (a diagnostic; the production path never stores them);
* ``histogram``: the weighted histogram as exact integers -- a counted weight becomes ``rint(w 2^(s - e))`` with ``wmax < 2^e`` and the
  cell is the int64 sum, so the plane is the same bits every run and in every batch; returned with ``(e, s)``;
* ``find_peaks``: binomial smoothing in int64 and the greedy picks with an exclusion box, exact;
* ``assign``: every cell to the peak with the smallest ``|a e^{-i delta omega} X1 - X2|^2 / (1 + a^2)``; masks and masked spectra;
* ``duet`` / ``duet_audio`` / ``separate_wav_duet``: the spectra, audio and wav paths.

Delays beyond ``pi / omega`` wrap: a phase difference is known modulo 2 pi, so row r resolves ``|delta| < n_fft / (2 r)`` samples
and the top rows only ``|delta| < 1``.  At 16 kHz with the front end's 2048-point STFT (hop 512) that means only delays below one
sample -- microphones a few centimetres apart -- are unambiguous over the whole band; amplitude-panned studio stereo sits at
``delta = 0`` and separates along the attenuation axis alone.

Conventions as in ``ft2d.py``: numpy or torch in, tensors on the GPU the input lives on out, ValueError for bad arguments before the
library is loaded, no host synchronisation.
"""
import math

import numpy as np
import torch

from . import _lib, audio
from .audio import _p, _s
from .repet import MAX_FRAMES, MAX_ROWS, MAX_SIGNALS, _check_flag, _check_range_int

MAX_BINS, MAX_SOURCES, MAX_SMOOTH = 16384, 16, 3
MAX_ELEMENTS = (1 << 31) - 1


def _number(v, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError("%s: expected a finite number, got %r" % (what, v))
    return float(v)


def _check_axis(axis, what):
    """(lo, hi, n): a finite range lo < hi cut into n >= 1 bins."""
    if not isinstance(axis, (tuple, list)) or len(axis) != 3:
        raise ValueError("%s: expected (lo, hi, bins), got %r" % (what, axis))
    lo, hi = _number(axis[0], what), _number(axis[1], what)
    n = _check_range_int(axis[2], what + " bins", 1, MAX_BINS)
    if not (lo < hi and math.isfinite(hi - lo)):
        raise ValueError("%s: expected lo < hi, got %r" % (what, tuple(axis)))
    return lo, hi, n


def _check_grid(attenuation, delay):
    a, d = _check_axis(attenuation, "attenuation"), _check_axis(delay, "delay")
    if a[2] * d[2] > MAX_BINS:
        raise ValueError("attenuation, delay: expected at most %d bins in all, got %d x %d" % (MAX_BINS, a[2], d[2]))
    return a + d


def _check_min_distance(min_distance):
    if not isinstance(min_distance, (tuple, list)) or len(min_distance) != 2:
        raise ValueError("min_distance: expected a pair of integers >= 0, got %r" % (min_distance,))
    return tuple(_check_range_int(v, "min_distance", 0, MAX_BINS) for v in min_distance)


def _check_model(num_sources, attenuation, delay, p, q, smooth, min_distance):
    S = _check_range_int(num_sources, "num_sources", 1, MAX_SOURCES)
    grid = _check_grid(attenuation, delay)
    return S, grid, _number(p, "p"), _number(q, "q"), _check_range_int(smooth, "smooth", 0, MAX_SMOOTH), _check_min_distance(min_distance)


def _check_stereo(X, what="X"):
    """[2, R, T] or [N, 2, R, T] complex within the kernels' ranges, as a tensor where it is."""
    x = X if torch.is_tensor(X) else torch.as_tensor(np.asarray(X))
    if x.dim() not in (3, 4) or x.shape[-3] != 2 or not 1 <= x.shape[-2] <= MAX_ROWS or not 1 <= x.shape[-1] <= MAX_FRAMES \
            or (x.dim() == 4 and x.shape[0] > MAX_SIGNALS) or x.numel() > MAX_ELEMENTS:
        raise ValueError("%s: expected [2, rows, T] or [N, 2, rows, T] with N <= %d, 1 <= rows <= %d, 1 <= T <= %d and at most 2^31 - 1 "
                         "elements, got %s" % (what, MAX_SIGNALS, MAX_ROWS, MAX_FRAMES, tuple(x.shape)))
    if not x.is_complex():
        raise ValueError("%s: expected the complex STFT of two channels, got %s" % (what, x.dtype))
    return x


def _stereo(X, what="X"):
    """... as complex64 contiguous on its GPU."""
    x = _check_stereo(X, what)
    return x.to(device=audio._device(x), dtype=torch.complex64).contiguous()


def _dims(x):
    """x [.., 2, R, T] -> (lead, nsig, R, T)."""
    R, T = x.shape[-2], x.shape[-1]
    return tuple(x.shape[:-3]), x.numel() // (2 * R * T), R, T


def _work(nbytes, dev):
    return torch.empty(max(nbytes // 8, 2), dtype=torch.float64, device=dev)


def _histogram(x, grid, p, q, smooth):
    lib = _lib.load()
    lead, nsig, R, T = _dims(x)
    hist = torch.empty(lead + (grid[2], grid[5]), dtype=torch.int64, device=x.device)
    es = torch.empty(lead + (2,), dtype=torch.int32, device=x.device)
    nbytes = lib.glowk_duet_hist_workspace_bytes(nsig, R * T, grid[2], grid[5])
    work = _work(nbytes, x.device)
    _lib.check(lib.glowk_duet_histogram_stft(_p(x), nsig, R, T, p, q, grid[0], grid[1], grid[2], grid[3], grid[4], grid[5], smooth, _p(hist), _p(es),
                                             _p(work), nbytes, _s(x)))
    return hist, es


def _peaks(hist, S, smooth, dist, want_smoothed):
    lib = _lib.load()
    n_a, n_d = hist.shape[-2], hist.shape[-1]
    lead = tuple(hist.shape[:-2])
    nsig = hist.numel() // (n_a * n_d)
    peaks = torch.empty(lead + (S, 2), dtype=torch.int32, device=hist.device)
    found = torch.empty(lead, dtype=torch.int32, device=hist.device)
    sm = torch.empty_like(hist) if want_smoothed else None
    nbytes = lib.glowk_duet_peaks_workspace_bytes(nsig, n_a, n_d)
    work = _work(nbytes, hist.device)
    _lib.check(lib.glowk_duet_peaks(_p(hist), nsig, n_a, n_d, smooth, S, dist[0], dist[1], _p(sm), _p(peaks), _p(found), _p(work), nbytes, _s(hist)))
    return peaks, found, sm


def _assign(x, peaks, found, grid):
    lib = _lib.load()
    lead, nsig, R, T = _dims(x)
    S = peaks.shape[-2]
    masks = torch.empty(lead + (S, R, T), dtype=torch.float32, device=x.device)
    spec = torch.empty(lead + (S, 2, R, T), dtype=torch.complex64, device=x.device)
    nbytes = lib.glowk_duet_assign_workspace_bytes(nsig, R, S)
    work = _work(nbytes, x.device)
    _lib.check(lib.glowk_duet_assign(_p(x), nsig, R, T, _p(peaks), _p(found), S, grid[0], grid[1], grid[2], grid[3], grid[4], grid[5], _p(masks), _p(spec),
                                     _p(work), nbytes, _s(x)))
    return masks, spec


def features(X, p=1.0, q=0.0):
    """The DUET features of a stereo STFT [2, R, T] or [N, 2, R, T] -> ``(alpha, delta, w)``, float64 [.., R, T].

    With ``m1 = |X1|``, ``m2 = |X2|``, ``omega_r = 2 pi r / (2 (R - 1))``: ``alpha = (m2^2 - m1^2) / (m1 m2)``, ``delta = -arg(X2 conj X1)
    / omega_r`` in samples, ``w = (m1 m2)^p omega_r^q``; all three are 0 in row 0 and where a channel is exactly 0.  fp64 after the load.
    ``glowk_duet_features``; ``histogram`` computes the same numbers in registers and never stores them."""
    p, q = _number(p, "p"), _number(q, "q")
    x = _stereo(X)
    lead, nsig, R, T = _dims(x)
    out = [torch.empty(lead + (R, T), dtype=torch.float64, device=x.device) for _ in range(3)]
    _lib.check(_lib.load().glowk_duet_features(_p(x), nsig, R, T, p, q, _p(out[0]), _p(out[1]), _p(out[2]), _s(x)))
    return tuple(out)


def histogram(X=None, attenuation=(-3, 3, 50), delay=(-3, 3, 50), p=1.0, q=0.0, smooth=1, features=None):
    """The weighted attenuation-delay histogram -> ``(hist, es)``: int64 [.., n_a, n_d] and int32 [.., 2] holding ``(e, s)``;
    ``hist 2^(e - s)`` is the histogram in the weights' units.

    A cell counts when its weight is finite and positive and ``i = floor((alpha - lo) n / (hi - lo))`` lies in [0, n) on both axes
    (half-open; fp64).  ``wmax < 2^e`` is the signal's largest counted weight, ``s = min(40, 62 - ceil_log2(max(cells, 2)) - 4 smooth)``,
    and a bin is the integer sum of ``rint(w 2^(s - e))``: exact, so bitwise reproducible and independent of the batch.  ``smooth`` is
    the number of passes ``find_peaks`` will make (it only sets the headroom in s).  A silent signal gives an all-zero plane, e = 0.

    From ``X`` [2, R, T] or [N, 2, R, T] in two passes over X (``glowk_duet_histogram_stft``), or with ``features = (alpha, delta, w)``
    (real, shaped [R, T] or [N, R, T] alike) from stored features (``glowk_duet_histogram``): the same bits."""
    grid = _check_grid(attenuation, delay)
    p, q = _number(p, "p"), _number(q, "q")
    smooth = _check_range_int(smooth, "smooth", 0, MAX_SMOOTH)
    if (X is None) == (features is None):
        raise ValueError("histogram: expected either X or features")
    if features is None:
        return _histogram(_stereo(X), grid, p, q, smooth)
    if not isinstance(features, (tuple, list)) or len(features) != 3:
        raise ValueError("features: expected (alpha, delta, w), got %r" % (type(features),))
    f = [t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t)) for t in features]
    if any(t.is_complex() for t in f) or len({tuple(t.shape) for t in f}) != 1 or f[0].dim() not in (2, 3) or f[0].shape[-1] < 1 or f[0].shape[-2] < 1:
        raise ValueError("features: expected three real tensors of one shape [R, T] or [N, R, T], got %s" % [tuple(t.shape) for t in f])
    lead = tuple(f[0].shape[:-2])
    nsig, cells = (f[0].shape[0] if lead else 1), f[0].shape[-2] * f[0].shape[-1]
    if nsig > MAX_SIGNALS or cells > MAX_ROWS * MAX_FRAMES or nsig * cells > MAX_ELEMENTS:
        raise ValueError("features: expected at most %d signals of at most 2^27 cells and 2^31 - 1 cells in all, got %s" % (MAX_SIGNALS, tuple(f[0].shape)))
    dev = audio._device(*f)
    f = [t.to(device=dev, dtype=torch.float64).contiguous() for t in f]
    lib = _lib.load()
    hist = torch.empty(lead + (grid[2], grid[5]), dtype=torch.int64, device=dev)
    es = torch.empty(lead + (2,), dtype=torch.int32, device=dev)
    nbytes = lib.glowk_duet_hist_workspace_bytes(nsig, cells, grid[2], grid[5])
    work = _work(nbytes, dev)
    _lib.check(lib.glowk_duet_histogram(_p(f[0]), _p(f[1]), _p(f[2]), nsig, cells, grid[0], grid[1], grid[2], grid[3], grid[4], grid[5], smooth, _p(hist),
                                        _p(es), _p(work), nbytes, _s(f[0])))
    return hist, es


def find_peaks(hist, num_sources, smooth=1, min_distance=(5, 5), return_smoothed=False):
    """The peaks of non-negative integer planes [n_a, n_d] or [N, n_a, n_d] -> ``(peaks, n_found)``: int32 [.., num_sources, 2] of
    (attenuation bin, delay bin), -1 where none was found, and int32 [..].

    ``smooth`` passes (0..3) of the binomial kernel ``[1 2 1] x [1 2 1]`` in int64, zero beyond the edges, no division (not nussl's
    box kernel, which turns an isolated cell into a 3 x 3 plateau of exact ties).  Then ``num_sources`` times: the largest value among
    the cells not yet excluded, ties to the lowest row-major index; stop at 0; exclude every cell within ``min_distance`` of the pick
    on both axes.  Exact.  ``return_smoothed`` adds the smoothed plane.  ``glowk_duet_peaks``: one launch."""
    S = _check_range_int(num_sources, "num_sources", 1, MAX_SOURCES)
    smooth = _check_range_int(smooth, "smooth", 0, MAX_SMOOTH)
    dist = _check_min_distance(min_distance)
    want = _check_flag(return_smoothed, "return_smoothed")
    h = hist if torch.is_tensor(hist) else torch.as_tensor(np.asarray(hist))
    if h.dim() not in (2, 3) or h.is_complex() or h.is_floating_point() or h.shape[-2] < 1 or h.shape[-1] < 1 \
            or h.shape[-2] * h.shape[-1] > MAX_BINS or (h.dim() == 3 and h.shape[0] > MAX_SIGNALS):
        raise ValueError("hist: expected integer planes [n_a, n_d] or [N, n_a, n_d] of at most %d bins, got %s %s" % (MAX_BINS, h.dtype, tuple(h.shape)))
    h = h.to(device=audio._device(h), dtype=torch.int64).contiguous()
    peaks, found, sm = _peaks(h, S, smooth, dist, want)
    return (peaks, found, sm) if want else (peaks, found)


def assign(X, peaks, n_found, attenuation=(-3, 3, 50), delay=(-3, 3, 50)):
    """Every cell of X [2, R, T] or [N, 2, R, T] to its nearest peak -> ``(masks, spectra)``: float32 [.., S, R, T] and complex64
    [.., S, 2, R, T] for ``peaks`` int [.., S, 2] and ``n_found`` int [..].

    Source j sits at the centres ``alpha_j, delta_j`` of its peak's bins, ``a_j = (alpha_j + sqrt(alpha_j^2 + 4)) / 2``; a cell goes to
    the lowest j < n_found that attains the smallest ``|a_j e^{-i delta_j omega_r} X1 - X2|^2 / (1 + a_j^2)`` (fp64; every row,
    row 0 included).  The masks are a partition where n_found >= 1 and all 0 where it is 0; the spectra are X where the mask is 1."""
    grid = _check_grid(attenuation, delay)
    x = _check_stereo(X)
    lead = tuple(x.shape[:-3])
    pk = peaks if torch.is_tensor(peaks) else torch.as_tensor(np.asarray(peaks))
    nf = n_found if torch.is_tensor(n_found) else torch.as_tensor(np.asarray(n_found))
    if pk.is_complex() or pk.is_floating_point() or pk.dim() != len(lead) + 2 or tuple(pk.shape[:-2]) != lead or pk.shape[-1] != 2 \
            or not 1 <= pk.shape[-2] <= MAX_SOURCES:
        raise ValueError("peaks: expected integers shaped %s + (S, 2) with 1 <= S <= %d, got %s %s" % (lead, MAX_SOURCES, pk.dtype, tuple(pk.shape)))
    if nf.is_complex() or nf.is_floating_point() or tuple(nf.shape) != lead:
        raise ValueError("n_found: expected integers shaped %s, got %s %s" % (lead, nf.dtype, tuple(nf.shape)))
    dev = audio._device(x, pk, nf)
    x = x.to(device=dev, dtype=torch.complex64).contiguous()
    return _assign(x, pk.to(device=dev, dtype=torch.int32).contiguous(), nf.to(device=dev, dtype=torch.int32).contiguous(), grid)


def duet(X, num_sources, attenuation=(-3, 3, 50), delay=(-3, 3, 50), p=1.0, q=0.0, smooth=1, min_distance=(5, 5), mask=False,
         return_model=False):
    """DUET on a stereo STFT [2, R, T] or [N, 2, R, T] -> the stems, complex64 [.., S, 2, R, T] (float32 masks [.., S, R, T] with
    ``mask=True``); a source that was not found is all zero.  ``histogram`` (two passes over X), ``find_peaks``, ``assign`` (one pass):
    five launches and a memset, no host synchronisation.  ``return_model`` adds a dict with ``hist``, ``es``, ``peaks`` and ``n_found``."""
    S, grid, p, q, smooth, dist = _check_model(num_sources, attenuation, delay, p, q, smooth, min_distance)
    mask, return_model = _check_flag(mask, "mask"), _check_flag(return_model, "return_model")
    x = _stereo(X)
    hist, es = _histogram(x, grid, p, q, smooth)
    peaks, found, _ = _peaks(hist, S, smooth, dist, False)
    masks, spec = _assign(x, peaks, found, grid)
    out = masks if mask else spec
    return (out, dict(hist=hist, es=es, peaks=peaks, n_found=found)) if return_model else out


_DUET_AUDIO_DEFAULTS = dict(attenuation=(-3, 3, 50), delay=(-3, 3, 50), p=1.0, q=0.0, smooth=1, min_distance=(5, 5), residual=False)


def _check_duet_audio_params(num_sources, attenuation, delay, p, q, smooth, min_distance, residual):
    _check_model(num_sources, attenuation, delay, p, q, smooth, min_distance)
    _check_flag(residual, "residual")


def duet_audio(y, num_sources, attenuation=(-3, 3, 50), delay=(-3, 3, 50), p=1.0, q=0.0, smooth=1, min_distance=(5, 5), residual=False):
    """DUET for two channels of 16 kHz audio [2, n], n > 1024 -> stems [S, 2, n] aligned with y; with ``residual`` also
    ``y - stems.sum(0)``.  The path of ``ft2d.ft2d_audio``: one STFT of the whole signal, ``duet`` on it, the masked magnitudes with the
    mixture's phase through one ``audio.griffinlim(n_iter=0)``, trimmed to n samples.  At most 32 768 frames."""
    _check_duet_audio_params(num_sources, attenuation, delay, p, q, smooth, min_distance, residual)
    t = audio._tensor(y, "y")
    if t.dim() != 2 or t.shape[0] != 2:
        raise ValueError("y: expected two channels [2, n], got %s" % (tuple(t.shape),))
    x = audio._long_audio(t)
    n = x.shape[1]
    if 1 + -(-n // audio.HOP) > MAX_FRAMES:
        raise ValueError("y: expected at most %d frames (%d samples), got %d samples" % (MAX_FRAMES, (MAX_FRAMES - 2) * audio.HOP, n))
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [2, 1025, F]
    masks = duet(X, num_sources, attenuation, delay, p, q, smooth, min_distance, mask=True)   # [S, 1025, F]
    S = masks.shape[0]
    mag = (masks[:, None] * X.abs()[None]).reshape((2 * S,) + tuple(X.shape[1:]))
    phase = torch.polar(torch.ones_like(X.real), X.angle()).repeat(S, 1, 1)
    stems = audio.griffinlim(mag, n_iter=0, init=phase)[:, :n].reshape(S, 2, n).contiguous()
    return (stems, x - stems.sum(0)) if residual else stems


def separate_wav_duet(path, num_sources, out_rate="input", **kwargs):
    """``duet_audio`` for a two-channel PCM wav at any rate -> ``(stems, rate)``, the wrapper ``ft2d.separate_wav_ft2d`` is around
    ``ft2d_audio``: stems [S, 2, n'] ([S + 1, 2, n'] with ``residual=True``, the residual last) at ``out_rate``: 'input' (the file's
    rate and exactly its sample count), an integer rate, or None (16 kHz).  ``kwargs`` are ``duet_audio``'s keyword arguments; any
    other is refused before the file is opened.  A file that does not have exactly two channels is refused."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    unknown = set(kwargs) - set(_DUET_AUDIO_DEFAULTS)
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected duet_audio's" % sorted(unknown))
    _check_duet_audio_params(num_sources, **dict(_DUET_AUDIO_DEFAULTS, **kwargs))
    y, native = audio.load_audio(path, sr=None, mono=False)
    if y.dim() != 2 or y.shape[0] != 2:
        raise ValueError("%s: expected a file with exactly two channels, got %d" % (path, 1 if y.dim() == 1 else y.shape[0]))
    n_file = y.shape[1]
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    out = duet_audio(y, num_sources, **kwargs)
    stems = torch.cat([out[0], out[1][None]]) if kwargs.get("residual", False) else out
    stems = audio.resample(stems, audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate
