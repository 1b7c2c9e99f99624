"""REPET-SIM (Rafii & Pardo 2012): separation of a foreground from a repeating background by nearest-neighbour median filtering,
with the semantics of librosa's "vocal separation" recipe -- ``librosa.decompose.nn_filter(S, aggregate=np.median,
metric='cosine', width=...)``, ``np.minimum``, two ``librosa.util.softmask`` calls.  Every frame is replaced by the per-bin median
of its most similar frames elsewhere in the signal: what repeats survives as the background, what does not becomes the
foreground.  Like ``hpss.py`` it needs no trained flows and no ground-truth stems; it is the prior-free figure for the question
the BASIS separations answer (a foreground instrument over an accompaniment).  Not in the reference.

Kernels in ``csrc/glowk_repet.h`` (``glowk_nn_neighbors``, ``glowk_nn_median``; formulas in include/glowk.h); the masks are
``glowk_hpss_mask``:

* ``neighbors``: per frame the k most cosine-similar frames at least ``width`` frames away, in decreasing similarity, equal
  similarities to the lower index, -1 where there are fewer than k candidates.  The frame-similarity matrix is a Gram matrix on
  the fp32 matrix cores with the selection in the same pass; it never exists in memory;
* ``nn_filter``: the per-row median over each frame's neighbours (a selection; at an even count the mean of the two middle ones);
* ``repet_sim``: ``rep = min(S, nn_filter(S))``, ``res = S - rep``, the two soft masks of ``librosa.util.softmask`` of each against
  the other times its margin, the masked spectra (complex input keeps its phase);
* ``repet_sim_audio``: 16 kHz audio in, stems as long as it out, the path of ``hpss.hpss_audio``;
* ``separate_wav_repet``: a PCM wav at any rate in, the stems at the file's rate and length out.

The original REPET (Rafii & Pardo 2013) and the adaptive REPET (Liutkus et al. 2012) share the filter and the masks; their front
end is in ``csrc/glowk_beat.h`` (``glowk_beat_spectrum``, ``glowk_beat_period``, ``glowk_period_neighbors``):

* ``beat_spectrum`` / ``beat_spectrogram``: the lag-wise autocorrelation of the power spectrogram, of the whole signal or per
  window -- the diagonal sums of the band of the frame Gram matrix on the fp32 matrix cores, summed in fp64;
* ``find_period``: the lag of the largest beat value in a range, equal values to the lower lag;
* ``period_neighbors``: per frame the frames whole periods away, nearest first, the index tensor ``nn_filter``'s median takes;
* ``repet`` / ``repet_adaptive``: one period per signal and the median over every repetition, or one period per window and the
  median over the ``order`` nearest; defaults ``power = 1``, ``margin = 1``: the published ratio mask;
* ``repet_audio`` / ``separate_wav_repet_periodic``: the audio and wav paths of the two.

Conventions as in ``hpss.py``: numpy or torch in, float32 (int32 for indices) tensors on the GPU the input lives on out,
ValueError for bad arguments before the library is loaded.
"""
import math

import numpy as np
import torch

from . import _lib, audio
from .audio import _p, _s

MAX_K, MAX_WIDTH = 512, 1 << 20                          # glowk_nn_neighbors: k in [1, 512], width in [1, 2^20]
MAX_ROWS, MAX_FRAMES, MAX_SIGNALS = 4096, 32768, 65535
MAX_ELEMENTS = (1 << 31) - 1


def default_k(F, width):
    """The neighbour count for F frames: ``2 ceil(sqrt(F - 2 width + 1))`` (librosa's recurrence_matrix default), in [1, 512]."""
    return min(MAX_K, max(1, 2 * math.isqrt(max(int(F) - 2 * int(width) + 1, 1) - 1) + 2))


def _check_int(v, what, top):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= v <= top:
        raise ValueError("%s: expected an integer in [1, %d], got %r" % (what, top, v))
    return int(v)


def _check_k_width(k, width):
    return (None if k is None else _check_int(k, "k", MAX_K)), _check_int(width, "width", MAX_WIDTH)


def _check_mask_params(power, margin):
    """power, (margin_background, margin_foreground) of ``repet_sim``, checked."""
    if isinstance(margin, (tuple, list)):
        if len(margin) != 2:
            raise ValueError("margin: expected a scalar or a (background, foreground) pair, got %r" % (margin,))
        margins = margin[0], margin[1]
    else:
        margins = margin, margin
    for m in margins:
        if isinstance(m, bool) or not isinstance(m, (int, float, np.integer, np.floating)) or not (math.isfinite(m) and m >= 1):
            raise ValueError("margin: expected finite numbers >= 1, got %r" % (margin,))
    if isinstance(power, bool) or not isinstance(power, (int, float, np.integer, np.floating)) or not power > 0:
        raise ValueError("power: expected a number > 0 (inf: the hard mask), got %r" % (power,))
    return float(power), (float(margins[0]), float(margins[1]))


def _spectra(S, what="S"):
    """[rows, F] or [N, rows, F] within the kernels' ranges, as a tensor where it is."""
    x = S if torch.is_tensor(S) else torch.as_tensor(np.asarray(S))
    if x.dim() not in (2, 3) or not 1 <= x.shape[-2] <= MAX_ROWS or not 1 <= x.shape[-1] <= MAX_FRAMES \
            or (x.dim() == 3 and x.shape[0] > MAX_SIGNALS) or x.numel() > MAX_ELEMENTS:
        raise ValueError("%s: expected [rows, F] or [N, rows, F] with N <= %d, 1 <= rows <= %d, 1 <= F <= %d and at most 2^31 - 1 "
                         "elements, got %s" % (what, MAX_SIGNALS, MAX_ROWS, MAX_FRAMES, tuple(x.shape)))
    return x


def _real(S, k, width):
    """S as float32 contiguous on its GPU, with k resolved."""
    k, width = _check_k_width(k, width)
    x = _spectra(S)
    if x.is_complex():
        raise ValueError("S: expected real spectra, got %s" % x.dtype)
    if k is None:
        k = default_k(x.shape[-1], width)
    nsig = x.numel() // (x.shape[-2] * x.shape[-1])
    if nsig * x.shape[-1] * k > MAX_ELEMENTS:
        raise ValueError("S: N * F * k must be at most 2^31 - 1, got N = %d, F = %d, k = %d" % (nsig, x.shape[-1], k))
    return x.to(device=audio._device(x), dtype=torch.float32).contiguous(), k, width


def _workspace(lib, x, nsig, k):
    nbytes = lib.glowk_nn_workspace_bytes(nsig, x.shape[-2], x.shape[-1], k)
    return torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=x.device), nbytes


def _neighbors(x, k, width, want_sim):
    """x: float32 contiguous [.., rows, F] on the GPU -> idx [.., F, k] int32, sim or None."""
    lib = _lib.load()
    F = x.shape[-1]
    nsig = x.numel() // (x.shape[-2] * F)
    idx = torch.empty(tuple(x.shape[:-2]) + (F, k), dtype=torch.int32, device=x.device)
    sim = torch.empty(idx.shape, dtype=torch.float32, device=x.device) if want_sim else None
    work, nbytes = _workspace(lib, x, nsig, k)
    _lib.check(lib.glowk_nn_neighbors(_p(x), nsig, x.shape[-2], F, k, width, _p(idx), None if sim is None else _p(sim), _p(work), nbytes,
                                      _s(x)))
    return idx, sim


def _median(x, idx):
    lib = _lib.load()
    F, k = x.shape[-1], idx.shape[-1]
    nsig = x.numel() // (x.shape[-2] * F)
    out = torch.empty_like(x)
    work, nbytes = _workspace(lib, x, nsig, k)
    _lib.check(lib.glowk_nn_median(_p(x), _p(idx), nsig, x.shape[-2], F, k, _p(out), _p(work), nbytes, _s(x)))
    return out


def neighbors(S, k=None, width=1, return_similarity=False):
    """The nearest neighbours of every frame of real spectra [rows, F] or [N, rows, F] -> ``idx`` [.., F, k] int32, with
    ``return_similarity`` also ``sim`` [.., F, k] float32.  The similarity of frames i and j is the cosine of their columns
    (0 for a silent frame); the candidates of frame i are the frames with ``|i - j| >= width``; ``idx[i]`` holds the k most similar
    in decreasing similarity, equal similarities to the lower index, and -1 (similarity 0) past the candidate count.  ``k`` in
    [1, 512], default ``default_k(F, width)``; ``width`` in [1, 2^20].  ``glowk_nn_neighbors``: two launches, bitwise
    reproducible, a batch gives what its signals give alone."""
    if not isinstance(return_similarity, (bool, np.bool_)):
        raise ValueError("return_similarity: expected True or False, got %r" % (return_similarity,))
    x, k, width = _real(S, k, width)
    idx, sim = _neighbors(x, k, width, bool(return_similarity))
    return (idx, sim) if return_similarity else idx


def nn_filter(S, k=None, width=1, return_neighbors=False):
    """``librosa.decompose.nn_filter(S, aggregate=np.median, metric='cosine', width=width)`` with ``k`` neighbours for real
    spectra [rows, F] or [N, rows, F]: every frame replaced by the per-row median over its ``neighbors`` (a frame with none stays).
    float32 out, shaped like S; with ``return_neighbors`` also the index tensor.  Four launches."""
    if not isinstance(return_neighbors, (bool, np.bool_)):
        raise ValueError("return_neighbors: expected True or False, got %r" % (return_neighbors,))
    x, k, width = _real(S, k, width)
    idx, _ = _neighbors(x, k, width, False)
    out = _median(x, idx)
    return (out, idx) if return_neighbors else out


def repet_sim(S, k=None, width=1, power=2.0, margin=(2.0, 10.0), mask=False):
    """REPET-SIM of spectra [rows, F] or [N, rows, F] -> ``(background, foreground)`` shaped like S.

    ``rep = min(S, nn_filter(S, k, width))`` is what repeats, ``res = S - rep`` what does not; the masks are
    ``librosa.util.softmask`` of each against the other times its ``margin`` with exponent ``power`` (inf: the hard mask), in fp32
    (``glowk_hpss_mask``).  ``margin`` (>= 1) is a scalar or a (background, foreground) pair.  Complex S is split into magnitude and
    phase, and the components come back complex64 with S's phase; real S gives float32 magnitudes.  ``mask=True`` returns the two
    masks instead.  With a margin above 1 the components no longer sum to S."""
    k, width = _check_k_width(k, width)
    power, (mb, mf) = _check_mask_params(power, margin)
    if not isinstance(mask, (bool, np.bool_)):
        raise ValueError("mask: expected True or False, got %r" % (mask,))
    x = _spectra(S)
    dev = audio._device(x)
    phase = None
    if x.is_complex():
        x = x.to(device=dev, dtype=torch.complex64)
        phase = torch.polar(torch.ones_like(x.real), x.angle())                          # exp(i angle(S)), angle(0) = 0
        x = x.abs()
    x, k, width = _real(x, k, width)
    idx, _ = _neighbors(x, k, width, False)
    rep = torch.minimum(x, _median(x, idx))
    res = x - rep
    out_b, out_f = torch.empty_like(x), torch.empty_like(x)
    _lib.check(_lib.load().glowk_hpss_mask(_p(rep), _p(res), None if mask else _p(x), x.numel(), power, mb, mf, _p(out_b), _p(out_f),
                                           _s(x)))
    if mask or phase is None:
        return out_b, out_f
    return out_b * phase, out_f * phase


def _check_audio_params(k, width_sec, power, margin, residual):
    if k is not None:
        _check_int(k, "k", MAX_K)
    if isinstance(width_sec, bool) or not isinstance(width_sec, (int, float, np.integer, np.floating)) \
            or not (math.isfinite(width_sec) and width_sec >= 0):
        raise ValueError("width_sec: expected a finite number of seconds >= 0, got %r" % (width_sec,))
    width = max(1, int(width_sec * audio.SR / audio.HOP))
    _check_int(width, "width_sec: the width in frames", MAX_WIDTH)
    _check_mask_params(power, margin)
    if not isinstance(residual, (bool, np.bool_)):
        raise ValueError("residual: expected True or False, got %r" % (residual,))
    return width


def repet_sim_audio(y, k=None, width_sec=2.0, power=2.0, margin=(2.0, 10.0), residual=False):
    """REPET-SIM for 16 kHz audio [n] or [C, n], n > 1024 -> ``(background, foreground)``, each shaped like y and aligned with it;
    with ``residual`` also ``y - background - foreground``.  One STFT of the whole signal (``audio.mel_frames``), ``repet_sim`` on
    |X| per channel with ``width = max(1, int(width_sec SR / HOP))`` frames, the masked magnitudes with the mixture's phase
    through one ``audio.griffinlim(n_iter=0)`` of all 2 C spectra, trimmed to n samples.  A channel's stems depend on that channel
    alone.  At most 32 768 frames: about 17 minutes."""
    width = _check_audio_params(k, width_sec, power, margin, residual)
    t = audio._tensor(y, "y")
    x = audio._long_audio(t)
    if x.shape[0] > MAX_SIGNALS:
        raise ValueError("y: expected at most %d channels, got %d" % (MAX_SIGNALS, x.shape[0]))
    lead, n = tuple(t.shape[:-1]), x.shape[1]
    if 1 + -(-n // audio.HOP) > MAX_FRAMES:
        raise ValueError("y: expected at most %d frames (%d samples), got %d samples" % (MAX_FRAMES, (MAX_FRAMES - 2) * audio.HOP, n))
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [C, 1025, F]
    mags = torch.cat(repet_sim(X.abs(), k=k, width=width, power=power, margin=margin))   # [2 C, 1025, F]
    phase = torch.polar(torch.ones_like(X.real), X.angle())
    stems = audio.griffinlim(mags, n_iter=0, init=torch.cat([phase, phase]))[:, :n].reshape((2,) + lead + (n,))
    b, f = stems[0].contiguous(), stems[1].contiguous()
    return (b, f, x.reshape(lead + (n,)) - b - f) if residual else (b, f)


def separate_wav_repet(path, out_rate="input", mono=False, **kwargs):
    """``repet_sim_audio`` for a PCM wav at any rate -> ``(stems, rate)``: stems [2, n'] (background, foreground; [3, n'] with
    ``residual=True``) of a one-channel file or with ``mono`` (the channels averaged), else [2 or 3, C, n'] with the file's C
    channels, at ``out_rate``: 'input' (the file's rate), an integer rate, or None (left at 16 kHz).  The file is resampled to 16 kHz
    on the GPU, the stems back in one launch; with ``out_rate='input'`` they have exactly the file's sample count.  ``kwargs`` are
    ``repet_sim_audio``'s keyword arguments."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    unknown = set(kwargs) - {"k", "width_sec", "power", "margin", "residual"}
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected repet_sim_audio's" % sorted(unknown))
    _check_audio_params(kwargs.get("k"), kwargs.get("width_sec", 2.0), kwargs.get("power", 2.0), kwargs.get("margin", (2.0, 10.0)),
                        kwargs.get("residual", False))
    y, native = audio.load_audio(path, sr=None, mono=False)
    n_file = y.shape[1]
    y = y.mean(0) if mono or y.shape[0] == 1 else y
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    stems = audio.resample(torch.stack(repet_sim_audio(y, **kwargs)), audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate


# ---- REPET and adaptive REPET: the period from the beat spectrum, the median over the frames whole periods away ---------------------
def _check_flag(v, what):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("%s: expected True or False, got %r" % (what, v))
    return bool(v)


def _check_range_int(v, what, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError("%s: expected an integer in [%d, %d], got %r" % (what, lo, hi, v))
    return int(v)


def _real32(S):
    """Real spectra [rows, F] or [N, rows, F] as float32 contiguous on their GPU."""
    x = _spectra(S)
    if x.is_complex():
        raise ValueError("S: expected real spectra, got %s" % x.dtype)
    return x.to(device=audio._device(x), dtype=torch.float32).contiguous()


def _nsig(x):
    return x.numel() // (x.shape[-2] * x.shape[-1])


def _check_beat(x, nlags, win, step):
    """(nlags, win, step, nwin) of a beat spectrogram of spectra shaped like x (win = 0: the beat spectrum), checked."""
    F = x.shape[-1]
    if win != 0:
        if F < 2:
            raise ValueError("S: a beat spectrogram needs at least 2 frames, got %d" % F)
        win = _check_range_int(win, "win", 2, F)
        step = max(1, win // 2) if step is None else _check_range_int(step, "step", 1, win)
    nlags = (F if win == 0 else win) if nlags is None else _check_range_int(nlags, "nlags", 1, F)
    nwin = 1 if win == 0 else -(-F // step)
    nsig = x.numel() // (x.shape[-2] * F) if x.dim() == 3 else 1
    if nsig * nwin * nlags > MAX_ELEMENTS:
        raise ValueError("S: N * nwin * nlags must be at most 2^31 - 1, got N = %d, nwin = %d, nlags = %d" % (nsig, nwin, nlags))
    return nlags, win, (0 if win == 0 else step), nwin


def _beat(x, nlags, win, step, nwin):
    """x: float32 contiguous [.., rows, F] on the GPU -> beat [.., nwin, nlags] float32."""
    lib = _lib.load()
    rows, F = x.shape[-2], x.shape[-1]
    nsig = _nsig(x)
    beat = torch.empty(tuple(x.shape[:-2]) + (nwin, nlags), dtype=torch.float32, device=x.device)
    nbytes = lib.glowk_beat_workspace_bytes(nsig, rows, F, nlags, win, step)
    if nsig and not nbytes:
        raise _lib.GlowkError("glowk_beat_workspace_bytes: %s" % lib.glowk_last_error().decode())
    work = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=x.device)
    _lib.check(lib.glowk_beat_spectrum(_p(x), nsig, rows, F, nlags, win, step, _p(beat), _p(work), nbytes, _s(x)))
    return beat


def beat_spectrum(S, nlags=None):
    """The beat spectrum of real spectra [rows, F] or [N, rows, F] -> [.., nlags] float32: the autocorrelation over the frames of
    the power spectrogram ``P = S * S``, averaged over the rows and the pairs, normalised by lag 0 --
    ``b[l] = (sum_r sum_j P[r, j] P[r, j + l] / (rows (F - l))) / (sum_r sum_j P[r, j]^2 / (rows F))``; all zeros for a silent
    signal.  ``nlags`` in [1, F], default F: only these lags are computed (the band of the frame Gram matrix of P on the fp32 matrix
    cores, summed along its diagonals in fp64; formulas and error bound in include/glowk.h).  ``glowk_beat_spectrum``: two
    launches, bitwise reproducible, a batch gives what its signals give alone."""
    x0 = _spectra(S)
    nlags, _, _, _ = _check_beat(x0, nlags, 0, 0)
    x = _real32(x0)
    return _beat(x, nlags, 0, 0, 1).squeeze(-2)


def beat_spectrogram(S, win, step=None, nlags=None):
    """The beat spectrogram of real spectra [rows, F] or [N, rows, F] -> [.., nwin, nlags] float32, ``nwin = ceil(F / step)``: the
    beat spectrum of window t, the frames ``[t step - win // 2, t step - win // 2 + win)`` that lie inside the signal (the first and
    last windows are shorter), both frames of a pair inside the window; 0 at the lags a window is too short for and for a silent
    window.  ``win`` in [2, F], ``step`` in [1, win] (default ``win // 2``), ``nlags`` in [1, F] (default ``win``)."""
    x0 = _spectra(S)
    if isinstance(win, (bool, np.bool_)) or not isinstance(win, (int, np.integer)) or win == 0:
        raise ValueError("win: expected an integer in [2, F], got %r" % (win,))
    nlags, win, step, nwin = _check_beat(x0, nlags, win, step)
    return _beat(_real32(x0), nlags, win, step, nwin)


def find_period(beat, pmin, pmax):
    """The repeating period of beat spectra [.., nlags] -> int32, shaped like ``beat`` without its last axis: the lag in
    ``[pmin, pmax]`` with the largest value, equal values to the lower lag (so all zeros give ``pmin``).
    ``1 <= pmin <= pmax <= nlags - 1``.  ``glowk_beat_period``: one launch."""
    b = beat if torch.is_tensor(beat) else torch.as_tensor(np.asarray(beat))
    if b.dim() < 1 or b.is_complex() or not b.is_floating_point() or not 2 <= b.shape[-1] <= MAX_FRAMES or b.numel() > MAX_ELEMENTS:
        raise ValueError("beat: expected real [.., nlags] with 2 <= nlags <= %d and at most 2^31 - 1 elements, got %s %s"
                         % (MAX_FRAMES, b.dtype, tuple(b.shape)))
    nlags = b.shape[-1]
    pmin = _check_range_int(pmin, "pmin", 1, nlags - 1)
    pmax = _check_range_int(pmax, "pmax", pmin, nlags - 1)
    b = b.to(device=audio._device(b), dtype=torch.float32).contiguous()
    period = torch.empty(tuple(b.shape[:-1]), dtype=torch.int32, device=b.device)
    _lib.check(_lib.load().glowk_beat_period(_p(b), b.numel() // nlags, nlags, pmin, pmax, _p(period), _s(b)))
    return period


def _check_periods(period, step):
    """period as an integer tensor where it is, [..] (one per signal) or with ``step`` [.., nper]; and nper."""
    if isinstance(period, (bool, np.bool_)):
        raise ValueError("period: expected integers, got %r" % (period,))
    p = period if torch.is_tensor(period) else torch.as_tensor(np.asarray(period))
    if p.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
        raise ValueError("period: expected integers, got %s" % p.dtype)
    if step is not None and p.dim() < 1:
        raise ValueError("period: with step expected [.., nper], one period per window, got a scalar")
    nper = 1 if step is None else p.shape[-1]
    if not 1 <= nper <= MAX_FRAMES:
        raise ValueError("period: expected 1 to %d periods per signal, got %d" % (MAX_FRAMES, nper))
    return p, nper


def period_neighbors(period, frames, k, step=None):
    """The periodic neighbours -> ``idx`` int32 [.., frames, k], the index tensor ``glowk_nn_median`` filters over.  Without
    ``step``, ``period`` (an integer or integers [..]) holds one period per signal; with it, ``period`` is [.., nper], one period per
    window, and frame j uses entry ``min((j + step // 2) // step, nper - 1)``.  A period below 1 counts as 1.  ``idx[j]`` lists the
    frames ``j + i p`` for i = 0, -1, +1, -2, +2, .. in that order: those inside ``[0, frames)`` until ``k`` are kept, then -1.  With
    ``k >= ceil(frames / p)`` that is every frame congruent to j mod p; with a small k the k nearest repetitions.  ``frames`` in
    [1, 32768], ``k`` in [1, 512], ``step`` in [1, 32768].  ``glowk_period_neighbors``: one launch."""
    frames = _check_range_int(frames, "frames", 1, MAX_FRAMES)
    k = _check_int(k, "k", MAX_K)
    if step is not None:
        step = _check_range_int(step, "step", 1, MAX_FRAMES)
    p, nper = _check_periods(period, step)
    lead = tuple(p.shape) if step is None else tuple(p.shape[:-1])
    nsig = p.numel() // nper
    if nsig > MAX_SIGNALS or nsig * frames * k > MAX_ELEMENTS:
        raise ValueError("period: expected at most %d signals and N * frames * k <= 2^31 - 1, got N = %d, frames = %d, k = %d"
                         % (MAX_SIGNALS, nsig, frames, k))
    p = p.to(device=audio._device(p), dtype=torch.int32).contiguous()
    idx = torch.empty(lead + (frames, k), dtype=torch.int32, device=p.device)
    _lib.check(_lib.load().glowk_period_neighbors(_p(p), nsig, frames, nper, 1 if step is None else step, k, _p(idx), _s(p)))
    return idx


def _check_period_range(period_range, top, what="period_range"):
    """(pmin, pmax) with 1 <= pmin <= pmax <= top; None: (2, top)."""
    if period_range is None:
        period_range = (2, top)
    if not isinstance(period_range, (tuple, list)) or len(period_range) != 2:
        raise ValueError("%s: expected a (pmin, pmax) pair, got %r" % (what, period_range))
    pmin, pmax = period_range
    for v in (pmin, pmax):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s: expected two integers, got %r" % (what, period_range))
    if not 1 <= pmin <= pmax <= top:
        raise ValueError("%s: expected 1 <= pmin <= pmax <= %d (the range is empty for so few frames), got %r" % (what, top, tuple(period_range)))
    return int(pmin), int(pmax)


def _magnitude(S):
    """(|S| float32 contiguous on the GPU, exp(i angle(S)) or None for real S)."""
    x = _spectra(S)
    dev = audio._device(x)
    phase = None
    if x.is_complex():
        x = x.to(device=dev, dtype=torch.complex64)
        phase = torch.polar(torch.ones_like(x.real), x.angle())
        x = x.abs()
    return x.to(device=dev, dtype=torch.float32).contiguous(), phase


def _median_and_masks(x, idx, power, mb, mf, mask, phase):
    rep = torch.minimum(x, _median(x, idx))
    res = x - rep
    out_b, out_f = torch.empty_like(x), torch.empty_like(x)
    _lib.check(_lib.load().glowk_hpss_mask(_p(rep), _p(res), None if mask else _p(x), x.numel(), power, mb, mf, _p(out_b), _p(out_f),
                                           _s(x)))
    if mask or phase is None:
        return out_b, out_f
    return out_b * phase, out_f * phase


def _host_period(period):
    p = period.cpu().numpy()
    return int(p) if p.ndim == 0 else p


def repet(S, period=None, period_range=None, k=None, power=1.0, margin=1.0, mask=False, return_period=False):
    """REPET (Rafii & Pardo 2013) of spectra [rows, F] or [N, rows, F] -> ``(background, foreground)`` shaped like S.

    The period is ``find_period(beat_spectrum(|S|, pmax + 1), pmin, pmax)`` with ``period_range = (pmin, pmax)``, default
    ``(2, F // 3)``: three repetitions at least (ValueError if that is empty) -- or ``period``, an integer or one integer per
    signal.  The repeating model is the per-row median over the frames whole periods away, ``period_neighbors(period, F, k)`` with
    ``k = min(512, ceil(F / pmin))`` (every such frame, the frame itself included: the segment median of the publication; with a
    given period ``ceil(F / period)``, and ``min(512, F)`` where the periods are a tensor, whose values the host does not read);
    ``rep = min(|S|, median)``, ``res = |S| - rep``, and the masks are those of ``repet_sim``, whose defaults here, ``power = 1`` and
    ``margin = 1``, give the published ratio mask ``rep / |S|``.  Complex S keeps its phase; ``mask=True`` returns the masks.  With
    ``return_period`` a third result, the period as an int (an int32 array [N] for a batch): the only host synchronisation."""
    power, (mb, mf) = _check_mask_params(power, margin)
    mask, return_period = _check_flag(mask, "mask"), _check_flag(return_period, "return_period")
    if k is not None:
        k = _check_int(k, "k", MAX_K)
    x0 = _spectra(S)
    F = x0.shape[-1]
    lead = tuple(x0.shape[:-2])
    if period is None:
        pmin, pmax = _check_period_range(period_range, F // 3 if period_range is None else F - 1)
        k = min(MAX_K, -(-F // pmin)) if k is None else k
    else:
        if period_range is not None:
            raise ValueError("period_range: not used with a given period")
        period, _ = _check_periods(period, None)
        if tuple(period.shape) not in ((), lead):
            raise ValueError("period: expected one integer or integers shaped %s, got %s" % (lead, tuple(period.shape)))
        if period.dim() == 0:
            if int(period) < 1:
                raise ValueError("period: expected a period >= 1, got %d" % int(period))
            k = min(MAX_K, -(-F // int(period))) if k is None else k
        else:
            k = min(MAX_K, F) if k is None else k
    if max(x0.numel() // (x0.shape[-2] * F), 1) * F * k > MAX_ELEMENTS:
        raise ValueError("S: N * F * k must be at most 2^31 - 1, got F = %d, k = %d" % (F, k))
    if period is None:
        _check_beat(x0, pmax + 1, 0, 0)
    x, phase = _magnitude(x0)
    if period is None:
        period = find_period(_beat(x, pmax + 1, 0, 0, 1).squeeze(-2), pmin, pmax)
    else:
        period = period.to(device=x.device, dtype=torch.int32).expand(lead).contiguous()
    idx = period_neighbors(period, F, k)
    out = _median_and_masks(x, idx, power, mb, mf, mask, phase)
    return out + (_host_period(period),) if return_period else out


def repet_adaptive(S, win, step=None, period_range=None, order=5, power=1.0, margin=1.0, mask=False, return_period=False):
    """Adaptive REPET (Liutkus, Rafii, Pardo, Pardo & Richard 2012) of spectra [rows, F] or [N, rows, F] -> ``(background,
    foreground)``: one period per window from ``beat_spectrogram(|S|, win, step, pmax + 1)`` (``period_range`` default
    ``(2, win // 3)``), frame j filtered with the period of the window centred nearest to it over its ``order`` nearest repetitions
    (``period_neighbors(periods, F, order, step)``), then as ``repet``.  With ``return_period`` also the periods, an int32 array
    [.., nwin] on the host."""
    power, (mb, mf) = _check_mask_params(power, margin)
    mask, return_period = _check_flag(mask, "mask"), _check_flag(return_period, "return_period")
    order = _check_int(order, "order", MAX_K)
    x0 = _spectra(S)
    F = x0.shape[-1]
    if isinstance(win, (bool, np.bool_)) or not isinstance(win, (int, np.integer)) or not 2 <= win <= F:
        raise ValueError("win: expected an integer in [2, F = %d], got %r" % (F, win))
    pmin, pmax = _check_period_range(period_range, win // 3 if period_range is None else min(win, F) - 1)
    nlags, win, step, nwin = _check_beat(x0, pmax + 1, win, step)
    if max(x0.numel() // (x0.shape[-2] * F), 1) * F * order > MAX_ELEMENTS:
        raise ValueError("S: N * F * order must be at most 2^31 - 1, got F = %d, order = %d" % (F, order))
    x, phase = _magnitude(x0)
    period = find_period(_beat(x, nlags, win, step, nwin), pmin, pmax)
    idx = period_neighbors(period, F, order, step)
    out = _median_and_masks(x, idx, power, mb, mf, mask, phase)
    return out + (_host_period(period),) if return_period else out


_REPET_AUDIO_DEFAULTS = dict(adaptive=False, period_sec=(0.8, 8.0), win_sec=10.0, step_sec=5.0, order=5, cutoff_hz=100.0, power=1.0,
                             margin=1.0, residual=False)


def _check_repet_audio_params(adaptive, period_sec, win_sec, step_sec, order, cutoff_hz, power, margin, residual):
    """The arguments of ``repet_audio`` that do not depend on the signal, checked -> (pmin, pmax, win, step, cutoff rows) in frames
    and rows, before any cap by the signal's length."""
    _check_flag(adaptive, "adaptive")
    _check_flag(residual, "residual")
    _check_mask_params(power, margin)
    _check_int(order, "order", MAX_K)
    number = lambda v: not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)
    if not isinstance(period_sec, (tuple, list)) or len(period_sec) != 2 or not all(number(v) for v in period_sec) \
            or not 0 < period_sec[0] <= period_sec[1]:
        raise ValueError("period_sec: expected (shortest, longest) in seconds with 0 < shortest <= longest, got %r" % (period_sec,))
    fps = audio.SR / audio.HOP
    if period_sec[1] * fps > MAX_FRAMES:
        raise ValueError("period_sec: expected periods of at most %d frames, got %r" % (MAX_FRAMES, period_sec))
    pmin, pmax = max(1, math.ceil(period_sec[0] * fps)), math.floor(period_sec[1] * fps)
    if pmin > pmax:
        raise ValueError("period_sec: no whole number of frames (%g per second) lies in %r" % (fps, period_sec))
    for name, v in (("win_sec", win_sec), ("step_sec", step_sec)):
        if not number(v) or not 0 < v * fps <= MAX_FRAMES:
            raise ValueError("%s: expected a number of seconds > 0, at most %d frames, got %r" % (name, MAX_FRAMES, v))
    if step_sec > win_sec:
        raise ValueError("step_sec: expected at most win_sec = %r, got %r" % (win_sec, step_sec))
    if not number(cutoff_hz) or not 0 <= cutoff_hz <= audio.SR / 2:
        raise ValueError("cutoff_hz: expected a frequency in [0, %g] (0: no cutoff), got %r" % (audio.SR / 2, cutoff_hz))
    n_fft = 2 * (audio.NBIN - 1)
    cut = 0 if cutoff_hz == 0 else min(audio.NBIN, math.floor(cutoff_hz * n_fft / audio.SR) + 1)
    return pmin, pmax, max(2, int(win_sec * fps)), max(1, int(step_sec * fps)), cut


def repet_audio(y, adaptive=False, period_sec=(0.8, 8.0), win_sec=10.0, step_sec=5.0, order=5, cutoff_hz=100.0, power=1.0, margin=1.0,
                residual=False):
    """REPET for 16 kHz audio [n] or [C, n], n > 1024 -> ``(background, foreground)``, each shaped like y and aligned with it; with
    ``residual`` also ``y - background - foreground``.  The path of ``repet_sim_audio``: one STFT of the whole signal, ``repet`` (or,
    with ``adaptive``, ``repet_adaptive`` with windows of ``win_sec`` every ``step_sec`` and ``order`` repetitions) on |X| per
    channel, the masked magnitudes with the mixture's phase through one ``audio.griffinlim(n_iter=0)``, trimmed to n samples.
    ``period_sec`` is the admissible period in seconds: in frames ``ceil(shortest SR / HOP) .. floor(longest SR / HOP)``, the upper
    end capped at a third of the signal (of the window with ``adaptive``); ValueError if nothing is left.  The STFT rows r with
    ``r SR / n_fft <= cutoff_hz`` go wholly to the background, as in the publication (0: none do)."""
    pmin, pmax, win, step, cut = _check_repet_audio_params(adaptive, period_sec, win_sec, step_sec, order, cutoff_hz, power, margin, residual)
    t = audio._tensor(y, "y")
    x = audio._long_audio(t)
    if x.shape[0] > MAX_SIGNALS:
        raise ValueError("y: expected at most %d channels, got %d" % (MAX_SIGNALS, x.shape[0]))
    lead, n = tuple(t.shape[:-1]), x.shape[1]
    F = 1 + -(-n // audio.HOP)
    if F > MAX_FRAMES:
        raise ValueError("y: expected at most %d frames (%d samples), got %d samples" % (MAX_FRAMES, (MAX_FRAMES - 2) * audio.HOP, n))
    win, step = min(win, F), min(step, win, F)
    pmax = min(pmax, (win if adaptive else F) // 3)
    if pmin > pmax:
        raise ValueError("period_sec: the shortest period, %d frames, is more than a third of the %s (%d frames)"
                         % (pmin, "window" if adaptive else "signal", win if adaptive else F))
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [C, 1025, F]
    mag = X.abs()
    if adaptive:
        b, f = repet_adaptive(mag, win, step, (pmin, pmax), order, power, margin)
    else:
        b, f = repet(mag, None, (pmin, pmax), None, power, margin)
    if cut:
        b[:, :cut], f[:, :cut] = mag[:, :cut], 0.0
    phase = torch.polar(torch.ones_like(X.real), X.angle())
    stems = audio.griffinlim(torch.cat([b, f]), n_iter=0, init=torch.cat([phase, phase]))[:, :n].reshape((2,) + lead + (n,))
    b, f = stems[0].contiguous(), stems[1].contiguous()
    return (b, f, x.reshape(lead + (n,)) - b - f) if residual else (b, f)


def separate_wav_repet_periodic(path, out_rate="input", mono=False, **kwargs):
    """``repet_audio`` for a PCM wav at any rate -> ``(stems, rate)``, the wrapper ``separate_wav_repet`` is around
    ``repet_sim_audio``: stems [2, n'] (background, foreground; [3, n'] with ``residual=True``) of a one-channel file or with ``mono``,
    else [2 or 3, C, n'], at ``out_rate``: 'input' (the file's rate and exactly its sample count), an integer rate, or None (16 kHz).
    ``kwargs`` are ``repet_audio``'s keyword arguments; any other is refused before the file is opened."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    _check_flag(mono, "mono")
    unknown = set(kwargs) - set(_REPET_AUDIO_DEFAULTS)
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected repet_audio's" % sorted(unknown))
    _check_repet_audio_params(**dict(_REPET_AUDIO_DEFAULTS, **kwargs))
    y, native = audio.load_audio(path, sr=None, mono=False)
    n_file = y.shape[1]
    y = y.mean(0) if mono or y.shape[0] == 1 else y
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    stems = audio.resample(torch.stack(repet_audio(y, **kwargs)), audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate
