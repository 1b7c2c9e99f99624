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
