"""Convolutive NMF (Smaragdis 2004, "NMFD"; Schmidt & Morup 2006; Smaragdis 2007 for supervised separation with convolutive bases):
every component is a small spectrogram patch of ``Tw`` frames instead of one spectrum, and the activations say where the patches
start.  What ``nmf.py`` cannot model -- an attack, a decay, a glide: sources whose long-term spectra agree and whose motion over a
few frames does not -- at the same surface.  Not in the reference.

V [.., rows, T] >= 0, W [.., rows, K, Tw], H [.., K, T]; ``K Tw <= 128``, ``Tw <= 32``.  The model is NMF on the ``K Tw`` stacked
components ``s = k Tw + tau`` with the dictionary ``W.reshape(.., rows, K Tw)`` and the activations ``stack(H, Tw)``,
``Hs[s, t] = H[k, t - tau]`` (0 for ``t < tau``), which the kernels never store.

Kernels in ``csrc/glowk_nmfd.h`` (formulas and error bounds in include/glowk.h):

* ``update_h`` / ``update_w`` / ``fit``: multiplicative updates for beta = 0, 1, 2.  The W update is the NMF W update on the stacked
  problem, bit for bit; the H update is the joint one over the ``Tw`` shifts.  One iteration is the W update (with the old H), then
  the H update (with the new W);
* ``divergence``, ``masks``: ``nmf``'s on the stacked problem, bit for bit (the sources own ranges of components);
* ``stack``, ``init``, ``decompose``, ``learn_dictionary``, ``nmfd_separate``, ``nmfd_audio``, ``separate_wav_nmfd``.

Conventions as in ``nmf.py``: numpy or torch in, tensors on the GPU the input lives on out, ValueError for bad arguments before the
library is loaded, no host synchronisation.  Results are bitwise reproducible and a batch gives what its signals give alone.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, audio
from .audio import _p, _s
from .nmf import (MAX_COMPONENTS, MAX_ITER, MAX_SOURCES, _check_beta, _check_mixture, _check_power, _check_seed, _check_separate_params, _check_sizes, _nonneg,
                  _own, _scale, _work)
from .repet import MAX_ELEMENTS, MAX_FRAMES, MAX_ROWS, MAX_SIGNALS, _check_flag, _check_range_int

MAX_TEMPLATE_FRAMES, MAX_STACKED = 32, 128
NMFD_STREAM = 11            # device RNG stream of ``init`` (0-3 serve the flows, 12 nmf / ilrma, 13 griffinlim, 14 / 15 separate_audio)


def _check_tw(Tw, K=None):
    Tw = _check_range_int(Tw, "Tw", 1, MAX_TEMPLATE_FRAMES)
    if K is not None and K * Tw > MAX_STACKED:
        raise ValueError("K * Tw: expected at most %d stacked components, got %d * %d" % (MAX_STACKED, K, Tw))
    return Tw


def _check_shapes(v, w, h, update_w):
    """V [.., R, T], W [.., R, K, Tw] (or one [R, K, Tw] for a batch when it is not updated), H [.., K, T] -> (nsig, R, T, K, Tw, nw)."""
    R, T = v.shape[-2], v.shape[-1]
    if not 1 <= R <= MAX_ROWS or not 1 <= T <= MAX_FRAMES or (v.dim() == 3 and v.shape[0] > MAX_SIGNALS) or v.numel() > MAX_ELEMENTS:
        raise ValueError("V: expected [rows, T] or [N, rows, T] with N <= %d, 1 <= rows <= %d, 1 <= T <= %d and at most 2^31 - 1 elements, "
                         "got %s" % (MAX_SIGNALS, MAX_ROWS, MAX_FRAMES, tuple(v.shape)))
    lead = tuple(v.shape[:-2])
    K, Tw = w.shape[-2], w.shape[-1]
    if not 1 <= K <= MAX_COMPONENTS or not 1 <= Tw <= MAX_TEMPLATE_FRAMES or K * Tw > MAX_STACKED:
        raise ValueError("W: expected [.., rows, K, Tw] with 1 <= K, 1 <= Tw <= %d and K * Tw <= %d, got %s" % (MAX_TEMPLATE_FRAMES, MAX_STACKED, tuple(w.shape)))
    if w.shape[-3] != R or tuple(w.shape[:-3]) not in (lead, ()):
        raise ValueError("W: expected %s + (%d, K, Tw) for V %s, got %s" % (lead, R, tuple(v.shape), tuple(w.shape)))
    nsig = v.shape[0] if v.dim() == 3 else 1
    shared = v.dim() == 3 and w.dim() == 3
    if shared and update_w:
        raise ValueError("W: one dictionary shared by a batch cannot be updated (update_w needs W %s + (%d, K, Tw))" % (lead, R))
    if tuple(h.shape) != lead + (K, T):
        raise ValueError("H: expected %s, got %s" % (lead + (K, T), tuple(h.shape)))
    if nsig * K * Tw * T > MAX_ELEMENTS or nsig * R * K * Tw > MAX_ELEMENTS:
        raise ValueError("W, stack(H): at most 2^31 - 1 elements each")
    return nsig, R, T, K, Tw, (1 if shared else nsig)


def _prepare(V, W, H, update_w):
    v, w, h = _nonneg(V, "V"), _nonneg(W, "W", (3, 4)), _nonneg(H, "H")
    dims = _check_shapes(v, w, h, update_w)
    dev = audio._device(v, w, h)
    return tuple(t.to(device=dev, dtype=torch.float32).contiguous() for t in (v, w, h)) + (dims,)


def _fit(v, w, h, dims, beta, n_iter, mode):
    """In place on w and h (float32 contiguous on v's GPU).  mode: glowk_nmfd_fit's update_w."""
    nsig, R, T, K, Tw, nw = dims
    if nsig == 0 or n_iter == 0:
        return
    lib = _lib.load()
    nbytes = lib.glowk_nmfd_workspace_bytes(nsig, R, T, K, Tw)
    work = _work(nbytes, v.device)
    _lib.check(lib.glowk_nmfd_fit(_p(v), nsig, R, T, _p(w), nw, _p(h), K, Tw, beta, n_iter, mode, _p(work), nbytes, _s(v)))


def stack(H, Tw):
    """The stacked activations ``Hs [.., K Tw, T]`` of H [.., K, T]: ``Hs[k Tw + tau, t] = H[k, t - tau]``, 0 for ``t < tau``.  The
    kernels never build it; with ``W.reshape(.., rows, K Tw)`` it is the NMF problem they solve."""
    h = H if torch.is_tensor(H) else torch.as_tensor(np.asarray(H))
    if h.is_complex() or h.dtype == torch.bool or h.dim() not in (2, 3):
        raise ValueError("H: expected a real array [K, T] or [N, K, T], got %s %s" % (h.dtype, tuple(h.shape)))
    Tw = _check_tw(Tw)
    K, T = h.shape[-2], h.shape[-1]
    out = h.new_zeros(tuple(h.shape[:-2]) + (K, Tw, T))
    for tau in range(min(Tw, T)):
        out[..., :, tau, tau:] = h[..., :, :T - tau]
    return out.reshape(tuple(h.shape[:-2]) + (K * Tw, T))


def init(V, K, Tw, seed=0):
    """The starting point ``(W0 [.., rows, K, Tw], H0 [.., K, T])``: uniforms of the device RNG (stream 11, step 0 for W and 1 for H,
    element order that of the arrays), which are never zero, times ``sqrt(mean(V) / (K Tw))`` per signal (the mean in float64, rounded
    to float32)."""
    K = _check_range_int(K, "K", 1, MAX_COMPONENTS)
    Tw = _check_tw(Tw, K)
    seed = _check_seed(seed)
    v = _nonneg(V, "V")
    R, T = v.shape[-2], v.shape[-1]
    lead = tuple(v.shape[:-2])
    _check_shapes(v, torch.empty(lead + (R, K, Tw), device="meta"), torch.empty(lead + (K, T), device="meta"), False)
    v = v.to(device=audio._device(v), dtype=torch.float32)
    lib = _lib.load()
    w = torch.empty(lead + (R, K, Tw), dtype=torch.float32, device=v.device)
    h = torch.empty(lead + (K, T), dtype=torch.float32, device=v.device)
    for t, step in ((w, 0), (h, 1)):
        if t.numel():
            _lib.check(lib.glowk_random(_p(t), t.numel(), seed, step, NMFD_STREAM, 1, 0, _s(t)))
    scale = _scale(v, K * Tw) if v.numel() else v.new_zeros(lead + (1, 1))
    return w * scale[..., None], h * scale


def fit(V, W, H, beta=1, n_iter=1, update_w=True):
    """``n_iter`` iterations from (W, H) -> ``(W', H')``, new float32 tensors; the inputs stay.  V [rows, T] or [N, rows, T] >= 0,
    W [.., rows, K, Tw], H [.., K, T].  With ``update_w=False`` W stays (and is returned as it is on the GPU) and a batch may share
    one W [rows, K, Tw].  ``4 n_iter`` launches (``2 n_iter`` without the W update)."""
    beta = _check_beta(beta)
    n_iter = _check_range_int(n_iter, "n_iter", 0, MAX_ITER)
    update_w = _check_flag(update_w, "update_w")
    v, w, h, dims = _prepare(V, W, H, update_w)
    w, h = (_own(w, W) if update_w else w), _own(h, H)
    _fit(v, w, h, dims, beta, n_iter, 1 if update_w else 0)
    return w, h


def update_h(V, W, H, beta=1):
    """One joint H update: ``N[k, t] = sum_tau sum_f W[f, k, tau] Q[f, t + tau]``, D with P, ``H' = H g(N / max(D, FLOOR))`` -> H'."""
    beta = _check_beta(beta)
    v, w, h, dims = _prepare(V, W, H, False)
    h = _own(h, H)
    _fit(v, w, h, dims, beta, 1, 0)
    return h


def update_w(V, W, H, beta=1):
    """One W update: ``W' = W g(Q Hs^T / max(P Hs^T, FLOOR))`` -> W', a new tensor."""
    beta = _check_beta(beta)
    v, w, h, dims = _prepare(V, W, H, True)
    w = _own(w, W)
    _fit(v, w, h, dims, beta, 1, 2)
    return w


def divergence(V, W, H, beta=1):
    """``D_beta(V | Ws Hs)`` -> float64, one value per signal ([N], or a scalar tensor for one signal)."""
    beta = _check_beta(beta)
    v, w, h, dims = _prepare(V, W, H, False)
    nsig, R, T, K, Tw, nw = dims
    out = torch.zeros(tuple(v.shape[:-2]), dtype=torch.float64, device=v.device)
    if nsig:
        lib = _lib.load()
        nbytes = lib.glowk_nmfd_workspace_bytes(nsig, R, T, K, Tw)
        work = _work(nbytes, v.device)
        _lib.check(lib.glowk_nmfd_divergence(_p(v), nsig, R, T, _p(w), nw, _p(h), K, Tw, beta, _p(out), _p(work), nbytes, _s(v)))
    return out


def decompose(S, n_components, template_frames, beta=1, n_iter=200, seed=0):
    """S [rows, T] (or a batch [N, rows, T]) >= 0 -> ``(templates [.., rows, K, Tw], activations [.., K, T])`` after ``n_iter``
    iterations from ``init(S, K, Tw, seed)``."""
    beta = _check_beta(beta)
    n_iter = _check_range_int(n_iter, "n_iter", 0, MAX_ITER)
    w, h = init(S, n_components, template_frames, seed)
    return fit(S, w, h, beta, n_iter, True)


def learn_dictionary(S, K, Tw, beta=1, n_iter=200, seed=0):
    """The templates W [.., rows, K, Tw] of ``decompose(S, K, Tw, ..)``: what an instrument's isolated material is made of."""
    return decompose(S, K, Tw, beta, n_iter, seed)[0]


def _masks(w, h, dims, bounds, power, x, C):
    nsig, R, T, K, Tw, nw = dims
    S = len(bounds) - 1
    lead = tuple(h.shape[:-2])
    m = torch.empty(lead + (S, R, T), dtype=torch.float32, device=h.device)
    spec = None if x is None else torch.empty(lead + (S, C, R, T), dtype=torch.complex64, device=h.device)
    if nsig:
        _lib.check(_lib.load().glowk_nmfd_masks(_p(w), nw, _p(h), nsig, R, T, K, Tw, bounds.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), S, power,
                                                _p(x), C, _p(m), _p(spec), _s(h)))
    return m, spec


def masks(W, H, sizes, power=1, X=None):
    """Ratio masks of the sources that own ``sizes[0], sizes[1], ..`` consecutive components (counts that add up to K, at most 16
    sources) -> float32 [.., S, rows, T]: ``m_s`` = (the model of source s's patches)^power, ``mask_s = m_s / sum m``, ``1 / S``
    where the sum is below 2^-40.  With ``X``, a spectrum [.., rows, T] or [.., C, rows, T] (C in {1, 2}), returns ``(masks,
    mask_s X)``.  One launch."""
    power = _check_power(power)
    w, h = _nonneg(W, "W", (3, 4)), _nonneg(H, "H")
    K, T, R = h.shape[-2], h.shape[-1], w.shape[-3]
    lead = tuple(h.shape[:-2])
    dims = _check_shapes(torch.empty(lead + (R, T), device="meta"), w, h, False)
    bounds = _check_sizes(sizes, K)
    S = len(bounds) - 1
    x, had_c = (None, False) if X is None else _check_mixture(X, lead, R, T)
    C = 1 if x is None else x.shape[-3]
    if dims[0] * S * C * R * T > MAX_ELEMENTS:
        raise ValueError("masks: N * S * C * rows * T must be at most 2^31 - 1")
    dev = audio._device(*(t for t in (w, h, x) if t is not None))
    w, h = (t.to(device=dev, dtype=torch.float32).contiguous() for t in (w, h))
    if x is not None:
        x = x.to(device=dev, dtype=torch.complex64).contiguous()
    m, spec = _masks(w, h, dims, bounds, power, x, C)
    if x is None:
        return m
    return m, (spec if had_c else spec.squeeze(-3))


def _check_dictionaries(dictionaries, R=None, Tw=None):
    """S arrays [rows, K_s, Tw] with one common Tw -> (tensors, sizes, Tw)."""
    if not isinstance(dictionaries, (tuple, list)) or not 1 <= len(dictionaries) <= MAX_SOURCES:
        raise ValueError("dictionaries: expected a list of 1 to %d arrays [rows, K_s, Tw], got %r" % (MAX_SOURCES, type(dictionaries).__name__))
    ws = [_nonneg(d, "dictionaries[%d]" % i, (3,)) for i, d in enumerate(dictionaries)]
    rows = ws[0].shape[0] if R is None else R
    tw = ws[0].shape[2] if Tw is None else _check_tw(Tw)
    for i, d in enumerate(ws):
        if d.shape[0] != rows or d.shape[1] < 1 or d.shape[2] != tw:
            raise ValueError("dictionaries[%d]: expected [%d, K_s, %d] with K_s >= 1 (one Tw for all), got %s" % (i, rows, tw, tuple(d.shape)))
    sizes = [int(d.shape[1]) for d in ws]
    if not 1 <= tw <= MAX_TEMPLATE_FRAMES or sum(sizes) > MAX_COMPONENTS or sum(sizes) * tw > MAX_STACKED:
        raise ValueError("dictionaries: expected Tw <= %d and at most %d stacked components (K * Tw) in all, got %d * %d"
                         % (MAX_TEMPLATE_FRAMES, MAX_STACKED, sum(sizes), tw))
    return ws, sizes, int(tw)


def nmfd_separate(X, dictionaries, Tw=None, beta=1, n_iter=100, power=1, seed=0, return_model=False):
    """Supervised separation of a complex STFT: mono [rows, T], channels [C, rows, T] (C in {1, 2}) or a batch [N, C, rows, T] ->
    ``(masks, spectra)`` as ``nmf.nmf_separate``.  ``dictionaries``: S arrays [rows, K_s, Tw] (``learn_dictionary``) with one common
    ``Tw`` (checked against the argument when that is given), at most 128 stacked components in all.  W is their concatenation along
    the components and stays; H starts at ``init(V, K, Tw, seed)`` and gets ``n_iter`` joint updates on V = |X| (the mean magnitude of
    the two channels); the masks are ``masks(W, H, sizes, power)`` and the spectra ``mask_s X`` per channel.  ``return_model`` adds a
    dict with ``W``, ``H`` and ``V``."""
    beta, n_iter, power, seed = _check_separate_params(beta, n_iter, power, seed)
    return_model = _check_flag(return_model, "return_model")
    x = X if torch.is_tensor(X) else torch.as_tensor(np.asarray(X))
    if x.dim() not in (2, 3, 4) or (x.dim() >= 3 and x.shape[-3] not in (1, 2)):
        raise ValueError("X: expected [rows, T], [C, rows, T] or [N, C, rows, T] with C in {1, 2}, got %s" % (tuple(x.shape),))
    R, T = x.shape[-2], x.shape[-1]
    ws, sizes, tw = _check_dictionaries(dictionaries, R, Tw)
    K = sum(sizes)
    mono = x.dim() == 2
    xc = x[None] if mono else x                                                           # [.., C, R, T]
    lead = tuple(xc.shape[:-3])
    _check_shapes(torch.empty(lead + (R, T), device="meta"), torch.empty((R, K, tw), device="meta"), torch.empty(lead + (K, T), device="meta"), False)
    nsig = xc.shape[0] if xc.dim() == 4 else 1
    if nsig * len(sizes) * xc.shape[-3] * R * T > MAX_ELEMENTS:
        raise ValueError("X: N * S * C * rows * T must be at most 2^31 - 1")
    dev = audio._device(xc, *ws)
    xc = xc.to(device=dev, dtype=torch.complex64).contiguous()
    w = torch.cat([d.to(device=dev, dtype=torch.float32) for d in ws], dim=1).contiguous()
    v = xc.abs().mean(dim=-3).contiguous()                                                # [.., R, T]
    h = init(v, K, tw, seed)[1]
    dims = (nsig, R, T, K, tw, 1)
    _fit(v, w, h, dims, beta, n_iter, 0)
    bounds = np.cumsum([0] + sizes).astype(np.int32)
    m, spec = _masks(w, h, dims, bounds, power, xc, xc.shape[-3])
    if mono:
        spec = spec.squeeze(-3)
    return (m, spec, dict(W=w, H=h, V=v)) if return_model else (m, spec)


_NMFD_AUDIO_DEFAULTS = dict(Tw=None, beta=1, n_iter=100, power=1, seed=0, residual=False)


def nmfd_audio(y, dictionaries, Tw=None, beta=1, n_iter=100, power=1, seed=0, residual=False):
    """Supervised convolutive NMF separation for 16 kHz audio [n] or [C, n] (C in {1, 2}), n > 1024 -> stems [S, n] or [S, C, n]
    aligned with y; with ``residual`` also ``y - stems.sum(0)``.  The path of ``nmf.nmf_audio``: one STFT of the whole signal (1025
    rows, so the dictionaries are [1025, K_s, Tw]), ``nmfd_separate`` on it, the masked magnitudes with the mixture's phase through
    one ``audio.griffinlim(n_iter=0)``, trimmed to n samples.  At most 32 768 frames."""
    _check_separate_params(beta, n_iter, power, seed)
    _check_flag(residual, "residual")
    _check_dictionaries(dictionaries, audio.NBIN, Tw)
    t = audio._tensor(y, "y")
    x = audio._long_audio(t)
    if x.shape[0] > 2:
        raise ValueError("y: expected one or two channels, got %d" % x.shape[0])
    C, n = x.shape
    if 1 + -(-n // audio.HOP) > MAX_FRAMES:
        raise ValueError("y: expected at most %d frames (%d samples), got %d samples" % (MAX_FRAMES, (MAX_FRAMES - 2) * audio.HOP, n))
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [C, 1025, F]
    m, _ = nmfd_separate(X, dictionaries, Tw, beta, n_iter, power, seed)                  # [S, 1025, F]
    S = m.shape[0]
    mag = (m[:, None] * X.abs()[None]).reshape((S * C,) + tuple(X.shape[1:]))
    phase = torch.polar(torch.ones_like(X.real), X.angle()).repeat(S, 1, 1)
    stems = audio.griffinlim(mag, n_iter=0, init=phase)[:, :n].reshape((S,) + tuple(t.shape[:-1]) + (n,)).contiguous()
    return (stems, x.reshape(tuple(t.shape)) - stems.sum(0)) if residual else stems


def _dictionary_from_wav(path, n_components, template_frames, beta, n_iter, seed):
    y, native = audio.load_audio(path, sr=None, mono=True)
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    _, X = audio.mel_frames(y, return_stft=True)
    return learn_dictionary(X.abs()[0], n_components, template_frames, beta, n_iter, seed)


def separate_wav_nmfd(path, dictionaries, out_rate="input", mono=False, n_components=4, template_frames=8, dictionary_iter=200, **kwargs):
    """``nmfd_audio`` for a PCM wav at any rate with one or two channels -> ``(stems, rate)``, shaped and resampled as
    ``nmf.separate_wav_nmf`` does: at ``out_rate`` 'input' the file's rate and exactly its sample count.  Each entry of
    ``dictionaries`` is an array [1025, K_s, template_frames] or the path of a wav of the isolated source, from which ``n_components``
    templates of ``template_frames`` frames are learned at the same STFT geometry (mono, resampled to 16 kHz, ``dictionary_iter``
    iterations at the same beta and seed).  ``kwargs`` are ``nmfd_audio``'s keyword arguments except ``Tw`` (that is
    ``template_frames``); any other is refused before a file is opened."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    _check_flag(mono, "mono")
    unknown = set(kwargs) - (set(_NMFD_AUDIO_DEFAULTS) - {"Tw"})
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected nmfd_audio's (Tw is template_frames)" % sorted(unknown))
    p = dict(_NMFD_AUDIO_DEFAULTS, **kwargs)
    _check_separate_params(p["beta"], p["n_iter"], p["power"], p["seed"])
    _check_flag(p["residual"], "residual")
    n_components = _check_range_int(n_components, "n_components", 1, MAX_COMPONENTS)
    template_frames = _check_tw(template_frames, n_components)
    dictionary_iter = _check_range_int(dictionary_iter, "dictionary_iter", 0, MAX_ITER)
    if not isinstance(dictionaries, (tuple, list)) or not 1 <= len(dictionaries) <= MAX_SOURCES:
        raise ValueError("dictionaries: expected a list of 1 to %d arrays [1025, K_s, Tw] or wav paths" % MAX_SOURCES)
    is_path = [isinstance(d, (str, os.PathLike)) for d in dictionaries]
    _check_dictionaries([torch.empty((audio.NBIN, n_components, template_frames), device="meta") if f else d for d, f in zip(dictionaries, is_path)],
                        audio.NBIN, template_frames)
    ws = [_dictionary_from_wav(d, n_components, template_frames, p["beta"], dictionary_iter, p["seed"]) if f else d for d, f in zip(dictionaries, is_path)]
    y, native = audio.load_audio(path, sr=None, mono=False)
    if y.shape[0] > 2 and not mono:
        raise ValueError("%s: expected a file with one or two channels (or mono=True), got %d" % (path, y.shape[0]))
    n_file = y.shape[1]
    y = y.mean(0) if mono or y.shape[0] == 1 else y
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    out = nmfd_audio(y, ws, Tw=template_frames, **kwargs)
    stems = torch.cat([out[0], out[1][None]]) if p["residual"] else out
    stems = audio.resample(stems, audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate
