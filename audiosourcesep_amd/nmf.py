"""Non-negative matrix factorisation (Lee & Seung 2001; the beta divergences and the majorise-minimise exponent of Fevotte & Idier
2011, as in ``sklearn.decomposition.NMF(solver='mu')``) and supervised separation with it: a small dictionary of spectra per
instrument, learned from a few seconds of isolated material; the mixture's spectrogram explained with the concatenated dictionaries;
ratio masks of each dictionary's share.  The classic supervised baseline between the fixed rules (``hpss``, ``repet``, ``ft2d``,
``duet``) and the trained priors of BASIS.  Not in the reference.

Kernels in ``csrc/glowk_nmf.h`` (formulas and error bounds in include/glowk.h):

* ``update_h`` / ``update_w`` / ``fit``: multiplicative updates for beta = 0 (Itakura-Saito), 1 (Kullback-Leibler), 2 (Euclidean).
  One update is two chained GEMMs on the fp32 matrix cores with the elementwise step between them in registers; ``W H`` is never
  stored.  One iteration is the W update (with the old H), then the H update (with the new W);
* ``divergence``: ``D_beta(V | W H)`` in fp64, fixed order;
* ``masks``: the sources own contiguous ranges of components, ``mask_s = (W_s H_s)^power / sum``; with ``X`` also ``mask_s X``;
* ``init``: the starting point from the device RNG (``glowk_random``), reproducible bit for bit;
* ``decompose`` (the surface of ``librosa.decompose.decompose``), ``learn_dictionary``, ``nmf_separate``, ``nmf_audio``,
  ``separate_wav_nmf``: spectra, audio and wav paths, those of ``duet.py`` / ``ft2d.py``.

Conventions as in ``repet.py``: numpy or torch in, tensors on the GPU the input lives on out, ValueError for bad arguments before
the library is loaded, no host synchronisation.  Results are bitwise reproducible and a batch gives what its signals give alone.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, audio
from .audio import _p, _s
from .repet import MAX_ELEMENTS, MAX_FRAMES, MAX_ROWS, MAX_SIGNALS, _check_flag, _check_range_int

MAX_COMPONENTS, MAX_SOURCES, MAX_ITER = 128, 16, 100000
NMF_STREAM = 12             # device RNG stream of ``init`` (0-3 serve the flows, 11 nmfd, 13 griffinlim, 14 / 15 separate_audio)


def _check_beta(beta):
    if isinstance(beta, (bool, np.bool_)) or not isinstance(beta, (int, np.integer)) or beta not in (0, 1, 2):
        raise ValueError("beta: expected 0 (Itakura-Saito), 1 (Kullback-Leibler) or 2 (Euclidean), got %r" % (beta,))
    return int(beta)


def _check_power(power):
    if isinstance(power, (bool, np.bool_)) or not isinstance(power, (int, np.integer)) or power not in (1, 2):
        raise ValueError("power: expected 1 or 2, got %r" % (power,))
    return int(power)


def _check_seed(seed):
    return _check_range_int(seed, "seed", 0, (1 << 64) - 1)


def _nonneg(a, what, lead_dims=(2, 3)):
    """A real array, finite and >= 0 where that can be seen without a device read (host inputs), as a tensor where it is."""
    x = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    if x.is_complex() or x.dtype == torch.bool or x.dim() not in lead_dims:
        raise ValueError("%s: expected a real array with %s dimensions, got %s %s" % (what, " or ".join(str(d) for d in lead_dims), x.dtype,
                                                                                      tuple(x.shape)))
    if x.device.type == "cpu" and x.numel():
        xf = x.to(torch.float32)
        if not bool(torch.isfinite(xf).all()) or bool((xf < 0).any()):
            raise ValueError("%s: expected finite, non-negative entries" % what)
    return x


def _check_shapes(v, w, h, update_w):
    """V [.., R, T], W [.., R, K] (or one [R, K] for a batch when it is not updated), H [.., K, T] -> (nsig, R, T, K, nw)."""
    R, T = v.shape[-2], v.shape[-1]
    if not 1 <= R <= MAX_ROWS or not 1 <= T <= MAX_FRAMES or (v.dim() == 3 and v.shape[0] > MAX_SIGNALS) or v.numel() > MAX_ELEMENTS:
        raise ValueError("V: expected [rows, T] or [N, rows, T] with N <= %d, 1 <= rows <= %d, 1 <= T <= %d and at most 2^31 - 1 elements, "
                         "got %s" % (MAX_SIGNALS, MAX_ROWS, MAX_FRAMES, tuple(v.shape)))
    lead = tuple(v.shape[:-2])
    K = w.shape[-1]
    if not 1 <= K <= MAX_COMPONENTS:
        raise ValueError("W: expected at most %d components, got %d" % (MAX_COMPONENTS, K))
    if w.shape[-2] != R or tuple(w.shape[:-2]) not in (lead, ()):
        raise ValueError("W: expected %s + (%d, K) for V %s, got %s" % (lead, R, tuple(v.shape), tuple(w.shape)))
    nsig = v.shape[0] if v.dim() == 3 else 1
    shared = v.dim() == 3 and w.dim() == 2
    if shared and update_w:
        raise ValueError("W: one dictionary shared by a batch cannot be updated (update_w needs W %s + (%d, K))" % (lead, R))
    if tuple(h.shape) != lead + (K, T):
        raise ValueError("H: expected %s, got %s" % (lead + (K, T), tuple(h.shape)))
    if nsig * K * T > MAX_ELEMENTS or nsig * R * K > MAX_ELEMENTS:
        raise ValueError("W, H: at most 2^31 - 1 elements each")
    return nsig, R, T, K, (1 if shared else nsig)


def _prepare(V, W, H, update_w):
    v, w, h = _nonneg(V, "V"), _nonneg(W, "W"), _nonneg(H, "H")
    dims = _check_shapes(v, w, h, update_w)
    dev = audio._device(v, w, h)
    return tuple(t.to(device=dev, dtype=torch.float32).contiguous() for t in (v, w, h)) + (dims,)


def _work(nbytes, dev):
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)


def _fit(v, w, h, dims, beta, n_iter, mode):
    """In place on w and h (float32 contiguous on v's GPU).  mode: glowk_nmf_fit's update_w."""
    nsig, R, T, K, nw = dims
    if nsig == 0 or n_iter == 0:
        return
    lib = _lib.load()
    nbytes = lib.glowk_nmf_workspace_bytes(nsig, R, T, K) if mode else 0
    work = _work(nbytes, v.device)
    _lib.check(lib.glowk_nmf_fit(_p(v), nsig, R, T, _p(w), nw, _p(h), K, beta, n_iter, mode, _p(work), nbytes, _s(v)))


def _own(t, src):
    """A tensor the kernels may overwrite: t itself if the conversion already copied, else a clone."""
    return t.clone() if torch.is_tensor(src) and t.data_ptr() == src.data_ptr() else t


def _scale(v, K):
    """sqrt(mean(V) / K) per signal: the mean in float64, rounded to float32 once."""
    return torch.sqrt(v.to(torch.float64).mean(dim=(-2, -1), keepdim=True) / K).to(torch.float32)


def init(V, K, seed=0):
    """The starting point ``(W0, H0)`` for V [rows, T] or [N, rows, T]: uniforms of the device RNG (stream 12, step 0 for W and 1
    for H, element order that of the arrays), which lie in [2^-25, 1 - 2^-24] and are never zero, times ``sqrt(mean(V) / K)`` per
    signal (the mean in float64, rounded to float32; scikit-learn's scale for its random start)."""
    K = _check_range_int(K, "K", 1, MAX_COMPONENTS)
    seed = _check_seed(seed)
    v = _nonneg(V, "V")
    R, T = v.shape[-2], v.shape[-1]
    lead = tuple(v.shape[:-2])
    _check_shapes(v, torch.empty(lead + (R, K), device="meta"), torch.empty(lead + (K, T), device="meta"), False)
    v = v.to(device=audio._device(v), dtype=torch.float32)
    lib = _lib.load()
    w = torch.empty(lead + (R, K), dtype=torch.float32, device=v.device)
    h = torch.empty(lead + (K, T), dtype=torch.float32, device=v.device)
    for t, step in ((w, 0), (h, 1)):
        if t.numel():
            _lib.check(lib.glowk_random(_p(t), t.numel(), seed, step, NMF_STREAM, 1, 0, _s(t)))
    scale = _scale(v, K) if v.numel() else v.new_zeros(lead + (1, 1))
    return w * scale, h * scale


def fit(V, W, H, beta=1, n_iter=1, update_w=True):
    """``n_iter`` iterations from (W, H) -> ``(W', H')``, new float32 tensors; the inputs stay.  V [rows, T] or [N, rows, T] >= 0,
    W [.., rows, K], H [.., K, T].  With ``update_w=False`` W stays (and is returned as it is on the GPU) and a batch may share one
    W [rows, K].  ``3 n_iter`` launches (``n_iter`` without the W update)."""
    beta = _check_beta(beta)
    n_iter = _check_range_int(n_iter, "n_iter", 0, MAX_ITER)
    update_w = _check_flag(update_w, "update_w")
    v, w, h, dims = _prepare(V, W, H, update_w)
    w, h = (_own(w, W) if update_w else w), _own(h, H)
    _fit(v, w, h, dims, beta, n_iter, 1 if update_w else 0)
    return w, h


def update_h(V, W, H, beta=1):
    """One H update: ``H' = H g(W^T Q / max(W^T P, FLOOR))`` -> H', a new tensor."""
    beta = _check_beta(beta)
    v, w, h, dims = _prepare(V, W, H, False)
    h = _own(h, H)
    _fit(v, w, h, dims, beta, 1, 0)
    return h


def update_w(V, W, H, beta=1):
    """One W update: ``W' = W g(Q H^T / max(P H^T, FLOOR))`` -> W', a new tensor."""
    beta = _check_beta(beta)
    v, w, h, dims = _prepare(V, W, H, True)
    w = _own(w, W)
    _fit(v, w, h, dims, beta, 1, 2)
    return w


def divergence(V, W, H, beta=1):
    """``D_beta(V | W H)`` -> float64, one value per signal ([N], or a scalar tensor for one signal)."""
    beta = _check_beta(beta)
    v, w, h, dims = _prepare(V, W, H, False)
    nsig, R, T, K, nw = dims
    out = torch.zeros(tuple(v.shape[:-2]), dtype=torch.float64, device=v.device)
    if nsig:
        lib = _lib.load()
        nbytes = lib.glowk_nmf_workspace_bytes(nsig, R, T, K)
        work = _work(nbytes, v.device)
        _lib.check(lib.glowk_nmf_divergence(_p(v), nsig, R, T, _p(w), nw, _p(h), K, beta, _p(out), _p(work), nbytes, _s(v)))
    return out


def decompose(S, n_components, beta=1, n_iter=200, seed=0):
    """``librosa.decompose.decompose``: S [rows, T] (or a batch [N, rows, T]) >= 0 -> ``(components [.., rows, K], activations
    [.., K, T])`` after ``n_iter`` iterations from ``init(S, K, seed)``."""
    beta = _check_beta(beta)
    n_iter = _check_range_int(n_iter, "n_iter", 0, MAX_ITER)
    w, h = init(S, n_components, seed)
    return fit(S, w, h, beta, n_iter, True)


def learn_dictionary(S, K, beta=1, n_iter=200, seed=0):
    """The dictionary W [.., rows, K] of ``decompose(S, K, ..)``: what an instrument's isolated material is made of."""
    return decompose(S, K, beta, n_iter, seed)[0]


def _check_sizes(sizes, K):
    if not isinstance(sizes, (tuple, list)) or not 1 <= len(sizes) <= MAX_SOURCES:
        raise ValueError("sizes: expected 1 to %d component counts, got %r" % (MAX_SOURCES, sizes))
    for n in sizes:
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError("sizes: expected positive integers, got %r" % (sizes,))
    if sum(int(n) for n in sizes) != K:
        raise ValueError("sizes: expected counts that add up to K = %d, got %r" % (K, tuple(sizes)))
    return np.cumsum([0] + [int(n) for n in sizes]).astype(np.int32)


def _masks(w, h, dims, bounds, power, x, C):
    nsig, R, T, K, nw = dims
    S = len(bounds) - 1
    lead = tuple(h.shape[:-2])
    m = torch.empty(lead + (S, R, T), dtype=torch.float32, device=h.device)
    spec = None if x is None else torch.empty(lead + (S, C, R, T), dtype=torch.complex64, device=h.device)
    if nsig:
        _lib.check(_lib.load().glowk_nmf_masks(_p(w), nw, _p(h), nsig, R, T, K, bounds.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), S, power,
                                               _p(x), C, _p(m), _p(spec), _s(h)))
    return m, spec


def _check_mixture(X, lead, R, T):
    """X complex (or real) [.., R, T] or [.., C, R, T] with C in {1, 2} for H's leading shape -> (tensor [.., C, R, T], had C)."""
    x = X if torch.is_tensor(X) else torch.as_tensor(np.asarray(X))
    n = len(lead)
    if x.dim() == n + 2 and tuple(x.shape) == lead + (R, T):
        return x.unsqueeze(n), False
    if x.dim() == n + 3 and tuple(x.shape[:n]) == lead and tuple(x.shape[n + 1:]) == (R, T) and x.shape[n] in (1, 2):
        return x, True
    raise ValueError("X: expected %s or %s with C in {1, 2}, got %s" % (lead + (R, T), lead + ("C", R, T), tuple(x.shape)))


def masks(W, H, sizes, power=1, X=None):
    """Ratio masks of the sources that own ``sizes[0], sizes[1], ..`` consecutive components (any sizes that add up to K, at most
    16 sources) -> float32 [.., S, rows, T]: ``m_s = (W_s H_s)^power``, ``mask_s = m_s / sum m``, ``1 / S`` where the sum is below
    2^-40.  With ``X``, a spectrum [.., rows, T] or [.., C, rows, T] (C in {1, 2}), returns ``(masks, mask_s X)``, the spectra
    complex64 [.., S, rows, T] or [.., S, C, rows, T].  One launch."""
    power = _check_power(power)
    w, h = _nonneg(W, "W"), _nonneg(H, "H")
    K, T, R = h.shape[-2], h.shape[-1], w.shape[-2]
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


def _check_dictionaries(dictionaries, R=None):
    if not isinstance(dictionaries, (tuple, list)) or not 1 <= len(dictionaries) <= MAX_SOURCES:
        raise ValueError("dictionaries: expected a list of 1 to %d arrays [rows, K_s], got %r" % (MAX_SOURCES, type(dictionaries).__name__))
    ws = [_nonneg(d, "dictionaries[%d]" % i, (2,)) for i, d in enumerate(dictionaries)]
    rows = ws[0].shape[0] if R is None else R
    for i, d in enumerate(ws):
        if d.shape[0] != rows or d.shape[1] < 1:
            raise ValueError("dictionaries[%d]: expected [%d, K_s] with K_s >= 1, got %s" % (i, rows, tuple(d.shape)))
    sizes = [int(d.shape[1]) for d in ws]
    if sum(sizes) > MAX_COMPONENTS:
        raise ValueError("dictionaries: expected at most %d components in all, got %d" % (MAX_COMPONENTS, sum(sizes)))
    return ws, sizes


def _check_separate_params(beta, n_iter, power, seed):
    return _check_beta(beta), _check_range_int(n_iter, "n_iter", 0, MAX_ITER), _check_power(power), _check_seed(seed)


def nmf_separate(X, dictionaries, beta=1, n_iter=100, power=1, seed=0, return_model=False):
    """Supervised separation of a complex STFT: mono [rows, T], channels [C, rows, T] (C in {1, 2}) or a batch [N, C, rows, T] ->
    ``(masks, spectra)``: float32 [.., S, rows, T] and complex64 shaped like X with S before its last two (three, with channels)
    dimensions.  ``dictionaries``: S arrays [rows, K_s] (``learn_dictionary``), at most 128 components in all.  W is their
    concatenation and stays; H starts at ``init(V, K, seed)`` and gets ``n_iter`` updates on V = |X| (the mean magnitude of the two
    channels); the masks are ``masks(W, H, sizes, power)`` and the spectra ``mask_s X`` per channel.  ``return_model`` adds a dict
    with ``W``, ``H`` and ``V``."""
    beta, n_iter, power, seed = _check_separate_params(beta, n_iter, power, seed)
    return_model = _check_flag(return_model, "return_model")
    x = X if torch.is_tensor(X) else torch.as_tensor(np.asarray(X))
    if x.dim() not in (2, 3, 4) or (x.dim() >= 3 and x.shape[-3] not in (1, 2)):
        raise ValueError("X: expected [rows, T], [C, rows, T] or [N, C, rows, T] with C in {1, 2}, got %s" % (tuple(x.shape),))
    R, T = x.shape[-2], x.shape[-1]
    ws, sizes = _check_dictionaries(dictionaries, R)
    K = sum(sizes)
    mono = x.dim() == 2
    xc = x[None] if mono else x                                                           # [.., C, R, T]
    lead = tuple(xc.shape[:-3])
    _check_shapes(torch.empty(lead + (R, T), device="meta"), torch.empty((R, K), device="meta"), torch.empty(lead + (K, T), device="meta"), False)
    nsig = xc.shape[0] if xc.dim() == 4 else 1
    if nsig * len(sizes) * xc.shape[-3] * R * T > MAX_ELEMENTS:
        raise ValueError("X: N * S * C * rows * T must be at most 2^31 - 1")
    dev = audio._device(xc, *ws)
    xc = xc.to(device=dev, dtype=torch.complex64).contiguous()
    w = torch.cat([d.to(device=dev, dtype=torch.float32) for d in ws], dim=1).contiguous()
    v = xc.abs().mean(dim=-3).contiguous()                                                # [.., R, T]
    h = init(v, K, seed)[1]
    dims = (nsig, R, T, K, 1)
    _fit(v, w, h, dims, beta, n_iter, 0)
    bounds = np.cumsum([0] + sizes).astype(np.int32)
    m, spec = _masks(w, h, dims, bounds, power, xc, xc.shape[-3])
    if mono:
        spec = spec.squeeze(-3)
    return (m, spec, dict(W=w, H=h, V=v)) if return_model else (m, spec)


_NMF_AUDIO_DEFAULTS = dict(beta=1, n_iter=100, power=1, seed=0, residual=False)


def nmf_audio(y, dictionaries, beta=1, n_iter=100, power=1, seed=0, residual=False):
    """Supervised NMF separation for 16 kHz audio [n] or [C, n] (C in {1, 2}), n > 1024 -> stems [S, n] or [S, C, n] aligned with
    y; with ``residual`` also ``y - stems.sum(0)``.  The path of ``duet.duet_audio``: one STFT of the whole signal (1025 rows, so the
    dictionaries are [1025, K_s]), ``nmf_separate`` on it, the masked magnitudes with the mixture's phase through one
    ``audio.griffinlim(n_iter=0)``, trimmed to n samples.  At most 32 768 frames."""
    _check_separate_params(beta, n_iter, power, seed)
    _check_flag(residual, "residual")
    _check_dictionaries(dictionaries, audio.NBIN)
    t = audio._tensor(y, "y")
    x = audio._long_audio(t)
    if x.shape[0] > 2:
        raise ValueError("y: expected one or two channels, got %d" % x.shape[0])
    C, n = x.shape
    if 1 + -(-n // audio.HOP) > MAX_FRAMES:
        raise ValueError("y: expected at most %d frames (%d samples), got %d samples" % (MAX_FRAMES, (MAX_FRAMES - 2) * audio.HOP, n))
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [C, 1025, F]
    m, _ = nmf_separate(X, dictionaries, beta, n_iter, power, seed)                       # [S, 1025, F]
    S = m.shape[0]
    mag = (m[:, None] * X.abs()[None]).reshape((S * C,) + tuple(X.shape[1:]))
    phase = torch.polar(torch.ones_like(X.real), X.angle()).repeat(S, 1, 1)
    stems = audio.griffinlim(mag, n_iter=0, init=phase)[:, :n].reshape((S,) + tuple(t.shape[:-1]) + (n,)).contiguous()
    return (stems, x.reshape(tuple(t.shape)) - stems.sum(0)) if residual else stems


def _dictionary_from_wav(path, n_components, beta, n_iter, seed):
    y, native = audio.load_audio(path, sr=None, mono=True)
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    _, X = audio.mel_frames(y, return_stft=True)
    return learn_dictionary(X.abs()[0], n_components, beta, n_iter, seed)


def separate_wav_nmf(path, dictionaries, out_rate="input", mono=False, n_components=16, dictionary_iter=200, **kwargs):
    """``nmf_audio`` for a PCM wav at any rate with one or two channels -> ``(stems, rate)``: stems [S, n'] of a one-channel file or
    with ``mono``, else [S, C, n'] ([S + 1, ..] with ``residual=True``, the residual last), at ``out_rate``: 'input' (the file's rate
    and exactly its sample count), an integer rate, or None (16 kHz).  Each entry of ``dictionaries`` is an array [1025, K_s] or the
    path of a wav of the isolated source, from which ``n_components`` atoms are learned at the same STFT geometry (mono, resampled
    to 16 kHz, ``dictionary_iter`` iterations at the same beta and seed).  ``kwargs`` are ``nmf_audio``'s keyword arguments; any
    other is refused before a file is opened."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    _check_flag(mono, "mono")
    unknown = set(kwargs) - set(_NMF_AUDIO_DEFAULTS)
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected nmf_audio's" % sorted(unknown))
    p = dict(_NMF_AUDIO_DEFAULTS, **kwargs)
    _check_separate_params(p["beta"], p["n_iter"], p["power"], p["seed"])
    _check_flag(p["residual"], "residual")
    n_components = _check_range_int(n_components, "n_components", 1, MAX_COMPONENTS)
    dictionary_iter = _check_range_int(dictionary_iter, "dictionary_iter", 0, MAX_ITER)
    if not isinstance(dictionaries, (tuple, list)) or not 1 <= len(dictionaries) <= MAX_SOURCES:
        raise ValueError("dictionaries: expected a list of 1 to %d arrays [1025, K_s] or wav paths" % MAX_SOURCES)
    is_path = [isinstance(d, (str, os.PathLike)) for d in dictionaries]
    _check_dictionaries([torch.empty((audio.NBIN, n_components), device="meta") if f else d for d, f in zip(dictionaries, is_path)], audio.NBIN)
    ws = [_dictionary_from_wav(d, n_components, p["beta"], dictionary_iter, p["seed"]) if f else d for d, f in zip(dictionaries, is_path)]
    y, native = audio.load_audio(path, sr=None, mono=False)
    if y.shape[0] > 2 and not mono:
        raise ValueError("%s: expected a file with one or two channels (or mono=True), got %d" % (path, y.shape[0]))
    n_file = y.shape[1]
    y = y.mean(0) if mono or y.shape[0] == 1 else y
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    out = nmf_audio(y, ws, **kwargs)
    stems = torch.cat([out[0], out[1][None]]) if p["residual"] else out
    stems = audio.resample(stems, audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate
