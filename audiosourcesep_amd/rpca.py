"""Robust principal component analysis for singing-voice separation (Huang, Chen, Smaragdis & Hasegawa-Johnson 2012; nussl's
``RPCA``): the accompaniment is the low-rank part of the magnitude spectrogram, the voice the sparse rest, found by the inexact
augmented Lagrange multiplier method (Lin et al. 2010).  The prior-free member of the family every singing-voice paper compares
against, beside ``hpss``, ``repet``, ``ft2d``, ``duet``, ``nmf``, ``iva`` and ``melody``.  Not in the reference.

Kernels in ``csrc/glowk_rpca.h`` (formulas, orders and error bounds in include/glowk.h), all fp64:

* ``gram`` / ``gemm``: products on the fp64 matrix cores: ``A A^T``, ``V diag(g) V^T`` (both exactly symmetric) and ``P A``;
* ``eigh``: a symmetric eigensolver, cyclic Jacobi in round-robin order, two launches per round; ``spectral_norm`` from it;
* ``shrink``, ``svt``: the two proximal steps; the singular value thresholding goes through the rows-side Gram matrix, no SVD;
* ``rpca_fit``: the whole loop in one C call; each signal of a batch stops on its own;
* ``masks``: the binary mask of Huang et al. or the soft pair of ``hpss``;
* ``rpca``, ``rpca_audio``, ``separate_wav_rpca``: spectra, audio and wav paths, those of ``hpss.py`` / ``ft2d.py``.

Conventions as in ``nmf.py``: numpy or torch in, tensors on the GPU the input lives on out, ValueError for bad arguments before the
library is loaded.  ``eigh`` (and what calls it) reads 4 bytes per signal on the host once per sweep, ``rpca_fit`` once per
iteration; nothing else synchronises.  Results are bitwise reproducible and a batch gives what its signals give alone.
"""
import math

import numpy as np
import torch

from . import _lib, audio
from .audio import _p, _s
from .repet import _check_flag, _check_mask_params, _check_range_int

MAX_ROWS, MAX_FRAMES, MAX_SIGNALS, MAX_ITER, MAX_SWEEPS = 2049, 65535, 65535, 100000, 30
MAX_AUDIO_FRAMES = 32768                                  # audio.mel_frames' limit
MAX_ELEMENTS = (1 << 31) - 1
GRAM, SCALED, APPLY = 0, 1, 2                             # glowk_rpca_gemm's forms
STATUS_SWEEP_CAP = 1


def _work(nbytes, dev):
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)


def _tensor(a):
    return a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))


def _planes(a, what, max_last=MAX_FRAMES, square=False):
    """A real array [.., n, k] with at most one leading dimension, within the kernels' ranges, as a tensor where it is."""
    x = _tensor(a)
    if x.is_complex() or x.dtype == torch.bool or x.dim() not in (2, 3):
        raise ValueError("%s: expected a real array with 2 or 3 dimensions, got %s %s" % (what, x.dtype, tuple(x.shape)))
    n, k = x.shape[-2], x.shape[-1]
    nsig = x.shape[0] if x.dim() == 3 else 1
    if not 1 <= n <= MAX_ROWS or not 1 <= k <= max_last or nsig > MAX_SIGNALS or nsig * n * k > MAX_ELEMENTS or nsig * n * n > MAX_ELEMENTS:
        raise ValueError("%s: expected [rows, F] or [N, rows, F] with N <= %d, 1 <= rows <= %d, 1 <= F <= %d and at most 2^31 - 1 elements "
                         "(N rows rows too), got %s" % (what, MAX_SIGNALS, MAX_ROWS, max_last, tuple(x.shape)))
    if square and n != k:
        raise ValueError("%s: expected square matrices, got %s" % (what, tuple(x.shape)))
    return x, nsig


def _f64(x, dev=None):
    return x.to(device=audio._device(x) if dev is None else dev, dtype=torch.float64).contiguous()


def _check_number(v, what, positive):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) \
            or (v <= 0 if positive else v < 0):
        raise ValueError("%s: expected a finite number %s 0, got %r" % (what, ">" if positive else ">=", v))
    return float(v)


def _gemm(form, a, b, scale, nsig, M, N, K):
    lib = _lib.load()
    c = torch.empty(tuple(a.shape[:-2]) + (M, N), dtype=torch.float64, device=a.device)
    if nsig:
        nbytes = lib.glowk_rpca_gemm_workspace_bytes(nsig, M, N, K, form)
        work = _work(nbytes, a.device)
        _lib.check(lib.glowk_rpca_gemm(_p(a), None if b is None else _p(b), None if scale is None else _p(scale), nsig, M, N, K, form, _p(c),
                                       _p(work), nbytes, _s(a)))
    return c


def gram(A):
    """``A A^T`` of A [rows, F] or [N, rows, F] -> float64 [.., rows, rows], exactly symmetric.  The fp64 matrix cores, K split in
    a fixed way (two launches above 1024 frames)."""
    x, nsig = _planes(A, "A")
    x = _f64(x)
    return _gemm(GRAM, x, None, None, nsig, x.shape[-2], x.shape[-2], x.shape[-1])


def scaled_gram(V, g):
    """``V diag(g) V^T`` of V [n, K] (or a batch) and g [K] -> float64 [.., n, n], exactly symmetric.  One launch."""
    x, nsig = _planes(V, "V")
    s = _tensor(g)
    if s.is_complex() or tuple(s.shape) != tuple(x.shape[:-2]) + (x.shape[-1],):
        raise ValueError("g: expected real %s, got %s" % (tuple(x.shape[:-2]) + (x.shape[-1],), tuple(s.shape)))
    dev = audio._device(x, s)
    x, s = _f64(x, dev), _f64(s, dev)
    return _gemm(SCALED, x, None, s, nsig, x.shape[-2], x.shape[-2], x.shape[-1])


def matmul(P, A):
    """``P A`` of P [M, K] and A [K, F] (or batches of both) -> float64 [.., M, F].  One launch."""
    p, nsig = _planes(P, "P")
    a = _tensor(A)
    if a.is_complex() or a.dim() != p.dim() or tuple(a.shape[:-1]) != tuple(p.shape[:-2]) + (p.shape[-1],) or not 1 <= a.shape[-1] <= MAX_FRAMES \
            or nsig * a.shape[-1] * max(p.shape[-1], p.shape[-2]) > MAX_ELEMENTS:
        raise ValueError("A: expected real %s with 1 <= F <= %d, got %s" % (tuple(p.shape[:-2]) + (p.shape[-1], "F"), MAX_FRAMES, tuple(a.shape)))
    dev = audio._device(p, a)
    p, a = _f64(p, dev), _f64(a, dev)
    return _gemm(APPLY, p, a, None, nsig, p.shape[-2], a.shape[-1], p.shape[-1])


def _eigh(g, nsig, n):
    """g: float64 contiguous on the GPU, overwritten -> l, V, sweeps, status in the solver's order."""
    lib = _lib.load()
    lead = tuple(g.shape[:-2])
    l = torch.empty(lead + (n,), dtype=torch.float64, device=g.device)
    v = torch.empty_like(g)
    sweeps = torch.zeros(lead, dtype=torch.int32, device=g.device)
    status = torch.zeros(lead, dtype=torch.int32, device=g.device)
    if nsig:
        nbytes = lib.glowk_rpca_eigh_workspace_bytes(nsig, n)
        work = _work(nbytes, g.device)
        _lib.check(lib.glowk_rpca_eigh(_p(g), nsig, n, _p(l), _p(v), _p(sweeps), _p(status), _p(work), nbytes, _s(g)))
    return l, v, sweeps, status


def eigh(G, return_status=False):
    """The eigendecomposition of symmetric G [n, n] or [N, n, n] (the upper triangle and the diagonal are what counts for a rotation's
    angle; G is taken as it is) -> ``(l, V, sweeps)``: eigenvalues float64 [.., n] ascending, eigenvectors in the columns of V, the
    Jacobi sweeps run (int32, at most 30; 1 for a diagonal matrix).  ``return_status`` adds the status (int32; bit 0: the cap of 30
    sweeps was reached while still rotating).  The order of equal eigenvalues is that of a stable sort of the solver's."""
    return_status = _check_flag(return_status, "return_status")
    x, nsig = _planes(G, "G", MAX_ROWS, square=True)
    g = _f64(x)
    if torch.is_tensor(G) and g.data_ptr() == G.data_ptr():
        g = g.clone()
    l, v, sweeps, status = _eigh(g, nsig, g.shape[-1])
    l, order = torch.sort(l, dim=-1, stable=True)
    v = torch.gather(v, -1, order.unsqueeze(-2).expand_as(v))
    return (l, v, sweeps, status) if return_status else (l, v, sweeps)


def spectral_norm(M):
    """``||M||_2`` of M [rows, F] or [N, rows, F] -> float64 [..]: the square root of the largest eigenvalue of ``gram(M)``."""
    x, nsig = _planes(M, "M")
    x = _f64(x)
    g = _gemm(GRAM, x, None, None, nsig, x.shape[-2], x.shape[-2], x.shape[-1])
    l = _eigh(g, nsig, x.shape[-2])[0]
    return torch.sqrt(l.max(dim=-1).values.clamp_min(0.0))


def shrink(T, thr):
    """``sign(T) max(|T| - thr, 0)`` of a real array of any shape -> float64, shaped like T.  One launch."""
    thr = _check_number(thr, "thr", False)
    t = _tensor(T)
    if t.is_complex() or t.numel() > MAX_ELEMENTS:
        raise ValueError("T: expected a real array with at most 2^31 - 1 elements, got %s %s" % (t.dtype, tuple(t.shape)))
    t = _f64(t)
    out = torch.empty_like(t)
    if t.numel():
        _lib.check(_lib.load().glowk_rpca_shrink(_p(t), t.numel(), thr, _p(out), _s(t)))
    return out


def _check_tau(tau, lead):
    t = _tensor(tau)
    if t.is_complex() or tuple(t.shape) not in ((), lead):
        raise ValueError("tau: expected a number or numbers shaped %s, got %s" % (lead, tuple(t.shape)))
    if t.device.type == "cpu" and not bool((torch.isfinite(t.to(torch.float64)) & (t >= 0)).all()):
        raise ValueError("tau: expected finite numbers >= 0")
    return t


def svt(A, tau, return_info=False):
    """Singular value thresholding ``U max(Sigma - tau, 0) V^T`` of A [rows, F] or [N, rows, F] -> float64 shaped like A, through
    ``gram(A)``, ``eigh`` and two more products (include/glowk.h).  ``tau``: a number or one per signal.  ``return_info`` adds a
    dict with the solves' ``sweeps`` and ``status``."""
    return_info = _check_flag(return_info, "return_info")
    x, nsig = _planes(A, "A")
    lead = tuple(x.shape[:-2])
    t = _check_tau(tau, lead)
    dev = audio._device(x, t)
    t = t.to(device=dev, dtype=torch.float64).expand(lead).contiguous()
    a = _f64(x, dev)
    rows, frames = a.shape[-2], a.shape[-1]
    out = torch.empty_like(a)
    sweeps = torch.zeros(lead, dtype=torch.int32, device=dev)
    status = torch.zeros(lead, dtype=torch.int32, device=dev)
    if nsig:
        lib = _lib.load()
        nbytes = lib.glowk_rpca_svt_workspace_bytes(nsig, rows, frames)
        work = _work(nbytes, dev)
        _lib.check(lib.glowk_rpca_svt(_p(a), nsig, rows, frames, _p(t), _p(out), _p(sweeps), _p(status), _p(work), nbytes, _s(a)))
    return (out, dict(sweeps=sweeps, status=status)) if return_info else out


def _check_fit_params(gain, tol, n_iter):
    return _check_number(gain, "gain", True), _check_number(tol, "tol", False), _check_range_int(n_iter, "n_iter", 0, MAX_ITER)


def rpca_fit(M, gain=1.0, tol=1e-7, n_iter=100, return_status=False):
    """Inexact ALM on M [rows, F] or [N, rows, F] (magnitudes; rounded to float32 on entry) -> ``(L, S, iterations)``: the low-rank
    and the sparse part, float64 shaped like M, and the iterations each signal ran (int32 [..]).  ``lam = gain / sqrt(max(rows,
    F))``; a signal stops when ``||M - L - S||_F / ||M||_F < tol`` or after ``n_iter`` iterations, and is frozen from then on; a silent
    signal gets zeros and 0 iterations.  ``return_status`` adds the OR of its eigensolves' status (bit 0: the sweep cap)."""
    gain, tol, n_iter = _check_fit_params(gain, tol, n_iter)
    return_status = _check_flag(return_status, "return_status")
    x, nsig = _planes(M, "M")
    m = x.to(device=audio._device(x), dtype=torch.float32).contiguous()
    rows, frames = m.shape[-2], m.shape[-1]
    lead = tuple(m.shape[:-2])
    L = torch.zeros(m.shape, dtype=torch.float64, device=m.device)
    S = torch.zeros_like(L)
    iters = torch.zeros(lead, dtype=torch.int32, device=m.device)
    status = torch.zeros(lead, dtype=torch.int32, device=m.device)
    if nsig:
        lib = _lib.load()
        nbytes = lib.glowk_rpca_workspace_bytes(nsig, rows, frames)
        work = _work(nbytes, m.device)
        _lib.check(lib.glowk_rpca_fit(_p(m), nsig, rows, frames, gain, tol, n_iter, _p(L), _p(S), _p(iters), _p(status), _p(work), nbytes, _s(m)))
    return (L, S, iters, status) if return_status else (L, S, iters)


def _check_kind(kind):
    if not isinstance(kind, str) or kind not in ("soft", "binary"):
        raise ValueError("kind: expected 'soft' or 'binary', got %r" % (kind,))
    return kind


def _binary(L, S, X, gain_mask):
    """L, S float64 contiguous on the GPU, X complex64 like them or None -> (mask_fg float32, bg, fg complex64 or None)."""
    mask = torch.empty(L.shape, dtype=torch.float32, device=L.device)
    bg = fg = None
    if X is not None:
        bg, fg = torch.empty_like(X), torch.empty_like(X)
    if L.numel():
        _lib.check(_lib.load().glowk_rpca_binary_mask(_p(L), _p(S), None if X is None else _p(X), L.numel(), gain_mask, _p(mask),
                                                      None if bg is None else _p(bg), None if fg is None else _p(fg), _s(L)))
    return mask, bg, fg


def _soft(L, S, x, power, mb, mf):
    """glowk_hpss_mask on |L| and |S| rounded to float32; with x (float32) the masked magnitudes instead of the masks."""
    a, b = L.abs().to(torch.float32).contiguous(), S.abs().to(torch.float32).contiguous()
    out_b, out_f = torch.empty_like(a), torch.empty_like(a)
    if a.numel():
        _lib.check(_lib.load().glowk_hpss_mask(_p(a), _p(b), None if x is None else _p(x), a.numel(), power, mb, mf, _p(out_b), _p(out_f), _s(a)))
    return out_b, out_f


def masks(L, S, kind="soft", gain_mask=1.0, power=2.0, margin=1.0):
    """``(background, foreground)`` masks, float32 shaped like L, from the two parts.  ``kind='binary'``: the mask of Huang et al.,
    foreground 1 where ``|S| > gain_mask |L|`` (fp64), background its complement.  ``kind='soft'``: ``hpss``'s soft masks
    (``glowk_hpss_mask``) of ``|L|`` against ``|S|`` rounded to float32, with ``hpss``'s ``power`` and ``margin``.  One launch."""
    kind = _check_kind(kind)
    gain_mask = _check_number(gain_mask, "gain_mask", False)
    power, (mb, mf) = _check_mask_params(power, margin)
    l, _ = _planes(L, "L")
    s = _tensor(S)
    if s.is_complex() or tuple(s.shape) != tuple(l.shape):
        raise ValueError("S: expected a real array shaped %s, got %s" % (tuple(l.shape), tuple(s.shape)))
    dev = audio._device(l, s)
    l, s = _f64(l, dev), _f64(s, dev)
    if kind == "binary":
        fg = _binary(l, s, None, gain_mask)[0]
        return 1.0 - fg, fg
    return _soft(l, s, None, power, mb, mf)


def rpca(S, gain=1.0, tol=1e-7, n_iter=100, kind="soft", gain_mask=1.0, power=2.0, margin=1.0, mask=False, return_model=False):
    """RPCA separation of spectra [rows, F] or [N, rows, F] -> ``(background, foreground)`` shaped like S: ``rpca_fit`` on |S|, then
    ``masks`` times S.  Complex S keeps its phase (complex64 out), real S gives float32 magnitudes; ``mask=True`` returns the two
    masks instead.  ``return_model`` adds a dict with ``L``, ``S``, ``iterations`` and ``status``."""
    gain, tol, n_iter = _check_fit_params(gain, tol, n_iter)
    kind = _check_kind(kind)
    gain_mask = _check_number(gain_mask, "gain_mask", False)
    power, (mb, mf) = _check_mask_params(power, margin)
    mask, return_model = _check_flag(mask, "mask"), _check_flag(return_model, "return_model")
    x = _tensor(S)
    if x.dtype == torch.bool or x.dim() not in (2, 3):
        raise ValueError("S: expected spectra [rows, F] or [N, rows, F], got %s %s" % (x.dtype, tuple(x.shape)))
    _planes(x.real if x.is_complex() else x, "S")
    dev = audio._device(x)
    X = None
    if x.is_complex():
        X = x.to(device=dev, dtype=torch.complex64).contiguous()
        x = X.abs()
    x = x.to(device=dev, dtype=torch.float32).contiguous()
    L, Sp, iters, status = rpca_fit(x, gain, tol, n_iter, return_status=True)
    if kind == "binary":
        fg, b, f = _binary(L, Sp, None if mask else X, gain_mask)
        if mask:
            b, f = 1.0 - fg, fg
        elif X is None:
            b, f = (1.0 - fg) * x, fg * x
    else:
        b, f = _soft(L, Sp, None if mask else x, power, mb, mf)
        if X is not None and not mask:
            phase = torch.polar(torch.ones_like(X.real), X.angle())
            b, f = b * phase, f * phase
    return (b, f, dict(L=L, S=Sp, iterations=iters, status=status)) if return_model else (b, f)


_RPCA_AUDIO_DEFAULTS = dict(gain=1.0, tol=1e-7, n_iter=100, kind="soft", gain_mask=1.0, power=2.0, margin=1.0, residual=False)


def _check_audio_params(gain, tol, n_iter, kind, gain_mask, power, margin, residual):
    _check_fit_params(gain, tol, n_iter)
    _check_kind(kind)
    _check_number(gain_mask, "gain_mask", False)
    _check_mask_params(power, margin)
    _check_flag(residual, "residual")


def rpca_audio(y, gain=1.0, tol=1e-7, n_iter=100, kind="soft", gain_mask=1.0, power=2.0, margin=1.0, residual=False):
    """RPCA separation for 16 kHz audio [n] or [C, n], n > 1024 -> ``(background, foreground)``, each shaped like y and aligned with
    it; with ``residual`` also ``y - background - foreground``.  The path of ``hpss.hpss_audio``: one STFT of the whole signal
    (1025 rows), ``rpca`` on |X| per channel, the masked magnitudes with the mixture's phase through one
    ``audio.griffinlim(n_iter=0)``, trimmed to n samples.  At most 32 768 frames."""
    _check_audio_params(gain, tol, n_iter, kind, gain_mask, power, margin, residual)
    t = audio._tensor(y, "y")
    x = audio._long_audio(t)
    if x.shape[0] > MAX_SIGNALS:
        raise ValueError("y: expected at most %d channels, got %d" % (MAX_SIGNALS, x.shape[0]))
    lead, n = tuple(t.shape[:-1]), x.shape[1]
    if 1 + -(-n // audio.HOP) > MAX_AUDIO_FRAMES:
        raise ValueError("y: expected at most %d frames (%d samples), got %d samples" % (MAX_AUDIO_FRAMES, (MAX_AUDIO_FRAMES - 2) * audio.HOP, n))
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [C, 1025, F]
    b, f = rpca(X.abs(), gain, tol, n_iter, kind, gain_mask, power, margin)
    phase = torch.polar(torch.ones_like(X.real), X.angle())
    stems = audio.griffinlim(torch.cat([b, f]), n_iter=0, init=torch.cat([phase, phase]))[:, :n].reshape((2,) + lead + (n,))
    b, f = stems[0].contiguous(), stems[1].contiguous()
    return (b, f, x.reshape(lead + (n,)) - b - f) if residual else (b, f)


def separate_wav_rpca(path, out_rate="input", mono=False, **kwargs):
    """``rpca_audio`` for a PCM wav at any rate (a path, or what ``audio.load_audio`` takes) -> ``(stems, rate)``: stems [2, n']
    (background, foreground; [3, n'] with ``residual=True``) of a one-channel file or with ``mono``, else [2 or 3, C, n'], at
    ``out_rate``: 'input' (the file's rate and exactly its sample count), an integer rate, or None (16 kHz).  ``kwargs`` are
    ``rpca_audio``'s keyword arguments; any other is refused before the file is opened."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    _check_flag(mono, "mono")
    unknown = set(kwargs) - set(_RPCA_AUDIO_DEFAULTS)
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected rpca_audio's" % sorted(unknown))
    _check_audio_params(**dict(_RPCA_AUDIO_DEFAULTS, **kwargs))
    y, native = audio.load_audio(path, sr=None, mono=False)
    n_file = y.shape[1]
    y = y.mean(0) if mono or y.shape[0] == 1 else y
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    stems = audio.resample(torch.stack(rpca_audio(y, **kwargs)), audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate
