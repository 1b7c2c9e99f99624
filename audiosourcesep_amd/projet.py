"""PROJET (Fitzgerald, Liutkus & Badeau, "PROJET -- spatial audio separation using projections", ICASSP 2016; ``Projet`` in nussl):
blind separation of a stereo mixture into any number of amplitude-panned sources, by soft filtering.  The two channels are
projected on M directions ``phi_m``; a source panned at ``theta`` vanishes from the projection orthogonal to it, so the magnitude of
projection m is modelled as ``sigma_m = sum_j P_j(f, t) (K Q)[m][j]`` with ``K[m][l] = |sin(theta_l - phi_m)|^alpha`` the gain of pan
position l seen through projection m, ``Q[l][j]`` the pan profile of source j and ``P_j`` its free time-frequency power.  P and Q are
fitted by multiplicative updates of the beta-divergence between ``V_m = |c_m|^alpha`` and ``sigma_m``; the stems are a Wiener-like
filter on every projection, brought back to two channels by the pseudo-inverse of the projections, and they add up to the mixture.
No priors, no training.  Not in the reference.

Kernels in ``csrc/glowk_projet.h`` (formulas in include/glowk.h, design in DESIGN 26):

* ``tables``: the projection and pan grids and ``U``, ``K``, ``Up`` in fp64 numpy -- the library takes tables, not formulas;
* ``projections``: ``V`` [.., M, R, T], a diagnostic (the fit never stores it);
* ``init``: the deterministic start -- every source the mixture's power over J, source j a triangular pan profile on the j-th sector,
  so that the sources come out in ascending pan order (random starts collapsed two sources onto one pan too often);
* ``gains``, ``update_p``, ``update_q``: the stages of an iteration; ``fit``: n iterations, one fused pass over X and P plus the Q
  kernel each, the outer sums ``R^T P'`` on the fp64 matrix cores;
* ``divergence``, ``separate``, ``pan_estimates``;
* ``projet`` / ``projet_audio`` / ``separate_wav_projet``: the spectra, audio and wav paths.

Conventions as in ``duet.py``: numpy or torch in, tensors on the GPU the input lives on out, ValueError for bad arguments before the
library is loaded, no host synchronisation.
"""
import math

import numpy as np
import torch

from . import _lib, audio
from .audio import _p, _s
from .duet import _check_stereo, _dims, _number, _stereo, _work
from .repet import MAX_FRAMES, _check_flag, _check_range_int

MIN_PROJECTIONS, MAX_PROJECTIONS, MAX_PANS, MAX_SOURCES, MAX_ITER = 2, 32, 128, 8, 100000
MAX_ELEMENTS = (1 << 31) - 1
FLOOR = 2.0 ** -40


def _check_alpha(alpha):
    a = _number(alpha, "alpha")
    if not 1.0 <= a <= 2.0:
        raise ValueError("alpha: expected a number in [1, 2], got %r" % (alpha,))
    return a


def _check_beta(beta):
    if isinstance(beta, (bool, np.bool_)) or not isinstance(beta, (int, np.integer)) or int(beta) not in (0, 1, 2):
        raise ValueError("beta: expected 0, 1 or 2, got %r" % (beta,))
    return int(beta)


def pan_angles(num_pans):
    """theta_l = l pi / (2 (L - 1)), and pi / 4 for L == 1."""
    L = _check_range_int(num_pans, "num_pans", 1, MAX_PANS)
    return np.full(1, math.pi / 4) if L == 1 else np.arange(L, dtype=np.float64) * math.pi / (2 * (L - 1))


def tables(num_projections=15, num_pans=41, alpha=1.0):
    """``dict(U, K, Up, phi, theta, alpha)`` in fp64 numpy: ``phi_m = m pi / (2 (M - 1))``, ``theta_l = l pi / (2 (L - 1))`` (pi / 4 for
    L == 1), ``U [M, 2] = (-sin phi_m, cos phi_m)``, ``K [M, L] = |sin(theta_l - phi_m)|^alpha``, ``Up [2, M] = (U^T U)^-1 U^T``."""
    M = _check_range_int(num_projections, "num_projections", MIN_PROJECTIONS, MAX_PROJECTIONS)
    theta = pan_angles(num_pans)
    alpha = _check_alpha(alpha)
    phi = np.arange(M, dtype=np.float64) * math.pi / (2 * (M - 1))
    U = np.stack([-np.sin(phi), np.cos(phi)], axis=1)
    K = np.abs(np.sin(theta[None, :] - phi[:, None])) ** alpha
    return dict(U=U, K=K, Up=_pinv(U), phi=phi, theta=theta, alpha=alpha)


def _pinv(U):
    """(U^T U)^-1 U^T by the closed 2 x 2 inverse; a U^T U that is not invertible in fp64 is refused."""
    A = U.T @ U
    det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    scale = abs(A[0, 0] * A[1, 1]) + abs(A[0, 1] * A[1, 0])
    if not (np.isfinite(det) and np.isfinite(scale) and abs(det) > 2.0 ** -40 * scale and scale > 0):
        raise ValueError("U: U^T U is not invertible in fp64 (the projections span one direction only)")
    inv = np.array([[A[1, 1], -A[0, 1]], [-A[1, 0], A[0, 0]]]) / det
    return inv @ U.T


def _check_tables(tab):
    """-> (U, K, Up, theta, alpha) as fp64 numpy, checked against the kernels' ranges."""
    if not isinstance(tab, dict) or not {"U", "K", "alpha"} <= set(tab):
        raise ValueError("tables: expected the dict of projet.tables (U, K, Up, theta, alpha), got %r" % (type(tab),))
    U, K = np.asarray(tab["U"], dtype=np.float64), np.asarray(tab["K"], dtype=np.float64)
    alpha = _check_alpha(tab["alpha"])
    if U.ndim != 2 or U.shape[1] != 2 or not MIN_PROJECTIONS <= U.shape[0] <= MAX_PROJECTIONS or not np.isfinite(U).all():
        raise ValueError("tables: U: expected finite [M, 2] with %d <= M <= %d, got %s" % (MIN_PROJECTIONS, MAX_PROJECTIONS, U.shape))
    if K.ndim != 2 or K.shape[0] != U.shape[0] or not 1 <= K.shape[1] <= MAX_PANS or not np.isfinite(K).all() or (K < 0).any():
        raise ValueError("tables: K: expected finite non-negative [M, L] with M = %d and 1 <= L <= %d, got %s" % (U.shape[0], MAX_PANS, K.shape))
    Up = _pinv(U) if tab.get("Up") is None else np.asarray(tab["Up"], dtype=np.float64)
    if tab.get("Up") is not None:
        _pinv(U)
    if Up.shape != (2, U.shape[0]) or not np.isfinite(Up).all():
        raise ValueError("tables: Up: expected finite [2, M], got %s" % (Up.shape,))
    theta = pan_angles(K.shape[1]) if tab.get("theta") is None else np.asarray(tab["theta"], dtype=np.float64)
    if theta.shape != (K.shape[1],):
        raise ValueError("tables: theta: expected [L] with L = %d, got %s" % (K.shape[1], theta.shape))
    return np.ascontiguousarray(U), np.ascontiguousarray(K), np.ascontiguousarray(Up), theta, alpha


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def _check_sizes(x, J):
    lead, nsig, R, T = _dims(x)
    if nsig * J * R * T > MAX_ELEMENTS:
        raise ValueError("X: expected at most 2^31 - 1 elements in P (N x num_sources x rows x T), got %d x %d x %d x %d" % (nsig, J, R, T))
    return lead, nsig, R, T


def _check_state(v, what, shape):
    """A real state tensor of the given shape (non-negative by contract)."""
    if v.is_complex() or tuple(v.shape) != tuple(shape):
        raise ValueError("%s: expected a real tensor shaped %s, got %s %s" % (what, tuple(shape), v.dtype, tuple(v.shape)))


def _sources(num_sources):
    return _check_range_int(num_sources, "num_sources", 1, MAX_SOURCES)


def projections(X, tab=None):
    """``V_m = |U[m][0] X_1 + U[m][1] X_2|^alpha`` of a stereo STFT [2, R, T] or [N, 2, R, T] -> float64 [.., M, R, T].  fp64 after the
    load; the fit computes the same bits in registers and never stores them.  ``glowk_projet_projections``: one launch."""
    U, K, Up, theta, alpha = _check_tables(tables() if tab is None else tab)
    x = _stereo(X)
    lead, nsig, R, T = _dims(x)
    M = U.shape[0]
    if nsig * M * R * T > MAX_ELEMENTS:
        raise ValueError("X: expected at most 2^31 - 1 projection values (N x M x rows x T), got %d x %d x %d x %d" % (nsig, M, R, T))
    V = torch.empty(lead + (M, R, T), dtype=torch.float64, device=x.device)
    Ud = _dev(U, x.device)
    _lib.check(_lib.load().glowk_projet_projections(_p(x), nsig, R, T, _p(Ud), M, alpha, _p(V), _s(x)))
    return V


def init_q(num_sources, theta):
    """The start of Q in fp64 numpy [L, J]: ``max(1 - |theta_l - t_j| / w, 0) + 0.05`` with ``t_j = (j + 1/2) pi / (2 J)`` and ``w = pi /
    (2 J)``, every column divided by its sum."""
    J = _sources(num_sources)
    theta = np.asarray(theta, dtype=np.float64)
    w = math.pi / (2 * J)
    t = (np.arange(J, dtype=np.float64) + 0.5) * math.pi / (2 * J)
    Q = np.maximum(1.0 - np.abs(theta[:, None] - t[None, :]) / w, 0.0) + 0.05
    return Q / Q.sum(axis=0, keepdims=True)


def init(X, num_sources, tab=None):
    """The deterministic start ``(P, Q)``: ``P_j = (|X_1|^2 + |X_2|^2)^(alpha / 2) / J`` [.., J, R, T] and ``init_q`` [.., L, J], float64.
    No RNG: source j starts in the j-th pan sector, so the sources come out in ascending pan order."""
    U, K, Up, theta, alpha = _check_tables(tables() if tab is None else tab)
    J = _sources(num_sources)
    x = _stereo(X)
    lead, nsig, R, T = _check_sizes(x, J)
    xr = torch.view_as_real(x).to(torch.float64)
    p1 = xr[..., 0, :, :, 0] * xr[..., 0, :, :, 0] + xr[..., 0, :, :, 1] * xr[..., 0, :, :, 1]
    p2 = xr[..., 1, :, :, 0] * xr[..., 1, :, :, 0] + xr[..., 1, :, :, 1] * xr[..., 1, :, :, 1]
    e = p1 + p2
    e = torch.sqrt(e) if alpha == 1.0 else e if alpha == 2.0 else torch.pow(e, alpha / 2)
    P = (e / J).unsqueeze(-3).expand(lead + (J, R, T)).contiguous()
    Q = _dev(init_q(J, theta), x.device).expand(lead + (len(theta), J)).contiguous()
    return P, Q


def _model(X, P, Q, tab, need_q=True):
    """The checked operands of a staged call: x, P, Q (or None), the tables (U, K, Up) on the device, alpha, dims."""
    U, K, Up, theta, alpha = _check_tables(tables() if tab is None else tab)
    x = _check_stereo(X)
    Pt = P if torch.is_tensor(P) else torch.as_tensor(np.asarray(P))
    if Pt.dim() != x.dim() or not 1 <= Pt.shape[-3] <= MAX_SOURCES:
        raise ValueError("P: expected [.., J, rows, T] with 1 <= J <= %d beside X %s, got %s" % (MAX_SOURCES, tuple(x.shape), tuple(Pt.shape)))
    J = Pt.shape[-3]
    lead, nsig, R, T = _check_sizes(x, J)
    Qt = Q if torch.is_tensor(Q) or Q is None else torch.as_tensor(np.asarray(Q))
    _check_state(Pt, "P", lead + (J, R, T))
    if need_q:
        _check_state(Qt, "Q", lead + (K.shape[1], J))
    x = x.to(device=audio._device(x, Pt, *([Qt] if need_q else [])), dtype=torch.complex64).contiguous()
    Pt = Pt.to(device=x.device, dtype=torch.float64).contiguous()
    Qt = Qt.to(device=x.device, dtype=torch.float64).contiguous() if need_q else None
    dev = (_dev(U, x.device), _dev(K, x.device), _dev(Up, x.device))                     # held by the caller until its launches are enqueued
    return x, Pt, Qt, dev, alpha, (lead, nsig, R, T, U.shape[0], K.shape[1], J)


def _gains(Kd, Q, nsig, M, L, J):
    G = torch.empty(tuple(Q.shape[:-2]) + (M, J), dtype=torch.float64, device=Q.device)
    _lib.check(_lib.load().glowk_projet_gains(_p(Kd), _p(Q), nsig, M, L, J, _p(G), _s(Q)))
    return G


def gains(Q, tab=None):
    """``G = K Q`` [.., M, J] for Q [L, J] or [N, L, J], l ascending.  ``glowk_projet_gains``: one launch."""
    U, K, Up, theta, alpha = _check_tables(tables() if tab is None else tab)
    q = Q if torch.is_tensor(Q) else torch.as_tensor(np.asarray(Q))
    if q.is_complex() or q.dim() not in (2, 3) or q.shape[-2] != K.shape[1] or not 1 <= q.shape[-1] <= MAX_SOURCES or (q.dim() == 3 and q.shape[0] > 65535):
        raise ValueError("Q: expected a real [L, J] or [N, L, J] with L = %d and 1 <= J <= %d, got %s" % (K.shape[1], MAX_SOURCES, tuple(q.shape)))
    q = q.to(device=audio._device(q), dtype=torch.float64).contiguous()
    nsig = q.shape[0] if q.dim() == 3 else 1
    return _gains(_dev(K, q.device), q, nsig, K.shape[0], K.shape[1], q.shape[-1])


def update_p(X, P, Q, tab=None, beta=1):
    """One P update -> the new P (a new tensor): ``P_j' = P_j g(sum_m G[m][j] V_m sigma_m^(beta-2) / max(sum_m G[m][j] sigma_m^(beta-1),
    FLOOR))`` with ``G = K Q``.  ``glowk_projet_gains`` and ``glowk_projet_update_p``: two launches."""
    beta = _check_beta(beta)
    x, Pt, Qt, (Ud, Kd, Upd), alpha, (lead, nsig, R, T, M, L, J) = _model(X, P, Q, tab)
    G = _gains(Kd, Qt, nsig, M, L, J)
    out = Pt.clone()
    _lib.check(_lib.load().glowk_projet_update_p(_p(x), nsig, R, T, _p(Ud), _p(G), M, J, alpha, beta, _p(out), _s(x)))
    return out


def update_q(X, P, Q, tab=None, beta=1):
    """One Q update from P as given -> the new Q (a new tensor): the outer sums ``An``, ``Ad`` over the cells on the fp64 matrix cores,
    then ``Q[l][j]' = Q[l][j] g(sum_m K[m][l] An[m][j] / max(sum_m K[m][l] Ad[m][j], FLOOR))``.  Three launches."""
    beta = _check_beta(beta)
    x, Pt, Qt, (Ud, Kd, Upd), alpha, (lead, nsig, R, T, M, L, J) = _model(X, P, Q, tab)
    lib = _lib.load()
    G = _gains(Kd, Qt, nsig, M, L, J)
    out = Qt.clone()
    nbytes = lib.glowk_projet_workspace_bytes(nsig, M, J, R, T)
    work = _work(nbytes, x.device)
    _lib.check(lib.glowk_projet_update_q(_p(x), _p(Pt), nsig, R, T, _p(Ud), _p(Kd), M, L, J, alpha, beta, _p(out), _p(G), _p(work), nbytes, _s(x)))
    return out


def _check_iter(n_iter):
    return _check_range_int(n_iter, "n_iter", 0, MAX_ITER)


def fit(X, P, Q, tab=None, beta=1, n_iter=100):
    """``n_iter`` iterations from (P, Q) -> the new ``(P, Q)``: per iteration one fused pass over X and P (the P update, then the outer
    sums of the new P in the same pass) and the Q kernel.  ``glowk_projet_fit``: ``2 n_iter + 1`` launches, bit for bit the staged calls."""
    beta, n_iter = _check_beta(beta), _check_iter(n_iter)
    x, Pt, Qt, (Ud, Kd, Upd), alpha, (lead, nsig, R, T, M, L, J) = _model(X, P, Q, tab)
    lib = _lib.load()
    Po, Qo = Pt.clone(), Qt.clone()
    G = torch.empty(lead + (M, J), dtype=torch.float64, device=x.device)
    nbytes = lib.glowk_projet_workspace_bytes(nsig, M, J, R, T)
    work = _work(nbytes, x.device)
    _lib.check(lib.glowk_projet_fit(_p(x), nsig, R, T, _p(Ud), _p(Kd), M, L, J, alpha, beta, n_iter, _p(Po), _p(Qo), _p(G),
                                    _p(work), nbytes, _s(x)))
    return Po, Qo


def divergence(X, P, Q, tab=None, beta=1):
    """``D = sum_{m, cells} d_beta(V_m | sigma_m)`` -> float64 [..] ([] for one signal).  Three launches."""
    beta = _check_beta(beta)
    x, Pt, Qt, (Ud, Kd, Upd), alpha, (lead, nsig, R, T, M, L, J) = _model(X, P, Q, tab)
    lib = _lib.load()
    G = _gains(Kd, Qt, nsig, M, L, J)
    d = torch.empty(lead, dtype=torch.float64, device=x.device)
    nbytes = lib.glowk_projet_workspace_bytes(nsig, M, J, R, T)
    work = _work(nbytes, x.device)
    _lib.check(lib.glowk_projet_divergence(_p(x), _p(Pt), nsig, R, T, _p(Ud), _p(G), M, J, alpha, beta, _p(d), _p(work), nbytes, _s(x)))
    return d


def separate(X, P, Q, tab=None):
    """The stems, complex64 [.., J, 2, R, T]: ``w_mj = P_j G[m][j] / sigma_m`` (1 / J where the model is below FLOOR), ``Y_j[ch] = sum_m
    Up[ch][m] w_mj c_m``.  The stems of a cell add up to X.  Two launches."""
    x, Pt, Qt, (Ud, Kd, Upd), alpha, (lead, nsig, R, T, M, L, J) = _model(X, P, Q, tab)
    G = _gains(Kd, Qt, nsig, M, L, J)
    Y = torch.empty(lead + (J, 2, R, T), dtype=torch.complex64, device=x.device)
    _lib.check(_lib.load().glowk_projet_separate(_p(x), _p(Pt), nsig, R, T, _p(Ud), _p(Upd), _p(G), M, J, _p(Y), _s(x)))
    return Y


def pan_estimates(Q, theta=None):
    """The pan angle of every source, ``theta[argmax_l Q[l][j]]`` -> float64 [.., J]; ties go to the lowest l.  ``theta`` defaults to the
    grid of ``pan_angles(L)``."""
    q = Q if torch.is_tensor(Q) else torch.as_tensor(np.asarray(Q))
    if q.is_complex() or q.dim() not in (2, 3) or not 1 <= q.shape[-2] <= MAX_PANS or not 1 <= q.shape[-1] <= MAX_SOURCES:
        raise ValueError("Q: expected a real [L, J] or [N, L, J] with 1 <= L <= %d and 1 <= J <= %d, got %s" % (MAX_PANS, MAX_SOURCES, tuple(q.shape)))
    L = q.shape[-2]
    th = pan_angles(L) if theta is None else np.asarray(theta, dtype=np.float64)
    if th.shape != (L,):
        raise ValueError("theta: expected [L] with L = %d, got %s" % (L, th.shape))
    best = q.max(dim=-2, keepdim=True).values
    first = torch.where(q == best, torch.arange(L, device=q.device).view(L, 1).expand_as(q), L).min(dim=-2).values   # the lowest l of a tie
    return torch.from_numpy(th).to(q.device)[first]


_PROJET_DEFAULTS = dict(num_projections=15, num_pans=41, alpha=1.0, beta=1, n_iter=100)


def _check_projet_params(num_sources, num_projections, num_pans, alpha, beta, n_iter):
    _sources(num_sources)
    _check_range_int(num_projections, "num_projections", MIN_PROJECTIONS, MAX_PROJECTIONS)
    _check_range_int(num_pans, "num_pans", 1, MAX_PANS)
    _check_alpha(alpha)
    _check_beta(beta)
    _check_iter(n_iter)


def projet(X, num_sources, num_projections=15, num_pans=41, alpha=1.0, beta=1, n_iter=100, return_model=False):
    """PROJET on a stereo STFT [2, R, T] or [N, 2, R, T] -> the stems, complex64 [.., J, 2, R, T], in ascending pan order.  ``init``,
    ``fit`` (``2 n_iter + 1`` launches), ``separate``; no host synchronisation.  ``return_model`` adds a dict with ``P``, ``Q`` and
    ``pans`` (``pan_estimates``)."""
    _check_projet_params(num_sources, num_projections, num_pans, alpha, beta, n_iter)
    return_model = _check_flag(return_model, "return_model")
    tab = tables(num_projections, num_pans, alpha)
    x = _stereo(X)
    P, Q = init(x, num_sources, tab)
    P, Q = fit(x, P, Q, tab, beta, n_iter)
    Y = separate(x, P, Q, tab)
    return (Y, dict(P=P, Q=Q, pans=pan_estimates(Q, tab["theta"]))) if return_model else Y


_PROJET_AUDIO_DEFAULTS = dict(_PROJET_DEFAULTS, residual=False)


def _check_projet_audio_params(num_sources, num_projections, num_pans, alpha, beta, n_iter, residual):
    _check_projet_params(num_sources, num_projections, num_pans, alpha, beta, n_iter)
    _check_flag(residual, "residual")


def projet_audio(y, num_sources, num_projections=15, num_pans=41, alpha=1.0, beta=1, n_iter=100, residual=False):
    """PROJET for two channels of 16 kHz audio [2, n], n > 1024 -> stems [J, 2, n] aligned with y, in ascending pan order; with
    ``residual`` also ``y - stems.sum(0)``.  The path of ``iva.iva_audio``: one STFT of the whole signal
    (``audio.mel_frames(return_stft=True)``), ``projet`` on it, one ``audio.istft`` of the stems, trimmed to n samples.  At most 32 768
    frames."""
    _check_projet_audio_params(num_sources, num_projections, num_pans, alpha, beta, n_iter, residual)
    t = audio._tensor(y, "y")
    if t.dim() != 2 or t.shape[0] != 2:
        raise ValueError("y: expected two channels [2, n], got %s" % (tuple(t.shape),))
    x = audio._long_audio(t)
    n = x.shape[1]
    if 1 + -(-n // audio.HOP) > MAX_FRAMES:
        raise ValueError("y: expected at most %d frames (%d samples), got %d samples" % (MAX_FRAMES, (MAX_FRAMES - 2) * audio.HOP, n))
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [2, 1025, F]
    Y = projet(X, num_sources, num_projections, num_pans, alpha, beta, n_iter)          # [J, 2, 1025, F]
    stems = audio.istft(Y)[..., :n].contiguous()                                         # [J, 2, n]
    return (stems, x - stems.sum(0)) if residual else stems


def separate_wav_projet(path, num_sources, out_rate="input", **kwargs):
    """``projet_audio`` for a two-channel PCM wav at any rate -> ``(stems, rate)``, the wrapper ``duet.separate_wav_duet`` is around
    ``duet_audio``: stems [J, 2, n'] ([J + 1, 2, n'] with ``residual=True``, the residual last) at ``out_rate``: 'input' (the file's
    rate and exactly its sample count), an integer rate, or None (16 kHz).  ``kwargs`` are ``projet_audio``'s keyword arguments; any
    other is refused before the file is opened.  A file that does not have exactly two channels is refused."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    unknown = set(kwargs) - set(_PROJET_AUDIO_DEFAULTS)
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected projet_audio's" % sorted(unknown))
    _check_projet_audio_params(num_sources, **dict(_PROJET_AUDIO_DEFAULTS, **kwargs))
    y, native = audio.load_audio(path, sr=None, mono=False)
    if y.dim() != 2 or y.shape[0] != 2:
        raise ValueError("%s: expected a file with exactly two channels, got %d" % (path, 1 if y.dim() == 1 else y.shape[0]))
    n_file = y.shape[1]
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    out = projet_audio(y, num_sources, **kwargs)
    stems = torch.cat([out[0], out[1][None]]) if kwargs.get("residual", False) else out
    stems = audio.resample(stems, audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate
