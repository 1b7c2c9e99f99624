"""Clustering of time-frequency cells: the mechanism behind nussl's ``PrimitiveClustering`` (Seetharaman, Wichern, Le Roux & Pardo,
"Bootstrapping single-channel source separation via unsupervised spatial clustering on stereo mixtures", 2019) and
``SpatialClustering``.  Every cell has a small feature vector and a weight; a Gaussian mixture with full covariances is fitted to the
weighted cells by EM and its posteriors are the masks.  Two separators are that mechanism on two feature sets: ``ensemble`` (the
foreground masks of several of the package's prior-free separators) and ``spatial`` (the pan angle, optionally the delay, of a stereo
STFT).  No priors, no training.  Not in the reference.

Kernels in ``csrc/glowk_cluster.h`` (formulas in include/glowk.h, design in DESIGN 27):

* ``init``: pass 0 (total weight and origin) and the deterministic principal-axis start -- no seed; the sources come out in ascending
  order along the principal axis of the weighted features;
* ``stats``, ``update``, ``log_likelihood``: the stages of an iteration; ``fit``: the whole loop in one library call, two launches per
  iteration, the weighted moments on the fp64 matrix cores, per-signal stop without host synchronisation;
* ``posteriors`` (masks, and masked spectra in the same pass), ``labels``;
* ``mask_features``, ``spatial_features``: the two feature sets;
* ``ensemble`` / ``spatial`` and their ``*_audio`` / ``separate_wav_*`` paths.

Conventions as in ``projet.py``: numpy or torch in, tensors on the GPU the input lives on out, ValueError for bad arguments before the
library is loaded, no host synchronisation.
"""
import statistics

import numpy as np
import torch

from . import _lib, audio
from .audio import _p, _s
from .duet import _number, _stereo, _work
from .repet import MAX_FRAMES, _check_flag, _check_range_int

MAX_FEATURES, MAX_CLUSTERS, MAX_ITER, MAX_SIGNALS, MAX_ROWS = 8, 8, 100000, 65535, 4096
MAX_ELEMENTS = (1 << 31) - 1
MIN_REG = 2.0 ** -40
STATUS_ZERO_WEIGHT, STATUS_DEAD, STATUS_CHOLESKY = 1, 2, 4
STATE_KEYS = ("weights", "means", "covariances", "origin", "total")


def quantiles(num_sources):
    """``z_j``: the standard-normal quantile of ``(j + 1/2) / J``, fp64 numpy [J] -- the table of the start."""
    J = _sources(num_sources)
    nd = statistics.NormalDist()
    return np.array([nd.inv_cdf((j + 0.5) / J) for j in range(J)], dtype=np.float64)


def stat_size(D, J):
    """The length of a signal's statistics: per cluster N, a [D] and the upper triangle of B; then LL."""
    return J * (1 + D + D * (D + 1) // 2) + 1


def _sources(num_sources):
    return _check_range_int(num_sources, "num_sources", 1, MAX_CLUSTERS)


def _check_reg(reg_covar):
    r = _number(reg_covar, "reg_covar")
    if not r >= MIN_REG:
        raise ValueError("reg_covar: expected a number >= 2^-40, got %r" % (reg_covar,))
    return r


def _check_tol(tol):
    t = _number(tol, "tol")
    if not t >= 0:
        raise ValueError("tol: expected a number >= 0, got %r" % (tol,))
    return t


def _check_iter(n_iter):
    return _check_range_int(n_iter, "n_iter", 0, MAX_ITER)


def _as_tensor(v):
    return v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))


def _check_features(F, w=None):
    """F [D, R, T] or [N, D, R, T] real (and w [R, T] or [N, R, T] beside it) -> (F, w, lead, nsig, D, R, T), tensors where they are."""
    f = _as_tensor(F)
    if f.is_complex() or f.dim() not in (3, 4) or not 1 <= f.shape[-3] <= MAX_FEATURES or not 1 <= f.shape[-2] <= MAX_ROWS \
            or not 1 <= f.shape[-1] <= MAX_FRAMES or (f.dim() == 4 and f.shape[0] > MAX_SIGNALS):
        raise ValueError("F: expected real features [D, rows, T] or [N, D, rows, T] with N <= %d, 1 <= D <= %d, 1 <= rows <= %d, 1 <= T <= %d, "
                         "got %s %s" % (MAX_SIGNALS, MAX_FEATURES, MAX_ROWS, MAX_FRAMES, f.dtype, tuple(f.shape)))
    D, R, T = f.shape[-3:]
    lead = tuple(f.shape[:-3])
    nsig = f.shape[0] if f.dim() == 4 else 1
    if nsig * max(D, MAX_CLUSTERS) * R * T > MAX_ELEMENTS:
        raise ValueError("F: expected at most 2^31 - 1 elements in N x 8 x rows x T, got %s" % (tuple(f.shape),))
    wt = None
    if w is not None:
        wt = _as_tensor(w)
        if wt.is_complex() or tuple(wt.shape) != lead + (R, T):
            raise ValueError("w: expected real weights shaped %s beside F %s, got %s %s" % (lead + (R, T), tuple(f.shape), wt.dtype, tuple(wt.shape)))
    return f, wt, lead, nsig, D, R, T


def _need_w(w):
    if w is None:
        raise ValueError("w: expected real weights beside F, got None")
    return w


def _to_dev(t, dev, dtype):
    return t.to(device=dev, dtype=dtype).contiguous()


def _check_state(state, lead, D, what="state"):
    """The state dict -> (J, the five tensors where they are), shapes checked against F's."""
    if not isinstance(state, dict) or not set(STATE_KEYS) <= set(state):
        raise ValueError("%s: expected the dict of cluster.init or cluster.fit (%s), got %r" % (what, ", ".join(STATE_KEYS), type(state)))
    ts = [_as_tensor(state[k]) for k in STATE_KEYS]
    pi = ts[0]
    if pi.is_complex() or pi.dim() != len(lead) + 1 or tuple(pi.shape[:-1]) != lead or not 1 <= pi.shape[-1] <= MAX_CLUSTERS:
        raise ValueError("%s: weights: expected real %s + [J] with 1 <= J <= %d, got %s" % (what, lead, MAX_CLUSTERS, tuple(pi.shape)))
    J = pi.shape[-1]
    for k, t, shape in zip(STATE_KEYS[1:], ts[1:], (lead + (J, D), lead + (J, D, D), lead + (D,), lead)):
        if t.is_complex() or tuple(t.shape) != shape:
            raise ValueError("%s: %s: expected a real tensor shaped %s, got %s %s" % (what, k, shape, t.dtype, tuple(t.shape)))
    return J, ts


def _state_dev(ts, dev):
    return [_to_dev(t, dev, torch.float64) for t in ts]


def _empty_state(lead, D, J, dev):
    f64 = dict(dtype=torch.float64, device=dev)
    return [torch.empty(lead + (J,), **f64), torch.empty(lead + (J, D), **f64), torch.empty(lead + (J, D, D), **f64), torch.empty(lead + (D,), **f64),
            torch.empty(lead, **f64)]


def _state_dict(ts, **extra):
    return dict(zip(STATE_KEYS, ts), **extra)


def init(F, w, num_sources, reg_covar=1e-6):
    """The deterministic start -> ``dict(weights [.., J], means [.., J, D], covariances [.., J, D, D], origin [.., D], total [..],
    status [..])``, float64 (status int32).  ``total = sum w``, ``origin = sum w x / total``; ``Sigma0`` the weighted covariance plus
    ``reg_covar I``; v its principal axis (64 power-iteration steps from all ones, the earliest component of largest magnitude positive);
    ``mu_j = mean + z_j sqrt(v^T Sigma0 v) v`` with ``z_j = quantiles(J)``; ``Sigma_j = Sigma0``; ``pi_j = 1 / J``.  No seed.
    ``glowk_cluster_init``: four launches."""
    J, reg = _sources(num_sources), _check_reg(reg_covar)
    f, wt, lead, nsig, D, R, T = _check_features(F, _need_w(w))
    dev = audio._device(f, wt)
    f, wt = _to_dev(f, dev, torch.float32), _to_dev(wt, dev, torch.float32)
    st = _empty_state(lead, D, J, dev)
    status = torch.zeros(lead, dtype=torch.int32, device=dev)
    lib = _lib.load()
    z = torch.from_numpy(quantiles(J)).to(dev)
    nbytes = lib.glowk_cluster_work_bytes(nsig, D, J, R, T)
    work = _work(nbytes, dev)
    _lib.check(lib.glowk_cluster_init(_p(f), _p(wt), nsig, D, J, R, T, _p(z), reg, *[_p(t) for t in st], _p(status), _p(work), nbytes, _s(f)))
    return _state_dict(st, status=status)


def stats(F, w, state):
    """The weighted moments of the E-step of ``state`` -> float64 [.., J (1 + D + D (D + 1) / 2) + 1]: per cluster ``N_j``, ``a_j`` and the
    upper triangle of ``B_j`` (moments of ``x - origin``), then ``LL = sum w lse``.  ``glowk_cluster_stats``: three launches."""
    f, wt, lead, nsig, D, R, T = _check_features(F, _need_w(w))
    J, ts = _check_state(state, lead, D)
    dev = audio._device(f, wt, *ts)
    f, wt, ts = _to_dev(f, dev, torch.float32), _to_dev(wt, dev, torch.float32), _state_dev(ts, dev)
    out = torch.empty(lead + (stat_size(D, J),), dtype=torch.float64, device=dev)
    status = torch.zeros(lead, dtype=torch.int32, device=dev)
    lib = _lib.load()
    nbytes = lib.glowk_cluster_work_bytes(nsig, D, J, R, T)
    work = _work(nbytes, dev)
    _lib.check(lib.glowk_cluster_stats(_p(f), _p(wt), nsig, D, J, R, T, *[_p(t) for t in ts], _p(out), _p(status), _p(work), nbytes, _s(f)))
    return out


def log_likelihood(stats, state):
    """``ll = LL / total`` of statistics -> float64 [..]; NaN where the total weight is 0."""
    s, W = _as_tensor(stats), _as_tensor(state["total"])
    if s.is_complex() or s.dim() != W.dim() + 1:
        raise ValueError("stats: expected the statistics of cluster.stats beside the state, got %s" % (tuple(s.shape),))
    W = W.to(s.device)
    return torch.where(W > 0, s[..., -1] / W, torch.full_like(W, float("nan")))


def update(stats, state, reg_covar=1e-6):
    """The M-step -> the new state (new tensors; ``log_likelihood`` and ``status`` added): ``pi_j = N_j / W``, ``mu_j = o + a_j / N_j``,
    ``Sigma_j = B_j / N_j - (a_j / N_j)(a_j / N_j)^T + reg_covar I``; a cluster with ``N_j < 2^-40 W`` is dead (pi 0, mu and Sigma kept);
    a failed Cholesky factorisation of any new covariance leaves the signal's state as it was.  ``glowk_cluster_update``: one launch."""
    reg = _check_reg(reg_covar)
    s = _as_tensor(stats)
    if s.is_complex() or s.dim() < 1:
        raise ValueError("stats: expected the statistics of cluster.stats, got %s %s" % (s.dtype, tuple(s.shape)))
    lead = tuple(s.shape[:-1])
    if not isinstance(state, dict) or "origin" not in state:
        raise ValueError("state: expected the dict of cluster.init or cluster.fit, got %r" % (type(state),))
    D = _as_tensor(state["origin"]).shape[-1] if _as_tensor(state["origin"]).dim() else 0
    if not 1 <= D <= MAX_FEATURES or len(lead) > 1:
        raise ValueError("state: origin: expected [D] or [N, D] with 1 <= D <= %d" % MAX_FEATURES)
    J, ts = _check_state(state, lead, D)
    if s.shape[-1] != stat_size(D, J):
        raise ValueError("stats: expected %d statistics per signal for D = %d, J = %d, got %d" % (stat_size(D, J), D, J, s.shape[-1]))
    dev = audio._device(s, *ts)
    s = _to_dev(s, dev, torch.float64)
    ts = [t.clone() for t in _state_dev(ts, dev)]
    nsig = s.shape[0] if lead else 1
    ll = torch.empty(lead, dtype=torch.float64, device=dev)
    status = torch.zeros(lead, dtype=torch.int32, device=dev)
    lib = _lib.load()
    nbytes = lib.glowk_cluster_work_bytes(nsig, D, J, 1, 1)
    work = _work(nbytes, dev)
    _lib.check(lib.glowk_cluster_update(_p(s), nsig, D, J, reg, _p(ts[0]), _p(ts[1]), _p(ts[2]), _p(ts[3]), _p(ts[4]), _p(ll), _p(status), _p(work), nbytes, _s(s)))
    return _state_dict(ts, log_likelihood=ll, status=status)


def _check_start(means, covariances, weights, lead, D, J):
    """Explicit start tensors (or None each), shapes checked."""
    out = []
    for name, v, shape in (("means", means, lead + (J, D)), ("covariances", covariances, lead + (J, D, D)), ("weights", weights, lead + (J,))):
        if v is None:
            out.append(None)
            continue
        t = _as_tensor(v)
        if t.is_complex() or tuple(t.shape) not in (shape, shape[len(lead):]):
            raise ValueError("%s: expected a real tensor shaped %s, got %s %s" % (name, shape, t.dtype, tuple(t.shape)))
        out.append(t)
    if means is None and (covariances is not None or weights is not None):
        raise ValueError("covariances, weights: an explicit start needs means")
    return out


def fit(F, w, num_sources, n_iter=50, tol=1e-6, reg_covar=1e-6, means=None, covariances=None, weights=None):
    """EM from the deterministic start (or from explicit ``means`` [.., J, D], with ``covariances`` and ``weights`` defaulting to the
    start's) -> the state plus ``log_likelihood`` [.., n_iter] (``ll_k`` of the state before update k; NaN after a signal stopped),
    ``iterations`` and ``status`` [..] int32.  A signal stops after update k >= 1 when ``ll_k - ll_{k-1} <= tol |ll_k|`` and is frozen;
    ``tol = 0`` runs all ``n_iter``.  ``glowk_cluster_fit``: two launches per iteration, bit for bit ``init`` and the staged calls."""
    J, n_iter, tol, reg = _sources(num_sources), _check_iter(n_iter), _check_tol(tol), _check_reg(reg_covar)
    f, wt, lead, nsig, D, R, T = _check_features(F, _need_w(w))
    start = _check_start(means, covariances, weights, lead, D, J)
    dev = audio._device(f, wt, *[t for t in start if t is not None])
    f, wt = _to_dev(f, dev, torch.float32), _to_dev(wt, dev, torch.float32)
    lib = _lib.load()
    nbytes = lib.glowk_cluster_work_bytes(nsig, D, J, R, T)
    work = _work(nbytes, dev)
    status = torch.zeros(lead, dtype=torch.int32, device=dev)
    z = torch.from_numpy(quantiles(J)).to(dev)
    st = _empty_state(lead, D, J, dev)
    if start[0] is not None:
        _lib.check(lib.glowk_cluster_init(_p(f), _p(wt), nsig, D, J, R, T, _p(z), reg, *[_p(t) for t in st], _p(status), _p(work), nbytes, _s(f)))
        for i, t in zip((1, 2, 0), start):
            if t is not None:
                st[i].copy_(t.to(device=dev, dtype=torch.float64).expand_as(st[i]))
    ll = torch.empty(lead + (n_iter,), dtype=torch.float64, device=dev)
    iters = torch.zeros(lead, dtype=torch.int32, device=dev)
    _lib.check(lib.glowk_cluster_fit(_p(f), _p(wt), nsig, D, J, R, T, _p(z) if start[0] is None else None, reg, n_iter, tol, *[_p(t) for t in st],
                                     _p(ll) if n_iter else None, _p(iters), _p(status), _p(work), nbytes, _s(f)))
    return _state_dict(st, log_likelihood=ll, iterations=iters, status=status)


def _check_spectrum(X, lead, R, T):
    """X [.., R, T] or [.., C, R, T] complex with C in {1, 2} -> (tensor where it is, C, whether it has the channel axis)."""
    x = _as_tensor(X)
    if not x.is_complex():
        raise ValueError("X: expected a complex spectrum, got %s" % (x.dtype,))
    if tuple(x.shape) == lead + (R, T):
        return x, 1, False
    if x.dim() == len(lead) + 3 and tuple(x.shape[:len(lead)]) == lead and x.shape[-3] in (1, 2) and tuple(x.shape[-2:]) == (R, T):
        return x, x.shape[-3], True
    raise ValueError("X: expected %s or %s with C in {1, 2}, got %s" % (lead + (R, T), lead + ("C", R, T), tuple(x.shape)))


def posteriors(F, state, X=None):
    """The masks ``r_j`` -> float32 [.., J, R, T]; with a complex spectrum X [.., R, T] or [.., C, R, T] (C in {1, 2}) the masked
    spectra ``mask_j X`` instead, complex64 [.., J, R, T] or [.., J, C, R, T], written in the same pass.  A signal whose total weight
    is 0 gets ``1 / J``.  ``glowk_cluster_posteriors``: two launches."""
    f, _, lead, nsig, D, R, T = _check_features(F)
    J, ts = _check_state(state, lead, D)
    xs = None if X is None else _check_spectrum(X, lead, R, T)
    if xs is not None and nsig * J * xs[1] * R * T > MAX_ELEMENTS:
        raise ValueError("X: expected at most 2^31 - 1 elements in the masked spectra")
    dev = audio._device(f, *ts, *([xs[0]] if xs else []))
    f, ts = _to_dev(f, dev, torch.float32), _state_dev(ts, dev)
    mask = torch.empty(lead + (J, R, T), dtype=torch.float32, device=dev)
    status = torch.zeros(lead, dtype=torch.int32, device=dev)
    x = y = None
    C = 1
    if xs is not None:
        x, C = _to_dev(xs[0], dev, torch.complex64), xs[1]
        y = torch.empty(lead + ((J, C, R, T) if xs[2] else (J, R, T)), dtype=torch.complex64, device=dev)
    lib = _lib.load()
    nbytes = lib.glowk_cluster_work_bytes(nsig, D, J, 1, 1)
    work = _work(nbytes, dev)
    _lib.check(lib.glowk_cluster_posteriors(_p(f), nsig, D, J, R, T, *[_p(t) for t in ts], _p(x), C, _p(mask), _p(y), _p(status), _p(work), nbytes, _s(f)))
    return mask if y is None else y


def labels(F, state):
    """The hard assignment: float32 [.., J, R, T], 1 for the cluster of largest posterior (the earliest of equals), else 0."""
    m = posteriors(F, state)
    J = m.shape[-3]
    best = m.max(dim=-3, keepdim=True).values
    idx = torch.arange(J, device=m.device).view(J, 1, 1).expand_as(m)
    first = torch.where(m == best, idx, J).min(dim=-3, keepdim=True).values
    return (idx == first).to(torch.float32)


def mask_features(*masks):
    """Real planes [R, T] or [N, R, T] of one shape -> the feature tensor float32 [.., D, R, T], 1 <= D <= 8."""
    if not 1 <= len(masks) <= MAX_FEATURES:
        raise ValueError("masks: expected 1 to %d planes, got %d" % (MAX_FEATURES, len(masks)))
    ts = [_as_tensor(m) for m in masks]
    for t in ts:
        if t.is_complex() or t.dim() not in (2, 3) or tuple(t.shape) != tuple(ts[0].shape):
            raise ValueError("masks: expected real planes [rows, T] or [N, rows, T] of one shape, got %s" % ([tuple(t.shape) for t in ts],))
    dev = audio._device(*ts)
    return torch.stack([t.to(device=dev, dtype=torch.float32) for t in ts], dim=-3).contiguous()


def _check_spatial_params(delay, max_delay, p):
    delay = _check_flag(delay, "delay")
    max_delay, p = _number(max_delay, "max_delay"), _number(p, "p")
    if not max_delay > 0:
        raise ValueError("max_delay: expected a number > 0, got %r" % (max_delay,))
    if not p > 0:
        raise ValueError("p: expected a number > 0, got %r" % (p,))
    return delay, max_delay, p


def spatial_features(X, delay=False, max_delay=3.0, p=1.0):
    """The spatial cues of a stereo STFT [2, R, T] or [N, 2, R, T] -> ``(F, w)``: ``F`` float32 [.., D, R, T] with ``pan = atan2(|X2|,
    |X1|) - pi / 4`` and, with ``delay``, DUET's ``delta`` (``duet.features``) clipped to ``+-max_delay`` (D = 2); ``w = (|X1|^2 +
    |X2|^2)^(p / 2)``, 0 in row 0 and where both channels are exactly 0.  fp64 arithmetic, rounded to float32.  The delay is off by
    default: on amplitude-panned mixtures it is noise and takes over the principal axis.  ``glowk_cluster_spatial_features``: one launch."""
    delay, max_delay, p = _check_spatial_params(delay, max_delay, p)
    x = _stereo(X)
    lead, R, T = tuple(x.shape[:-3]), x.shape[-2], x.shape[-1]
    nsig = x.shape[0] if x.dim() == 4 else 1
    F = torch.empty(lead + (2 if delay else 1, R, T), dtype=torch.float32, device=x.device)
    w = torch.empty(lead + (R, T), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().glowk_cluster_spatial_features(_p(x), nsig, R, T, int(delay), max_delay, p, _p(F), _p(w), _s(x)))
    return F, w


_FIT_DEFAULTS = dict(n_iter=50, tol=1e-6, reg_covar=1e-6)


def _check_fit_kwargs(kw):
    unknown = set(kw) - set(_FIT_DEFAULTS)
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected n_iter, tol, reg_covar" % sorted(unknown))
    k = dict(_FIT_DEFAULTS, **kw)
    _check_iter(k["n_iter"]), _check_tol(k["tol"]), _check_reg(k["reg_covar"])
    return k


def spatial(X, num_sources, delay=False, max_delay=3.0, p=1.0, mask=False, return_model=False, **fit_kwargs):
    """Spatial clustering of a stereo STFT [2, R, T] or [N, 2, R, T] -> the stems, complex64 [.., J, 2, R, T], in ascending pan order;
    ``mask=True`` returns the masks [.., J, R, T] instead.  ``spatial_features``, ``fit``, ``posteriors``; ``fit_kwargs`` are ``n_iter``,
    ``tol`` and ``reg_covar``.  ``return_model`` adds the fitted state."""
    J = _sources(num_sources)
    _check_spatial_params(delay, max_delay, p)
    mask, return_model = _check_flag(mask, "mask"), _check_flag(return_model, "return_model")
    kw = _check_fit_kwargs(fit_kwargs)
    x = _stereo(X)
    F, w = spatial_features(x, delay, max_delay, p)
    model = fit(F, w, J, **kw)
    out = posteriors(F, model, None if mask else x)
    return (out, model) if return_model else out


PRIMITIVES = ("melody", "repet_sim", "ft2d", "hpss", "rpca", "repet", "repet_adaptive")


def _primitive_mask(name, kwargs, mag):
    """The foreground (lead, percussive) mask of one named separator on the magnitudes."""
    from . import ft2d, hpss, melody, repet, rpca
    if name == "melody":
        return melody.melody(mag, mask=True, **kwargs)[0]
    if name == "hpss":
        return hpss.hpss(mag, mask=True, **kwargs)[1]
    if name == "repet_sim":
        return repet.repet_sim(mag, mask=True, **kwargs)[1]
    if name == "ft2d":
        return ft2d.ft2d(mag, mask=True, **kwargs)[1]
    if name == "rpca":
        return rpca.rpca(mag, mask=True, **kwargs)[1]
    if name == "repet":
        return repet.repet(mag, mask=True, **kwargs)[1]
    if "win" not in kwargs:
        kwargs = dict(kwargs, win=min(mag.shape[-1], 128))
    return repet.repet_adaptive(mag, mask=True, **kwargs)[1]


def _check_primitives(primitives):
    """-> a list of (name, kwargs) pairs and ready mask tensors."""
    if not isinstance(primitives, (tuple, list)) or not 1 <= len(primitives) <= MAX_FEATURES:
        raise ValueError("primitives: expected 1 to %d names, (name, kwargs) pairs or mask tensors, got %r" % (MAX_FEATURES, primitives))
    out = []
    for prim in primitives:
        if isinstance(prim, str):
            prim = (prim, {})
        if isinstance(prim, tuple) and len(prim) == 2 and isinstance(prim[0], str) and isinstance(prim[1], dict):
            if prim[0] not in PRIMITIVES:
                raise ValueError("primitives: expected names among %s, got %r" % (PRIMITIVES, prim[0]))
            if "mask" in prim[1]:
                raise ValueError("primitives: %s: 'mask' is set by ensemble" % (prim[0],))
            out.append(prim)
        elif torch.is_tensor(prim) or isinstance(prim, np.ndarray):
            out.append(_as_tensor(prim))
        else:
            raise ValueError("primitives: expected a name, a (name, kwargs) pair or a mask tensor, got %r" % (type(prim),))
    return out


def _check_power(power):
    p = _number(power, "power")
    if not p > 0:
        raise ValueError("power: expected a number > 0, got %r" % (power,))
    return p


def ensemble(S, primitives=("melody", "repet_sim", "ft2d", "hpss"), num_sources=2, power=1.0, mask=False, return_model=False, **fit_kwargs):
    """Ensemble (primitive) clustering of spectra [rows, T] or [N, rows, T] -> the stems [.., J, rows, T] (complex64 with S's phase for
    complex S, else float32 magnitudes); ``mask=True`` returns the masks instead.  The named separators run on ``|S|`` with
    ``mask=True`` and each one's foreground (lead, percussive) mask is one feature of a cell; ``primitives`` may also hold ``(name,
    kwargs)`` pairs or ready mask tensors shaped like S.  The weights are ``|S|^power``.  The sources come out in ascending order along
    the principal axis of the masks, so the last one is the most "foreground".  ``fit_kwargs`` are ``n_iter``, ``tol`` and
    ``reg_covar``; ``return_model`` adds the fitted state and the features."""
    from .hpss import _spectra
    prims = _check_primitives(primitives)
    J, power = _sources(num_sources), _check_power(power)
    mask, return_model = _check_flag(mask, "mask"), _check_flag(return_model, "return_model")
    kw = _check_fit_kwargs(fit_kwargs)
    x = _spectra(S)
    for t in prims:
        if torch.is_tensor(t) and (t.is_complex() or tuple(t.shape) != tuple(x.shape)):
            raise ValueError("primitives: expected real mask tensors shaped like S %s, got %s %s" % (tuple(x.shape), t.dtype, tuple(t.shape)))
    dev = audio._device(x, *[t for t in prims if torch.is_tensor(t)])
    if x.is_complex():
        x = x.to(device=dev, dtype=torch.complex64).contiguous()
        mag = x.abs()
    else:
        x = None
        mag = _spectra(S).to(device=dev, dtype=torch.float32).contiguous()
    F = mask_features(*[t.to(dev) if torch.is_tensor(t) else _primitive_mask(t[0], t[1], mag) for t in prims])
    w = mag if power == 1.0 else mag * mag if power == 2.0 else mag ** power
    model = fit(F, w, J, **kw)
    if mask:
        out = posteriors(F, model)
    elif x is not None:
        out = posteriors(F, model, x)
    else:
        out = posteriors(F, model) * mag.unsqueeze(-3)
    return (out, dict(model, features=F)) if return_model else out


def _audio_in(y, what="y"):
    t = audio._tensor(y, what)
    x = audio._long_audio(t)
    n = x.shape[1]
    if 1 + -(-n // audio.HOP) > MAX_FRAMES:
        raise ValueError("y: expected at most %d frames (%d samples), got %d samples" % (MAX_FRAMES, (MAX_FRAMES - 2) * audio.HOP, n))
    return t, x, n


_ENSEMBLE_AUDIO_KEYS = {"primitives", "num_sources", "power", "residual"} | set(_FIT_DEFAULTS)
_SPATIAL_AUDIO_KEYS = {"delay", "max_delay", "p", "residual"} | set(_FIT_DEFAULTS)


def ensemble_audio(y, primitives=("melody", "repet_sim", "ft2d", "hpss"), num_sources=2, power=1.0, residual=False, **fit_kwargs):
    """``ensemble`` for 16 kHz audio [n] or [C, n], n > 1024 -> stems [J, n] or [J, C, n] aligned with y; with ``residual`` also ``y -
    stems.sum(0)``.  One STFT of the whole signal (``audio.mel_frames``), ``ensemble`` per channel, one ``audio.istft`` of the stems,
    trimmed to n samples.  At most 32 768 frames."""
    _check_primitives(primitives), _sources(num_sources), _check_power(power), _check_fit_kwargs(fit_kwargs)
    residual = _check_flag(residual, "residual")
    t, x, n = _audio_in(y)
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [C, 1025, F]
    Y = ensemble(X, primitives, num_sources, power, **fit_kwargs)                        # [C, J, 1025, F]
    stems = audio.istft(Y)[..., :n].transpose(0, 1).contiguous()                         # [J, C, n]
    if t.dim() == 1:
        stems, x = stems[:, 0], x[0]
    return (stems, x - stems.sum(0)) if residual else stems


def spatial_audio(y, num_sources, delay=False, max_delay=3.0, p=1.0, residual=False, **fit_kwargs):
    """``spatial`` for two channels of 16 kHz audio [2, n], n > 1024 -> stems [J, 2, n] aligned with y, in ascending pan order; with
    ``residual`` also ``y - stems.sum(0)``.  The path of ``projet.projet_audio``."""
    _sources(num_sources), _check_spatial_params(delay, max_delay, p), _check_fit_kwargs(fit_kwargs)
    residual = _check_flag(residual, "residual")
    t, x, n = _audio_in(y)
    if t.dim() != 2 or t.shape[0] != 2:
        raise ValueError("y: expected two channels [2, n], got %s" % (tuple(t.shape),))
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [2, 1025, F]
    Y = spatial(X, num_sources, delay, max_delay, p, **fit_kwargs)                       # [J, 2, 1025, F]
    stems = audio.istft(Y)[..., :n].contiguous()
    return (stems, x - stems.sum(0)) if residual else stems


def _check_out_rate(out_rate):
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    return out_rate


def _wav_out(out, residual, native, out_rate, n_file):
    stems = torch.cat([out[0], out[1][None]]) if residual else out
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    stems = audio.resample(stems, audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate


def separate_wav_ensemble(path, out_rate="input", mono=False, **kwargs):
    """``ensemble_audio`` for a PCM wav at any rate -> ``(stems, rate)``: stems [J, n'] of a one-channel file or with ``mono`` (the
    channels averaged), else [J, C, n'] ([J + 1, ..] with ``residual=True``, the residual last), at ``out_rate``: 'input' (the file's
    rate and exactly its sample count), an integer rate, or None (16 kHz).  ``kwargs`` are ``ensemble_audio``'s keyword arguments; any
    other is refused before the file is opened."""
    out_rate, mono = _check_out_rate(out_rate), _check_flag(mono, "mono")
    unknown = set(kwargs) - _ENSEMBLE_AUDIO_KEYS
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected ensemble_audio's" % sorted(unknown))
    _check_primitives(kwargs.get("primitives", ("melody", "repet_sim", "ft2d", "hpss"))), _sources(kwargs.get("num_sources", 2))
    _check_power(kwargs.get("power", 1.0)), _check_flag(kwargs.get("residual", False), "residual")
    _check_fit_kwargs({k: v for k, v in kwargs.items() if k in _FIT_DEFAULTS})
    y, native = audio.load_audio(path, sr=None, mono=False)
    n_file = y.shape[1]
    y = y.mean(0) if mono or y.shape[0] == 1 else y
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    return _wav_out(ensemble_audio(y, **kwargs), kwargs.get("residual", False), native, out_rate, n_file)


def separate_wav_spatial(path, num_sources, out_rate="input", **kwargs):
    """``spatial_audio`` for a two-channel PCM wav at any rate -> ``(stems, rate)``: stems [J, 2, n'] ([J + 1, 2, n'] with
    ``residual=True``, the residual last) at ``out_rate`` as in ``separate_wav_ensemble``.  A file that does not have exactly two
    channels is refused."""
    out_rate = _check_out_rate(out_rate)
    unknown = set(kwargs) - _SPATIAL_AUDIO_KEYS
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected spatial_audio's" % sorted(unknown))
    _sources(num_sources)
    _check_spatial_params(kwargs.get("delay", False), kwargs.get("max_delay", 3.0), kwargs.get("p", 1.0))
    _check_flag(kwargs.get("residual", False), "residual")
    _check_fit_kwargs({k: v for k, v in kwargs.items() if k in _FIT_DEFAULTS})
    y, native = audio.load_audio(path, sr=None, mono=False)
    if y.dim() != 2 or y.shape[0] != 2:
        raise ValueError("%s: expected a file with exactly two channels, got %d" % (path, 1 if y.dim() == 1 else y.shape[0]))
    n_file = y.shape[1]
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    return _wav_out(spatial_audio(y, num_sources, **kwargs), kwargs.get("residual", False), native, out_rate, n_file)
