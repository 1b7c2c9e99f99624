"""AuxIVA (Ono 2011) and ILRMA (Kitamura et al. 2016): blind separation of a determined multichannel mixture -- as many sources as
channels -- by *filtering*: one M x M demixing matrix per frequency row, updated by iterative projection.  No masks, so no musical
noise and no sparsity assumption, and the stems (the sources' images in the channels) add up to the mixture.  AuxIVA models a source
by one variance per frame shared by all rows; ILRMA by a low-rank NMF model of its power spectrogram, whose update is one
Itakura-Saito iteration of ``nmf.fit``.  The blind baseline next to ``duet.py``, and the one ``audio.separate_stereo`` should be read
against.  Not in the reference.

Kernels in ``csrc/glowk_iva.h`` (formulas and the error bound in include/glowk.h, design in DESIGN 23):

* ``source_weights``: ``phi_k(t)`` from the frame norms ``r_k(t) = sum_f |y_k(f, t)|^2``, y computed in registers;
* ``covariances``: ``V_k(f) = (1/T) sum_t phi_k x x^H`` with AuxIVA's weights ``[M, T]`` or ILRMA's low-rank model;
* ``ip_update``: the M sequential row updates of every ``W_f``;
* ``power`` / ``normalize``: ILRMA's float32 power planes and its scale normalisation;
* ``inverse`` / ``demix`` / ``images``: ``W^-1``, ``Y = W X`` and the minimal-distortion images ``W^-1[m, k] y_k``;
* ``auxiva`` / ``ilrma`` (``ilrma_fit``): the loops, one C call each (the covariances are never stored there: the projection runs in their launch);
* ``iva_audio`` / ``separate_wav_iva``: the audio and wav paths.

X is ``[M, R, T]`` or ``[N, M, R, T]`` complex, ``2 <= M <= 4``, ``M <= T <= 32768``, ``R <= 4096``; W is ``[.., R, M, M]`` complex128
with row k of ``W_f`` the conjugated demixing vector of source k.  Everything after the load of X is fp64 in a fixed order: results
are bitwise reproducible and a batch gives what its signals give alone.

Conventions as in ``duet.py``: numpy or torch in, tensors on the GPU the input lives on out, ValueError for bad arguments before the
library is loaded, no host synchronisation.
"""
import numpy as np
import torch

from . import _lib, audio, nmf
from .audio import _p, _s
from .repet import MAX_ELEMENTS, MAX_FRAMES, MAX_ROWS, MAX_SIGNALS, _check_flag, _check_range_int

MIN_CHANNELS, MAX_CHANNELS, MAX_ITER = 2, 4, 100000
MODELS = ("laplace", "gauss")
METHODS = ("auxiva", "ilrma")


def _check_model(model):
    if not isinstance(model, str) or model not in MODELS:
        raise ValueError("model: expected 'laplace' or 'gauss', got %r" % (model,))
    return MODELS.index(model)


def _check_mix(X, what="X"):
    """[M, R, T] or [N, M, R, T] complex within the kernels' ranges, as a tensor where it is."""
    x = X if torch.is_tensor(X) else torch.as_tensor(np.asarray(X))
    if x.dim() not in (3, 4) or not MIN_CHANNELS <= x.shape[-3] <= MAX_CHANNELS or not 1 <= x.shape[-2] <= MAX_ROWS \
            or not x.shape[-3] <= x.shape[-1] <= MAX_FRAMES or (x.dim() == 4 and x.shape[0] > MAX_SIGNALS) or x.numel() > MAX_ELEMENTS:
        raise ValueError("%s: expected [M, rows, T] or [N, M, rows, T] with N <= %d, 2 <= M <= 4, 1 <= rows <= %d, M <= T <= %d and at most "
                         "2^31 - 1 elements, got %s" % (what, MAX_SIGNALS, MAX_ROWS, MAX_FRAMES, tuple(x.shape)))
    if not x.is_complex():
        raise ValueError("%s: expected the complex STFT of M channels, got %s" % (what, x.dtype))
    return x


def _dims(x):
    """x [.., M, R, T] -> (lead, nsig, M, R, T)."""
    M, R, T = x.shape[-3:]
    return tuple(x.shape[:-3]), (x.shape[0] if x.dim() == 4 else 1), M, R, T


def _check_w(W, x, what="W"):
    """The demixing matrices [.., R, M, M] that go with x, complex, as a tensor where they are."""
    lead, _, M, R, _ = _dims(x)
    w = W if torch.is_tensor(W) else torch.as_tensor(np.asarray(W))
    if tuple(w.shape) != lead + (R, M, M) or not w.is_complex():
        raise ValueError("%s: expected complex demixing matrices %s for X %s, got %s %s" % (what, lead + (R, M, M), tuple(x.shape), w.dtype, tuple(w.shape)))
    return w


def _pair(X, W):
    """(x complex64, w complex128), contiguous on one GPU."""
    x = _check_mix(X)
    w = _check_w(W, x)
    dev = audio._device(x, w)
    return x.to(device=dev, dtype=torch.complex64).contiguous(), w.to(device=dev, dtype=torch.complex128).contiguous()


def _own(t, src):
    """A tensor the kernels may overwrite: t itself if the conversion already copied, else a clone."""
    return t.clone() if torch.is_tensor(src) and t.data_ptr() == src.data_ptr() else t


def _work(nbytes, dev):
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)


def _identity(x, dev):
    lead, _, M, R, _ = _dims(x)
    return torch.eye(M, dtype=torch.complex128, device=dev).expand(lead + (R, M, M)).contiguous()


def _check_factors(basis, act, x):
    """ILRMA's factors for x: basis [.., M, R, K] and act [.., M, K, T], real; -> (basis, act, K) as tensors where they are."""
    lead, nsig, M, R, T = _dims(x)
    b = basis if torch.is_tensor(basis) else torch.as_tensor(np.asarray(basis))
    a = act if torch.is_tensor(act) else torch.as_tensor(np.asarray(act))
    if b.is_complex() or a.is_complex() or b.dim() != len(lead) + 3 or not 1 <= b.shape[-1] <= nmf.MAX_COMPONENTS \
            or tuple(b.shape[:-1]) != lead + (M, R) or tuple(a.shape) != lead + (M, b.shape[-1], T):
        raise ValueError("basis, act: expected real %s + (K,) and %s with 1 <= K <= %d for X %s, got %s and %s"
                         % (lead + (M, R), lead + (M, "K", T), nmf.MAX_COMPONENTS, tuple(x.shape), tuple(b.shape), tuple(a.shape)))
    _check_factor_sizes(nsig, M, R, T, b.shape[-1])
    return b, a, b.shape[-1]


def _check_factor_sizes(nsig, M, R, T, K):
    if nsig * M > MAX_SIGNALS or nsig * M * R * K > MAX_ELEMENTS or nsig * M * K * T > MAX_ELEMENTS:
        raise ValueError("ilrma: expected N * M <= %d and factors of at most 2^31 - 1 elements each" % MAX_SIGNALS)


def init(X):
    """The starting point: the identity in every row, complex128 [.., R, M, M] on X's GPU."""
    x = _check_mix(X)
    return _identity(x, audio._device(x))


def source_weights(X, W, model="laplace"):
    """AuxIVA's weights ``phi`` [.., M, T] float64: with ``r_k(t) = sum_f |y_k(f, t)|^2``, ``1 / max(sqrt(r), 2^-40)`` for 'laplace'
    and ``1 / max(r / R, 2^-40)`` for 'gauss'.  ``glowk_iva_weights``: two launches, y in registers."""
    model = _check_model(model)
    x, w = _pair(X, W)
    lead, nsig, M, R, T = _dims(x)
    phi = torch.empty(lead + (M, T), dtype=torch.float64, device=x.device)
    if nsig:
        lib = _lib.load()
        nbytes = lib.glowk_iva_workspace_bytes(nsig, M, R, T)
        work = _work(nbytes, x.device)
        _lib.check(lib.glowk_iva_weights(_p(x), _p(w), nsig, M, R, T, model, _p(phi), _p(work), nbytes, _s(x)))
    return phi


def covariances(X, phi=None, factors=None):
    """The weighted covariances ``V_k(f) = (1/T) sum_t phi_k x(f, t) x(f, t)^H`` -> complex128 [.., R, M, M, M] (row, source k, then
    the Hermitian matrix, both triangles).  ``phi`` [.., M, T] are AuxIVA's weights; ``factors = (basis [.., M, R, K], act [.., M, K, T])``
    gives ILRMA's ``1 / max(sum_l basis_k(f, l) act_k(l, t), 2^-40)``, evaluated in registers.  ``glowk_iva_covariances``: one launch."""
    x = _check_mix(X)
    lead, nsig, M, R, T = _dims(x)
    if (phi is None) == (factors is None):
        raise ValueError("covariances: expected either phi or factors")
    if phi is not None:
        ph = phi if torch.is_tensor(phi) else torch.as_tensor(np.asarray(phi))
        if ph.is_complex() or tuple(ph.shape) != lead + (M, T):
            raise ValueError("phi: expected real weights %s, got %s %s" % (lead + (M, T), ph.dtype, tuple(ph.shape)))
        dev = audio._device(x, ph)
        ph, b, a, K = ph.to(device=dev, dtype=torch.float64).contiguous(), None, None, 0
    else:
        if not isinstance(factors, (tuple, list)) or len(factors) != 2:
            raise ValueError("factors: expected (basis, act), got %r" % (type(factors).__name__,))
        b, a, K = _check_factors(factors[0], factors[1], x)
        dev = audio._device(x, b, a)
        ph, b, a = None, b.to(device=dev, dtype=torch.float32).contiguous(), a.to(device=dev, dtype=torch.float32).contiguous()
    x = x.to(device=dev, dtype=torch.complex64).contiguous()
    V = torch.empty(lead + (R, M, M, M), dtype=torch.complex128, device=dev)
    if nsig:
        _lib.check(_lib.load().glowk_iva_covariances(_p(x), nsig, M, R, T, _p(ph), _p(b), _p(a), K, _p(V), _s(x)))
    return V


def ip_update(W, V):
    """Iterative projection: for k = 0 .. M - 1 in order, ``u = (W_f V_k(f))^-1 e_k``, ``d = u^H V_k(f) u``, row k of ``W_f`` becomes
    ``(u / sqrt(d))^H`` where u and d are finite and d > 0 (else it stays) -> W', a new tensor.  W [.., R, M, M], V [.., R, M, M, M].
    ``glowk_iva_ip_update``: one launch."""
    w = W if torch.is_tensor(W) else torch.as_tensor(np.asarray(W))
    v = V if torch.is_tensor(V) else torch.as_tensor(np.asarray(V))
    if not w.is_complex() or w.dim() not in (3, 4) or w.shape[-1] != w.shape[-2] or not MIN_CHANNELS <= w.shape[-1] <= MAX_CHANNELS \
            or not 1 <= w.shape[-3] <= MAX_ROWS or (w.dim() == 4 and w.shape[0] > MAX_SIGNALS):
        raise ValueError("W: expected complex [rows, M, M] or [N, rows, M, M] with 2 <= M <= 4, got %s %s" % (w.dtype, tuple(w.shape)))
    M = w.shape[-1]
    if not v.is_complex() or tuple(v.shape) != tuple(w.shape[:-2]) + (M, M, M):
        raise ValueError("V: expected complex %s, got %s %s" % (tuple(w.shape[:-2]) + (M, M, M), v.dtype, tuple(v.shape)))
    dev = audio._device(w, v)
    wd = _own(w.to(device=dev, dtype=torch.complex128).contiguous(), W)
    v = v.to(device=dev, dtype=torch.complex128).contiguous()
    nsig = w.shape[0] if w.dim() == 4 else 1
    if nsig:
        _lib.check(_lib.load().glowk_iva_ip_update(_p(wd), _p(v), nsig, M, w.shape[-3], _s(wd)))
    return wd


def power(X, W):
    """ILRMA's NMF input: ``P_k = |y_k|^2`` in fp64, rounded once to float32 -> [.., M, R, T].  ``glowk_iva_power``."""
    x, w = _pair(X, W)
    lead, nsig, M, R, T = _dims(x)
    P = torch.empty(lead + (M, R, T), dtype=torch.float32, device=x.device)
    if nsig:
        _lib.check(_lib.load().glowk_iva_power(_p(x), _p(w), nsig, M, R, T, _p(P), _s(x)))
    return P


def normalize(X, W, basis):
    """ILRMA's scale normalisation: ``lambda_k = sqrt(mean_{f,t} |y_k|^2)``; where it is finite and positive row k of every ``W_f`` is
    divided by it and ``basis_k`` by its square (rounded once to float32) -> ``(W', basis')``, new tensors.  ``glowk_iva_normalize``."""
    x = _check_mix(X)
    w = _check_w(W, x)
    lead, nsig, M, R, T = _dims(x)
    b = basis if torch.is_tensor(basis) else torch.as_tensor(np.asarray(basis))
    if b.is_complex() or b.dim() != len(lead) + 3 or tuple(b.shape[:-1]) != lead + (M, R) or not 1 <= b.shape[-1] <= nmf.MAX_COMPONENTS:
        raise ValueError("basis: expected real %s + (K,) with 1 <= K <= %d, got %s" % (lead + (M, R), nmf.MAX_COMPONENTS, tuple(b.shape)))
    K = b.shape[-1]
    _check_factor_sizes(nsig, M, R, T, K)
    dev = audio._device(x, w, b)
    x = x.to(device=dev, dtype=torch.complex64).contiguous()
    w = _own(w.to(device=dev, dtype=torch.complex128).contiguous(), W)
    bd = _own(b.to(device=dev, dtype=torch.float32).contiguous(), basis)
    if nsig:
        lib = _lib.load()
        nbytes = lib.glowk_iva_workspace_bytes(nsig, M, R, T)
        work = _work(nbytes, x.device)
        _lib.check(lib.glowk_iva_normalize(_p(x), _p(w), _p(bd), nsig, M, R, T, K, _p(work), nbytes, _s(x)))
    return w, bd


def inverse(W):
    """``W_f^-1`` in fp64 -> complex128 like W; a row whose inverse is not finite gets an all-zero matrix.  ``glowk_iva_inverse``."""
    w = W if torch.is_tensor(W) else torch.as_tensor(np.asarray(W))
    if not w.is_complex() or w.dim() not in (3, 4) or w.shape[-1] != w.shape[-2] or not MIN_CHANNELS <= w.shape[-1] <= MAX_CHANNELS \
            or not 1 <= w.shape[-3] <= MAX_ROWS or (w.dim() == 4 and w.shape[0] > MAX_SIGNALS):
        raise ValueError("W: expected complex [rows, M, M] or [N, rows, M, M] with 2 <= M <= 4, got %s %s" % (w.dtype, tuple(w.shape)))
    w = w.to(device=audio._device(w), dtype=torch.complex128).contiguous()
    return _inverse(w)


def _inverse(w):
    out = torch.empty_like(w)
    nsig = w.shape[0] if w.dim() == 4 else 1
    if nsig:
        _lib.check(_lib.load().glowk_iva_inverse(_p(w), nsig, w.shape[-1], w.shape[-3], _p(out), _s(w)))
    return out


def demix(X, W):
    """``Y = W X``: ``y_k(f, t) = sum_m W_f[k, m] X[m, f, t]`` in fp64 -> complex64 like X.  ``glowk_iva_demix``: one pass."""
    x, w = _pair(X, W)
    _, nsig, M, R, T = _dims(x)
    y = torch.empty_like(x)
    if nsig:
        _lib.check(_lib.load().glowk_iva_demix(_p(x), _p(w), nsig, M, R, T, _p(y), _s(x)))
    return y


def _images(x, w, want_y=False):
    lead, nsig, M, R, T = _dims(x)
    if nsig * M * M * R * T > MAX_ELEMENTS:
        raise ValueError("images: N * M * M * rows * T must be at most 2^31 - 1")
    img = torch.empty(lead + (M, M, R, T), dtype=torch.complex64, device=x.device)
    y = torch.empty_like(x) if want_y else None
    if nsig:
        winv = _inverse(w)
        _lib.check(_lib.load().glowk_iva_images(_p(x), _p(w), _p(winv), nsig, M, R, T, _p(y), _p(img), _s(x)))
    return img, y


def images(X, W, return_demixed=False):
    """The sources' images in the channels, the minimal-distortion projection: ``img[k, m, f, t] = (W_f^-1)[m, k] y_k(f, t)`` with
    ``y_k`` the complex64 value ``demix`` returns -> complex64 [.., M, M, R, T] (source, then channel, the layout of DUET's stems).
    The images of one cell add up to X; a row whose fp64 inverse is not finite gets zero images.  ``glowk_iva_inverse`` and
    ``glowk_iva_images``: one pass over X.  ``return_demixed`` adds Y."""
    want = _check_flag(return_demixed, "return_demixed")
    x, w = _pair(X, W)
    img, y = _images(x, w, want)
    return (img, y) if want else img


def _start(X, W):
    x = _check_mix(X)
    if W is None:
        x = x.to(device=audio._device(x), dtype=torch.complex64).contiguous()
        return x, _identity(x, x.device)
    x, w = _pair(X, W)
    return x, _own(w, W)


def auxiva(X, n_iter=20, model="laplace", W=None, return_model=False):
    """AuxIVA on X [M, R, T] or [N, M, R, T] -> the images, complex64 [.., M, M, R, T] (source, then channel).  ``n_iter`` iterations
    (weights, covariances, iterative projection; three launches each, all in one C call, ``glowk_auxiva_fit``) from ``W`` (the identity
    by default), then ``images``.  ``return_model`` adds a dict with ``W`` and the demixed ``Y``."""
    n_iter = _check_range_int(n_iter, "n_iter", 0, MAX_ITER)
    model = _check_model(model)
    return_model = _check_flag(return_model, "return_model")
    x, w = _start(X, W)
    lead, nsig, M, R, T = _dims(x)
    if nsig * M * M * R * T > MAX_ELEMENTS:
        raise ValueError("X: N * M * M * rows * T must be at most 2^31 - 1")
    if nsig and n_iter:
        lib = _lib.load()
        nbytes = lib.glowk_iva_workspace_bytes(nsig, M, R, T)
        work = _work(nbytes, x.device)
        _lib.check(lib.glowk_auxiva_fit(_p(x), _p(w), nsig, M, R, T, model, n_iter, _p(work), nbytes, _s(x)))
    img, y = _images(x, w, return_model)
    return (img, dict(W=w, Y=y)) if return_model else img


def init_factors(P, n_components, seed=0):
    """ILRMA's starting factors for power planes P [.., M, R, T]: ``(basis [.., M, R, K], act [.., M, K, T])``, for every signal of a
    batch exactly ``nmf.init(P[n], K, seed)`` (the M planes of one signal as ``nmf``'s batch), so a batch starts where its signals start
    alone."""
    K = _check_range_int(n_components, "n_components", 1, nmf.MAX_COMPONENTS)
    seed = nmf._check_seed(seed)
    p = nmf._nonneg(P, "P", (3, 4))
    M, R, T = p.shape[-3:]
    lead = tuple(p.shape[:-3])
    p = p.to(device=audio._device(p), dtype=torch.float32)
    lib = _lib.load()
    b = torch.empty((M, R, K), dtype=torch.float32, device=p.device)
    a = torch.empty((M, K, T), dtype=torch.float32, device=p.device)
    for t, step in ((b, 0), (a, 1)):
        if t.numel() and p.numel():
            _lib.check(lib.glowk_random(_p(t), t.numel(), seed, step, nmf.NMF_STREAM, 1, 0, _s(t)))
    scale = nmf._scale(p, K) if p.numel() else p.new_zeros(lead + (M, 1, 1))
    return b * scale, a * scale


def ilrma_fit(X, W, basis, act, n_iter=1):
    """``n_iter`` ILRMA iterations from the state ``(W, basis, act)`` -> ``(W', basis', act')``, new tensors; the inputs stay.  basis
    [.., M, R, K] and act [.., M, K, T] are real.  One iteration: ``P = power(X, W)``; one Itakura-Saito iteration of ``nmf.fit`` on
    P; the covariances with the factors' weights and the iterative projection; ``normalize``.  All ``n_iter`` in one C call
    (``glowk_ilrma_fit``, nine launches per iteration)."""
    n_iter = _check_range_int(n_iter, "n_iter", 0, MAX_ITER)
    xc = _check_mix(X)
    wc = _check_w(W, xc)
    fb, fa, K = _check_factors(basis, act, xc)
    _, nsig, M, R, T = _dims(xc)
    dev = audio._device(xc, wc, fb, fa)
    x = xc.to(device=dev, dtype=torch.complex64).contiguous()
    w = _own(wc.to(device=dev, dtype=torch.complex128).contiguous(), W)
    b = _own(fb.to(device=dev, dtype=torch.float32).contiguous(), basis)
    a = _own(fa.to(device=dev, dtype=torch.float32).contiguous(), act)
    if nsig and n_iter:
        lib = _lib.load()
        nbytes = lib.glowk_ilrma_workspace_bytes(nsig, M, R, T, K)
        work = _work(nbytes, dev)
        _lib.check(lib.glowk_ilrma_fit(_p(x), _p(w), _p(b), _p(a), nsig, M, R, T, K, n_iter, _p(work), nbytes, _s(x)))
    return w, b, a


def ilrma(X, n_components=4, n_iter=50, seed=0, W=None, return_model=False):
    """ILRMA on X [M, R, T] or [N, M, R, T] -> the images, complex64 [.., M, M, R, T].  Every source has ``n_components`` NMF
    components.  The factors start from ``init_factors(power(X, W), n_components, seed)``: ``nmf.init`` on the float32 planes
    ``|y_k|^2`` of the starting W (the identity by default), which are the channel planes ``|X_m|^2`` for the identity.  Then
    ``ilrma_fit`` for ``n_iter`` iterations and ``images``.  ``return_model`` adds a dict with ``W``, ``Y``, ``basis`` and ``act``."""
    K = _check_range_int(n_components, "n_components", 1, nmf.MAX_COMPONENTS)
    n_iter = _check_range_int(n_iter, "n_iter", 0, MAX_ITER)
    seed = nmf._check_seed(seed)
    return_model = _check_flag(return_model, "return_model")
    xc = _check_mix(X)
    _, nsig, M, R, T = _dims(xc)
    if nsig * M * M * R * T > MAX_ELEMENTS:
        raise ValueError("X: N * M * M * rows * T must be at most 2^31 - 1")
    _check_factor_sizes(nsig, M, R, T, K)
    x, w = _start(xc, W)
    b, a = init_factors(power(x, w), K, seed)
    w, b, a = ilrma_fit(x, w, b, a, n_iter)
    img, y = _images(x, w, return_model)
    return (img, dict(W=w, Y=y, basis=b, act=a)) if return_model else img


_IVA_AUDIO_DEFAULTS = dict(method="auxiva", n_iter=None, model="laplace", n_components=4, seed=0)


def _check_iva_audio_params(method, n_iter, model, n_components, seed):
    if not isinstance(method, str) or method not in METHODS:
        raise ValueError("method: expected 'auxiva' or 'ilrma', got %r" % (method,))
    if n_iter is not None:
        _check_range_int(n_iter, "n_iter", 0, MAX_ITER)
    _check_model(model)
    _check_range_int(n_components, "n_components", 1, nmf.MAX_COMPONENTS)
    nmf._check_seed(seed)


def iva_audio(y, method="auxiva", n_iter=None, model="laplace", n_components=4, seed=0):
    """Blind separation of M channels of 16 kHz audio [M, n], 2 <= M <= 4, n > 1024 -> stems [M, M, n] aligned with y: stem k is the
    image of source k in the M channels, and the stems add up to y (up to the STFT's own round trip).  One STFT of the whole signal
    (``audio.mel_frames(return_stft=True)``), ``auxiva`` (``n_iter`` 20 by default, ``model``) or ``ilrma`` (50, ``n_components``,
    ``seed``) on it, one ``audio.istft`` of the images, trimmed to n samples.  At most 32 768 frames."""
    _check_iva_audio_params(method, n_iter, model, n_components, seed)
    t = audio._tensor(y, "y")
    if t.dim() != 2 or not MIN_CHANNELS <= t.shape[0] <= MAX_CHANNELS:
        raise ValueError("y: expected two to four channels [M, n], got %s" % (tuple(t.shape),))
    x = audio._long_audio(t)
    M, n = x.shape
    if 1 + -(-n // audio.HOP) > MAX_FRAMES:
        raise ValueError("y: expected at most %d frames (%d samples), got %d samples" % (MAX_FRAMES, (MAX_FRAMES - 2) * audio.HOP, n))
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [M, 1025, F]
    if method == "auxiva":
        img = auxiva(X, 20 if n_iter is None else n_iter, model)
    else:
        img = ilrma(X, n_components, 50 if n_iter is None else n_iter, seed)
    return audio.istft(img)[..., :n].contiguous()                                        # [M, M, n]


def separate_wav_iva(path, out_rate="input", **kwargs):
    """``iva_audio`` for a PCM wav with two to four channels at any rate -> ``(stems, rate)``, the wrapper ``duet.separate_wav_duet``
    is around ``duet_audio``: stems [M, M, n'] at ``out_rate``: 'input' (the file's rate and exactly its sample count), an integer
    rate, or None (16 kHz).  ``kwargs`` are ``iva_audio``'s keyword arguments; any other is refused before the file is opened.  A
    file with one channel or more than four is refused."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    unknown = set(kwargs) - set(_IVA_AUDIO_DEFAULTS)
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected iva_audio's" % sorted(unknown))
    _check_iva_audio_params(**dict(_IVA_AUDIO_DEFAULTS, **kwargs))
    y, native = audio.load_audio(path, sr=None, mono=False)
    if y.dim() != 2 or not MIN_CHANNELS <= y.shape[0] <= MAX_CHANNELS:
        raise ValueError("%s: expected a file with two to four channels, got %d" % (path, 1 if y.dim() == 1 else y.shape[0]))
    n_file = y.shape[1]
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    stems = audio.resample(iva_audio(y, **kwargs), audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate
