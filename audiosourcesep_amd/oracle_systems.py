"""Oracle source separation systems on the GPU: the upper bounds a separation is judged against.

Replaces the reference's ``oracle_systems.py`` (adapted from sigsep-mus-oracle) with the same names, argument names, defaults and
shapes: ``IBM`` (ideal binary mask), ``IRM`` (ideal ratio mask), ``MWF`` (multichannel Wiener filter) and the two mel-domain masks
``IBM_melspec`` / ``IRM_melspec``; plus the STFT pair they are built on, ``stft`` / ``istft``, in scipy.signal's conventions for
nperseg 2048 (periodic Hann, hop 1024, 1024 zeros on each side, zero-padded to whole frames, scaled by 1 / sum(win) = 1/1024;
T = ceil(n / 1024) + 1 frames).  The kernels are in ``csrc/glowk_oracle.h``:

* the STFT and iSTFT are GEMMs on the exact-fp32 MFMA; float64 input is computed in fp32 and returned as float64 (the reference
  computes in fp64 for fp64 input);
* the masks, the MWF statistics (time means per frequency), the 2 x 2 inversions, the refined PSDs and the gains are fp64;
  every reduction runs in a fixed order, so two calls give bitwise identical results;
* the mel variants are elementwise and follow the reference under numpy 2's promotion bit for bit: the IRM's source sum in the
  sources' dtype, in source order; + eps, the ratio, the threshold and the product in fp64; one rounding to the sources' dtype.

Divergences from the reference, deliberate:

* ``IRM`` reads each source itself (the reference reads ``source.audio``, which fails on arrays);
* ``MWF`` returns every source's estimate (the reference's last loop reuses ``i`` as its channel index, so every estimate lands in
  slot nchan - 1 and the other slots stay zero);
* ``MWF`` refuses nchan != 2 with a ValueError (the reference's 2 x 2 ``invert`` fails with an IndexError) and more than 16
  sources (a kernel bound);
* fewer than 2048 samples are refused (scipy silently shrinks nperseg there).

Kept on purpose: ``MWF``'s normalisation ``R * I / np.trace(R)`` on the [F, 2, 2] array traces axes 0 and 1, i.e. column k of
every R(f) is scaled by 2 / (R(f=0)[0, k] + R(f=1)[1, k]); this quirk comes from sigsep-mus-oracle and changes the estimates.

NumPy in gives NumPy out in the dtype of ``sources``; torch tensors on one CUDA device give tensors there (on the caller's current
stream, with no host join); host tensors are computed on the current device and come back to the host.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .audio import _device

NFFT, HOP = 2048, 1024
NBIN = NFFT // 2 + 1
MWF_MAX_SOURCES = 16
EPS = float(np.finfo(np.float64).eps)


def nframes(n):
    """Frames of ``stft`` for n samples: ceil(n / 1024) + 1."""
    return -(-int(n) // HOP) + 1


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _s(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _tensor(x, what):
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if t.is_complex() or t.dtype == torch.bool:
        raise ValueError("%s: expected a real array, got %s" % (what, t.dtype))
    return t


def _finish(y, like_numpy, host, dtype=None):
    """Result tensor -> what the caller gets: NumPy, a host tensor or the device tensor."""
    if dtype is not None:
        y = y.to(dtype)
    if like_numpy:
        return y.cpu().numpy()
    return y.cpu() if host else y


def _torch_dtype(x):
    return x.dtype if torch.is_tensor(x) else torch.from_numpy(np.zeros(0, dtype=np.asarray(x).dtype)).dtype


def stft(x):
    """real [..., n] -> complex [..., 1025, T] (scipy.signal.stft(x, nperseg=2048)[-1]), computed in fp32: complex64, or
    complex128 for float64 NumPy input."""
    t = _tensor(x, "x")
    if t.dim() < 1 or t.shape[-1] < 1:
        raise ValueError("x: expected [..., n] with n >= 1, got %s" % (tuple(t.shape),))
    dev = _device(t)
    n = t.shape[-1]
    flat = t.to(device=dev, dtype=torch.float32).reshape(-1, n).contiguous()
    T = nframes(n)
    spec = torch.empty((flat.shape[0], NBIN, T, 2), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().glowk_sp_stft(_p(flat), flat.shape[0], n, _p(spec), _s(dev)))
    out = torch.view_as_complex(spec).reshape(tuple(t.shape[:-1]) + (NBIN, T))
    wide = t.dtype == torch.float64 and not torch.is_tensor(x)
    return _finish(out, not torch.is_tensor(x), not t.is_cuda, torch.complex128 if wide else None)


def istft(X, length):
    """complex [..., 1025, T] -> real [..., length] (scipy.signal.istft(X)[1][..., :length]), length <= (T - 1) * 1024; computed
    in fp32: float32, or float64 for complex128 NumPy input."""
    t = X if torch.is_tensor(X) else torch.as_tensor(np.asarray(X))
    if not t.is_complex() or t.dim() < 2 or t.shape[-2] != NBIN or t.shape[-1] < 2:
        raise ValueError("X: expected a complex [..., 1025, T] spectrum with T >= 2, got %s %s" % (t.dtype, tuple(t.shape)))
    T = t.shape[-1]
    length = int(length)
    if not 0 <= length <= (T - 1) * HOP:
        raise ValueError("length must be in [0, (T - 1) * 1024] = [0, %d], got %d" % ((T - 1) * HOP, length))
    dev = _device(t)
    spec = torch.view_as_real(t.to(device=dev, dtype=torch.complex64).reshape(-1, NBIN, T)).contiguous()
    y = torch.empty((spec.shape[0], length), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().glowk_sp_istft(_p(spec), spec.shape[0], T, length, _p(y), _s(dev)))
    y = y.reshape(tuple(t.shape[:-2]) + (length,))
    wide = t.dtype == torch.complex128 and not torch.is_tensor(X)
    return _finish(y, not torch.is_tensor(X), not t.is_cuda, torch.float64 if wide else None)


def _check_pair(mixture, sources):
    """(mixture tensor, sources tensor, NumPy out?, host out?) after the reference's shape conventions are checked."""
    mix, src = _tensor(mixture, "mixture"), _tensor(sources, "sources")
    if mix.dim() != 2:
        raise ValueError("mixture: expected (nsampl, nchan), got shape %s" % (tuple(mix.shape),))
    if src.dim() != 3:
        raise ValueError("sources: expected (nsrc, nsampl, nchan), got shape %s" % (tuple(src.shape),))
    if tuple(src.shape[1:]) != tuple(mix.shape) or src.shape[0] < 1:
        raise ValueError("sources %s do not match mixture %s: expected (nsrc >= 1, nsampl, nchan)" % (tuple(src.shape), tuple(mix.shape)))
    if mix.shape[0] < NFFT:
        raise ValueError("nsampl = %d: at least 2048 samples are needed (nperseg = 2048)" % mix.shape[0])
    if mix.shape[1] < 1:
        raise ValueError("mixture: nchan must be >= 1")
    numpy_out = not (torch.is_tensor(mixture) or torch.is_tensor(sources))
    return mix, src, numpy_out, not (mix.is_cuda or src.is_cuda)


def _spectra(mix, src, dev):
    """The STFT of every channel of the mixture and the sources in one launch: [(1 + nsrc) nchan, 1025, T, 2] (re, im)."""
    nsrc, n, nchan = src.shape
    sig = torch.cat([mix.to(device=dev, dtype=torch.float32).t(),
                     src.to(device=dev, dtype=torch.float32).permute(0, 2, 1).reshape(nsrc * nchan, n)]).contiguous()
    spec = torch.empty((sig.shape[0], NBIN, nframes(n), 2), device=dev, dtype=torch.float32)
    _lib.check(_lib.load().glowk_sp_stft(_p(sig), sig.shape[0], n, _p(spec), _s(dev)))
    return spec


def _estimates(spec, nsrc, n, nchan, dev):
    """iSTFT of the source rows (overwritten with the estimates' spectra) -> (nsrc, nsampl, nchan) float32."""
    y = torch.empty((nsrc * nchan, n), device=dev, dtype=torch.float32)
    _lib.check(_lib.load().glowk_sp_istft(_p(spec[nchan:]), nsrc * nchan, spec.shape[2], n, _p(y), _s(dev)))
    return y.reshape(nsrc, nchan, n).permute(0, 2, 1).contiguous()


def _number(v, what):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be a real number, got %r" % (what, v)) from None
    if np.isnan(v):
        raise ValueError("%s must be a real number, got nan" % what)
    return v


def _masked(mixture, sources, irm, alpha, theta, return_mask):
    mix, src, numpy_out, host = _check_pair(mixture, sources)
    alpha, theta = _number(alpha, "alpha"), _number(theta, "theta")
    if not np.isfinite(alpha):
        raise ValueError("alpha must be finite, got %r" % alpha)
    dev = _device(mix, src)
    nsrc, n, nchan = src.shape
    with torch.cuda.device(dev):
        spec = _spectra(mix, src, dev)
        T = spec.shape[2]
        mask = torch.empty((nsrc, nchan, NBIN, T), device=dev, dtype=torch.uint8) if return_mask else None
        _lib.check(_lib.load().glowk_oracle_mask(_p(spec), nsrc, nchan, T, 1 if irm else 0, alpha, theta, _p(mask), _s(dev)))
        est = _finish(_estimates(spec, nsrc, n, nchan, dev), numpy_out, host, _torch_dtype(sources))
        if return_mask:
            return est, _finish(mask, numpy_out, host)
    return est


def IBM(mixture, sources, alpha=1, theta=0.5, return_mask=False):
    """Ideal binary mask, each channel on its own: mask = |Y_j|^alpha / (eps + |X|^alpha) >= theta, estimate = istft(X mask).
    mixture (nsampl, nchan), sources (nsrc, nsampl, nchan) -> estimates (nsrc, nsampl, nchan); with ``return_mask`` also the
    uint8 mask [nsrc, nchan, 1025, T]."""
    return _masked(mixture, sources, False, alpha, theta, return_mask)


def IRM(mixture, sources, alpha=2):
    """Ideal ratio mask, each channel on its own: mask_j = |Y_j|^alpha / (eps + sum_k |Y_k|^alpha), estimate = istft(X mask_j).
    mixture (nsampl, nchan), sources (nsrc, nsampl, nchan) -> estimates (nsrc, nsampl, nchan)."""
    return _masked(mixture, sources, True, alpha, 0.0, False)


def MWF(mixture, sources):
    """Multichannel Wiener filter (stereo; at most 16 sources) with time-invariant spatial covariances R_j(f), normalised as the
    reference does (see the module docstring), refined PSDs P_j = Re tr(R_j^-1 Y_j Y_j^H) / 2 and the gains
    G_j = P_j R_j (sum_k P_k R_k)^-1.  mixture (nsampl, 2), sources (nsrc, nsampl, 2) -> estimates (nsrc, nsampl, 2), every source's
    estimate in its own slot."""
    mix, src, numpy_out, host = _check_pair(mixture, sources)
    nsrc, n, nchan = src.shape
    if nchan != 2:
        raise ValueError("MWF: only stereo is supported (the 2 x 2 covariance inversion), got nchan = %d" % nchan)
    if nsrc > MWF_MAX_SOURCES:
        raise ValueError("MWF: at most %d sources are supported, got %d" % (MWF_MAX_SOURCES, nsrc))
    dev = _device(mix, src)
    with torch.cuda.device(dev):
        spec = _spectra(mix, src, dev)
        _lib.check(_lib.load().glowk_mwf(_p(spec), nsrc, spec.shape[2], _s(dev)))
        return _finish(_estimates(spec, nsrc, n, nchan, dev), numpy_out, host, _torch_dtype(sources))


def _mel(mixture, sources, irm, theta):
    mix, src = _tensor(mixture, "mixture"), _tensor(sources, "sources")
    if mix.dim() != 3:
        raise ValueError("mixture: expected (nsample, f, t), got shape %s" % (tuple(mix.shape),))
    if src.dim() != 4:
        raise ValueError("sources: expected (nsrc, nsample, f, t), got shape %s" % (tuple(src.shape),))
    if tuple(src.shape[1:]) != tuple(mix.shape) or src.shape[0] < 1:
        raise ValueError("sources %s do not match mixture %s: expected (nsrc >= 1, nsample, f, t)" % (tuple(src.shape), tuple(mix.shape)))
    if src.dtype in (torch.float16, torch.bfloat16) or mix.dtype in (torch.float16, torch.bfloat16):
        raise ValueError("mel variants: half-precision input is not supported (float32, float64 or integers)")
    numpy_out = not (torch.is_tensor(mixture) or torch.is_tensor(sources))
    host = not (mix.is_cuda or src.is_cuda)
    dev = _device(mix, src)
    out_dtype = src.dtype
    work = src.dtype if src.dtype in (torch.float32, torch.float64) else torch.float64   # integers: exact in fp64
    nsrc, n = src.shape[0], mix.numel()
    with torch.cuda.device(dev):
        m = mix.to(device=dev, dtype=torch.float64).contiguous()
        s = src.to(device=dev, dtype=work).contiguous()
        out = torch.empty(s.shape, device=dev, dtype=work)
        _lib.check(_lib.load().glowk_oracle_mel(_p(m), _p(s), nsrc, n, 1 if work == torch.float64 else 0, 1 if irm else 0, theta,
                                                _p(out), _s(dev)))
        return _finish(out, numpy_out, host, out_dtype if out_dtype != work else None)


def IBM_melspec(mixture, sources, theta=0.5):
    """Ideal binary mask on mel spectrograms, elementwise: mixture (nsample, f, t), sources (nsrc, nsample, f, t) ->
    estimates (nsrc, nsample, f, t) = mixture [sources / (eps + mixture) >= theta]."""
    return _mel(mixture, sources, False, _number(theta, "theta"))


def IRM_melspec(mixture, sources, alpha=2):
    """Ideal ratio mask on mel spectrograms, elementwise: estimates = mixture sources / (sum(sources) + eps).  ``alpha`` is
    accepted and ignored, as in the reference."""
    return _mel(mixture, sources, True, 0.0)
