"""BSS Eval v4 on the GPU: SDR / ISR / SIR / SAR of separated signals against their references.

Replaces the reference's ``bsseval_v4.py`` (sigsep's BSS Eval v4 with the v3 wrappers) with the same public surface: ``bss_eval``,
``bss_eval_sources``, ``bss_eval_sources_framewise``, ``bss_eval_images``, ``bss_eval_images_framewise``; same argument names,
defaults, errors and return shapes.  Inputs are numpy arrays or torch tensors (host or one CUDA device) of shape (nsampl),
(nsrc, nsampl) or (nsrc, nsampl, nchan) (``np.atleast_3d``); every kernel computes in fp64 (``csrc/glowk_bsseval.h``):

* ``glowk_bss_xcorr``: the linear lagged correlations of reference x reference (G, block Toeplitz) and reference x estimate (D)
  over each window's slices, by direct sums (the reference uses zero-padded FFTs: same values to rounding);
* ``glowk_bss_solve``: (G + eps I) C = D by a batched Cholesky, one workgroup per system: per filter window one system over all
  references (C) and one per reference alone (Cj).  The reference solves by LU and falls back to ``lstsq`` on LinAlgError; here a
  pivot that is not positive and finite marks the system, and the host redoes exactly those systems with fp64
  ``torch.linalg.lstsq`` on the CPU from the device's correlations (``last_fallbacks()`` counts them).  An ill-conditioned G
  can make the two solvers choose different systems to redo;
* ``glowk_bss_project``: the FIR projections of each window's reference slices and the energy sums of ``_bss_crit``.

The dB conversion, NaN / inf handling and the permutation choice run on the host in fp64.  Bounds: filters_len <= 512 and
M = nsrc * nchan * filters_len <= 2048 (the Cholesky workspace is M^2 doubles per system, 8 MB at M = 1024; systems run in
chunks of at most 2 GiB of workspace).  Filters are computed per window with ``framewise_filters`` (v3), else once over the
whole signal (v4).  A window where a reference or an estimate is silent gives NaN, as in the reference.
"""
import ctypes
import itertools
import warnings

import numpy as np
import torch

from . import _lib

MAX_SOURCES = 100
MAX_FILTERS_LEN = 512
MAX_M = 2048
EPS = np.finfo(np.float64).eps
_fallbacks = 0


def last_fallbacks():
    """Number of systems the last call redid by least squares on the host (a Cholesky pivot was not positive and finite)."""
    return _fallbacks


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _any_source_silent(sources):
    """True if any source is all zeros after summing its channels (bsseval_v4.py:73-76)."""
    return np.any(np.all(np.sum(sources, axis=tuple(range(2, sources.ndim))) == 0, axis=1))


def validate(reference_sources, estimated_sources):
    """The reference's input checks (bsseval_v4.py:13-71): ValueError on a shape mismatch, ndim > 3, a silent source or too
    many sources; a warning for empty inputs."""
    if reference_sources.shape != estimated_sources.shape:
        raise ValueError("The shape of estimated sources and the true sources should match. reference_sources.shape = {}, "
                         "estimated_sources.shape = {}".format(reference_sources.shape, estimated_sources.shape))
    if reference_sources.ndim > 3 or estimated_sources.ndim > 3:
        raise ValueError("The number of dimensions is too high (must be less than 3). reference_sources.ndim = {}, "
                         "estimated_sources.ndim = {}".format(reference_sources.ndim, estimated_sources.ndim))
    if reference_sources.size == 0:
        warnings.warn("reference_sources is empty, should be of size (nsrc, nsample, nchan). sdr, isr sir, sar, and perm "
                      "will all be empty np.ndarrays")
    elif _any_source_silent(reference_sources):
        raise ValueError("All the reference sources should be non-silent (not all-zeros), but at least one of the reference "
                         "sources is all 0s, which introduces ambiguity to the evaluation.")
    if estimated_sources.size == 0:
        warnings.warn("estimated_sources is empty, should be of size (nsrc, nsample, nchan).  sdr, isr, sir, sar, and perm "
                      "will all be empty np.ndarrays")
    elif _any_source_silent(estimated_sources):
        raise ValueError("All the estimated sources should be non-silent (not all-zeros), but at least one of the estimated "
                         "sources is all 0s.")
    if estimated_sources.shape[0] > MAX_SOURCES or reference_sources.shape[0] > MAX_SOURCES:
        raise ValueError("The supplied matrices should be of shape (nsrc, nsampl, nchan) but reference_sources.shape[0] = {} "
                         "and estimated_sources.shape[0] = {} which is greater than bsseval.MAX_SOURCES = {}."
                         .format(reference_sources.shape[0], estimated_sources.shape[0], MAX_SOURCES))


def framing(window, hop, length):
    """The windows of the reference's ``Framing`` (bsseval_v4.py:382-418) as (start, stop) pairs: nwin = floor((length - window +
    hop) / hop) if window < length else 1; start and stop floored, inf / nan start -> 0, stop -> length."""
    nwin = int(np.floor((length - window + hop) / hop)) if window < length else 1
    out = []
    for cur in range(nwin):
        start = cur * hop
        if np.isnan(start) or np.isinf(start):
            start = 0
        stop = min(cur * hop + window, length)
        if np.isnan(stop) or np.isinf(stop):
            stop = length
        out.append((int(np.floor(start)), int(np.floor(stop))))
    return out


def _safe_db(num, den):
    if den == 0:
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10 * np.log10(np.float64(num) / np.float64(den))


def _crit(e, sources_version):
    """_bss_crit (bsseval_v4.py:584-608) from the device's energies (glowk_bss_project)."""
    if sources_version:
        return _safe_db(e[3], e[7]), np.nan, _safe_db(e[3], e[4]), _safe_db(e[5], e[6])
    return _safe_db(e[0], e[1]), _safe_db(e[0], e[2]), _safe_db(e[3], e[4]), _safe_db(e[5], e[6])


def _host_array(x):
    if torch.is_tensor(x):
        if x.is_complex():
            raise ValueError("bss_eval: complex input")
        return x.detach().cpu().numpy()
    x = np.asarray(x)
    if np.iscomplexobj(x):
        raise ValueError("bss_eval: complex input")
    return x


def _device(*xs):
    """The CUDA device of the inputs, None if they are all on the host; inputs on two GPUs are refused (as audio._device does)."""
    devs = {x.device for x in xs if torch.is_tensor(x) and x.is_cuda}
    if len(devs) > 1:
        raise ValueError("inputs on different devices: %s" % sorted(str(d) for d in devs))
    return devs.pop() if devs else None


def lstsq_systems(corr, P, L, systems, nchan_sys):
    """Least-squares distortion filters (np.linalg.lstsq(G, D) of bsseval_v4.py:545-548, no eps) for the given systems
    [(window, p0)], assembled from the correlations corr [nwin][2 P^2][L] the way glowk_bss_solve assembles them; fp64
    torch.linalg.lstsq (gelsd) on the CPU.  Returns [len(systems), P, nchan_sys * L] in glowk_bss_solve's layout."""
    M = nchan_sys * L
    out = np.empty((len(systems), P, M))
    d = np.arange(L)[:, None] - np.arange(L)[None, :]
    for k, (w, p0) in enumerate(systems):
        c = corr[w]
        G = np.empty((M, M))
        D = np.empty((M, P))
        for pl in range(nchan_sys):
            p = p0 + pl
            for ql in range(nchan_sys):
                q = p0 + ql
                G[pl * L:(pl + 1) * L, ql * L:(ql + 1) * L] = np.where(d >= 0, c[p * P + q][np.abs(d)], c[q * P + p][np.abs(d)])
            for e in range(P):
                D[pl * L:(pl + 1) * L, e] = c[P * P + p * P + e]
        sol = torch.linalg.lstsq(torch.from_numpy(G), torch.from_numpy(D), driver="gelsd").solution
        out[k] = sol.numpy().T
    return out


def bss_eval(reference_sources, estimated_sources, window=2 * 44100, hop=1.5 * 44100, compute_permutation=False, filters_len=512,
             framewise_filters=False, bsseval_sources_version=False):
    """BSS Eval version 4 (bsseval_v4.py:79-301) on the GPU -> (sdr, isr, sir, sar, perm), float64 arrays of shape
    (nsrc, nwin) and perm int64 (nsrc, 1), or (nsrc, nwin) with ``framewise_filters``.  ``window`` / ``hop`` may be floats or
    inf (a window of at least the signal's length is one window over the whole signal)."""
    global _fallbacks
    _fallbacks = 0
    dev = _device(reference_sources, estimated_sources)
    est = np.atleast_3d(_host_array(estimated_sources))
    ref = np.atleast_3d(_host_array(reference_sources))
    validate(ref, est)
    if ref.size == 0 or est.size == 0:
        return np.array([]), np.array([]), np.array([]), np.array([]), np.array([])
    nsrc, nsampl, nchan = est.shape
    if filters_len != int(filters_len) or not 1 <= int(filters_len) <= MAX_FILTERS_LEN:
        raise ValueError("filters_len must be an integer in [1, %d], got %r" % (MAX_FILTERS_LEN, filters_len))
    L = int(filters_len)
    P = nsrc * nchan
    if P * L > MAX_M:
        raise ValueError("nsrc * nchan * filters_len = %d * %d * %d = %d exceeds the supported M <= %d"
                         % (nsrc, nchan, L, P * L, MAX_M))
    if compute_permutation:
        cands = np.array(list(itertools.permutations(list(range(nsrc)))))
    else:
        cands = np.array(np.arange(nsrc))[None, :]
    wins = framing(window, hop, nsampl)
    nwin = len(wins)

    # silent windows (_any_source_silent of each slice): counts of samples whose channel sum is non-zero
    def counts(x):
        return np.concatenate([np.zeros((nsrc, 1), np.int64), np.cumsum(np.sum(x, axis=2) != 0, axis=1)], axis=1)
    cr, ce = counts(ref), counts(est)
    live = [t for t, (s, e) in enumerate(wins)
            if not (np.any(cr[:, max(e, s)] - cr[:, s] == 0) or np.any(ce[:, max(e, s)] - ce[:, s] == 0))]

    s_r = np.full((4, nsrc, nsrc, nwin), np.nan)
    if live:
        corr_wins = [wins[t] for t in live] if framewise_filters else [(0, nsampl)]
        cw_of = {t: (i if framewise_filters else 0) for i, t in enumerate(live)}
        items, where = [], []
        for t in live:
            s, e = wins[t]
            for jtrue in range(nsrc):
                for jest in dict.fromkeys(cands[:, jtrue].tolist()):     # each (jtrue, jest) pair once, as `done` does
                    items.append((s, e, jtrue, int(jest), cw_of[t], cw_of[t] * nsrc + jtrue))
                    where.append((jtrue, int(jest), t))
        dev = dev if dev is not None else torch.device("cuda", torch.cuda.current_device())
        energies = _run(dev, ref, est, L, corr_wins, items, max(wins[t][1] - wins[t][0] for t in live))
        for (jtrue, jest, t), en in zip(where, energies):
            s_r[:, jtrue, jest, t] = _crit(en, bsseval_sources_version)

    # the best ordering (bsseval_v4.py:278-301), NaN propagation as np.mean / np.argmax give it
    SDR, ISR, SIR, SAR = range(4)
    if framewise_filters:
        mean_sir = np.empty((len(cands), nwin))
        axis_mean = 0
    else:
        mean_sir = np.empty((len(cands), 1))
        axis_mean = None
    dum = np.arange(nsrc)
    for i, perm in enumerate(cands):
        mean_sir[i] = np.mean(s_r[SIR, dum, perm, :], axis=axis_mean)
    popt = cands[np.argmax(mean_sir, axis=0)].T
    if not framewise_filters:
        result = s_r[:, dum, popt[:, 0], :]
    else:
        result = np.empty((4, nsrc, nwin))
        for m, t in itertools.product(range(4), range(nwin)):
            result[m, :, t] = s_r[m, dum, popt[:, t], t]
    return result[SDR], result[ISR], result[SIR], result[SAR], popt


def _run(dev, ref, est, L, corr_wins, items, max_len):
    """The three device calls for one evaluation -> energies [len(items)][8] (numpy); one synchronisation, a second one only
    when a system needs the least-squares fallback."""
    global _fallbacks
    lib = _lib.load()
    nsrc, nsampl, nchan = est.shape
    P = nsrc * nchan
    sig = np.concatenate([ref.transpose(0, 2, 1).reshape(P, nsampl), est.transpose(0, 2, 1).reshape(P, nsampl)]).astype(np.float64)
    pairs = [(p, q) for p in range(P) for q in range(P)] + [(p, P + e) for p in range(P) for e in range(P)]
    ncw = len(corr_wins)
    sys_c = [(w, 0) for w in range(ncw)]
    sys_j = [(w, j * nchan) for w in range(ncw) for j in range(nsrc)]
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        d_sig = torch.from_numpy(sig).to(dev)
        d_win = torch.tensor(corr_wins, dtype=torch.int64, device=dev)
        d_pairs = torch.tensor(pairs, dtype=torch.int32, device=dev)
        d_sys_c = torch.tensor(sys_c, dtype=torch.int32, device=dev)
        d_sys_j = torch.tensor(sys_j, dtype=torch.int32, device=dev)
        d_items = torch.tensor(items, dtype=torch.int64, device=dev)
        corr = torch.empty((ncw, len(pairs), L), dtype=torch.float64, device=dev)
        coef_c = torch.empty((ncw, P, P * L), dtype=torch.float64, device=dev)
        coef_j = torch.empty((ncw * nsrc, P, nchan * L), dtype=torch.float64, device=dev)
        status = torch.empty(ncw * (1 + nsrc), dtype=torch.int32, device=dev)
        energy = torch.empty((len(items), 8), dtype=torch.float64, device=dev)
        corr_len = max(e - s for s, e in corr_wins)
        _lib.check(lib.glowk_bss_xcorr(_p(d_sig), 2 * P, nsampl, _p(d_win), ncw, corr_len, _p(d_pairs), len(pairs), L, _p(corr), stream))
        _lib.check(lib.glowk_bss_solve(_p(corr), ncw, len(pairs), P, L, P, _p(d_sys_c), ncw, _p(coef_c), _p(status), stream))
        _lib.check(lib.glowk_bss_solve(_p(corr), ncw, len(pairs), P, L, nchan, _p(d_sys_j), ncw * nsrc, _p(coef_j),
                                       ctypes.c_void_p(status.data_ptr() + 4 * ncw), stream))

        def project():
            _lib.check(lib.glowk_bss_project(_p(d_sig), nsampl, nsrc, nchan, L, _p(d_items), len(items), max_len, _p(coef_c), ncw,
                                             _p(coef_j), ncw * nsrc, _p(energy), stream))
            return energy.cpu().numpy()

        out = project()
        st = status.cpu().numpy()
        if np.any(st == 2):
            raise _lib.GlowkError("bss_solve: bad system descriptor (status 2)")
        bad_c, bad_j = np.nonzero(st[:ncw])[0], np.nonzero(st[ncw:])[0]
        _fallbacks = len(bad_c) + len(bad_j)
        if _fallbacks:
            c = corr.cpu().numpy()
            if len(bad_c):
                fix = lstsq_systems(c, P, L, [sys_c[k] for k in bad_c], P)
                coef_c[torch.from_numpy(bad_c).to(dev)] = torch.from_numpy(fix).to(dev)
            if len(bad_j):
                fix = lstsq_systems(c, P, L, [sys_j[k] for k in bad_j], nchan)
                coef_j[torch.from_numpy(bad_j).to(dev)] = torch.from_numpy(fix).to(dev)
            out = project()
    return out


def bss_eval_sources(reference_sources, estimated_sources, compute_permutation=True):
    """BSS Eval v3 bss_eval_sources (bsseval_v4.py:304-322): whole signal, sources version -> (sdr, sir, sar, perm)."""
    sdr, _, sir, sar, perm = bss_eval(reference_sources, estimated_sources, window=np.inf, hop=np.inf,
                                      compute_permutation=compute_permutation, filters_len=512, framewise_filters=True,
                                      bsseval_sources_version=True)
    return sdr, sir, sar, perm


def bss_eval_sources_framewise(reference_sources, estimated_sources, window=30 * 44100, hop=15 * 44100, compute_permutation=False):
    """BSS Eval v3 bss_eval_sources_framewise (bsseval_v4.py:325-343) -> (sdr, sir, sar, perm)."""
    sdr, _, sir, sar, perm = bss_eval(reference_sources, estimated_sources, window=window, hop=hop,
                                      compute_permutation=compute_permutation, filters_len=512, framewise_filters=True,
                                      bsseval_sources_version=True)
    return sdr, sir, sar, perm


def bss_eval_images(reference_sources, estimated_sources, compute_permutation=True):
    """BSS Eval v3 bss_eval_images (bsseval_v4.py:346-359) -> (sdr, isr, sir, sar, perm)."""
    return bss_eval(reference_sources, estimated_sources, window=np.inf, hop=np.inf, compute_permutation=compute_permutation,
                    filters_len=512, framewise_filters=True, bsseval_sources_version=False)


def bss_eval_images_framewise(reference_sources, estimated_sources, window=30 * 44100, hop=15 * 44100, compute_permutation=False):
    """BSS Eval v3 bss_eval_images_framewise (bsseval_v4.py:362-378) -> (sdr, isr, sir, sar, perm)."""
    return bss_eval(reference_sources, estimated_sources, window=window, hop=hop, compute_permutation=compute_permutation,
                    filters_len=512, framewise_filters=True, bsseval_sources_version=False)
