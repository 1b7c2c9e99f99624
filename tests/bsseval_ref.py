"""fp64 NumPy oracle of BSS Eval v4 (a helper of the bsseval tests, not a test module).

Restates the reference's ``bsseval_v4.py`` from its formulas with numpy only (no scipy):

* windows: ``Framing`` (:382-418);
* G[(i,c1,a),(j,c2,b)] = sum_n s_{i,c1}[n-a] s_{j,c2}[n-b] and D[(j,cj,a), c] = sum_n s_{j,cj}[n-a] est_c[n], linear correlations over
  the zero-padded slices (_compute_reference_correlations :465-498, _compute_projection_filters :501-554);
* (G + eps I) C = D, LU with the ``lstsq(G, D)`` fallback on LinAlgError (:540-548);
* _bss_decomp_mtifilt (:421-437) with _project (:557-581), _bss_crit (:584-608), _safe_db (:611-617), the permutation choice
  (:278-301) and the NaN rows of silent windows (:250-276).

``algo="fft"`` computes the correlations with zero-padded FFTs and solves by LU, as the reference does; ``algo="direct"`` is the
kernels' algorithm: correlations as direct lag sums and a Cholesky solve (a pivot that is not positive -> lstsq).  The distance
between the two on real audio is what the GPU tolerances are derived from.
"""
import itertools

import numpy as np

EPS = np.finfo(np.float64).eps


def framing(window, hop, length):
    nwin = int(np.floor((length - window + hop) / hop)) if window < length else 1
    out = []
    for cur in range(nwin):
        start = cur * hop
        if np.isnan(start) or np.isinf(start):
            start = 0
        stop = min(cur * hop + window, length)
        if np.isnan(stop) or np.isinf(stop):
            stop = length
        out.append(slice(int(np.floor(start)), int(np.floor(stop))))
    return out


def any_source_silent(sources):
    return np.any(np.all(np.sum(sources, axis=tuple(range(2, sources.ndim))) == 0, axis=1))


def _xcorr(u, v, L, algo):
    """r[d] = sum_m u[m] v[m + d], d = 0..L-1 (linear)."""
    n = len(u)
    if algo == "direct":
        return np.array([np.dot(u[:n - d], v[d:]) if d < n else 0.0 for d in range(L)])
    nfft = int(2 ** np.ceil(np.log2(n + L - 1.0)))
    r = np.fft.irfft(np.conj(np.fft.rfft(u, nfft)) * np.fft.rfft(v, nfft), nfft)
    return r[:L]


def _gram(refs, L, algo):
    """refs [nsrc, n, nchan] -> G [P L, P L] (rows (i, c1, a))."""
    nsrc, n, nchan = refs.shape
    x = refs.transpose(0, 2, 1).reshape(nsrc * nchan, n)
    P = len(x)
    G = np.empty((P * L, P * L))
    d = np.arange(L)[:, None] - np.arange(L)[None, :]
    for p in range(P):
        for q in range(P):
            rpq, rqp = _xcorr(x[p], x[q], L, algo), _xcorr(x[q], x[p], L, algo)
            G[p * L:(p + 1) * L, q * L:(q + 1) * L] = np.where(d >= 0, rpq[np.abs(d)], rqp[np.abs(d)])
    return G


def _rhs(refs, est, L, algo):
    """D [P L, nchan]: D[(j,cj,a), c] = sum_n s_{j,cj}[n-a] est_c[n]."""
    nsrc, n, nchan = refs.shape
    x = refs.transpose(0, 2, 1).reshape(nsrc * nchan, n)
    return np.stack([np.concatenate([_xcorr(x[p], est[:, c], L, algo) for p in range(len(x))]) for c in range(nchan)], axis=1)


def _solve(G, D, algo, stats):
    if algo == "direct":
        try:
            Lc = np.linalg.cholesky(G + EPS * np.eye(len(G)))
            return np.linalg.solve(Lc.T, np.linalg.solve(Lc, D))
        except np.linalg.LinAlgError:
            stats["fallbacks"] += 1
            return np.linalg.lstsq(G, D, rcond=None)[0]
    try:
        return np.linalg.solve(G + EPS * np.eye(len(G)), D)
    except np.linalg.LinAlgError:
        stats["fallbacks"] += 1
        return np.linalg.lstsq(G, D, rcond=None)[0]


def _conv(h, x, nout):
    """full linear convolution, first nout samples (fftconvolve(h, x)[:nout])."""
    nfft = int(2 ** np.ceil(np.log2(len(h) + len(x) - 1.0)))
    return np.fft.irfft(np.fft.rfft(h, nfft) * np.fft.rfft(x, nfft), nfft)[:nout]


def _project(refs, C, L):
    """refs [nsrc, n, nchan], C [nsrc, nchan, L, nchan] -> [n + L - 1, nchan]."""
    nsrc, n, nchan = refs.shape
    out = np.zeros((n + L - 1, nchan))
    for j, cj, c in itertools.product(range(nsrc), range(nchan), range(nchan)):
        out[:, c] += _conv(C[j, cj, :, c], refs[j, :, cj], n + L - 1)
    return out


def _safe_db(num, den):
    if den == 0:
        return np.inf
    with np.errstate(divide="ignore"):
        return 10 * np.log10(num / den)


def _crit(s_true, e_spat, e_interf, e_artif, sources_version):
    if sources_version:
        s_filt = s_true + e_spat
        e = np.sum(s_filt ** 2)
        return (_safe_db(e, np.sum((e_interf + e_artif) ** 2)), np.nan, _safe_db(e, np.sum(e_interf ** 2)),
                _safe_db(np.sum((s_filt + e_interf) ** 2), np.sum(e_artif ** 2)))
    e = np.sum(s_true ** 2)
    return (_safe_db(e, np.sum((e_spat + e_interf + e_artif) ** 2)), _safe_db(e, np.sum(e_spat ** 2)),
            _safe_db(np.sum((s_true + e_spat) ** 2), np.sum(e_interf ** 2)),
            _safe_db(np.sum((s_true + e_spat + e_interf) ** 2), np.sum(e_artif ** 2)))


def bss_eval(reference_sources, estimated_sources, window=2 * 44100, hop=1.5 * 44100, compute_permutation=False, filters_len=512,
             framewise_filters=False, bsseval_sources_version=False, algo="fft", stats=None):
    """-> (sdr, isr, sir, sar, perm) as the reference returns them.  ``stats`` (a dict) receives the number of lstsq fallbacks."""
    stats = {} if stats is None else stats
    stats["fallbacks"] = 0
    est = np.atleast_3d(np.asarray(estimated_sources, dtype=np.float64))
    ref = np.atleast_3d(np.asarray(reference_sources, dtype=np.float64))
    nsrc, nsampl, nchan = est.shape
    L = filters_len
    cands = (np.array(list(itertools.permutations(range(nsrc)))) if compute_permutation else np.arange(nsrc)[None, :])
    wins = framing(window, hop, nsampl)
    nwin = len(wins)
    s_r = np.full((4, nsrc, nsrc, nwin), np.nan)

    def filters(win):
        r = ref[:, win]
        G = _gram(r, L, algo)
        C = [_solve(G, _rhs(r, est[j, win], L, algo), algo, stats).reshape(nsrc, nchan, L, nchan) for j in range(nsrc)]
        Cj = {}
        for jtrue in range(nsrc):
            Gj = G[jtrue * nchan * L:(jtrue + 1) * nchan * L, jtrue * nchan * L:(jtrue + 1) * nchan * L]
            for jest in set(cands[:, jtrue].tolist()):
                Cj[jtrue, jest] = _solve(Gj, _rhs(r[jtrue:jtrue + 1], est[jest, win], L, algo), algo, stats).reshape(1, nchan, L, nchan)
        return C, Cj

    if not framewise_filters:
        C, Cj = filters(slice(0, nsampl))
    for t, win in enumerate(wins):
        r, e = ref[:, win], est[:, win]
        if any_source_silent(r) or any_source_silent(e):
            continue
        if framewise_filters:
            C, Cj = filters(win)
        n = r.shape[1]
        for jtrue in range(nsrc):
            for jest in set(cands[:, jtrue].tolist()):
                s_true = np.zeros((n + L - 1, nchan))
                s_true[:n] = r[jtrue]
                e_spat = _project(r[jtrue:jtrue + 1], Cj[jtrue, jest], L) - s_true
                e_interf = _project(r, C[jest], L) - s_true - e_spat
                e_artif = -s_true - e_spat - e_interf
                e_artif[:n] += e[jest]
                s_r[:, jtrue, jest, t] = _crit(s_true, e_spat, e_interf, e_artif, bsseval_sources_version)

    if framewise_filters:
        mean_sir = np.empty((len(cands), nwin))
        axis_mean = 0
    else:
        mean_sir = np.empty((len(cands), 1))
        axis_mean = None
    dum = np.arange(nsrc)
    for i, perm in enumerate(cands):
        mean_sir[i] = np.mean(s_r[2, dum, perm, :], axis=axis_mean)
    popt = cands[np.argmax(mean_sir, axis=0)].T
    if not framewise_filters:
        result = s_r[:, dum, popt[:, 0], :]
    else:
        result = np.empty((4, nsrc, nwin))
        for m, t in itertools.product(range(4), range(nwin)):
            result[m, :, t] = s_r[m, dum, popt[:, t], t]
    return result[0], result[1], result[2], result[3], popt
