"""BSS Eval v4 on the GPU (csrc/glowk_bsseval.h through audiosourcesep_amd/bsseval.py): the host and kernel paths that
tests/test_gpu_bsseval.py does not reach, against the fp64 restatement of tests/bsseval_ref.py.

* P = nsrc * nchan > 8: k_bss_chol solves its right-hand sides 8 at a time, so P = 10 and P = 9 take a second pass;
* filters_len that leaves the last of the XC_LAGS = 4 lag slots of a k_bss_xcorr thread partial (100, 129, 511), exactly full
  (128) or one short (127), and windows shorter than filters_len (lags past the window's end are sums of nothing);
* more Cholesky systems than the 2 GiB workspace cap admits in one launch (bss_solve's second chunk, sys0 = 64);
* more long windows than the 256 MB cap on the partial sums admits in one correlation launch group (bss_xcorr's w0 = 4);
* the descriptor contract of the three C entry points: out-of-range windows are clipped, out-of-range indices give zeros or
  status 2, and nothing outside the output tensors is written.

Bounds and where each number comes from:
* metrics against R.bss_eval: TOL_SYNTH_DB = 1e-6 dB of tests/test_gpu_bsseval.py (well-conditioned G; measured there at the
  1e-12 level).  On the CPU the restatement's two algorithms (FFT + LU, and the kernels' direct lag sums + Cholesky) agree on
  every case of this module small enough for both to <= 8.2e-14 dB, and the FFT form alone ran the three long cases, with no
  LinAlgError and no NaN but the ISR of the sources version: the cases are no worse conditioned than that module's.  The one
  infinity is the SIR of the single-source case (no interference: C and Cj are the same system).  Measured on an MI355X:
  <= 1.3e-13 dB on every case.  perm and the NaN / inf pattern must be identical and ``last_fallbacks()`` 0;
* correlations through the C ABI against NumPy: 1e-12 of sum |u| |v| over the window.  Both are fp64 sums of n <= 3000 products
  in different orders, each within n * 2^-53 * sum |u| |v| = 3.3e-13 of the exact value;
* repeated calls: bitwise.

What ``Framing`` allows: every window it makes has the full length ``window`` (samples after the last whole window are dropped),
so "a last window shorter than filters_len" exists only when the one window is the whole signal.  That case, and a short last
window in a list of windows, are run here on the correlations, where the shorter window matters; through ``bss_eval`` a signal
shorter than filters_len is run with one mono source (with P >= 2 the system has M = P L > n + L - 1 unknowns and is singular:
the reference then solves rounding noise, which no other solver reproduces)."""
import ctypes
import time

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, bsseval
from tests import bsseval_ref as R
from tests.footprint import Guarded
from tests.test_bsseval_cpu import assert_metrics
from tests.test_gpu_bsseval import TOL_SYNTH_DB, synthetic

pytestmark = pytest.mark.gpu
NAMES = ("sdr", "isr", "sir", "sar")


def inputs(nsrc, nchan, n, seed):
    ref, est = synthetic(nsrc, nchan, n, seed)
    return (ref[..., 0], est[..., 0]) if nchan == 1 else (ref, est)


def check(ref, est, kw):
    got = bsseval.bss_eval(ref, est, **kw)
    assert bsseval.last_fallbacks() == 0
    stats = {}
    want = R.bss_eval(ref, est, stats=stats, **kw)
    assert stats["fallbacks"] == 0
    worst = max(float(np.nanmax(np.abs(g - w))) for g, w in zip(got[:4], want[:4]) if np.isfinite(w).any())
    print("bss_eval %s vs restatement: %.2e dB" % ({k: v for k, v in kw.items() if k != "hop"}, worst))
    assert_metrics(dict(zip(NAMES, got[:4])), dict(zip(NAMES, want[:4])), TOL_SYNTH_DB)
    assert got[4].dtype == np.int64 and np.array_equal(got[4], want[4])
    return got


# (nsrc, nchan, filters_len): P = 10 and 9; the largest filters_len with P * L <= 2048 (M = 2040 and 2043), and 32
MANY_CHANNELS = [(5, 2, 204), (5, 2, 32), (9, 1, 227), (9, 1, 32)]


@pytest.mark.parametrize("sources_version", [False, True])
@pytest.mark.parametrize("framewise", [False, True])
@pytest.mark.parametrize("nsrc,nchan,L", MANY_CHANNELS)
def test_more_than_eight_right_hand_sides(nsrc, nchan, L, framewise, sources_version):
    """k_bss_chol: ``for e0 ... += 8`` runs twice, the second pass with ne = 2 (P = 10) or 1 (P = 9)."""
    ref, est = inputs(nsrc, nchan, 16000, 50 + nsrc)
    check(ref, est, dict(window=8000, hop=8000, filters_len=L, framewise_filters=framewise, bsseval_sources_version=sources_version))


@pytest.mark.parametrize("nchan", [1, 2])
@pytest.mark.parametrize("L", [2, 100, 127, 128, 129, 511])
def test_filters_len_off_the_lag_grid(L, nchan):
    """A k_bss_xcorr thread owns lags t, t + 128, t + 256, t + 384: L = 100 leaves slot 0 partial, 129 gives slot 1 one lag,
    511 leaves one lag of slot 3 out, 127 / 128 sit at the edge of slot 0."""
    ref, est = inputs(2, nchan, 12000, 60 + L + nchan)
    check(ref, est, dict(window=5000, hop=3500, filters_len=L, framewise_filters=nchan == 1, compute_permutation=True))


def test_windows_shorter_than_filters_len():
    """The projections of windows of 100 samples through filters of 129 taps computed over the whole signal (len + L - 1 = 228
    output samples, more than half of them past the window), and a whole signal of 300 samples shorter than its 511 lags."""
    ref, est = inputs(2, 1, 1000, 71)
    got = check(ref, est, dict(window=100, hop=100, filters_len=129))
    assert got[0].shape == (2, 10)
    ref, est = inputs(1, 1, 300, 72)
    for framewise in (False, True):
        check(ref, est, dict(window=np.inf, hop=np.inf, filters_len=511, framewise_filters=framewise))


def test_more_cholesky_systems_than_one_launch_holds():
    """nsrc = nchan = 2 and filters_len = 512: M = 2048, a 32 MB workspace per system, so BSS_CHOL_CAP = 2 GiB admits 64 systems a
    launch; 66 windows with framewise filters are 66 systems over all references (chunks k0 = 0 and 64: ``sys0 > 0``) and 132 at
    M = 1024 (8 MB each: one launch).  M = 2048 is used, not the cheaper way past the cap (M = 1024 with 258 systems).
    Wall time on an MI355X host: the GPU call 0.3 s, the restatement 23.4 s on 16 cores."""
    ref, est = inputs(2, 2, 66 * 8192, 81)
    kw = dict(window=8192, hop=8192, filters_len=512, framewise_filters=True)
    t0 = time.time()
    got = bsseval.bss_eval(ref, est, **kw)
    t1 = time.time()
    assert bsseval.last_fallbacks() == 0 and got[0].shape == (2, 66)
    want = R.bss_eval(ref, est, **kw)
    t2 = time.time()
    print("66 systems of M = 2048: GPU call %.1f s, restatement %.1f s" % (t1 - t0, t2 - t1))
    assert_metrics(dict(zip(NAMES, got[:4])), dict(zip(NAMES, want[:4])), TOL_SYNTH_DB)
    assert np.array_equal(got[4], want[4])


def test_more_long_windows_than_one_correlation_group_holds():
    """Six windows of 30 s at 16 kHz, stereo, two sources, filters_len 512, framewise filters: npairs = 2 P^2 = 32,
    nsub = ceil(480000 / 1024) = 469 chunks, one per workgroup (nblk = 469), so one window's partial sums are
    per_win = 32 * 469 * 512 * 8 B = 61 472 768 B and BSS_SCRATCH_CAP / per_win = 268 435 456 / 61 472 768 = 4.37: groups of 4
    windows, launched at w0 = 0 and w0 = 4."""
    n = 6 * 480000
    ref, est = inputs(2, 2, n, 91)
    kw = dict(window=30 * 16000, hop=30 * 16000, framewise_filters=True)
    got = check(ref, est, kw)
    assert got[0].shape == (2, 6)
    again = bsseval.bss_eval(ref, est, **kw)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)


def test_one_long_window():
    """window = inf over 30 s: 469 workgroups per pair, their partials added by k_bss_xcorr_sum."""
    ref, est = inputs(2, 1, 30 * 16000, 95)
    kw = dict(window=np.inf, hop=np.inf)
    got = check(ref, est, kw)
    again = bsseval.bss_eval(ref, est, **kw)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)


# ---- the C entry points on descriptors outside the tensors ---------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def numpy_xcorr(u, v, s, e, L):
    """r[d] = sum_m u[m] v[m + d] over the window [s, e) clipped to the signal, and sum |u| |v| (the scale of its rounding)."""
    s, e = max(s, 0), min(e, len(u))
    u, v = (u[s:e], v[s:e]) if e > s else (u[:0], v[:0])
    n = len(u)
    return np.array([np.dot(u[:n - d], v[d:]) if d < n else 0.0 for d in range(L)]), float(np.dot(np.abs(u), np.abs(v)))


def run_xcorr(sig, wins, pairs, L, max_len):
    nsig, nsampl = sig.shape
    corr = Guarded((len(wins), len(pairs), L), torch.float64, float("nan"))
    d_sig, d_win = torch.from_numpy(sig).cuda(), torch.tensor(wins, dtype=torch.int64, device="cuda")
    d_pairs = torch.tensor(pairs, dtype=torch.int32, device="cuda")
    rc = _lib.load().glowk_bss_xcorr(_p(d_sig), nsig, nsampl, _p(d_win), len(wins), max_len, _p(d_pairs), len(pairs), L, corr.ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and corr.intact()
    return corr.t.cpu().numpy()


@pytest.mark.parametrize("L", [2, 100, 127, 128, 129, 511, 512])
def test_xcorr_lag_slots_and_short_windows_against_numpy(L):
    """Windows longer than, equal to and shorter than filters_len, the last one short, at every fill of the lag slots."""
    rng = np.random.default_rng(L)
    sig = rng.standard_normal((3, 3000))
    wins = [(0, 3000), (100, 150), (1000, 1000 + L), (7, 1031), (2990, 3000)]
    pairs = [(0, 1), (1, 0), (2, 2)]
    got = run_xcorr(sig, wins, pairs, L, 3000)
    for w, (s, e) in enumerate(wins):
        for k, (u, v) in enumerate(pairs):
            want, scale = numpy_xcorr(sig[u], sig[v], s, e, L)
            assert np.abs(got[w, k] - want).max() <= 1e-12 * scale, (w, k)
            if e - s < L:
                assert (got[w, k, e - s:] == 0).all()              # lags past the window: sums of nothing, exactly 0


def test_xcorr_descriptors_outside_the_signal():
    """Windows that start below 0, stop beyond nsampl, are empty, inverted or wholly outside are clipped to the signal; a pair
    with an index outside [0, nsig) gives zeros; the call succeeds and writes nothing outside corr."""
    rng = np.random.default_rng(3)
    sig = rng.standard_normal((4, 1000))
    big = 1 << 40
    wins = [(-50, 300), (700, 1200), (400, 400), (600, 500), (-10, 5), (990, 1000), (2000, 3000), (-100, -5), (-big, big), (995, big)]
    pairs = [(0, 1), (1, 0), (2, 3), (0, 0), (4, 0), (0, -1), (7, 9), (-big // 1024, 2)]
    L = 16
    got = run_xcorr(sig, wins, pairs, L, 1000)
    for w, (s, e) in enumerate(wins):
        for k, (u, v) in enumerate(pairs):
            if 0 <= u < 4 and 0 <= v < 4:
                want, scale = numpy_xcorr(sig[u], sig[v], s, e, L)
                assert np.abs(got[w, k] - want).max() <= 1e-12 * max(scale, 1e-300), (w, k)
            else:
                assert (got[w, k] == 0).all(), (w, k)
    assert (got[2] == 0).all() and (got[3] == 0).all() and (got[6] == 0).all() and (got[7] == 0).all()


def test_solve_and_project_descriptors_out_of_range():
    """glowk_bss_solve: a window or p0 outside the correlations gives status 2 for that system, the others are solved.
    glowk_bss_project: jtrue, jest or a system index out of range gives zero energies for that item; windows are clipped."""
    lib = _lib.load()
    rng = np.random.default_rng(4)
    nsrc, nchan, L, nsampl = 2, 1, 8, 1000
    P = nsrc * nchan
    sig = rng.standard_normal((2 * P, nsampl))
    sig[P:] = 0.8 * sig[:P] + 0.3 * sig[:P][::-1] + 0.1 * rng.standard_normal((P, nsampl))
    pairs = [(p, q) for p in range(P) for q in range(P)] + [(p, P + e) for p in range(P) for e in range(P)]
    wins = [(0, 1000), (0, 500), (300, 1000)]
    corr_np = run_xcorr(sig, wins, pairs, L, nsampl)
    corr = torch.from_numpy(corr_np).cuda()

    systems = [(0, 0), (3, 0), (-1, 0), (1, 1), (1, 0), (2, -1), (2, 0), (1 << 30, 0)]
    good = [0, 4, 6]
    d_sys = torch.tensor(systems, dtype=torch.int32, device="cuda")
    coef = Guarded((len(systems), P, P * L), torch.float64, float("nan"))
    status = Guarded((len(systems),), torch.int32, -1, canary=77)
    rc = lib.glowk_bss_solve(_p(corr), len(wins), len(pairs), P, L, P, _p(d_sys), len(systems), coef.ptr(), status.ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and coef.intact() and status.intact()
    st = status.t.cpu().numpy()
    assert st.tolist() == [0 if k in good else 2 for k in range(len(systems))]
    want = bsseval.lstsq_systems(corr_np, P, L, [systems[k] for k in good], P)   # fp64 least squares of the same G and D
    sol = coef.t.cpu().numpy()
    assert np.abs(sol[good] - want).max() <= 1e-9 * np.abs(want).max()   # cond(G) < 10 here: eps I and the solver move 1e-15

    # filters of window 0: C over both references, Cj over each reference alone
    sys_j = torch.tensor([(0, 0), (0, 1)], dtype=torch.int32, device="cuda")
    coef_c = coef.t[:1].contiguous()
    coef_j = torch.empty((2, P, nchan * L), dtype=torch.float64, device="cuda")
    st_j = torch.empty(2, dtype=torch.int32, device="cuda")
    assert lib.glowk_bss_solve(_p(corr), len(wins), len(pairs), P, L, nchan, _p(sys_j), 2, _p(coef_j), _p(st_j), None) == 0
    assert st_j.cpu().tolist() == [0, 0]
    big = 1 << 40
    items = [(0, 500, 0, 0, 0, 0), (0, 500, 2, 0, 0, 0), (0, 500, 0, -1, 0, 0), (0, 500, 0, 0, 5, 0), (0, 500, 0, 0, 0, -3),
             (100, 2000, 1, 1, 0, 1), (100, 1000, 1, 1, 0, 1), (-20, 300, 1, 0, 0, 1), (0, 300, 1, 0, 0, 1), (0, 500, big, 0, 0, 0),
             (600, 400, 0, 0, 0, 0), (0, 500, 0, 0, 0, 2), (-big, big, 0, 1, 0, 0), (0, 1000, 0, 1, 0, 0)]
    zero = [1, 2, 3, 4, 9, 11]
    d_items = torch.tensor(items, dtype=torch.int64, device="cuda")
    energy = Guarded((len(items), 8), torch.float64, float("nan"))
    rc = lib.glowk_bss_project(_p(torch.from_numpy(sig).cuda()), nsampl, nsrc, nchan, L, _p(d_items), len(items), nsampl, _p(coef_c), 1,
                               _p(coef_j), 2, energy.ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and energy.intact()
    en = energy.t.cpu().numpy()
    assert np.isfinite(en).all()
    for k in zero:
        assert (en[k] == 0).all(), k
    assert (en[10] == 0).all()                                   # an inverted window is empty
    assert np.array_equal(en[5], en[6]) and np.array_equal(en[7], en[8]) and np.array_equal(en[12], en[13])   # clipped windows
    for k in (0, 5, 7, 12):
        assert (en[k] > 0).all(), k
    # item 0 against NumPy: proj_all = sum_p C[p] * s_p, proj_j = Cj * s_jtrue over len + L - 1 samples
    C, Cj = coef_c.cpu().numpy()[0], coef_j.cpu().numpy()[0]
    s = sig[:, :500]
    pa = sum(np.convolve(C[0][p * L:(p + 1) * L], s[p]) for p in range(P))
    pj = np.convolve(Cj[0][:L], s[0])
    t, y = np.concatenate([s[0], np.zeros(L - 1)]), np.concatenate([s[P], np.zeros(L - 1)])
    want = [t @ t, (y - t) @ (y - t), (pj - t) @ (pj - t), pj @ pj, (pa - pj) @ (pa - pj), pa @ pa, (y - pa) @ (y - pa), (y - pj) @ (y - pj)]
    assert np.abs(en[0] - want).max() <= 1e-10 * max(want)       # fp64 sums of ~500 terms in another order
