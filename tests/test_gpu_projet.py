"""PROJET on the GPU (audiosourcesep_amd/projet.py, csrc/glowk_projet.h) against the fp64 restatement of tests/projet_ref.py.

What is exact is compared bit for bit: the fused fit against the staged calls, a batch against its signals, two runs, the stored
projections against the V the fused pass holds in registers.  The rest carries a bound, u = 2^-53; the test allows twice each bound
because the restatement carries an equal share.

V: c_m is two exact-in-order products and one add per component, V one more add and a root, so for alpha 1 and 2 the device and numpy
round alike and the bound 8 u (|X_1| + |X_2|)^alpha is absolute only because c_m may cancel.  For other alpha V goes through pow; no
error bound of the device's fp64 pow is documented, so the project's cap for an fp64 library function is used, 1e-12 of that scale
(tests/test_gpu_duet.py).
update_p, fed the device's V: every term is non-negative, so the bound is relative: sigma is J products and adds, the weights two
divisions, num and den M products and adds each, then a quotient, a root and a product: (2 M + 2 J + 16) u.
update_q, fed the device's V and the device's P': one element of An is a sum of non-negative terms whose longest chain of additions is
c = glowk_projet_index.h's chain(rows, frames) (it is restated below and checked against the header in tests/test_projet_cpu.py);
then M products and adds over m, twice, and the quotient: 2 (c + 2 M + J + 16) u relative.  The restatement adds the cells in long double
here (and for the divergence): numpy's own fp64 sum over the cells has an order of its own and its error would be measured, not the device's.
divergence: (c + M + J + 8) u times the sum over the terms of the magnitudes of their parts (|V ln(V / s)| + V + s; q + |ln q| + 1;
(V + s)^2 / 2, because V - s cancels).
separate: w is at most 1 with J + 3 roundings, the sum over m has M terms: (M + J + 16) u sum_m |Up[ch][m]| |c_m|, plus the one
rounding to complex64, 2^-24 |Y| (not doubled: the restatement is compared before its rounding).  The stems' sum: that bound summed over j."""
import ctypes
import functools
import json
import math
import wave

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, audio, projet
from tests import projet_ref as R

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
CAP = 1e-12
# (nsig, rows, frames): the issue's nine, then both sides of every edge the kernels have.  A matrix-core instruction takes 4 cells (3, 4,
# 5 cells), a wave 64 (63, 64, 65), a workgroup step 256 (255, 256), the second workgroup of a signal starts at 257 cells; the workgroups
# of a signal stop growing at 1024 (262 144 cells: 512 x 512, one step each), and from 262 145 cells (545 x 481) a workgroup walks a
# second step of 256 cells.
ISSUE_SHAPES = [(1, 1, 1), (1, 2, 1), (2, 3, 5), (1, 33, 40), (3, 17, 24), (1, 65, 130), (1, 129, 257), (1, 1025, 24), (1, 4096, 5)]
EDGE_SHAPES = [(1, 1, 3), (1, 1, 4), (1, 1, 5), (1, 1, 63), (1, 1, 64), (2, 1, 65), (1, 1, 255), (1, 1, 256), (2, 1, 257)]
BIG_SHAPES = [(1, 512, 512), (1, 545, 481)]
MODELS = [(2, 1, 1), (2, 3, 2), (12, 21, 3), (15, 41, 4), (16, 41, 8), (17, 40, 5), (32, 128, 8)]
POWERS = [(a, b) for a in (1.0, 2.0, 1.5) for b in (0, 1, 2)]
BIG_POWERS = [(1.0, 0), (2.0, 1), (1.5, 2)]          # the two 262 k-cell shapes are this file's own: one beta per alpha keeps them to seconds
IDS = lambda s: "-".join(map(str, s))
WORST = {}


def chain(rows, frames):
    """glowk_projet_index.h's chain(): 64 steps + 4 waves + the workgroups."""
    cells = rows * frames
    g = max(1, min(1024, -(-cells // 256)))
    per = -(-(-(-cells // g)) // 256) * 256
    return (per // 256) * 64 + 4 + -(-cells // per)


def note(name, frac):
    WORST[name] = max(WORST.get(name, 0.0), float(frac))


@functools.lru_cache(maxsize=None)
def stft(shape, M):
    """Complex Gaussian channels, every cell scaled by 10^uniform(-3, 1), about 5 % exact zeros in each channel, some cells zero in both,
    some panned exactly at a projection angle (c_m cancels); rounded to complex64; never modified."""
    rng = np.random.default_rng(1000 * shape[1] + shape[2] + M)
    full = (shape[0], 2) + shape[1:]
    X = (rng.standard_normal(full) + 1j * rng.standard_normal(full)) * 10.0 ** rng.uniform(-3, 1, full)
    X *= rng.random(full) >= 0.05
    X *= (rng.random((shape[0], 1) + shape[1:]) >= 0.03)
    phi = np.arange(M) * math.pi / (2 * (M - 1))
    m = rng.integers(0, M, (shape[0],) + shape[1:])
    s = X[:, 0].copy()
    at = rng.random(m.shape) < 0.1
    X[:, 0] = np.where(at, np.cos(phi[m]) * s, X[:, 0])
    X[:, 1] = np.where(at, np.sin(phi[m]) * s, X[:, 1])
    X = X.astype(np.complex64)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def state(shape, model, alpha):
    """(P [N, J, R, T], Q [N, L, J]) in fp64: the deterministic start, P scattered by uniform(0.5, 1.5) with about 3 % exact zeros."""
    M, L, J = model
    tab = R.tables(M, L, alpha)
    X = stft(shape, M)
    rng = np.random.default_rng(7 + shape[1] * shape[2] + J)
    P, Q = [], []
    for n in range(shape[0]):
        p, q = R.init(X[n], J, tab)
        P.append(p * rng.uniform(0.5, 1.5, p.shape) * (rng.random(p.shape) >= 0.03))
        Q.append(q * rng.uniform(0.5, 1.5, q.shape))
    P, Q = np.stack(P), np.stack(Q)
    P.setflags(write=False)
    Q.setflags(write=False)
    return P, Q


def cuda(a):
    return torch.from_numpy(np.array(a)).cuda()                                          # a copy: the cached inputs are read-only


def check_case(shape, model, powers):
    M, L, J = model
    N = shape[0]
    X = stft(shape, M)
    x = cuda(X)
    c = chain(shape[1], shape[2])
    mag = np.abs(X.astype(np.complex128))
    for alpha in sorted({a for a, _ in powers}):
        tab = projet.tables(M, L, alpha)
        rt = R.tables(M, L, alpha)
        assert np.array_equal(tab["U"], rt["U"]) and np.array_equal(tab["K"], rt["K"]) and np.abs(tab["Up"] - rt["Up"]).max() <= 1e-14 * np.abs(rt["Up"]).max()
        rt["Up"] = tab["Up"]
        V = projet.projections(x, tab)
        assert V.is_cuda and V.dtype == torch.float64 and tuple(V.shape) == (N, M) + shape[1:]
        V = V.cpu().numpy()
        scale = (mag[:, 0] + mag[:, 1]) ** alpha
        bound = 2 * (8 * U53 if alpha in (1.0, 2.0) else CAP) * scale
        Vr = np.stack([R.projections(X[n], rt) for n in range(N)])
        err = np.abs(V - Vr)
        assert (err <= bound[:, None]).all(), (alpha, (err / np.maximum(bound[:, None], 1e-300)).max())
        note("V", (err / np.where(bound > 0, bound, 1.0)[:, None]).max())
        P0, Q0 = state(shape, model, alpha)
        p0, q0 = cuda(P0), cuda(Q0)
        for beta in [b for a, b in powers if a == alpha]:
            tag = "%s %s alpha %g beta %d" % (IDS(shape), IDS(model), alpha, beta)
            G = projet.gains(q0, tab).cpu().numpy()
            Gr = np.stack([R.gains(Q0[n], rt["K"]) for n in range(N)])
            assert (np.abs(G - Gr) <= 2 * (L + 2) * U53 * Gr).all(), tag
            # update_p, fed the device's V
            P1 = projet.update_p(x, p0, q0, tab, beta)
            assert P1.is_cuda and P1.dtype == torch.float64 and tuple(P1.shape) == P0.shape and P1.data_ptr() != p0.data_ptr()
            P1 = P1.cpu().numpy()
            P1r = np.stack([R.update_p(V[n], P0[n], G[n], beta) for n in range(N)])
            assert np.isfinite(P1).all() and (P1 >= 0).all() and not P1[P1r == 0].any(), tag
            rel = np.abs(P1 - P1r) / np.where(P1r > 0, P1r, 1.0)
            bp = 2 * (2 * M + 2 * J + 16) * U53
            print("update_p %s: %.3f of the bound" % (tag, rel.max() / bp))
            assert rel.max() <= bp, tag
            note("update_p", rel.max() / bp)
            # update_q, fed the device's V and the device's P'
            p1 = cuda(P1)
            Q1 = projet.update_q(x, p1, q0, tab, beta).cpu().numpy()
            Q1r = np.stack([R.update_q(V[n], P1[n], Q0[n], rt["K"], beta, G[n], wide=True) for n in range(N)])
            assert np.isfinite(Q1).all() and (Q1 >= 0).all() and not Q1[Q1r == 0].any(), tag
            rel = np.abs(Q1 - Q1r) / np.where(Q1r > 0, Q1r, 1.0)
            bq = 2 * 2 * (c + 2 * M + J + 16) * U53
            print("update_q %s: %.3f of the bound" % (tag, rel.max() / bq))
            assert rel.max() <= bq, tag
            note("update_q", rel.max() / bq)
            # the divergence
            D = projet.divergence(x, p1, q0, tab, beta).cpu().numpy().reshape(N)
            for n in range(N):
                d, a = R.divergence_terms(V[n], P1[n], G[n], beta)
                bd, dr = 2 * (c + M + J + 8) * U53 * a.sum(), float(d.astype(np.longdouble).sum())
                assert abs(D[n] - dr) <= bd, (tag, D[n], dr, bd)
                note("divergence", abs(D[n] - dr) / bd)
            if beta != 1:
                continue
            # the separation (it does not depend on beta) and the stems' sum
            Y = projet.separate(x, p1, q0, tab)
            assert Y.is_cuda and Y.dtype == torch.complex64 and tuple(Y.shape) == (N, J, 2) + shape[1:]
            Y = Y.cpu().numpy()
            total = np.zeros((N, 2) + shape[1:])
            for n in range(N):
                Yr = R.separate(X[n], P1[n], G[n], rt, dtype=None)
                by = 2 * (M + J + 16) * U53 * R.separate_scale(X[n], rt)[None] + 2.0 ** -24 * np.abs(Yr)
                err = np.maximum(np.abs(Y[n].real - Yr.real), np.abs(Y[n].imag - Yr.imag))
                assert (err <= by).all(), (tag, (err / np.maximum(by, 1e-300)).max())
                note("separate", (err / np.where(by > 0, by, 1.0)).max())
                total[n] = by.sum(axis=0)
            gap = np.abs(Y.astype(np.complex128).sum(axis=1) - X)
            assert (gap <= total * math.sqrt(2)).all(), tag
            note("stems' sum", (gap / np.where(total > 0, total * math.sqrt(2), 1.0)).max())
            for n in range(N):                                                           # a cell that is 0 in both channels is 0 in every stem
                assert not Y[n][:, :, (mag[n, 0] == 0) & (mag[n, 1] == 0)].any(), tag


@pytest.mark.parametrize("shape", ISSUE_SHAPES + EDGE_SHAPES, ids=IDS)
def test_every_stage_within_its_bound_at_every_shape(shape):
    check_case(shape, (12, 21, 3), POWERS)


@pytest.mark.parametrize("shape", BIG_SHAPES, ids=IDS)
def test_every_stage_within_its_bound_where_the_workgroups_stop_growing(shape):
    check_case(shape, (12, 21, 3), BIG_POWERS)


@pytest.mark.parametrize("model", MODELS, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 65, 130)], ids=IDS)
def test_every_stage_within_its_bound_for_every_model(shape, model):
    check_case(shape, model, POWERS)


def test_the_worst_fractions_of_the_bounds():
    """Printed for profiles/projet_time.json and the README; the assertions are in the tests above."""
    print("largest measured fraction of each bound (of twice the bound, as asserted):", json.dumps({k: round(v, 4) for k, v in sorted(WORST.items())}))


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------------
def same(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("model", [(12, 21, 3), (17, 40, 5)], ids=IDS)
@pytest.mark.parametrize("shape", [(2, 3, 5), (3, 17, 24), (2, 1, 257), (1, 129, 257)], ids=IDS)
def test_fit_is_the_staged_calls_a_batch_its_signals_and_a_run_its_repeat(shape, model):
    M, L, J = model
    for alpha, beta in ((1.0, 1), (2.0, 2), (1.5, 0)):
        tab = projet.tables(M, L, alpha)
        x = cuda(stft(shape, M))
        P0, Q0 = state(shape, model, alpha)
        p, q = cuda(P0), cuda(Q0)
        Pf, Qf = projet.fit(x, p, q, tab, beta, 3)
        assert same(p, cuda(P0)) and same(q, cuda(Q0))                                   # the inputs stand
        for _ in range(3):
            p = projet.update_p(x, p, q, tab, beta)
            q = projet.update_q(x, p, q, tab, beta)
        assert same(Pf, p) and same(Qf, q), (alpha, beta)
        again = projet.fit(x, cuda(P0), cuda(Q0), tab, beta, 3)
        assert same(again[0], Pf) and same(again[1], Qf)
        D = projet.divergence(x, Pf, Qf, tab, beta)
        Y = projet.separate(x, Pf, Qf, tab)
        for n in range(shape[0]):
            Pn, Qn = projet.fit(x[n], cuda(P0[n]), cuda(Q0[n]), tab, beta, 3)
            assert same(Pn, Pf[n]) and same(Qn, Qf[n]), (alpha, beta, n)
            assert same(projet.divergence(x[n], Pn, Qn, tab, beta).reshape(1), D[n].reshape(1))
            assert torch.equal(torch.view_as_real(projet.separate(x[n], Pn, Qn, tab)), torch.view_as_real(Y[n]))
        zero = projet.fit(x, cuda(P0), cuda(Q0), tab, beta, 0)
        assert same(zero[0], cuda(P0)) and same(zero[1], cuda(Q0))


@pytest.mark.parametrize("alpha", [1.0, 2.0, 1.5])
@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 33, 40), (2, 1, 257)], ids=IDS)
def test_the_stored_projections_are_the_bits_the_fused_pass_uses(shape, alpha):
    """update_p with P = 1, beta 2 and a one-hot G (K the identity, Q one-hot at m0, J = 1): num = V_m0 and den = 1 exactly, so the new P
    is the V_m0 the pass held in registers."""
    M = 12
    x = cuda(stft(shape, M))
    tab = projet.tables(M, 21, alpha)
    V = projet.projections(x, tab)
    eye = dict(U=tab["U"], K=np.eye(M), alpha=alpha)
    ones = torch.ones((shape[0], 1) + shape[1:], dtype=torch.float64, device="cuda")
    for m0 in range(M):
        Q = torch.zeros((shape[0], M, 1), dtype=torch.float64, device="cuda")
        Q[:, m0] = 1.0
        P = projet.update_p(x, ones, Q, eye, 2)
        assert same(P[:, 0].contiguous(), V[:, m0].contiguous()), (alpha, m0)


# ---- chains ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", [(33, 40, (0.2, 0.8, 1.35), 0.25), (17, 24, (0.3, 1.2), 0.5)], ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("alpha,beta", [(1.0, 1), (1.0, 0), (2.0, 2), (1.5, 1)])
def test_fifty_iterations_stay_with_the_restatement(scene, alpha, beta):
    """max |dP| / max P and max |dQ| / max Q after 50 iterations stay below 1000 times what reversing rows and frames changes in the
    restatement itself (never below 1e-13): the factor covers what a reordering does not have, sqrt against hypot and the order within
    a cell.  The SDR gains equal the restatement's to 0.001 dB."""
    Rr, T, pans, density = scene
    J = len(pans)
    X, imgs = R.scene(Rr, T, pans, density)
    rt = R.tables(12, 21, alpha)
    Pr, Qr = R.fit(X, J, rt, beta, 50)
    Pb, Qb = R.fit(X[:, ::-1, ::-1], J, rt, beta, 50)
    Pb = Pb[:, ::-1, ::-1]
    dp, dq = np.abs(Pr - Pb).max() / Pr.max(), np.abs(Qr - Qb).max() / Qr.max()
    tab = projet.tables(12, 21, alpha)
    x = cuda(X)
    P, Q = projet.init(x, J, tab)
    P, Q = projet.fit(x, P, Q, tab, beta, 50)
    ep = np.abs(P.cpu().numpy() - Pr).max() / Pr.max()
    eq = np.abs(Q.cpu().numpy() - Qr).max() / Qr.max()
    print("chain %dx%d alpha %g beta %d: dP %.2e dQ %.2e, the restatement's reordering %.2e %.2e" % (Rr, T, alpha, beta, ep, eq, dp, dq))
    assert ep <= max(1000 * dp, 1e-13) and eq <= max(1000 * dq, 1e-13)
    Y = projet.separate(x, P, Q, tab).cpu().numpy()
    Yr = R.separate(X, Pr, R.gains(Qr, rt["K"]), rt)
    assert np.abs(R.sdr_gains(Y, X, imgs) - R.sdr_gains(Yr, X, imgs)).max() <= 0.001
    whole, model = projet.projet(x, J, 12, 21, alpha, beta, 50, return_model=True)
    assert same(model["P"], P) and same(model["Q"], Q) and torch.equal(torch.view_as_real(whole), torch.view_as_real(cuda(Y)))
    assert np.array_equal(model["pans"].cpu().numpy(), R.pan_estimates(Q.cpu().numpy(), rt["theta"]))


# ---- audio -------------------------------------------------------------------------------------------------------------------------------
TONES = ((330.0, 0.25), (1270.0, 0.8), (3100.0, 1.3))      # (Hz, pan): far apart in frequency, so that the restatement separates them


def tones(n=32000):
    t = np.arange(n) / audio.SR
    src = [np.sin(2 * np.pi * f * t) * (0.5 + 0.4 * np.sin(2 * np.pi * (1.0 + k) * t)) for k, (f, _) in enumerate(TONES)]
    imgs = np.stack([np.stack([math.cos(th) * s, math.sin(th) * s]) for s, (_, th) in zip(src, TONES)]).astype(np.float32)
    return imgs.sum(axis=0), imgs


def test_projet_audio_returns_aligned_stems_that_add_up_to_the_input():
    y, imgs = tones()
    n = y.shape[1]
    stems, res = projet.projet_audio(y, 3, n_iter=50, residual=True)
    assert stems.is_cuda and stems.dtype == torch.float32 and tuple(stems.shape) == (3, 2, n) and tuple(res.shape) == (2, n)
    s = stems.cpu().numpy().astype(np.float64)
    # the CPU restatement separates these tones (tests/test_projet_cpu.py holds it to 8 dB over y / 3); the device does as well
    for j in range(3):
        base = 10 * math.log10((imgs[j] ** 2).sum() / ((imgs[j] - y / 3) ** 2).sum())
        got = 10 * math.log10((imgs[j] ** 2).sum() / ((imgs[j] - s[j]) ** 2).sum())
        print("tone %d: %.1f dB over y / 3" % (j, got - base))
        assert got - base >= 8.0
    # the stems' sum: audio.istft's own round trip of y, plus the separation's bound on the stems' sum carried through the inverse
    # transform.  Per bin b = sum_j (2 (M + J + 16) u sqrt(2) scale + 5 2^-24 |Y_j|): the rounding to complex64 and the four float32
    # roundings of istft's magnitude, angle, polar form and product, once per stem.  A sample is sum_t w irfft(Y_t) / sum_t w^2 over the
    # frames that cover it: an error e in every bin of a frame moves its irfft by at most (2 / n_fft) sum_f e, and sum w / sum w^2 is at
    # most 4 / 3 for the Hann window at a quarter hop.
    yd = torch.from_numpy(y).cuda()
    _, X = audio.mel_frames(yd, return_stft=True)
    Y = projet.projet(X, 3, n_iter=50).cpu().numpy()
    tab = R.tables(15, 41, 1.0)
    b = 2 * (15 + 3 + 16) * U53 * math.sqrt(2) * 3 * R.separate_scale(X.cpu().numpy(), tab) + 5 * 2.0 ** -24 * np.abs(Y).sum(axis=0)
    carried = 4.0 / 3.0 * (2.0 / 2048) * b.sum(axis=1).max()
    trip = (audio.istft(X)[..., :n] - yd).abs().max().item()
    gap = (stems.sum(0) - yd).abs().max().item()
    print("stems' sum: %.2e, the round trip alone %.2e, the separation's bound carried through the inverse %.2e" % (gap, trip, carried))
    assert gap <= trip + carried
    assert torch.equal(res, yd - stems.sum(0))


def test_separate_wav_projet_returns_the_files_rate_and_sample_count(tmp_path):
    y, _ = tones(22050 * 2)
    path = str(tmp_path / "mix.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(2)
        f.setframerate(22050)
        f.writeframes((np.clip(y.T, -1, 1) * 32767).astype("<i2").tobytes())
    stems, rate = projet.separate_wav_projet(path, 3, n_iter=5)
    assert rate == 22050 and tuple(stems.shape) == (3, 2, 44100) and stems.is_cuda
    stems, rate = projet.separate_wav_projet(path, 2, out_rate=None, n_iter=2, residual=True)
    assert rate == audio.SR and stems.shape[0] == 3 and stems.shape[1] == 2
    mono = str(tmp_path / "mono.wav")
    with wave.open(mono, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.zeros(4000, "<i2").tobytes())
    with pytest.raises(ValueError, match="two channels"):
        projet.separate_wav_projet(mono, 2)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_a_host_pointer_and_every_out_of_range_argument_are_refused_through_ctypes():
    lib = _lib.load()
    z = ctypes.c_void_p(0)
    err = lambda: lib.glowk_last_error().decode()
    M, L, J, Rr, T = 4, 5, 2, 3, 7
    d = lambda *s: torch.ones(s, dtype=torch.float64, device="cuda")
    x = torch.ones((1, 2, Rr, T, 2), dtype=torch.float32, device="cuda")
    u, k, up, p, q, g, v, dd = d(M, 2), d(M, L), d(2, M), d(1, J, Rr, T), d(1, L, J), d(1, M, J), d(1, M, Rr, T), d(1)
    y = torch.zeros((1, J, 2, Rr, T, 2), dtype=torch.float32, device="cuda")
    nbytes = lib.glowk_projet_workspace_bytes(1, M, J, Rr, T)
    assert nbytes == 16 * M * J
    work = d(max(nbytes // 8, 2))
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    host = ctypes.c_void_p(torch.ones(4096, dtype=torch.float64).data_ptr())

    def fit(x=P(x), nsig=1, rows=Rr, frames=T, u=P(u), k=P(k), M=M, L=L, J=J, alpha=1.0, beta=1, n_iter=1, p=P(p), q=P(q), g=P(g), work=P(work), nbytes=nbytes):
        return lib.glowk_projet_fit(x, nsig, rows, frames, u, k, M, L, J, alpha, beta, n_iter, p, q, g, work, nbytes, z)

    assert fit() == _lib.OK
    cases = [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(rows=0), "rows"), (dict(rows=4097), "rows"), (dict(frames=0), "frames"),
             (dict(frames=32769), "frames"), (dict(M=1), "M must"), (dict(M=33), "M must"), (dict(L=0), "L must"), (dict(L=129), "L must"), (dict(J=0), "J must"),
             (dict(J=9), "J must"), (dict(alpha=0.99), "alpha"), (dict(alpha=2.01), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(beta=-1), "beta"),
             (dict(beta=3), "beta"), (dict(n_iter=-1), "n_iter"), (dict(n_iter=100001), "n_iter"), (dict(nsig=65535, rows=4096, frames=32768), "2^31"),
             (dict(p=z), "null"), (dict(nbytes=8), "work_bytes"), (dict(q=ctypes.c_void_p(q.data_ptr() + 4)), "aligned"), (dict(g=P(q)), "overlap"),
             (dict(x=host), "device memory"), (dict(p=host), "device memory")]
    for kw, word in cases:
        assert fit(**kw) == _lib.ERR and word in err(), (kw, err())
    assert fit(nsig=0) == _lib.OK
    calls = [
        lambda **o: lib.glowk_projet_projections(o.get("x", P(x)), 1, o.get("rows", Rr), T, P(u), o.get("M", M), o.get("alpha", 1.0), P(v), z),
        lambda **o: lib.glowk_projet_gains(o.get("x", P(k)), P(q), 1, o.get("M", M), L, J, P(g), z),
        lambda **o: lib.glowk_projet_update_p(o.get("x", P(x)), 1, o.get("rows", Rr), T, P(u), P(g), o.get("M", M), J, o.get("alpha", 1.0), 1, P(p), z),
        lambda **o: lib.glowk_projet_update_q(o.get("x", P(x)), P(p), 1, o.get("rows", Rr), T, P(u), P(k), o.get("M", M), L, J, o.get("alpha", 1.0), 1, P(q), P(g), P(work),
                                              nbytes, z),
        lambda **o: lib.glowk_projet_divergence(o.get("x", P(x)), P(p), 1, o.get("rows", Rr), T, P(u), P(g), o.get("M", M), J, o.get("alpha", 1.0), 1, P(dd), P(work),
                                                nbytes, z),
        lambda **o: lib.glowk_projet_separate(o.get("x", P(x)), P(p), 1, o.get("rows", Rr), T, P(u), P(up), P(g), o.get("M", M), J, P(y), z),
    ]
    for n, call in enumerate(calls):
        assert call() == _lib.OK, (n, err())
        assert call(x=host) == _lib.ERR and "device memory" in err(), n
        assert call(M=33) == _lib.ERR and "M must" in err(), n
        if n != 1:
            assert call(rows=4097) == _lib.ERR and "rows" in err(), n
        if n not in (1, 5):
            assert call(alpha=3.0) == _lib.ERR and "alpha" in err(), n
    torch.cuda.synchronize()
    for args in [(0, M, J, Rr, T), (1, 1, J, Rr, T), (1, M, 9, Rr, T), (1, M, J, 4097, T), (1, M, J, Rr, 32769), (65535, M, 8, 4096, 32768)]:
        assert lib.glowk_projet_workspace_bytes(*args) == 0, args
