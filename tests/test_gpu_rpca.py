"""RPCA on the GPU (csrc/glowk_rpca.h through ``audiosourcesep_amd.rpca``) against the fp64 restatement of tests/rpca_ref.py.

Bars (u = 2^-53).
GEMM: (K + 4) u sum_k |a_ik| |b_kj| per element against the product of the device's own inputs in extended precision: a chain of K
fused multiply-adds, the scaling's rounding, and at most 8 parts of K added in order; the symmetric products are bitwise symmetric.
Eigensolver: residual max |G V - V diag(l)| <= C_RESIDUAL n u ||G||_2 and max |V^T V - I| <= C_ORTH n u.  The plain-loop restatement,
run on the same matrices, reaches 1.87 and 4.88 (its worst ratios over every matrix below); the device gets 4 x those, C_RESIDUAL = 7.5
and C_ORTH = 19.5, because its rounding differs only through the order inside a rotation's updates.  Sweeps: at most 30, and the
restatement's within one.
SVT and one iteration: max |dL| <= C_SVT (rows + frames) u max(1, ||A||_2 / tau) ||A||_2 against the restatement's SVD route fed the
device's own inputs.  The restatement's own Gram route (Jacobi loops) against its SVD route over these shapes, at the start of a
chain and ten iterations in, reaches 0.16 of (rows + frames) u max(1, ||A||_2 / tau); the device gets 4 x that, C_SVT = 0.64.  S and
Y of the iteration follow L: S and A are three elementwise roundings each, Y moves by mu dL.
Chain: never element by element; exact recovery of the scenes to 1e-5 within 40 iterations.  Masks: bitwise.  Audio: 1e-5 of the
mixture's peak, the bar of tests/test_gpu_hpss.py for the same property."""
import functools
import math
import wave

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, audio, hpss, rpca
from audiosourcesep_amd.audio import _p, _s
from tests import rpca_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
C_RESIDUAL, C_ORTH, C_SVT = 7.5, 19.5, 0.64
# (nsig, rows, frames): degenerate sizes; the 16-wide MFMA tile edge, the K = 4 edge and odd n with its bye; frames < rows (a
# rank-deficient Gram matrix); more than one 64 x 64 tile in every dimension
SHAPES = [(1, 1, 1), (1, 2, 3), (1, 5, 1), (2, 16, 12), (1, 17, 40), (3, 33, 80), (1, 48, 20), (1, 65, 203), (1, 130, 67)]
GEMM_SHAPES = SHAPES + [(1, 17, 1100)]      # and K above 1024: two parts of K, added by the second launch


def ident(shape):
    return "%dx%dx%d" % shape


def scene32(rows, frames, seed=0):
    Lt, St = R.scene(rows, frames, seed=seed)
    return (Lt + St).astype(np.float32)


def batch32(nsig, rows, frames):
    return np.stack([scene32(rows, frames, seed) for seed in range(nsig)])


def exact_product(a, b):
    return (a.astype(np.longdouble) @ b.astype(np.longdouble))


# ---- 1. the three products ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=ident)
def test_gemm_one_product_at_a_time(shape):
    nsig, rows, frames = shape
    rng = np.random.default_rng(rows * 1000 + frames)
    A = rng.standard_normal((nsig, rows, frames))
    V = rng.standard_normal((nsig, rows, rows))
    g = rng.random((nsig, rows))
    g[:, ::3] = 0.0
    P = rng.standard_normal((nsig, rows, rows))
    Ad, Vd, gd, Pd = (torch.from_numpy(x).cuda() for x in (A, V, g, P))
    G, S, L = rpca.gram(Ad), rpca.scaled_gram(Vd, gd), rpca.matmul(Pd, Ad)
    assert G.dtype == S.dtype == L.dtype == torch.float64 and tuple(G.shape) == tuple(S.shape) == (nsig, rows, rows) and tuple(L.shape) == A.shape
    assert torch.equal(G, G.transpose(-1, -2)) and torch.equal(S, S.transpose(-1, -2))
    worst = []
    for sig in range(nsig):
        Vg = g[sig][None, :] * V[sig]                                                    # rounded once, as the kernel's scale_k a_jk
        for got, a, b, K in ((G, A[sig], A[sig].T, frames), (S, V[sig], Vg.T, rows), (L, P[sig], A[sig], rows)):
            want = exact_product(a, b)
            bar = (K + 4) * U * (np.abs(a) @ np.abs(b))
            err = np.abs(got[sig].cpu().numpy().astype(np.longdouble) - want).astype(np.float64)
            assert (err <= bar).all(), (sig, K, float((err / np.maximum(bar, 1e-300)).max()))
            worst.append(float((err / np.maximum(bar, 1e-300)).max()))
    print("gemm %s: worst error / bar: gram %.3f, scaled %.3f, apply %.3f" % (ident(shape), max(worst[0::3]), max(worst[1::3]), max(worst[2::3])))
    assert torch.equal(rpca.gram(Ad[0]), G[0]) and torch.equal(rpca.matmul(Pd[0], Ad[0]), L[0])      # [rows, F] is the batch of one


# ---- 2. the eigensolver --------------------------------------------------------------------------------------------------------------------
EIGH_SIZES = [1, 2, 5, 16, 17, 33, 48, 65, 130]


def eigh_matrices(n):
    """Random symmetric, repeated eigenvalues (2, -1, 0), the zero matrix, a diagonal matrix, a rank-1 matrix, a Gram matrix of
    fewer columns than rows.  From 65 up only the first and the last two: the restatement's loops take seconds there."""
    rng = np.random.default_rng(100 + n)
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    sym = lambda d: ((Q * d) @ Q.T + ((Q * d) @ Q.T).T) / 2
    B = rng.standard_normal((n, max(1, n // 3)))
    out = [sym(rng.standard_normal(n)), sym(np.repeat([2.0, -1.0, 0.0], -(-n // 3))[:n]), np.zeros((n, n)), np.diag(rng.standard_normal(n)),
           sym(np.r_[3.0, np.zeros(n - 1)]), B @ B.T]
    return out if n < 65 else [out[0], out[4], out[5]]


@functools.lru_cache(maxsize=None)
def eigh_reference(n):
    return [R.jacobi(G) for G in eigh_matrices(n)]


@pytest.mark.parametrize("n", EIGH_SIZES)
def test_eigh_residual_orthogonality_and_sweeps(n):
    mats = eigh_matrices(n)
    l, V, sweeps, status = rpca.eigh(np.stack(mats), return_status=True)
    assert l.dtype == V.dtype == torch.float64 and sweeps.dtype == status.dtype == torch.int32
    l, V, sweeps, status = l.cpu().numpy(), V.cpu().numpy(), sweeps.cpu().numpy(), status.cpu().numpy()
    worst = [0.0] * 4
    for k, (G, ref) in enumerate(zip(mats, eigh_reference(n))):
        lr, Vr, sr, capped = ref
        n2 = np.abs(np.linalg.eigvalsh(G)).max()
        assert not capped and status[k] == 0 and 1 <= sweeps[k] <= 30 and abs(int(sweeps[k]) - sr) <= 1, (k, sweeps[k], sr)
        assert (np.diff(l[k]) >= 0).all() and np.abs(l[k] - np.linalg.eigvalsh(G)).max() <= C_RESIDUAL * n * n * U * n2
        res, orth = np.abs(G @ V[k] - V[k] * l[k]).max(), np.abs(V[k].T @ V[k] - np.eye(n)).max()
        assert res <= C_RESIDUAL * n * U * n2 and orth <= C_ORTH * n * U, (k, res / (n * U * max(n2, 1e-300)), orth / (n * U))
        if n2 > 0:
            worst[0], worst[2] = max(worst[0], res / (n * U * n2)), max(worst[2], np.abs(G @ Vr - Vr * lr).max() / (n * U * n2))
        worst[1], worst[3] = max(worst[1], orth / (n * U)), max(worst[3], np.abs(Vr.T @ Vr - np.eye(n)).max() / (n * U))
        if np.array_equal(G, np.diag(np.diag(G))):                                       # no work: one sweep that rotates nothing
            assert sweeps[k] == 1 and np.array_equal(l[k], np.sort(np.diag(G))) and np.array_equal(np.abs(V[k]).sum(0), np.ones(n))
    print("eigh n = %d: residual %.2f (restatement %.2f) of n u ||G||_2, orthogonality %.2f (restatement %.2f) of n u" % (n, worst[0], worst[2], worst[1], worst[3]))
    one = rpca.eigh(mats[0])
    assert len(one) == 3 and np.array_equal(one[0].cpu().numpy(), l[0]) and np.array_equal(one[1].cpu().numpy(), V[0]) and int(one[2]) == sweeps[0]


# ---- 3. one SVT and one whole iteration --------------------------------------------------------------------------------------------------
def staged_chain(M32, n_iter, gain=1.0):
    """The chain by hand on one signal [rows, frames] (float32 tensor on the GPU, not silent): ``rpca.spectral_norm``, ``rpca.shrink``,
    ``rpca.svt`` and torch's fp64 elementwise arithmetic in the library's order -> the states ``(L, S, Y, mu, A)`` after each
    iteration, the start first (S and A None).  Every division is tensor by tensor: torch turns a division by a Python number into
    a multiplication by its inverse."""
    M = M32.double()
    rows, frames = M.shape
    lam = gain / math.sqrt(max(rows, frames))
    const = lambda v: torch.tensor(v, dtype=torch.float64, device=M.device)
    n2 = rpca.spectral_norm(M32)
    Y = M / torch.maximum(n2, M.abs().max() / const(lam))
    mu = const(1.25) / n2
    mu_bar = mu * 1e7
    L = torch.zeros_like(M)
    states = [(L, None, Y, mu, None)]
    for _ in range(n_iter):
        ym = Y / mu
        S = rpca.shrink((M - L) + ym, lam / float(mu))
        A = (M - S) + ym
        L = rpca.svt(A, const(1.0) / mu)
        Z = (M - L) - S
        Y = Y + mu * Z
        mu = torch.minimum(1.5 * mu, mu_bar)
        states.append((L, S, Y, mu, A))
    return states, lam


@pytest.mark.parametrize("shape", SHAPES, ids=ident)
def test_svt_and_one_iteration_against_the_restatement(shape):
    nsig, rows, frames = shape
    worst = 0.0
    for sig in range(nsig):
        M32 = torch.from_numpy(scene32(rows, frames, sig)).cuda()
        M = M32.double().cpu().numpy()
        states, lam = staged_chain(M32, 11)
        for at in (0, 10):
            L0, Y0, mu = states[at][0].cpu().numpy(), states[at][2].cpu().numpy(), float(states[at][3])
            L1, S1, Y1, mu1, A = (x.cpu().numpy() for x in states[at + 1])
            n2 = np.linalg.norm(A, 2)
            bar = C_SVT * (rows + frames) * U * max(1.0, n2 * mu) * n2
            # the thresholding alone: the restatement's SVD route on the device's own A
            eL = np.abs(L1 - R.svt_svd(A, 1.0 / mu)).max()
            # the whole iteration from the device's (L, Y, mu): S and A are elementwise (three roundings each), L within the bar of
            # its own A, Y moves by mu dL
            wL, wS, wY, wmu, wA, _ = R.step(M, L0, Y0, mu, 1e7 * float(states[0][3]), lam)
            top = np.abs(M).max() + np.abs(L0).max() + np.abs(Y0 / mu).max()
            eS, eA, eL2, eY = np.abs(S1 - wS).max(), np.abs(A - wA).max(), np.abs(L1 - wL).max(), np.abs(Y1 - wY).max()
            assert eS <= 4 * U * top and eA <= 8 * U * top and float(mu1) == wmu, (sig, at, eS / (U * top), eA / (U * top))
            assert eL <= bar and eL2 <= bar + 8 * U * top and eY <= mu * (bar + 16 * U * top) + 4 * U * np.abs(wY).max(), (sig, at, eL / bar, eL2 / bar, eY)
            worst = max(worst, eL / bar * C_SVT)
    print("svt %s: worst |dL| = %.4f of (rows + frames) u max(1, ||A||_2 / tau) ||A||_2 (bar %.2f)" % (ident(shape), worst, C_SVT))


def test_a_silent_signal_gives_zeros_and_a_zero_matrix_thresholds_to_zero():
    Z = np.zeros((2, 9, 14), np.float32)
    L, S, it, status = rpca.rpca_fit(Z, return_status=True)
    assert not L.any() and not S.any() and it.tolist() == [0, 0] and status.tolist() == [0, 0]
    assert not rpca.svt(Z, 0.5).any() and not rpca.shrink(Z, 0.5).any() and not rpca.spectral_norm(Z).any()
    assert np.array_equal(R.svt_svd(Z[0].astype(np.float64), 0.5), np.zeros((9, 14)))


# ---- 4. bitwise self-consistency --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ident)
def test_fit_equals_the_staged_calls_and_repeats_bit_for_bit(shape):
    nsig, rows, frames = shape
    M = torch.from_numpy(batch32(nsig, rows, frames)).cuda()
    L, S, it = rpca.rpca_fit(M, tol=0.0, n_iter=3)
    L2, S2, it2 = rpca.rpca_fit(M, tol=0.0, n_iter=3)
    assert torch.equal(L, L2) and torch.equal(S, S2) and torch.equal(it, it2) and it.tolist() == [3] * nsig
    for sig in range(nsig):
        Ls, Ss = staged_chain(M[sig], 3)[0][3][:2]
        assert torch.equal(L[sig], Ls) and torch.equal(S[sig], Ss), sig


def test_a_batch_gives_what_its_signals_give_alone():
    """Signals that stop after different numbers of iterations, one that never stops within the cap, and a silent one in the middle."""
    rows, frames = 33, 80
    mix = lambda rank, dens, seed: sum(R.scene(rows, frames, rank=rank, dens=dens, seed=seed)).astype(np.float32)
    M = np.stack([mix(3, 0.06, 0), np.zeros((rows, frames), np.float32), mix(1, 0.01, 2), mix(2, 0.03, 1), mix(5, 0.1, 3)])   # the restatement: 13, 0, 8, 11, 14
    L, S, it, status = rpca.rpca_fit(M, tol=1e-4, n_iter=14, return_status=True)
    counts = it.tolist()
    print("iterations of the batch:", counts)
    assert counts[1] == 0 and len(set(counts)) >= 4 and max(counts) == 14 and status.tolist() == [0] * 5
    for sig in range(5):
        Ls, Ss, its, sts = rpca.rpca_fit(M[sig], tol=1e-4, n_iter=14, return_status=True)
        assert torch.equal(L[sig], Ls) and torch.equal(S[sig], Ss) and int(its) == counts[sig] and int(sts) == 0, sig
    # frozen: more iterations allowed change nothing for the signals that had stopped
    L2, S2, it2 = rpca.rpca_fit(M, tol=1e-4, n_iter=16)
    for sig in range(5):
        if counts[sig] < 14:
            assert torch.equal(L[sig], L2[sig]) and torch.equal(S[sig], S2[sig]) and int(it2[sig]) == counts[sig]


# ---- 5. the chain as a whole --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,frames", [(33, 80), (65, 200)])
def test_exact_recovery_of_the_scene(rows, frames):
    Lt, St = R.scene(rows, frames)
    L, S, it, status = rpca.rpca_fit((Lt + St).astype(np.float32), tol=1e-7, n_iter=40, return_status=True)
    L, S = L.cpu().numpy(), S.cpu().numpy()
    eL, eS = np.linalg.norm(L - Lt) / np.linalg.norm(Lt), np.linalg.norm(S - St) / np.linalg.norm(St)
    print("scene %d x %d: %d iterations, ||L - L*|| / ||L*|| = %.2e, ||S - S*|| / ||S*|| = %.2e" % (rows, frames, int(it), eL, eS))
    assert int(it) <= 40 and int(status) == 0 and eL <= 1e-5 and eS <= 1e-5


# ---- 6. masks and audio -----------------------------------------------------------------------------------------------------------------------
def test_masks_and_masked_spectra():
    rows, frames = 33, 80
    rng = np.random.default_rng(9)
    M = batch32(2, rows, frames)
    X = (M * np.exp(1j * rng.uniform(-np.pi, np.pi, M.shape))).astype(np.complex64)
    b, f, model = rpca.rpca(X, n_iter=6, kind="binary", gain_mask=1.5, return_model=True)
    L, S = model["L"], model["S"]
    want = R.binary_mask(L.cpu().numpy(), S.cpu().numpy(), 1.5)
    mb, mf = rpca.masks(L, S, kind="binary", gain_mask=1.5)
    assert np.array_equal(mf.cpu().numpy(), want) and np.array_equal(mb.cpu().numpy(), 1.0 - want) and 0 < want.mean() < 1
    assert np.array_equal(f.cpu().numpy(), want * X) and np.array_equal(b.cpu().numpy(), (1.0 - want) * X)
    assert torch.equal(b + f, torch.from_numpy(X).cuda())                              # a binary pair returns the mixture exactly
    mb2, mf2 = rpca.rpca(X, n_iter=6, kind="binary", gain_mask=1.5, mask=True)
    assert torch.equal(mb2, mb) and torch.equal(mf2, mf)
    # the soft pair is hpss's mask kernel on |L| and |S| rounded to float32
    for power, margin in ((2.0, 1.0), (1.0, (2.0, 1.5))):
        sb, sf = rpca.masks(L, S, power=power, margin=margin)
        mh, mp = hpss._pair(margin, "margin")
        a32, b32 = L.abs().float().contiguous(), S.abs().float().contiguous()
        wb, wf = torch.empty_like(a32), torch.empty_like(a32)
        _lib.check(_lib.load().glowk_hpss_mask(_p(a32), _p(b32), None, a32.numel(), power, mh, mp, _p(wb), _p(wf), _s(a32)))
        assert torch.equal(sb, wb) and torch.equal(sf, wf)
    # background plus foreground return the mixture's STFT: the masks add up to one within the mask bar (1e-6 each)
    cb, cf = rpca.rpca(X, n_iter=6)
    assert cb.dtype == torch.complex64 and tuple(cb.shape) == X.shape
    assert float((cb + cf - torch.from_numpy(X).cuda()).abs().max()) <= 2e-6 * float(np.abs(X).max())
    rb, rf = rpca.rpca(np.abs(X), n_iter=6)
    assert rb.dtype == torch.float32 and float((cb.abs() - rb).abs().max()) <= 1e-6 * float(np.abs(X).max())


N_AUDIO = 8192
AUDIO_BAR = 1e-5


def test_separate_wav_rpca_returns_the_files_rate_and_length(tmp_path):
    """Two iterations keep the 1025-row solves short; the stems' sum does not depend on how far the chain got."""
    rate = 22050
    t = np.arange(N_AUDIO) / rate
    y = 0.4 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 1330.0 * t) * (np.sin(2 * np.pi * 3.0 * t) > 0.6)
    q = np.rint(np.clip(y, -1.0, 1.0) * 32767.0).astype("<i2")
    path = tmp_path / "mono.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(q.tobytes())
    stems, out_rate = rpca.separate_wav_rpca(str(path), n_iter=2)
    assert out_rate == rate and tuple(stems.shape) == (2, N_AUDIO) and stems.dtype == torch.float32 and bool(torch.isfinite(stems).all())
    yq = torch.from_numpy(q.astype(np.float32) / 32768.0).cuda()
    trip = audio.resample(audio.resample(yq, rate, audio.SR), audio.SR, rate)[:N_AUDIO]
    peak = float(yq.abs().max())
    err = float((stems.double().sum(0) - trip.double()).abs().max()) / peak
    print("separate_wav_rpca: background + foreground - round trip = %.2e of the peak" % err)
    assert err <= AUDIO_BAR and float(stems.abs().max()) > 0.05
    stems, out_rate = rpca.separate_wav_rpca(str(path), out_rate=None, n_iter=1, kind="binary", residual=True)
    assert out_rate == audio.SR and tuple(stems.shape) == (3, -(-N_AUDIO * audio.SR // rate))
