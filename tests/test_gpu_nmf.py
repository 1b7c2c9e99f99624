"""NMF on the GPU (csrc/glowk_nmf.h through ``audiosourcesep_amd.nmf``) against the fp64 restatement of tests/nmf_ref.py.

The design keeps the comparison from being chaotic: a device result is compared with the restatement one update at a time, each
fed the device's own inputs; runs of several iterations are checked for bitwise self-consistency and for descent, never element by
element against fp64.

Bars (derived in tests/nmf_ref.py, u = 2^-24; where the restatement is zero the device must be zero):
  one update   |dev - ref| <= (3 K + 2 n + 16) u ref per element, n = rows for H, frames for W
  divergence   |dev - ref| <= (K + 4) u sum(w), w = (V + L)^2, V + L, q + 1 for beta 2, 1, 0
  masks        |dev - ref| <= power (2 K + 2 S + 8) u absolute; the masks of a cell add up to 1 within 4 S u; spectra: the bar |X|

Measured on an MI355X (largest |dev - ref| / bar per shape): see the table in DESIGN section 22."""
import functools
import wave

import numpy as np
import pytest
import torch

from audiosourcesep_amd import nmf
from tests import nmf_ref as N

pytestmark = pytest.mark.gpu

IDS = lambda s: "-".join(map(str, s))


@functools.lru_cache(maxsize=None)
def problem(shape):
    """(V, W0, H0) of a shape: V from the restatement's generator, the start from ``nmf.init`` (device RNG), all read-only numpy."""
    nsig, rows, frames, K = shape
    V = N.spectra(((nsig,) if nsig != 1 else ()) + (rows, frames), 1000 * rows + frames)
    W, H = nmf.init(V.copy(), K, seed=5)
    out = V, W.cpu().numpy(), H.cpu().numpy()
    for a in out:
        a.setflags(write=False)
    return out


def worst_ratio(dev, ref, bar):
    """The largest |dev - ref| / (bar ref); where ref is 0 the device must be 0."""
    assert dev.shape == ref.shape and dev.dtype == np.float32 and np.isfinite(dev).all()
    zero = ref == 0
    assert not dev[zero].any()
    if zero.all():
        return 0.0
    return float((np.abs(dev[~zero].astype(np.float64) - ref[~zero]) / (bar * ref[~zero])).max())


def test_init_is_the_device_rng_scaled():
    from tests import rng_ref
    V = N.spectra((2, 9, 21), 3)
    W, H = nmf.init(V.copy(), 4, seed=7)
    assert W.is_cuda and W.dtype == torch.float32 and tuple(W.shape) == (2, 9, 4) and tuple(H.shape) == (2, 4, 21)
    scale = torch.sqrt(torch.from_numpy(V.copy()).cuda().double().mean(dim=(-2, -1), keepdim=True) / 4).float().cpu().numpy()
    uw = rng_ref.uniform(7, step=0, which=nmf.NMF_STREAM, n=W.numel()).reshape(2, 9, 4)
    uh = rng_ref.uniform(7, step=1, which=nmf.NMF_STREAM, n=H.numel()).reshape(2, 4, 21)
    assert uw.min() > 0 and np.array_equal(W.cpu().numpy(), uw * scale) and np.array_equal(H.cpu().numpy(), uh * scale)
    assert abs(float(scale[0, 0, 0]) - np.sqrt(V[0].mean() / 4)) <= 1e-6 * float(scale[0, 0, 0])


@pytest.mark.parametrize("beta", N.BETAS)
@pytest.mark.parametrize("shape", N.SHAPES, ids=IDS)
def test_one_update_against_the_restatement(shape, beta):
    """Each update is fed the device's own inputs: at the start, and at the point two device iterations later."""
    nsig, rows, frames, K = shape
    V, W, H = problem(shape)
    worst_h = worst_w = 0.0
    for stage in range(2):
        dw = nmf.update_w(V.copy(), W.copy(), H.copy(), beta)
        dh = nmf.update_h(V.copy(), W.copy(), H.copy(), beta)
        assert dw.is_cuda and dw.dtype == torch.float32 and tuple(dw.shape) == W.shape and tuple(dh.shape) == H.shape
        worst_w = max(worst_w, worst_ratio(dw.cpu().numpy(), N.update_w(V, W, H, beta), N.update_bar(K, frames)))
        worst_h = max(worst_h, worst_ratio(dh.cpu().numpy(), N.update_h(V, W, H, beta), N.update_bar(K, rows)))
        if stage == 0:
            W, H = (t.cpu().numpy() for t in nmf.fit(V.copy(), W.copy(), H.copy(), beta, 2))
    print("nmf update %s beta %d: worst |dev - ref| / bar: W %.3f, H %.3f" % (shape, beta, worst_w, worst_h))
    assert worst_w <= 1.0 and worst_h <= 1.0


@pytest.mark.parametrize("beta", N.BETAS)
@pytest.mark.parametrize("shape", N.SHAPES, ids=IDS)
def test_divergence_against_the_restatement(shape, beta):
    nsig, rows, frames, K = shape
    V, W, H = problem(shape)
    d = nmf.divergence(V.copy(), W.copy(), H.copy(), beta)
    assert d.is_cuda and d.dtype == torch.float64 and tuple(d.shape) == V.shape[:-2]
    ref, bar = N.divergence(V, W, H, beta), N.divergence_bar(K, N.divergence_weight(V, W, H, beta))
    ratio = N.ratio(np.abs(d.cpu().numpy() - ref), bar)
    print("nmf divergence %s beta %d: worst |dev - ref| / bar: %.3f" % (shape, beta, ratio))
    assert ratio <= 1.0
    assert torch.equal(d, nmf.divergence(torch.from_numpy(V.copy()).cuda(), W.copy(), H.copy(), beta))
    if nsig > 1:                                                                    # a signal of a batch, alone; one shared dictionary
        assert torch.equal(nmf.divergence(V[1].copy(), W[1].copy(), H[1].copy(), beta), d[1])
        shared = nmf.divergence(V.copy(), W[0].copy(), H.copy(), beta)
        assert torch.equal(shared[1], nmf.divergence(V[1].copy(), W[0].copy(), H[1].copy(), beta)) and torch.equal(shared[0], d[0])


@pytest.mark.parametrize("power", (1, 2))
@pytest.mark.parametrize("shape", N.SHAPES, ids=IDS)
def test_masks_against_the_restatement(shape, power):
    nsig, rows, frames, K = shape
    V, W, H = problem(shape)
    worst = 0.0
    for sizes in {(K,), tuple([1] * min(K, 16))[:-1] + (K - min(K, 16) + 1,), (K // 3, K - K // 3) if K >= 3 else (K,)}:
        S = len(sizes)
        rng = np.random.default_rng(K + S)
        X = (rng.standard_normal(V.shape[:-2] + (2,) + V.shape[-2:]) + 1j * rng.standard_normal(V.shape[:-2] + (2,) + V.shape[-2:])).astype(np.complex64)
        m, spec = nmf.masks(W.copy(), H.copy(), list(sizes), power, X.copy())
        assert m.dtype == torch.float32 and tuple(m.shape) == V.shape[:-2] + (S, rows, frames)
        assert spec.dtype == torch.complex64 and tuple(spec.shape) == V.shape[:-2] + (S, 2, rows, frames)
        assert torch.equal(m, nmf.masks(W.copy(), H.copy(), list(sizes), power))
        m, spec = m.cpu().numpy(), spec.cpu().numpy()
        ref = N.masks(W, H, sizes, power)
        bar = N.mask_bar(K, S, power)
        assert np.isfinite(m).all() and np.abs(m.astype(np.float64).sum(axis=-3) - 1.0).max() <= N.mask_sum_bar(S)
        worst = max(worst, float(np.abs(m - ref).max() / bar))
        want = ref[..., :, None, :, :] * X[..., None, :, :, :].astype(np.complex128)
        assert (np.abs(spec - want) <= bar * np.abs(X[..., None, :, :, :]) + 1e-30).all()
        mono, sm = nmf.masks(W.copy(), H.copy(), list(sizes), power, X[..., 0, :, :].copy())
        assert tuple(sm.shape) == V.shape[:-2] + (S, rows, frames) and np.array_equal(sm.cpu().numpy(), spec[..., 0, :, :])
    print("nmf masks %s power %d: worst |dev - ref| / bar: %.3f" % (shape, power, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("beta", N.BETAS)
@pytest.mark.parametrize("shape", N.SHAPES[1:4] + N.SHAPES[5:6], ids=IDS)
def test_chains_are_bitwise_consistent(shape, beta):
    nsig, rows, frames, K = shape
    V, W, H = problem(shape)
    n = 3
    Wn, Hn = nmf.fit(V.copy(), W.copy(), H.copy(), beta, n)
    w1, h1 = torch.from_numpy(W.copy()), torch.from_numpy(H.copy())
    w2, h2 = w1, h1
    for _ in range(n):
        w1, h1 = nmf.fit(V.copy(), w1, h1, beta, 1)
        w2 = nmf.update_w(V.copy(), w2, h2, beta)
        h2 = nmf.update_h(V.copy(), w2, h2, beta)
    assert torch.equal(Wn, w1) and torch.equal(Hn, h1) and torch.equal(Wn, w2) and torch.equal(Hn, h2)
    dV, dW, dH = (torch.from_numpy(a.copy()).cuda() for a in (V, W, H))
    keep = dW.clone(), dH.clone()
    Wd, Hd = nmf.fit(dV, dW, dH, beta, n)                                           # a second run, from device tensors, which stay
    assert torch.equal(Wn, Wd) and torch.equal(Hn, Hd) and torch.equal(dW, keep[0]) and torch.equal(dH, keep[1])
    assert not torch.equal(Wn, dW) and not torch.equal(Hn, dH)
    if nsig > 1:                                                                    # every signal of a batch alone
        for i in range(nsig):
            wi, hi = nmf.fit(V[i].copy(), W[i].copy(), H[i].copy(), beta, n)
            assert torch.equal(wi, Wn[i]) and torch.equal(hi, Hn[i])
        ws, hs = nmf.fit(V.copy(), W[0].copy(), H.copy(), beta, n, update_w=False)  # one shared dictionary, H alone moves
        assert tuple(ws.shape) == W[0].shape and np.array_equal(ws.cpu().numpy(), W[0])
        for i in range(nsig):
            assert torch.equal(nmf.fit(V[i].copy(), W[0].copy(), H[i].copy(), beta, n, update_w=False)[1], hs[i])


@pytest.mark.parametrize("beta", N.BETAS)
@pytest.mark.parametrize("shape", N.SHAPES[1:], ids=IDS)
def test_descent_over_30_iterations(shape, beta):
    """The fp64 divergence of the device's (W, H) after every iteration never rises by more than the divergence bar."""
    nsig, rows, frames, K = shape
    V = problem(shape)[0]
    if beta == 0:
        V = np.maximum(V, np.float32(1e-3))
    W, H = nmf.init(V.copy(), K, seed=5)
    dV = torch.from_numpy(V.copy()).cuda()
    states = [(W, H)]
    for _ in range(30):
        states.append(nmf.fit(dV, states[-1][0], states[-1][1], beta, 1))
    host = [(w.cpu().numpy(), h.cpu().numpy()) for w, h in states]
    D = np.array([np.atleast_1d(N.divergence(V, w, h, beta)) for w, h in host])      # [31, nsig]
    bar = np.array([np.atleast_1d(N.divergence_bar(K, N.divergence_weight(V, w, h, beta))) for w, h in host])
    rise = D[1:] - D[:-1]
    print("nmf descent %s beta %d: D %.6e -> %.6e, largest rise / bar %.3f" % (shape, beta, D[0].sum(), D[-1].sum(), N.ratio(np.maximum(rise, 0), bar[1:])))
    assert np.isfinite(D).all() and (rise <= bar[1:]).all() and (D[-1] < D[0]).all()


@pytest.mark.parametrize("beta", N.BETAS)
def test_defined_edges(beta):
    nsig, rows, frames, K = 1, 33, 95, 5
    V, W, H = (a.copy() for a in problem((nsig, rows, frames, K)))
    V[:, 7] = 0.0
    W[:, 2] = 0.0
    h = nmf.update_h(V, W, H, beta).cpu().numpy()
    assert np.isfinite(h).all() and not h[2].any() and h[[0, 1, 3, 4]].any(axis=1).all()      # a zero atom: a zero row of H'
    assert not h[:, 7].any()                                                        # a silent frame: a zero column of H' (for beta 0, too: Q = 0)
    for n_iter in (0,):
        w0, h0 = nmf.fit(V, W, H, beta, n_iter)
        assert np.array_equal(w0.cpu().numpy(), W) and np.array_equal(h0.cpu().numpy(), H)
    e = lambda *s: np.zeros(s, np.float32)
    w0, h0 = nmf.fit(e(0, rows, frames), e(0, rows, K), e(0, K, frames), beta, 3)    # nsig = 0
    assert tuple(w0.shape) == (0, rows, K) and tuple(h0.shape) == (0, K, frames) and tuple(nmf.divergence(e(0, 4, 6), e(0, 4, 2), e(0, 2, 6), beta).shape) == (0,)
    Hz = H.copy()
    Hz[:, 11] = 0.0                                                                 # every Lambda_s = 0 in frame 11: the mask is 1 / S
    m = nmf.masks(W, Hz, [2, 2, 1]).cpu().numpy()
    assert (m[:, :, 11] == np.float32(1.0 / 3)).all() and tuple(nmf.masks(e(0, rows, K), e(0, K, frames), [2, 3]).shape) == (0, 2, rows, frames)
    for shape in N.SHAPES:                                                          # no NaN or Inf after ten iterations at any shape
        Vs, Ws, Hs = problem(shape)
        wn, hn = nmf.fit(Vs.copy(), Ws.copy(), Hs.copy(), beta, 10)
        assert bool(torch.isfinite(wn).all()) and bool(torch.isfinite(hn).all()) and bool((wn >= 0).all()) and bool((hn >= 0).all())


def test_decompose_and_learn_dictionary():
    V = problem((1, 33, 95, 5))[0]
    comps, acts = nmf.decompose(V.copy(), 5, beta=1, n_iter=20, seed=5)
    assert tuple(comps.shape) == (33, 5) and tuple(acts.shape) == (5, 95)
    W0, H0 = problem((1, 33, 95, 5))[1:]
    want = nmf.fit(V.copy(), W0.copy(), H0.copy(), 1, 20)
    assert torch.equal(comps, want[0]) and torch.equal(acts, want[1]) and torch.equal(nmf.learn_dictionary(V.copy(), 5, 1, 20, 5), comps)
    assert float(N.divergence(V, comps.cpu().numpy(), acts.cpu().numpy(), 1)) < float(N.divergence(V, W0, H0, 1))


def test_separation_with_the_true_dictionaries():
    X, Ws, mags = N.two_sources()
    m, spec, model = nmf.nmf_separate(X.copy(), [w.copy() for w in Ws], beta=1, n_iter=50, power=1, seed=0, return_model=True)
    assert tuple(m.shape) == (2,) + X.shape and tuple(spec.shape) == (2,) + X.shape and spec.dtype == torch.complex64
    W, H = model["W"].cpu().numpy(), model["H"].cpu().numpy()
    assert np.array_equal(W, np.concatenate(Ws, axis=1)) and np.allclose(model["V"].cpu().numpy(), np.abs(X), rtol=1e-6, atol=0)
    ref = N.masks(W, H, [5, 4], 1)
    bar = N.mask_bar(9, 2, 1)
    m, spec = m.cpu().numpy(), spec.cpu().numpy()
    print("nmf separation: worst mask |dev - ref| / bar %.3f" % float(np.abs(m - ref).max() / bar))
    assert (np.abs(m - ref) <= bar).all()
    assert (np.abs(spec - ref * X.astype(np.complex128)) <= bar * np.abs(X) + 1e-30).all()
    for s in range(2):
        own, other = np.linalg.norm(np.abs(spec[s]) - mags[s]), np.linalg.norm(np.abs(spec[s]) - mags[1 - s])
        print("nmf separation: source %d is %.3e from its own magnitude, %.3e from the other" % (s, own, other))
        assert own < other
    # stereo and a batch: the mean magnitude drives H, every channel is masked
    X2 = np.stack([X, 0.5 * X])
    m2, spec2 = nmf.nmf_separate(X2.copy(), Ws, n_iter=5)
    assert tuple(m2.shape) == (2,) + X.shape and tuple(spec2.shape) == (2, 2) + X.shape
    mb, sb = nmf.nmf_separate(np.stack([X2, X2[::-1]]), Ws, n_iter=5)
    assert tuple(mb.shape) == (2, 2) + X.shape and tuple(sb.shape) == (2, 2, 2) + X.shape
    assert torch.allclose(mb[0], m2, atol=1e-4)                                        # (the second signal starts from other draws)


def _dictionaries(seed, sizes=(3, 2)):
    rng = np.random.default_rng(seed)
    return [rng.random((1025, k)).astype(np.float32) + 0.01 for k in sizes]


@pytest.mark.parametrize("channels", (1, 2))
def test_audio_stems_add_up_to_the_input(channels):
    rng = np.random.default_rng(channels)
    n = 5000
    y = (0.3 * rng.standard_normal((channels, n))).astype(np.float32)
    y = y[0] if channels == 1 else y
    stems, rest = nmf.nmf_audio(y.copy(), _dictionaries(1), n_iter=5, residual=True)
    assert stems.is_cuda and tuple(stems.shape) == (2,) + y.shape and tuple(rest.shape) == y.shape
    err = float(np.abs(stems.sum(0).cpu().numpy() - y).max())
    print("nmf_audio %d channel(s): |sum of stems - y| = %.3e of the peak" % (channels, err / np.abs(y).max()))
    assert err <= 1e-5 * np.abs(y).max() and float(rest.abs().max()) <= 1e-5 * np.abs(y).max()
    assert torch.equal(nmf.nmf_audio(y.copy(), _dictionaries(1), n_iter=5), stems)


def _write_wav(path, y, rate):
    pcm = np.clip(np.round(np.atleast_2d(y).T * 32767), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


def test_separate_wav_nmf(tmp_path):
    rng = np.random.default_rng(4)
    rate, n = 22050, 7001
    t = np.arange(n) / rate
    tone, noise = 0.3 * np.sin(2 * np.pi * 440 * t), 0.1 * rng.standard_normal(n)
    _write_wav(tmp_path / "mix.wav", tone + noise, rate)
    _write_wav(tmp_path / "tone.wav", tone, rate)
    stems, out_rate = nmf.separate_wav_nmf(str(tmp_path / "mix.wav"), [str(tmp_path / "tone.wav"), _dictionaries(2, (4,))[0]], n_components=3,
                                           dictionary_iter=10, n_iter=10)
    assert out_rate == rate and tuple(stems.shape) == (2, n) and bool(torch.isfinite(stems).all())
    _write_wav(tmp_path / "stereo.wav", np.stack([tone + noise, tone - noise]), rate)
    stems, out_rate = nmf.separate_wav_nmf(str(tmp_path / "stereo.wav"), _dictionaries(3), out_rate=None, n_iter=3, residual=True)
    assert out_rate == 16000 and tuple(stems.shape[:2]) == (3, 2) and abs(stems.shape[2] - n * 16000 / rate) <= 2
