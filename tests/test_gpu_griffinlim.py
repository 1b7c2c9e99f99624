"""Griffin-Lim and the `whole` inversion on the GPU (csrc/glowk_audio.h through audiosourcesep_amd/audio.py) against the fp64
oracle of tests/griffinlim_ref.py, fed the same magnitudes and the same start phases."""
import math
import os

import numpy as np
import pytest
import torch

from audiosourcesep_amd import audio, basis
from audiosourcesep_amd.flow_models.flow_builder import build_glow
from tests import audio_ref as R
from tests import griffinlim_ref as G

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEL = dict(data_type="melspec", minval=-100.0, maxval=20.0, use_logit=False)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def random_phases(shape, seed):
    u = np.random.default_rng(seed).uniform(0.0, 1.0, shape)
    return np.exp(2j * np.pi * u).astype(np.complex64)


@pytest.fixture(scope="module")
def mags():
    """sqrt(NNLS) of the 4 real gt1 tiles: [4, 1025, 64] float32 on the GPU, as mel_to_audio computes it."""
    t = np.load(os.path.join(GOLDEN, "real_mel_tiles.npz"))["gt1"].astype(np.float32)
    return torch.sqrt(audio.mel_to_power(torch.from_numpy(t).cuda(), 200))


@pytest.mark.parametrize("method", ["frame", "whole"])
def test_against_the_oracle_with_the_same_start(mags, method):
    S = mags if method == "frame" else mags.permute(1, 0, 2).reshape(1, 1025, -1).contiguous()
    init = random_phases(tuple(S.shape), 7)
    Sn = S.cpu().numpy().astype(np.float64)
    assert Sn.shape[-1] == (64 if method == "frame" else 256)
    worst = {}
    sc = {}
    for n_iter in (0, 1, 4, 32):
        y = audio.griffinlim(S, n_iter=n_iter, init=torch.from_numpy(init).cuda()).cpu().numpy()
        assert y.shape == (S.shape[0], (S.shape[2] - 1) * 512)
        errs = []
        for i in range(S.shape[0]):
            ref = G.griffinlim(Sn[i], n_iter=n_iter, init=init[i])
            errs.append(rel(y[i], ref))
            sc.setdefault(n_iter, []).append((G.spectral_convergence(y[i], Sn[i]), G.spectral_convergence(ref, Sn[i])))
        worst[n_iter] = max(errs)
    print("Griffin-Lim (%s) vs fp64 oracle, relative L2 by n_iter: %s; spectral convergence (gpu, oracle) at 0 / 32: %s / %s"
          % (method, {k: "%.2e" % v for k, v in worst.items()}, sc[0], sc[32]))
    assert max(worst[0], worst[1], worst[4]) <= 2e-5
    assert worst[32] <= 2e-3
    assert max(abs(g - o) for g, o in sc[32]) <= 1e-3
    for (g0, _), (g32, _) in zip(sc[0], sc[32]):            # convergence: 32 iterations cut the spectral distance by >= 30 %
        assert g32 <= 0.7 * g0


@pytest.mark.parametrize("F", [4, 37, 161])
def test_frame_counts_off_the_tile_grid(F):
    """Partial 32-frame tiles of both kernels, the shortest signal (4 frames, 1536 samples) and no momentum.  The magnitudes are
    those of real audio: random ones make an inconsistent spectrum on which R - beta P cancels in some bins, and the fp64 oracle
    itself then moves by 36x a 6e-8 perturbation of its inputs at F = 4."""
    pcm = np.load(os.path.join(GOLDEN, "real_audio_excerpt.npz"))["pcm"].astype(np.float64).reshape(-1) / 32768.0
    n = (F - 1) * 512
    S = np.stack([np.abs(R.stft(pcm[o:o + n])) for o in (0, 50000)]).astype(np.float32)
    init = random_phases(S.shape, F)
    for momentum in (0.0, 0.99):
        y = audio.griffinlim(torch.from_numpy(S).cuda(), n_iter=3, momentum=momentum, init=torch.from_numpy(init).cuda()).cpu().numpy()
        assert y.shape == (2, (F - 1) * 512)
        for i in range(2):
            assert rel(y[i], G.griffinlim(S[i], n_iter=3, momentum=momentum, init=init[i])) <= 2e-5


def test_init_forms_and_reproducibility(mags):
    S = mags[:2].contiguous()
    u = basis.device_randn(tuple(S.shape), S.device, seed=5, which=audio.GRIFFINLIM_STREAM, uniform=True)
    y = audio.griffinlim(S, n_iter=4, init="random", seed=5)
    init = torch.exp(2j * math.pi * u.double()).to(torch.complex64)
    for n_iter in (0, 4):
        ref = audio.griffinlim(S, n_iter=n_iter, init=init)
        assert rel(audio.griffinlim(S, n_iter=n_iter, init="random", seed=5).cpu(), ref.cpu()) <= 1e-6
    assert torch.equal(y, audio.griffinlim(S, n_iter=4, init="random", seed=5))
    assert not torch.equal(y, audio.griffinlim(S, n_iter=4, init="random", seed=6))
    ones = torch.ones(S.shape, dtype=torch.complex64, device=S.device)
    for n_iter in (0, 2):
        assert torch.equal(audio.griffinlim(S, n_iter=n_iter, init=None), audio.griffinlim(S, n_iter=n_iter, init=ones))
    # host inputs are moved; a side stream gives the same bits
    assert torch.equal(audio.griffinlim(S.cpu(), n_iter=4, init="random", seed=5), y)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        z = audio.griffinlim(S, n_iter=4, init="random", seed=5)
    s.synchronize()
    assert torch.equal(z, y)


def test_zero_magnitudes_give_zero_audio():
    y = audio.griffinlim(torch.zeros((2, 1025, 40), device="cuda"), n_iter=5)
    assert tuple(y.shape) == (2, 39 * 512) and bool((y == 0).all())


def test_whole_equals_frame_for_one_tile_and_the_oracle_for_many():
    pcm = np.load(os.path.join(GOLDEN, "real_audio_excerpt.npz"))["pcm"].astype(np.float32) / 32768.0
    mel, X = audio.mel_tiles(torch.from_numpy(pcm[:4]).cuda(), return_stft=True)
    t = np.load(os.path.join(GOLDEN, "real_mel_tiles.npz"))
    tiles = [torch.from_numpy(t[k]).cuda() for k in ("gt1", "gt2")]
    for wiener in (False, True):
        one = [x[:1] for x in tiles]
        frame = audio.invert(one, X[:1], wiener=wiener, iters=50)
        whole = audio.invert(one, X[:1], wiener=wiener, iters=50, method="whole")
        assert tuple(whole.shape) == tuple(frame.shape) == (2, 63 * 512)
        assert rel(whole.cpu(), frame.cpu()) <= 1e-6, wiener
        # 4 tiles -> one signal of (4 * 64 - 1) * 512 samples per source
        y = audio.invert(tiles, X, wiener=wiener, iters=50, method="whole").cpu().numpy()
        assert y.shape == (2, 255 * 512)
        P = [G.whole(audio.mel_to_power(x, 50).cpu().numpy().astype(np.float64)) for x in tiles]
        Xw = G.whole(X.cpu().numpy().astype(np.complex128))
        ref = R.masked_istft(P, Xw, wiener=wiener)
        for s in range(2):
            assert rel(y[s], ref[s]) <= 1e-5, (wiener, s)
    # Griffin-Lim 'whole' through invert is griffinlim of the concatenated magnitudes, from the 'random' start of its seed
    g = audio.invert(tiles, algorithm="griffin", method="whole", iters=50, n_iter=4, seed=3)
    S = torch.stack([torch.sqrt(audio.mel_to_power(x, 50)).permute(1, 0, 2).reshape(1025, -1) for x in tiles])
    assert torch.equal(g, audio.griffinlim(S, n_iter=4, seed=3))
    m = audio.mel_to_audio(tiles[0], n_iter=4, seed=3, iters=50, method="whole")
    assert torch.equal(m, audio.griffinlim(S[:1], n_iter=4, seed=3).reshape(-1))
    f = audio.mel_to_audio(tiles[0], n_iter=4, seed=3, iters=50)
    assert tuple(f.shape) == (4 * 63 * 512,)
    assert torch.equal(f, audio.griffinlim(S[0].reshape(1025, 4, 64).permute(1, 0, 2).contiguous(), n_iter=4, seed=3).reshape(-1))


@pytest.fixture(scope="module")
def flows():
    f = np.load(os.path.join(GOLDEN, "basis_real_tiles.npz"))
    out = []
    for i, k in enumerate(("gt1", "gt2")):
        mb = torch.from_numpy(f[k][:8].astype(np.float32))[..., None].cuda()
        out.append(build_glow(mb, [96, 64, 1], L=3, K=2, n_filters=128, learntop=True, seed=40 + i, **MEL))
    return out


def test_separate_audio_griffin_whole(flows):
    pcm = np.load(os.path.join(GOLDEN, "real_audio_excerpt.npz"))["pcm"].astype(np.float32) / 32768.0
    y = pcm[:4].reshape(-1)
    sig = np.array([20.0, 5.0], np.float32)
    kw = dict(T=4, delta=1e-4, seed=9, algorithm="griffin", method="whole")
    y1, y2, mixed, x1, x2 = audio.separate_audio(y, flows[0], flows[1], sig, **kw)
    assert tuple(y1.shape) == tuple(y2.shape) == ((4 * 64 - 1) * 512,)
    assert bool(torch.isfinite(y1).all()) and bool(torch.isfinite(y2).all()) and float(y1.abs().max()) > 0
    r1, r2, *_ = audio.separate_audio(y, flows[0], flows[1], sig, **kw)
    assert torch.equal(r1, y1) and torch.equal(r2, y2)
    h = audio.invert([x1, x2], algorithm="griffin", method="whole", seed=9)
    assert torch.equal(h[0], y1) and torch.equal(h[1], y2)


def test_one_minute_whole_signal():
    """30 tiles as one 1920-frame signal (the reference's sep1.wav / sep2.wav length) at the default 32 iterations."""
    t = np.load(os.path.join(GOLDEN, "real_mel_tiles.npz"))
    tiles = torch.from_numpy(np.concatenate([t["gt1"], t["gt2"], t["mixed"]] * 3)[:30]).cuda()
    y = audio.mel_to_audio(tiles, method="whole")
    assert tuple(y.shape) == ((30 * 64 - 1) * 512,) and bool(torch.isfinite(y).all())
    assert torch.equal(y, audio.mel_to_audio(tiles, method="whole"))


def test_host_pointers_are_refused():
    import ctypes
    from audiosourcesep_amd import _lib
    lib = _lib.load()
    host = np.zeros((1, 1025, 8), np.float32)
    out = torch.empty((1, 7 * 512), device="cuda")
    rc = lib.glowk_griffinlim(ctypes.c_void_p(host.ctypes.data), None, 1, 8, 2, 0.99, ctypes.c_void_p(out.data_ptr()), None)
    assert rc != 0 and b"device memory" in lib.glowk_last_error()
