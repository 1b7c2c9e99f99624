"""The audio ends on the GPU (csrc/glowk_audio.h through audiosourcesep_amd/audio.py) against the fp64 oracle of
tests/audio_ref.py.  Each bound is 5-10x the fp32 error of a CPU emulation of the kernels' arithmetic."""
import os

import numpy as np
import pytest
import torch

from audiosourcesep_amd import audio, basis
from audiosourcesep_amd.flow_models.flow_builder import build_glow
from tests import audio_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEL = dict(data_type="melspec", minval=-100.0, maxval=20.0, use_logit=False)


def excerpt():
    return np.load(os.path.join(GOLDEN, "real_audio_excerpt.npz"))["pcm"].astype(np.float32) / 32768.0


def synthetic():
    rng = np.random.default_rng(5)
    t = np.arange(R.EXTRACT) / 16000.0
    tones = 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 1234.5 * t) + 0.1 * np.sin(2 * np.pi * 5000.0 * t)
    chirp = 0.2 * np.sin(2 * np.pi * (100.0 * t + 0.5 * 3500.0 * t * t / 2.04))
    mixed = tones + chirp + 0.01 * rng.standard_normal(R.EXTRACT)
    square = np.where(np.sin(2 * np.pi * 220.0 * t) >= 0, 1.0, -1.0)
    return np.stack([mixed, np.zeros(R.EXTRACT), square]).astype(np.float32)


@pytest.mark.parametrize("top_db", [80.0, None])
def test_front_end_against_the_oracle(top_db):
    y = np.concatenate([excerpt(), synthetic()])
    mel, X = audio.mel_tiles(torch.from_numpy(y).cuda(), top_db=top_db, return_stft=True)
    assert tuple(mel.shape) == (9, 96, 64, 1) and tuple(X.shape) == (9, 1025, 64) and X.dtype == torch.complex64
    mel, X = mel[..., 0].cpu().numpy(), X.cpu().numpy()
    worst_db, worst_x = 0.0, 0.0
    for i in range(len(y)):
        L, Xr = R.mel_db(y[i].astype(np.float64), top_db=top_db, return_stft=True)
        worst_db = max(worst_db, float(np.abs(mel[i] - L).max()))
        worst_x = max(worst_x, float(np.abs(X[i] - Xr).max() / max(np.abs(Xr).max(), 1e-30)))
        if top_db and mel[i].max() < 20.0:
            floor = mel[i].max() - np.float32(80.0)
            assert mel[i].min() >= floor
            active = L < L.max() - 80.0 - 0.01
            assert (mel[i][active] == floor).all()
    print("front end vs fp64 oracle (top_db %s): mel max |d| %.2e dB, STFT max |d| %.2e of max |X|" % (top_db, worst_db, worst_x))
    assert worst_db <= 2e-3 and worst_x <= 1e-5
    assert (mel[7] == -100.0).all()                                  # the all-zero extract


def test_nnls_against_the_oracle_iterate():
    f = np.load(os.path.join(GOLDEN, "basis_real_tiles.npz"))
    tiles = np.concatenate([f[k][[0, 5, 10, 15, 20, 25]] for k in ("x1", "x2", "mixed")]).astype(np.float32)
    p = audio.mel_to_power(torch.from_numpy(tiles)[..., None].cuda(), iters=200).cpu().numpy()
    assert p.shape == (18, 1025, 64)
    setup = R.nnls_setup()
    outside = (R.mel_filterbank() > 0).sum(axis=0) == 0
    worst = 0.0
    for i in range(len(tiles)):
        ref = R.mel_to_power(tiles[i], 200, setup)
        rel = np.linalg.norm(p[i] - ref, axis=0) / np.linalg.norm(ref, axis=0)
        worst = max(worst, float(rel.max()))
    print("NNLS (FISTA, 200 iterations) vs fp64 oracle: worst per-frame relative L2 %.2e" % worst)
    assert worst <= 1e-3
    assert (p >= 0).all() and (p[:, outside, :] == 0).all() and outside.sum() > 0


def test_istft_reuse_phase_wiener_and_length():
    y = excerpt()[:3]
    mel, X = audio.mel_tiles(torch.from_numpy(y).cuda(), return_stft=True)
    pw = (X.abs() ** 2)[None].contiguous()
    back = audio.masked_istft(pw, X).cpu().numpy()[0]
    assert back.shape == (3, 32256)
    err = np.abs(back - y[:, :32256]).max() / np.abs(y).max()
    rng = np.random.default_rng(3)
    u = torch.from_numpy(rng.uniform(0.0, 1.0, (2,) + tuple(pw.shape[1:])).astype(np.float32)).cuda()
    pw2 = (u * pw).contiguous()
    w = audio.masked_istft(pw2, X, wiener=True).cpu().numpy()
    Xn, pn = X.cpu().numpy().astype(np.complex128), pw2.cpu().numpy().astype(np.float64)
    werr = 0.0
    for i in range(3):
        ref = R.masked_istft([pn[0, i], pn[1, i]], Xn[i], wiener=True)
        for s in range(2):
            werr = max(werr, float(np.abs(w[s, i] - ref[s]).max() / np.abs(ref[s]).max()))
    print("iSTFT: reuse phase of |X|^2 returns the signal to %.2e of max |y|; Wiener vs oracle %.2e" % (err, werr))
    assert err <= 1e-5 and werr <= 1e-5
    # 30 tiles -> 967 680 samples, the length of every wav the reference ships for this separation
    y30 = np.tile(excerpt(), (5, 1))
    mel, X = audio.mel_tiles(torch.from_numpy(y30).cuda(), return_stft=True)
    out = audio.invert([mel, mel], X, wiener=True, iters=20)
    assert tuple(out.shape) == (2, 967680) and torch.isfinite(out).all()


@pytest.fixture(scope="module")
def flows():
    f = np.load(os.path.join(GOLDEN, "basis_real_tiles.npz"))
    out = []
    for i, k in enumerate(("gt1", "gt2")):
        mb = torch.from_numpy(f[k][:8].astype(np.float32))[..., None].cuda()
        out.append(build_glow(mb, [96, 64, 1], L=3, K=2, n_filters=128, learntop=True, seed=40 + i, **MEL))
    return out


def test_separate_audio_end_to_end(flows, tmp_path):
    y = excerpt()[:4].reshape(-1)
    path = tmp_path / "mix.wav"
    audio.write_wav(path, y)
    sig = np.array([20.0, 5.0], np.float32)
    kw = dict(T=4, delta=1e-4, seed=9)
    y1, y2, mixed, x1, x2 = audio.separate_audio(str(path), flows[0], flows[1], sig, **kw)
    assert tuple(y1.shape) == (4 * 32256,) and tuple(y2.shape) == (4 * 32256,) and tuple(mixed.shape) == (4, 96, 64, 1)
    assert all(bool(torch.isfinite(t).all()) for t in (y1, y2, x1, x2))
    # the same thing composed by hand from the stages
    m, X = audio.mel_tiles(audio.extracts(audio.read_wav(path)), return_stft=True)
    a1 = -100.0 + 120.0 * basis.device_randn(tuple(m.shape), m.device, seed=9, which=14, uniform=True)
    a2 = -100.0 + 120.0 * basis.device_randn(tuple(m.shape), m.device, seed=9, which=15, uniform=True)
    a1, a2, _ = basis.basis_outer_loop(m, a1, a2, flows[0], flows[1], sig, T=4, delta=1e-4, seed=9)
    h = audio.invert([a1, a2], X)
    assert torch.equal(m, mixed) and torch.equal(a1, x1) and torch.equal(a2, x2)
    assert torch.equal(h[0], y1) and torch.equal(h[1], y2)
    r1, r2, *_ = audio.separate_audio(str(path), flows[0], flows[1], sig, **kw)
    assert torch.equal(r1, y1) and torch.equal(r2, y2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        q1, q2, *_ = audio.separate_audio(str(path), flows[0], flows[1], sig, **kw)
    s.synchronize()
    assert torch.equal(q1, y1) and torch.equal(q2, y2)
    for k, v in (("sep1", y1), ("sep2", y2)):
        audio.write_wav(tmp_path / (k + ".wav"), v)
        assert audio.read_wav(tmp_path / (k + ".wav")).shape == (4 * 32256,)


def test_host_inputs_are_moved_and_host_pointers_refused():
    """invert on the tiles as a reader of results.npz has them (host arrays) equals invert on device tensors; the C entry points
    refuse a host pointer before any launch."""
    import ctypes
    from audiosourcesep_amd import _lib
    y = excerpt()[:2]
    mel, X = audio.mel_tiles(y, return_stft=True)                             # a host array in
    f = np.load(os.path.join(GOLDEN, "basis_real_tiles.npz"))
    t1, t2 = (f[k][:2].astype(np.float32) for k in ("x1", "x2"))
    ref = audio.invert([torch.from_numpy(t1).cuda(), torch.from_numpy(t2).cuda()], X, wiener=True, iters=20)
    got = audio.invert([t1, torch.from_numpy(t2)], X.cpu(), wiener=True, iters=20)
    assert got.is_cuda and torch.equal(got, ref)
    # one NNLS launch over both sources gives what one launch per source gives
    p = torch.stack([audio.mel_to_power(torch.from_numpy(t).cuda(), 20) for t in (t1, t2)])
    assert torch.equal(audio.masked_istft(p, X, wiener=True).reshape(2, -1), ref)
    lib = _lib.load()
    host = np.zeros((2, 96, 64), np.float32)
    out = torch.empty((2, 1025, 64), device="cuda")
    rc = lib.glowk_mel_to_power(ctypes.c_void_p(host.ctypes.data), 2, 64, 20, ctypes.c_void_p(out.data_ptr()), None)
    assert rc != 0 and b"device memory" in lib.glowk_last_error()
