"""The stereo EM Wiener filter on the GPU (``glowk_mwf_em`` in csrc/glowk_stereo.h through ``audio.multichannel_wiener``) against
the fp64 restatement of tests/stereo_ref.py, its bitwise properties, degenerate inputs, and ``audio.separate_stereo`` /
``separate_wav_stereo`` end to end.

The bar against the restatement, 2e-6 of the largest reference value for Y, v and R alike: the output is rounded once to fp32
(2^-24 = 6e-8); the only other fp32 step is the storage of v between iterations, whose effect on the fp64 restatement was measured
at <= 1.8e-7 max|Y| after 50 iterations with 16 sources; the bar is ten times that.  Both sides see the same fp32 inputs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, audio
from audiosourcesep_amd.config import GlowConfig
from tests import stereo_ref as R

pytestmark = pytest.mark.gpu
BAR = 2e-6


def run(x, v, n_iter):
    """The kernel on fp32 copies of x [P, 2, 1025, T], v [S, P, 1025, T] -> (Y, v, R) as numpy arrays."""
    Y, vf, Rf = audio.multichannel_wiener(torch.from_numpy(v.astype(np.float32)), torch.from_numpy(x.astype(np.complex64)), n_iter,
                                          return_model=True)
    return Y.cpu().numpy(), vf.cpu().numpy(), Rf.cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(S, T, P, n_iter, bins=1025):
    """The generator's problem (a fixed seed per shape) and the restatement's (Y, v, R) for it: computed once, never modified."""
    pr = R.problem(S, T, bins, P=P, seed=1000 * S + 10 * T + P)
    return pr, R.multichannel_wiener(pr["x"], pr["v"], n_iter, return_model=True)


def worst(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


# every S in {1, 2, 3, 16}, T in {7, 64, 65, 300} (one wave, a full wave, a tail in a second wave, two chunks of four waves with a
# tail), P in {1, 3} and n_iter in {0, 1, 2, 10} appears; the rows are staged in LDS at all of these sizes
@pytest.mark.parametrize("S,T,P,n_iter", [(1, 7, 3, 2), (3, 7, 1, 0), (2, 64, 1, 10), (3, 65, 3, 1), (2, 300, 1, 2), (16, 64, 1, 1),
                                          (16, 7, 1, 10)])
def test_against_the_restatement(S, T, P, n_iter):
    pr, (Yr, vr, Rr) = reference(S, T, P, n_iter)
    Y, v, Rm = run(pr["x"], pr["v"], n_iter)
    assert Y.shape == (S, P, 2, 1025, T) and Y.dtype == np.complex64 and v.shape == (S, P, 1025, T) and Rm.shape == (S, P, 1025, 2, 2)
    eY, ev, eR = worst(Y, Yr), worst(v, vr), worst(Rm, Rr)
    print("S = %d, T = %d, P = %d, n_iter = %d: max|d| / max|ref|  Y %.2e  v %.2e  R %.2e" % (S, T, P, n_iter, eY, ev, eR))
    assert eY <= BAR and ev <= BAR and eR <= BAR
    if n_iter == 0:
        assert np.array_equal(v, pr["v"].astype(np.float32)) and np.array_equal(Rm, R.start(pr["v"]))


def test_rows_too_long_for_lds_are_streamed_in_place():
    """S = 16, T = 800: 64 KB of rows per (problem, bin), past the staging limit, so the kernel updates v in global memory; four
    256-frame chunks with a tail.  41 distinct bins laid out 25 times fill the 1025: every copy must give the same bits."""
    pr, (Yr, vr, Rr) = reference(16, 800, 1, 2, bins=41)
    Y, v, Rm = run(np.tile(pr["x"], (1, 1, 25, 1)), np.tile(pr["v"], (1, 1, 25, 1)), 2)
    for k in range(1, 25):
        sl = slice(41 * k, 41 * k + 41)
        assert np.array_equal(Y[:, :, :, sl], Y[:, :, :, :41]) and np.array_equal(v[:, :, sl], v[:, :, :41])
        assert np.array_equal(Rm[:, :, sl], Rm[:, :, :41])
    eY, ev, eR = worst(Y[:, :, :, :41], Yr), worst(v[:, :, :41], vr), worst(Rm[:, :, :41], Rr)
    print("S = 16, T = 800 (streamed), n_iter = 2: max|d| / max|ref|  Y %.2e  v %.2e  R %.2e" % (eY, ev, eR))
    assert eY <= BAR and ev <= BAR and eR <= BAR


def test_bitwise_properties():
    pr, _ = reference(3, 65, 3, 1)
    x, v0 = pr["x"], pr["v"]
    a, b = run(x, v0, 2), run(x, v0, 2)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))                       # two calls
    one = run(x[1:2], v0[:, 1:2], 2)                                             # a problem alone is its slice of the batch
    assert np.array_equal(one[0], a[0][:, 1:2]) and np.array_equal(one[1], a[1][:, 1:2]) and np.array_equal(one[2], a[2][:, 1:2])
    x2, v2 = 3.0 * x, 0.5 * v0                                                   # every other bin's inputs change
    x2[:, :, 100], v2[:, :, 100] = x[:, :, 100], v0[:, :, 100]
    c = run(x2, v2, 2)
    assert np.array_equal(c[0][:, :, :, 100], a[0][:, :, :, 100]) and np.array_equal(c[1][:, :, 100], a[1][:, :, 100])
    assert np.array_equal(c[2][:, :, 100], a[2][:, :, 100]) and not np.array_equal(c[0][:, :, :, 101], a[0][:, :, :, 101])
    # the filters sum to I - eps Cx^-1: fp64 gives 5e-11; the slack is the fp32 rounding of the S outputs
    assert float(np.abs(v0.sum(0)).min()) >= 1e-6
    err = float(np.abs(a[0].astype(np.complex128).sum(0) - x).max() / np.abs(x).max())
    print("sum_j Y_j - x: %.2e of max|x|" % err)
    assert err <= 1e-5


def test_only_the_psds_are_written_and_the_wrapper_keeps_the_callers():
    pr, _ = reference(3, 65, 3, 1)
    X = torch.view_as_real(torch.from_numpy(pr["x"].astype(np.complex64)).cuda()).contiguous()
    v = torch.from_numpy(pr["v"].astype(np.float32)).cuda()
    X0, v0 = X.clone(), v.clone()
    Y = torch.empty((3, 3, 2, 1025, 65, 2), device="cuda")
    r = torch.empty((3, 3, 1025, 4), device="cuda", dtype=torch.float64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lib = _lib.load()
    _lib.check(lib.glowk_mwf_em(p(X), p(v), 3, 3, 65, 2, p(Y), p(r), None))
    torch.cuda.synchronize()
    assert torch.equal(X, X0) and not torch.equal(v, v0)
    Yw, vw, Rw = audio.multichannel_wiener(v0, torch.view_as_complex(X0), 2, return_model=True)
    assert torch.equal(v0, torch.from_numpy(pr["v"].astype(np.float32)).cuda())  # float32, contiguous, on the device: still the caller's
    assert torch.equal(torch.view_as_real(Yw), Y) and torch.equal(vw, v) and torch.equal(Rw[..., 0, 1], torch.complex(r[..., 2], r[..., 3]))
    assert torch.equal(audio.multichannel_wiener(v0, torch.view_as_complex(X0), 2), Yw)          # without the model output
    _lib.check(lib.glowk_mwf_em(p(X), p(v0), 3, 3, 65, 0, p(Y), None, None))     # no iteration: nothing but y is written
    torch.cuda.synchronize()
    assert torch.equal(v0, torch.from_numpy(pr["v"].astype(np.float32)).cuda()) and torch.equal(X, X0)
    host = np.zeros((1, 2, 1025, 8, 2), np.float32)
    rc = lib.glowk_mwf_em(ctypes.c_void_p(host.ctypes.data), p(v), 1, 1, 8, 1, p(Y), None, None)
    assert rc == _lib.ERR and "device memory" in lib.glowk_last_error().decode()
    assert lib.glowk_mwf_em(None, None, 2, 0, 8, 1, None, None, None) == 0


def test_likelihood_never_falls_and_quality_follows_the_restatement():
    """S = 2, T = 64: L of the kernel's (v, R) at n_iter = 0..5, and the SDR gain of 10 iterations against the restatement's."""
    pr, (Yr10, _, _) = reference(2, 64, 1, 10)
    x, v0, src = pr["x"], pr["v"], pr["sources"]
    L = []
    for n in range(6):
        _, v, Rm = run(x, v0, n)
        L.append(R.log_likelihood(x, v.astype(np.float64), Rm))
    print("log-likelihood at n_iter = 0..5:", ["%.6e" % l for l in L])
    assert all(b >= a - 1e-6 * abs(a) for a, b in zip(L, L[1:])), L
    Yr0 = R.multichannel_wiener(x, v0, 0)
    gain_ref = R.sdr(src, Yr10) - R.sdr(src, Yr0)
    gain = R.sdr(src, run(x, v0, 10)[0]) - R.sdr(src, run(x, v0, 0)[0])
    print("SDR gain of 10 iterations: kernel %+.4f dB, restatement %+.4f dB" % (gain, gain_ref))
    assert gain_ref >= 1.0 and abs(gain - gain_ref) <= 0.05


def test_degenerate_inputs_stay_finite():
    """Covariances singular up to the ridge: finiteness at every iteration count, correctness at n_iter = 0 only (two correct fp64
    evaluation orders can differ above the bar beyond it)."""
    pr = R.problem(2, 64, 1025, P=2, seed=77)
    x, v = pr["sources"].copy(), pr["v"].copy()
    x[0, :, 1] = 0.0                                      # source 0 hard-panned left: exactly rank 1
    x[1, 1, 1] = 0.0                                      # problem 1: both sources on the left, the right channel silent
    x = x.sum(0).astype(np.complex64).astype(np.complex128)
    x[:, :, 5] = 0.0                                      # an all-zero bin
    v[:, :, 9] = 0.0                                      # a bin with every v = 0
    v[0, :, 11, ::2] = 0.0                                # and zeros scattered in one source
    cases = [(x, v), (x[:, :, :, :1].copy(), v[:, :, :, :1].copy())]             # T = 64 and T = 1
    for xc, vc in cases:
        for n_iter in (0, 1, 3, 10):
            Y, vf, Rm = run(xc, vc, n_iter)
            assert np.isfinite(Y).all() and np.isfinite(vf).all() and np.isfinite(Rm).all(), (xc.shape, n_iter)
            assert (vf >= 0).all()
            if n_iter == 0:
                assert worst(Y, R.single_channel_mask(xc, vc)) <= BAR
                assert not Y[:, :, :, 5].any() and not Y[:, :, :, 9].any()


# ---- audio ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def audio_flows():
    """Tiny K = 1 priors, as tests/test_gpu_basis_sources.py builds them."""
    from audiosourcesep_amd.flow_models.flow_glow import GlowFlow
    from audiosourcesep_amd.synthetic import calibrated_engine
    cfg = GlowConfig(H=96, W=64, C=1, L=2, K=1, F=128)
    return [GlowFlow(calibrated_engine(cfg, device=0, init_tiles=8, seed=50 + k)[0]) for k in range(2)]


def synthetic_stereo():
    """Two extracts of two differently panned tones plus noise: [2, 65280]."""
    rng = np.random.default_rng(8)
    t = np.arange(2 * audio.EXTRACT) / 16000.0
    a, b = 0.3 * np.sin(2 * np.pi * 440.0 * t), 0.2 * np.sin(2 * np.pi * (200.0 * t + 900.0 * t * t))
    y = np.stack([0.9 * a + 0.2 * b, 0.3 * a + 0.8 * b]) + 0.01 * rng.standard_normal((2, t.size))
    return y.astype(np.float32)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def test_separate_stereo_end_to_end(audio_flows):
    y = synthetic_stereo()
    sig = np.array([20.0, 5.0], np.float32)
    kw = dict(T=2, delta=1e-4, seed=9)
    ys, mixed, xs = audio.separate_stereo(y, audio_flows, sig, **kw)
    assert tuple(ys.shape) == (2, 2, 2 * 32256) and tuple(mixed.shape) == (2, 96, 64, 1) and tuple(xs.shape) == (2, 2, 96, 64, 1)
    assert bool(torch.isfinite(ys).all()) and float(ys.abs().max()) > 0
    ys2, _, xs2 = audio.separate_stereo(torch.from_numpy(y), audio_flows, sig, **kw)
    assert torch.equal(ys, ys2) and torch.equal(xs, xs2)
    ys3, _, xs3 = audio.separate_stereo(y, audio_flows, sig, T=2, delta=1e-4, seed=10)
    assert not torch.equal(xs, xs3) and not torch.equal(ys, ys3)
    yw, mw, xw = audio.separate_stereo(y, audio_flows, sig, method="whole", **kw)
    assert tuple(yw.shape) == (2, 2, (2 * 64 - 1) * 512) and bool(torch.isfinite(yw).all()) and torch.equal(xw, xs) and torch.equal(mw, mixed)
    # the priors see the downmix: the tiles are separate_sources' own
    down = (y[0] + y[1]) / 2
    _, md, xd = audio.separate_sources(down, audio_flows, sig, **kw)
    assert torch.equal(md, mixed) and torch.equal(xd, xs)
    # without EM the filter is the single-channel Wiener mask on each channel.  The bar between the masked_istft and the
    # griffinlim(n_iter=0) inversion paths is the relative L2 of 1e-6 that
    # tests/test_gpu_griffinlim.py::test_whole_equals_frame_for_one_tile_and_the_oracle_for_many sets between them
    y0, _, x0 = audio.separate_stereo(y, audio_flows, sig, em_iter=0, **kw)
    assert torch.equal(x0, xs)
    for c in range(2):
        _, Xc = audio.mel_tiles(audio.extracts(torch.from_numpy(y[c])), return_stft=True)
        want = audio.invert(list(xs), Xc, wiener=True)
        err = rel(y0[:, c], want)
        print("em_iter = 0, channel %d against invert(wiener=True): relative L2 %.2e" % (c, err))
        assert err <= 1e-6
    assert not torch.equal(y0, ys)
    with pytest.raises(ValueError):
        audio.separate_stereo(y[0], audio_flows, sig, **kw)


def test_separate_wav_stereo_resamples_all_outputs(audio_flows, tmp_path):
    y = synthetic_stereo()
    y8 = audio.resample(y, 16000, 8000).cpu().numpy()
    path, mono = tmp_path / "mix8k.wav", tmp_path / "mono8k.wav"
    audio.save_audio(path, y8, 8000)
    audio.save_audio(mono, y8[0], 8000)
    sig = np.array([20.0, 5.0], np.float32)
    ys, mixed, xs, rate = audio.separate_wav_stereo(str(path), audio_flows, sig, T=1, delta=1e-4, seed=9)
    n16 = xs.shape[1] * 32256
    assert rate == 8000 and tuple(ys.shape) == (2, 2, n16 // 2) and bool(torch.isfinite(ys).all())
    ys16, *_, rate16 = audio.separate_wav_stereo(str(path), audio_flows, sig, out_rate=None, T=1, delta=1e-4, seed=9)
    assert rate16 == 16000 and tuple(ys16.shape) == (2, 2, n16)
    with pytest.raises(ValueError, match="separate_wav_sources"):
        audio.separate_wav_stereo(str(mono), audio_flows, sig, T=1, delta=1e-4, seed=9)


def test_istft_inverts_the_front_ends_stft():
    y = torch.from_numpy(synthetic_stereo()[:, :audio.EXTRACT])
    _, X = audio.mel_tiles(y, return_stft=True)
    back = audio.istft(X)
    assert tuple(back.shape) == (2, 63 * 512)
    assert rel(back[:, 1024:-1024].cpu(), y[:, 1024:63 * 512 - 1024]) <= 1e-5
    assert tuple(audio.istft(X.reshape(2, 1, 1025, 64)).shape) == (2, 1, 63 * 512)
