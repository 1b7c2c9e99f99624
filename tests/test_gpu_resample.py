"""The sample-rate converter on the GPU (csrc/glowk_resample.h through audiosourcesep_amd/audio.py) against the fp64 restatement
of tests/resample_ref.py, on real material (tests/golden/real_audio_excerpt.npz: 195 840 samples, peak 0.068).

The bound, BOUND = 6e-6 of the input's peak, and where it comes from: ``resample_ref.emulate_fp32`` restates the kernel's
arithmetic on the CPU in its summation order (float32 table pairs, integer table positions, one fp32 FMA chain outwards on each
side of the centre).  Against the fp64 restatement, on the excerpt (n_in 1000, 32 640 from two offsets, and all 195 840 samples)
its worst error as a fraction of the peak was, per rate pair: 44100->16000 6.0e-7, 48000->16000 5.6e-7, 22050->16000 4.8e-7,
11025->16000 4.8e-7, 8000->16000 5.4e-7, 96000->16000 7.3e-7 (the longest chains: up to 769 taps), 16000->44100 5.8e-7,
16000->48000 6.1e-7, 44101->16000 5.1e-7.  Worst 7.3e-7; allowed 8 x that, rounded: 6e-6 (below the 1e-5 of the iSTFT tests,
whose sums are longer).  Nothing in it comes from the kernel's output.

Bitwise claims rest on the order of one output's sum being fixed relative to its centre q, with taps outside the signal
multiplying a staged zero: it cannot depend on the batch, the workgroup, the signal's length or the position in the signal."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, audio
from audiosourcesep_amd.flow_models.flow_builder import build_glow
from tests import resample_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEL = dict(data_type="melspec", minval=-100.0, maxval=20.0, use_logit=False)
BOUND = 6e-6
PAIRS = [(44100, 16000), (48000, 16000), (22050, 16000), (11025, 16000), (8000, 16000), (96000, 16000), (16000, 44100),
         (16000, 48000), (44101, 16000)]
LENGTHS = [1, 2, 127, 128, 129, 1000, 32640, 195840]


def track():
    """The six real extracts end to end: 195 840 samples in [-1, 1)."""
    return np.load(os.path.join(GOLDEN, "real_audio_excerpt.npz"))["pcm"].astype(np.float32).reshape(-1) / 32768.0


def signals(nsig, n):
    """nsig slices of the track, from different places (the first from its loudest region for the short lengths)."""
    y = track()
    starts = [min(30000, len(y) - n), min(101000, len(y) - n), min(60000, len(y) - n)]
    return np.stack([y[s:s + n] for s in starts[:nsig]]).copy()


@pytest.fixture(scope="module")
def table():
    return R.table()


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_against_the_restatement(sr_in, sr_out, table):
    worst = 0.0
    for n in LENGTHS:
        for nsig in (1, 3):
            x = signals(nsig, n)
            y = audio.resample(torch.from_numpy(x).cuda(), sr_in, sr_out)
            assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == (nsig, R.length(n, sr_in, sr_out))
            assert y.shape[1] == -((-n * sr_out) // sr_in)
            y = y.cpu().numpy()
            for i in range(nsig if n <= 32640 else 1):             # the long case: one signal against the restatement
                ref = R.resample(x[i], sr_in, sr_out, T=table)
                err = float(np.abs(y[i] - ref).max() / max(np.abs(x[i]).max(), 1e-30))     # a silent slice: y = 0 exactly
                worst = max(worst, err)
                assert err <= BOUND, (n, nsig, i, err)
    print("%d -> %d Hz vs fp64 restatement: worst max |d| %.2e of the peak (bound %.0e)" % (sr_in, sr_out, worst, BOUND))


@pytest.mark.parametrize("sr_in,sr_out", [(44100, 16000), (16000, 44100), (96000, 16000), (44101, 16000)])
def test_bitwise_invariances(sr_in, sr_out):
    a, b = R.ratio(sr_in, sr_out)
    x = torch.from_numpy(signals(3, 32640)).cuda()
    y = audio.resample(x, sr_in, sr_out)
    assert torch.equal(audio.resample(x, sr_in, sr_out), y)                       # a second run
    for i in range(3):                                                            # a signal of a batch, alone
        assert torch.equal(audio.resample(x[i].clone(), sr_in, sr_out), y[i])
    if a <= 1000:                                                                 # x delayed by a samples: y delayed by b, every output
        xd = torch.cat([torch.zeros(3, a, device="cuda"), x], dim=1)
        yd = audio.resample(xd, sr_in, sr_out)
        assert yd.shape[1] == y.shape[1] + b and torch.equal(yd[:, b:], y)
    # a truncated copy: equal wherever every tap lies inside the kept part.  Output t reads x[q - H + 1 .. q + H], q = t a // b
    keep = 20000
    yt = audio.resample(x[:, :keep].contiguous(), sr_in, sr_out)
    H = (R.Z * max(a, b)) // b + 1
    t = np.arange(yt.shape[1], dtype=np.int64)
    inside = torch.from_numpy((t * a) // b + H < keep).cuda()
    assert int(inside.sum()) > 0.8 * keep * b / a - 2 * H * b / a - 2
    assert torch.equal(yt[:, inside], y[:, :yt.shape[1]][:, inside])
    s = torch.cuda.Stream()                                                       # on another stream
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ys = audio.resample(x, sr_in, sr_out)
    s.synchronize()
    assert torch.equal(ys, y)


def test_positions_beyond_32_bits(table):
    """20 minutes of 44.1 kHz audio: t a exceeds 2^32 in the last tenth of the output."""
    y0 = track()
    n = 20 * 60 * 44100
    x = np.tile(y0, n // len(y0) + 1)[:n]
    y = audio.resample(torch.from_numpy(x).cuda(), 44100, 16000)
    n_out = R.length(n, 44100, 16000)
    assert tuple(y.shape) == (n_out,) and n_out == 19200000
    idx = np.sort(np.random.default_rng(11).choice(np.arange(n_out - n_out // 10, n_out), 4096, replace=False))
    assert idx[0] * 441 > 1 << 32
    ref = R.resample(x, 44100, 16000, idx=idx, T=table)
    got = y[torch.from_numpy(idx).cuda()].cpu().numpy()
    err = float(np.abs(got - ref).max() / np.abs(x).max())
    print("20 min 44.1 kHz -> 16 kHz, 4096 outputs of the last tenth vs fp64 restatement: %.2e of the peak" % err)
    assert err <= BOUND
    assert bool(torch.isfinite(y).all())


def test_edges_and_refusals():
    lib = _lib.load()
    z = ctypes.c_void_p(0)
    x = torch.from_numpy(signals(1, 1000)).cuda()
    assert tuple(audio.resample(torch.zeros(0, device="cuda"), 44100, 16000).shape) == (0,)        # n_in = 0
    assert tuple(audio.resample(torch.zeros((0, 100), device="cuda"), 44100, 16000).shape) == (0, 37)   # nsig = 0
    assert tuple(audio.resample(torch.zeros((2, 3, 100), device="cuda"), 16000, 44100).shape) == (2, 3, 276)
    assert lib.glowk_resample(z, 0, 1000, 44100, 16000, z, z) == 0 and lib.glowk_resample(z, 2, 0, 44100, 16000, z, z) == 0
    same = audio.resample(x, 16000, 16000)                                        # equal rates: the input, no launch
    assert same.data_ptr() == x.data_ptr()
    host = audio.resample(x.cpu().numpy()[0], 44100, 16000)                        # a host array in, a CUDA tensor out
    assert host.is_cuda and torch.equal(host, audio.resample(x, 44100, 16000)[0])
    out = torch.full((1, 363), 7.0, device="cuda")
    px, po = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr())
    for sr_in, sr_out, word in [(999, 16000, "[1000, 768000]"), (16000, 768001, "[1000, 768000]"), (1000, 64001, "1/64"), (64001, 1000, "1/64")]:
        assert lib.glowk_resample(px, 1, 1000, sr_in, sr_out, po, z) == _lib.ERR and word in lib.glowk_last_error().decode()
    harr = np.zeros(1000, np.float32)
    assert lib.glowk_resample(ctypes.c_void_p(harr.ctypes.data), 1, 1000, 44100, 16000, po, z) == _lib.ERR
    assert "device memory" in lib.glowk_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                # nothing was launched


@pytest.fixture(scope="module")
def flows():
    f = np.load(os.path.join(GOLDEN, "basis_real_tiles.npz"))
    out = []
    for i, k in enumerate(("gt1", "gt2")):
        mb = torch.from_numpy(f[k][:8].astype(np.float32))[..., None].cuda()
        out.append(build_glow(mb, [96, 64, 1], L=3, K=2, n_filters=128, learntop=True, seed=40 + i, **MEL))
    return out


def test_files_end_to_end(flows, tmp_path, table):
    """A 44.1 kHz 16-bit stereo wav (the excerpt's first four extracts upsampled by the restatement, L = R) through load_audio and
    separate_wav."""
    y16 = track()[:4 * 32640]
    up = R.resample(y16, 16000, 44100, T=table)
    path = tmp_path / "mix441.wav"
    audio.save_audio(path, np.stack([up, up]), 44100)
    with wave.open(str(path), "rb") as w:
        assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (44100, 2, 2, len(up))
    quant = np.rint(np.clip(up, -1.0, 1.0) * 32767.0) / 32768.0                   # what the file holds (L = R: the mean is exact)
    y, rate = audio.load_audio(path)
    assert rate == 44100 and y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (R.length(len(up), 44100, 16000),)
    ref = R.resample(quant.astype(np.float32), 44100, 16000, T=table)
    err = float(np.abs(y.cpu().numpy() - ref).max() / np.abs(quant).max())
    print("load_audio of the 44.1 kHz stereo file vs the restatement: %.2e of the peak" % err)
    assert err <= BOUND
    native, rate = audio.load_audio(path, sr=None, mono=False)
    assert rate == 44100 and not native.is_cuda and tuple(native.shape) == (2, len(up))
    mel = audio.mel_tiles(audio.extracts(y))
    assert tuple(mel.shape) == (len(y) // 32640, 96, 64, 1) and bool(torch.isfinite(mel).all())

    sig = np.array([20.0, 5.0], np.float32)
    kw = dict(T=4, delta=1e-4, seed=9)
    y1, y2, mixed, x1, x2, out_rate = audio.separate_wav(str(path), flows[0], flows[1], sig, **kw)
    a1, a2, m, b1, b2 = audio.separate_audio(y, flows[0], flows[1], sig, **kw)
    assert out_rate == 44100 and torch.equal(m, mixed) and torch.equal(b1, x1) and torch.equal(b2, x2)
    n441 = _lib.load().glowk_resample_length(a1.shape[0], 16000, 44100)
    assert tuple(y1.shape) == (n441,) and tuple(y2.shape) == (n441,)
    assert bool(torch.isfinite(y1).all()) and bool(torch.isfinite(y2).all())
    assert torch.equal(y1, audio.resample(a1, 16000, 44100)) and torch.equal(y2, audio.resample(a2, 16000, 44100))
    k1, k2, *_, r16 = audio.separate_wav(str(path), flows[0], flows[1], sig, out_rate=None, **kw)
    assert r16 == 16000 and torch.equal(k1, a1) and torch.equal(k2, a2)
    e1, _, *_, r8 = audio.separate_wav(str(path), flows[0], flows[1], sig, out_rate=8000, **kw)
    assert r8 == 8000 and torch.equal(e1, audio.resample(a1, 16000, 8000))
    audio.save_audio(tmp_path / "sep1.wav", y1, out_rate)
    back, rate = audio.load_audio(tmp_path / "sep1.wav", sr=None)
    assert rate == 44100 and tuple(back.shape) == (n441,)
