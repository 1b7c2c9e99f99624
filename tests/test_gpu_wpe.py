"""WPE dereverberation on the GPU (csrc/glowk_wpe.h through audiosourcesep_amd/wpe.py) against the fp64 restatement tests/wpe_ref.py.

Every stage is held to the bound include/glowk.h states for it, with the stage's inputs taken from the restatement so that the stages
are judged one by one: the weights relatively, the correlations elementwise against sums in extended precision, the solve by its
residual (condition-free), the filter within one complex64 rounding.  The loop is held to twice its stated bound on the AR scenes,
and to the same 20 dB of dereverberation as the restatement.  Every figure is printed before it is asserted, the largest fractions
as ``wpe-accuracy <name> <value>`` lines (profiles/wpe_accuracy.json is made from them)."""
import functools
import wave

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, audio, iva, wpe
from tests import wpe_ref as W
from tests.footprint import guarded_allocations

pytestmark = pytest.mark.gpu

# ([N, M, R, T], K, delay, context)
CASES = [
    ((1, 1, 1, 7), 3, 1, 0),        # D = 3, less than a tile; T not a multiple of 4
    ((1, 2, 5, 203), 3, 2, 0),
    ((3, 2, 5, 203), 10, 3, 1),     # a batch, D = 20: two row tiles
    ((1, 3, 2, 301), 7, 3, 0),      # D = 21
    ((2, 4, 3, 301), 16, 2, 2),     # D = 64, the maximum: 14 tile pairs, four to a wave
    ((1, 2, 2, 4), 3, 2, 0),        # T < delay + K
    ((1, 4, 1, 40), 16, 1, 0),      # T < D
    ((1, 2, 3, 1029), 32, 16, 8),   # the top of K, delay and the context; five frame chunks with a halo of 47
]
IDS = ["x".join(map(str, c[0])) + "-K%d-d%d-c%d" % c[1:] for c in CASES]
MIN_GAIN_DB = 20.0


def gpu(a):
    return torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same(a, b):
    """Bit for bit, tensors of one dtype."""
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all())


def record(name, value):
    print("wpe-accuracy %s %.6g" % (name, value))


@functools.lru_cache(maxsize=None)
def mixture(shape, seed=3):
    """A reverberant-looking complex64 STFT [N, M, R, T]: Gaussian cells under a slow envelope, smeared over the following frames."""
    rng = np.random.default_rng(seed)
    N, M, R, T = shape
    t = np.arange(T)
    env = np.exp(1.2 * np.sin(2 * np.pi * (t / 29.0 + rng.uniform(size=(N, M, R, 1)))))
    s = env * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    x = s.copy()
    for lag, g in ((1, 0.5), (2, 0.35 + 0.2j), (4, -0.25j), (7, 0.15)):
        if lag < T:
            x[..., lag:] += g * s[..., :T - lag]
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


def each_row(X):
    """(index into [.., R], x [M, T]) for every row of X [N, M, R, T]."""
    N, M, R, T = X.shape
    for n in range(N):
        for r in range(R):
            yield (n, r), X[n, :, r]


@functools.lru_cache(maxsize=None)
def reference(i):
    """The restatement's stages for case i, each from the stage before: w, max, R, P and their bounds, the loaded R, L, G, y."""
    shape, K, delay, c = CASES[i]
    X = mixture(shape)
    N, M, R, T = shape
    D = M * K
    out = dict(w=np.zeros((N, R, T)), pm=np.zeros((N, R)), R=np.zeros((N, R, D, D), np.complex128), P=np.zeros((N, R, D, M), np.complex128),
               bR=np.zeros((N, R, D, D), np.complex128), bP=np.zeros((N, R, D, M), np.complex128), G=np.zeros((N, R, D, M), np.complex128),
               status=np.zeros((N, R), np.int32), loaded={}, L={}, y=np.zeros(shape, np.complex128), mag=np.zeros(shape))
    for (n, r), x in each_row(X):
        out["w"][n, r], out["pm"][n, r], _ = W.inv_power(x, c)
        out["R"][n, r], out["P"][n, r], out["bR"][n, r], out["bP"][n, r] = W.correlations(x, out["w"][n, r], K, delay)
        out["G"][n, r], out["status"][n, r], info = W.solve(out["R"][n, r], out["P"][n, r])
        out["loaded"][n, r], out["L"][n, r] = info["loaded"], info["L"]
        out["y"][n, :, r], out["mag"][n, :, r] = W.filter(x, out["G"][n, r], K, delay)
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_power_inverse_is_within_its_bound(i):
    shape, K, delay, c = CASES[i]
    ref = reference(i)
    w, mx = wpe.power_inverse(gpu(mixture(shape)), c, return_max=True)
    assert w.dtype == torch.float64 and tuple(w.shape) == (shape[0],) + shape[2:] and tuple(mx.shape) == (shape[0], shape[2])
    frac = float(np.max(np.abs(host(w) - ref["w"]) / ref["w"])) / W.inv_power_bound(shape[1], c)
    record("power_inverse/" + IDS[i], frac)
    assert frac <= 1.0
    assert np.max(np.abs(host(mx) - ref["pm"]) / ref["pm"]) <= W.inv_power_bound(shape[1], c)
    assert same(wpe.power_inverse(gpu(mixture(shape)), c), w)


@pytest.mark.parametrize("c", [0, 1, 8])
def test_the_row_maximum_is_the_restatements_bit_for_bit_on_exact_values(c):
    """Cells that are small multiples of 1/8: every square, sum and mean count below is exact or rounds the same way in any order but
    the divisions, which the restatement does as the kernel does; the maximum is then the same double."""
    rng = np.random.default_rng(11)
    shape = (2, 3, 4, 301)
    Y = ((rng.integers(-40, 41, size=shape) + 1j * rng.integers(-40, 41, size=shape)) / 8.0).astype(np.complex64)
    Y[1, :, 2] = 0                                                                   # a silent row: maximum 0, weights 0
    w, mx = wpe.power_inverse(gpu(Y), c, return_max=True)
    for (n, r), y in each_row(Y):
        wr, pm, ok = W.inv_power(y, c)
        assert host(mx)[n, r].tobytes() == np.float64(pm).tobytes(), (n, r)
        assert ok == (not (n == 1 and r == 2))
        if ok:
            assert np.max(np.abs(host(w)[n, r] - wr) / wr) <= W.inv_power_bound(3, c)
        else:
            assert not host(w)[n, r].any()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_correlations_are_within_the_elementwise_bound_and_hermitian(i):
    shape, K, delay, c = CASES[i]
    ref = reference(i)
    Rm, P = wpe.correlations(gpu(mixture(shape)), gpu(ref["w"]), K, delay)
    D = shape[1] * K
    assert Rm.dtype == P.dtype == torch.complex128 and tuple(Rm.shape) == (shape[0], shape[2], D, D) and tuple(P.shape) == (shape[0], shape[2], D, shape[1])
    r, p = host(Rm), host(P)
    fracs = []
    for got, want, bound in ((r, ref["R"], ref["bR"]), (p, ref["P"], ref["bP"])):
        for part in ("real", "imag"):
            err, b = np.abs(getattr(got, part) - getattr(want, part)), getattr(bound, part)
            assert (err[b == 0] == 0).all()                                          # an exact zero where every term is zero
            fracs.append(float(np.max(err[b > 0] / b[b > 0])) if (b > 0).any() else 0.0)
    record("correlations/" + IDS[i], max(fracs))
    assert max(fracs) <= 1.0
    iu = np.triu_indices(D, 1)
    up, low = r[..., iu[0], iu[1]], r[..., iu[1], iu[0]]
    assert up.real.tobytes() == low.real.tobytes() and up.imag.tobytes() == (-low.imag).tobytes()   # bitwise Hermitian
    assert not np.diagonal(r, axis1=-2, axis2=-1).imag.any()                         # and the diagonal exactly real
    assert (np.diagonal(r, axis1=-2, axis2=-1).real >= 0).all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_solves_residual_is_within_the_backward_bound(i):
    shape, K, delay, c = CASES[i]
    ref = reference(i)
    G, status = wpe.solve(gpu(ref["R"]), gpu(ref["P"]))
    assert G.dtype == torch.complex128 and status.dtype == torch.int32 and tuple(status.shape) == (shape[0], shape[2])
    assert np.array_equal(host(status), ref["status"]) and not ref["status"].any()
    g, worst = host(G), 0.0
    for key, L in ref["L"].items():
        res, bound = np.abs(ref["loaded"][key] @ g[key] - ref["P"][key]), W.solve_residual_bound(L, g[key])
        assert (res[bound == 0] == 0).all()                                          # all-zero history: exact zeros
        worst = max(worst, float(np.max(res[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0)
    record("solve/" + IDS[i], worst)
    assert worst <= 1.0


def test_the_solve_flags_the_degenerate_rows_as_the_restatement_does():
    shape, K, delay = (3, 2, 4, 60), 3, 2
    X = np.array(mixture(shape))
    D = shape[1] * K
    Rm, P = np.zeros((3, 4, D, D), np.complex128), np.zeros((3, 4, D, 2), np.complex128)
    for (n, r), x in each_row(X):
        Rm[n, r], P[n, r], _, _ = W.correlations(x, W.inv_power(x)[0], K, delay)
    Rm[1, 2], P[1, 2] = 0, 0                                                         # a silent row inside the batch
    Rm[0, 1] = -Rm[0, 1]                                                             # a negative definite one
    Rm[2, 3, 4, 4] = float("nan")                                                    # a pivot that is not finite
    Rm[2, 0, 5, 5] = -1.0                                                            # the last pivot
    want = np.array([[W.solve(Rm[n, r], P[n, r])[1] for r in range(4)] for n in range(3)], np.int32)
    G, status = wpe.solve(gpu(Rm), gpu(P))
    assert np.array_equal(host(status), want) and want.sum() == 4
    g = host(G)
    assert not g[want == 1].any() and np.isfinite(g).all() and all(g[n, r].any() for n in range(3) for r in range(4) if not want[n, r])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_the_filter_is_within_one_complex64_rounding(i):
    shape, K, delay, c = CASES[i]
    ref = reference(i)
    y = wpe.filter(gpu(mixture(shape)), gpu(ref["G"]), K, delay)
    assert y.dtype == torch.complex64 and tuple(y.shape) == shape
    got = host(y).astype(np.complex128)
    bound = W.filter_bound(ref["mag"], shape[1] * K)
    frac = max(float(np.max(np.abs(got.real - ref["y"].real) / bound)), float(np.max(np.abs(got.imag - ref["y"].imag) / bound)))
    record("filter/" + IDS[i], frac)
    assert frac <= 1.0
    zero = wpe.filter(gpu(mixture(shape)), torch.zeros_like(gpu(ref["G"])), K, delay)  # G = 0: a copy
    assert same(zero, gpu(mixture(shape)))


@functools.lru_cache(maxsize=None)
def ar(j):
    X, S = W.ar_scene(*W.AR_SCENES[j])
    X.setflags(write=False)
    return X, S


@pytest.mark.parametrize("j", range(len(W.AR_SCENES)), ids=["M%d-K%d-d%d-T%d" % s for s in W.AR_SCENES])
def test_wpe_end_to_end_on_the_ar_scenes(j):
    M, K, delay, T = W.AR_SCENES[j]
    X, S = ar(j)
    Yr, Gr, sr, infos = W.wpe_rows(X, K, delay, 3)
    Y, G, status = wpe.wpe(gpu(X), K, delay, 3, return_filters=True, return_status=True)
    assert Y.dtype == torch.complex64 and tuple(Y.shape) == X.shape and np.array_equal(host(status), sr) and not sr.any()
    y, worst = host(Y).astype(np.complex128), 0.0
    for (r,), info in infos.items():
        bound = 2.0 * W.wpe_bound(info, Gr[r], X[:, r], K, delay)
        d = y[:, r] - Yr[:, r].astype(np.complex128)
        worst = max(worst, float(np.max(np.abs(d.real) / bound)), float(np.max(np.abs(d.imag) / bound)))
    record("wpe/M%d-K%d-d%d-T%d" % W.AR_SCENES[j], worst)
    before, after, after_ref = W.drr_db(S, X), W.drr_db(S, host(Y)), W.drr_db(S, Yr)
    print("M %d K %d delay %d T %d: %.2f dB -> %.2f dB on the device, %.2f dB in the restatement" % (M, K, delay, T, before, after, after_ref))
    assert worst <= 1.0
    assert abs(after - after_ref) <= 0.01 and after > before
    if W.AR_SCENES[j] in W.AR_GAIN_SCENES:                                           # the mono scene has no bar: see tests/wpe_ref.py
        assert after - before >= MIN_GAIN_DB


def staged(X, K, delay, iterations, c=0):
    y = X
    for _ in range(iterations):
        w = wpe.power_inverse(y, c)
        Rm, P = wpe.correlations(X, w, K, delay)
        G, status = wpe.solve(Rm, P)
        y = wpe.filter(X, G, K, delay)
    return y, G, status


@pytest.mark.parametrize("i", [1, 2, 4, 5, 7], ids=[IDS[i] for i in (1, 2, 4, 5, 7)])
def test_the_loop_is_the_staged_calls_and_repeats_its_bits(i):
    shape, K, delay, c = CASES[i]
    X = gpu(mixture(shape))
    for iterations in (1, 3):
        Y, G, status = wpe.wpe(X, K, delay, iterations, psd_context=c, return_filters=True, return_status=True)
        ys, gs, ss = staged(X, K, delay, iterations, c)
        assert same(Y, ys) and same(G, gs) and same(status, ss), iterations        # return_filters: the G of the last iteration
        again = wpe.wpe(X, K, delay, iterations, psd_context=c)
        assert same(again, Y)
    assert same(wpe.wpe(X, K, delay, 0), X)
    G0, s0 = wpe.wpe(X, K, delay, 0, return_filters=True, return_status=True)[1:]
    assert not host(G0).any() and not host(s0).any()


def test_a_batch_gives_what_its_signals_give_alone_with_a_silent_row_inside():
    shape, K, delay, c = CASES[2]
    X = np.array(mixture(shape))
    X[1, :, 3] = 0
    Xd = gpu(X)
    Y, G, status = wpe.wpe(Xd, K, delay, 3, psd_context=c, return_filters=True, return_status=True)
    want = np.zeros((3, 5), np.int32)
    want[1, 3] = wpe.STATUS_PIVOT
    assert np.array_equal(host(status), want) and same(Y[1, :, 3], Xd[1, :, 3]) and not host(G[1, 3]).any()
    for n in range(3):
        y1, g1, s1 = wpe.wpe(Xd[n], K, delay, 3, psd_context=c, return_filters=True, return_status=True)
        assert tuple(y1.shape) == shape[1:] and same(y1, Y[n]) and same(g1, G[n]) and same(s1, status[n])
    Yr, Gr, sr, _ = W.wpe_rows(X[1:2, :, 2:4], K, delay, 3, c)                        # the restatement's flags on the same rows
    assert np.array_equal(sr, want[1:2, 2:4]) and np.array_equal(Yr[0, :, 1], X[1, :, 3])


def flatten(res):
    return list(res) if isinstance(res, tuple) else [res]


def test_every_wrapper_stays_inside_its_tensors_and_reads_nothing_undefined():
    """Every new wrapper under tests/footprint.guarded_allocations with both poisons: no guard byte changes, the results are the same bits
    as without guards, every returned tensor is a view of a recorded payload, and the work space of the loop has the size the query
    gives."""
    for i in (0, 2, 4, 6, 7):
        shape, K, delay, c = CASES[i]
        ref = reference(i)
        X, w, Rm, P, G = gpu(mixture(shape)), gpu(ref["w"]), gpu(ref["R"]), gpu(ref["P"]), gpu(ref["G"])
        calls = {"power_inverse": lambda: wpe.power_inverse(X, c, return_max=True), "correlations": lambda: wpe.correlations(X, w, K, delay),
                 "solve": lambda: wpe.solve(Rm, P), "filter": lambda: wpe.filter(X, G, K, delay),
                 "wpe": lambda: wpe.wpe(X, K, delay, 2, psd_context=c, return_filters=True, return_status=True)}
        inputs = [t.clone() for t in (X, w, Rm, P, G)]
        for name, call in calls.items():
            plain = flatten(call())
            for poison in (0xFF, 0x00):
                with guarded_allocations(poison) as rec:
                    res = flatten(call())
                assert rec.violations() == [], (IDS[i], name, poison, rec.violations())
                for k, (a, b) in enumerate(zip(plain, res)):
                    assert same(a, b), (IDS[i], name, poison, k)
                    assert rec.find(b) is not None, (IDS[i], name, poison, k)
                if name == "wpe":
                    nbytes = _lib.load().glowk_wpe_workspace_bytes(shape[0], shape[1], K, shape[2], shape[3])
                    assert nbytes % 8 == 0 and any(a.nbytes == nbytes for a in rec.allocations), (IDS[i], nbytes)
        for t, u in zip((X, w, Rm, P, G), inputs):
            assert same(t, u)


def test_the_audio_wrappers_stay_inside_their_tensors_too(tmp_path):
    """wpe_audio and dereverb_wav under the guards: they add torch allocations and the STFT pair's to the loop's."""
    wet, _ = W.audio_scene()
    yd = gpu(wet[:, :20001])
    src = tmp_path / "room.wav"
    write_wav(src, wet[:, :20001], 22050)
    calls = {"wpe_audio": lambda: wpe.wpe_audio(yd, taps=4, iterations=2), "wpe_audio mono": lambda: wpe.wpe_audio(yd[0], taps=4, iterations=1),
             "dereverb_wav": lambda: wpe.dereverb_wav(str(src), taps=4, iterations=1)[0],
             "dereverb_wav auxiva": lambda: wpe.dereverb_wav(str(src), separate="auxiva", n_iter=2, taps=4, iterations=1)[0]}
    for name, call in calls.items():
        plain = call()
        for poison in (0xFF, 0x00):
            with guarded_allocations(poison) as rec:
                res = call()
            assert rec.violations() == [], (name, poison, rec.violations())
            assert same(plain, res), (name, poison)
            assert rec.find(res) is not None, (name, poison)


# ---- audio -----------------------------------------------------------------------------------------------------------------------------
def write_wav(path, y, rate):
    q = np.rint(np.clip(y, -1.0, 1.0) * 32767.0).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1 if y.ndim == 1 else y.shape[0])
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(np.ascontiguousarray(q.T).tobytes())


@functools.lru_cache(maxsize=None)
def audio_scene():
    return W.audio_scene()


def test_wpe_audio_keeps_shape_and_length_and_zero_iterations_are_the_round_trip():
    wet, _ = audio_scene()
    n = 30001                                                                        # not a multiple of the hop
    for y in (wet[:, :n], wet[0, :n]):
        yd = gpu(y)
        out = wpe.wpe_audio(yd, taps=4, iterations=1)
        assert out.dtype == torch.float32 and tuple(out.shape) == y.shape and bool(torch.isfinite(out).all())
        trip = wpe.wpe_audio(yd, iterations=0)
        Xs = audio.mel_frames(yd, return_stft=True)[1]
        want = audio.istft(Xs)[..., :n].contiguous()
        assert same(trip, want[0] if y.ndim == 1 else want)
        assert float((trip - yd).abs().max()) < 1e-5


def test_the_audio_scene_is_dereverberated_as_in_the_restatement():
    wet, dry = audio_scene()
    out = host(wpe.wpe_audio(gpu(wet), taps=10, delay=3, iterations=3))
    want = W.wpe_audio(wet, 10, 3, 3)
    before, got, ref = W.sdr_db(dry, wet), W.sdr_db(dry, out), W.sdr_db(dry, want)
    print("audio scene: SDR against the early reference %.2f dB -> %.2f dB on the device, %.2f dB in the restatement pipeline" % (before, got, ref))
    record("audio/sdr_in_db", before)
    record("audio/sdr_device_db", got)
    record("audio/sdr_restatement_db", ref)
    assert abs(got - ref) <= 0.05


def test_dereverb_wav_keeps_the_files_rate_and_length_and_feeds_auxiva(tmp_path):
    wet, _ = audio_scene()
    rate = 22050
    y = host(audio.resample(wet, 16000, rate))
    n = y.shape[1] - 7
    src, dst = tmp_path / "room.wav", tmp_path / "dry.wav"
    write_wav(src, y[:, :n], rate)
    out, out_rate = wpe.dereverb_wav(str(src), out=str(dst), taps=6, iterations=2)
    assert out_rate == rate and tuple(out.shape) == (2, n) and bool(torch.isfinite(out).all())
    back, back_rate = audio.load_audio(str(dst), sr=None, mono=False)
    assert back_rate == rate and tuple(back.shape) == (2, n)
    assert float((torch.as_tensor(back).cuda() - out.clamp(-1, 1)).abs().max()) <= 2.0 / 32768          # the 16-bit file's own rounding
    mono, mono_rate = wpe.dereverb_wav(y[0, :n], sr=rate, taps=6, iterations=1)
    assert mono_rate == rate and tuple(mono.shape) == (n,)
    stems, stems_rate = wpe.dereverb_wav(str(src), separate="auxiva", n_iter=3, taps=6, iterations=2)
    ref_stems, ref_rate = iva.separate_wav_iva(str(src), n_iter=3)
    assert stems_rate == ref_rate == rate and stems.shape == ref_stems.shape == (2, 2, n) and stems.dtype == ref_stems.dtype
    assert bool(torch.isfinite(stems).all()) and float(stems.abs().max()) > 1e-3
    with pytest.raises(ValueError, match="two to four channels"):
        wpe.dereverb_wav(y[0, :n], sr=rate, separate="ilrma")
