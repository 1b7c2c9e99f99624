"""Melody separation on the GPU against the fp64 restatement of tests/melody_ref.py, on every cell of every shape.

Bars.  Salience, from the same float32 S: |d| <= 2^-24 |sal| + (H + 4) 2^-52 sum_h |term_h| + 2^-149 (the final rounding, the five fp64
roundings of a term and the H - 1 of the sum on each side).  Emission: the maximum exact, |de| <= 2^-52 e (one division on each side).
Track: fed the device's own emission plane, the device's path equals the restatement's in every frame.  Mask, from the device's own
path: |dm| <= 2^-24 + 2^-52 (4 + 3 R bin_hz / width).  Staged calls and the fused call, a batch and its signals alone, one run and the
next: bit for bit.  Audio: lead + accompaniment returns y within 1e-5 of its peak, the bar tests/test_gpu_hpss.py holds the HPSS stems'
sum to.

Largest fractions of the bounds reached on an MI355X: salience 0.998 (the final rounding to float32: the device's plane is held
against the restatement's fp64 sum), emission 0.000 (every division gave the restatement's bits), mask 0.500 (the float32 rounding just
below 1); every path equal.  The scene: 96 of 97 lead frames within 50 cents and SDR gains of +6.7881 dB and +8.3744 dB on the device
as in the restatement; lead + accompaniment - y 1.5e-6 of the peak."""
import ctypes
import functools
import wave

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, audio, melody
from tests import melody_ref as M
from tests.test_gpu_hpss import AUDIO_BAR

pytestmark = pytest.mark.gpu

BIN_HZ = M.BIN_HZ
# (N, R, T, B, H, J)
SHAPES = [
    (1, 2, 1, 1, 1, 0), (1, 2, 2, 2, 1, 0), (1, 3, 5, 2, 2, 5), (2, 9, 7, 5, 3, 1), (1, 33, 63, 63, 8, 12), (1, 33, 64, 64, 8, 12),
    (3, 65, 65, 65, 8, 64), (1, 129, 255, 17, 32, 3), (1, 129, 256, 300, 8, 12), (1, 17, 257, 1024, 2, 1023), (1, 1025, 126, 300, 8, 12),
    (1, 4, 4100, 3, 1, 1),
    # the edges of these kernels
    (1, 4096, 11, 5, 32, 2),                              # the most rows and harmonics.  The salience has 256 (bin, frame) pairs per
                                                          # workgroup: 64 x 64 above fills 16 exactly, 300 x 256 fills 300, the rest leave
                                                          # a part of a signal's last one idle
    (1, 9, 20, 62, 2, 3),                                 # the track's threads: B = 62, 63 fill one wave with the unvoiced state's
    (1, 17, 40, 1023, 2, 5),                              # thread (63, 64 above: it opens a second wave); 1023 fills 1024 threads,
                                                          # and at 1024 (above) thread 0 owns bin 0 and the unvoiced state
    (1, 4, 4609, 3, 1, 1), (1, 4, 4610, 3, 1, 1),         # the back-trace chunk of 18432 / (B + 1) = 4608 frames: one chunk, two chunks
    (2, 5, 123, 300, 4, 12),                              # B = 300: chunks of 61 frames, 122 = 2 x 61 back pointers exactly (126: a rest)
]
IDS = ["-".join(map(str, s)) for s in SHAPES]
reached = {"salience": 0.0, "emission": 0.0, "mask": 0.0}


def grid_for(R, B, H):
    """B fundamentals whose lowest has every harmonic below the last row and whose highest has some (all, for H = 1) beyond it."""
    top = (R - 1) * BIN_HZ
    g = np.geomspace(top / (3.0 * H), top * (1.2 if H == 1 else 0.7), B) if B > 1 else np.array([top / 3.0])
    assert (np.diff(g) > 0).all()
    return g


@functools.lru_cache(maxsize=None)
def case(shape):
    """(S float32 [N, R, T], grid, weights) of a shape and the device's salience, emission and maximum of it.  Never modified."""
    N, R, T, B, H, J = shape
    rng = np.random.default_rng(abs(hash(shape)) % (1 << 32))
    S = (rng.random((N, R, T)) ** 3).astype(np.float32)
    S[rng.random(S.shape) < 0.1] = 0.0
    grid, w = grid_for(R, B, H), M.weights(H, 0.8)
    sal = melody.salience(S, grid, weights=w)
    e, m = melody.emission(sal, return_max=True)
    out = (S, grid, w, sal.cpu().numpy(), e.cpu().numpy(), m.cpu().numpy())
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_salience(shape):
    N, R, T, B, H, J = shape
    S, grid, w, sal, _, _ = case(shape)
    assert sal.shape == (N, B, T) and sal.dtype == np.float32
    dead = ~M.positions(grid, H, BIN_HZ, R)[2]
    assert dead.any() or (B == 1 and H == 1), "no harmonic beyond the last row"
    worst, other = 0.0, 0
    for n in range(N):
        want32, want, weight = M.salience(S[n], grid, w, return_weight=True)
        bound = 2.0 ** -24 * np.abs(want) + (H + 4) * 2.0 ** -52 * weight + 2.0 ** -149
        frac = float((np.abs(sal[n].astype(np.float64) - want) / bound).max())
        worst = max(worst, frac)
        other += int((sal[n].view(np.uint32) != want32.view(np.uint32)).sum())
    reached["salience"] = max(reached["salience"], worst)
    print("salience %s: %.3f of the bound (largest so far %.3f); %d cells differ in bits from the restatement's float32" %
          (shape, worst, reached["salience"], other))
    assert worst <= 1.0


def test_salience_with_a_batch_on_the_default_grid_and_decay():
    S = case(SHAPES[10])[0]
    sal = melody.salience(S[0], melody.f0_grid()).cpu().numpy()
    want, acc, weight = M.salience(S[0], M.f0_grid(), M.weights(), return_weight=True)
    assert (np.abs(sal - acc) <= 2.0 ** -24 * np.abs(acc) + 12 * 2.0 ** -52 * weight + 2.0 ** -149).all()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_emission(shape):
    N, R, T, B, H, J = shape
    _, _, _, sal, e, m = case(shape)
    worst = 0.0
    for n in range(N):
        want, wm = M.emission(sal[n])
        assert m.reshape(N)[n] == wm
        err = np.abs(e[n] - want)
        assert (err <= 2.0 ** -52 * want).all()
        worst = max(worst, float((err[want > 0] / (2.0 ** -52 * want[want > 0])).max()) if (want > 0).any() else 0.0)
    reached["emission"] = max(reached["emission"], worst)
    print("emission %s: %.3f of the bound (largest so far %.3f)" % (shape, worst, reached["emission"]))


@pytest.mark.parametrize("B,T", [(1024, 1024), (1024, 1025), (3, 1400), (1, 1)], ids=str)
def test_emission_on_either_side_of_the_256_partial_maxima_and_of_a_zero_plane(B, T):
    """4096 x 256 cells are the most that get a partial maximum per 4096 (the shapes above have up to 65 groups; 64 x 64 and 65 x 65
    straddle one group); the plane's maximum sits in its last cell, then in its first; an all-zero plane divides by 2^-40."""
    rng = np.random.default_rng(B + T)
    sal = rng.random((B, T)).astype(np.float32)
    for where in (-1, 0):
        sal.reshape(-1)[where] = 2.0
        e, m = melody.emission(sal, return_max=True)
        want, wm = M.emission(sal)
        assert float(m) == 2.0 == wm and (np.abs(e.cpu().numpy() - want) <= 2.0 ** -52 * want).all()
        sal.reshape(-1)[where] = 0.5
    e, m = melody.emission(np.zeros((B, T), np.float32), return_max=True)
    assert float(m) == 0.0 and not bool(e.any())
    tiny = np.full((B, T), 2.0 ** -60, np.float32)
    assert bool((melody.emission(tiny) == 2.0 ** -20).all())


def quarter_plane(shape, seed):
    N, R, T, B, H, J = shape
    return np.round(np.random.default_rng(seed).random((N, B, T)) * 4) / 4


def paths_equal(e, **kw):
    got = melody.track(e, **kw).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (e.shape[0], e.shape[2])
    for n in range(e.shape[0]):
        want = M.track(e[n], kw["threshold"], kw["jump_penalty"], kw["voicing_penalty"], kw["max_jump"])
        diff = np.nonzero(got[n] != want)[0]
        assert len(diff) == 0, "signal %d: %d frames differ, first %d: %d against %d" % (n, len(diff), diff[0], got[n][diff[0]], want[diff[0]])
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_track_equals_the_restatement(shape):
    """The device's own emission plane and a plane of multiples of 1/4 (many exact ties, with jump penalties of 1/4 and 0) at the
    shape's J; the all-zero plane; theta above and below every emission; nu = 0; J = 0 and J >= B.  Where the shape's J is large the
    further planes run with J = 12: the restatement's table has 2 J + 2 columns."""
    N, R, T, B, H, J = shape
    e = case(shape)[4]
    q = quarter_plane(shape, 7)
    Jv = min(J, 12)
    base = dict(threshold=0.2, jump_penalty=0.02, voicing_penalty=0.5, max_jump=J)
    voiced = paths_equal(e, **base)
    paths_equal(q, threshold=0.5, jump_penalty=0.25, voicing_penalty=0.5, max_jump=J)
    small = dict(base, max_jump=Jv)
    paths_equal(q, **dict(small, threshold=0.75, jump_penalty=0.0, voicing_penalty=0.25))
    zero = np.zeros_like(q)
    for kw in (small, dict(small, threshold=0.0, jump_penalty=0.0, voicing_penalty=0.0), dict(small, threshold=0.0, jump_penalty=0.0)):
        paths_equal(zero, **kw)
    above = paths_equal(e, **dict(small, threshold=2.0))
    below = paths_equal(e, **dict(small, threshold=-1.0))
    # theta = 2 beats every emission (<= 1) in every frame; with theta = -1 the path starts and ends in a bin (>= 0 against -1), though
    # it may still cross the unvoiced state to reach a distant bin
    assert (above == B).all() and (below[:, 0] < B).all() and (below[:, -1] < B).all()
    paths_equal(q, **dict(small, threshold=0.5, jump_penalty=0.25, voicing_penalty=0.0))
    paths_equal(e, **dict(small, voicing_penalty=0.0))
    paths_equal(q, **dict(base, threshold=0.5, jump_penalty=0.25, max_jump=0))
    paths_equal(e, **dict(base, max_jump=0))
    if B <= 300:
        paths_equal(q, **dict(base, threshold=0.5, jump_penalty=0.25, max_jump=B))
        paths_equal(e, **dict(base, max_jump=min(B + 7, 1023)))
    assert voiced.min() >= 0 and voiced.max() <= B


def test_the_all_zero_plane_gives_the_hand_derived_paths():
    """tests/test_melody_cpu.py derives them: with theta = nu = jump_penalty = 0 every back pointer is B and the end is state 0."""
    e = np.zeros((4, 6))
    assert melody.track(e, 0.0, 0.0, 0.0, 2).tolist() == [4, 4, 4, 4, 4, 0]
    assert melody.track(e, 0.0, 0.0, 0.5, 1).tolist() == [0] * 6
    assert melody.track(e).tolist() == [4] * 6
    big = np.zeros((1024, 40))
    assert melody.track(big, 0.0, 0.0, 0.0, 1023).tolist() == [1024] * 39 + [0]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mask_and_the_three_reproducibilities(shape):
    N, R, T, B, H, J = shape
    S, grid, w, sal, e, m = case(shape)
    width, Hm = 2.5 * BIN_HZ, 20
    kw = dict(threshold=0.2, jump_penalty=0.02, voicing_penalty=0.5, max_jump=J)
    path = melody.track(e, **kw)
    mask = melody.harmonic_mask(path, grid, rows=R, n_harmonics=Hm, width=width)
    assert tuple(mask.shape) == (N, R, T) and mask.dtype == torch.float32
    got, p = mask.cpu().numpy(), path.cpu().numpy()
    bound = 2.0 ** -24 + 2.0 ** -52 * (4 + 3 * R * BIN_HZ / width)
    worst, other = 0.0, 0
    for n in range(N):
        want = M.harmonic_mask(p[n], grid, R, Hm, width, BIN_HZ, as_float64=True)
        worst = max(worst, float(np.abs(got[n] - want).max() / bound))
        other += int((got[n] != want.astype(np.float32)).sum())
        assert not got[n][:, p[n] == B].any()
    reached["mask"] = max(reached["mask"], worst)
    print("mask %s: %.3f of the bound (largest so far %.3f); %d cells differ from the restatement's float32; %d of %d frames voiced" %
          (shape, worst, reached["mask"], other, int((p < B).sum()), p.size))
    assert worst <= 1.0
    # staged calls and the fused call
    fused = melody.melody(S, f0s=grid, weights=w, n_harmonics=Hm, width=width, power=1, mask=True, return_f0=True, **kw)
    assert torch.equal(fused[0], mask) and torch.equal(fused[1], 1.0 - mask)
    table = torch.cat([torch.from_numpy(grid), torch.zeros(1, dtype=torch.float64)]).cuda()
    assert torch.equal(fused[2], table[path.long()])
    # one run and the next
    again = melody.melody(torch.from_numpy(S).cuda(), f0s=grid, weights=w, n_harmonics=Hm, width=width, power=1, mask=True, return_f0=True, **kw)
    assert all(torch.equal(a, b) for a, b in zip(fused, again))
    assert torch.equal(melody.track(e, **kw), path) and torch.equal(melody.salience(S, grid, weights=w).cpu(), torch.from_numpy(sal))
    # a batch and its signals alone
    if N > 1:
        for n in range(N):
            alone = melody.melody(S[n], f0s=grid, weights=w, n_harmonics=Hm, width=width, power=1, mask=True, return_f0=True, **kw)
            assert all(torch.equal(a, b[n]) for a, b in zip(alone, fused))
            assert torch.equal(melody.salience(S[n], grid, weights=w).cpu(), torch.from_numpy(sal[n]))
            en, mn = melody.emission(sal[n], return_max=True)
            assert torch.equal(en.cpu(), torch.from_numpy(e[n])) and float(mn) == m[n]
            assert torch.equal(melody.track(e[n], **kw), path[n]) and torch.equal(melody.harmonic_mask(path[n], grid, R, Hm, width), mask[n])


def test_the_separator_masks_spectra_and_keeps_the_phase():
    S, grid, w = case(SHAPES[6])[:3]
    kw = dict(f0s=grid, weights=w, width=2.5 * BIN_HZ, max_jump=64)
    x = torch.from_numpy(S).cuda()
    m, rest = melody.melody(S, power=1, mask=True, **kw)
    for power in (1, 2.0, float("inf")):
        ml, ma = melody.melody(S, power=power, mask=True, **kw)
        lead, acc = melody.melody(S, power=power, **kw)
        assert torch.equal(lead, ml * x) and torch.equal(acc, ma * x)
        want_l = M.softmask((m * x).cpu().numpy(), (rest * x).cpu().numpy(), power) if power != 1 else m.cpu().numpy()
        want_a = M.softmask((rest * x).cpu().numpy(), (m * x).cpu().numpy(), power) if power != 1 else rest.cpu().numpy()
        assert np.abs(ml.cpu().numpy() - want_l).max() <= 1e-6 and np.abs(ma.cpu().numpy() - want_a).max() <= 1e-6     # glowk_hpss_mask's bar
    ph = np.exp(2j * np.pi * np.random.default_rng(3).random(S.shape))
    lead_c, acc_c = melody.melody((S * ph).astype(np.complex64), **kw)
    lead, acc = melody.melody(np.abs((S * ph).astype(np.complex64)), **kw)
    assert lead_c.dtype == torch.complex64 and float((lead_c.abs() - lead).abs().max()) <= 1e-6 * float(lead.max())
    live = lead.cpu().numpy() > 1e-3
    assert live.any() and np.abs(lead_c.cpu().numpy()[live] / lead.cpu().numpy()[live] - ph[live]).max() <= 1e-6
    assert float((acc_c.abs() - acc).abs().max()) <= 1e-6 * float(acc.max())
    empty = torch.empty((0, 9, 4), device="cuda")
    assert all(tuple(t.shape) == (0, 9, 4) for t in melody.melody(empty, f0s=grid)) and tuple(melody.salience(empty, grid).shape) == (0, 65, 4)


@functools.lru_cache(maxsize=None)
def the_scene():
    lead, acc, f0_true, lead_on = M.scene()
    out = (lead, acc, lead + acc, f0_true, lead_on)
    for a in out:
        a.setflags(write=False)
    return out


def test_the_scene_end_to_end():
    lead, acc, y, f0_true, lead_on = the_scene()
    _, X = audio.mel_frames(np.stack([y, lead, acc]), return_stft=True)
    assert tuple(X.shape) == (3, 1025, 126)
    mag = X[0].abs().contiguous()
    ml, ma, f0_hat = melody.melody(mag, mask=True, return_f0=True)
    Xn = X.cpu().numpy().astype(np.complex128)
    dev = M.scene_figures(Xn[1], Xn[2], Xn[0], f0_true, lead_on, ml.cpu().numpy().astype(np.float64), ma.cpu().numpy().astype(np.float64), f0_hat.cpu().numpy())
    wl, wa, _, wf0 = M.melody(mag.cpu().numpy())
    ref = M.scene_figures(Xn[1], Xn[2], Xn[0], f0_true, lead_on, wl, wa, wf0)
    base = (M.sdr(Xn[1], Xn[0]), M.sdr(Xn[2], Xn[0]))
    print("scene: device %d of %d lead frames within 50 cents, SDR gains %+.4f dB (lead) %+.4f dB (accompaniment)" % dev)
    print("scene: restatement %d of %d, %+.4f dB, %+.4f dB; the mixture itself %.2f dB, %.2f dB; %d frames differ in f0" %
          (ref + base + (int((f0_hat.cpu().numpy() != wf0).sum()),)))
    assert dev[0] >= ref[0] - 2 and abs(dev[2] - ref[2]) <= 0.1 and abs(dev[3] - ref[3]) <= 0.1
    assert ref[0] >= 0.9 * ref[1] and ref[2] >= 3.0 and ref[3] >= 3.0


@pytest.mark.parametrize("power", [1, 2.0])
def test_melody_audio_stems_add_up_to_the_input(power):
    y = the_scene()[2]
    peak = float(np.abs(y).max())
    lead, acc = melody.melody_audio(y.copy(), power=power)
    assert lead.is_cuda and lead.dtype == torch.float32 and tuple(lead.shape) == tuple(acc.shape) == y.shape
    e_sum = float(np.abs(lead.cpu().numpy().astype(np.float64) + acc.cpu().numpy() - y).max() / peak)
    # aligned with y: the lead stem correlates with the true lead at lag 0 better than at any lag of up to a hop
    true = torch.from_numpy(the_scene()[0].copy()).cuda()
    corr = [float((lead[512:-512] * true[512 + lag:len(true) - 512 + lag]).sum()) for lag in (-512, -64, -1, 0, 1, 64, 512)]
    print("melody_audio power = %s: lead + accompaniment - y %.2e of the peak; correlation with the true lead by lag %s" % (power, e_sum, np.round(corr, 1)))
    assert e_sum <= AUDIO_BAR and int(np.argmax(corr)) == 3
    two = np.stack([y, 0.5 * y[::-1]]).astype(np.float32)
    l2, a2 = melody.melody_audio(two, power=power)
    assert tuple(l2.shape) == (2, len(y)) and torch.equal(l2[0], lead) and torch.equal(a2[0], acc)       # a channel's stems depend on it alone


def test_separate_wav_melody_returns_the_files_rate_and_length(tmp_path):
    rate, n = 44100, 60000
    t = np.arange(n) / rate
    y = 0.3 * sum(np.sin(2 * np.pi * 440.0 * h * t) / h for h in range(1, 6)) + 0.2 * np.sin(2 * np.pi * 110.0 * t)
    q = np.rint(np.clip(np.stack([y, 0.5 * y]), -1.0, 1.0) * 32767.0).astype("<i2")
    path = tmp_path / "stereo.wav"
    with wave.open(str(path), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(q.T).tobytes())
    stems, out_rate = melody.separate_wav_melody(str(path))
    assert out_rate == rate and tuple(stems.shape) == (2, 2, n) and bool(torch.isfinite(stems).all()) and float(stems.abs().max()) > 0.05
    stems, out_rate = melody.separate_wav_melody(str(path), mono=True, out_rate=None, power=1)
    assert out_rate == audio.SR and stems.dim() == 2 and stems.shape[0] == 2


def test_bad_calls_are_refused_with_a_message_and_launch_nothing():
    lib = _lib.load()
    R, T, B, H, J = 12, 30, 5, 3, 2
    grid = grid_for(R, B, H)
    dev = lambda a, dt: torch.as_tensor(a, dtype=dt).cuda()
    x = torch.rand(R, T, device="cuda")
    idx, frac, w = dev(np.zeros((B, H)), torch.int32), dev(np.zeros((B, H)), torch.float64), dev(np.ones(H), torch.float64)
    f0, pen = dev(grid, torch.float64), dev(np.arange(J + 1) * 0.02, torch.float64)
    sal = torch.full((B, T), 7.0, device="cuda")
    e = torch.full((B, T), 7.0, dtype=torch.float64, device="cuda")
    m = torch.full((1,), 7.0, device="cuda")
    path = torch.full((T,), 7, dtype=torch.int32, device="cuda")
    mask = torch.full((R, T), 7.0, device="cuda")
    nbytes = lib.glowk_melody_workspace_bytes(1, B, T)
    work = torch.zeros(nbytes // 8 + 64, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    z = ctypes.c_void_p(0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    err = lambda: lib.glowk_last_error().decode()
    host = np.zeros((R, T), np.float32)
    hp = host.ctypes.data_as(ctypes.c_void_p)
    big = work.numel() * 8
    S = lambda **k: lib.glowk_melody_salience(k.get("s", p(x)), k.get("nsig", 1), k.get("rows", R), k.get("frames", T), p(idx), p(frac), p(w), k.get("B", B),
                                              k.get("H", H), k.get("out", p(sal)), st)
    E = lambda **k: lib.glowk_melody_emission(k.get("s", p(sal)), k.get("nsig", 1), k.get("B", B), k.get("frames", T), k.get("out", p(e)), p(m), k.get("work", p(work)),
                                              k.get("nbytes", big), st)
    K = lambda **k: lib.glowk_melody_track(k.get("e", p(e)), k.get("nsig", 1), k.get("B", B), k.get("frames", T), p(pen), k.get("J", J), k.get("theta", 0.2),
                                           k.get("nu", 0.5), k.get("out", p(path)), z, k.get("work", p(work)), k.get("nbytes", big), st)
    Q = lambda **k: lib.glowk_melody_mask(k.get("path", p(path)), k.get("nsig", 1), k.get("frames", T), p(f0), k.get("B", B), k.get("rows", R), k.get("Hm", 20),
                                          k.get("width", 40.0), k.get("bin_hz", BIN_HZ), k.get("out", p(mask)), st)
    F = lambda **k: lib.glowk_melody_fit(k.get("s", p(x)), k.get("nsig", 1), k.get("rows", R), k.get("frames", T), p(idx), p(frac), p(w), p(f0), k.get("B", B),
                                         k.get("H", H), p(pen), k.get("J", J), k.get("theta", 0.2), 0.5, k.get("Hm", 20), k.get("width", 40.0), BIN_HZ, p(path),
                                         k.get("mask", p(mask)), p(m), k.get("work", p(work)), k.get("nbytes", big), st)
    bad = [
        (S, dict(nsig=-1), "nsig"), (S, dict(nsig=65536), "nsig"), (S, dict(rows=1), "rows"), (S, dict(rows=4097), "rows"), (S, dict(frames=0), "frames"),
        (S, dict(frames=32769), "frames"), (S, dict(B=0), "B must"), (S, dict(B=1025), "B must"), (S, dict(H=0), "H must"), (S, dict(H=33), "H must"),
        (S, dict(nsig=65535, rows=4096, frames=9), "2^31"), (S, dict(s=hp), "device memory"), (S, dict(out=p(x)), "overlap"), (S, dict(s=z), "null"),
        (E, dict(nsig=65536), "nsig"), (E, dict(B=1025), "B must"), (E, dict(frames=32769), "frames"), (E, dict(nsig=64, B=1024, frames=32768), "2^31"),
        (E, dict(nbytes=0), "work_bytes"), (E, dict(s=hp), "device memory"), (E, dict(work=p(e)), "overlap"),
        (K, dict(nsig=-1), "nsig"), (K, dict(B=0), "B must"), (K, dict(frames=0), "frames"), (K, dict(J=-1), "J must"), (K, dict(J=1024), "J must"),
        (K, dict(theta=float("nan")), "finite"), (K, dict(nu=float("inf")), "finite"), (K, dict(nbytes=8), "work_bytes"), (K, dict(e=hp), "device memory"),
        (K, dict(work=p(e)), "overlap"),
        (Q, dict(rows=1), "rows"), (Q, dict(rows=4097), "rows"), (Q, dict(Hm=0), "Hm must"), (Q, dict(Hm=1025), "Hm must"), (Q, dict(width=0.0), "width"),
        (Q, dict(width=float("inf")), "width"), (Q, dict(bin_hz=-1.0), "bin_hz"), (Q, dict(path=hp), "device memory"), (Q, dict(out=p(path)), "overlap"),
        (F, dict(nsig=65536), "nsig"), (F, dict(rows=1), "rows"), (F, dict(frames=32769), "frames"), (F, dict(B=1025), "B must"), (F, dict(H=33), "H must"),
        (F, dict(J=1024), "J must"), (F, dict(theta=float("inf")), "finite"), (F, dict(Hm=0), "Hm must"), (F, dict(width=-1.0), "width"),
        (F, dict(nbytes=nbytes - 1), "work_bytes"), (F, dict(s=hp), "device memory"), (F, dict(mask=p(x)), "overlap"), (F, dict(work=p(x)), "overlap"),
    ]
    for n, (call, kw, word) in enumerate(bad):
        assert call(**kw) == _lib.ERR and word in err(), (n, kw, err())
    torch.cuda.synchronize()
    for canary in (sal, e, m, mask):
        assert bool((canary == 7.0).all())
    assert bool((path == 7).all()) and not bool(work.any())                              # nothing was launched
    assert S(nsig=0) == E(nsig=0) == K(nsig=0) == Q(nsig=0) == F(nsig=0) == _lib.OK
    assert F(nbytes=nbytes) == _lib.OK                                                   # and the valid call goes through
    torch.cuda.synchronize()
    assert not bool((mask == 7.0).any()) and not bool((path == 7).any()) and float(m) != 7.0
