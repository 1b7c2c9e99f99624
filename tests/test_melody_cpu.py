"""Melody separation without a GPU: the restatement of tests/melody_ref.py on the synthetic scene and on planes of exact ties, the
Python argument checks of ``audiosourcesep_amd.melody`` (ValueError with the argument's name before the library is loaded), the boundary
of the C entries (declared, exported, bound with the header's signatures; every refusal before any device call), and the host-side
rules the kernels share with the host under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, melody
from tests import melody_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ("glowk_melody_positions", "glowk_melody_emission_workspace_bytes", "glowk_melody_track_workspace_bytes", "glowk_melody_workspace_bytes",
         "glowk_melody_salience", "glowk_melody_emission", "glowk_melody_track", "glowk_melody_mask", "glowk_melody_fit")


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def test_the_restatement_tracks_and_separates_the_scene():
    """The prototype's figures: 96 of 97 lead frames within 50 cents, +6.8 dB (lead) and +8.4 dB (accompaniment).  The margins only guard
    against a scene or a default that stops working."""
    lead, acc, f0_true, lead_on = M.scene()
    Xl, Xa = M.stft(lead), M.stft(acc)
    Xm = Xl + Xa
    assert Xm.shape == (1025, 126) and int(lead_on.sum()) == 97
    for power in (2.0, 1):
        ml, ma, path, f0_hat = M.melody(np.abs(Xm).astype(np.float32), power=power)
        hit, total, gain_l, gain_a = M.scene_figures(Xl, Xa, Xm, f0_true, lead_on, ml, ma, f0_hat)
        print("power %s: %d of %d lead frames within 50 cents, SDR gains %+.2f dB (lead) %+.2f dB (accompaniment)" % (power, hit, total, gain_l, gain_a))
        assert hit >= 0.9 * total and gain_l >= 3.0 and gain_a >= 3.0
        assert path.dtype == np.int32 and path.min() >= 0 and path.max() <= 300 and (f0_hat[path == 300] == 0).all()


def test_ties_follow_the_order_rule():
    """An all-zero emission plane, B = 4, T = 6, derived by hand.
    (a) theta = nu = jump_penalty = 0: every score stays 0.  A voiced state's first candidate is state B (0), and no later candidate is
        strictly greater: every voiced back pointer is B; the unvoiced state's first candidate is itself.  The first maximum at the end
        is state 0, whose back pointer leads to B, where the path stays: B B B B B 0.
    (b) theta = 0, nu = 0.5, jump_penalty = 0, J = 1: state B offers -0.5, the first bin of the window, max(0, b - 1), offers 0 and wins;
        the unvoiced state keeps 0 against -0.5.  All scores stay 0, the end is state 0, and 0's back pointer is 0: all zeros.
    (c) the defaults: the unvoiced state gains theta = 0.2 per frame and the bins gain nothing: unvoiced throughout."""
    e = np.zeros((4, 6))
    for fn in (M.track, M.track_loops):
        assert fn(e, 0.0, 0.0, 0.0, 2).tolist() == [4, 4, 4, 4, 4, 0]
        assert fn(e, 0.0, 0.0, 0.5, 1).tolist() == [0, 0, 0, 0, 0, 0]
        assert fn(e, 0.2, 0.02, 0.5, 12).tolist() == [4] * 6
    assert M.track(np.zeros((3, 1)), 0.0, 0.0, 0.0, 0).tolist() == [0] and M.track(np.zeros((3, 1)), 0.2, 0.0, 0.0, 0).tolist() == [3]
    # and the candidate table agrees with the plain loops where ties are frequent
    rng = np.random.default_rng(1)
    for B, T, J in [(5, 9, 1), (7, 12, 3), (4, 6, 10), (6, 8, 0), (1, 5, 0)]:
        q = np.round(rng.random((B, T)) * 4) / 4
        for theta, nu in [(0.25, 0.5), (0.5, 0.0), (2.0, 0.25), (-1.0, 0.25)]:
            assert np.array_equal(M.track(q, theta, 0.25, nu, J), M.track_loops(q, theta, 0.25, nu, J)), (B, T, J, theta, nu)


def test_dead_terms_and_the_mask_edges():
    f0 = np.array([100.0, 150.0, 900.0])
    i, a, live = M.positions(f0, 4, 100.0, 6)                                          # rows 0 .. 5: a term needs i + 1 <= 5
    assert live.tolist() == [[True, True, True, True], [True, True, True, False], [False, False, False, False]]
    assert i[0].tolist() == [1, 2, 3, 4] and not a[0].any() and i[1, :3].tolist() == [1, 3, 4] and a[1, :3].tolist() == [0.5, 0.0, 0.5]
    S = np.arange(12, dtype=np.float32).reshape(6, 2)
    sal = M.salience(S, f0, np.array([1.0, 0.5, 0.25, 0.125]), 100.0)
    assert sal[0].tolist() == [2 + 2 + 1.5 + 1, 3 + 2.5 + 1.75 + 1.125] and sal[1].tolist() == [3 + 3 + 2.25, 4 + 3.5 + 2.5] and not sal[2].any()
    m = M.harmonic_mask(np.array([0, 3, 2, -1]), f0, rows=6, n_harmonics=2, width=50.0, bin_hz=100.0)
    assert m[:, 0].tolist() == [0, 1, 1, 0, 0, 0] and not m[:, 1].any() and not m[:, 3].any() and not m[:, 2].any()
    m = M.harmonic_mask(np.array([1]), f0, rows=6, n_harmonics=3, width=100.0, bin_hz=100.0)
    assert m[:, 0].tolist() == [0, 0.5, 0.5, 1, 0.5, 0.5]


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def test_bad_arguments_are_refused_before_the_library_loads(no_library, tmp_path):
    meta = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="meta")      # shapes without storage
    S, f0 = np.ones((4, 3), np.float32), np.array([10.0, 20.0])
    e, path = np.zeros((2, 3)), np.zeros(3, np.int32)
    wav = str(tmp_path / "never_opened.wav")
    bad = [
        # section 1's range edges, each with the argument's name
        (lambda: melody.salience(meta(65536, 2, 1), f0), "S"),                           # nsig
        (lambda: melody.salience(np.ones((1, 3), np.float32), f0), "S"),                 # rows
        (lambda: melody.salience(meta(4097, 3), f0), "S"),
        (lambda: melody.salience(np.ones((4, 0), np.float32), f0), "S"),                 # frames
        (lambda: melody.salience(meta(4, 32769), f0), "S"),
        (lambda: melody.salience(meta(65535, 4096, 9), f0), "S"),                        # nsig rows frames
        (lambda: melody.salience(meta(64, 2, 32768), np.arange(1, 1025.0)), "f0s"),      # nsig (B + 1) frames
        (lambda: melody.salience(S, np.zeros(0)), "f0s"),                                # B
        (lambda: melody.salience(S, np.arange(1, 1026.0)), "f0s"),
        (lambda: melody.salience(S, f0, harmonics=0), "harmonics"),                      # H
        (lambda: melody.salience(S, f0, harmonics=33), "harmonics"),
        (lambda: melody.salience(S, f0, weights=np.ones(0)), "weights"),
        (lambda: melody.salience(S, f0, weights=np.ones(33)), "weights"),
        (lambda: melody.melody(meta(65536, 2, 1)), "S"),
        (lambda: melody.melody(np.ones((1, 3), np.float32)), "S"),
        (lambda: melody.melody(meta(4097, 3)), "S"),
        (lambda: melody.melody(meta(4, 32769)), "S"),
        (lambda: melody.melody(meta(65535, 4096, 9)), "S"),
        (lambda: melody.melody(meta(64, 2, 32768), f0s=np.arange(1, 1025.0)), "f0s"),
        (lambda: melody.melody(S, f0s=np.arange(1, 1026.0)), "f0s"),
        (lambda: melody.melody(S, harmonics=33), "harmonics"),
        (lambda: melody.emission(meta(65536, 1, 1)), "sal"),
        (lambda: melody.emission(meta(1025, 3)), "sal"),
        (lambda: melody.emission(meta(0, 3)), "sal"),
        (lambda: melody.emission(meta(2, 32769)), "sal"),
        (lambda: melody.emission(meta(64, 1024, 32768)), "sal"),
        (lambda: melody.track(meta(65536, 1, 1, dtype=torch.float64)), "e"),
        (lambda: melody.track(meta(1025, 3, dtype=torch.float64)), "e"),
        (lambda: melody.track(meta(2, 0, dtype=torch.float64)), "e"),
        (lambda: melody.track(meta(2, 32769, dtype=torch.float64)), "e"),
        (lambda: melody.track(meta(64, 1024, 32768, dtype=torch.float64)), "e"),
        (lambda: melody.track(e, max_jump=-1), "max_jump"),                              # J
        (lambda: melody.track(e, max_jump=1024), "max_jump"),
        (lambda: melody.harmonic_mask(path, f0, rows=1), "rows"),
        (lambda: melody.harmonic_mask(path, f0, rows=4097), "rows"),
        (lambda: melody.harmonic_mask(meta(32769, dtype=torch.int32), f0), "path"),
        (lambda: melody.harmonic_mask(meta(65536, 1, dtype=torch.int32), f0), "path"),
        (lambda: melody.harmonic_mask(meta(65535, 9, dtype=torch.int32), f0, rows=4096), "rows"),
        (lambda: melody.harmonic_mask(path, f0, n_harmonics=0), "n_harmonics"),          # Hm
        (lambda: melody.harmonic_mask(path, f0, n_harmonics=1025), "n_harmonics"),
        (lambda: melody.harmonic_mask(path, f0, width=0.0), "width"),
        # the tables and the scalars
        (lambda: melody.salience(S, np.array([20.0, 10.0])), "f0s"),
        (lambda: melody.salience(S, np.array([10.0, 10.0])), "f0s"),
        (lambda: melody.salience(S, np.array([0.0, 10.0])), "f0s"),
        (lambda: melody.salience(S, np.array([10.0, np.inf])), "f0s"),
        (lambda: melody.salience(S, np.ones((2, 2))), "f0s"),
        (lambda: melody.salience(S, f0, decay=0.0), "decay"),
        (lambda: melody.salience(S, f0, weights=np.array([1.0, -1.0])), "weights"),
        (lambda: melody.salience(S, f0, weights=np.array([1.0, np.nan])), "weights"),
        (lambda: melody.salience(S, f0, bin_hz=0.0), "bin_hz"),
        (lambda: melody.salience(S, f0, bin_hz=float("inf")), "bin_hz"),
        (lambda: melody.salience(S.astype(np.complex64), f0), "S"),
        (lambda: melody.salience(np.ones(4, np.float32), f0), "S"),
        (lambda: melody.track(e, threshold=float("nan")), "threshold"),
        (lambda: melody.track(e, jump_penalty=-0.1), "jump_penalty"),
        (lambda: melody.track(e, voicing_penalty=float("inf")), "voicing_penalty"),
        (lambda: melody.track(e, max_jump=1.5), "max_jump"),
        (lambda: melody.harmonic_mask(path.astype(np.float32), f0), "path"),
        (lambda: melody.harmonic_mask(path, f0, width=float("nan")), "width"),
        (lambda: melody.melody(S, power=0), "power"),
        (lambda: melody.melody(S, mask=1), "mask"),
        (lambda: melody.melody(S, return_f0="yes"), "return_f0"),
        (lambda: melody.f0_grid(fmin=0.0), "fmin"),
        (lambda: melody.f0_grid(n_octaves=0), "n_octaves"),
        (lambda: melody.f0_grid(n_octaves=5, bins_per_octave=300), "bins_per_octave"),
        (lambda: melody.melody_audio(np.zeros(1000, np.float32)), "y"),
        (lambda: melody.melody_audio(np.zeros(4096, np.float32), max_jump=2000), "max_jump"),
        (lambda: melody.melody_audio(np.zeros(4096, np.float32), mask=True), "mask"),
        (lambda: melody.separate_wav_melody(wav, out_rate="native"), "out_rate"),
        (lambda: melody.separate_wav_melody(wav, width=-1.0), "width"),
        (lambda: melody.separate_wav_melody(wav, kernel_size=31), "kernel_size"),
        (lambda: melody.separate_wav_melody(wav, mono=2), "mono"),
    ]
    for n, (call, word) in enumerate(bad):
        with pytest.raises(ValueError, match=word):
            call()
            pytest.fail("case %d was accepted" % n)
    assert not os.path.exists(wav)
    g = melody.f0_grid()
    assert g.dtype == np.float64 and g.shape == (300,) and np.array_equal(g, M.f0_grid()) and g[0] == 55.0 and g[60] == 110.0
    assert np.array_equal(melody._weights(8, 0.8, None), M.weights()) and np.array_equal(melody._track_params(0.2, 0.02, 0.5, 12)[1], M.penalties())


def _ctype(arg):
    if "*" in arg:
        return ctypes.c_void_p
    return {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}[arg.split()[0]]


def test_the_entries_are_declared_exported_and_bound_with_the_headers_signatures(lib):
    text = open(os.path.join(REPO, "include", "glowk.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NAMES:
        m = re.search(r"\b(int|size_t) %s\(([^;]*)\);" % name, code)
        assert m, name
        res = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[m.group(1)]
        args = [_ctype(" ".join(a.split())) for a in m.group(2).split(",")]
        assert _lib.SYMBOLS[name] == (res, args), name
        assert getattr(lib, name) is not None
    bound = sorted(n for n in _lib.SYMBOLS if n.startswith("glowk_melody"))
    assert bound == sorted(NAMES) and sorted(set(re.findall(r"\bglowk_melody\w*(?=\()", code))) == bound
    version = int(re.search(r"#define GLOWK_VERSION (\d+)", text).group(1))
    assert lib.glowk_version() == version >= 553 and "Since version 553" in text


def test_the_workspaces(lib):
    for nsig, B, T in [(1, 1, 1), (2, 5, 7), (1, 300, 126), (1, 1024, 257), (3, 65, 65), (1, 300, 5626)]:
        groups = min(256, -(-B * T // 4096))
        emi, trk = -(-nsig * groups * 4 // 8) * 8, nsig * (-(-T * (B + 1) * 2 // 8) * 8)
        assert lib.glowk_melody_emission_workspace_bytes(nsig, B, T) == emi and lib.glowk_melody_track_workspace_bytes(nsig, B, T) == trk
        assert lib.glowk_melody_workspace_bytes(nsig, B, T) == nsig * B * T * 8 + -(-nsig * B * T * 4 // 8) * 8 + emi + trk
    for fn in (lib.glowk_melody_emission_workspace_bytes, lib.glowk_melody_track_workspace_bytes, lib.glowk_melody_workspace_bytes):
        for args in [(0, 4, 4), (-1, 4, 4), (65536, 1, 1), (1, 0, 4), (1, 1025, 4), (1, 4, 0), (1, 4, 32769), (64, 1024, 32768)]:
            assert fn(*args) == 0, args


def test_the_entries_refuse_bad_arguments_before_touching_a_device(lib):
    z = ctypes.c_void_p(0)
    a, b, c, d, e, f, g, h, i, j = (ctypes.c_void_p(v << 28) for v in range(1, 11))      # never dereferenced, far apart
    odd = ctypes.c_void_p((11 << 28) + 4)
    err = lambda: lib.glowk_last_error().decode()
    big = 1 << 40

    def sal(s=a, nsig=1, rows=4, frames=9, idx=b, frac=c, w=d, B=3, H=2, out=e):
        return lib.glowk_melody_salience(s, nsig, rows, frames, idx, frac, w, B, H, out, z)

    def emi(s=a, nsig=1, B=3, frames=9, out=b, m=c, work=d, nbytes=big):
        return lib.glowk_melody_emission(s, nsig, B, frames, out, m, work, nbytes, z)

    def trk(x=a, nsig=1, B=3, frames=9, pen=b, J=1, theta=0.2, nu=0.5, path=c, ticks=z, work=d, nbytes=big):
        return lib.glowk_melody_track(x, nsig, B, frames, pen, J, theta, nu, path, ticks, work, nbytes, z)

    def msk(path=a, nsig=1, frames=9, f0=b, B=3, rows=4, Hm=2, width=40.0, bin_hz=7.8125, out=c):
        return lib.glowk_melody_mask(path, nsig, frames, f0, B, rows, Hm, width, bin_hz, out, z)

    def fit(s=a, nsig=1, rows=4, frames=9, idx=b, frac=c, w=d, f0=e, B=3, H=2, pen=f, J=1, theta=0.2, nu=0.5, Hm=2, width=40.0, bin_hz=7.8125, path=g, mask=h,
            m=i, work=j, nbytes=big):
        return lib.glowk_melody_fit(s, nsig, rows, frames, idx, frac, w, f0, B, H, pen, J, theta, nu, Hm, width, bin_hz, path, mask, m, work, nbytes, z)

    shape = [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(frames=0), "frames"), (dict(frames=32769), "frames"), (dict(B=0), "B must"),
             (dict(B=1025), "B must")]
    rows = [(dict(rows=1), "rows"), (dict(rows=4097), "rows"), (dict(nsig=65535, rows=4096, frames=9), "2^31")]
    harm = [(dict(H=0), "H must"), (dict(H=33), "H must")]
    trkp = [(dict(J=-1), "J must"), (dict(J=1024), "J must"), (dict(theta=float("nan")), "finite"), (dict(nu=float("inf")), "finite")]
    mskp = [(dict(Hm=0), "Hm must"), (dict(Hm=1025), "Hm must"), (dict(width=0.0), "width"), (dict(width=float("nan")), "width"), (dict(bin_hz=0.0), "bin_hz")]
    last = [(dict(), "device memory")]
    for call, cases in ((sal, shape + rows + harm + [(dict(s=z), "null"), (dict(frac=odd), "aligned"), (dict(out=a), "overlap")] + last),
                        (emi, shape + [(dict(nsig=64, B=1024, frames=32768), "2^31"), (dict(m=z), "null"), (dict(nbytes=0), "work_bytes"), (dict(out=odd), "aligned"),
                                       (dict(out=a), "overlap"), (dict(work=b), "overlap")] + last),
                        (trk, shape + trkp + [(dict(path=z), "null"), (dict(nbytes=8), "work_bytes"), (dict(pen=odd), "aligned"), (dict(path=a), "overlap")] + last),
                        (msk, shape + rows + mskp + [(dict(f0=z), "null"), (dict(f0=odd), "aligned"), (dict(out=a), "overlap")] + last),
                        (fit, shape + rows + harm + trkp + mskp + [(dict(m=z), "null"), (dict(nbytes=64), "work_bytes"), (dict(work=odd), "aligned"),
                                                                  (dict(mask=a), "overlap"), (dict(work=e), "overlap")] + last)):
        for kw, word in cases:
            assert call(**kw) == _lib.ERR and word in err(), (call.__name__, kw, err())
        assert call(nsig=0) == _lib.OK
    host = torch.ones(4 * 9)                                                             # a host pointer is refused, not dereferenced
    assert sal(s=ctypes.c_void_p(host.data_ptr())) == _lib.ERR and "device memory" in err()
    # the position table is a host function: exact, and it refuses the grids the kernels could not use
    f0 = np.array([100.0, 150.0, 900.0])
    idx, frac = np.full((3, 4), 7, np.int32), np.full((3, 4), 7.0)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert lib.glowk_melody_positions(p(f0), 3, 4, 100.0, 6, p(idx), p(frac)) == _lib.OK
    ri, ra, live = M.positions(f0, 4, 100.0, 6)
    assert np.array_equal(idx, np.where(live, ri, -1)) and np.array_equal(frac, np.where(live, ra, 0.0))
    grid = M.f0_grid()
    idx, frac = np.empty((300, 8), np.int32), np.empty((300, 8))
    assert lib.glowk_melody_positions(p(grid), 300, 8, M.BIN_HZ, 1025, p(idx), p(frac)) == _lib.OK
    ri, ra, live = M.positions(grid, 8, M.BIN_HZ, 1025)
    assert np.array_equal(idx, np.where(live, ri, -1)) and np.array_equal(frac, np.where(live, ra, 0.0)) and not live.all() and live.any()
    keep = idx.copy()
    for args, word in [((p(f0[::-1].copy()), 3, 4, 100.0, 6), "ascending"), ((p(np.array([0.0, 1.0, 2.0])), 3, 4, 100.0, 6), "positive"),
                       ((p(f0), 3, 4, 0.0, 6), "bin_hz"), ((p(f0), 0, 4, 100.0, 6), "B must"), ((p(f0), 3, 33, 100.0, 6), "H must"), ((p(f0), 3, 4, 100.0, 1), "rows"),
                       ((z, 3, 4, 100.0, 6), "null")]:
        assert lib.glowk_melody_positions(*args, p(idx), p(frac)) == _lib.ERR and word in err(), err()
    assert np.array_equal(idx, keep)


def test_the_index_rules_under_address_and_ub_sanitizers(tmp_path):
    """glowk_melody_index.h -- the position table, the salience slab, the emission's chunks, the track's thread and back-trace rules,
    the fused call's workspace -- compiled without HIP into a stand-alone program with its own main
    (tests/melody_index_sanitize_main.cpp) and swept against straightforward loops."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "melody_index_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "melody_index_sanitize_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "MELODY_INDEX_SANITIZE_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
