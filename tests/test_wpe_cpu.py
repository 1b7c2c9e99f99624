"""WPE dereverberation without a GPU: ``wpe.py`` refuses bad arguments before the library is loaded, the fp64 restatement
(tests/wpe_ref.py) dereverberates the scenes the GPU tests use and handles the degenerate rows, the ABI entries are declared, exported
and bound, and the index rules of the kernels hold under AddressSanitizer and UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, wpe
from tests import wpe_ref as W

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ["glowk_wpe_workspace_bytes", "glowk_wpe_power", "glowk_wpe_correlations", "glowk_wpe_solve", "glowk_wpe_filter", "glowk_wpe_fit"]
MIN_GAIN_DB = 20.0


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("scene", W.AR_SCENES)
def test_the_restatement_gains_20_db_on_the_ar_scenes(scene):
    M, K, delay, T = scene
    X, S = W.ar_scene(*scene)
    Y, G, status, _ = W.wpe_rows(X, K, delay, 3)
    before, after = W.drr_db(S, X), W.drr_db(S, Y)
    print("M %d K %d delay %d T %d: %.1f dB -> %.1f dB" % (M, K, delay, T, before, after))
    assert (status == 0).all() and after > before
    if scene in W.AR_GAIN_SCENES:                                                    # the mono scene has no bar: see tests/wpe_ref.py
        assert after - before >= MIN_GAIN_DB


def test_the_restatements_degenerate_rows():
    X, _ = W.ar_scene(2, 3, 2, 40, n_rows=3)
    X[:, 1] = 0
    Y, G, status, _ = W.wpe_rows(X, 3, 2, 2)
    assert status.tolist() == [0, 1, 0] and np.array_equal(Y[:, 1], X[:, 1]) and not G[1].any() and G[0].any()
    w, pm, ok = W.inv_power(X[:, 1])
    assert not ok and pm == 0.0 and not w.any()
    # T = 4 with K = 3, delay = 2: nearly all of the past is the zero history; the loading keeps the system definite
    X4, _ = W.ar_scene(2, 3, 2, 4, n_rows=2)
    Y4, G4, s4, _ = W.wpe_rows(X4, 3, 2, 3)
    assert Y4.shape == X4.shape and np.isfinite(Y4).all() and s4.tolist() == [0, 0]
    # T < D
    X5, _ = W.ar_scene(4, 16, 1, 40, n_rows=1)
    Y5, _, s5, _ = W.wpe_rows(X5, 16, 1, 1)
    assert np.isfinite(Y5).all() and s5.tolist() == [0]
    # zero iterations
    Y0, G0, s0, _ = W.wpe_rows(X, 3, 2, 0)
    assert np.array_equal(Y0, X) and not G0.any() and not s0.any()
    # a context averages over the frames that exist
    y = np.arange(1, 6, dtype=np.float64)[None, :] + 0j
    assert np.allclose(W.power(y, 1), [(1 + 4) / 2, (1 + 4 + 9) / 3, (4 + 9 + 16) / 3, (9 + 16 + 25) / 3, (16 + 25) / 2])


def test_the_restatements_pieces_agree_with_plain_linear_algebra():
    X, _ = W.ar_scene(3, 3, 3, 64, n_rows=1)
    x = X[:, 0]
    w, _, _ = W.inv_power(x, 2)
    R, P, bR, bP = W.correlations(x, w, 3, 3)
    xt = W.stacked(x, 3, 3)
    assert np.allclose(R, (xt * w) @ xt.conj().T) and np.allclose(P, (xt * w) @ W.c128(x).conj().T) and np.array_equal(R, R.conj().T)
    assert (bR.real > 0).all() and (bP.real > 0).all()
    G, status, info = W.solve(R, P)
    assert status == 0 and np.allclose(info["loaded"] @ G, P) and np.allclose(info["L"] @ info["L"].conj().T, info["loaded"])
    assert (np.abs(info["loaded"] @ G - P) <= 4 * W.solve_residual_bound(info["L"], G)).all()
    y, mag = W.filter(x, G, 3, 3)
    assert np.allclose(y, W.c128(x) - G.conj().T @ xt) and (mag >= np.abs(y) * (1 - 1e-12) / np.sqrt(2)).all()


def _x(shape, dtype=np.complex64):
    return np.zeros(shape, dtype)


def test_bad_arguments_are_refused_before_the_library_loads(no_library):
    good = _x((2, 3, 5))
    w, G = np.ones((3, 5)), np.zeros((3, 6, 2), np.complex128)
    Rm, P = np.zeros((3, 6, 6), np.complex128), np.zeros((3, 6, 2), np.complex128)
    calls = [wpe.wpe, wpe.power_inverse, lambda x: wpe.correlations(x, w, 3, 2), lambda x: wpe.filter(x, G, 3, 2)]
    for bad in (_x((0, 3, 5)), _x((5, 3, 5)), _x((2, 0, 5)), _x((2, 4097, 2)), _x((2, 1, 32769)), _x((2, 3, 0)), _x((3, 5)), _x((2, 3, 5), np.float32),
                _x((1, 1, 2, 3, 5))):
        for call in calls:
            with pytest.raises(ValueError):
                call(bad)
    bad_kw = [dict(taps=0), dict(taps=33), dict(taps=2.0), dict(taps=True), dict(delay=0), dict(delay=17), dict(delay=1.0), dict(iterations=-1),
              dict(iterations=1001), dict(iterations=1.5), dict(psd_context=-1), dict(psd_context=9), dict(psd_context=0.5), dict(eps=0.0), dict(eps=-1e-3),
              dict(eps=2.0), dict(eps=float("nan")), dict(eps="1"), dict(loading=-1e-3), dict(loading=1.5), dict(loading=float("inf")), dict(loading=None),
              dict(return_filters=1), dict(return_status="yes")]
    for kw in bad_kw:
        with pytest.raises(ValueError):
            wpe.wpe(good, **kw)
    with pytest.raises(ValueError, match="taps"):
        wpe.wpe(_x((4, 3, 5)), taps=17)                                              # M K = 68
    with pytest.raises(ValueError, match="taps"):
        wpe.wpe(_x((3, 3, 5)), taps=22)
    for kw in (dict(psd_context=9), dict(eps=0.0), dict(eps=1.5), dict(return_max=1)):
        with pytest.raises(ValueError):
            wpe.power_inverse(good, **kw)
    for call in (lambda: wpe.correlations(good, np.ones((3, 4)), 3, 2), lambda: wpe.correlations(good, w + 0j, 3, 2), lambda: wpe.correlations(good, w, 33, 2),
                 lambda: wpe.correlations(good, w, 3, 0), lambda: wpe.filter(good, G[:, :5], 3, 2), lambda: wpe.filter(good, G.real, 3, 2),
                 lambda: wpe.filter(good, G, 3, 17), lambda: wpe.solve(Rm[:, :5], P), lambda: wpe.solve(Rm.real, P), lambda: wpe.solve(Rm, P[:, :5]),
                 lambda: wpe.solve(Rm, P.real), lambda: wpe.solve(Rm, np.zeros((3, 6, 5), np.complex128)), lambda: wpe.solve(Rm, P, loading=-1.0),
                 lambda: wpe.solve(np.zeros((3, 65, 65), np.complex128), np.zeros((3, 65, 2), np.complex128)), lambda: wpe.solve(Rm[0], P[0])):
        with pytest.raises(ValueError):
            call()
    audio = np.zeros((2, 4000), np.float32)
    for call in (lambda: wpe.wpe_audio(np.zeros((5, 4000), np.float32)), lambda: wpe.wpe_audio(np.zeros((2, 1000), np.float32)),
                 lambda: wpe.wpe_audio(audio, taps=0), lambda: wpe.wpe_audio(audio, sr=16000), lambda: wpe.wpe_audio(audio, n_fft=512, hop_length=128),
                 lambda: wpe.wpe_audio(audio, window=3), lambda: wpe.wpe_audio(np.zeros((4, 4000), np.float32), taps=17),
                 lambda: wpe.dereverb_wav("/nonexistent.wav", separate="duet"), lambda: wpe.dereverb_wav("/nonexistent.wav", taps=40),
                 lambda: wpe.dereverb_wav("/nonexistent.wav", window=3), lambda: wpe.dereverb_wav("/nonexistent.wav", n_iter=-1),
                 lambda: wpe.dereverb_wav("/nonexistent.wav", out="x.wav", separate="auxiva"), lambda: wpe.dereverb_wav("/nonexistent.wav", sr=16000),
                 lambda: wpe.dereverb_wav(np.zeros(4000, np.float32), separate="auxiva"), lambda: wpe.dereverb_wav(audio, sr=10)):
        with pytest.raises(ValueError):
            call()


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
    bound = sorted(n for n in _lib.SYMBOLS if n.startswith("glowk_wpe"))
    assert bound == sorted(NAMES) and sorted(set(re.findall(r"\bglowk_wpe\w*(?=\()", code))) == bound
    version = int(re.search(r"#define GLOWK_VERSION (\d+)", text).group(1))
    assert lib.glowk_version() == version >= 559 and "Since version 559" in text


def test_the_workspace(lib):
    for nsig, M, K, rows, frames in [(1, 1, 1, 1, 1), (3, 2, 10, 5, 203), (2, 4, 16, 3, 301), (1, 2, 10, 1025, 5626), (1, 4, 16, 1025, 5626), (1, 2, 32, 4096, 32768)]:
        D = M * K
        assert lib.glowk_wpe_workspace_bytes(nsig, M, K, rows, frames) == nsig * rows * (8 * frames + 16 * D * D + 16 * D * M)
    for args in [(0, 2, 3, 3, 7), (-1, 2, 3, 3, 7), (65536, 1, 1, 1, 1), (1, 0, 3, 3, 7), (1, 5, 3, 3, 7), (1, 2, 0, 3, 7), (1, 2, 33, 3, 7), (1, 4, 17, 3, 7),
                 (1, 2, 3, 0, 7), (1, 2, 3, 4097, 7), (1, 2, 3, 3, 0), (1, 2, 3, 3, 32769), (65535, 4, 1, 4096, 32768)]:
        assert lib.glowk_wpe_workspace_bytes(*args) == 0, args


def test_the_entries_refuse_bad_arguments_before_touching_a_device(lib):
    z = ctypes.c_void_p(0)
    a, b, c, d, e, f = (ctypes.c_void_p(v << 32) for v in range(1, 7))                     # never dereferenced, far apart
    odd = ctypes.c_void_p((11 << 32) + 4)
    odd2 = ctypes.c_void_p((12 << 32) + 2)
    err = lambda: lib.glowk_last_error().decode()
    big = 1 << 40

    def power(y=a, nsig=1, M=2, rows=3, frames=7, context=0, eps=1e-10, w=b, mx=z):
        return lib.glowk_wpe_power(y, nsig, M, rows, frames, context, eps, w, mx, z)

    def corr(x=a, w=b, nsig=1, M=2, rows=3, frames=7, K=3, delay=2, r=c, p=d):
        return lib.glowk_wpe_correlations(x, w, nsig, M, rows, frames, K, delay, r, p, z)

    def solve(r=a, p=b, nsig=1, rows=3, D=6, M=2, loading=1e-10, g=c, status=d):
        return lib.glowk_wpe_solve(r, p, nsig, rows, D, M, loading, g, status, z)

    def filt(x=a, g=b, nsig=1, M=2, rows=3, frames=7, K=3, delay=2, y=c):
        return lib.glowk_wpe_filter(x, g, nsig, M, rows, frames, K, delay, y, z)

    def fit(x=a, nsig=1, M=2, rows=3, frames=7, K=3, delay=2, iterations=2, context=0, eps=1e-10, loading=1e-10, y=b, g=c, status=d, work=e, nbytes=big):
        return lib.glowk_wpe_fit(x, nsig, M, rows, frames, K, delay, iterations, context, eps, loading, y, g, status, work, nbytes, z)

    plane = [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(M=0), "M must"), (dict(M=5), "M must"), (dict(rows=0), "rows"), (dict(rows=4097), "rows"),
             (dict(frames=0), "frames"), (dict(frames=32769), "frames"), (dict(nsig=65535, rows=4096, frames=32768), "2\\^31")]
    model = [(dict(K=0), "K must"), (dict(K=33), "K must"), (dict(M=4, K=17), "M \\* K"), (dict(delay=0), "delay"), (dict(delay=17), "delay")]
    pw = [(dict(context=-1), "context"), (dict(context=9), "context"), (dict(eps=0.0), "eps"), (dict(eps=2.0), "eps"), (dict(eps=float("nan")), "eps")]
    ld = [(dict(loading=-1.0), "loading"), (dict(loading=2.0), "loading"), (dict(loading=float("nan")), "loading")]
    last = [(dict(), "device memory")]
    for call, cases in (
            (power, plane + pw + [(dict(w=z), "null"), (dict(w=odd), "aligned"), (dict(mx=odd), "aligned"), (dict(w=a), "overlap"), (dict(mx=b), "overlap")] + last),
            (corr, plane + model + [(dict(r=z), "null"), (dict(p=odd), "aligned"), (dict(r=a), "overlap"), (dict(p=b), "overlap"), (dict(p=c), "overlap")] + last),
            (solve, [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(rows=0), "rows"), (dict(rows=4097), "rows"), (dict(M=0), "M must"), (dict(M=5), "M must"),
                     (dict(D=0), "D must"), (dict(D=65), "D must")] + ld + [(dict(g=z), "null"), (dict(g=odd), "aligned"), (dict(status=odd2), "aligned"),
                                                                           (dict(g=a), "overlap"), (dict(status=b), "overlap")] + last),
            (filt, plane + model + [(dict(y=z), "null"), (dict(g=odd), "aligned"), (dict(y=a), "overlap"), (dict(y=b), "overlap")] + last),
            (fit, plane + model + pw + ld + [(dict(iterations=-1), "iterations"), (dict(iterations=1001), "iterations"), (dict(nbytes=8), "work_bytes"),
                                             (dict(work=z), "null"), (dict(y=odd), "aligned"), (dict(status=odd2), "aligned"), (dict(y=a), "overlap"),
                                             (dict(g=b), "overlap"), (dict(work=c), "overlap")] + last)):
        for kw, word in cases:
            assert call(**kw) == _lib.ERR and re.search(word, err()), (call.__name__, kw, err())
        assert call(nsig=0) == _lib.OK
    assert fit(iterations=0) == _lib.OK
    host = torch.ones(4096, dtype=torch.float64)                                         # a host pointer is refused, not dereferenced
    assert solve(r=ctypes.c_void_p(host.data_ptr())) == _lib.ERR and "device memory" in err()


def test_the_index_rules_under_address_and_ub_sanitizers(tmp_path):
    """glowk_wpe_index.h -- the stacked past and its halo, the chunk plans and every LDS column a lane touches, the tile pairs and the
    stores of R and P, the packed triangle, the LDS bytes, the workspace and the grids -- compiled without HIP into a stand-alone program
    with its own main (tests/wpe_index_sanitize_main.cpp) and swept over the documented ranges against straightforward loops."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "wpe_index_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "wpe_index_sanitize_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "WPE_INDEX_SANITIZE_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
