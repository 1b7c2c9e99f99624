"""NMF without a GPU: the restatement of tests/nmf_ref.py on its own properties (descent for every beta, the fixed point, masks that
add up to one, the bars against plain fp32 numpy), the Python argument checks of ``audiosourcesep_amd.nmf`` (refused with ValueError
before the library is loaded), the boundary of the C entries (declared, exported, bound; every refusal before any device call), and
the plan rules the kernels share with the host under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, nmf
from tests import nmf_ref as N

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ("glowk_nmf_workspace_bytes", "glowk_nmf_fit", "glowk_nmf_divergence", "glowk_nmf_masks")
SMALL = [s for s in N.SHAPES if s[1] * s[2] <= 40000]


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def start(shape, seed=0, beta=1):
    nsig, rows, frames, K = shape
    V = N.spectra(((nsig,) if nsig != 1 else ()) + (rows, frames), seed)
    if beta == 0:
        V = np.maximum(V, np.float32(1e-3))
    rng = np.random.default_rng(seed + 1)
    s = np.sqrt(V.mean(axis=(-2, -1), keepdims=True) / K)
    return V, (rng.random(V.shape[:-2] + (rows, K)) * s).astype(np.float32) + 1e-6, (rng.random(V.shape[:-2] + (K, frames)) * s).astype(np.float32) + 1e-6


@pytest.mark.parametrize("beta", N.BETAS)
@pytest.mark.parametrize("shape", SMALL[1:], ids=lambda s: "-".join(map(str, s)))
def test_the_restatement_descends(shape, beta):
    V, W, H = start(shape, 1, beta)
    D = [N.divergence(V, W, H, beta)]
    for _ in range(30):
        W, H = N.iterate(V, W, H, beta)
        D.append(N.divergence(V, W, H, beta))
    D = np.array(D).reshape(31, -1)
    assert np.isfinite(D).all() and (D[1:] <= D[:-1] * (1 + 1e-12)).all() and (D[-1] < D[0]).all()
    W2, H2 = N.iterate(V, W, H, beta, update_w_too=False)                              # H alone: W stays, D still falls
    assert W2 is W and (np.atleast_1d(N.divergence(V, W, H2, beta)) <= D[-1] * (1 + 1e-12)).all()


@pytest.mark.parametrize("beta", N.BETAS)
def test_the_fixed_point_and_the_bars_against_fp32_numpy(beta):
    """V = W H: both updates return their input within the bar; and plain fp32 numpy stays well inside the bars the device is held to."""
    rows, frames, K = 33, 95, 5
    W, H = N.random_factors(1, rows, frames, K, 2)
    V = N.f64(W) @ N.f64(H)
    assert np.abs(N.update_h(V, W, H, beta) / H - 1).max() <= N.update_bar(K, rows)
    assert np.abs(N.update_w(V, W, H, beta) / W - 1).max() <= N.update_bar(K, frames)
    assert abs(N.divergence(V, W, H, beta)) <= 1e-20 * V.sum()
    V32, W32, H32 = start((1, rows, frames, K), 3, beta)
    L = W32 @ H32
    Q, P = (a.astype(np.float32) for a in N.qp(V32, L, beta))
    h32 = H32 * N.g((W32.T @ Q) / np.maximum(W32.T @ P, np.float32(N.FLOOR)), beta).astype(np.float32)
    ref = N.update_h(V32, W32, H32, beta)
    assert h32.dtype == np.float32 and (np.abs(h32 - ref) <= N.update_bar(K, rows) * ref).all()
    d32 = N.divergence_terms(V32, L, beta).sum()
    assert abs(d32 - N.divergence(V32, W32, H32, beta)) <= N.divergence_bar(K, N.divergence_weight(V32, W32, H32, beta))


def test_masks_add_up_to_one_and_the_defined_edges():
    W, H = N.random_factors(2, 9, 14, 7, 4)
    H = H.copy()
    H[:, :, 3] = 0.0
    for power in (1, 2):
        m = N.masks(W, H, (2, 4, 1), power)
        assert m.shape == (2, 3, 9, 14) and np.abs(m.sum(axis=1) - 1).max() <= 1e-15 and (m[:, :, :, 3] == 1.0 / 3).all()
    assert np.array_equal(N.masks(W, H, (7,)), np.ones((2, 1, 9, 14)))
    V = N.spectra((9, 14), 5)
    V[:, 2] = 0.0
    W1 = W[0].copy()
    W1[:, 4] = 0.0
    for beta in N.BETAS:
        h = N.update_h(V, W1, H[0] + 0.1, beta)
        assert not h[4].any() and not h[:, 2].any() and np.isfinite(h).all()
    X, Ws, mags = N.two_sources()
    assert X.shape == (65, 120) and [w.shape[1] for w in Ws] == [5, 4] and np.allclose(np.abs(X), mags[0] + mags[1], rtol=1e-6)
    assert np.linalg.matrix_rank(np.concatenate(Ws, axis=1)) == 9                     # no atom is a mixture of the others


def test_bad_arguments_are_refused_before_the_library_is_loaded(tmp_path, monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    V, W, H = np.ones((4, 9), np.float32), np.ones((4, 3), np.float32), np.ones((3, 9), np.float32)
    X = np.ones((4, 9), np.complex64)
    D = [np.ones((4, 2), np.float32), np.ones((4, 1), np.float32)]
    y = np.zeros(4096, np.float32)
    D16 = [np.ones((1025, 2), np.float32)]
    wav = tmp_path / "never_opened.wav"
    bad = [
        lambda: nmf.fit(np.ones(9, np.float32), W, H),                                 # shapes
        lambda: nmf.fit(V, np.ones((5, 3), np.float32), H),
        lambda: nmf.fit(V, W, np.ones((3, 8), np.float32)),
        lambda: nmf.fit(V, W, np.ones((2, 9), np.float32)),
        lambda: nmf.fit(np.ones((2, 4, 9), np.float32), W, np.ones((2, 3, 9), np.float32)),      # a shared W cannot be updated
        lambda: nmf.fit(np.ones((4097, 2), np.float32), np.ones((4097, 1), np.float32), np.ones((1, 2), np.float32)),
        lambda: nmf.fit(np.ones((1, 32769), np.float32), np.ones((1, 1), np.float32), np.ones((1, 32769), np.float32)),
        lambda: nmf.fit(V, np.ones((4, 129), np.float32), np.ones((129, 9), np.float32)),         # K > 128
        lambda: nmf.fit(-V, W, H),                                                     # negative or non-finite host entries
        lambda: nmf.fit(V, W * np.float32(np.nan), H),
        lambda: nmf.update_h(V, W, H * np.float32(np.inf)),
        lambda: nmf.fit(V.astype(np.complex64), W, H),
        lambda: nmf.fit(V, W, H, beta=3),
        lambda: nmf.fit(V, W, H, beta=1.0),
        lambda: nmf.fit(V, W, H, beta=True),
        lambda: nmf.update_w(V, W, H, beta=-1),
        lambda: nmf.divergence(V, W, H, beta=0.5),
        lambda: nmf.fit(V, W, H, n_iter=-1),
        lambda: nmf.fit(V, W, H, n_iter=100001),
        lambda: nmf.fit(V, W, H, update_w=1),
        lambda: nmf.init(V, 0),
        lambda: nmf.init(V, 129),
        lambda: nmf.init(V, 3, seed=-1),
        lambda: nmf.init(-V, 3),
        lambda: nmf.decompose(V, 200),
        lambda: nmf.decompose(V, 3, n_iter=2.5),
        lambda: nmf.learn_dictionary(V, 3, beta=4),
        lambda: nmf.masks(W, H, [2, 2]),                                               # sizes not summing to K
        lambda: nmf.masks(W, H, [3, 0]),
        lambda: nmf.masks(W, H, []),
        lambda: nmf.masks(W, H, 3),
        lambda: nmf.masks(W, H, [1, 2], power=3),
        lambda: nmf.masks(W, H, [1, 2], power=1.0),
        lambda: nmf.masks(W, H, [1, 2], X=np.ones((3, 4, 9), np.complex64)),           # C not in {1, 2}
        lambda: nmf.masks(W, H, [1, 2], X=np.ones((4, 8), np.complex64)),
        lambda: nmf.masks(np.ones((4, 17), np.float32), np.ones((17, 9), np.float32), [1] * 17),
        lambda: nmf.nmf_separate(np.ones((3, 4, 9), np.complex64), D),                 # stereo with C not in {1, 2}
        lambda: nmf.nmf_separate(np.ones(9, np.complex64), D),
        lambda: nmf.nmf_separate(X, []),
        lambda: nmf.nmf_separate(X, [np.ones((5, 2), np.float32)]),
        lambda: nmf.nmf_separate(X, [np.ones((4, 100), np.float32), np.ones((4, 29), np.float32)]),
        lambda: nmf.nmf_separate(X, [-D[0]]),
        lambda: nmf.nmf_separate(X, D, beta=5),
        lambda: nmf.nmf_separate(X, D, power=0),
        lambda: nmf.nmf_separate(X, D, n_iter=-3),
        lambda: nmf.nmf_audio(y, D),                                                   # dictionaries of the wrong height
        lambda: nmf.nmf_audio(np.zeros(100, np.float32), D16),
        lambda: nmf.nmf_audio(np.zeros((3, 4096), np.float32), D16),
        lambda: nmf.nmf_audio(y, D16, residual=1),
        lambda: nmf.separate_wav_nmf(str(wav), D16, out_rate="native"),
        lambda: nmf.separate_wav_nmf(str(wav), D16, neighborhood=3),
        lambda: nmf.separate_wav_nmf(str(wav), D16, beta=7),
        lambda: nmf.separate_wav_nmf(str(wav), D16, n_components=0),
        lambda: nmf.separate_wav_nmf(str(wav), D, n_iter=1),
        lambda: nmf.separate_wav_nmf(str(wav), [str(wav)] * 17),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % i)
    assert not wav.exists()


def test_the_entries_are_declared_exported_and_bound(lib):
    text = open(os.path.join(REPO, "include", "glowk.h")).read()
    for name in NAMES:
        assert (" %s(" % name) in text and name in _lib.SYMBOLS and getattr(lib, name) is not None, name
    version = int(re.search(r"#define GLOWK_VERSION (\d+)", text).group(1))
    assert lib.glowk_version() == version >= 550 and "Since version 550" in text


def plan(rows, frames):
    rtiles, ftiles = -(-rows // 32), -(-frames // 32)
    want = min(max(1, 256 // rtiles), max(1, ftiles // 4))
    tpc = -(-ftiles // want)
    return rtiles, -(-ftiles // tpc)


def test_the_workspace(lib):
    wb = lib.glowk_nmf_workspace_bytes
    for nsig, rows, frames, K in N.SHAPES + [(1, 1025, 5626, 128), (2, 32, 32768, 128)]:
        rtiles, nch = plan(rows, frames)
        assert wb(nsig, rows, frames, K) == nsig * max(8 * nch * rows * K, 8 * rtiles * nch), (nsig, rows, frames, K)
        assert wb(3, rows, frames, K) == 3 * wb(1, rows, frames, K)                     # the cut never depends on nsig
    assert plan(2, 4500)[1] > 2 and plan(1025, 5626) == (33, 7)
    for args in [(-1, 4, 4, 1), (65536, 4, 4, 1), (1, 0, 4, 1), (1, 4097, 4, 1), (1, 4, 0, 1), (1, 4, 32769, 1), (1, 4, 4, 0), (1, 4, 4, 129),
                 (65535, 4096, 32768, 1), (0, 4, 4, 1)]:
        assert wb(*args) == 0, args


def test_the_entries_refuse_bad_arguments_before_touching_a_device(lib):
    z, a, b, c, d = (ctypes.c_void_p(v) for v in (0, 1 << 20, 1 << 30, 1 << 31, 3 << 30))          # never dereferenced
    err = lambda: lib.glowk_last_error().decode()
    big = 1 << 40

    def fit(v=a, nsig=1, rows=4, frames=9, w=b, nw=1, h=c, K=3, beta=1, n_iter=1, update_w=1, work=d, nbytes=big):
        return lib.glowk_nmf_fit(v, nsig, rows, frames, w, nw, h, K, beta, n_iter, update_w, work, nbytes, z)

    def div(v=a, nsig=1, rows=4, frames=9, w=b, nw=1, h=c, K=3, beta=1, out=ctypes.c_void_p(1 << 32), work=d, nbytes=big):
        return lib.glowk_nmf_divergence(v, nsig, rows, frames, w, nw, h, K, beta, out, work, nbytes, z)

    def msk(w=a, nw=1, h=b, nsig=1, rows=4, frames=9, K=3, bounds=(0, 1, 3), S=2, power=1, x=z, C=1, m=c, spec=z):
        arr = (ctypes.c_int32 * len(bounds))(*bounds)
        return lib.glowk_nmf_masks(w, nw, h, nsig, rows, frames, K, arr, S, power, x, C, m, spec, z)

    for kw, word in [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(rows=0), "rows"), (dict(rows=4097), "rows"), (dict(frames=0), "frames"),
                     (dict(frames=32769), "frames"), (dict(K=0), "K must"), (dict(K=129), "K must"), (dict(nsig=65535, rows=4096, frames=32768), "2^31"),
                     (dict(beta=3), "beta"), (dict(beta=-1), "beta"), (dict(nsig=2, nw=3), "nw"), (dict(n_iter=-1), "n_iter"), (dict(n_iter=100001), "n_iter"),
                     (dict(update_w=3), "update_w"), (dict(nsig=2, nw=1), "shared"), (dict(v=z), "null"), (dict(work=z), "null"), (dict(nbytes=8), "work_bytes"),
                     (dict(work=ctypes.c_void_p((3 << 30) + 4)), "aligned"), (dict(w=a), "overlap"), (dict(work=c), "overlap"), (dict(), "device memory")]:
        assert fit(**kw) == _lib.ERR and word in err(), (kw, err())
    assert fit(n_iter=0) == _lib.OK and fit(nsig=0, nw=0) == _lib.OK and fit(nsig=0, nw=1, update_w=0, v=z, w=z, h=z, work=z) == _lib.OK   # no-ops
    assert fit(nsig=2, nw=1, update_w=0) == _lib.ERR and "device memory" in err()       # a shared W is fine when it stays
    for kw, word in [(dict(rows=0), "rows"), (dict(K=129), "K must"), (dict(beta=4), "beta"), (dict(nsig=3, nw=2), "nw"), (dict(out=z), "null"),
                     (dict(nbytes=0), "work_bytes"), (dict(out=ctypes.c_void_p((1 << 32) + 4)), "aligned"), (dict(out=a), "overlap"), (dict(), "device memory")]:
        assert div(**kw) == _lib.ERR and word in err(), (kw, err())
    assert div(nsig=0) == _lib.OK
    for kw, word in [(dict(frames=0), "frames"), (dict(K=129, bounds=(0, 1, 129)), "K must"), (dict(S=0), "sources"), (dict(S=17), "sources"), (dict(power=0), "power"),
                     (dict(power=3), "power"), (dict(bounds=(1, 2, 3)), "bounds"), (dict(bounds=(0, 1, 2)), "bounds"), (dict(bounds=(0, 3, 3)), "bounds"),
                     (dict(bounds=(0, 2, 1)), "bounds"), (dict(nsig=2, nw=3), "nw"), (dict(x=d), "together"), (dict(spec=d), "together"),
                     (dict(x=d, spec=ctypes.c_void_p(1 << 32), C=3), "channel"), (dict(m=z), "null"), (dict(m=a), "overlap"),
                     (dict(x=ctypes.c_void_p((3 << 30) + 4), spec=ctypes.c_void_p(1 << 32), C=1), "aligned"), (dict(), "device memory")]:
        assert msk(**kw) == _lib.ERR and word in err(), (kw, err())
    assert msk(nsig=0) == _lib.OK
    assert lib.glowk_nmf_masks(a, 1, b, 1, 4, 9, 3, None, 2, 1, z, 1, c, z, z) == _lib.ERR and "bounds_host" in err()
    host = torch.ones(4 * 9)                                                           # a host pointer is refused, not dereferenced
    hp = ctypes.c_void_p(host.data_ptr())
    assert fit(v=hp) == _lib.ERR and "device memory" in err() and msk(h=hp) == _lib.ERR and "device memory" in err()


def test_the_plan_rules_under_address_and_ub_sanitizers(tmp_path):
    """glowk_nmf_index.h -- the cut, the workspace size, the offsets of the partial sums and the accumulator-row permutation that
    the kernels and the entry points call -- compiled without HIP into a stand-alone program with its own main
    (tests/nmf_index_sanitize_main.cpp) and swept against straightforward loops."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "nmf_index_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "nmf_index_sanitize_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "NMF_INDEX_SANITIZE_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
