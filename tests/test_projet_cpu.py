"""PROJET without a GPU: the restatement of tests/projet_ref.py on the synthetic scenes (the separation it reaches, the pan estimates,
the monotone divergence, the stems' sum, its sensitivity to a reordering of the cells), the Python argument checks of
``audiosourcesep_amd.projet`` (ValueError before the library is loaded), the boundary of the C entries (declared, exported, bound with
the header's signatures; every refusal before any device call), and the host-side rules the kernels share with the host under
AddressSanitizer + UBSan in a stand-alone program."""
import ctypes
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, projet
from tests import audio_ref as A
from tests import projet_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ("glowk_projet_workspace_bytes", "glowk_projet_projections", "glowk_projet_gains", "glowk_projet_update_p", "glowk_projet_update_q",
         "glowk_projet_fit", "glowk_projet_divergence", "glowk_projet_separate")
# (rows, frames, pans, density, (M, L), the SDR gain over X / J every source must reach)
SCENES = [(33, 40, (0.2, 0.8, 1.35), 0.25, (12, 21), 8.0), (17, 24, (0.3, 1.2), 0.5, (12, 21), 12.0), (33, 40, (0.1, 0.5, 0.95, 1.4), 0.25, (15, 41), 5.0)]
POWERS = [(1.0, 1), (1.0, 0), (2.0, 2), (1.5, 1)]


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


@functools.lru_cache(maxsize=None)
def fitted(scene, alpha, beta):
    """(X, images, tables, P, Q, the divergence after every half step) of 100 iterations; computed once."""
    rows, frames, pans, density, (M, L), _ = SCENES[scene]
    X, imgs = R.scene(rows, frames, pans, density)
    tab = R.tables(M, L, alpha)
    trace = []
    P, Q = R.fit(X, len(pans), tab, beta, 100, trace)
    return X, imgs, tab, P, Q, np.array(trace)


@pytest.mark.parametrize("alpha,beta", POWERS)
@pytest.mark.parametrize("scene", range(len(SCENES)))
def test_the_scenes_are_separated_in_pan_order(scene, alpha, beta):
    X, imgs, tab, P, Q, _ = fitted(scene, alpha, beta)
    pans, floor = SCENES[scene][2], SCENES[scene][5]
    Y = R.separate(X, P, R.gains(Q, tab["K"]), tab)
    gain = R.sdr_gains(Y, X, imgs)                                                       # index order against ascending pans: no permutation
    step = tab["theta"][1] - tab["theta"][0]
    off = np.abs(R.pan_estimates(Q, tab["theta"]) - np.array(pans)) / step
    print("scene %d alpha %g beta %d: SDR gains %s dB, pans off by %s grid steps" % (scene, alpha, beta, np.round(gain, 2), np.round(off, 2)))
    assert (gain >= floor).all()
    assert (off <= 3.0).all()
    # the package's own tables, start and pan estimates are the restatement's
    mine = projet.tables(*SCENES[scene][4], alpha)
    assert np.array_equal(mine["U"], tab["U"]) and np.array_equal(mine["K"], tab["K"]) and np.array_equal(mine["theta"], tab["theta"])
    assert np.abs(mine["Up"] - tab["Up"]).max() <= 1e-14 and np.abs(mine["Up"] @ mine["U"] - np.eye(2)).max() <= 1e-14
    assert np.array_equal(projet.init_q(len(pans), mine["theta"]), R.init(X, len(pans), tab)[1])
    assert np.array_equal(projet.pan_estimates(Q).numpy(), R.pan_estimates(Q, tab["theta"]))


@pytest.mark.parametrize("beta", [0, 1, 2])
@pytest.mark.parametrize("scene", range(len(SCENES)))
def test_no_half_step_raises_the_divergence(scene, beta):
    trace = fitted(scene, 1.0, beta)[5]
    assert len(trace) == 201 and np.isfinite(trace).all()
    rise = (trace[1:] - trace[:-1]) / np.abs(trace[:-1])
    print("scene %d beta %d: D %.4g -> %.4g, largest relative change of a half step %.2e" % (scene, beta, trace[0], trace[-1], rise.max()))
    assert rise.max() <= 1e-12


@pytest.mark.parametrize("alpha,beta", POWERS)
def test_the_stems_add_up_to_the_mixture(alpha, beta):
    X, imgs, tab, P, Q, _ = fitted(0, alpha, beta)
    X = X.copy()
    X[:, :2, :3] = 0                                                                     # cells that are exactly 0 in both channels
    X[0, 5, :4] = 0                                                                      # and in one
    Y = R.separate(X, P, R.gains(Q, tab["K"]), tab, dtype=None)
    gap = np.abs(Y.sum(axis=0) - X).max() / np.abs(X).max()
    print("alpha %g beta %d: stems' sum off by %.2e max |X|" % (alpha, beta, gap))
    assert gap <= 1e-14
    assert not Y[:, :, :2, :3].any()
    Pz = P.copy()
    Pz[:, 7:9] = 0                                                                       # a model below FLOOR: the cell is shared evenly
    Yz = R.separate(X, Pz, R.gains(Q, tab["K"]), tab, dtype=None)
    assert np.abs(Yz.sum(axis=0) - X).max() <= 1e-14 * np.abs(X).max()
    assert np.abs(Yz[:, :, 7:9] - X[None, :, 7:9].astype(np.complex128) / Pz.shape[0]).max() <= 1e-14 * np.abs(X).max()


@pytest.mark.parametrize("alpha,beta", POWERS)
@pytest.mark.parametrize("scene", [0, 1])
def test_a_reordering_of_the_cells_moves_fifty_iterations_by_rounding_only(scene, alpha, beta):
    """The figure the GPU chain test scales: the restatement on the scene and on the scene with rows and frames reversed."""
    rows, frames, pans, density, (M, L), _ = SCENES[scene]
    X, _ = R.scene(rows, frames, pans, density)
    tab = R.tables(M, L, alpha)
    P, Q = R.fit(X, len(pans), tab, beta, 50)
    Pb, Qb = R.fit(X[:, ::-1, ::-1], len(pans), tab, beta, 50)
    dp, dq = np.abs(P - Pb[:, ::-1, ::-1]).max() / P.max(), np.abs(Q - Qb).max() / Q.max()
    print("scene %d alpha %g beta %d: dP %.1e max P, dQ %.1e max Q" % (scene, alpha, beta, dp, dq))
    assert dp <= 1e-12 and dq <= 1e-12


def test_the_audio_tests_tones_are_separated_by_the_restatement():
    """The three panned tones of tests/test_gpu_projet.py, through the restatement and the reference STFT: every source gains 8 dB over
    y / 3 in the time domain and comes out in pan order (the prototype-level condition the GPU audio test relies on)."""
    from tests.test_gpu_projet import TONES, tones
    y, imgs = tones()
    n = y.shape[1]
    X = np.stack([A.stft(np.pad(c, (0, -n % 512))) for c in y]).astype(np.complex64)
    tab = R.tables(15, 41, 1.0)
    Y, P, Q = R.projet(X, 3, tab, 1, 50)
    off = np.abs(R.pan_estimates(Q, tab["theta"]) - np.array([th for _, th in TONES])) / (tab["theta"][1] - tab["theta"][0])
    assert (off <= 3.0).all(), off
    for j in range(3):
        s = np.stack([A.istft(Y[j, ch].astype(np.complex128))[:n] for ch in range(2)])
        base = 10 * math.log10((imgs[j] ** 2).sum() / ((imgs[j] - y / 3) ** 2).sum())
        got = 10 * math.log10((imgs[j] ** 2).sum() / ((imgs[j] - s) ** 2).sum())
        print("tone %d: %.1f dB over y / 3" % (j, got - base))
        assert got - base >= 8.0


def test_every_bad_argument_is_a_value_error_before_the_library_is_loaded():
    X = np.ones((2, 3, 4), np.complex64)
    tab = projet.tables(4, 5)
    P, Q = np.ones((2, 3, 4)), np.ones((5, 2))
    one_dir = dict(U=np.array([[1.0, 2.0], [2.0, 4.0]]), K=np.ones((2, 5)), alpha=1.0)
    bad = [
        (lambda: projet.tables(1), "num_projections"), (lambda: projet.tables(33), "num_projections"), (lambda: projet.tables(4.0), "num_projections"),
        (lambda: projet.tables(4, 0), "num_pans"), (lambda: projet.tables(4, 129), "num_pans"), (lambda: projet.tables(4, 5, 0.5), "alpha"),
        (lambda: projet.tables(4, 5, 2.5), "alpha"), (lambda: projet.tables(4, 5, float("nan")), "alpha"), (lambda: projet.tables(4, 5, "1"), "alpha"),
        (lambda: projet.projections(X, one_dir), "not invertible"), (lambda: projet.projections(X, dict(U=np.ones((4, 3)), K=np.ones((4, 5)), alpha=1.0)), "U"),
        (lambda: projet.projections(X, dict(U=tab["U"], K=np.ones((3, 5)), alpha=1.0)), "K"), (lambda: projet.projections(X, dict(U=tab["U"], K=-tab["K"], alpha=1.0)), "K"),
        (lambda: projet.projections(X, [1]), "tables"), (lambda: projet.projections(np.ones((2, 3, 4)), tab), "complex"),
        (lambda: projet.projections(np.ones((3, 3, 4), np.complex64), tab), "X"), (lambda: projet.projections(np.ones((2, 4097, 1), np.complex64), tab), "X"),
        (lambda: projet.init(X, 0, tab), "num_sources"), (lambda: projet.init(X, 9, tab), "num_sources"), (lambda: projet.init(X, True, tab), "num_sources"),
        (lambda: projet.gains(np.ones((4, 2)), tab), "Q"), (lambda: projet.gains(np.ones((5, 9)), tab), "Q"),
        (lambda: projet.update_p(X, np.ones((9, 3, 4)), np.ones((5, 9)), tab), "P"), (lambda: projet.update_p(X, np.ones((2, 3, 5)), Q, tab), "P"),
        (lambda: projet.update_p(X, P, np.ones((4, 2)), tab), "Q"), (lambda: projet.update_p(X, P, Q, tab, beta=3), "beta"),
        (lambda: projet.update_q(X, P, Q, tab, beta=1.0), "beta"), (lambda: projet.update_q(X, P, Q, tab, beta=True), "beta"),
        (lambda: projet.fit(X, P, Q, tab, n_iter=-1), "n_iter"), (lambda: projet.fit(X, P, Q, tab, n_iter=100001), "n_iter"),
        (lambda: projet.fit(X, P, Q, tab, beta=-1), "beta"), (lambda: projet.divergence(X, P, Q, tab, beta=4), "beta"),
        (lambda: projet.separate(X, P + 0j, Q, tab), "P"), (lambda: projet.pan_estimates(np.ones((129, 2))), "Q"), (lambda: projet.pan_estimates(np.ones((5, 2)), np.ones(4)), "theta"),
        (lambda: projet.projet(X, 0), "num_sources"), (lambda: projet.projet(X, 2, num_projections=1), "num_projections"), (lambda: projet.projet(X, 2, num_pans=0), "num_pans"),
        (lambda: projet.projet(X, 2, alpha=3), "alpha"), (lambda: projet.projet(X, 2, beta=5), "beta"), (lambda: projet.projet(X, 2, n_iter=1.5), "n_iter"),
        (lambda: projet.projet(X, 2, return_model=1), "return_model"), (lambda: projet.projet(np.ones((2, 3, 4)), 2), "complex"),
        (lambda: projet.projet_audio(np.zeros((2, 4000), np.float32), 0), "num_sources"), (lambda: projet.projet_audio(np.zeros((2, 4000), np.float32), 2, residual=2), "residual"),
        (lambda: projet.projet_audio(np.zeros((3, 4000), np.float32), 2), "two channels"), (lambda: projet.projet_audio(np.zeros(4000, np.float32), 2), "two channels"),
        (lambda: projet.separate_wav_projet("/nonexistent.wav", 2, out_rate="native"), "out_rate"),
        (lambda: projet.separate_wav_projet("/nonexistent.wav", 2, kernel_size=5), "kernel_size"), (lambda: projet.separate_wav_projet("/nonexistent.wav", 2, alpha=9), "alpha"),
        (lambda: projet.separate_wav_projet("/nonexistent.wav", 9), "num_sources"),
    ]
    for n, (call, word) in enumerate(bad):
        with pytest.raises(ValueError, match=word):
            call()
            pytest.fail("case %d was accepted" % n)
    # ties of pan_estimates go to the lowest l; the grid defaults to the pans of tables()
    Qt = np.array([[1.0, 0.0], [1.0, 2.0], [0.5, 2.0]])
    assert np.array_equal(projet.pan_estimates(Qt).numpy(), np.array([0.0, math.pi / 4]))
    assert projet.pan_estimates(np.ones((1, 3))).numpy().tolist() == [math.pi / 4] * 3


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
    bound = sorted(n for n in _lib.SYMBOLS if n.startswith("glowk_projet"))
    assert bound == sorted(NAMES) and sorted(set(re.findall(r"\bglowk_projet\w*(?=\()", code))) == bound
    version = int(re.search(r"#define GLOWK_VERSION (\d+)", text).group(1))
    assert lib.glowk_version() == version >= 555 and "Since version 555" in text


def _groups(cells):
    g = max(1, min(1024, -(-cells // 256)))
    per = -(-(-(-cells // g)) // 256) * 256
    return -(-cells // per)


def test_the_workspace(lib):
    for nsig, M, J, rows, frames in [(1, 2, 1, 1, 1), (2, 12, 3, 3, 5), (3, 15, 4, 17, 24), (1, 32, 8, 129, 257), (1, 15, 4, 1025, 5626), (1, 17, 5, 4096, 32768)]:
        assert lib.glowk_projet_workspace_bytes(nsig, M, J, rows, frames) == 16 * nsig * _groups(rows * frames) * M * J
    assert _groups(1025 * 5626) == 1024 and _groups(257) == 2 and _groups(256) == 1
    for args in [(0, 4, 2, 3, 7), (-1, 4, 2, 3, 7), (65536, 4, 2, 1, 1), (1, 1, 2, 3, 7), (1, 33, 2, 3, 7), (1, 4, 0, 3, 7), (1, 4, 9, 3, 7), (1, 4, 2, 0, 7), (1, 4, 2, 4097, 7),
                 (1, 4, 2, 3, 0), (1, 4, 2, 3, 32769), (2, 4, 8, 4096, 32768)]:
        assert lib.glowk_projet_workspace_bytes(*args) == 0, args


def test_the_entries_refuse_bad_arguments_before_touching_a_device(lib):
    z = ctypes.c_void_p(0)
    a, b, c, d, e, f, g, h = (ctypes.c_void_p(v << 32) for v in range(1, 9))              # never dereferenced, far apart
    odd = ctypes.c_void_p((11 << 32) + 4)
    err = lambda: lib.glowk_last_error().decode()
    big = 1 << 40

    def proj(x=a, nsig=1, rows=3, frames=7, u=b, M=4, alpha=1.0, v=c):
        return lib.glowk_projet_projections(x, nsig, rows, frames, u, M, alpha, v, z)

    def gains(k=a, q=b, nsig=1, M=4, L=5, J=2, out=c):
        return lib.glowk_projet_gains(k, q, nsig, M, L, J, out, z)

    def up(x=a, nsig=1, rows=3, frames=7, u=b, gg=c, M=4, J=2, alpha=1.0, beta=1, p=d):
        return lib.glowk_projet_update_p(x, nsig, rows, frames, u, gg, M, J, alpha, beta, p, z)

    def uq(x=a, p=b, nsig=1, rows=3, frames=7, u=c, k=d, M=4, L=5, J=2, alpha=1.0, beta=1, q=e, gg=f, work=g, nbytes=big):
        return lib.glowk_projet_update_q(x, p, nsig, rows, frames, u, k, M, L, J, alpha, beta, q, gg, work, nbytes, z)

    def fit(x=a, nsig=1, rows=3, frames=7, u=b, k=c, M=4, L=5, J=2, alpha=1.0, beta=1, n_iter=2, p=d, q=e, gg=f, work=g, nbytes=big):
        return lib.glowk_projet_fit(x, nsig, rows, frames, u, k, M, L, J, alpha, beta, n_iter, p, q, gg, work, nbytes, z)

    def div(x=a, p=b, nsig=1, rows=3, frames=7, u=c, gg=d, M=4, J=2, alpha=1.0, beta=1, out=e, work=f, nbytes=big):
        return lib.glowk_projet_divergence(x, p, nsig, rows, frames, u, gg, M, J, alpha, beta, out, work, nbytes, z)

    def sep(x=a, p=b, nsig=1, rows=3, frames=7, u=c, upi=d, gg=e, M=4, J=2, y=f):
        return lib.glowk_projet_separate(x, p, nsig, rows, frames, u, upi, gg, M, J, y, z)

    plane = [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(rows=0), "rows"), (dict(rows=4097), "rows"), (dict(frames=0), "frames"),
             (dict(frames=32769), "frames"), (dict(nsig=65535, rows=4096, frames=32768), "2^31")]
    nm = [(dict(M=1), "M must"), (dict(M=33), "M must")]
    nj = [(dict(J=0), "J must"), (dict(J=9), "J must")]
    nl = [(dict(L=0), "L must"), (dict(L=129), "L must")]
    al = [(dict(alpha=0.5), "alpha"), (dict(alpha=2.5), "alpha"), (dict(alpha=float("nan")), "alpha")]
    be = [(dict(beta=-1), "beta"), (dict(beta=3), "beta")]
    wk = [(dict(nbytes=8), "work_bytes"), (dict(work=z), "null")]
    last = [(dict(), "device memory")]
    for call, cases in (
            (proj, plane + nm + al + [(dict(v=z), "null"), (dict(u=odd), "aligned"), (dict(v=a), "overlap")] + last),
            (gains, [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig")] + nm + nl + nj + [(dict(q=z), "null"), (dict(out=odd), "aligned"), (dict(out=b), "overlap")] + last),
            (up, plane + nm + nj + al + be + [(dict(p=z), "null"), (dict(p=odd), "aligned"), (dict(p=a), "overlap"), (dict(gg=d), "overlap")] + last),
            (uq, plane + nm + nl + nj + al + be + wk + [(dict(q=z), "null"), (dict(gg=odd), "aligned"), (dict(q=b), "overlap"), (dict(work=e), "overlap"),
                                                        (dict(gg=d), "overlap")] + last),
            (fit, plane + nm + nl + nj + al + be + wk + [(dict(n_iter=-1), "n_iter"), (dict(n_iter=100001), "n_iter"), (dict(p=z), "null"), (dict(q=odd), "aligned"),
                                                         (dict(p=a), "overlap"), (dict(gg=e), "overlap"), (dict(work=d), "overlap")] + last),
            (div, plane + nm + nj + al + be + wk + [(dict(out=z), "null"), (dict(out=odd), "aligned"), (dict(out=b), "overlap"), (dict(work=a), "overlap")] + last),
            (sep, plane + nm + nj + [(dict(upi=z), "null"), (dict(y=odd), "aligned"), (dict(y=b), "overlap")] + last)):
        for kw, word in cases:
            assert call(**kw) == _lib.ERR and word in err(), (call.__name__, kw, err())
        assert call(nsig=0) == _lib.OK
    host = torch.ones(4096, dtype=torch.float64)                                         # a host pointer is refused, not dereferenced
    assert gains(k=ctypes.c_void_p(host.data_ptr())) == _lib.ERR and "device memory" in err()


def test_the_index_rules_under_address_and_ub_sanitizers(tmp_path):
    """glowk_projet_index.h -- the tiles of M, the workgroups and chunks of a signal, the chain behind an outer sum, the workspace --
    compiled without HIP into a stand-alone program with its own main (tests/projet_index_sanitize_main.cpp) and swept against
    straightforward loops.  The same program prints chain() for the GPU tests' shapes, which restate it in Python."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "projet_index_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "projet_index_sanitize_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "PROJET_INDEX_SANITIZE_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    from tests.test_gpu_projet import BIG_SHAPES, EDGE_SHAPES, ISSUE_SHAPES, chain
    shapes = [s[1:] for s in ISSUE_SHAPES + EDGE_SHAPES + BIG_SHAPES] + [(1025, 5626), (4096, 32768)]
    r = subprocess.run([exe, "chain"] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and [int(v) for v in r.stdout.split()] == [chain(*s) for s in shapes]
