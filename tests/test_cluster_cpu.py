"""Clustering without a GPU: the restatement of tests/cluster_ref.py (its fp64 statistics inside the a-priori bound of the longdouble
ones on every GPU-test input, a likelihood that never falls, the scenes' separation, agreement with scikit-learn), the Python argument
checks of ``audiosourcesep_amd.cluster`` (ValueError before the library is loaded), the boundary of the C entries, and the host-side
rules the kernels share with the host under AddressSanitizer + UBSan in a stand-alone program."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, cluster
from tests import cluster_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAMES = ("glowk_cluster_work_bytes", "glowk_cluster_init", "glowk_cluster_stats", "glowk_cluster_update", "glowk_cluster_fit",
         "glowk_cluster_posteriors", "glowk_cluster_spatial_features")
SPATIAL_SCENES = [(33, 47, (0.3, 1.2), 0.15), (65, 120, (0.2, 0.8, 1.4), 0.1)]


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


@pytest.mark.parametrize("shape", R.GPU_SHAPES)
def test_the_fp64_restatement_lies_inside_the_bound_of_the_longdouble_one(shape):
    """The bound is checked against the reference, not against the code under test; also the GPU label test's premise: no cell of the
    restatement has its two largest posteriors within the bound of each other."""
    N, D, J, rows, frames = shape
    F, w = R.inputs(shape)
    for n in range(N):
        st = R.random_state(F[n], w[n], J)
        s64, sld, b = R.stats(F[n], w[n], st), R.stats_longdouble(F[n], w[n], st), R.stats_bound(F[n], w[n], st)
        frac = np.abs((s64 - sld).astype(np.float64)) / b
        print("shape %s signal %d: worst fraction of the bound %.3g" % (shape, n, frac.max()))
        assert (b > 0).all() and (frac <= 1.0).all()
        assert R.label_ties(F[n], st) == 0


@pytest.mark.parametrize("shape", R.GPU_SHAPES[:4])
def test_the_likelihood_never_falls_on_random_mixtures(shape):
    N, D, J, rows, frames = shape
    F, w = R.inputs(shape)
    for n in range(N):
        ll = R.fit(F[n], w[n], J, n_iter=30, tol=0.0)["log_likelihood"]
        assert np.isfinite(ll).all() and (np.diff(ll) >= -1e-12 * np.abs(ll[1:])).all(), ll


@functools.lru_cache(maxsize=None)
def spatial_fitted(i):
    rows, frames, pans, density = SPATIAL_SCENES[i]
    X, imgs = R.spatial_scene(rows, frames, pans, density)
    Y, st = R.spatial_separate(X, len(pans), n_iter=30)
    return X, imgs, Y, st


@pytest.mark.parametrize("i,floor", [(0, 7.9), (1, 2.9)])
def test_the_spatial_scenes_are_separated_in_pan_order(i, floor):
    """Measured with the principal-axis start, p = 1, 30 iterations: see the print."""
    X, imgs, Y, st = spatial_fitted(i)
    pans = np.array(SPATIAL_SCENES[i][2])
    gain = R.sdr_gains(Y, X, imgs)
    means = st["means"][:, 0] + np.pi / 4
    print("scene %d: SDR gains %s dB, means %s rad" % (i, np.round(gain, 2), np.round(means, 3)))
    assert (np.diff(means) > 0).all() and (np.abs(means - pans) < 0.1).all()
    assert (gain >= floor).all()
    ll = st["log_likelihood"]
    assert (np.diff(ll) >= -1e-12 * np.abs(ll[1:])).all()


def test_the_ensemble_is_above_the_median_primitive_on_the_melody_scene():
    """The restatements of melody, hpss and repet_sim as primitives, J = 2, magnitude weights, 30 iterations; gains over the mixture."""
    from tests import hpss_ref, melody_ref, repet_ref
    X_lead, X_acc, X_mix = R.melody_scene()
    mag = np.abs(X_mix).astype(np.float32)
    masks = [melody_ref.melody(mag)[0], hpss_ref.hpss(mag, mask=True)[1], repet_ref.repet_sim(mag, mask=True)[1]]
    base = [R.sdr(X_mix, X_acc), R.sdr(X_mix, X_lead)]
    own = np.array([[R.sdr((1 - m) * X_mix, X_acc) - base[0], R.sdr(m * X_mix, X_lead) - base[1]] for m in masks])
    r, st = R.ensemble_separate(masks, mag, 2, n_iter=30)
    gain = np.array([R.sdr(r[0] * X_mix, X_acc) - base[0], R.sdr(r[1] * X_mix, X_lead) - base[1]])
    print("ensemble: SDR gains (accompaniment, lead) %s dB, the primitives' %s" % (np.round(gain, 2), np.round(own, 2).tolist()))
    assert (gain >= np.median(own, axis=0)).all() and (gain >= [3.0, 1.4]).all()
    ll = st["log_likelihood"]
    assert (np.diff(ll) >= -1e-12 * np.abs(ll[1:])).all() and st["status"] == 0


def test_the_restatement_matches_scikit_learn():
    mixture = pytest.importorskip("sklearn.mixture")
    for shape in [(1, 2, 3, 17, 45), (1, 5, 2, 17, 45)]:
        N, D, J, rows, frames = shape
        F, _ = R.inputs(shape)
        w = np.ones((rows, frames), np.float32)
        st = R.random_state(F[0], w, J)
        n = 7
        ours = R.fit(F[0], w, J, n_iter=n, tol=0.0, means=st["means"], covariances=st["covariances"], weights=st["weights"])
        gm = mixture.GaussianMixture(J, covariance_type="full", tol=0.0, max_iter=n, reg_covar=1e-6, means_init=st["means"], weights_init=st["weights"],
                                     precisions_init=np.linalg.inv(st["covariances"]))
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            gm.fit(F[0].reshape(D, -1).T.astype(np.float64))
        assert np.abs(gm.means_ - ours["means"]).max() < 1e-9
        assert np.abs(gm.weights_ - ours["weights"]).max() < 1e-9 and np.abs(gm.covariances_ - ours["covariances"]).max() < 1e-9


def test_bad_arguments_raise_before_the_library_is_loaded(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(torch.cuda, "current_device", boom)
    F, w = np.zeros((2, 3, 4), np.float32), np.ones((3, 4), np.float32)
    X = np.zeros((2, 3, 4), np.complex64)
    st = dict(weights=np.ones(2) / 2, means=np.zeros((2, 2)), covariances=np.tile(np.eye(2), (2, 1, 1)), origin=np.zeros(2), total=np.ones(()))
    bad = [
        lambda: cluster.init(F, w, 0), lambda: cluster.init(F, w, 9), lambda: cluster.init(F, w, 2.0), lambda: cluster.init(F, w, 2, reg_covar=0.0),
        lambda: cluster.init(F, w, 2, reg_covar=float("nan")), lambda: cluster.init(F, None, 2), lambda: cluster.init(F, w[:2], 2),
        lambda: cluster.init(np.zeros((9, 3, 4), np.float32), w, 2), lambda: cluster.init(F.astype(np.complex64), w, 2), lambda: cluster.init(F[0], w, 2),
        lambda: cluster.stats(F, w, dict(st, means=np.zeros((2, 3)))), lambda: cluster.stats(F, w, "state"), lambda: cluster.stats(F, w, {k: st[k] for k in ("weights", "means")}),
        lambda: cluster.update(np.zeros(5), st), lambda: cluster.update(np.zeros(13), st, reg_covar=-1.0), lambda: cluster.update(np.zeros(13), dict(st, origin=np.zeros(()))),
        lambda: cluster.fit(F, w, 2, n_iter=-1), lambda: cluster.fit(F, w, 2, n_iter=100001), lambda: cluster.fit(F, w, 2, tol=-1.0), lambda: cluster.fit(F, w, 2, tol="x"),
        lambda: cluster.fit(F, w, 2, means=np.zeros((3, 2))), lambda: cluster.fit(F, w, 2, covariances=np.zeros((2, 2, 2))), lambda: cluster.fit(F, w, 2, weights=np.ones(2)),
        lambda: cluster.posteriors(F, st, X=np.zeros((3, 4), np.float32)), lambda: cluster.posteriors(F, st, X=np.zeros((3, 3, 4), np.complex64)),
        lambda: cluster.posteriors(F, dict(st, weights=np.ones(9) / 9)), lambda: cluster.labels(F[0], st),
        lambda: cluster.mask_features(), lambda: cluster.mask_features(w, w[:2]), lambda: cluster.mask_features(*([w] * 9)), lambda: cluster.mask_features(X[0]),
        lambda: cluster.spatial_features(X[:1]), lambda: cluster.spatial_features(X.real), lambda: cluster.spatial_features(X, delay=1), lambda: cluster.spatial_features(X, max_delay=0.0),
        lambda: cluster.spatial_features(X, p=0.0), lambda: cluster.spatial(X, 0), lambda: cluster.spatial(X, 2, mask=1), lambda: cluster.spatial(X, 2, iterations=3),
        lambda: cluster.spatial(X, 2, n_iter=-1), lambda: cluster.ensemble(w, primitives=()), lambda: cluster.ensemble(w, primitives=("nmf",)),
        lambda: cluster.ensemble(w, primitives=(("hpss", dict(mask=True)),)), lambda: cluster.ensemble(w, primitives=(3,)), lambda: cluster.ensemble(w, power=0.0),
        lambda: cluster.ensemble(w, num_sources=9), lambda: cluster.ensemble(w, primitives=(np.ones((2, 2), np.float32),)), lambda: cluster.ensemble(w, tolerance=1.0),
        lambda: cluster.ensemble_audio(np.zeros(100, np.float32)), lambda: cluster.ensemble_audio(np.zeros(4000, np.float32), residual=2),
        lambda: cluster.spatial_audio(np.zeros(4000, np.float32), 2), lambda: cluster.spatial_audio(np.zeros((2, 4000), np.float32), 0),
        lambda: cluster.separate_wav_ensemble("nowhere.wav", out_rate="native"), lambda: cluster.separate_wav_ensemble("nowhere.wav", kernel_size=3),
        lambda: cluster.separate_wav_spatial("nowhere.wav", 2, out_rate=3.5), lambda: cluster.separate_wav_spatial("nowhere.wav", 2, mask=True),
        lambda: cluster.separate_wav_spatial("nowhere.wav", 9),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d raised nothing" % i)
    assert np.allclose(cluster.quantiles(2), [-0.6744897501960817, 0.6744897501960817]) and cluster.stat_size(2, 2) == 13
    assert np.array_equal(cluster.quantiles(5), R.quantiles(5))


def _ctype(decl):
    if "*" in decl:
        return ctypes.c_void_p
    base = decl.rsplit(" ", 1)[0]
    return {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}[base]


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
    bound = sorted(n for n in _lib.SYMBOLS if n.startswith("glowk_cluster"))
    assert bound == sorted(NAMES) and sorted(set(re.findall(r"\bglowk_cluster\w*(?=\()", code))) == bound
    version = int(re.search(r"#define GLOWK_VERSION (\d+)", text).group(1))
    assert lib.glowk_version() == version >= 556 and "Since version 556" in text


def test_the_workspace(lib):
    for nsig, D, J, rows, frames in [(1, 1, 1, 1, 1), (3, 5, 2, 17, 45), (1, 8, 8, 33, 64), (1, 2, 3, 513, 515), (1, 4, 2, 1025, 5626)]:
        P1 = 1 + D + D * (D + 1) // 2
        want = 8 * (nsig * R.groups(rows * frames) * (J * P1 + 1) + nsig * (J * P1 + 1) + nsig * (D + J * (1 + D + D * D)) + 2 * nsig)
        assert lib.glowk_cluster_work_bytes(nsig, D, J, rows, frames) == want
    assert R.groups(513 * 515) == 517 and R.chunk_cells(513 * 515) == 512 and R.groups(1025 * 5626) == 1024
    for args in [(0, 1, 1, 3, 7), (-1, 1, 1, 3, 7), (65536, 1, 1, 1, 1), (1, 0, 1, 3, 7), (1, 9, 1, 3, 7), (1, 1, 0, 3, 7), (1, 1, 9, 3, 7), (1, 1, 1, 0, 7),
                 (1, 1, 1, 4097, 7), (1, 1, 1, 3, 0), (1, 1, 1, 3, 32769), (3, 8, 2, 4096, 32768)]:
        assert lib.glowk_cluster_work_bytes(*args) == 0, args


def test_the_entries_refuse_bad_arguments_before_touching_a_device(lib):
    z = ctypes.c_void_p(0)
    p = [ctypes.c_void_p(v << 32) for v in range(1, 16)]                                  # never dereferenced, far apart
    odd8, odd4 = ctypes.c_void_p((31 << 32) + 4), ctypes.c_void_p((31 << 32) + 2)
    err = lambda: lib.glowk_last_error().decode()
    big = 1 << 40

    def init(f=p[0], w=p[1], nsig=1, D=2, J=2, rows=3, frames=7, zq=p[2], reg=1e-6, pi=p[3], mu=p[4], sg=p[5], o=p[6], tot=p[7], status=p[8], work=p[9], nbytes=big):
        return lib.glowk_cluster_init(f, w, nsig, D, J, rows, frames, zq, reg, pi, mu, sg, o, tot, status, work, nbytes, z)

    def stats(f=p[0], w=p[1], nsig=1, D=2, J=2, rows=3, frames=7, pi=p[3], mu=p[4], sg=p[5], o=p[6], tot=p[7], out=p[10], status=p[8], work=p[9], nbytes=big):
        return lib.glowk_cluster_stats(f, w, nsig, D, J, rows, frames, pi, mu, sg, o, tot, out, status, work, nbytes, z)

    def update(s=p[10], nsig=1, D=2, J=2, reg=1e-6, pi=p[3], mu=p[4], sg=p[5], o=p[6], tot=p[7], ll=p[11], status=p[8], work=p[9], nbytes=big):
        return lib.glowk_cluster_update(s, nsig, D, J, reg, pi, mu, sg, o, tot, ll, status, work, nbytes, z)

    def fit(f=p[0], w=p[1], nsig=1, D=2, J=2, rows=3, frames=7, zq=p[2], reg=1e-6, n_iter=2, tol=0.0, pi=p[3], mu=p[4], sg=p[5], o=p[6], tot=p[7], ll=p[11],
            iters=p[12], status=p[8], work=p[9], nbytes=big):
        return lib.glowk_cluster_fit(f, w, nsig, D, J, rows, frames, zq, reg, n_iter, tol, pi, mu, sg, o, tot, ll, iters, status, work, nbytes, z)

    def post(f=p[0], nsig=1, D=2, J=2, rows=3, frames=7, pi=p[3], mu=p[4], sg=p[5], o=p[6], tot=p[7], x=p[13], C=2, mask=p[14], y=p[12], status=p[8], work=p[9],
             nbytes=big):
        return lib.glowk_cluster_posteriors(f, nsig, D, J, rows, frames, pi, mu, sg, o, tot, x, C, mask, y, status, work, nbytes, z)

    def spat(x=p[0], nsig=1, rows=3, frames=7, delay=0, max_delay=3.0, pw=1.0, feat=p[1], w=p[2]):
        return lib.glowk_cluster_spatial_features(x, nsig, rows, frames, delay, max_delay, pw, feat, w, z)

    plane = [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(rows=0), "rows"), (dict(rows=4097), "rows"), (dict(frames=0), "frames"),
             (dict(frames=32769), "frames"), (dict(nsig=65535, rows=4096, frames=32768), "2^31")]
    dj = [(dict(D=0), "D must"), (dict(D=9), "D must"), (dict(J=0), "J must"), (dict(J=9), "J must")]
    rg = [(dict(reg=0.0), "reg_covar"), (dict(reg=float("nan")), "reg_covar"), (dict(reg=float("inf")), "reg_covar")]
    wk = [(dict(nbytes=8), "work_bytes"), (dict(work=z), "null")]
    last = [(dict(), "device memory")]
    for call, cases in (
            (init, plane + dj + rg + wk + [(dict(zq=z), "null"), (dict(pi=odd8), "aligned"), (dict(f=odd4), "aligned"), (dict(mu=p[0]), "overlap"), (dict(work=p[3]), "overlap")] + last),
            (stats, plane + dj + wk + [(dict(out=z), "null"), (dict(out=odd8), "aligned"), (dict(out=p[3]), "overlap"), (dict(status=p[0]), "overlap")] + last),
            (update, [(dict(nsig=-1), "nsig")] + dj + rg + wk + [(dict(ll=z), "null"), (dict(sg=odd8), "aligned"), (dict(pi=p[10]), "overlap"), (dict(ll=p[7]), "overlap")] + last),
            (fit, plane + dj + rg + wk + [(dict(n_iter=-1), "n_iter"), (dict(n_iter=100001), "n_iter"), (dict(tol=-1.0), "tol"), (dict(tol=float("nan")), "tol"),
                                          (dict(iters=z), "null"), (dict(ll=odd8), "aligned"), (dict(w=odd4), "aligned"), (dict(o=p[0]), "overlap"), (dict(ll=p[9]), "overlap")] + last),
            (post, plane + dj + wk + [(dict(C=0), "C must"), (dict(C=3), "C must"), (dict(y=z), "go together"), (dict(mask=z), "null"), (dict(x=odd8), "aligned"),
                                      (dict(mask=p[0]), "overlap"), (dict(y=p[13]), "overlap")] + last),
            (spat, plane + [(dict(delay=2), "delay"), (dict(max_delay=0.0), "max_delay"), (dict(pw=0.0), "p must"), (dict(pw=float("nan")), "p must"), (dict(w=z), "null"),
                            (dict(x=odd8), "aligned"), (dict(feat=p[0]), "overlap")] + last)):
        for kw, word in cases:
            if call is update and "rows" in kw:
                continue
            assert call(**kw) == _lib.ERR and word in err(), (call.__name__, kw, err())
        assert call(nsig=0) == _lib.OK
    host = torch.ones(4096, dtype=torch.float64)                                         # a host pointer is refused, not dereferenced
    assert spat(x=ctypes.c_void_p(host.data_ptr())) == _lib.ERR and "device memory" in err()


def test_the_index_rules_under_address_and_ub_sanitizers(tmp_path):
    """glowk_cluster_index.h -- the columns of the moment matrix, the workgroups and chunks of a signal, the chain behind a statistic, the
    workspace -- compiled without HIP into a stand-alone program with its own main (tests/cluster_index_sanitize_main.cpp) and swept
    against straightforward loops.  The same program prints chain() for the GPU tests' shapes, which tests/cluster_ref.py restates."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "cluster_index_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "cluster_index_sanitize_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "CLUSTER_INDEX_SANITIZE_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    shapes = [s[3:] for s in R.GPU_SHAPES] + [(33, 47), (65, 120), (1025, 5626), (4096, 32768)]
    r = subprocess.run([exe, "chain"] + [str(v) for s in shapes for v in s], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and [int(v) for v in r.stdout.split()] == [R.chain(*s) for s in shapes]
