"""REPET-SIM without a GPU: the restatement of tests/repet_ref.py against an independent sklearn recipe on a planted input and
against numpy's median, ``default_k``, the Python argument checks of ``audiosourcesep_amd.repet`` (refused with ValueError before
the library is loaded), and the boundary of the three C entries: declared, exported, bound, and their range checks, which run
before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, repet
from tests import repet_ref as R


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def test_the_neighbour_rule_against_sklearn_on_the_planted_input():
    """12 patterns tiled 5 times with 2 % noise: every frame's neighbours are its 4 other copies, by the restatement and by
    NearestNeighbors(k + 2 width, cosine) with the band removed and the first k kept (librosa's recurrence_matrix recipe)."""
    nn = pytest.importorskip("sklearn.neighbors")
    rows, P, k, width = 33, 12, 4, 5
    S = R.planted(np.random.default_rng(rows + P), rows, P, k + 1)
    F = S.shape[1]
    sim = R.similarity(S)
    idx, val, kth = R.select(sim, k, width)
    j = np.arange(F)
    gap = min(kth[i] - np.sort(sim[i, np.abs(j - i) >= width])[::-1][k] for i in range(F))
    print("planted input: the 4th and 5th candidate are at least %.3f apart" % gap)
    assert gap > 0.1
    _, near = nn.NearestNeighbors(n_neighbors=min(F - 1, k + 2 * width), metric="cosine").fit(S.T.astype(np.float64)).kneighbors()
    copies = R.copies_of(F, P)
    for i in range(F):
        kept = [int(n) for n in near[i] if abs(int(n) - i) >= width][:k]
        assert set(kept) == copies[i] == set(int(n) for n in idx[i]), i
    assert (np.diff(val, axis=1) <= 0).all() and (idx >= 0).all()


def test_the_restatements_rule_on_ties_bands_and_short_signals():
    S = np.zeros((1, 9), np.float32)
    S[0, [0, 2, 3, 5, 6, 8]] = [1.0, 2.0, 0.5, 3.0, 1.5, 4.0]                      # one row: every cosine is 1 or 0
    idx, val = R.neighbors(S, 3, 2)
    assert idx[0].tolist() == [2, 3, 5] and idx[3].tolist() == [0, 5, 6] and idx[8].tolist() == [0, 2, 3]   # ties: the lower index
    assert idx[1].tolist() == [3, 4, 5] and val[1].tolist() == [0.0, 0.0, 0.0]     # a silent frame: everything ties at 0
    assert idx[4].tolist() == [0, 1, 2] and idx[2].tolist() == [0, 5, 6]           # |i - j| >= 2; zeros lose to ones
    idx, val = R.neighbors(np.ones((3, 7), np.float32), 16, 3)                     # k above the candidate count
    assert [int((row >= 0).sum()) for row in idx] == [4, 3, 2, 2, 2, 3, 4] and (val[idx < 0] == 0).all()
    assert idx[3].tolist()[:2] == [0, 6] and (idx[3, 2:] == -1).all()
    idx, _ = R.neighbors(np.ones((3, 7), np.float32), 4, 7)                        # no candidates at all
    assert (idx == -1).all()
    assert np.array_equal(R.gather_median(np.arange(21, dtype=np.float32).reshape(3, 7), idx), np.arange(21, dtype=np.float32).reshape(3, 7))


def test_the_median_restatement_is_numpys_median_of_the_gathered_columns():
    rng = np.random.default_rng(5)
    S = (np.abs(rng.standard_normal((9, 40))) ** 2).astype(np.float32)
    for k, width in ((1, 1), (4, 3), (5, 3), (16, 30)):                           # odd, even and mixed counts
        idx, _ = R.neighbors(S, k, width)
        got = R.gather_median(S, idx)
        assert got.dtype == np.float32
        for i in range(S.shape[1]):
            nb = idx[i][idx[i] >= 0]
            want = np.median(S[:, nb], axis=1) if len(nb) else S[:, i]
            assert np.array_equal(got[:, i].view(np.uint32), want.astype(np.float32).view(np.uint32)), (k, width, i)
    rep, res = R.rep_res(S, got)
    assert (rep <= S).all() and (res >= 0).all() and np.allclose(rep + res, S, rtol=1e-15, atol=0)


def test_default_k():
    for F, width, want in [(5626, 62, 150), (95, 12, 18), (60, 5, 16), (10, 10, 2), (1, 1, 2), (5, 1, 4), (4, 1, 4), (32768, 1, 364),
                           (6, 1, 6), (17, 1, 8), (18, 1, 10)]:
        assert repet.default_k(F, width) == want == R.default_k(F, width), (F, width)
    assert all(repet.default_k(F, w) == R.default_k(F, w) for F in range(1, 400) for w in (1, 2, 7, 200))
    assert repet.default_k(1 << 20, 1) == 512                                      # the cap


def test_bad_arguments_are_refused_before_the_library_loads(monkeypatch, tmp_path):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "_lib", None)
    S, y = np.zeros((12, 30), np.float32), np.zeros(4096, np.float32)
    wav = tmp_path / "none.wav"                                                     # never opened: the arguments are checked first
    bad = []
    for f in (repet.neighbors, repet.nn_filter, repet.repet_sim):
        bad += [
            lambda f=f: f(S, k=0),                                                # k and width: out of range, no integer, boolean
            lambda f=f: f(S, k=513),
            lambda f=f: f(S, k=-1),
            lambda f=f: f(S, k=4.0),
            lambda f=f: f(S, k=True),
            lambda f=f: f(S, k="4"),
            lambda f=f: f(S, width=0),
            lambda f=f: f(S, width=(1 << 20) + 1),
            lambda f=f: f(S, width=2.0),
            lambda f=f: f(S, width=False),
            lambda f=f: f(S, width=None),
            lambda f=f: f(S[0]),                                                  # [F], [a, b, rows, F], no rows, too many rows / frames
            lambda f=f: f(S[None, None]),
            lambda f=f: f(np.zeros((0, 30), np.float32)),
            lambda f=f: f(np.zeros((4097, 2), np.float32)),
            lambda f=f: f(torch.zeros(1, 32769)),
        ]
    bad += [
        lambda: repet.neighbors(S.astype(np.complex64)),
        lambda: repet.nn_filter(S.astype(np.complex64)),
        lambda: repet.neighbors(S, return_similarity=1),
        lambda: repet.nn_filter(S, return_neighbors="yes"),
        lambda: repet.repet_sim(S, margin=0.5),
        lambda: repet.repet_sim(S, margin=(1.0, 0.99)),
        lambda: repet.repet_sim(S, margin=(2.0,)),
        lambda: repet.repet_sim(S, margin=(2.0, 10.0, 1.0)),
        lambda: repet.repet_sim(S, margin=float("inf")),
        lambda: repet.repet_sim(S, margin=(2.0, float("nan"))),
        lambda: repet.repet_sim(S, margin="2"),
        lambda: repet.repet_sim(S, power=0),
        lambda: repet.repet_sim(S, power=-2.0),
        lambda: repet.repet_sim(S, power=float("nan")),
        lambda: repet.repet_sim(S, power=None),
        lambda: repet.repet_sim(S, mask=1),
        lambda: repet.repet_sim(np.zeros((4097, 2), np.complex64)),
        lambda: repet.repet_sim_audio(y[:1024]),                                  # n <= 1024
        lambda: repet.repet_sim_audio(np.zeros((2, 3, 4096), np.float32)),
        lambda: repet.repet_sim_audio(y.astype(np.complex64)),
        lambda: repet.repet_sim_audio(y, k=0),
        lambda: repet.repet_sim_audio(y, k=600),
        lambda: repet.repet_sim_audio(y, k=True),
        lambda: repet.repet_sim_audio(y, width_sec=-1.0),
        lambda: repet.repet_sim_audio(y, width_sec=float("nan")),
        lambda: repet.repet_sim_audio(y, width_sec="2"),
        lambda: repet.repet_sim_audio(y, width_sec=1e6),
        lambda: repet.repet_sim_audio(y, margin=0.0),
        lambda: repet.repet_sim_audio(y, power=0.0),
        lambda: repet.repet_sim_audio(y, residual="yes"),
        lambda: repet.separate_wav_repet(str(wav), out_rate="native"),
        lambda: repet.separate_wav_repet(str(wav), out_rate=10),
        lambda: repet.separate_wav_repet(str(wav), k=0),
        lambda: repet.separate_wav_repet(str(wav), margin=0.5),
        lambda: repet.separate_wav_repet(str(wav), power=-1.0),
        lambda: repet.separate_wav_repet(str(wav), width=3),                      # no argument of repet_sim_audio
        lambda: repet.separate_wav_repet(str(wav), kernel_size=31),
    ]
    for n, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % n)
    with pytest.raises(TypeError):
        repet.repet_sim(S, kernel_size=31)                                        # an unknown keyword of a plain function


def test_the_three_entries_are_declared_exported_and_bound(lib, repo_root):
    text = open(os.path.join(repo_root, "include", "glowk.h")).read()
    for proto in (
        "size_t glowk_nn_workspace_bytes(int nsig, int rows, int frames, int k);",
        "int glowk_nn_neighbors(const float* s_dev, int nsig, int rows, int frames, int k, int width,\n"
        "                       int32_t* idx_dev /* [nsig][frames][k] */, float* sim_dev /* same shape, may be null; 0 where idx is -1 */,\n"
        "                       void* work_dev, size_t work_bytes, void* stream);",
        "int glowk_nn_median(const float* s_dev, const int32_t* idx_dev, int nsig, int rows, int frames, int k,\n"
        "                    float* out_dev /* [nsig][rows][frames], not s_dev */, void* work_dev, size_t work_bytes, void* stream);",
    ):
        assert proto in text, proto
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert _lib.SYMBOLS["glowk_nn_workspace_bytes"] == (sz, [i, i, i, i])
    assert _lib.SYMBOLS["glowk_nn_neighbors"] == (i, [vp, i, i, i, i, i, vp, vp, vp, sz, vp])
    assert _lib.SYMBOLS["glowk_nn_median"] == (i, [vp, vp, i, i, i, i, vp, vp, sz, vp])
    for name in ("glowk_nn_workspace_bytes", "glowk_nn_neighbors", "glowk_nn_median"):
        assert getattr(lib, name) is not None
    version = int(re.search(r"#define GLOWK_VERSION (\d+)", text).group(1))
    assert lib.glowk_version() == version >= 520                                  # (the version that introduced them)
    assert "Since version 520" in text


def _err(lib):
    return lib.glowk_last_error().decode()


def test_the_workspace_is_positive_and_linear_in_the_frames(lib):
    for nsig, rows, F, k in [(1, 1, 1, 1), (1, 1025, 5626, 150), (3, 33, 129, 8), (1, 4096, 66, 6), (1, 5, 600, 512), (2, 96, 16384, 512),
                             (1, 2, 31, 16), (3, 33, 95, 3)]:
        one, two = lib.glowk_nn_workspace_bytes(nsig, rows, F, k), lib.glowk_nn_workspace_bytes(nsig, rows, 2 * F, k)
        assert one == (4 * nsig * F * (rows + 1) + 7) // 8 * 8                       # the norms and the frame-major copy, in 8-byte words:
        assert one % 8 == 0                                                         # 93 and 9690 floats (the last two) are odd counts
        assert one > 0 and two <= 2 * one + 65536, (nsig, rows, F, k)
        assert one <= 4 * nsig * F * (rows + k) + 65536                            # like nsig frames (rows + k), never frames^2
    for args in [(-1, 12, 30, 4), (65536, 12, 30, 4), (1, 0, 30, 4), (1, 4097, 30, 4), (1, 12, 0, 4), (1, 12, 32769, 4), (1, 12, 30, 0),
                 (1, 12, 30, 513)]:
        assert lib.glowk_nn_workspace_bytes(*args) == 0
    assert lib.glowk_nn_workspace_bytes(0, 12, 30, 4) == 0                         # no signals need no workspace


def test_the_entries_refuse_bad_ranges_before_touching_a_device(lib):
    z, a, b, c, w = (ctypes.c_void_p(v) for v in (0, 1 << 20, 1 << 30, 1 << 31, 1 << 32))   # never dereferenced: refused first
    big = 1 << 40

    def nb(nsig=1, rows=12, F=30, k=4, width=2, s=a, idx=b, sim=c, work=w, nbytes=big):
        return lib.glowk_nn_neighbors(s, nsig, rows, F, k, width, idx, sim, work, nbytes, z)

    def med(nsig=1, rows=12, F=30, k=4, s=a, idx=b, out=c, work=w, nbytes=big):
        return lib.glowk_nn_median(s, idx, nsig, rows, F, k, out, work, nbytes, z)

    ranges = [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(rows=0), "rows"), (dict(rows=4097), "rows"), (dict(F=0), "frames"),
              (dict(F=32769), "frames"), (dict(k=0), "k must"), (dict(k=513), "k must"), (dict(k=-4), "k must"),
              (dict(nsig=65535, rows=4096, F=9), "2^31"), (dict(nsig=16, rows=4096, F=32768), "2^31"),
              (dict(nsig=65535, rows=1, F=32768, k=2), "2^31"), (dict(nsig=4096, rows=1, F=32768, k=512), "2^31")]
    for kw, word in ranges:
        assert nb(**kw) == _lib.ERR and word in _err(lib), kw
        assert med(**kw) == _lib.ERR and word in _err(lib), kw
    for width in (0, -1, (1 << 20) + 1):
        assert nb(width=width) == _lib.ERR and "width" in _err(lib)
    assert nb(width=1) == _lib.ERR and "device memory" in _err(lib)               # the bounds themselves pass the range checks
    assert nb(width=1 << 20, k=512, rows=4096) == _lib.ERR and "device memory" in _err(lib)
    assert nb(nsig=0, s=z, idx=z, sim=z, work=z, nbytes=0) == _lib.OK               # no signals: a successful no-op ...
    assert med(nsig=0, s=z, idx=z, out=z, work=z, nbytes=0) == _lib.OK
    assert nb(nsig=0, k=0, s=z, idx=z, sim=z, work=z, nbytes=0) == _lib.ERR         # ... of valid arguments only
    assert nb(nsig=0, width=0, s=z, idx=z, sim=z, work=z, nbytes=0) == _lib.ERR
    assert med(nsig=0, rows=0, s=z, idx=z, out=z, work=z, nbytes=0) == _lib.ERR
    for kw in (dict(s=z), dict(idx=z), dict(work=z)):
        assert nb(**kw) == _lib.ERR and "null" in _err(lib), kw
    for kw in (dict(s=z), dict(idx=z), dict(out=z), dict(work=z)):
        assert med(**kw) == _lib.ERR and "null" in _err(lib), kw
    assert nb(sim=z) == _lib.ERR and "device memory" in _err(lib)                  # sim_dev may be null
    need = lib.glowk_nn_workspace_bytes(1, 12, 30, 4)
    assert nb(nbytes=need - 1) == _lib.ERR and "work_bytes" in _err(lib)
    assert med(nbytes=need - 1) == _lib.ERR and "work_bytes" in _err(lib)
    assert nb(nbytes=0) == _lib.ERR and "work_bytes" in _err(lib)
    assert nb(nbytes=need) == _lib.ERR and "device memory" in _err(lib)            # exactly enough passes this check
    assert med(out=a) == _lib.ERR and "out_dev" in _err(lib)                       # in place
    assert med(out=ctypes.c_void_p((1 << 20) + 4 * 359)) == _lib.ERR and "out_dev" in _err(lib)
    assert med(out=ctypes.c_void_p((1 << 20) - 4 * 359)) == _lib.ERR and "out_dev" in _err(lib)
    assert nb(sim=b) == _lib.ERR and "overlap" in _err(lib)
    assert nb(work=a) == _lib.ERR and "work_dev" in _err(lib)
    assert med(work=c) == _lib.ERR and "work_dev" in _err(lib)
    # a host pointer is refused (where there is no device at all, every pointer is one)
    host, idx, out = np.zeros(12 * 30, np.float32), np.zeros(30 * 4, np.int32), np.zeros(12 * 30, np.float32)
    work = np.zeros(need // 4 + 1, np.float32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert nb(s=p(host), idx=p(idx), sim=z, work=p(work), nbytes=work.nbytes) == _lib.ERR and "device memory" in _err(lib)
    assert med(s=p(host), idx=p(idx), out=p(out), work=p(work), nbytes=work.nbytes) == _lib.ERR and "device memory" in _err(lib)
