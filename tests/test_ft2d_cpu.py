"""The 2DFT separation without a GPU: the restatement of tests/ft2d_ref.py against numpy.fft and scipy.ndimage (scipy's own
``mode='wrap'`` is right at halos deeper than the axis -- checked here against a tiled copy, unlike its reflect of DESIGN section 17),
the symmetry of the peak mask, the linearity identity, the undecidable share of the end-to-end shapes, the Python argument checks of
``audiosourcesep_amd.ft2d`` (ValueError before the library is loaded), the boundary of the C entries (declared, exported, bound,
version 540; every refusal before any device call), and the index rules the kernels share with the host under AddressSanitizer +
UBSan in a stand-alone program."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from scipy import ndimage

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, ft2d
from tests import ft2d_ref as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SHAPES = [(1, 1), (1, 2), (2, 3), (3, 5), (33, 64), (65, 130), (17, 75)]
E2E = [(33, 64, 8), (65, 130, 13), (129, 257, 16), (96, 600, 25), (1025, 96, 12)]    # (rows, frames, period) of the GPU end-to-end test
E2E_MULTIPLIER = 4.5                        # tests/test_gpu_ft2d.py derives it


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def plane(shape, seed=0):
    return np.abs(np.random.default_rng(seed).standard_normal(shape)) ** 2


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_transforms_are_numpys(shape):
    R, T = shape
    x = plane(shape, 1)
    scale = np.abs(x).sum()
    assert np.abs(F.rfft2_matrix(x) - np.fft.rfft2(x)).max() <= 1e-13 * scale
    assert np.array_equal(F.rfft2(x.astype(np.float32)), np.fft.rfft2(x.astype(np.float32).astype(np.float64)))
    rng = np.random.default_rng(2)
    G = rng.standard_normal((R, T // 2 + 1)) + 1j * rng.standard_normal((R, T // 2 + 1))    # self-conjugate columns with imaginary parts
    want = np.fft.irfft2(G, s=(R, T))
    assert np.abs(F.irfft2_matrix(G, T) - want).max() <= 1e-13 * np.abs(G).sum() / (R * T) * 4 + 1e-15
    assert np.array_equal(F.irfft2(G, T), want)
    G0 = G.copy()
    G0[:, 0] = G0[:, 0].real
    if T % 2 == 0:
        G0[:, -1] = G0[:, -1].real
    R1 = np.fft.ifft(G0, axis=0)                                                       # dropping them after the row stage is numpy's rule
    R2 = np.fft.ifft(G, axis=0)
    R2[:, 0] = R2[:, 0].real
    if T % 2 == 0:
        R2[:, -1] = R2[:, -1].real
    assert np.abs(np.fft.irfft(R2, T, axis=1) - want).max() <= 1e-13
    del R1
    assert np.abs(F.irfft2_matrix(F.rfft2_matrix(x), T) - x).max() <= 1e-12 * x.max()
    M = (rng.random((R, T)) < 0.5).astype(np.float64)
    assert np.array_equal(F.irfft2(G, T, M), np.fft.irfft2(G * M[:, :T // 2 + 1], s=(R, T)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_magnitude_plane_is_the_full_transforms(shape):
    R, T = shape
    x = plane(shape, 3)
    mag = F.magnitude_plane(F.rfft2(x), T)
    full = np.abs(np.fft.fft2(x))
    assert mag.shape == (R, T) and np.abs(mag - full).max() <= 1e-12 * x.sum()
    u, v = np.meshgrid(np.arange(R), np.arange(T), indexing="ij")
    assert np.array_equal(mag, mag[(R - u) % R, (T - v) % T])                         # Hermitian in its bits
    copy, uu, vv = F.copied_cells(R, T)
    assert not copy[uu[copy], vv[copy]].any() and copy.sum() == (R * T - np.sum((uu == u) & (vv == v))) // 2   # one of every pair
    m32 = F.magnitude_plane(F.rfft2(x).astype(np.complex64), T, np.float32)
    assert m32.dtype == np.float32 and np.array_equal(m32, m32[(R - u) % R, (T - v) % T])
    mean, std = F.plane_std(mag)
    assert mean == mag.mean() and std == np.sqrt(((mag - mag.mean()) ** 2).mean())


def tiled_filter(fn, P, nb):
    """scipy's filter on a copy tiled far enough that no halo leaves it: the periodic filter whatever scipy's edge code does."""
    reps = [2 * (-(-(n // 2) // s)) + 1 for n, s in zip(nb, P.shape)]
    off = [(r // 2) * s for r, s in zip(reps, P.shape)]
    return fn(np.tile(P, reps), size=nb, mode="wrap")[off[0]:off[0] + P.shape[0], off[1]:off[1] + P.shape[1]]


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (3, 4), (5, 7), (33, 64)], ids=lambda s: "%dx%d" % s)
def test_the_peak_rule_is_scipys_wrap_filters(shape):
    rng = np.random.default_rng(4)
    ties = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], np.float32), shape)
    for P in (rng.standard_normal(shape).astype(np.float32), ties, np.full(shape, 1.5, np.float32)):
        for nb in [(1, 1), (1, 25), (3, 5), (127, 1), (1, 127), (5, 2 * shape[1] + 1)]:     # the last four longer than an axis here
            mx, mn = F.extrema(P, nb)
            assert mx.dtype == np.float32
            for got, fn in ((mx, ndimage.maximum_filter), (mn, ndimage.minimum_filter)):
                assert np.array_equal(got, fn(P, size=nb, mode="wrap")) and np.array_equal(got, tiled_filter(fn, P, nb))
            assert np.array_equal(F.peaks(P, nb), (P == mx).astype(np.float32))
            d = (mx - mn).ravel()
            thr = d[len(d) // 2]
            M = F.peaks(P, nb, thr)
            assert np.array_equal(M, ((P == mx) & ((mx - mn) > thr)).astype(np.float32))           # strict
            assert not M[(mx - mn) == thr].any()
    assert np.array_equal(F.peaks(np.float32([[1, 3, 2, 3, 0]]), (1, 3)), np.float32([[0, 1, 0, 1, 0]]))
    assert np.array_equal(F.peaks(np.float32([[4, 1, 2, 3, 0]]), (1, 3)), np.float32([[1, 0, 0, 1, 0]]))   # the edges wrap: 0 sees 4
    assert np.array_equal(F.peaks(np.float32([[4, 1, 2, 3, 0]]), (1, 3), 3.0), np.float32([[1, 0, 0, 0, 0]]))   # 3 - 0 is not > 3


@pytest.mark.parametrize("nb", [(1, 25), (3, 5), (5, 1)], ids=str)
def test_the_mask_is_symmetric_and_the_masked_inverse_is_real(nb):
    for shape in [(33, 64), (17, 75), (2, 3)]:
        R, T = shape
        x = plane(shape, 5)
        r = F.ft2d(x, nb, 0.5)
        M = r["M"]
        u, v = np.meshgrid(np.arange(R), np.arange(T), indexing="ij")
        assert np.array_equal(M, M[(R - u) % R, (T - v) % T]) and 0 < M.sum() < M.size or M.size <= 6
        full = np.fft.ifft2(np.fft.fft2(x) * M)
        assert np.abs(full.imag).max() <= 1e-12 * x.max() and np.abs(full.real - r["B"]).max() <= 1e-12 * x.max()


def test_the_foregrounds_inverse_is_the_difference():
    x = plane((33, 64), 6)
    r = F.ft2d(x, (1, 25), 1.0)
    fore = F.irfft2(r["F"], 64, 1.0 - r["M"])
    assert np.abs(fore - (x - r["B"])).max() <= 1e-12 * x.max()
    assert np.array_equal(r["res"], np.abs(x - r["B"])) and np.array_equal(r["rep"], np.abs(r["B"]))
    assert np.abs(r["mask_b"] + r["mask_f"] - 1.0).max() <= 1e-12                       # unit margins, power 1: a partition


@pytest.mark.parametrize("case", E2E, ids=lambda c: "%dx%d" % c[:2])
def test_the_end_to_end_inputs_stay_under_the_undecidable_cap(case):
    R, T, p = case
    bg, fg = F.crafted(R, T, p, 7)
    x = (bg + fg).astype(np.float32)
    und, r = F.undecidable(x, (1, 25), 1.0, E2E_MULTIPLIER)
    share = und.mean()
    print("ft2d end to end %dx%d: %.4f %% of the cells undecidable at %.1f bars, %d peaks" % (R, T, 100 * share, E2E_MULTIPLIER, r["M"].sum()))
    assert share <= 0.01
    if (R, T) == (96, 600):
        keep_b = (r["mask_b"] * bg).sum() / bg.sum()
        keep_f = (r["mask_f"] * fg).sum() / fg.sum()
        print("ft2d at 96x600: background keeps %.3f of bg, foreground keeps %.3f of fg" % (keep_b, keep_f))
        assert keep_b > 0.5 and keep_f > 0.5


def test_bad_arguments_are_refused_before_the_library_is_loaded(tmp_path, monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    S = np.ones((4, 9), np.float32)
    y = np.zeros(4096, np.float32)
    wav = tmp_path / "never_opened.wav"
    bad = [
        lambda: ft2d.ft2d(S, neighborhood=(1, 24)),
        lambda: ft2d.ft2d(S, neighborhood=(0, 25)),
        lambda: ft2d.ft2d(S, neighborhood=(1, 129)),
        lambda: ft2d.ft2d(S, neighborhood=25),
        lambda: ft2d.ft2d(S, neighborhood=(1, 25, 1)),
        lambda: ft2d.ft2d(S, neighborhood=(1.0, 25)),
        lambda: ft2d.ft2d(S, neighborhood=(True, 25)),
        lambda: ft2d.ft2d(S, threshold_scale=-1.0),
        lambda: ft2d.ft2d(S, threshold_scale=float("nan")),
        lambda: ft2d.ft2d(S, threshold_scale="1"),
        lambda: ft2d.ft2d(S, power=0.0),
        lambda: ft2d.ft2d(S, margin=0.5),
        lambda: ft2d.ft2d(S, margin=(1.0, 2.0, 3.0)),
        lambda: ft2d.ft2d(S, mask="yes"),
        lambda: ft2d.ft2d(S, return_peaks=1),
        lambda: ft2d.ft2d(np.ones(9, np.float32)),
        lambda: ft2d.ft2d(np.ones((1, 4097, 2), np.float32)),
        lambda: ft2d.ft2d(torch.empty((2, 3, 32769), device="meta")),
        lambda: ft2d.rfft2(S, return_magnitude="yes"),
        lambda: ft2d.rfft2(S.astype(np.complex64)),
        lambda: ft2d.rfft2(np.ones((2, 2, 2, 2), np.float32)),
        lambda: ft2d.irfft2(np.ones((4, 5), np.complex64), 0),
        lambda: ft2d.irfft2(np.ones((4, 5), np.complex64), 10),                       # 10 frames have 6 columns
        lambda: ft2d.irfft2(np.ones((4, 5), np.complex64), 32769),
        lambda: ft2d.irfft2(np.ones((4, 5), np.complex64), 9.0),
        lambda: ft2d.irfft2(np.ones((4, 5), np.complex64), 9, mask=np.ones((4, 5), np.float32)),   # the mask is a full plane
        lambda: ft2d.irfft2(np.ones((4, 5), np.complex64), 9, mask=np.ones((4, 9), np.complex64)),
        lambda: ft2d.irfft2(np.ones((4097, 5), np.complex64), 9),
        lambda: ft2d.peak_mask(S, neighborhood=(2, 25)),
        lambda: ft2d.peak_mask(S, threshold=np.ones(3, np.float32)),
        lambda: ft2d.peak_mask(S, threshold=True),
        lambda: ft2d.peak_mask(S.astype(np.complex64)),
        lambda: ft2d.peak_mask(S, return_extrema="yes"),
        lambda: ft2d.ft2d_audio(y, neighborhood=(1, 2)),
        lambda: ft2d.ft2d_audio(y, threshold_scale=None),
        lambda: ft2d.ft2d_audio(y, cutoff_hz=-1.0),
        lambda: ft2d.ft2d_audio(y, cutoff_hz=9000.0),
        lambda: ft2d.ft2d_audio(y, cutoff_hz=None),
        lambda: ft2d.ft2d_audio(y, margin=0.0),
        lambda: ft2d.ft2d_audio(y, power=0.0),
        lambda: ft2d.ft2d_audio(y, residual="yes"),
        lambda: ft2d.ft2d_audio(np.zeros(1024, np.float32)),
        lambda: ft2d.separate_wav_ft2d(str(wav), out_rate="native"),
        lambda: ft2d.separate_wav_ft2d(str(wav), out_rate=10),
        lambda: ft2d.separate_wav_ft2d(str(wav), mono="yes"),
        lambda: ft2d.separate_wav_ft2d(str(wav), neighborhood=(1, 4)),
        lambda: ft2d.separate_wav_ft2d(str(wav), margin=0.5),
        lambda: ft2d.separate_wav_ft2d(str(wav), period_sec=(0.3, 0.8)),                # repet_audio's, not ft2d_audio's
        lambda: ft2d.separate_wav_ft2d(str(wav), k=8),
    ]
    for n, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % n)
    with pytest.raises(TypeError):
        ft2d.ft2d(S, period=7)                                                          # an unknown keyword of a plain function
    assert not wav.exists()


PROTOTYPES = (
    "size_t glowk_dft2_workspace_bytes(int nsig, int rows, int frames);",
    "int glowk_rdft2(const float* s_dev, int nsig, int rows, int frames, float* spec_dev /* [nsig][rows][fc] interleaved complex64 */,\n"
    "                float* mag_dev /* [nsig][rows][frames], may be null */, void* work_dev, size_t work_bytes, void* stream);",
    "int glowk_irdft2(const float* spec_dev, const float* mask_dev /* [nsig][rows][frames], may be null */, int nsig, int rows, int frames,\n"
    "                 float* out_dev /* [nsig][rows][frames] */, void* work_dev, size_t work_bytes, void* stream);",
    "size_t glowk_plane_std_workspace_bytes(int nsig, int64_t n);",
    "int glowk_plane_std(const float* plane_dev /* [nsig][n] */, int nsig, int64_t n, double* out_dev /* [nsig][2] */, void* work_dev,\n"
    "                    size_t work_bytes, void* stream);",
    "size_t glowk_peak_workspace_bytes(int nsig, int rows, int cols);",
    "int glowk_peak_mask(const float* plane_dev, int nsig, int rows, int cols, int nb_r, int nb_c, const float* thr_dev /* [nsig], may be null */,\n"
    "                    float* mask_dev, float* max_dev /* may be null */, float* min_dev /* may be null */, void* work_dev, size_t work_bytes,\n"
    "                    void* stream);",
)
NAMES = ("glowk_dft2_workspace_bytes", "glowk_rdft2", "glowk_irdft2", "glowk_plane_std_workspace_bytes", "glowk_plane_std",
         "glowk_peak_workspace_bytes", "glowk_peak_mask")


def test_the_entries_are_declared_exported_and_bound(lib):
    text = open(os.path.join(REPO, "include", "glowk.h")).read()
    for proto in PROTOTYPES:
        assert proto in text, proto
    vp, i, sz, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int64
    assert _lib.SYMBOLS["glowk_dft2_workspace_bytes"] == (sz, [i, i, i])
    assert _lib.SYMBOLS["glowk_rdft2"] == (i, [vp, i, i, i, vp, vp, vp, sz, vp])
    assert _lib.SYMBOLS["glowk_irdft2"] == (i, [vp, vp, i, i, i, vp, vp, sz, vp])
    assert _lib.SYMBOLS["glowk_plane_std_workspace_bytes"] == (sz, [i, i64])
    assert _lib.SYMBOLS["glowk_plane_std"] == (i, [vp, i, i64, vp, vp, sz, vp])
    assert _lib.SYMBOLS["glowk_peak_workspace_bytes"] == (sz, [i, i, i])
    assert _lib.SYMBOLS["glowk_peak_mask"] == (i, [vp, i, i, i, i, i, vp, vp, vp, vp, vp, sz, vp])
    for name in NAMES:
        assert getattr(lib, name) is not None
    version = int(re.search(r"#define GLOWK_VERSION (\d+)", text).group(1))
    assert lib.glowk_version() == version >= 540                                  # (the version that introduced them)
    assert "Since version 540" in text


def _err(lib):
    return lib.glowk_last_error().decode()


def test_the_workspace_is_linear_in_the_input(lib):
    ws = lib.glowk_dft2_workspace_bytes
    for nsig, rows, T in [(1, 1, 1), (1, 1025, 5626), (3, 65, 130), (1, 4096, 34), (2, 96, 32768)]:
        got = ws(nsig, rows, T)
        assert got == 8 * (T + rows + nsig * rows * (T // 2 + 1))
        assert ws(2 * nsig, rows, T) - got == 8 * nsig * rows * (T // 2 + 1)           # a batch is its signals side by side
    assert ws(1, 1025, 5626) <= 1.01 * 4 * 1025 * 5628                                # the plane between the stages, no more
    for args in [(-1, 12, 30), (65536, 12, 30), (1, 0, 30), (1, 4097, 30), (1, 12, 0), (1, 12, 32769), (16, 4096, 32768)]:
        assert ws(*args) == 0, args
        assert lib.glowk_peak_workspace_bytes(*args) == 0, args
    assert ws(0, 12, 30) == 0
    assert lib.glowk_peak_workspace_bytes(2, 12, 30) == 8 * 2 * 12 * 30
    sw = lib.glowk_plane_std_workspace_bytes
    assert sw(1, 1) == 16 and sw(1, 4096) == 16 and sw(1, 4097) == 32 and sw(3, 1025 * 5626) == 3 * 256 * 16
    assert sw(0, 5) == 0 and sw(1, 0) == 0 and sw(2, 1 << 30) == 0 and sw(65536, 1) == 0


def test_the_entries_refuse_bad_arguments_before_touching_a_device(lib):
    z, a, b, c, d, w = (ctypes.c_void_p(v) for v in (0, 1 << 20, 1 << 30, 1 << 31, 3 << 30, 1 << 32))   # never dereferenced: refused first
    big = 1 << 40

    def fw(nsig=1, rows=12, T=30, s=a, spec=b, mag=z, work=w, nbytes=big):
        return lib.glowk_rdft2(s, nsig, rows, T, spec, mag, work, nbytes, z)

    def iv(nsig=1, rows=12, T=30, spec=a, mask=z, out=b, work=w, nbytes=big):
        return lib.glowk_irdft2(spec, mask, nsig, rows, T, out, work, nbytes, z)

    def sd(nsig=1, n=360, plane=a, out=b, work=w, nbytes=big):
        return lib.glowk_plane_std(plane, nsig, n, out, work, nbytes, z)

    def pk(nsig=1, rows=12, cols=30, nb_r=1, nb_c=25, plane=a, thr=z, mask=b, mx=z, mn=z, work=w, nbytes=big):
        return lib.glowk_peak_mask(plane, nsig, rows, cols, nb_r, nb_c, thr, mask, mx, mn, work, nbytes, z)

    ranges = [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(rows=0), "rows"), (dict(rows=4097), "rows"), (dict(T=0), "frames"),
              (dict(T=32769), "frames"), (dict(nsig=16, rows=4096, T=32768), "2^31")]
    for call in (fw, iv):
        for kw, word in ranges:
            assert call(**kw) == _lib.ERR and word in _err(lib), kw
        assert call() == _lib.ERR and "device memory" in _err(lib)                     # valid ranges reach the pointer check
        assert call(rows=4096, T=1) == _lib.ERR and "device memory" in _err(lib)
        assert call(rows=1, T=32768) == _lib.ERR and "device memory" in _err(lib)
        assert call(nsig=0, work=z, nbytes=0) == _lib.OK                               # no signals: a successful no-op ...
        assert call(nsig=0, rows=0, work=z, nbytes=0) == _lib.ERR                      # ... of valid arguments only
        assert call(work=z) == _lib.ERR and "null" in _err(lib)
        need = lib.glowk_dft2_workspace_bytes(1, 12, 30)
        assert call(nbytes=need - 1) == _lib.ERR and "work_bytes" in _err(lib)
        assert call(nbytes=need) == _lib.ERR and "device memory" in _err(lib)
        assert call(work=ctypes.c_void_p((1 << 32) + 4)) == _lib.ERR and "aligned" in _err(lib)
        assert call(work=a) == _lib.ERR and "work_dev" in _err(lib)
        assert call(work=b) == _lib.ERR and "work_dev" in _err(lib)
    for kw in (dict(s=z), dict(spec=z)):
        assert fw(**kw) == _lib.ERR and "null" in _err(lib), kw
    assert fw(spec=a) == _lib.ERR and "overlap" in _err(lib)
    assert fw(spec=ctypes.c_void_p((1 << 20) + 8 * 179)) == _lib.ERR and "overlap" in _err(lib)      # inside s
    assert fw(mag=a) == _lib.ERR and "overlap" in _err(lib)
    assert fw(mag=b) == _lib.ERR and "overlap" in _err(lib)
    assert fw(mag=w) == _lib.ERR and "work_dev" in _err(lib)
    assert fw(spec=ctypes.c_void_p((1 << 30) + 4)) == _lib.ERR and "aligned" in _err(lib)
    for kw in (dict(spec=z), dict(out=z)):
        assert iv(**kw) == _lib.ERR and "null" in _err(lib), kw
    assert iv(out=a) == _lib.ERR and "overlap" in _err(lib)
    assert iv(mask=b) == _lib.ERR and "overlap" in _err(lib)
    assert iv(mask=w) == _lib.ERR and "work_dev" in _err(lib)
    assert iv(mask=c) == _lib.ERR and "device memory" in _err(lib)

    for kw, word in [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(n=0), "n must"), (dict(n=1 << 31), "n must"),
                     (dict(nsig=3, n=1 << 30), "2^31")]:
        assert sd(**kw) == _lib.ERR and word in _err(lib), kw
    assert sd() == _lib.ERR and "device memory" in _err(lib)
    assert sd(nsig=0, plane=z, out=z, work=z, nbytes=0) == _lib.OK and sd(nsig=0, n=0, plane=z, out=z, work=z, nbytes=0) == _lib.ERR
    for kw in (dict(plane=z), dict(out=z), dict(work=z)):
        assert sd(**kw) == _lib.ERR and "null" in _err(lib), kw
    assert sd(nbytes=15) == _lib.ERR and "work_bytes" in _err(lib)
    assert sd(nbytes=16) == _lib.ERR and "device memory" in _err(lib)
    assert sd(out=ctypes.c_void_p((1 << 30) + 4)) == _lib.ERR and "aligned" in _err(lib)
    assert sd(out=ctypes.c_void_p((1 << 20) + 8)) == _lib.ERR and "overlap" in _err(lib)
    assert sd(work=a) == _lib.ERR and "work_dev" in _err(lib)

    for kw, word in [(dict(nsig=-1), "nsig"), (dict(nsig=65536), "nsig"), (dict(rows=0), "rows"), (dict(rows=4097), "rows"), (dict(cols=0), "frames"),
                     (dict(cols=32769), "frames"), (dict(nsig=16, rows=4096, cols=32768), "2^31"), (dict(nb_r=0), "nb_r"), (dict(nb_r=2), "nb_r"),
                     (dict(nb_r=129), "nb_r"), (dict(nb_r=-1), "nb_r"), (dict(nb_c=0), "nb_c"), (dict(nb_c=24), "nb_c"), (dict(nb_c=128), "nb_c"),
                     (dict(nb_c=129), "nb_c")]:
        assert pk(**kw) == _lib.ERR and word in _err(lib), kw
    assert pk() == _lib.ERR and "device memory" in _err(lib)
    assert pk(nb_r=127, nb_c=127) == _lib.ERR and "device memory" in _err(lib)
    assert pk(nsig=0, plane=z, mask=z, work=z, nbytes=0) == _lib.OK and pk(nsig=0, nb_c=2, plane=z, mask=z, work=z, nbytes=0) == _lib.ERR
    for kw in (dict(plane=z), dict(mask=z), dict(work=z)):
        assert pk(**kw) == _lib.ERR and "null" in _err(lib), kw
    need = lib.glowk_peak_workspace_bytes(1, 12, 30)
    assert pk(nbytes=need - 1) == _lib.ERR and "work_bytes" in _err(lib)
    assert pk(nbytes=need) == _lib.ERR and "device memory" in _err(lib)
    assert pk(mask=a) == _lib.ERR and "overlap" in _err(lib)
    assert pk(mx=b) == _lib.ERR and "overlap" in _err(lib)
    assert pk(mx=c, mn=c) == _lib.ERR and "overlap" in _err(lib)
    assert pk(mn=a) == _lib.ERR and "overlap" in _err(lib)
    assert pk(thr=b) == _lib.ERR and "overlap" in _err(lib)
    assert pk(work=b) == _lib.ERR and "work_dev" in _err(lib)
    assert pk(mx=c, mn=d) == _lib.ERR and "device memory" in _err(lib)
    # a host pointer is refused (where there is no device at all, every pointer is one)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    host, spec, work = np.zeros(12 * 30, np.float32), np.zeros(12 * 16, np.complex64), np.zeros(need // 8 + 64, np.float64)
    out, mask = np.zeros(12 * 30, np.float32), np.zeros(12 * 30, np.float32)
    nb = work.nbytes
    assert lib.glowk_rdft2(p(host), 1, 12, 30, p(spec), z, p(work), nb, z) == _lib.ERR and "device memory" in _err(lib)
    assert lib.glowk_irdft2(p(spec), z, 1, 12, 30, p(out), p(work), nb, z) == _lib.ERR and "device memory" in _err(lib)
    assert lib.glowk_plane_std(p(host), 1, 360, p(work[:2]), p(work[8:]), nb - 64, z) == _lib.ERR and "device memory" in _err(lib)
    assert lib.glowk_peak_mask(p(host), 1, 12, 30, 1, 25, z, p(mask), z, z, p(work), nb, z) == _lib.ERR and "device memory" in _err(lib)


def test_the_index_rules_under_address_and_ub_sanitizers(tmp_path):
    """glowk_dft2_index.h -- the wrap map, the twiddle index stepping, the tiling plan and the workspace layout that the kernels and
    the entry points call -- compiled without HIP into a stand-alone program with its own main (tests/dft2_index_sanitize_main.cpp)
    and swept against straightforward loops."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "dft2_index_asan")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "dft2_index_sanitize_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "DFT2_INDEX_SANITIZE_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
