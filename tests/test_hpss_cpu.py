"""Harmonic / percussive separation without a GPU: the restatement of tests/hpss_ref.py against scipy.ndimage (bit for bit, where
scipy imports) and against numpy's own symmetric padding, the Python argument checks of ``audiosourcesep_amd.hpss`` (refused with
ValueError before the library is loaded), and the boundary of the two C entries: declared, exported, bound, and their range
checks, which run before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, hpss
from tests import hpss_ref as R

AXIS_LENGTHS = [1, 3, 4, 5, 30, 31, 40, 70]              # with sizes up to 127: windows many times longer than the axis
SIZES = [1, 3, 5, 17, 31, 127]


def quantised(rng, shape):
    """|N(0, 1)| quantised to 8 levels (multiples of 1/2), 30 % exact zeros: ties and equal runs are the norm."""
    x = np.minimum(np.floor(np.abs(rng.standard_normal(shape)) * 2.0), 7.0) / 2.0
    x[rng.random(shape) < 0.3] = 0.0
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


@pytest.mark.parametrize("n", AXIS_LENGTHS)
def test_the_index_map_is_numpys_symmetric_extension(n):
    a = np.arange(n)
    for h in (0, 1, 2, 15, 63):
        want = np.pad(a, h, mode="symmetric")                                      # d c b a | a b c d | d c b a, any number of times
        assert np.array_equal(R.reflect_index(np.arange(-h, n + h), n), want), (n, h)


def scipy_median(ndimage, S, size, ax):
    """scipy's median of ``size`` along array axis ``ax`` of the 2-D S with mode='reflect'.  scipy 1.15.3's own extension of a line
    goes wrong once the halo reaches four axis lengths (size // 2 >= 4 n: for even n the result is another one, for odd n values
    appear that are not in the input and change from run to run -- measured for n = 2 .. 8), so from there on scipy filters the
    array extended by numpy's symmetric padding, which ``test_the_index_map_is_numpys_symmetric_extension`` pins, and the middle is
    cut out: scipy's selection either way."""
    shape = [1, 1]
    shape[ax] = size
    h, n = size // 2, S.shape[ax]
    if h < 4 * n:
        return ndimage.median_filter(S, size=tuple(shape), mode="reflect")
    pad = [(0, 0), (0, 0)]
    pad[ax] = (h, h)
    out = ndimage.median_filter(np.pad(S, pad, mode="symmetric"), size=tuple(shape), mode="constant")
    return out[h:h + n] if ax == 0 else out[:, h:h + n]


@pytest.mark.parametrize("n", AXIS_LENGTHS)
def test_the_restatement_equals_scipy_bit_for_bit(n):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(100 + n)
    for other in (1, 6):
        for size in SIZES:
            S = quantised(rng, (n, other))                                         # the rows axis has length n ...
            want = scipy_median(ndimage, S, size, 0)
            got = R.median_filter(S, size, 1)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, other, size, "rows")
            S = np.ascontiguousarray(S.T)                                          # ... then the frames axis
            want = scipy_median(ndimage, S, size, 1)
            got = R.median_filter(S, size, 0)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, other, size, "frames")
    S = rng.standard_normal((2, n, 7)).astype(np.float32)                          # a batch, continuous values
    for axis, size3 in ((0, (1, 1, 5)), (1, (1, 5, 1))):
        assert np.array_equal(R.median_filter(S, 5, axis), ndimage.median_filter(S, size=size3, mode="reflect"))


def test_the_restatements_selection_rule_and_masks():
    rng = np.random.default_rng(7)
    S = quantised(rng, (9, 40))
    for axis in (0, 1):
        med = R.median_filter(S, 5, axis)
        n = S.shape[1 - axis]
        idx = R.reflect_index(np.arange(n)[:, None] + np.arange(-2, 3)[None, :], n)
        win = S[:, idx] if axis == 0 else np.moveaxis(S[idx, :], 2, 0)             # [rows, F, 5] / [F, rows, 5]
        v = med[..., None] if axis == 0 else med.T[..., None]
        assert ((win < v).sum(-1) <= 2).all() and ((win <= v).sum(-1) > 2).all()    # #(w < v) <= size / 2 < #(w <= v)
    assert np.array_equal(R.median_filter(S, 1, 0), S) and np.array_equal(R.median_filter(S, 1, 1), S)
    h, p = quantised(rng, (4, 50)), quantised(rng, (4, 50))
    zero = (h == 0) & (p == 0)
    assert zero.any() and not zero.all()
    for power in (0.5, 1.0, 2.0, 10.0):
        mh, mp = R.masks(h, p, power, 1.0)
        assert (mh[zero] == 0.5).all() and (mp[zero] == 0.5).all() and np.abs(mh + mp - 1.0).max() <= 1e-15
        mh, mp = R.masks(h, p, power, (2.5, 1.0))
        assert (mh[zero] == 0.0).all() and (mp[zero] == 0.0).all() and (mh + mp <= 1.0 + 1e-15).all()
    mh, mp = R.masks(h, p, np.inf, (1.0, 3.0))
    assert np.array_equal(mh, (h > p).astype(np.float64)) and np.array_equal(mp, (p > 3.0 * h).astype(np.float64))


def test_the_restatement_separates_sines_from_clicks():
    """The sanity bar of the GPU test on the restatement alone: the masks of the mixture, applied to each component's own STFT."""
    from tests import audio_ref as A
    sines, clicks = R.sines_and_clicks()
    mag = np.abs(A.stft(sines + clicks)).astype(np.float32)
    for k in (31, 17):
        mask_h, mask_p = R.hpss(mag, k, 2.0, True, 1.0)
        Xs, Xc = A.stft(sines), A.stft(clicks)
        in_h = float((np.abs(mask_h * Xs) ** 2).sum() / (np.abs(Xs) ** 2).sum())
        in_p = float((np.abs(mask_p * Xc) ** 2).sum() / (np.abs(Xc) ** 2).sum())
        print("kernel_size %d: %.4f of the sines' energy in the harmonic stem, %.4f of the clicks' in the percussive" % (k, in_h, in_p))
        assert in_h >= 0.9 and in_p >= 0.9
    h, p, r = R.hpss_audio(sines + clicks, residual=True)
    assert h.shape == p.shape == r.shape == sines.shape and np.abs(r).max() <= 1e-6   # unit margin: the masks sum to one
                                                                                      # (mag is |X| rounded to float32: 6e-8 of it)


def test_bad_arguments_are_refused_before_the_library_loads(monkeypatch, tmp_path):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "_lib", None)
    S, y = np.zeros((12, 30), np.float32), np.zeros(4096, np.float32)
    wav = tmp_path / "none.wav"                                                     # never opened: the arguments are checked first
    bad = [
        lambda: hpss.median_filter(S, 4, 0),                                      # even, out of range, no integer
        lambda: hpss.median_filter(S, 0, 0),
        lambda: hpss.median_filter(S, 129, 0),
        lambda: hpss.median_filter(S, -3, 1),
        lambda: hpss.median_filter(S, 5.0, 0),
        lambda: hpss.median_filter(S, True, 0),
        lambda: hpss.median_filter(S, 5, 2),                                      # no such axis
        lambda: hpss.median_filter(S, 5, -1),
        lambda: hpss.median_filter(S, 5, "time"),
        lambda: hpss.median_filter(S, 5, True),
        lambda: hpss.median_filter(S, 5, 0.0),
        lambda: hpss.median_filter(S[0], 5, 0),                                   # [F], [a, b, rows, F], no rows, too many rows
        lambda: hpss.median_filter(S[None, None], 5, 0),
        lambda: hpss.median_filter(np.zeros((0, 30), np.float32), 5, 0),
        lambda: hpss.median_filter(np.zeros((4097, 2), np.float32), 5, 1),
        lambda: hpss.median_filter(torch.zeros(2, (1 << 20) + 1), 5, 0),
        lambda: hpss.median_filter(S.astype(np.complex64), 5, 0),
        lambda: hpss.hpss(S, kernel_size=30),
        lambda: hpss.hpss(S, kernel_size=(31, 16)),
        lambda: hpss.hpss(S, kernel_size=(31, 17, 5)),
        lambda: hpss.hpss(S, kernel_size=129),
        lambda: hpss.hpss(S, kernel_size=31.0),
        lambda: hpss.hpss(S, margin=0.5),
        lambda: hpss.hpss(S, margin=(1.0, 0.99)),
        lambda: hpss.hpss(S, margin=(1.0,)),
        lambda: hpss.hpss(S, margin=float("inf")),
        lambda: hpss.hpss(S, margin=float("nan")),
        lambda: hpss.hpss(S, margin="1"),
        lambda: hpss.hpss(S, power=0),
        lambda: hpss.hpss(S, power=-2.0),
        lambda: hpss.hpss(S, power=float("nan")),
        lambda: hpss.hpss(S, power=None),
        lambda: hpss.hpss(S, mask=1),
        lambda: hpss.hpss(S[0]),
        lambda: hpss.hpss(np.zeros((4097, 2), np.complex64)),
        lambda: hpss.hpss_audio(y[:1024]),                                        # n <= 1024
        lambda: hpss.hpss_audio(np.zeros((2, 3, 4096), np.float32)),
        lambda: hpss.hpss_audio(y.astype(np.complex64)),
        lambda: hpss.hpss_audio(y, kernel_size=32),
        lambda: hpss.hpss_audio(y, margin=0.0),
        lambda: hpss.hpss_audio(y, power=0.0),
        lambda: hpss.hpss_audio(y, residual="yes"),
        lambda: hpss.separate_wav_hpss(str(wav), out_rate="native"),
        lambda: hpss.separate_wav_hpss(str(wav), out_rate=10),
        lambda: hpss.separate_wav_hpss(str(wav), kernel_size=8),
        lambda: hpss.separate_wav_hpss(str(wav), margin=0.5),
        lambda: hpss.separate_wav_hpss(str(wav), power=-1.0),
        lambda: hpss.separate_wav_hpss(str(wav), n_iter=3),                       # no argument of hpss_audio
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % k)


def test_the_two_entries_are_declared_exported_and_bound(lib, repo_root):
    text = open(os.path.join(repo_root, "include", "glowk.h")).read()
    assert re.search(r"\bint glowk_median_filter\(const float\* s_dev, int nsig, int rows, int frames, int size, int axis, float\* out_dev, "
                     r"void\* stream\);", text)
    assert re.search(r"\bint glowk_hpss_mask\(const float\* harm_dev, const float\* perc_dev, const float\* s_dev, size_t n, float power, "
                     r"float margin_h,\s+float margin_p, float\* out_h_dev, float\* out_p_dev, void\* stream\);", text)
    for name, nargs in (("glowk_median_filter", 8), ("glowk_hpss_mask", 10)):
        assert len(_lib.SYMBOLS[name][1]) == nargs and getattr(lib, name) is not None
    assert _lib.SYMBOLS["glowk_hpss_mask"][1][3] is ctypes.c_size_t and _lib.SYMBOLS["glowk_hpss_mask"][1][4:7] == [ctypes.c_float] * 3
    version = int(re.search(r"#define GLOWK_VERSION (\d+)", text).group(1))
    assert lib.glowk_version() == version >= 500                                  # (the version that introduced them)


def _err(lib):
    return lib.glowk_last_error().decode()


def test_the_entries_refuse_bad_ranges_before_touching_a_device(lib):
    z, a, b = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)   # never dereferenced: refused first
    for nsig, rows, F, size, axis, word in [(-1, 12, 30, 5, 0, "nsig"), (65536, 12, 30, 5, 0, "nsig"), (1, 0, 30, 5, 0, "rows"),
                                            (1, 4097, 30, 5, 0, "rows"), (1, 12, 0, 5, 0, "frames"), (1, 12, (1 << 20) + 1, 5, 0, "frames"),
                                            (1, 2048, 1 << 20, 5, 0, "2^31"), (65535, 4096, 9, 5, 1, "2^31"), (1, 12, 30, 0, 0, "size"),
                                            (1, 12, 30, 4, 0, "size"), (1, 12, 30, 129, 0, "size"), (1, 12, 30, -1, 1, "size"),
                                            (1, 12, 30, 5, 2, "axis"), (1, 12, 30, 5, -1, "axis")]:
        assert lib.glowk_median_filter(a, nsig, rows, F, size, axis, b, z) == _lib.ERR and word in _err(lib), (nsig, rows, F, size, axis)
    for axis in (0, 1):
        assert lib.glowk_median_filter(z, 0, 12, 30, 5, axis, z, z) == _lib.OK     # no signals: a successful no-op ...
        assert lib.glowk_median_filter(z, 0, 12, 30, 4, axis, z, z) == _lib.ERR    # ... of valid arguments only
        assert lib.glowk_median_filter(z, 1, 12, 30, 5, axis, b, z) == _lib.ERR and "null" in _err(lib)
        assert lib.glowk_median_filter(a, 1, 12, 30, 5, axis, z, z) == _lib.ERR and "null" in _err(lib)
        assert lib.glowk_median_filter(a, 1, 12, 30, 5, axis, a, z) == _lib.ERR and "out_dev" in _err(lib)   # in place
        assert lib.glowk_median_filter(a, 1, 12, 30, 5, axis, ctypes.c_void_p((1 << 20) + 4 * 359), z) == _lib.ERR and "out_dev" in _err(lib)
    inf, nan = float("inf"), float("nan")
    for power, mh, mp, word in [(0.0, 1.0, 1.0, "power"), (-1.0, 1.0, 1.0, "power"), (nan, 1.0, 1.0, "power"), (-inf, 1.0, 1.0, "power"),
                                (2.0, 0.5, 1.0, "margin"), (2.0, 1.0, 0.999, "margin"), (2.0, inf, 1.0, "margin"), (2.0, 1.0, inf, "margin"),
                                (2.0, nan, 1.0, "margin"), (2.0, 1.0, nan, "margin"), (2.0, -1.0, 1.0, "margin")]:
        assert lib.glowk_hpss_mask(a, a, z, 16, power, mh, mp, b, b, z) == _lib.ERR and word in _err(lib), (power, mh, mp)
    assert lib.glowk_hpss_mask(a, a, z, (1 << 40) + 1, 2.0, 1.0, 1.0, b, b, z) == _lib.ERR and "2^40" in _err(lib)
    assert lib.glowk_hpss_mask(z, z, z, 0, 2.0, 1.0, 1.0, z, z, z) == _lib.OK
    assert lib.glowk_hpss_mask(z, z, z, 0, inf, 1.0, 3.0, z, z, z) == _lib.OK      # the hard mask is a valid power
    assert lib.glowk_hpss_mask(z, z, z, 0, 0.0, 1.0, 1.0, z, z, z) == _lib.ERR
    for args in [(z, a, z, 16, 2.0, 1.0, 1.0, b, ctypes.c_void_p(1 << 29), z), (a, z, z, 16, 2.0, 1.0, 1.0, b, ctypes.c_void_p(1 << 29), z),
                 (a, a, z, 16, 2.0, 1.0, 1.0, z, b, z), (a, a, z, 16, 2.0, 1.0, 1.0, b, z, z)]:
        assert lib.glowk_hpss_mask(*args) == _lib.ERR and "null" in _err(lib)
    assert lib.glowk_hpss_mask(a, a, z, 16, 2.0, 1.0, 1.0, b, b, z) == _lib.ERR and "distinct" in _err(lib)
    # a host pointer is refused (where there is no device at all, every pointer is one)
    host = np.zeros(12 * 30, np.float32)
    hp, out = host.ctypes.data_as(ctypes.c_void_p), np.zeros(12 * 30, np.float32)
    assert lib.glowk_median_filter(hp, 1, 12, 30, 5, 0, out.ctypes.data_as(ctypes.c_void_p), z) == _lib.ERR and "device memory" in _err(lib)
    assert lib.glowk_hpss_mask(hp, hp, z, 360, 2.0, 1.0, 1.0, out.ctypes.data_as(ctypes.c_void_p), hp, z) == _lib.ERR
