"""The whole-signal path without a GPU: the restatement of tests/longform_ref.py against itself (round trip, window, cut then
stitch), the Python argument checks (refused with ValueError before the library is loaded), and the boundary of the three C
entries: declared, exported, bound, and their range checks, which run before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, audio
from tests import longform_ref as R

# (F, hop) at width 64 and the tile counts they give: one short tile, one full tile, a one-frame tail, three and four tiles,
# a hop that is no divisor of the width, hop 1, disjoint tiles
CASES = [(5, 32, 1), (64, 32, 1), (65, 32, 2), (100, 32, 3), (138, 32, 4), (138, 48, 3), (70, 1, 7), (138, 64, 3)]


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def test_round_trip_of_a_signal_that_is_no_hop_multiple():
    rng = np.random.default_rng(0)
    y = rng.standard_normal(70001)
    back = R.round_trip(y)
    err = float(np.abs(back - y).max() / np.abs(y).max())
    print("zero-pad, STFT, iSTFT, trim at n = 70001: %.2e of max|y|" % err)
    assert back.shape == y.shape and err <= 1e-12
    assert R.pad_hop(y).shape == (70144,) and not R.pad_hop(y)[70001:].any()
    assert R.mel_frames(y).shape == (96, 138)


@pytest.mark.parametrize("width", [2, 32, 64, 128])
def test_the_windows_halves_sum_to_one(width):
    # sin^2 + cos^2 in fp64: each term carries the sine's rounding, the argument's and the square's (<= 3 ulp), the sum one more:
    # 7 x 2^-53 = 7.8e-16, rounded up
    w = R.window(width)
    assert (w > 0).all() and np.abs(w[:width // 2] + w[width // 2:] - 1.0).max() <= 1e-15


@pytest.mark.parametrize("F,hop,N", CASES)
def test_cut_then_stitch_returns_the_frames(F, hop, N):
    rng = np.random.default_rng(F * 100 + hop)
    L = rng.uniform(-100.0, 20.0, (96, F))
    assert R.tile_count(F, 64, hop) == N == audio.tile_count(F, 64, hop)
    tiles = R.cut(L, 64, hop)
    assert tiles.shape == (N, 96, 64)
    assert (tiles.reshape(N, 96, -1)[-1][:, F - (N - 1) * hop:] == -100.0).all()          # the pad of the last tile
    back = R.stitch(tiles, F, hop)
    err = float(np.abs(back - L).max())
    print("F = %d, hop = %d, N = %d: cut then stitch %.2e dB" % (F, hop, N, err))
    assert err <= 1e-12
    floored = R.cut(L, 64, hop, top_db=80.0)
    assert all(floored[k].min() >= max(-100.0, tiles[k].max() - 80.0) for k in range(N))


class FakeFlow:
    def __init__(self, *shape):
        self.event_shape = shape


def test_bad_arguments_are_refused_before_the_library_loads(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(_lib, "_lib", None)
    y = np.zeros(4096, np.float32)
    flows, sig = [FakeFlow(96, 64, 1), FakeFlow(96, 64, 1)], [1.0]
    bad = [
        lambda: audio.mel_frames(y[:1024]),                                      # n <= 1024
        lambda: audio.mel_frames(np.zeros((2, 3, 4096), np.float32)),
        lambda: audio.mel_frames(np.zeros(4096, np.complex64)),
        lambda: audio.separate_long(y[:1024], flows, sig),
        lambda: audio.separate_long(np.zeros((3, 4096), np.float32), flows, sig),       # neither mono nor stereo
        lambda: audio.separate_long(np.zeros((1, 4096), np.float32), flows, sig),
        lambda: audio.separate_long(y, flows, sig, tile_hop=0),                  # tile_hop outside [1, W]
        lambda: audio.separate_long(y, flows, sig, tile_hop=65),
        lambda: audio.separate_long(y, flows, sig, tile_hop=32.0),
        lambda: audio.separate_long(y, [FakeFlow(64, 64, 1)] * 2, sig),          # a flow whose height is not 96
        lambda: audio.separate_long(y, [FakeFlow(96, 64, 1), FakeFlow(96, 32, 1)], sig),
        lambda: audio.separate_long(y, [FakeFlow(96, 64, 2)] * 2, sig),
        lambda: audio.separate_long(y, [FakeFlow(96, 256, 1)] * 2, sig),
        lambda: audio.separate_long(y, [object(), object()], sig),
        lambda: audio.separate_long(y, flows[:1], sig),                          # fewer than 2, more than 16 flows
        lambda: audio.separate_long(y, flows * 9, sig[:1]),
        lambda: audio.separate_long(y, flows, sig, em_iter=-1),
        lambda: audio.frame_tiles(torch.zeros(1, 95, 10)),
        lambda: audio.frame_tiles(torch.zeros(1, 96, 10), width=129),
        lambda: audio.frame_tiles(torch.zeros(1, 96, 10), width=1),
        lambda: audio.frame_tiles(torch.zeros(1, 96, 10), tile_hop=65),
        lambda: audio.frame_tiles(torch.zeros(1, 96, 10), tile_hop=0),
        lambda: audio.frame_tiles(torch.zeros(1, 96, 10), top_db=float("nan")),
        lambda: audio.stitch_tiles(torch.zeros(1, 2, 96, 64, 1), 97),            # (N - 1) hop + width = 96 frames at the most
        lambda: audio.stitch_tiles(torch.zeros(1, 2, 96, 64, 1), 0),
        lambda: audio.stitch_tiles(torch.zeros(1, 2, 96, 64, 1), 96, tile_hop=65),
        lambda: audio.stitch_tiles(torch.zeros(2, 96, 64), 64),
        lambda: audio.invert_frames(torch.zeros(2, 96, 8), torch.zeros(1025, 9, dtype=torch.complex64), 100),
        lambda: audio.invert_frames(torch.zeros(2, 96, 8), torch.zeros(1025, 8, dtype=torch.complex64), 7 * 512 + 1),
        lambda: audio.invert_frames(torch.zeros(1, 96, 8), torch.zeros(1025, 8, dtype=torch.complex64), 100, wiener=True),
        lambda: audio.invert_frames(torch.zeros(2, 96, 8), torch.zeros(1025, 8), 100),
        lambda: audio.mask_istft_long(torch.zeros(2, 1025, 3), torch.zeros(1025, 3, dtype=torch.complex64), 100),
        lambda: audio.mask_istft_long(torch.zeros(2, 1025, 8), torch.zeros(3, 1025, 8, dtype=torch.complex64), 100),
        lambda: audio.mask_istft_long(torch.zeros(2, 1025, 8), torch.zeros(2, 1025, 8, dtype=torch.complex64), 100, em_iter=1001),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % k)


def test_the_three_entries_are_declared_exported_and_bound(lib, repo_root):
    text = open(os.path.join(repo_root, "include", "glowk.h")).read()
    assert re.search(r"\bint glowk_mel_frames\(const float\* audio_dev, int nsig, int64_t n_samples, float\* mel_db_dev, float\* stft_dev, "
                     r"void\* stream\);", text)
    assert re.search(r"\bint glowk_tile_cut\(const float\* frames_dev, int nsig, int frames, int width, int hop, float top_db, "
                     r"float\* tiles_dev, void\* stream\);", text)
    assert re.search(r"\bint glowk_tile_stitch\(const float\* tiles_dev, int nsig, int N, int width, int hop, int frames, "
                     r"float\* frames_dev, void\* stream\);", text)
    for name, nargs in (("glowk_mel_frames", 6), ("glowk_tile_cut", 8), ("glowk_tile_stitch", 8)):
        assert len(_lib.SYMBOLS[name][1]) == nargs and getattr(lib, name) is not None
    assert _lib.SYMBOLS["glowk_mel_frames"][1][2] is ctypes.c_int64 and _lib.SYMBOLS["glowk_tile_cut"][1][5] is ctypes.c_float
    assert lib.glowk_version() == int(re.search(r"#define GLOWK_VERSION (\d+)", text).group(1))


def _err(lib):
    return lib.glowk_last_error().decode()


def test_the_entries_refuse_bad_ranges_before_touching_a_device(lib):
    z = ctypes.c_void_p(0)
    top = (1 << 20) - 1
    for nsig, n, word in [(-1, 1536, "nsig"), ((1 << 20) + 1, 1536, "nsig"), (1, 1024, "n_samples"), (1, 1537, "n_samples"),
                          (1, (top + 1) * 512, "n_samples"), (1, -512, "n_samples"), (1 << 20, top * 512, "one launch")]:
        assert lib.glowk_mel_frames(z, nsig, n, z, z, z) == _lib.ERR and word in _err(lib), (nsig, n)
    assert lib.glowk_mel_frames(z, 0, 1536, z, z, z) == 0                        # no signals: a successful no-op ...
    assert lib.glowk_mel_frames(z, 0, 1000, z, z, z) == _lib.ERR                 # ... of valid arguments only
    assert lib.glowk_mel_frames(z, 1, 1536, z, z, z) == _lib.ERR and "null" in _err(lib)
    for nsig, F, width, hop, top_db, word in [(-1, 10, 64, 32, 80.0, "nsig"), (1, 0, 64, 32, 80.0, "frames"),
                                              (1, (1 << 20) + 1, 64, 32, 80.0, "frames"), (1, 10, 1, 1, 80.0, "width"),
                                              (1, 10, 129, 32, 80.0, "width"), (1, 10, 64, 0, 80.0, "hop"), (1, 10, 64, 65, 80.0, "hop"),
                                              (1, 10, 64, 32, float("inf"), "top_db"), (1 << 20, 1 << 20, 64, 1, 80.0, "one launch")]:
        assert lib.glowk_tile_cut(z, nsig, F, width, hop, top_db, z, z) == _lib.ERR and word in _err(lib), (nsig, F, width, hop)
    assert lib.glowk_tile_cut(z, 0, 10, 64, 32, 80.0, z, z) == 0
    assert lib.glowk_tile_cut(z, 0, 10, 64, 65, 80.0, z, z) == _lib.ERR
    assert lib.glowk_tile_cut(z, 1, 10, 64, 32, 80.0, z, z) == _lib.ERR and "null" in _err(lib)
    for nsig, N, width, hop, F, word in [(-1, 2, 64, 32, 96, "nsig"), (1, 0, 64, 32, 1, "N must"), (1, (1 << 20) + 1, 64, 32, 96, "N must"),
                                         (1, 2, 130, 32, 96, "width"), (1, 2, 64, 65, 96, "hop"), (1, 2, 64, 32, 97, "frames"),
                                         (1, 2, 64, 32, 0, "frames"), (1, 1 << 20, 64, 32, (1 << 20) + 1, "frames")]:
        assert lib.glowk_tile_stitch(z, nsig, N, width, hop, F, z, z) == _lib.ERR and word in _err(lib), (nsig, N, width, hop, F)
    assert lib.glowk_tile_stitch(z, 0, 2, 64, 32, 96, z, z) == 0
    assert lib.glowk_tile_stitch(z, 0, 2, 64, 32, 97, z, z) == _lib.ERR
    assert lib.glowk_tile_stitch(z, 1, 2, 64, 32, 96, z, z) == _lib.ERR and "null" in _err(lib)
