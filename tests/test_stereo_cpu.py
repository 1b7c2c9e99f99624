"""Stereo separation without a GPU: the fp64 restatement of the EM Wiener filter (tests/stereo_ref.py) against the properties that
make its inputs meaningful, and the boundary of ``glowk_mwf_em``: declared, exported, bound, version 480, and the argument checks
of the C call and of the Python wrappers that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as graft
from audiosourcesep_amd import _lib, audio
from tests import stereo_ref as R


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


@pytest.mark.parametrize("S,T", [(2, 7), (2, 64), (3, 7), (3, 64)])
def test_the_reference_against_itself(S, T):
    pr = R.problem(S, T, bins=6, seed=100 * S + T)
    x, v0 = pr["x"], pr["v"]
    v, Rm = v0, R.start(v0)
    L = [R.log_likelihood(x, v, Rm)]
    for _ in range(10):
        v, Rm = R.em_step(x, v, Rm)
        L.append(R.log_likelihood(x, v, Rm))
    assert all(b >= a for a, b in zip(L, L[1:])), L                              # EM never lowers the likelihood
    Y0, (Y10, v10, R10) = R.multichannel_wiener(x, v0, 0), R.multichannel_wiener(x, v0, 10, return_model=True)
    assert np.array_equal(v10, v) and np.array_equal(R10, Rm)
    xmax = np.abs(x).max()
    for Y in (Y0, Y10):
        assert Y.shape == (S, 1, 2, 6, T)
        assert np.abs(Y.sum(0) - x).max() <= 1e-9 * xmax                         # the filters sum to I - eps Cx^-1
    assert np.abs(Y0 - R.single_channel_mask(x, v0)).max() <= 1e-12 * xmax       # R = I: the per-channel mask, to fp64 rounding
    assert np.allclose(R10, np.conj(np.swapaxes(R10, -1, -2))) and (v10 >= 0).all()
    gain = R.sdr(pr["sources"], Y10) - R.sdr(pr["sources"], Y0)
    print("S = %d, T = %d: SDR %.2f dB at 0 iterations, %+.2f dB after 10" % (S, T, R.sdr(pr["sources"], Y0), gain))
    if (S, T) == (2, 64):
        assert gain >= 1.0


def test_the_generator_draws_what_it_says():
    pr = R.problem(2, 4000, bins=2, seed=3, cond=10.0)
    s, vt, Rt = pr["sources"], pr["v_true"], pr["R_true"]
    assert np.allclose(np.trace(Rt, axis1=-2, axis2=-1).real, 2.0) and np.allclose(np.linalg.cond(Rt), 10.0)
    sv = np.moveaxis(s, 2, -1)[..., None] / np.sqrt(vt)[..., None, None]          # unit-PSD sources [S, P, B, T, 2, 1]
    emp = (sv @ np.conj(np.swapaxes(sv, -1, -2))).mean(3)
    assert np.abs(emp - Rt).max() <= 0.15                                        # 4000 draws: 6 sigma of 2 / sqrt(4000)
    assert np.array_equal(pr["x"], pr["x"].astype(np.complex64)) and np.array_equal(pr["v"], pr["v"].astype(np.float32))


def test_mwf_em_is_declared_exported_and_bound(lib, repo_root):
    text = open(os.path.join(repo_root, "include", "glowk.h")).read()
    assert re.search(r"\bint glowk_mwf_em\(const float\* x_dev, float\* v_dev, int nsrc, int nprob, int frames, int n_iter,", text)
    assert "glowk_mwf_em" in _lib.SYMBOLS and lib.glowk_mwf_em is not None
    assert len(_lib.SYMBOLS["glowk_mwf_em"][1]) == 9
    assert lib.glowk_version() >= 480                                           # (the version that introduced it)


def test_mwf_em_refuses_bad_ranges_before_touching_a_device(lib):
    z = ctypes.c_void_p(0)
    for nsrc, nprob, frames, n_iter, word in [(0, 1, 8, 1, "nsrc"), (17, 1, 8, 1, "nsrc"), (2, -1, 8, 1, "nprob"),
                                              (2, (1 << 20) + 1, 8, 1, "nprob"), (2, 1, 0, 1, "frames"), (2, 1, (1 << 20) + 1, 1, "frames"),
                                              (2, 1, 8, -1, "n_iter"), (2, 1, 8, 1001, "n_iter")]:
        assert lib.glowk_mwf_em(z, z, nsrc, nprob, frames, n_iter, z, z, z) == _lib.ERR
        assert word in lib.glowk_last_error().decode()
    assert lib.glowk_mwf_em(z, z, 2, 0, 8, 1, z, z, z) == 0                      # no problems: a successful no-op
    assert lib.glowk_mwf_em(z, z, 17, 0, 8, 1, z, z, z) == _lib.ERR              # ... of valid arguments only
    assert lib.glowk_mwf_em(z, z, 2, 1, 8, 1, z, z, z) == _lib.ERR and "null" in lib.glowk_last_error().decode()


def test_python_argument_checks_need_no_device(tmp_path):
    p, X = torch.zeros(2, 1, 1025, 8), torch.zeros(1, 2, 1025, 8, dtype=torch.complex64)
    bad = [dict(powers=p[0], stft_mixture=X), dict(powers=p[:, :, :1024], stft_mixture=X), dict(powers=torch.zeros(17, 1, 1025, 8), stft_mixture=X),
           dict(powers=p, stft_mixture=X[:, :1]), dict(powers=p, stft_mixture=X.real), dict(powers=X, stft_mixture=X),
           dict(powers=p, stft_mixture=X[..., :7]), dict(powers=p, stft_mixture=X, n_iter=-1), dict(powers=p, stft_mixture=X, n_iter=1001),
           dict(powers=p, stft_mixture=X, n_iter=1.5), dict(powers=p, stft_mixture=X, n_iter=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            audio.multichannel_wiener(**kw)
    with pytest.raises(ValueError, match=r"\[N, 2, 1025, F\]"):
        audio.multichannel_wiener(p, X[0])
    for Y in (X[0, 0, :, :3], X[0, 0, :1000], X[0, 0].real, X[0, 0, 0]):
        with pytest.raises(ValueError, match=r"1025, F\]"):
            audio.istft(Y)
    stereo = np.zeros((2, 2 * audio.EXTRACT), np.float32)
    for kw in (dict(method="tile"), dict(em_iter=-1), dict(em_iter=1001), dict(em_iter=2.0)):
        with pytest.raises(ValueError):
            audio.separate_stereo(stereo, [None, None], [1.0], **kw)
    with pytest.raises(ValueError, match="2..16"):
        audio.separate_stereo(stereo, [None], [1.0])
    for mix in (stereo[0], np.zeros((3, 100), np.float32), stereo.T):
        with pytest.raises(ValueError, match=r"\[2, n\]"):
            audio.separate_stereo(mix, [None, None], [1.0])
    mono = tmp_path / "mono.wav"
    audio.save_audio(mono, np.zeros(1000, np.float32), 8000)
    with pytest.raises(ValueError, match="separate_wav_sources"):
        audio.separate_wav_stereo(str(mono), [None, None], [1.0])
    with pytest.raises(ValueError, match="out_rate"):
        audio.separate_wav_stereo(str(mono), [None, None], [1.0], out_rate="native")
