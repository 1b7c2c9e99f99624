"""Oracle separation systems without a GPU: the fp64 NumPy restatement (tests/oracle_systems_ref.py) against the reference's own
outputs stored in tests/golden/real_oracle.npz and against scipy.signal, and the errors of audiosourcesep_amd/oracle_systems.py
(all raised before any device call).

Measured when the fixture was made: the restatement reproduces every stored estimate to <= 2.9e-8 relative L2 (the fixture is
float32; the reference and the restatement are fp64; the bound is 1e-6), its stft / istft match scipy.signal to <= 2e-15 (bound
1e-12), and the mel variants bit for bit.  A per-frequency trace in MWF moves the estimates by 28 % relative; without the
complex64 gain the restatement's MWF would be 1.1e-4 away."""
import os

import numpy as np
import pytest

from audiosourcesep_amd import _lib, oracle_systems as O
from tests import oracle_systems_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_oracle.npz")
MEL_TILES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_mel_tiles.npz")
TOL_REL = 1e-6
LEAD, LEN = 8, 16000
PANS = [(0.75, 0.5), (0.25, 0.875)]
DELAYS = [(0, 3), (5, 0)]
IBM_CASES = [(1, 0.5), (2, 0.3)]


def golden():
    return np.load(GOLDEN)


def mono(z):
    """(mixture (16000, 1), sources (2, 16000, 1)) float64, as tests/golden/make_oracle_golden.py built them."""
    s = (z["gt"][:, LEAD:].astype(np.float64) / 32768.0)[:, :, None]
    return s.sum(0), s


def stereo(z):
    x = z["gt"].astype(np.float64) / 32768.0
    s = np.empty((2, LEN, 2))
    for j in range(2):
        for c in range(2):
            d = DELAYS[j][c]
            s[j, :, c] = PANS[j][c] * x[j, LEAD - d:LEAD - d + LEN]
    return s.sum(0), s


def mel_inputs():
    t = np.load(MEL_TILES)
    off = np.float32(100.0)
    return t["mixed"][:1] + off, np.stack([t["gt1"][:1] + off, t["gt2"][:1] + off])


def rel(got, want):
    """Per-source relative L2 error, the largest."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return max(np.linalg.norm(got[j] - want[j]) / np.linalg.norm(want[j]) for j in range(len(want)))


@pytest.mark.parametrize("alpha,theta", IBM_CASES)
def test_restatement_ibm_reproduces_the_reference(alpha, theta):
    z = golden()
    mix, src = mono(z)
    assert rel(R.IBM(mix, src, alpha=alpha, theta=theta), z["IBM_a%g_t%g" % (alpha, theta)]) <= TOL_REL
    assert float(np.min(z["margin"])) > 1e-4


def test_restatement_irm_and_mwf_reproduce_the_reference():
    z = golden()
    mix, src = stereo(z)
    assert rel(R.IRM(mix, src), z["IRM"]) <= TOL_REL
    assert rel(R.MWF(mix, src), z["MWF"]) <= TOL_REL


def test_fixture_pins_the_trace_quirk():
    z = golden()
    mix, src = stereo(z)
    assert rel(R.MWF(mix, src, per_frequency_trace=True), z["MWF"]) > 1e-2


def test_restatement_mel_variants_are_bitwise():
    z = golden()
    mix, src = mel_inputs()
    for name, fn in (("IBM_melspec", R.IBM_melspec), ("IRM_melspec", R.IRM_melspec)):
        got = fn(mix, src)
        assert got.dtype == np.float32 and np.array_equal(got, z[name]), name


def test_restatement_stft_matches_scipy():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(7)
    for n in (2048, 2049, 5 * 1024, 16000):
        x = rng.standard_normal((3, n))
        X = R.stft(x)
        assert X.shape == (3, 1025, R.nframes(n)) == signal.stft(x, nperseg=2048)[-1].shape
        assert np.max(np.abs(X - signal.stft(x, nperseg=2048)[-1])) <= 1e-12
        assert np.max(np.abs(R.istft(X, n) - signal.istft(X)[1][..., :n])) <= 1e-12
        assert np.max(np.abs(R.istft(X, n) - x)) <= 1e-12


@pytest.fixture
def no_device(monkeypatch):
    """Every ValueError must come before the library is loaded or a device is touched."""
    def refuse(*a, **k):
        raise AssertionError("device path reached")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(O, "_device", refuse)


def test_value_errors_before_any_device_call(no_device):
    rng = np.random.default_rng(0)
    mix = rng.standard_normal((4096, 2))
    src = rng.standard_normal((2, 4096, 2))
    for fn in (O.IBM, O.IRM, O.MWF):
        with pytest.raises(ValueError, match="2048"):
            fn(mix[:2047], src[:, :2047])
        with pytest.raises(ValueError, match="do not match"):
            fn(mix, src[:, :4000])
        with pytest.raises(ValueError, match="do not match"):
            fn(mix[:, :1], src)
        with pytest.raises(ValueError, match="nsampl, nchan"):
            fn(mix[:, 0], src)
        with pytest.raises(ValueError, match="nsrc, nsampl, nchan"):
            fn(mix, src[0])
        with pytest.raises(ValueError, match="real"):
            fn(mix.astype(np.complex64), src)
    with pytest.raises(ValueError, match="stereo"):
        O.MWF(mix[:, :1], src[:, :, :1])
    with pytest.raises(ValueError, match="stereo"):
        O.MWF(np.zeros((4096, 3)), np.zeros((2, 4096, 3)))
    with pytest.raises(ValueError, match="16 sources"):
        O.MWF(mix, np.zeros((17, 4096, 2)))
    with pytest.raises(ValueError, match="alpha"):
        O.IBM(mix, src, alpha=np.inf)
    with pytest.raises(ValueError, match="theta"):
        O.IBM(mix, src, theta=np.nan)
    t = rng.standard_normal((2, 96, 64)).astype(np.float32)
    s = rng.standard_normal((2, 2, 96, 64)).astype(np.float32)
    for fn in (O.IBM_melspec, O.IRM_melspec):
        with pytest.raises(ValueError, match="do not match"):
            fn(t, s[:, :, :95])
        with pytest.raises(ValueError, match="nsample, f, t"):
            fn(t[0], s)
        with pytest.raises(ValueError, match="nsrc, nsample, f, t"):
            fn(t, s[0])
        with pytest.raises(ValueError, match="half"):
            fn(t, s.astype(np.float16))
    with pytest.raises(ValueError, match="n >= 1"):
        O.stft(np.zeros((2, 0)))
    with pytest.raises(ValueError, match="complex"):
        O.istft(np.zeros((1025, 4)), 100)
    with pytest.raises(ValueError, match="length"):
        O.istft(np.zeros((1025, 4), np.complex64), 3 * 1024 + 1)


def test_empty_calls_succeed_with_null_pointers_and_no_device():
    """An empty tensor has no storage (torch gives it a null data pointer): length = 0, zero signals and n = 0, all inside the
    ranges of include/glowk.h, return 0 before any pointer or device is looked at; the same sizes out of range are refused."""
    lib = _lib.load()
    z = None
    assert lib.glowk_sp_istft(z, 3, 34, 0, z, z) == 0
    assert lib.glowk_sp_istft(z, 0, 34, 100, z, z) == 0
    assert lib.glowk_sp_stft(z, 0, 5000, z, z) == 0
    assert lib.glowk_oracle_mel(z, z, 7, 0, 0, 1, 0.5, z, z) == 0
    assert lib.glowk_sp_istft(z, 3, 34, -1, z, z) != 0 and b"length" in lib.glowk_last_error()
    assert lib.glowk_sp_istft(z, 3, 34, 100, z, z) != 0 and b"null" in lib.glowk_last_error()
    assert lib.glowk_sp_stft(z, 1, 5000, z, z) != 0 and b"null" in lib.glowk_last_error()
    assert lib.glowk_oracle_mel(z, z, 7, 1, 0, 1, 0.5, z, z) != 0 and b"null" in lib.glowk_last_error()


def test_frame_count():
    assert [O.nframes(n) for n in (1, 1024, 1025, 2048, 2049, 16000)] == [2, 2, 3, 3, 4, 17]
    assert all(O.nframes(n) == R.nframes(n) for n in range(1, 5000, 37))
