"""Oracle separation systems on the GPU (csrc/glowk_oracle.h through audiosourcesep_amd/oracle_systems.py) against the reference's
own outputs (tests/golden/real_oracle.npz) and the fp64 restatement of tests/oracle_systems_ref.py.

Bounds and their reasons (measured on an MI355X):
* stft / istft against the fp64 restatement and the round trip, per signal relative L2: 1e-5 (measured <= 9.6e-7: fp32 sums of
  2048 terms);
* IBM and IRM, per source relative L2: 1e-4 (measured <= 1.2e-6 against the fixture, the restatement and on three sources);
* MWF on well-conditioned synthetic sources: 1e-4 (measured 1.8e-6 from float64 input, 2.2e-5 from float32 input);
* MWF on the fixture: 1e-3 (measured 3.5e-4).  Its sources are pans with 3- and 5-sample delays, so each spatial covariance is
  within ~1e-3 of rank one and MWF amplifies any rounding of the spectra by the inverse of its smallest eigenvalue: on the CPU,
  rounding the reference's own fp64 spectra to complex64 moves its estimates by 1.5e-4, and an error of 1e-9 of the largest bin
  by 1.8e-4.  The kernels after the STFT are checked on their own against the restatement fed the GPU's spectra: 1e-4
  (measured 5.5e-7);
* IBM mask bits: identical to fp64 wherever the fp64 ratio is more than a relative 1e-4 from theta (no bit differed at all);
* the mel variants and repeated calls: bitwise."""
import numpy as np
import pytest
import torch

from audiosourcesep_amd import bsseval, oracle_systems as O
from tests import oracle_systems_ref as R
from tests.test_oracle_systems_cpu import IBM_CASES, golden, mel_inputs, mono, rel, stereo

pytestmark = pytest.mark.gpu
TOL_SPEC = 1e-5
TOL_SYS = 1e-4
TOL_MWF_FIXTURE = 1e-3


def synthetic(nsrc, n, nchan, seed):
    """Sources: per channel, filtered (a shared signal + an independent one of the same power), so that every source's spatial
    covariance is well conditioned (MWF amplifies spectral rounding by the inverse of its smallest eigenvalue)."""
    rng = np.random.default_rng(seed)
    src = np.empty((nsrc, n, nchan))
    for j in range(nsrc):
        base = rng.standard_normal(n)
        for c in range(nchan):
            src[j, :, c] = np.convolve(base + rng.standard_normal(n), rng.standard_normal(8 + 4 * j) / (2 + j), mode="same")
    return src.sum(0), src


def sig_rel(got, want):
    got, want = np.asarray(got).reshape(-1, np.shape(want)[-1]), np.asarray(want).reshape(-1, np.shape(want)[-1])
    return max(np.linalg.norm(g - w) / np.linalg.norm(w) for g, w in zip(got, want))


@pytest.mark.parametrize("n", [2048, 2049, 16000, 5 * 1024, 32000, 33 * 1024])   # the last two: a second tile of frames
def test_stft_istft_against_the_restatement(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n)).astype(np.float32)
    X = O.stft(x)
    assert X.dtype == np.complex64 and X.shape == (3, 1025, R.nframes(n))
    W = R.stft(x)
    assert max(np.linalg.norm(X[i] - W[i]) / np.linalg.norm(W[i]) for i in range(3)) <= TOL_SPEC
    y = O.istft(W.astype(np.complex64), n)
    assert y.dtype == np.float32 and y.shape == (3, n)
    assert sig_rel(y, R.istft(W, n)) <= TOL_SPEC
    assert sig_rel(O.istft(X, n), x) <= TOL_SPEC                # round trip
    assert sig_rel(O.istft(X, n - 5), x[:, :n - 5]) <= TOL_SPEC


@pytest.mark.parametrize("alpha,theta", IBM_CASES)
def test_ibm_against_the_fixture(alpha, theta):
    z = golden()
    mix, src = mono(z)
    got = O.IBM(mix, src, alpha=alpha, theta=theta)
    assert got.dtype == np.float64 and got.shape == src.shape
    assert rel(got, z["IBM_a%g_t%g" % (alpha, theta)]) <= TOL_SYS
    assert rel(got, R.IBM(mix, src, alpha=alpha, theta=theta)) <= TOL_SYS


def test_irm_and_mwf_against_the_fixture():
    z = golden()
    mix, src = stereo(z)
    got = O.IRM(mix, src)
    assert got.shape == src.shape
    assert rel(got, z["IRM"]) <= TOL_SYS
    assert rel(got, R.IRM(mix, src)) <= TOL_SYS
    got = O.MWF(mix, src)
    assert got.shape == src.shape
    assert rel(got, z["MWF"]) <= TOL_MWF_FIXTURE
    assert rel(got, R.MWF(mix, src)) <= TOL_MWF_FIXTURE
    # the kernels after the STFT: the restatement's MWF from the GPU's own spectra
    want = R.MWF_spectra(O.stft(mix.T), O.stft(src.transpose(0, 2, 1)), mix.shape[0])
    assert rel(got, want) <= TOL_SYS


def test_ibm_mask_bits_and_estimates_on_synthetic_audio():
    mix, src = synthetic(2, 20000, 2, 11)
    est, mask = O.IBM(mix, src, return_mask=True)
    T = R.nframes(20000)
    assert mask.dtype == np.uint8 and mask.shape == (2, 2, 1025, T)
    ratio = R.IBM_ratio(mix, src)
    far = np.abs(ratio - 0.5) / 0.5 > 1e-4
    assert np.array_equal(mask[far], (ratio[far] >= 0.5).astype(np.uint8))
    X = R.stft(mix.T)
    want = R.istft(X[None] * mask, 20000).transpose(0, 2, 1)
    assert rel(est, want) <= TOL_SYS


@pytest.mark.parametrize("nchan", [1, 2])
def test_three_sources(nchan):
    mix, src = synthetic(3, 12345, nchan, 5 + nchan)
    assert rel(O.IBM(mix, src, alpha=2, theta=0.4), R.IBM(mix, src, alpha=2, theta=0.4)) <= TOL_SYS
    assert rel(O.IRM(mix, src, alpha=1), R.IRM(mix, src, alpha=1)) <= TOL_SYS
    if nchan == 2:
        assert rel(O.MWF(mix, src), R.MWF(mix, src)) <= TOL_SYS


def test_dtypes_and_devices():
    mix, src = synthetic(2, 9000, 2, 3)
    want = R.IRM(mix, src)
    got = O.IRM(mix, src)                                       # float64 NumPy
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and rel(got, want) <= TOL_SYS
    got = O.IRM(mix.astype(np.float32), src.astype(np.float32))
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and rel(got, want) <= TOL_SYS
    tm, ts = torch.from_numpy(mix).cuda(), torch.from_numpy(src).float().cuda()
    got = O.MWF(tm, ts)
    assert torch.is_tensor(got) and got.is_cuda and got.device == ts.device and got.dtype == torch.float32
    assert rel(got.cpu().numpy(), R.MWF(mix, src)) <= TOL_SYS
    got = O.IBM(torch.from_numpy(mix), torch.from_numpy(src))  # host tensors: computed on the GPU, returned to the host
    assert torch.is_tensor(got) and not got.is_cuda and got.dtype == torch.float64
    X = O.stft(torch.from_numpy(mix.T).cuda())
    assert X.is_cuda and X.dtype == torch.complex64 and X.shape == (2, 1025, R.nframes(9000))
    y = O.istft(X, 9000)
    assert y.is_cuda and y.dtype == torch.float32 and sig_rel(y.cpu().numpy(), mix.T) <= TOL_SPEC
    assert O.stft(mix.T).dtype == np.complex128 and O.istft(R.stft(mix.T), 9000).dtype == np.float64


def test_mel_variants_are_bitwise():
    z = golden()
    mix, src = mel_inputs()
    for name, fn in (("IBM_melspec", O.IBM_melspec), ("IRM_melspec", O.IRM_melspec)):
        got = fn(mix, src)
        assert got.dtype == np.float32 and np.array_equal(got, z[name]), name
        assert np.array_equal(got, getattr(R, name)(mix, src)), name
    rng = np.random.default_rng(2)
    m = rng.random((3, 40, 17))
    s = np.stack([m * rng.random(m.shape), m * rng.random(m.shape), rng.random(m.shape)])
    s[0, 0, 0, :4] = 0.0
    for theta in (0.5, 0.25, 1.5):
        assert np.array_equal(O.IBM_melspec(m, s, theta=theta), R.IBM_melspec(m, s, theta=theta)), theta
    assert np.array_equal(O.IRM_melspec(m, s), R.IRM_melspec(m, s))
    t = O.IRM_melspec(torch.from_numpy(m).cuda(), torch.from_numpy(s).float().cuda(), alpha=7)
    assert t.is_cuda and t.dtype == torch.float32
    assert np.array_equal(t.cpu().numpy(), R.IRM_melspec(m, s.astype(np.float32)))


def test_two_calls_are_bitwise_identical():
    mix, src = synthetic(3, 30000, 2, 9)
    tm, ts = torch.from_numpy(mix).float().cuda(), torch.from_numpy(src).float().cuda()
    for fn in (O.IBM, O.IRM, O.MWF):
        a, b = fn(tm, ts), fn(tm, ts)
        assert torch.equal(a, b), fn.__name__


def test_bss_eval_on_oracle_estimates():
    z = golden()
    mix, src = stereo(z)
    for fn in (O.IRM, O.MWF):
        est = fn(mix, src)
        sdr, isr, sir, sar, perm = bsseval.bss_eval(src, est, window=8000, hop=8000, filters_len=64)
        assert sdr.shape == (2, 2) and np.all(np.isfinite(sdr)) and np.all(sdr > 0), (fn.__name__, sdr)
