"""BSS Eval v4 on the GPU (csrc/glowk_bsseval.h through audiosourcesep_amd/bsseval.py) against the reference's own outputs
(tests/golden/real_bsseval.npz) and the fp64 restatement of tests/bsseval_ref.py.

Bounds and their reasons:
* golden cases (real excerpts and the stored synthetic ones): 1e-9 dB.  On the CPU the restatement in the reference's algorithm
  (FFT + LU) is within 5.9e-11 dB of the reference, and in the kernels' algorithm (direct lag sums + Cholesky) within 4.6e-11 dB;
  the kernels differ from the latter only in the order of their fp64 sums.  1e-9 is ~17x the larger number;
* synthetic cases against the restatement: 1e-6 dB (well-conditioned G; the measured distance is at the 1e-12 level);
* the fallback case: SDR / ISR / SAR to 1e-6 dB; its SIR divides rounding noise (the interference is 0 in exact arithmetic), so
  it is only required to be above 250 dB, as the reference's 311-317 dB are.
perm and the NaN / inf pattern must be identical everywhere."""
import numpy as np
import pytest
import torch

from audiosourcesep_amd import bsseval
from tests import bsseval_ref as R
from tests.test_bsseval_cpu import assert_metrics, case_inputs, cases, expected, fallback_case, golden

pytestmark = pytest.mark.gpu
TOL_GOLDEN_DB = 1e-9
TOL_SYNTH_DB = 1e-6


def metrics(res):
    names = ("sdr", "isr", "sir", "sar") if len(res) == 5 else ("sdr", "sir", "sar")
    return dict(zip(names, res[:-1])), res[-1]


@pytest.mark.parametrize("name", [c["name"] for c in cases()])
def test_golden_case(name):
    z = golden()
    case = next(c for c in cases() if c["name"] == name)
    ref, est = case_inputs(z, case)
    got, perm = metrics(getattr(bsseval, case["fn"])(ref, est, **case["kw"]))
    want, wperm = expected(z, case)
    assert_metrics(got, want, TOL_GOLDEN_DB)
    assert perm.dtype == np.int64 and np.array_equal(perm, wperm)
    assert bsseval.last_fallbacks() == 0


def test_images_sdr_does_not_depend_on_the_filters():
    z = golden()
    case = next(c for c in cases() if c["name"] == "images_framewise")
    ref, est = case_inputs(z, case)
    a = bsseval.bss_eval(ref, est, window=15000, hop=15000, framewise_filters=True)
    b = bsseval.bss_eval(ref, est, window=15000, hop=15000, framewise_filters=False)
    assert np.max(np.abs(a[0] - b[0])) < 1e-9


def synthetic(nsrc, nchan, n, seed, alpha=0.2):
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((nsrc, n, nchan))
    for j in range(nsrc):
        for c in range(nchan):
            src[j, :, c] = np.convolve(src[j, :, c], rng.standard_normal(16) / 4.0, mode="same")
    est = np.empty_like(src)
    for j in range(nsrc):
        est[j] = 0.9 * src[j] + 0.1 * np.roll(src[j], 3, axis=0) + alpha * src[(j + 1) % nsrc] + 0.05 * rng.standard_normal((n, nchan))
    return src, est


@pytest.mark.parametrize("nsrc,nchan,n,kw", [
    (3, 1, 6000, dict(window=2500, hop=1700, compute_permutation=True)),
    (2, 2, 5000, dict(window=2000, hop=2000, framewise_filters=True, compute_permutation=True)),
    (4, 1, 3000, dict(window=np.inf, hop=np.inf, framewise_filters=True, bsseval_sources_version=True)),
    (2, 1, 30 * 16000, dict(window=16000, hop=16000)),
])
def test_synthetic_against_the_restatement(nsrc, nchan, n, kw):
    ref, est = synthetic(nsrc, nchan, n, seed=nsrc * 10 + nchan)
    if nchan == 1:
        ref, est = ref[..., 0], est[..., 0]
    got = bsseval.bss_eval(ref, est, **kw)
    want = R.bss_eval(ref, est, **kw)
    assert_metrics(dict(zip(("sdr", "isr", "sir", "sar"), got[:4])), dict(zip(("sdr", "isr", "sir", "sar"), want[:4])), TOL_SYNTH_DB)
    assert np.array_equal(got[4], want[4])


def test_bitwise_reproducible_and_input_forms_agree():
    z = golden()
    case = next(c for c in cases() if c["name"] == "stereo")
    ref32, est32 = z[case["ref"]], z[case["est"]]               # float32 as stored
    kw = case["kw"]
    a = bsseval.bss_eval(ref32, est32, **kw)
    b = bsseval.bss_eval(ref32, est32, **kw)
    c = bsseval.bss_eval(ref32.astype(np.float64), est32.astype(np.float64), **kw)
    d = bsseval.bss_eval(torch.from_numpy(ref32).cuda(), torch.from_numpy(est32).cuda(), **kw)
    e = bsseval.bss_eval(torch.from_numpy(ref32), torch.from_numpy(est32).double().cuda(), **kw)
    for other in (b, c, d, e):
        for x, y in zip(a, other):
            assert np.array_equal(x, y, equal_nan=True)


def test_least_squares_fallback():
    ref, est = fallback_case()
    got = bsseval.bss_eval(ref, est, window=np.inf, hop=np.inf, filters_len=1)
    assert bsseval.last_fallbacks() == 1                        # the one system over both references
    want = R.bss_eval(ref, est, window=np.inf, hop=np.inf, filters_len=1, algo="direct")
    for k in (0, 1, 3):
        assert np.max(np.abs(got[k] - want[k])) < TOL_SYNTH_DB, k
    assert np.all(got[2] > 250.0)
    assert np.array_equal(got[4], want[4])
    bsseval.bss_eval(*synthetic(2, 1, 2000, 1), window=np.inf, hop=np.inf)
    assert bsseval.last_fallbacks() == 0


def test_identical_estimate():
    ref, _ = synthetic(2, 1, 4000, 7)
    sdr, isr, sir, sar, _ = bsseval.bss_eval(ref[..., 0], ref[..., 0].copy(), window=np.inf, hop=np.inf, filters_len=32)
    for m in (sdr, sir, sar):
        assert np.all(m > 100.0)


def test_inputs_on_two_devices_are_refused():
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    ref, est = synthetic(2, 1, 1000, 2)
    with pytest.raises(ValueError, match="different devices"):
        bsseval.bss_eval(torch.from_numpy(ref).to("cuda:0"), torch.from_numpy(est).to("cuda:1"))
