"""The 2DFT separation on the GPU (audiosourcesep_amd/ft2d.py, csrc/glowk_dft2.h) against the fp64 restatement of tests/ft2d_ref.py.

Bars -- derived, not measured; u = 2^-24, R = rows, T = frames, S = sum |x| of one signal.

Forward, per real or imaginary component: ``|dev - ref| <= (2 R + 2 T + 8) u S``.  The kernels keep the summation order the bar was
written for: one fp32 fma chain per output and stage, in index order (a 32x32x2 MFMA adds its two products to the accumulator one
after the other).  Stage along frames: Y[r][v] is a chain of T terms x[r][t] w, each table entry rounded once (relative u / 2 per
factor, the entries are at most 1 in magnitude), so per component |dY| <= (T + 1) u sum_t |x[r][t]| to first order.  Stage along
rows: a chain of 2 R terms whose summands Yre c + Yim s are bounded by |Y[r][v]| (Cauchy-Schwarz), again with rounded table
entries: (2 R + 1) u sum_r |Y[r][v]| <= (2 R + 1) u S; the first stage's error (dYre, dYim) passes through one rotation, at most
sqrt 2 (T + 1) u sum_t |x[r][t]| per row, summed over the rows: sqrt 2 (T + 1) u S.  Together (2 R + 1.42 T + 2.42) u S, below the
bar with its constant unchanged.

Impulses (the sharp check: the bar above would not see one dropped element at the larger shapes): ``x = a`` at one position gives
``a exp(-2 pi i (u r / R + v t / T))``; every other term is an exact zero, so two table roundings, two products and one sum remain:
``8 u a`` per component.

Inverse, per element: ``(2 R + 2 T + 8) u sum |F M| / (R T)`` over the full Hermitian plane.  Stage along rows as above with
(2 R + 1) u; stage along frames a chain of 2 fc <= T + 2 terms (the weight 2 is exact), one rounded table entry per term and one
final product with the rounded 1 / (R T): (T + 5) u; the first stage's error passes with the factor sqrt 2 at most: below the bar.

End to end in fp64: a peak decision compares magnitudes that carry the forward error.  A magnitude moves by at most
sqrt 2 bar S (two components), a difference of two magnitudes (mx - mn, or mx - mag) by 2 sqrt 2 bar S, and the threshold
threshold_scale std by at most threshold_scale sqrt 2 bar S (a standard deviation is 1-Lipschitz in the root-mean-square norm of
its data): (2 + threshold_scale) sqrt 2 = 4.25 bars at threshold_scale = 1; the fp32 roundings of the magnitude, of the one
subtraction and of thr add less than 3 u S, inside the 0.25 that rounds the multiplier up to 4.5.  A cell is undecidable when it is
a local maximum of the fp64 plane with |(mx - mn) - thr| within that, or not one with mx - mag within it; at most 1 % of a shape's
cells may be (tests/test_ft2d_cpu.py measures the share on the CPU: 0, 0, 0.20, 0.11 and 0.38 %).

Measured on an MI355X (largest |dev - ref| / bar per shape): profiles/ft2d_accuracy.json and the table in DESIGN section 20."""
import ctypes
import functools
import json
import os
import wave

import numpy as np
import pytest
import torch
from scipy import ndimage

from audiosourcesep_amd import _lib, audio, ft2d
from tests import audio_ref as A
from tests import ft2d_ref as F
from tests import hpss_ref as H
from tests import repet_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# (nsig, rows, frames).  Small, odd, single-row and single-frame shapes with even and odd frames (with and without a Nyquist
# column), then both sides of every edge of the kernels' tiling: along fc a tile is 32 columns, a wave 64 (forward) or 32 (rows
# stage), a workgroup 256 or 128; along frames (inverse) 32, 128 and 512; 32 along rows and along nsig * rows; the K loops run in
# chunks of 8; and at 8192 frames the twiddle table moves from LDS to global memory
SHAPES = [(1, 1, 1), (1, 1, 2), (1, 2, 3), (2, 3, 5), (1, 33, 64), (3, 65, 130), (1, 129, 257), (1, 96, 600), (1, 1025, 96), (1, 4096, 34),
          (1, 31, 61), (1, 32, 62), (2, 16, 63), (1, 3, 31), (1, 2, 32), (1, 5, 65), (1, 2, 125), (1, 3, 127), (1, 2, 128), (1, 2, 129),
          (1, 3, 253), (1, 2, 254), (1, 2, 255), (1, 3, 256), (1, 33, 258), (1, 2, 509), (1, 3, 510), (1, 2, 511), (1, 2, 512), (1, 2, 513),
          (1, 2, 8192), (1, 1, 8193)]
IDS = lambda s: "-".join(map(str, s))
ACCURACY = {}


def continuous(rng, shape):
    """|N(0, 1)|^2 with about 5 % all-zero frames (none in a signal of fewer than 8 frames): tests/test_gpu_repet_beat.py's."""
    x = (np.abs(rng.standard_normal(shape)) ** 2).astype(np.float32)
    silent = (rng.random(shape[-1]) < 0.05) & (shape[-1] >= 8)
    if shape[-1] >= 8:
        silent[shape[-1] // 2] = True
    x[..., silent] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def spectra(shape):
    S = continuous(np.random.default_rng(1000 * shape[1] + shape[2]), shape)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def forward(shape):
    """(x, the device's spec as complex64, the device's mag), computed once per shape and never modified."""
    x = spectra(shape)
    spec, mag = ft2d.rfft2(x.copy(), return_magnitude=True)
    assert spec.is_cuda and spec.dtype == torch.complex64 and tuple(spec.shape) == shape[:2] + (shape[2] // 2 + 1,)
    assert mag.dtype == torch.float32 and tuple(mag.shape) == shape
    out = spec.cpu().numpy(), mag.cpu().numpy()
    for a in out:
        a.setflags(write=False)
    return (x,) + out


def bar(rows, frames):
    return F.component_bar(rows, frames)


def record(kind, shape, ratio):
    ACCURACY.setdefault(kind, {})[IDS(shape)] = round(float(ratio), 4)
    path = os.environ.get("FT2D_ACCURACY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(ACCURACY, f, indent=1, sort_keys=True)


def full_plane_sum(G, T):
    """sum |G| over the full Hermitian plane of a half spectrum [.., R, fc]: the self-conjugate columns once, the others twice."""
    fc = G.shape[-1]
    w = np.full(fc, 2.0)
    w[0] = 1.0
    if T % 2 == 0:
        w[-1] = 1.0
    return (np.abs(G.astype(np.complex128)) * w).sum(axis=(-2, -1))


# ---- the transforms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_transform_within_the_worst_case_bar(shape):
    nsig, rows, T = shape
    x, spec, _ = forward(shape)
    ref = np.fft.rfft2(x.astype(np.float64))
    worst = 0.0
    for s in range(nsig):
        lim = bar(rows, T) * float(np.abs(x[s].astype(np.float64)).sum())
        d = spec[s].astype(np.complex128) - ref[s]
        err = max(float(np.abs(d.real).max()), float(np.abs(d.imag).max()))
        worst = max(worst, err / lim if lim > 0 else float(err > 0))
    print("rdft2 %s: largest |dev - ref| / bar = %.4f" % (IDS(shape), worst))
    record("forward", shape, worst)
    assert worst <= 1.0


def impulse_positions(rows, T):
    rs = sorted({r for r in (0, 1, 31, 32, 33, rows // 2, rows - 2, rows - 1) if 0 <= r < rows})
    ts = sorted({t for t in (0, 1, 7, 8, 31, 32, 33, 127, 128, 129, T // 2, T - 2, T - 1) if 0 <= t < T})
    pos = {(r, t) for r in (0, rows - 1) for t in ts} | {(r, t) for r in rs for t in (0, T - 1)}
    pos |= {(r, t) for r in (31, 32) for t in (31, 32) if r < rows and t < T}
    return sorted(pos)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_transform_of_impulses(shape):
    _, rows, T = shape
    a = np.float32(0.7)
    pos = impulse_positions(rows, T)
    x = np.zeros((len(pos), rows, T), np.float32)
    for i, (r, t) in enumerate(pos):
        x[i, r, t] = a
    spec = ft2d.rfft2(x).cpu().numpy().astype(np.complex128)
    u, v = np.arange(rows)[:, None], np.arange(T // 2 + 1)[None, :]
    worst = 0.0
    for i, (r, t) in enumerate(pos):
        ang = 2.0 * np.pi * (((u * r) % rows) / rows + ((v * t) % T) / T)
        d = spec[i] - float(a) * (np.cos(ang) - 1j * np.sin(ang))
        worst = max(worst, float(np.abs(d.real).max()), float(np.abs(d.imag).max()))
    ratio = worst / (8 * U * float(a))
    print("rdft2 impulses %s: %d positions, largest error / (8 u a) = %.4f" % (IDS(shape), len(pos), ratio))
    record("impulse", shape, ratio)
    assert ratio <= 1.0


def symmetric_mask(rng, rows, T):
    M = (rng.random((rows, T)) < 0.5)
    u, v = np.meshgrid(np.arange(rows), np.arange(T), indexing="ij")
    copy, uu, vv = F.copied_cells(rows, T)
    M[copy] = M[uu[copy], vv[copy]]
    assert np.array_equal(M, M[(rows - u) % rows, (T - v) % T])
    return M.astype(np.float32)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_inverse_transform_within_the_worst_case_bar(shape, masked):
    nsig, rows, T = shape
    fc = T // 2 + 1
    rng = np.random.default_rng(7 * rows + T)
    G = (rng.standard_normal((nsig, rows, fc)) + 1j * rng.standard_normal((nsig, rows, fc))).astype(np.complex64)
    assert np.abs(G[..., 0].imag).min() > 0                                          # the self-conjugate columns have imaginary parts
    M = np.stack([symmetric_mask(rng, rows, T) for _ in range(nsig)]) if masked else None
    out = ft2d.irfft2(G.copy(), T, mask=None if M is None else M.copy())
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == shape
    out = out.cpu().numpy()
    Gm = G.astype(np.complex128) * (M[..., :fc] if masked else 1.0)
    ref = np.fft.irfft2(Gm, s=(rows, T))                                             # numpy drops those imaginary parts
    lim = bar(rows, T) * full_plane_sum(Gm, T) / (rows * T)
    err = np.abs(out - ref).max(axis=(-2, -1))
    worst = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), err > 0)))
    print("irdft2 %s %s: largest |dev - ref| / bar = %.4f" % (IDS(shape), "masked" if masked else "plain", worst))
    record("inverse_masked" if masked else "inverse", shape, worst)
    assert worst <= 1.0
    if not masked:                                                                    # a mask of ones is no mask, bit for bit
        ones = ft2d.irfft2(G.copy(), T, mask=np.ones(shape, np.float32)).cpu().numpy()
        np.testing.assert_array_equal(ones.view(np.uint32), out.view(np.uint32))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_round_trip_under_the_sum_of_the_two_bars(shape):
    nsig, rows, T = shape
    x, spec, _ = forward(shape)
    back = ft2d.irfft2(spec.copy(), T).cpu().numpy()
    worst = 0.0
    for s in range(nsig):
        lim = bar(rows, T) * (float(np.abs(x[s].astype(np.float64)).sum()) + float(full_plane_sum(spec[s], T)) / (rows * T))
        err = float(np.abs(back[s].astype(np.float64) - x[s]).max())
        worst = max(worst, err / lim if lim > 0 else float(err > 0))
    print("round trip %s: largest error / (sum of the bars) = %.4f" % (IDS(shape), worst))
    record("round_trip", shape, worst)
    assert worst <= 1.0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_magnitude_plane_formula_and_bitwise_copies(shape):
    nsig, rows, T = shape
    _, spec, mag = forward(shape)
    fc = T // 2 + 1
    copy, uu, vv = F.copied_cells(rows, T)
    for s in range(nsig):
        re, im = spec[s].real.astype(np.float64), spec[s].imag.astype(np.float64)
        want = np.sqrt(re * re + im * im).astype(np.float32)
        got = mag[s][:, :fc]
        ulp = np.spacing(np.maximum(want, np.float32(1e-30)))
        computed = ~copy[:, :fc]
        assert (np.abs(got.astype(np.float64) - want)[computed] <= ulp[computed]).all()
        np.testing.assert_array_equal(mag[s][copy].view(np.uint32), mag[s][uu[copy], vv[copy]].view(np.uint32))
        u, v = np.meshgrid(np.arange(rows), np.arange(T), indexing="ij")
        np.testing.assert_array_equal(mag[s], mag[s][(rows - u) % rows, (T - v) % T])  # Hermitian in its bits
        np.testing.assert_array_equal(mag[s][:, fc:], mag[s][(rows - u[:, fc:]) % rows, T - v[:, fc:]])   # the plain index map of the mirrored columns


# ---- the standard deviation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (3, 65, 130), (1, 96, 600), (1, 1025, 96), (1, 64, 64), (1, 4097, 1), (2, 1025, 1100)], ids=IDS)
def test_plane_std_against_numpy(shape):
    nsig, rows, T = shape
    n = rows * T
    x = spectra(shape) if shape[1] <= 4096 else spectra((nsig, 1, n)).reshape(shape)
    dev = torch.from_numpy(x.copy()).cuda()
    got = ft2d._plane_std(dev)
    assert got.dtype == torch.float64 and tuple(got.shape) == (nsig, 2)
    got = got.cpu().numpy()
    x64 = x.astype(np.float64).reshape(nsig, n)
    for s in range(nsig):
        mean, std = x64[s].mean(), x64[s].std()
        assert abs(got[s, 0] - mean) <= n * 2.0 ** -52 * abs(mean) and abs(got[s, 1] - std) <= n * 2.0 ** -52 * std
        alone = ft2d._plane_std(dev[s:s + 1]).cpu().numpy()
        np.testing.assert_array_equal(alone[0].view(np.uint64), got[s].view(np.uint64))   # a batch equals its signals alone


# ---- the peak rule ----------------------------------------------------------------------------------------------------------------------
PEAK_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 33, 64), (3, 65, 130), (1, 129, 257), (1, 4096, 34), (1, 31, 61), (1, 2, 255), (1, 3, 256), (1, 33, 258)]


def peak_planes(kind, shape):
    rng = np.random.default_rng(11 * shape[1] + shape[2])
    if kind == "random":
        return rng.standard_normal(shape).astype(np.float32)
    if kind == "ties":
        return rng.choice(np.array([0.0, 0.5, 1.0, 2.0], np.float32), shape)
    if kind == "constant":
        return np.full(shape, 1.5, np.float32)
    return forward(shape)[2].copy()                                                 # the device's own magnitude plane


@pytest.mark.parametrize("kind", ["random", "ties", "constant", "mag"])
@pytest.mark.parametrize("shape", PEAK_SHAPES, ids=IDS)
def test_peak_mask_equals_the_restatement_bit_for_bit(shape, kind):
    nsig, rows, cols = shape
    P = peak_planes(kind, shape)
    dev = torch.from_numpy(P).cuda()
    nbs = [(1, 1), (1, 25), (3, 5), (127, 1), (1, 127)] + ([(5, 2 * cols + 1)] if 2 * cols + 1 <= 127 else [])
    for nb in nbs:
        mask, mx, mn = ft2d.peak_mask(dev, nb, None, return_extrema=True)
        mask, mx, mn = mask.cpu().numpy(), mx.cpu().numpy(), mn.cpu().numpy()
        thr = np.zeros(nsig, np.float32)
        for s in range(nsig):
            want_mx, want_mn = ndimage.maximum_filter(P[s], size=nb, mode="wrap"), ndimage.minimum_filter(P[s], size=nb, mode="wrap")
            np.testing.assert_array_equal(mx[s], want_mx)
            np.testing.assert_array_equal(mn[s], want_mn)
            np.testing.assert_array_equal(mask[s], F.peaks(P[s], nb))
            d = np.sort((want_mx - want_mn).ravel())
            thr[s] = d[len(d) // 2]                                                 # one of the plane's own mx - mn values: the rule is strict
        for t in (np.zeros(nsig, np.float32), thr):
            got = ft2d.peak_mask(dev, nb, t).cpu().numpy()
            for s in range(nsig):
                np.testing.assert_array_equal(got[s], F.peaks(P[s], nb, t[s]))
        one = ft2d.peak_mask(dev[0], nb, float(thr[0])).cpu().numpy()                # [rows, cols] and a plain number
        np.testing.assert_array_equal(one, F.peaks(P[0], nb, thr[0]))


# ---- the staged pipeline ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power,margin", [(1.0, 1.0), (2.0, (2.0, 10.0))], ids=["ratio", "margins"])
@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 33, 64), (3, 65, 130), (1, 129, 257), (1, 96, 600), (1, 1025, 96)], ids=IDS)
def test_ft2d_stage_by_stage(shape, power, margin):
    nsig, rows, T = shape
    x, spec, mag = forward(shape)
    nb, scale = (1, 25), 1.0
    mb, mf, peaks = ft2d.ft2d(x.copy(), nb, scale, power, margin, mask=True, return_peaks=True)
    ob, of = ft2d.ft2d(x.copy(), nb, scale, power, margin)
    std = ft2d._plane_std(torch.from_numpy(mag.copy()).cuda()).cpu().numpy()[:, 1]
    thr = (scale * std).astype(np.float32)
    back = ft2d.irfft2(spec.copy(), T, mask=peaks).cpu().numpy()
    rep, res = np.abs(back), np.abs(x - back)
    mb, mf, peaks = mb.cpu().numpy(), mf.cpu().numpy(), peaks.cpu().numpy()
    for s in range(nsig):
        n = rows * T
        assert abs(std[s] - mag[s].astype(np.float64).std()) <= n * 2.0 ** -52 * std[s]
        np.testing.assert_array_equal(peaks[s], F.peaks(mag[s], nb, thr[s]))         # exact, on the device's own plane
        want = F.irfft2(spec[s], T, peaks[s])
        lim = bar(rows, T) * float(full_plane_sum(spec[s] * peaks[s][:, :T // 2 + 1], T)) / n
        assert np.abs(rep[s] - np.abs(want)).max() <= lim
        wb, wf = H.masks(rep[s], res[s], power, margin)
        assert max(np.abs(mb[s] - wb).max(), np.abs(mf[s] - wf).max()) <= 1e-6
    np.testing.assert_array_equal(ob.cpu().numpy(), x * mb)
    np.testing.assert_array_equal(of.cpu().numpy(), x * mf)


def test_ft2d_of_complex_spectra_keeps_the_phase():
    rng = np.random.default_rng(21)
    S = continuous(rng, (2, 33, 65))
    Sc = (S * np.exp(1j * rng.uniform(-np.pi, np.pi, S.shape))).astype(np.complex64)
    mag = np.abs(Sc)
    for c, r in zip(ft2d.ft2d(Sc), ft2d.ft2d(mag)):
        assert c.dtype == torch.complex64 and tuple(c.shape) == S.shape and r.dtype == torch.float32
        c, r = c.cpu().numpy(), r.cpu().numpy()
        live = r > 0
        assert live.any() and np.abs(c[live] / np.abs(c[live]) - Sc[live] / mag[live]).max() <= 1e-6
        assert np.abs(np.abs(c) - r).max() <= 1e-6 * r.max() and not c[~live].any()


# ---- all fp64, end to end -----------------------------------------------------------------------------------------------------------------
E2E_MULTIPLIER = 4.5                        # (2 + threshold_scale) sqrt 2, rounded up: the module docstring


@pytest.mark.parametrize("case", [(33, 64, 8), (65, 130, 13), (129, 257, 16), (96, 600, 25), (1025, 96, 12)], ids=lambda c: "%dx%d" % c[:2])
def test_ft2d_end_to_end_against_fp64(case):
    rows, T, p = case
    bg, fg = F.crafted(rows, T, p, 7)
    x = bg + fg
    mask_b, mask_f, peaks = ft2d.ft2d(x.copy(), (1, 25), 1.0, mask=True, return_peaks=True)
    und, ref = F.undecidable(x, (1, 25), 1.0, E2E_MULTIPLIER)
    share = float(und.mean())
    peaks = peaks.cpu().numpy()
    wrong = (peaks != ref["M"]) & ~und
    print("ft2d end to end %dx%d: %.4f %% undecidable, %d of %d peaks differ inside them, %d outside" %
          (rows, T, 100 * share, int(((peaks != ref["M"]) & und).sum()), int(ref["M"].sum()), int(wrong.sum())))
    assert share <= 0.01                                                              # the cap: a condition, not a measurement
    assert not wrong.any()
    if (rows, T) == (96, 600):
        keep_b = float((mask_b.cpu().numpy().astype(np.float64) * bg).sum() / bg.sum())
        keep_f = float((mask_f.cpu().numpy().astype(np.float64) * fg).sum() / fg.sum())
        print("ft2d at 96x600: the background mask keeps %.3f of bg, the foreground mask %.3f of fg" % (keep_b, keep_f))
        assert keep_b > 0.5 and keep_f > 0.5


# ---- the launch contract ----------------------------------------------------------------------------------------------------------------
def test_runs_are_reproducible_and_a_batch_is_its_signals_alone():
    shape = (3, 65, 130)
    x, spec, mag = forward(shape)
    dev = torch.from_numpy(x.copy()).cuda()

    def everything(t):
        s, m = ft2d.rfft2(t, return_magnitude=True)
        pk = ft2d.peak_mask(m, (3, 5), 0.25)
        back = ft2d.irfft2(s, t.shape[-1], mask=pk)
        return (torch.view_as_real(s), m, pk, back) + tuple(ft2d.ft2d(t, (3, 5), 0.5, return_peaks=True))

    first, second = everything(dev), everything(dev)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    np.testing.assert_array_equal(first[0].cpu().numpy().view(np.uint32), spec.view(np.float32).reshape(first[0].shape).view(np.uint32))
    for s in range(3):
        for a, b in zip(everything(dev[s]), first):
            assert torch.equal(a, b[s])
    empty = torch.empty((0, 4, 9), device="cuda")
    s, m = ft2d.rfft2(empty, return_magnitude=True)
    assert tuple(s.shape) == (0, 4, 5) and tuple(m.shape) == (0, 4, 9)
    assert tuple(ft2d.irfft2(s, 9).shape) == (0, 4, 9) and tuple(ft2d.peak_mask(m).shape) == (0, 4, 9)
    assert all(tuple(t.shape) == (0, 4, 9) for t in ft2d.ft2d(empty))


def test_bad_calls_are_refused_with_a_message_and_launch_nothing():
    lib = _lib.load()
    rows, T, fc = 12, 30, 16
    x = torch.rand(rows, T, device="cuda")
    canary = torch.full((rows, fc, 2), 7.0, device="cuda")
    out = torch.full((rows, T), 7.0, device="cuda")
    nbytes = lib.glowk_dft2_workspace_bytes(1, rows, T)
    work = torch.zeros(nbytes // 8 + 1024, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    z = ctypes.c_void_p(0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    err = lambda: lib.glowk_last_error().decode()
    host = np.zeros((rows, T), np.float32)
    hp = host.ctypes.data_as(ctypes.c_void_p)
    big = work.numel() * 8
    bad = [
        (lambda: lib.glowk_rdft2(p(x), -1, rows, T, p(canary), z, p(work), big, st), "nsig"),
        (lambda: lib.glowk_rdft2(p(x), 65536, rows, T, p(canary), z, p(work), big, st), "nsig"),
        (lambda: lib.glowk_rdft2(p(x), 1, 0, T, p(canary), z, p(work), big, st), "rows"),
        (lambda: lib.glowk_rdft2(p(x), 1, 4097, T, p(canary), z, p(work), big, st), "rows"),
        (lambda: lib.glowk_rdft2(p(x), 1, rows, 0, p(canary), z, p(work), big, st), "frames"),
        (lambda: lib.glowk_rdft2(p(x), 1, rows, 32769, p(canary), z, p(work), big, st), "frames"),
        (lambda: lib.glowk_rdft2(p(x), 16, 4096, 32768, p(canary), z, p(work), big, st), "2^31"),
        (lambda: lib.glowk_rdft2(p(x), 1, rows, T, p(canary), z, p(work), nbytes - 1, st), "work_bytes"),
        (lambda: lib.glowk_rdft2(hp, 1, rows, T, p(canary), z, p(work), big, st), "device memory"),
        (lambda: lib.glowk_rdft2(p(x), 1, rows, T, p(x), z, p(work), big, st), "overlap"),
        (lambda: lib.glowk_rdft2(p(x), 1, rows, T, p(canary), p(x), p(work), big, st), "overlap"),
        (lambda: lib.glowk_rdft2(p(x), 1, rows, T, p(canary), z, p(x), big, st), "work_dev"),
        (lambda: lib.glowk_irdft2(p(canary), z, 1, rows, 32769, p(out), p(work), big, st), "frames"),
        (lambda: lib.glowk_irdft2(p(canary), z, 1, 4097, T, p(out), p(work), big, st), "rows"),
        (lambda: lib.glowk_irdft2(p(canary), z, 1, rows, T, hp, p(work), big, st), "device memory"),
        (lambda: lib.glowk_irdft2(p(canary), z, 1, rows, T, p(canary), p(work), big, st), "overlap"),
        (lambda: lib.glowk_irdft2(p(canary), p(out), 1, rows, T, p(out), p(work), big, st), "overlap"),
        (lambda: lib.glowk_plane_std(p(x), 1, 0, p(work), p(work[64:]), 1024, st), "n must"),
        (lambda: lib.glowk_plane_std(hp, 1, rows * T, p(work), p(work[64:]), 1024, st), "device memory"),
        (lambda: lib.glowk_plane_std(p(x), 1, rows * T, p(x), p(work), 1024, st), "overlap"),
        (lambda: lib.glowk_peak_mask(p(x), 1, rows, T, 2, 25, z, p(out), z, z, p(work), big, st), "nb_r"),
        (lambda: lib.glowk_peak_mask(p(x), 1, rows, T, 1, 24, z, p(out), z, z, p(work), big, st), "nb_c"),
        (lambda: lib.glowk_peak_mask(p(x), 1, rows, T, 1, 129, z, p(out), z, z, p(work), big, st), "nb_c"),
        (lambda: lib.glowk_peak_mask(p(x), 1, rows, 32769, 1, 25, z, p(out), z, z, p(work), big, st), "frames"),
        (lambda: lib.glowk_peak_mask(hp, 1, rows, T, 1, 25, z, p(out), z, z, p(work), big, st), "device memory"),
        (lambda: lib.glowk_peak_mask(p(x), 1, rows, T, 1, 25, z, p(x), z, z, p(work), big, st), "overlap"),
        (lambda: lib.glowk_peak_mask(p(x), 1, rows, T, 1, 25, z, p(out), p(out), z, p(work), big, st), "overlap"),
        (lambda: lib.glowk_peak_mask(p(x), 1, rows, T, 1, 25, z, p(out), z, z, p(work), 8 * rows * T - 1, st), "work_bytes"),
    ]
    for n, (call, word) in enumerate(bad):
        assert call() == _lib.ERR and word in err(), (n, err())
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all()) and bool((out == 7.0).all()) and not bool(work.any())     # nothing was launched
    assert lib.glowk_rdft2(z, 0, rows, T, z, z, z, 0, st) == _lib.OK and lib.glowk_irdft2(z, z, 0, rows, T, z, z, 0, st) == _lib.OK
    assert lib.glowk_plane_std(z, 0, 5, z, z, 0, st) == _lib.OK and lib.glowk_peak_mask(z, 0, rows, T, 1, 25, z, z, z, z, z, 0, st) == _lib.OK
    assert lib.glowk_rdft2(p(x), 1, rows, T, p(canary), z, p(work), nbytes, st) == _lib.OK       # and the valid call goes through
    torch.cuda.synchronize()
    assert not bool((canary == 7.0).any())


# ---- audio ---------------------------------------------------------------------------------------------------------------------------
N_AUDIO = 48000
AUDIO_BAR = 1e-5
CUT_ROWS = 13                               # rows r with r 16000 / 2048 <= 100 Hz: 0 .. 12


def test_ft2d_audio_against_the_restatement():
    pattern, chirp = R.pattern_and_chirp(N_AUDIO)
    y = (pattern + chirp).astype(np.float32)
    peak = float(np.abs(y).max())
    b, f, r = ft2d.ft2d_audio(y.copy(), residual=True)
    assert b.is_cuda and tuple(b.shape) == tuple(f.shape) == tuple(r.shape) == (N_AUDIO,) and b.dtype == torch.float32
    assert torch.equal(r, torch.from_numpy(y).cuda() - b - f)
    b, f = b.cpu().numpy(), f.cpu().numpy()
    _, X = audio.mel_frames(y[None], return_stft=True)
    wb, wf = (m[0].cpu().numpy().astype(np.float64) for m in ft2d.ft2d(X.abs(), mask=True))
    wb[:CUT_ROWS], wf[:CUT_ROWS] = 1.0, 0.0                                         # at most 100 Hz: wholly background
    X0 = X[0].cpu().numpy().astype(np.complex128)
    want_b, want_f = (A.istft(X0 * m)[:N_AUDIO] for m in (wb, wf))
    e_b, e_f = float(np.abs(b - want_b).max() / peak), float(np.abs(f - want_f).max() / peak)
    e_sum = float(np.abs(b.astype(np.float64) + f - y).max() / peak)
    print("ft2d_audio: background %.2e, foreground %.2e, background + foreground - y %.2e of the peak" % (e_b, e_f, e_sum))
    assert e_b <= AUDIO_BAR and e_f <= AUDIO_BAR and e_sum <= AUDIO_BAR              # unit margins: the stems sum to the mixture
    two = np.stack([y, 0.5 * y[::-1]]).astype(np.float32)                             # a channel's stems depend on that channel alone
    b2, f2 = ft2d.ft2d_audio(two, cutoff_hz=0.0)
    b1, f1 = ft2d.ft2d_audio(two[1], cutoff_hz=0.0)
    assert tuple(b2.shape) == (2, N_AUDIO) and torch.equal(b2[1], b1) and torch.equal(f2[1], f1)


def test_separate_wav_ft2d_returns_the_files_rate_and_length(tmp_path):
    rate = 22050
    pattern, chirp = R.pattern_and_chirp(N_AUDIO, rate)
    y = pattern + chirp
    q = np.rint(np.clip(np.stack([y, 0.5 * y]), -1.0, 1.0) * 32767.0).astype("<i2")
    stereo = tmp_path / "stereo.wav"
    with wave.open(str(stereo), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(q.T).tobytes())
    stems, out_rate = ft2d.separate_wav_ft2d(str(stereo))
    assert out_rate == rate and tuple(stems.shape) == (2, 2, N_AUDIO) and bool(torch.isfinite(stems).all()) and float(stems.abs().max()) > 0.1
    n16 = -(-N_AUDIO * 16000 // rate)
    stems, out_rate = ft2d.separate_wav_ft2d(str(stereo), out_rate=None, mono=True, neighborhood=(3, 5), threshold_scale=0.5, residual=True)
    assert out_rate == 16000 and tuple(stems.shape) == (3, n16) and bool(torch.isfinite(stems).all())
    stems, out_rate = ft2d.separate_wav_ft2d(str(stereo), residual=True)
    assert out_rate == rate and tuple(stems.shape) == (3, 2, N_AUDIO)
    missing = tmp_path / "missing.wav"
    with pytest.raises(ValueError, match="unexpected keyword"):
        ft2d.separate_wav_ft2d(str(missing), period_sec=(0.3, 0.8))                   # refused before the file is opened
