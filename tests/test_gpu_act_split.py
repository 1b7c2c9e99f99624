"""The split kernels' activation + fp16 hi/lo split as one ReLU and two mixed-precision FMAs per value (csrc/glowk_kernels.h: split8).

The kernels used to compute  t = a * sc,  v = max(t, 0),  hi = fp16(v),  lo = fp16(v - fp32(hi))  with separate instructions.  For sc a
power of two (NetArgs::sc1 / sc2 always are: 2^-S) the product is exact and  v - hi  is exact in fp32, so
    v = max(a, 0),  hi = fp16(fma(v, sc, 0)),  lo = fp16(fma(v, sc, -hi))
gives the same bits; the FMA rounds its exact result to fp32 and then to fp16 (v_fma_mixlo / mixhi_f16).  That holds for v >= +0, which
the ReLU guarantees.  Signed values (the gathered inputs, the backward network) keep the multiply-then-split chain in the kernels: for
them the FMA form differs in the sign of a zero -- hi of v = -0, and lo of a negative product that underflows fp32 altogether.

* CPU: the identity in NumPy (fp64 holds the FMA's exact result), 0 differences over random exponents -30 .. 17, fp16 rounding ties and
  their fp32 neighbours, the fp16- and fp32-subnormal ranges, +-0 and the fp16 maximum, for S in {0, 1, 2, 5, 9, 14}; with sc = 0.3 the
  two forms must differ (the check can fail); and without the ReLU, on signed inputs, they differ in signs of zero only.
* GPU: glowk_split_probe -- one small kernel around the very helpers the network kernels inline -- against the NumPy restatement of the
  OLD arithmetic, uint16 equality, no tolerance: the classes above plus negatives, NaN and +-inf, ~5e5 values, three scales, all three
  modes (ReLU; two-term: hi only, lo = 0; no activation: the gather prologues).  max(t, 0) is restated as fmaxf computes it on the device
  (NaN -> 0, -0 -> +0).  The NaN that inf - inf creates is the negative quiet one (lo = 0xfe00) in NumPy on x86, in the old device
  arithmetic (measured with the previous helpers) and in the FMA form alike; a NaN input keeps its sign through both.
* GPU: a small flow (32 x 32 x 1, L = 2, K = 2, n_filters 128; 3 and 129 tiles) in f16x3 and f16x2 against the exact-fp32 kernels within
  the bars of tests/test_gpu_net_lattice.py (log_prob 2e-6 / 5e-5 relative; gradient atol 3e-4 max|g|, rtol 3e-3, its log_prob 2e-6 --
  in f16x2 the bar of that arithmetic's log_prob), and a second call repeats the first bit for bit."""
import ctypes

import numpy as np
import pytest

SHIFTS = (0, 1, 2, 5, 9, 14)


# ---- the two formulations in NumPy ------------------------------------------------------------------------------------------------
def relu32(t):
    """fmaxf(t, 0) as v_max_f32 computes it: NaN -> 0, -0 -> +0"""
    return np.where(t > 0, t, np.float32(0.0)).astype(np.float32)


def split_old(x, sc, mode):
    """multiply, activate, convert, convert back, subtract, convert: every step rounded to its format (mode 0 ReLU, 1 two-term, 2 none)"""
    with np.errstate(all="ignore"):
        t = (x.astype(np.float32) * np.float32(sc)).astype(np.float32)
        v = t if mode == 2 else relu32(t)
        hi = v.astype(np.float16)
        d = (v - hi.astype(np.float32)).astype(np.float32)
        lo = d.astype(np.float16)
    if mode == 1:
        lo = np.zeros_like(hi)
    return hi.view(np.uint16), lo.view(np.uint16)


def fma_f16(a, b, c):
    """fp16(fp32(a b + c)) with the sum exact before the first rounding: what v_fma_mix*_f16 computes (a b + c is exact in fp64 for the
    operands used here: 24-bit a, power-of-two or short b, and c = 0 or -fp16(a b))"""
    with np.errstate(all="ignore"):
        return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32).astype(np.float16)


def split_fma(x, sc, mode):
    x = x.astype(np.float32)
    v = x if mode == 2 else relu32(x)
    sc = np.float32(sc)
    hi = fma_f16(v, sc, np.zeros(v.shape))
    lo = fma_f16(v, sc, -hi.astype(np.float64))
    if mode == 1:
        lo = np.zeros_like(hi)
    return hi.view(np.uint16), lo.view(np.uint16)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def value_classes(n_random, rng):
    """{class: non-negative fp32 values} in the units of the SCALED value t; callers add signs and the inverse scale"""
    out = {}
    out["random exponents -30 .. 17"] = np.ldexp(rng.uniform(1.0, 2.0, n_random), rng.integers(-30, 18, n_random)).astype(np.float32)
    # fp16 rounding ties: midpoints of neighbouring fp16 values (normal and subnormal), and the fp32 values next to each midpoint
    h = rng.integers(0, 0x7BFF, n_random // 8).astype(np.uint16)
    mid = (h.view(np.float16).astype(np.float64) + (h + np.uint16(1)).view(np.float16).astype(np.float64)) / 2
    mid = mid.astype(np.float32)                                                # (12 significant bits: exact)
    out["fp16 ties"] = mid
    out["fp16 ties, fp32 neighbours"] = np.concatenate([np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))])
    out["fp16 subnormal range"] = np.ldexp(rng.uniform(1.0, 2.0, n_random // 8), rng.integers(-27, -13, n_random // 8)).astype(np.float32)
    out["fp32 subnormal range"] = (rng.integers(1, 1 << 23, n_random // 8).astype(np.uint32)).view(np.float32)
    out["fp32 smallest normals"] = np.ldexp(rng.uniform(1.0, 2.0, n_random // 16), rng.integers(-126, -110, n_random // 16)).astype(np.float32)
    top = np.float32(65504.0)
    out["zero and the fp16 maximum"] = np.array([0.0, top, np.nextafter(top, np.float32(0)), np.nextafter(top, np.float32(np.inf)), 65519.0,
                                                 65519.996, 65520.0, 65536.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -14, 1.0], dtype=np.float32)
    return out


def inputs_for(shift, n_random, rng, signed):
    """the classes as scaled values t and as inputs x = t 2^shift (so that x 2^-shift lands on the class), + negatives if asked"""
    cls = value_classes(n_random, rng)
    with np.errstate(over="ignore"):
        x = np.concatenate([np.concatenate([v, np.ldexp(v, shift).astype(np.float32)]) for v in cls.values()])
    x = np.concatenate([x, np.array([-0.0], dtype=np.float32)])
    if signed:
        x = np.concatenate([x, -x, np.array([np.nan, np.inf, -np.inf], dtype=np.float32)])
    return x[np.isfinite(x) | signed]


@pytest.mark.parametrize("shift", SHIFTS)
def test_the_fma_split_equals_the_multiply_split_for_powers_of_two(shift):
    """behind the ReLU (modes 0, 1) on signed inputs; without it (mode 2) on the non-negative ones"""
    rng = np.random.default_rng(100 + shift)
    x = inputs_for(shift, 200_000, rng, signed=True)
    x = x[np.isfinite(x)]
    assert np.sum(~np.signbit(x)) >= 400_000
    sc = 2.0 ** -shift
    for mode in (0, 1, 2):
        xm = x[~np.signbit(x)] if mode == 2 else x
        ho, lo_ = split_old(xm, sc, mode)
        hn, ln = split_fma(xm, sc, mode)
        print("S = %d mode %d: %d values, %d hi and %d lo differ" % (shift, mode, xm.size, np.sum(ho != hn), np.sum(lo_ != ln)))
        assert np.array_equal(ho, hn) and np.array_equal(lo_, ln)


def test_without_the_relu_the_fma_split_differs_in_signs_of_zero_only():
    """why the kernels keep the multiply for signed values: v = -0 (hi +0 for -0, lo -0 for +0) and negative products that round to zero in fp32 (lo -0 for +0)"""
    rng = np.random.default_rng(114)
    x = inputs_for(14, 200_000, rng, signed=True)
    x = x[np.isfinite(x)]
    ho, lo_ = split_old(x, 2.0 ** -14, 2)
    hn, ln = split_fma(x, 2.0 ** -14, 2)
    dh, dl = np.flatnonzero(ho != hn), np.flatnonzero(lo_ != ln)
    print("S = 14, no activation, signed: %d values, %d hi and %d lo differ" % (x.size, dh.size, dl.size))
    assert dh.size > 0 and np.all(x[dh] == 0) and np.all(np.signbit(x[dh])) and np.all(ho[dh] == 0x8000) and np.all(hn[dh] == 0)
    assert dl.size > 0 and np.all(lo_[dl] == 0) and np.all(ln[dl] == 0x8000)
    assert np.all(np.signbit(x[dl]) & (np.abs(x[dl].astype(np.float64)) * 2.0 ** -14 < 2.0 ** -149))


def test_the_two_splits_differ_for_a_scale_that_is_no_power_of_two():
    rng = np.random.default_rng(7)
    x = inputs_for(0, 200_000, rng, signed=False)
    assert x.size >= 400_000
    ho, lo_ = split_old(x, 0.3, 0)
    hn, ln = split_fma(x, 0.3, 0)
    n_hi, n_lo = int(np.sum(ho != hn)), int(np.sum(lo_ != ln))
    print("sc = 0.3: %d values, %d hi and %d lo differ" % (x.size, n_hi, n_lo))
    assert n_lo > 1000        # (the product is rounded before the split in one form and not in the other)


# ---- the device helpers -----------------------------------------------------------------------------------------------------------
def probe(x, sc, mode):
    import torch
    from audiosourcesep_amd import _lib
    lib = _lib.load()
    xd = torch.from_numpy(x).cuda()
    hi = torch.full((x.size,), -1, dtype=torch.int16, device="cuda")
    lo = torch.full((x.size,), -1, dtype=torch.int16, device="cuda")
    _lib.check(lib.glowk_split_probe(xd.data_ptr(), x.size, ctypes.c_float(sc), mode, hi.data_ptr(), lo.data_ptr(), None))
    torch.cuda.synchronize()
    return hi.cpu().numpy().view(np.uint16), lo.cpu().numpy().view(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", (0, 5, 14))
def test_the_device_split_gives_the_bits_of_the_old_arithmetic(shift):
    rng = np.random.default_rng(200 + shift)
    x = inputs_for(shift, 75_000, rng, signed=True)
    assert x.size >= 450_000 and np.isnan(x).any() and np.isinf(x).any()
    sc = 2.0 ** -shift
    bad = []
    for mode in (0, 1, 2):
        hd, ld = probe(x, sc, mode)
        hr, lr = split_old(x, sc, mode)
        dh, dl = np.flatnonzero(hd != hr), np.flatnonzero(ld != lr)
        print("S = %d mode %d: %d values, %d hi and %d lo differ" % (shift, mode, x.size, dh.size, dl.size))
        for name, idx, dev, ref in (("hi", dh, hd, hr), ("lo", dl, ld, lr)):
            for i in idx[:8]:
                print("   %s x = %r (bits %08x): device %04x, reference %04x" % (name, float(x[i]), int(x[i:i + 1].view(np.uint32)[0]), dev[i], ref[i]))
        bad.append((mode, dh.size, dl.size))
    assert all(h == 0 and l == 0 for _, h, l in bad), bad


@pytest.mark.gpu
def test_the_probe_refuses_a_scale_that_is_no_power_of_two():
    from audiosourcesep_amd import _lib
    x = np.ones(8, dtype=np.float32)
    for sc in (0.3, 0.0, -0.5, float("inf")):
        with pytest.raises(_lib.GlowkError):
            probe(x, sc, 0)
    hi, lo = probe(np.array([3.0, -3.0, 1.0 + 2.0 ** -12], dtype=np.float32), 0.5, 0)      # (n below one thread's eight values)
    assert list(hi) == [0x3E00, 0, 0x3800] and list(lo) == [0, 0, 0x0800]


# ---- a small flow -----------------------------------------------------------------------------------------------------------------
_flow = {}


def flow():
    """engine, 129 tiles and the exact-fp32 kernels' answers (computed once)"""
    if not _flow:
        import torch
        from audiosourcesep_amd import _lib
        from audiosourcesep_amd.config import GlowConfig
        from tests.test_gpu_training_shapes import engine_for, mel_tiles
        cfg = GlowConfig(H=32, W=32, C=1, L=2, K=2, F=128)
        eng, _ = engine_for(cfg)
        eng.set_range_policy("error")
        x = torch.from_numpy(mel_tiles(129, cfg, 17)).cuda()
        eng.set_precision(_lib.PREC_F32)
        lp = eng.log_prob(x).double()
        _, g = eng.log_prob_grad(x)
        _flow.update(eng=eng, x=x, lp=lp, g=g.double().clone())
    return _flow


@pytest.mark.gpu
@pytest.mark.parametrize("n", (3, 129))
@pytest.mark.parametrize("prec", ("f16x3", "f16x2"))
def test_a_small_flow_in_the_split_arithmetics_against_the_exact_kernels(prec, n):
    import torch
    from audiosourcesep_amd import _lib
    from tests.test_gpu_net_lattice import G_ATOL, G_RTOL, LP_TOL, LPG_TOL
    f = flow()
    eng, x, lp_ref, g_ref = f["eng"], f["x"][:n], f["lp"][:n], f["g"][:n]
    p = {"f16x3": _lib.PREC_F16X3, "f16x2": _lib.PREC_F16X2}[prec]
    eng.set_precision(p)
    lp = eng.log_prob(x).clone()
    lpg, g = eng.log_prob_grad(x)
    lpg, g = lpg.clone(), g.clone()
    lp2 = eng.log_prob(x).clone()
    lpg2, g2 = eng.log_prob_grad(x)
    e_lp = float(((lp.double() - lp_ref).abs() / lp_ref.abs()).max())
    e_lpg = float(((lpg.double() - lp_ref).abs() / lp_ref.abs()).max())
    gmax = float(g_ref.abs().max())
    e_g = float(torch.nan_to_num((g.double() - g_ref).abs() / (G_ATOL * gmax + G_RTOL * g_ref.abs()), nan=float("inf")).max())
    lpg_bar = LPG_TOL if p == _lib.PREC_F16X3 else LP_TOL[p]
    print("%s, %d tiles: log_prob %.2e (bar %.0e), log_prob_grad's log_prob %.2e (bar %.0e), gradient %.4f of its bar" % (
        prec, n, e_lp, LP_TOL[p], e_lpg, lpg_bar, e_g))
    assert e_lp <= LP_TOL[p] and e_lpg <= lpg_bar and e_g <= 1.0
    assert torch.equal(lp, lp2) and torch.equal(lpg, lpg2) and torch.equal(g, g2)
    assert eng.range_status() == (False, 0)
