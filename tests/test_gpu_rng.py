"""The device RNG (philox4x32_10 / normal4 / k_basis_noise / k_add_noise, csrc/glowk_basis.h) against its restatement from the
specification in include/glowk.h (tests/rng_ref.py, held to Philox4x32-10 by the known answers of tests/test_rng_cpu.py): the
U(0, 1) draws bit for bit, the N(0, 1) draws within 4e-6, at every stream id, source pair, seed, step and offset where a counter
word changes hands, and the consumers of the stream at the far counters.

The normal bar: the restatement forms u1, u2 and theta = fl32(2 pi) u2 in float32 as the kernel does, so what is left is the error
of the device's logf, sqrtf and sincosf times r <= sqrt(50 ln 2) = 5.89.  A correctly rounded float32 evaluation of the same
formula is within 6.0e-7 of the restatement over 2^20 draws; 4e-6 leaves the device's math library about 2 ulp per function."""
import ctypes

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, basis
from audiosourcesep_amd.config import GlowConfig
from tests import rng_ref as R

pytestmark = pytest.mark.gpu
NORMAL_BAR = 4e-6
BASES = [dict(seed=7, step=5, which=1, pair=3, offset=0, n=1025), dict(seed=1234, step=(1 << 32) + 9, which=14, pair=0, offset=1020, n=37)]
FAR_OFFSET = 4 * (2 ** 32 - 2)              # with n = 16 the quads 2^32 - 2 .. 2^32 + 1: over the carry of c0 into c1


def cases():
    """One argument at a time around the two base points."""
    out = []
    for base in BASES:
        out.append(dict(base))
        out += [dict(base, which=w) for w in range(16)]
        out += [dict(base, pair=p, step=base["step"] & (2 ** 48 - 1)) for p in (0, 1, 7, 65535)]
        out += [dict(base, n=n) for n in (1, 3, 4, 5, 1023, 1024, 1025)]
        out += [dict(base, seed=s) for s in (0, 7, 1234, 0xDEADBEEF12345678, 2 ** 64 - 1)]
        out += [dict(base, step=t) for t in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 48 - 1)]
        out.append(dict(base, step=2 ** 63 + 5, pair=0))                           # (a source pair needs step < 2^48)
        out += [dict(base, offset=o) for o in (0, 4, 1020, 2 ** 40)]
        out.append(dict(base, offset=FAR_OFFSET, n=16))
    seen, uniq = set(), []
    for c in out:
        key = tuple(sorted(c.items()))
        if key not in seen:
            seen.add(key)
            uniq.append(c)
    return uniq


def device(c, uniform):
    return basis.device_randn((c["n"],), "cuda", c["seed"], c["step"], c["which"], uniform=uniform, offset=c["offset"], pair=c["pair"]).cpu().numpy()


def test_uniform_draws_are_the_restatement_bit_for_bit():
    cs = cases()
    for c in cs:
        got = device(c, True)
        assert got.dtype == np.float32 and np.array_equal(got, R.uniform(**c)), c
    print("%d launches" % len(cs))


def test_normal_draws_are_within_the_bar_of_the_restatement():
    worst, at = 0.0, None
    for c in cases():
        err = float(np.abs(device(c, False).astype(np.float64) - R.normal(**c)).max())
        if err > worst:
            worst, at = err, c
    print("normal draws: max |device - fp64 restatement| %.3e (bar %.1e) at %s" % (worst, NORMAL_BAR, at))
    assert worst <= NORMAL_BAR, at


def test_boundary_draws():
    """The words whose top 24 bits are all ones or all zero (found by search on the CPU): the uniform draw stays strictly inside
    (0, 1) -- before the clamp it was exactly 1.0 at the all-ones elements -- and Box-Muller's two ends come out as they should:
    u1 = 1 the pair (0, 0), u1 = 2^-25 the largest radius sqrt(50 ln 2)."""
    n_ones = n_u1_one = n_u1_small = 0
    for seed in (0, 1234):
        ones, zero = R.boundary_elements(seed)
        for e in ones + zero:
            off = e - e % 4
            u = basis.device_randn((4,), "cuda", seed, uniform=True, offset=off).cpu().numpy()
            z = basis.device_randn((4,), "cuda", seed, offset=off).cpu().numpy().astype(np.float64)
            print("seed %d element %d (%s): uniform draw %r, normal pair (%r, %r)" % (seed, e, "ones" if e in ones else "zero", float(u[e % 4]),
                                                                                    z[(e % 4) & 2], z[((e % 4) & 2) + 1]))
            assert (u > 0.0).all() and (u < 1.0).all(), (seed, e, u)
            assert np.array_equal(u, R.uniform(seed, offset=off, n=4))
            assert u[e % 4] == (R.BELOW_ONE if e in ones else np.float32(2.0 ** -25))
            assert np.abs(z - R.normal(seed, offset=off, n=4)).max() <= NORMAL_BAR
            n_ones += e in ones
            if e % 2 == 0:                                                         # the word is u1 of its pair
                if e in ones:
                    assert z[e % 4] == 0.0 and z[e % 4 + 1] == 0.0
                    n_u1_one += 1
                else:
                    assert abs(np.hypot(z[e % 4], z[e % 4 + 1]) - np.sqrt(50.0 * np.log(2.0))) <= NORMAL_BAR
                    n_u1_small += 1
    assert n_ones >= 2 and n_u1_one >= 1 and n_u1_small >= 1                        # every branch above was reached


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("sigma", [0.0, 0.01, 120.0])
def test_add_noise(sigma):
    """out = x + sigma z with the restatement's z: within 4e-6 sigma plus one ulp of the result; in place gives the same bits."""
    n, seed, step, which, offset = 1029, 7, 2 ** 48 - 1, 2, 1020
    x = np.random.default_rng(3).uniform(-100.0, 20.0, n).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    out = basis.add_device_noise(xd, sigma, seed, step, which, offset)
    want = x.astype(np.float64) + float(np.float32(sigma)) * R.normal(seed, step, which, 0, offset, n)
    got = out.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    bound = NORMAL_BAR * sigma + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print("sigma %g: max |d| %.3e, max of |d| / bound %.3f" % (sigma, err.max(), (err / bound).max()))
    assert (err <= bound).all()
    assert torch.equal(xd.cpu(), torch.from_numpy(x))                              # the input is left alone
    if sigma == 0.0:
        assert np.array_equal(got, x)
    else:
        assert not np.array_equal(got, x)
    p = ctypes.c_void_p(xd.data_ptr())
    assert _lib.load().glowk_add_noise(p, p, n, ctypes.c_float(sigma), seed, step, which, offset, _st()) == _lib.OK
    assert torch.equal(xd, out)


ETA, LAM = 2e-5 * 37.0, 1.0 / 0.3 ** 2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


@pytest.mark.parametrize("offset", [0, 1020, FAR_OFFSET])
def test_update_draws_at_the_far_counters(offset):
    """langevin_update_n with its own draws at step 2^48 - 1 for 16 sources (pairs 0..7) == the same call with the draws
    device_randn reports for (which k & 1, pair k >> 1) at that step and offset, bit for bit."""
    S, n, seed, step = 16, 1029, 99, 2 ** 48 - 1
    rng = np.random.default_rng(5 + offset % 1000)
    xs, gs, mixed = rng.uniform(-80, 10, (S, n)), rng.normal(0, 5, (S, n)), rng.uniform(-80, 10, n)

    def run(eps, **kw):
        ys = [dev(x) for x in xs]
        basis.langevin_update_n(dev(mixed), ys, [dev(g) for g in gs], ETA, LAM, eps, **kw)
        return torch.stack(ys)

    own = run(None, seed=seed, step=step, offset=offset)
    rep = [basis.device_randn((n,), "cuda", seed, step, which=k & 1, pair=k >> 1, offset=offset) for k in range(S)]
    assert torch.equal(own, run(rep))
    for k in (0, 1, 14, 15):                                                       # and those draws are the restatement's
        assert np.abs(rep[k].cpu().numpy() - R.normal(seed, step, k & 1, k >> 1, offset, n)).max() <= NORMAL_BAR
    assert not any(torch.equal(own[k], o) for o in (run(None, seed=seed, step=5, offset=offset),) for k in range(S))


def test_frame_update_draws_at_the_far_step():
    """langevin_update_frames, 16 sources at step 2^48 - 1: element b F + f of each source's stream at offset 0."""
    S, rows, width, F, hop, seed, step = 16, 16, 16, 37, 5, 99, 2 ** 48 - 1
    N = basis.tile_count(F, width, hop)
    rng = np.random.default_rng(6)
    xs, gs, mixed = rng.uniform(-80, 10, (S, rows, F)), rng.normal(0, 5, (S, N, rows, width)), rng.uniform(-80, 10, (rows, F))

    def run(eps, **kw):
        y = dev(xs)
        basis.langevin_update_frames(dev(mixed), y, [dev(g) for g in gs], width, hop, ETA, LAM, eps, **kw)
        return y

    own = run(None, seed=seed, step=step)
    rep = [basis.device_randn((rows, F), "cuda", seed, step, which=k & 1, pair=k >> 1) for k in range(S)]
    assert torch.equal(own, run(rep))
    for k in (0, 15):
        assert np.abs(rep[k].cpu().numpy().reshape(-1) - R.normal(seed, step, k & 1, k >> 1, 0, rows * F)).max() <= NORMAL_BAR
    other = run(None, seed=seed, step=5)
    assert not any(torch.equal(own[k], other[k]) for k in range(S))


def test_sample_draws_stream_3():
    from audiosourcesep_amd.flow_models.flow_glow import GlowFlow
    from audiosourcesep_amd.synthetic import calibrated_engine
    cfg = GlowConfig(H=8, W=8, C=1, L=2, K=1, F=128)
    eng, _ = calibrated_engine(cfg, device=0, init_tiles=8)
    flow = GlowFlow(eng)
    n, seed = 5, 11
    shape = (n,) + tuple(cfg.latent_shape())
    eps = basis.device_randn(shape, "cuda", seed, step=0, which=3)
    assert np.abs(eps.cpu().numpy().reshape(-1) - R.normal(seed, 0, 3, 0, 0, eps.numel())).max() <= NORMAL_BAR
    x = flow.sample(n, seed)
    assert torch.isfinite(x).all() and torch.equal(x, eng.sample_from_eps(eps)) and torch.equal(x, flow.sample(n, seed))
    assert not torch.equal(x, flow.sample(n, seed + 1))
    assert not torch.equal(flow.sample(n), flow.sample(n))                         # unseeded: a fresh stream per call


def test_streams_end_at_element_2_to_the_62():
    """From element 2^62 on hi32(q) would reach the bits of `which` in c1: refused by all four entry points, before a launch; the
    last four elements below it are still the restatement's."""
    last = 2 ** 62 - 4
    assert np.array_equal(basis.device_randn((4,), "cuda", 7, which=5, uniform=True, offset=last).cpu().numpy(),
                          R.uniform(7, which=5, offset=last, n=4))
    for kw in (dict(offset=last, n=5), dict(offset=2 ** 62, n=4), dict(offset=2 ** 64 - 4, n=8), dict(offset=2 ** 62 + 4, n=1)):
        for pair in (0, 1):
            with pytest.raises(_lib.GlowkError, match="2\\^62"):
                basis.device_randn((kw["n"],), "cuda", 7, offset=kw["offset"], pair=pair)
        x = torch.zeros(kw["n"], device="cuda")
        with pytest.raises(_lib.GlowkError, match="2\\^62"):
            basis.add_device_noise(x, 1.0, 7, offset=kw["offset"])
        xs = [torch.zeros(kw["n"], device="cuda") for _ in range(2)]
        with pytest.raises(_lib.GlowkError, match="2\\^62"):
            basis.langevin_update_n(x, xs, [torch.ones_like(x)] * 2, ETA, LAM, seed=7, offset=kw["offset"])
        assert all(float(t.abs().max()) == 0.0 for t in xs)                        # nothing was launched
