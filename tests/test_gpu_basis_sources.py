"""BASIS for any number of sources on the GPU: ``glowk_basis_update_n`` / ``glowk_basis_mix_n`` / ``glowk_random_source`` against
the float64 formulas, their bitwise properties, the S-source loop against an fp64 oracle loop (tests/basis_sources_ref.py) and
``audio.separate_sources`` end to end; the two-source entry points against the recorded results of the kernels they had."""
import ctypes
import os

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, audio, basis
from audiosourcesep_amd.config import GlowConfig
from audiosourcesep_amd.synthetic import synthetic_mel_tiles
from tests import basis_sources_ref as ref

pytestmark = pytest.mark.gpu
SHAPE = (7, 16, 12, 1)            # 1344 elements: not a multiple of the 1024-element workgroup
ETA, LAM = 2e-5 * 37.0, 1.0 / 0.3 ** 2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def offset_view(a):
    """The same values in a buffer that starts one float past an allocation: no pointer of it is 16-byte aligned."""
    t = dev(a)
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def draw(S, shape=SHAPE, seed=5):
    rng = np.random.default_rng(seed)
    xs = rng.uniform(-80, 10, (S,) + shape)
    mixed = rng.uniform(-80, 10, shape)
    gs = rng.normal(0, 5, (S,) + shape)
    eps = rng.standard_normal((S,) + shape)
    return mixed, list(xs), list(gs), list(eps)


@pytest.mark.parametrize("S,process,unaligned", [(S, p, False) for p in ("db", "mean") for S in (2, 3, 5, 16)] + [(3, "db", True)])
def test_update_kernel_against_the_formulas(S, process, unaligned):
    """glowk_basis_update_n == run_basis_sep.py:163-181 for S sources written out in float64, with injected noise: whole quads as
    16-byte accesses (1344 elements end inside the second workgroup), and element by element from buffers offset by one float
    (test_partial_last_quad covers a last thread with fewer than four elements).  glowk_basis_mix_n against g alone; S = 2 bit for
    bit against the two-source entry points."""
    put = offset_view if unaligned else dev
    mixed, xs, gs, eps = draw(S)
    want = ref.update(mixed, xs, gs, eps, ETA, LAM, process)
    mix = basis.mixing([put(x) for x in xs], process)
    err = float(np.abs(mix.cpu().numpy() - ref.g(xs, process)).max())
    print("S=%d %s: mix max |d| %.3e" % (S, process, err))
    np.testing.assert_allclose(mix.cpu().numpy(), ref.g(xs, process), rtol=2e-6, atol=2e-5)
    ys = [put(x) for x in xs]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    basis.langevin_update_n(put(mixed), ys, [put(g) for g in gs], ETA, LAM, [put(e) for e in eps], nonfinite=flag, mixing=process)
    print("S=%d %s: update max |d| %.3e" % (S, process, max(float(np.abs(y.cpu().numpy() - w).max()) for y, w in zip(ys, want))))
    for y, w in zip(ys, want):
        np.testing.assert_allclose(y.cpu().numpy(), w, rtol=1e-5, atol=1e-4)
    assert int(flag.item()) == 0
    if S == 2 and process == "db":
        z1, z2 = dev(xs[0]), dev(xs[1])
        basis.langevin_update(dev(mixed), z1, z2, dev(gs[0]), dev(gs[1]), ETA, LAM, dev(eps[0]), dev(eps[1]))
        assert torch.equal(ys[0], z1) and torch.equal(ys[1], z2)
        assert torch.equal(mix, basis.mixing_db(dev(xs[0]), dev(xs[1])))


def test_partial_last_quad():
    """n = 1343: the last thread holds three elements and must neither read nor write the fourth."""
    S, n = 3, 1343
    mixed, xs, gs, eps = draw(S, shape=(n + 1,), seed=6)
    want = ref.update(mixed, xs, gs, eps, ETA, LAM)
    full = [dev(x) for x in xs]
    ys = [f[:n] for f in full]
    basis.langevin_update_n(dev(mixed)[:n], ys, [dev(g)[:n] for g in gs], ETA, LAM, [dev(e)[:n] for e in eps])
    for f, x, w in zip(full, xs, want):
        np.testing.assert_allclose(f[:n].cpu().numpy(), w[:n], rtol=1e-5, atol=1e-4)
        assert float(f[n]) == np.float32(x[n])


def test_two_sources_reproduce_the_recorded_two_source_kernels():
    """tests/golden/basis_two_source.npz holds what k_basis_update / k_basis_mix, the two-source kernels that the S = 2 instance
    replaced, returned on an MI355X at the last commit that had them (tests/golden/basis_two_source.md): n = 1343 elements (a
    full workgroup, a second one, a last thread with three elements), states in [-100, 20] dB with equal pairs and pairs more
    than 100 dB apart.  Both update entry points and both mixture entry points return those bits: with injected noise, with the
    device RNG at a stream offset, and from buffers offset by one float, which go element by element."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "basis_two_source.npz"))
    eta, lam = float(z["eta"]), float(z["lambda_recon"])
    assert z["x1"].shape == (1343,) and int((z["x1"] == z["x2"]).sum()) >= 40 and int((np.abs(z["x1"] - z["x2"]) > 100.0).sum()) >= 60
    for case, put, inject, kw in (("injected", dev, True, {}), ("device_rng", dev, False, dict(seed=99, step=5, offset=8)),
                                  ("offset", offset_view, True, {})):
        want = [dev(z[case + "_y1"]), dev(z[case + "_y2"])]
        eps = [put(z["eps1"]), put(z["eps2"])] if inject else [None, None]
        a, b = put(z["x1"]), put(z["x2"])
        basis.langevin_update(put(z["mixed"]), a, b, put(z["g1"]), put(z["g2"]), eta, lam, eps[0], eps[1], **kw)
        assert torch.equal(a, want[0]) and torch.equal(b, want[1]), case
        ys = [put(z["x1"]), put(z["x2"])]
        basis.langevin_update_n(put(z["mixed"]), ys, [put(z["g1"]), put(z["g2"])], eta, lam, eps if inject else None, **kw)
        assert torch.equal(ys[0], want[0]) and torch.equal(ys[1], want[1]), case
    a, b, mix = dev(z["x1"]), dev(z["x2"]), dev(z["mix"])
    assert torch.equal(basis.mixing_db(a, b), mix) and torch.equal(basis.mixing([a, b]), mix)
    out = torch.empty_like(a)                                  # (mixing_db goes through glowk_basis_mix_n: the C entry itself)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert _lib.load().glowk_basis_mix(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                       a.numel(), st) == _lib.OK
    assert torch.equal(out, mix)


def source_draw(k, shape, seed, step, offset=0):
    return basis.device_randn(shape, "cuda", seed, step, which=k & 1, pair=k >> 1, offset=offset)


def test_bitwise_properties_of_the_update():
    S = 5
    mixed, xs, gs, eps = draw(S)
    m, g = dev(mixed), [dev(a) for a in gs]

    def run(e, **kw):
        ys = [dev(x) for x in xs]
        basis.langevin_update_n(m, ys, g, ETA, LAM, e, **kw)
        return ys

    # the same call twice
    a, b = run(None, seed=99, step=5), run(None, seed=99, step=5)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # the device RNG == injecting the draws glowk_random_source reports for source k
    rep = [source_draw(k, SHAPE, 99, 5) for k in range(S)]
    c = run(rep)
    assert all(torch.equal(p, q) for p, q in zip(a, c))
    assert not any(torch.equal(p, q) for p, q in zip(a, run(None, seed=99, step=6)))
    assert not any(torch.equal(p, q) for p, q in zip(a, run(None, seed=98, step=5)))
    # sources 0 and 1 draw what the two-source path draws
    assert torch.equal(rep[0], basis.device_randn(SHAPE, "cuda", 99, 5, 0)) and torch.equal(rep[1], basis.device_randn(SHAPE, "cuda", 99, 5, 1))
    # some entries given, some NULL: each source follows its own entry
    given = [dev(eps[0]), None, dev(eps[2]), None, None]
    d = run(given, seed=99, step=5)
    e = run([given[k] if given[k] is not None else rep[k] for k in range(S)])
    assert all(torch.equal(p, q) for p, q in zip(d, e))
    # (the mixture term depends on the incoming states only: a source left to the device RNG ends where it ended in the all-device run)
    assert all(torch.equal(d[k], a[k]) for k in (1, 3, 4)) and not torch.equal(d[0], a[0]) and not torch.equal(d[2], a[2])


def test_a_shard_equals_its_slice_of_the_whole_batch():
    S, E = 3, 16 * 16
    rng = np.random.default_rng(2)
    mk = lambda scale=1.0: dev(rng.uniform(-80, 10, (12, 16, 16, 1)) * scale)   # noqa: E731
    mixed, xs, gs = mk(), [mk() for _ in range(S)], [mk(0.01) for _ in range(S)]
    whole = [x.clone() for x in xs]
    basis.langevin_update_n(mixed, whole, gs, 1e-3, 4.0, seed=77, step=3)
    for a, b in ((0, 5), (5, 9), (9, 12)):                                       # three ragged shards
        part = [x[a:b].clone().contiguous() for x in xs]
        basis.langevin_update_n(mixed[a:b].contiguous(), part, [g[a:b].contiguous() for g in gs], 1e-3, 4.0, seed=77, step=3, offset=a * E)
        assert all(torch.equal(p, w[a:b]) for p, w in zip(part, whole))
    assert not torch.equal(whole[0][0:4] - xs[0][0:4], whole[0][4:8] - xs[0][4:8])


def test_source_streams():
    """glowk_random_source: pair 0 is glowk_random; the 16 sources' draws at one (seed, step) are pairwise different and
    uncorrelated (|mean(a b)| < 5 / sqrt(n), the criterion of the existing stream test)."""
    n = 1 << 20
    lib = _lib.load()
    for which in (0, 1, 14, 15):
        for uniform in (0, 1):
            a = basis.device_randn((n,), "cuda", seed=1234, step=7, which=which, uniform=bool(uniform))
            b = torch.empty_like(a)
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            assert lib.glowk_random_source(ctypes.c_void_p(b.data_ptr()), n, 1234, 7, which, 0, uniform, 0, st) == 0
            assert torch.equal(a, b)
    # a step at and above 2^32 (its high word is where the pair goes): still glowk_random for pair 0, and pairs stay apart
    a = basis.device_randn((4096,), "cuda", seed=1, step=(1 << 32) + 3, which=0)
    b = basis.device_randn((4096,), "cuda", seed=1, step=(1 << 32) + 3, which=0, pair=1)
    c = basis.device_randn((4096,), "cuda", seed=1, step=3, which=0, pair=1)
    assert not torch.equal(a, b) and not torch.equal(b, c) and torch.isfinite(b).all()
    Z = torch.stack([source_draw(k, (n,), 1234, 7) for k in range(16)]).double()
    m, v = Z.mean(1), Z.var(1)
    assert float(m.abs().max()) < 5.0 / n ** 0.5 and float((v - 1.0).abs().max()) < 1e-2
    G = (Z @ Z.T / n).cpu().numpy()
    off = np.abs(G - np.diag(np.diag(G)))
    print("source streams: worst |mean(a b)| %.3e (bound %.3e)" % (off.max(), 5.0 / n ** 0.5))
    assert off.max() < 5.0 / n ** 0.5
    for k in range(16):
        for l in range(k):
            assert not torch.equal(Z[k], Z[l])
    # the uniform start states of separate_sources (streams 14 / 15) are apart in the same way
    U = torch.stack([basis.device_randn((n,), "cuda", seed=3, which=14 + (k & 1), uniform=True, pair=k >> 1) for k in range(4)]).double() - 0.5
    Gu = (U @ U.T / n).cpu().numpy() * 12.0
    assert np.abs(Gu - np.diag(np.diag(Gu))).max() < 5.0 / n ** 0.5 and float(U.min()) > -0.5 and float(U.max()) < 0.5


def _raw_update(xs, gs, mixed, nsrc=None, eps=None, mixing=0, step=0, offset=0, n=None, flag=None):
    nsrc = len(xs) if nsrc is None else nsrc
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _lib.load().glowk_basis_update_n(basis._ptrs(xs), basis._ptrs(gs), basis._ptrs(eps) if eps is not None else None, nsrc,
                                            ctypes.c_void_p(mixed.data_ptr()), xs[0].numel() if n is None else n, mixing, ETA, LAM, 1, step,
                                            offset, ctypes.c_void_p(flag.data_ptr()) if flag is not None else None, st)


def test_flag_and_argument_checks():
    S = 5
    mixed, xs, gs, eps = draw(S)
    m, g, e = dev(mixed), [dev(a) for a in gs], [dev(a) for a in eps]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    basis.langevin_update_n(m, [dev(x) for x in xs], g, ETA, LAM, e, nonfinite=flag)
    assert int(flag.item()) == 0
    basis.langevin_update_n(m, [dev(x) for x in xs], g, ETA, LAM, None, nonfinite=flag)
    assert int(flag.item()) == 0
    gbad = [t.clone() for t in g]
    gbad[3][3, 2, 1, 0] = float("nan")
    basis.langevin_update_n(m, [dev(x) for x in xs], gbad, ETA, LAM, e, nonfinite=flag)
    assert int(flag.item()) == 1
    flag.zero_()
    gbad[3][3, 2, 1, 0] = float("inf")
    basis.langevin_update_n(m, [dev(x) for x in xs], gbad, ETA, LAM, e, nonfinite=flag, mixing="mean")
    assert int(flag.item()) == 1
    # refused before anything is launched
    x = [dev(a) for a in xs]
    keep = [t.clone() for t in x]
    more = [torch.zeros_like(m) for _ in range(17)]
    assert _raw_update(x, g, m) == _lib.OK
    x = [t.clone() for t in keep]
    assert _raw_update(x[:1], g[:1], m) == _lib.ERR                               # one source
    assert _raw_update(more, more, m) == _lib.ERR                                 # seventeen
    assert _raw_update([x[0], x[1], x[0]], g[:3], m) == _lib.ERR                  # a repeated state
    assert _raw_update([x[0], m, x[2]], g[:3], m) == _lib.ERR                     # a state that is the mixture
    assert _raw_update(x, g, m, offset=2) == _lib.ERR
    assert _raw_update(x, g, m, step=1 << 48) == _lib.ERR
    assert _raw_update(x, g, m, mixing=2) == _lib.ERR and _raw_update(x, g, m, mixing=-1) == _lib.ERR
    assert b"mixing" in _lib.load().glowk_last_error()
    assert all(torch.equal(a, b) for a, b in zip(x, keep))                        # nothing was launched
    assert _raw_update(x, g, m, step=(1 << 48) - 1) == _lib.OK
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty_like(m)
    assert _lib.load().glowk_basis_mix_n(basis._ptrs(x[:1]), 1, ctypes.c_void_p(out.data_ptr()), m.numel(), 0, st) == _lib.ERR
    assert _lib.load().glowk_basis_mix_n(basis._ptrs(more), 17, ctypes.c_void_p(out.data_ptr()), m.numel(), 0, st) == _lib.ERR
    assert _lib.load().glowk_basis_mix_n(basis._ptrs(x), 5, ctypes.c_void_p(out.data_ptr()), m.numel(), 3, st) == _lib.ERR
    with pytest.raises(_lib.GlowkError):
        basis.langevin_update_n(m, [x[0], x[0]], g[:2], ETA, LAM)
    with pytest.raises(_lib.GlowkError):
        basis.langevin_update(m, x[0], x[0], g[0], g[1], ETA, LAM)                # the two-source entry makes the same checks
    with pytest.raises(_lib.GlowkError):
        basis.langevin_update(m, x[0], x[1], g[0], g[1], ETA, LAM, step=1 << 48)
    with pytest.raises(_lib.GlowkError):
        basis.device_randn((8,), "cuda", seed=1, step=1 << 48, pair=1)
    with pytest.raises(ValueError):
        basis.langevin_update_n(m, x, g, ETA, LAM, mixing="power")
    with pytest.raises(ValueError):
        basis.langevin_update_n(m, [t[:, ::2] for t in x], g, ETA, LAM)           # in place needs contiguous states


# ---- the loop ------------------------------------------------------------------------------------------------------------------------
CFG = GlowConfig(H=16, W=16, C=1, L=2, K=3, F=128)
N_TILES, T_STEPS, SIDX = 4, 3, 9


@pytest.fixture(scope="module")
def priors():
    from audiosourcesep_amd.flow_models.flow_glow import GlowFlow
    from audiosourcesep_amd.synthetic import calibrated_engine
    made = [calibrated_engine(CFG, device=0, init_tiles=16, seed=s) for s in (1, 2, 3)]
    return [GlowFlow(e) for e, _ in made], [p for _, p in made]


@pytest.fixture(scope="module")
def problem(priors):
    """Start states, mixture, noise and the float64 loop's result: computed once, read by both arithmetics."""
    truth = [synthetic_mel_tiles(N_TILES, CFG, seed=10 + k).astype(np.float64) for k in range(3)]
    mixed = ref.g(truth)
    xs = [synthetic_mel_tiles(N_TILES, CFG, seed=20 + k).astype(np.float64) for k in range(3)]
    noise = np.random.default_rng(3).standard_normal((T_STEPS, 3) + xs[0].shape)
    sigmas = basis.get_sigmas(1.0, 0.01, 10)
    want = ref.inner_loop(mixed, xs, priors[1], CFG.as_dict(), SIDX, sigmas, noise, T=T_STEPS)
    for a in [mixed, noise] + xs + want:
        a.setflags(write=False)
    return mixed, xs, noise, sigmas, want


@pytest.mark.parametrize("arith", ["f32", "f16x3"])
def test_three_source_loop_matches_the_fp64_loop(priors, problem, arith):
    flows, _ = priors
    mixed, xs, noise, sigmas, want = problem
    saved = [(f.engine.get_precision(), int(f.engine.lib.glowk_get_range_policy(f.engine.h))) for f in flows]
    try:
        if arith == "f16x3":
            for f in flows:
                f.engine.set_precision(_lib.PREC_F16X3)
                f.engine.set_range_policy("error")
        got = basis.basis_inner_loop_n(dev(mixed), [dev(x) for x in xs], flows, SIDX, sigmas, T=T_STEPS, debug=True,
                                       noise_fn=lambda t, k, shape: dev(noise[t][k]))
        assert isinstance(got, list) and len(got) == 3
        print("%s: max |d| to the fp64 loop %.3e dB" % (arith, max(float(np.abs(y.cpu().numpy() - w).max()) for y, w in zip(got, want))))
        for y, w, x in zip(got, want, xs):
            np.testing.assert_allclose(y.cpu().numpy(), w, atol=2e-3)                  # dB units, range 120
            assert np.abs(w - x).max() > 1e-3                                          # the update moved the state
        # one stream for all three gives the same numbers
        seq = basis.basis_inner_loop_n(dev(mixed), [dev(x) for x in xs], flows, SIDX, sigmas, T=T_STEPS, streams=None,
                                       noise_fn=lambda t, k, shape: dev(noise[t][k]))
        assert all(torch.equal(a, b) for a, b in zip(got, seq))
        out, arr = basis.basis_outer_loop_n(dev(mixed), [dev(x) for x in xs], flows, sigmas[-2:], T=2,
                                            restores=[{float(s): flows[0].state_dict() for s in sigmas[-2:]}, None, None])
        assert len(out) == 3 and all(bool(torch.isfinite(o).all()) for o in out)
        assert sorted(arr) == ["x1", "x2", "x3"] and all(len(v) == 3 for v in arr.values())
    finally:
        for f, (prec, pol) in zip(flows, saved):
            f.engine.set_precision(prec)
            f.engine.set_range_policy(pol)


def test_loop_with_the_device_rng_is_reproducible_and_leaves_inputs_alone(priors, problem):
    flows, _ = priors
    mixed, xs, _, sigmas, _ = problem
    m, x = dev(mixed), [dev(a) for a in xs]
    keep = [t.clone() for t in x]
    a = basis.basis_inner_loop_n(m, x, flows, SIDX, sigmas, T=3, seed=4, debug=True)
    b = basis.basis_inner_loop_n(m, x, flows, SIDX, sigmas, T=3, seed=4)
    c = basis.basis_inner_loop_n(m, x, flows, SIDX, sigmas, T=3, seed=5)
    assert all(torch.equal(p, q) for p, q in zip(x, keep))
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and not any(torch.equal(p, q) for p, q in zip(a, c))
    assert all(bool(torch.isfinite(p).all()) for p in a) and float((a[2] - x[2]).abs().max()) > 1e-3
    # a prior that serves two sources is evaluated for both, one after the other
    d = basis.basis_inner_loop_n(m, x, [flows[0], flows[1], flows[0]], SIDX, sigmas, T=2, seed=4)
    e = basis.basis_inner_loop_n(m, x, [flows[0], flows[1], flows[0]], SIDX, sigmas, T=2, seed=4, streams=None)
    assert all(torch.equal(p, q) for p, q in zip(d, e))


# ---- audio ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def audio_flows():
    from audiosourcesep_amd.flow_models.flow_glow import GlowFlow
    from audiosourcesep_amd.synthetic import calibrated_engine
    cfg = GlowConfig(H=96, W=64, C=1, L=2, K=1, F=128)
    return [GlowFlow(calibrated_engine(cfg, device=0, init_tiles=8, seed=50 + k)[0]) for k in range(3)]


def synthetic_audio():
    rng = np.random.default_rng(8)
    t = np.arange(2 * audio.EXTRACT) / 16000.0
    y = 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * (200.0 * t + 900.0 * t * t)) + 0.1 * np.sign(np.sin(2 * np.pi * 150.0 * t))
    return (y + 0.01 * rng.standard_normal(t.shape)).astype(np.float32)


def test_separate_sources_end_to_end(audio_flows):
    y = synthetic_audio()
    sig = np.array([20.0, 5.0], np.float32)
    kw = dict(T=2, delta=1e-4, seed=9)
    ys, mixed, xs = audio.separate_sources(y, audio_flows, sig, **kw)
    assert tuple(ys.shape) == (3, 2 * 32256) and tuple(xs.shape) == (3, 2, 96, 64, 1) and tuple(mixed.shape) == (2, 96, 64, 1)
    assert bool(torch.isfinite(ys).all()) and bool(torch.isfinite(xs).all())
    ys2, _, xs2 = audio.separate_sources(y, audio_flows, sig, **kw)
    assert torch.equal(ys, ys2) and torch.equal(xs, xs2)
    ys3, _, xs3 = audio.separate_sources(y, audio_flows, sig, T=2, delta=1e-4, seed=10)
    assert not torch.equal(xs, xs3) and not torch.equal(ys, ys3)
    # two flows: the two-source signature's tiles (same start states, same noise, the same loop and kernel)
    y1, y2, m2, x1, x2 = audio.separate_audio(y, audio_flows[0], audio_flows[1], sig, **kw)
    yp, mp, xp = audio.separate_sources(y, audio_flows[:2], sig, **kw)
    assert torch.equal(mp, m2) and tuple(yp.shape) == (2, 2 * 32256)
    print("two flows: tiles max |d| to separate_audio %.3e dB" % max(float((xp[0] - x1).abs().max()), float((xp[1] - x2).abs().max())))
    np.testing.assert_allclose(xp[0].cpu().numpy(), x1.cpu().numpy(), atol=2e-3)
    np.testing.assert_allclose(xp[1].cpu().numpy(), x2.cpu().numpy(), atol=2e-3)
    with pytest.raises(ValueError):
        audio.separate_sources(y, audio_flows[:1], sig, **kw)


def test_separate_wav_sources_resamples_all_outputs(audio_flows, tmp_path):
    y = synthetic_audio()
    y8 = audio.resample(y, 16000, 8000).cpu().numpy()
    path = tmp_path / "mix8k.wav"
    audio.save_audio(path, y8, 8000)
    sig = np.array([20.0, 5.0], np.float32)
    ys, mixed, xs, rate = audio.separate_wav_sources(str(path), audio_flows, sig, T=1, delta=1e-4, seed=9)
    n16 = xs.shape[1] * 32256
    assert rate == 8000 and tuple(xs.shape[0:1]) == (3,) and tuple(ys.shape) == (3, n16 // 2) and bool(torch.isfinite(ys).all())
    ys16, *_, rate16 = audio.separate_wav_sources(str(path), audio_flows, sig, out_rate=None, T=1, delta=1e-4, seed=9)
    assert rate16 == 16000 and tuple(ys16.shape) == (3, n16)
    with pytest.raises(ValueError):
        audio.separate_wav_sources(str(path), audio_flows, sig, out_rate="native")
