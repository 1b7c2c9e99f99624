"""BASIS as one chain over a whole signal's frames on the GPU (csrc/glowk_frames.h through ``basis.cut_frames`` /
``langevin_update_frames`` / ``basis_inner_loop_frames`` / ``basis_outer_loop_frames`` and ``audio.separate_long(coupled=True)``)
against the fp64 restatement of tests/frames_chain_ref.py, against the per-tile chain where the two must coincide, and by the
bitwise properties of the update kernel whose device code it shares.

Bars.  Cut: bitwise (a gather).  Update: ``rtol=1e-5, atol=1e-4``, the bar of the S-source update (tests/test_gpu_basis_sources.py);
the stitch in front of it adds at most eta 2^-15 max|g| (``STITCH_BAR`` of tests/test_gpu_longform.py times the step size), which at
eta = 7.4e-4 and |g| <= 30 is below 1e-6.  Loop: ``atol=2e-3`` dB, the bar of the S-source loop for the same priors, depth and step
count."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib, audio, basis
from audiosourcesep_amd.config import GlowConfig
from audiosourcesep_amd.synthetic import synthetic_mel_tiles
from tests import basis_sources_ref as ref
from tests import frames_chain_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ETA, LAM = 2e-5 * 37.0, 1.0 / 0.3 ** 2
LONG_CASES = [(5, 32), (64, 32), (65, 32), (100, 32), (138, 32), (138, 48), (70, 1), (138, 64)]   # tests/test_gpu_longform.py::CASES
# (rows, width, F, hop): frames under 4 tiles and a short last tile; disjoint tiles; one tile wider than the signal; an exact fit
SMALL = [(16, 16, 37, 5), (16, 16, 16, 16), (16, 16, 7, 8), (16, 16, 40, 8)]
TILE = (96, 64, 138, 32)                                                                           # the front end's geometry


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


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---- cut -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,width,F,hop", [(96, 64, F, hop) for F, hop in LONG_CASES] + [(16, 16, 37, 5)])
def test_cut_frames_bitwise(rows, width, F, hop):
    rng = np.random.default_rng(1000 * F + 10 * hop + width)
    x = rng.uniform(-150.0, 50.0, (3, rows, F)).astype(np.float32)                 # far outside [-100, 20]: nothing may be clipped
    N = R.tile_count(F, width, hop)
    for pad in (-100.0, -77.5):
        tiles = basis.cut_frames(dev(x), width, hop, pad=pad)
        assert tuple(tiles.shape) == (3, N, rows, width) and tiles.dtype == torch.float32 and tiles.is_cuda
        tiles = tiles.cpu().numpy()
        assert np.array_equal(tiles, R.cut(x, width, hop, pad=pad, dtype=np.float32))
        reach = (N - 1) * hop + width - F
        assert reach == 0 or (tiles[:, -1, :, width - reach:] == np.float32(pad)).all()        # the cells past the signal's end
    assert float(tiles.min()) < -100.0 and float(tiles.max()) > 20.0
    one = basis.cut_frames(dev(x[1]), width, hop)
    assert tuple(one.shape) == (N, rows, width) and np.array_equal(one.cpu().numpy(), R.cut(x[1], width, hop, dtype=np.float32))


# ---- the update kernel against the fp64 formulas ---------------------------------------------------------------------------------------
def draw(S, rows, width, F, hop, seed=5):
    """float32-representable states, mixture, gradient tiles (pad cells included) and noise, as float64."""
    rng = np.random.default_rng(seed + 7 * F + hop)
    N = R.tile_count(F, width, hop)
    xs = f32(rng.uniform(-80, 10, (S, rows, F)))
    mixed = f32(rng.uniform(-80, 10, (rows, F)))
    gs = f32(rng.normal(0, 5, (S, N, rows, width)))
    eps = f32(rng.standard_normal((S, rows, F)))
    return mixed, xs, gs, eps


@pytest.mark.parametrize("rows,width,F,hop,unaligned", [g + (False,) for g in SMALL + [TILE]] + [(16, 16, 37, 5, True)])
@pytest.mark.parametrize("process", ["db", "mean"])
@pytest.mark.parametrize("S", [2, 3, 16])
def test_update_kernel_against_the_formulas(S, process, rows, width, F, hop, unaligned):
    """glowk_basis_update_frames == the stitched score and run_basis_sep.py:163-181 written out in float64, with injected noise and
    gradient tiles.  The bar is the S-source update's, rtol 1e-5 and atol 1e-4; the fp32 stitch adds at most eta 2^-15 max|g| <
    1e-6 to it.  rows F is 592 (whole 16-byte quads that run over row ends), 256, 112, 640 and 13 248; from buffers offset by one
    float every access goes element by element.  ``tiles_out`` is the cut of the updated states, bit for bit, pad cells included."""
    put = offset_view if unaligned else dev
    mixed, xs, gs, eps = draw(S, rows, width, F, hop)
    want = R.update(mixed, list(xs), list(gs), list(eps), hop, ETA, LAM, process)
    x = put(xs)
    tiles = put(np.full(gs.shape, 1e30))                                           # every cell has to be overwritten
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    basis.langevin_update_frames(put(mixed), x, [put(g)[..., None] for g in gs], width, hop, ETA, LAM, [put(e) for e in eps],
                                 nonfinite=flag, mixing=process, tiles_out=tiles)
    got = x.cpu().numpy()
    worst = max(float(np.abs(got[k] - want[k]).max()) for k in range(S))
    print("S=%d %s rows=%d W=%d F=%d hop=%d%s: update max |d| %.3e (bar 1e-4 + 1e-5 |x|)" % (S, process, rows, width, F, hop,
                                                                                             " unaligned" if unaligned else "", worst))
    for k in range(S):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-5, atol=1e-4)
    assert int(flag.item()) == 0 and float(np.abs(got - xs).max()) > 1e-2
    assert np.array_equal(tiles.cpu().numpy(), R.cut(got, width, hop, dtype=np.float32))
    assert torch.equal(tiles, basis.cut_frames(x, width, hop))
    # without tiles_out the states are the same
    y = put(xs)
    basis.langevin_update_frames(put(mixed), y, [put(g) for g in gs], width, hop, ETA, LAM, [put(e) for e in eps], mixing=process)
    assert torch.equal(x, y)


# ---- bitwise properties ----------------------------------------------------------------------------------------------------------------
def test_bitwise_properties_of_the_update():
    S, (rows, width, F, hop) = 5, SMALL[0]
    mixed, xs, gs, eps = draw(S, rows, width, F, hop)
    m, g = dev(mixed), [dev(a) for a in gs]

    def run(e, **kw):
        y = dev(xs)
        basis.langevin_update_frames(m, y, g, width, hop, ETA, LAM, e, **kw)
        return y

    a, b = run(None, seed=99, step=5), run(None, seed=99, step=5)
    assert torch.equal(a, b)
    # the device RNG == injecting the draws glowk_random_source reports for source k: element b F + f of the stream at offset 0
    rep = [basis.device_randn((rows, F), "cuda", 99, 5, which=k & 1, pair=k >> 1) for k in range(S)]
    assert torch.equal(a, run(rep))
    for other in (run(None, seed=99, step=6), run(None, seed=98, step=5)):
        assert not any(torch.equal(a[k], other[k]) for k in range(S))
    # a supplied eps for one source changes that source only
    d = run([None, None, dev(eps[2]), None, None], seed=99, step=5)
    assert all(torch.equal(d[k], a[k]) for k in (0, 1, 3, 4)) and not torch.equal(d[2], a[2])
    assert torch.equal(d, run([rep[0], rep[1], dev(eps[2]), rep[3], rep[4]]))


@pytest.mark.parametrize("process", ["db", "mean"])
@pytest.mark.parametrize("S", [2, 5])
def test_disjoint_tiles_equal_the_tile_update_bit_for_bit(S, process):
    """hop = W, F = 3 W: every frame has one tile, whose gradient is taken as it is, and the update expression is the device code
    of k_basis_update_n: one call equals ``langevin_update_n`` on the tile-layout permutation of the same inputs."""
    rows, width = 16, 16
    F = 3 * width
    mixed, xs, gs, eps = draw(S, rows, width, F, width)
    perm = lambda a: dev(R.tiles_of_frames(a, width))                              # noqa: E731
    x = dev(xs)
    basis.langevin_update_frames(dev(mixed), x, [dev(g) for g in gs], width, width, ETA, LAM, [dev(e) for e in eps], mixing=process)
    ys = [perm(a) for a in xs]
    basis.langevin_update_n(perm(mixed), ys, [dev(g) for g in gs], ETA, LAM, [perm(e) for e in eps], mixing=process)
    for k in range(S):
        assert torch.equal(perm(x[k].cpu().numpy()), ys[k])


# ---- flag and argument checks ----------------------------------------------------------------------------------------------------------
def raw_update(x, gs, mixed, rows, F, width, hop, nsrc=None, eps=None, mixing=0, eta=ETA, step=0, pad=-100.0, tiles_out=None, flag=None):
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _lib.load().glowk_basis_update_frames(p(x), basis._ptrs(gs), basis._ptrs(eps) if eps is not None else None,
                                                 len(gs) if nsrc is None else nsrc, p(mixed), rows, F, width, hop, mixing, eta, LAM, 1, step, pad,
                                                 p(tiles_out), p(flag), st)


def test_flag_and_argument_checks():
    S, (rows, width, F, hop) = 3, SMALL[0]
    mixed, xs, gs, eps = draw(S, rows, width, F, hop)
    N = R.tile_count(F, width, hop)
    m, g, e = dev(mixed), [dev(a) for a in gs], [dev(a) for a in eps]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for noise in (e, None):
        basis.langevin_update_frames(m, dev(xs), g, width, hop, ETA, LAM, noise, nonfinite=flag)
        assert int(flag.item()) == 0
    # a non-finite gradient in a cell that a frame reads raises the flag; one in a pad cell is dropped with the cell
    for value, process in ((float("nan"), "db"), (float("inf"), "mean")):
        gbad = [t.clone() for t in g]
        gbad[1][2, 3, 4] = value
        flag.zero_()
        basis.langevin_update_frames(m, dev(xs), gbad, width, hop, ETA, LAM, e, nonfinite=flag, mixing=process)
        assert int(flag.item()) == 1
    assert (N - 1) * hop + width > F
    gpad = [t.clone() for t in g]
    gpad[1][N - 1, 3, width - 1] = float("nan")
    flag.zero_()
    y = dev(xs)
    basis.langevin_update_frames(m, y, gpad, width, hop, ETA, LAM, e, nonfinite=flag)
    z = dev(xs)
    basis.langevin_update_frames(m, z, g, width, hop, ETA, LAM, e)
    assert int(flag.item()) == 0 and torch.equal(y, z)
    mbad = m.clone()
    mbad[0, 0] = float("inf")
    basis.langevin_update_frames(mbad, dev(xs), g, width, hop, ETA, LAM, e, nonfinite=flag)
    assert int(flag.item()) == 1
    # refused before anything is launched
    x = dev(xs)
    keep = x.clone()
    tiles = torch.zeros((S, N, rows, width), device="cuda")
    many = [torch.zeros_like(g[0]) for _ in range(17)]

    def ok(gs=g, mixed=m, **kw):
        geometry = [kw.pop(name, value) for name, value in (("rows", rows), ("F", F), ("width", width), ("hop", hop))]
        return raw_update(x, gs, mixed, *geometry, **kw)

    assert ok(gs=g[:1]) == _lib.ERR and ok(gs=many) == _lib.ERR                    # one source, seventeen
    assert ok(rows=0) == _lib.ERR and ok(rows=65537) == _lib.ERR
    assert ok(F=0) == _lib.ERR and ok(F=(1 << 20) + 1) == _lib.ERR
    assert ok(width=1, hop=1) == _lib.ERR and ok(width=129) == _lib.ERR
    assert ok(hop=0) == _lib.ERR and ok(hop=width + 1) == _lib.ERR
    assert b"hop" in _lib.load().glowk_last_error()
    assert ok(step=1 << 48) == _lib.ERR and ok(mixing=2) == _lib.ERR and ok(mixing=-1) == _lib.ERR
    assert ok(eta=-1.0) == _lib.ERR and ok(pad=float("nan")) == _lib.ERR
    assert ok(mixed=x[0]) == _lib.ERR                                              # the mixture inside the states
    assert ok(gs=[g[0], x.reshape(-1)[:g[1].numel()], g[2]]) == _lib.ERR             # a gradient inside the states
    assert ok(tiles_out=x) == _lib.ERR and ok(tiles_out=g[0]) == _lib.ERR          # tiles_out over the states, over a gradient
    assert ok(gs=[g[0], None, g[2]]) == _lib.ERR
    assert ok(gs=[g[0], torch.zeros(g[0].shape), g[2]]) == _lib.ERR                # a host pointer
    assert torch.equal(x, keep) and not bool(tiles.any())                          # nothing was launched
    assert ok(step=(1 << 48) - 1, tiles_out=tiles) == _lib.OK and not torch.equal(x, keep)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cut = lambda rows_=rows, F_=F, width_=width, hop_=hop, pad=-100.0, out=tiles: _lib.load().glowk_frames_to_tiles(   # noqa: E731
        ctypes.c_void_p(keep.data_ptr()), S, rows_, F_, width_, hop_, pad, ctypes.c_void_p(out.data_ptr()), st)
    tiles.zero_()
    assert cut(rows_=0) == _lib.ERR and cut(F_=0) == _lib.ERR and cut(width_=1, hop_=1) == _lib.ERR and cut(hop_=width + 1) == _lib.ERR
    assert cut(pad=float("inf")) == _lib.ERR and cut(out=keep) == _lib.ERR and not bool(tiles.any())
    assert cut() == _lib.OK and torch.equal(tiles, basis.cut_frames(keep, width, hop))
    with pytest.raises(_lib.GlowkError):
        basis.langevin_update_frames(m, x, g, width, hop, ETA, LAM, step=1 << 48)
    with pytest.raises(ValueError):
        basis.langevin_update_frames(m, x[:, :, ::2], g, width, hop, ETA, LAM)       # in place needs contiguous states


# ---- the loop --------------------------------------------------------------------------------------------------------------------------
CFG = GlowConfig(H=16, W=16, C=1, L=2, K=3, F=128)
T_STEPS, SIDX = 3, 9


@pytest.fixture(scope="module")
def priors():
    from audiosourcesep_amd.flow_models.flow_glow import GlowFlow
    from audiosourcesep_amd.synthetic import calibrated_engine
    made = [calibrated_engine(CFG, device=0, init_tiles=16, seed=s) for s in (1, 2, 3)]
    return [GlowFlow(e) for e, _ in made], [p for _, p in made]


def frames_of(seed, F):
    """[16, F] dB frames: three synthetic tiles side by side."""
    t = synthetic_mel_tiles(3, CFG, seed=seed).astype(np.float64)[..., 0]
    return np.ascontiguousarray(np.concatenate(list(t), axis=1)[:, :F])


@functools.lru_cache(maxsize=None)
def frames_problem(F):
    """Start states, mixture and noise of a three-source problem on F frames.  Never modified."""
    xs = np.stack([frames_of(20 + k, F) for k in range(3)])
    mixed = ref.g([frames_of(10 + k, F) for k in range(3)])
    noise = np.random.default_rng(3).standard_normal((2, T_STEPS, 3, 16, F))       # [level, step, source]
    for a in (xs, mixed, noise):
        a.setflags(write=False)
    return mixed, xs, noise, basis.get_sigmas(1.0, 0.01, 10)


@pytest.fixture(scope="module")
def fp64_loop(priors):
    """The float64 loop's result at F = 40, hop 8: computed once, read by both arithmetics."""
    mixed, xs, noise, sigmas = frames_problem(40)
    want = R.inner_loop(mixed, list(xs), [R.glow_grad_fn(p, CFG.as_dict()) for p in priors[1]], 16, 8, SIDX, sigmas, noise[0], T=T_STEPS)
    for a in want:
        a.setflags(write=False)
    return want


@pytest.mark.parametrize("arith", ["f32", "f16x3"])
def test_frame_loop_matches_the_fp64_loop(priors, fp64_loop, arith):
    flows, _ = priors
    mixed, xs, noise, sigmas = frames_problem(40)
    saved = [(f.engine.get_precision(), int(f.engine.lib.glowk_get_range_policy(f.engine.h))) for f in flows]
    try:
        if arith == "f16x3":
            for f in flows:
                f.engine.set_precision(_lib.PREC_F16X3)
                f.engine.set_range_policy("error")
        nf = lambda t, k, shape: dev(noise[0][t][k])                               # noqa: E731
        got = basis.basis_inner_loop_frames(dev(mixed), dev(xs), flows, SIDX, sigmas, 16, 8, T=T_STEPS, debug=True, noise_fn=nf)
        assert tuple(got.shape) == (3, 16, 40)
        print("%s: max |d| to the fp64 loop %.3e dB (bar 2e-3)" % (arith, float(np.abs(got.cpu().numpy() - np.stack(fp64_loop)).max())))
        for y, w, x in zip(got, fp64_loop, xs):
            np.testing.assert_allclose(y.cpu().numpy(), w, atol=2e-3)              # dB units, range 120
            assert np.abs(w - x).max() > 1e-3                                      # the update moved the state
        seq = basis.basis_inner_loop_frames(dev(mixed), dev(xs), flows, SIDX, sigmas, 16, 8, T=T_STEPS, streams=None, noise_fn=nf)
        assert torch.equal(got, seq)                                               # one stream for all three: the same numbers
    finally:
        for f, (prec, pol) in zip(flows, saved):
            f.engine.set_precision(prec)
            f.engine.set_range_policy(pol)


def test_disjoint_tiles_through_real_priors_equal_the_per_tile_chain(priors):
    """F = 48, hop = W = 16, two noise levels: ``basis_outer_loop_frames`` equals ``basis_outer_loop_n`` on the three disjoint tiles
    with the noise permuted, bit for bit -- both feed the same 3-tile batches to the same deterministic gradient kernels, and the
    update expression is shared.  At hop 8 the tiles overlap and the result is another one."""
    flows, _ = priors
    mixed, xs, noise, sigmas = frames_problem(48)
    perm = lambda a: dev(R.tiles_of_frames(a, 16))[..., None]                      # noqa: E731
    got, arr = basis.basis_outer_loop_frames(dev(mixed), dev(xs), flows, sigmas[-2:], 16, 16, T=T_STEPS,
                                             noise_fn=lambda s, t, k, shape: dev(noise[s][t][k]))
    want, _ = basis.basis_outer_loop_n(perm(mixed), [perm(x) for x in xs], flows, sigmas[-2:], T=T_STEPS,
                                       noise_fn=lambda s, t, k, shape: perm(noise[s][t][k]))
    assert tuple(got.shape) == (3, 16, 48) and sorted(arr) == ["x1", "x2", "x3"] and all(len(v) == 3 for v in arr.values())
    for k in range(3):
        assert tuple(want[k].shape) == (3, 16, 16, 1) and torch.equal(perm(got[k].cpu().numpy()), want[k])
        assert float((got[k] - dev(xs[k])).abs().max()) > 1e-3
    half, _ = basis.basis_outer_loop_frames(dev(mixed), dev(xs), flows, sigmas[-2:], 16, 8, T=T_STEPS,
                                            noise_fn=lambda s, t, k, shape: dev(noise[s][t][k]))
    print("hop 8 against hop 16: max |d| %.3e dB" % float((half - got).abs().max()))
    assert bool(torch.isfinite(half).all()) and not torch.equal(half, got)


def test_overlapping_tiles_hold_one_value_per_frame_after_every_step(priors):
    flows, _ = priors
    mixed, xs, _, sigmas = frames_problem(40)
    width, hop, F = 16, 8, 40
    eta, lam = R.step_sizes(SIDX, sigmas, 2e-5)
    x, m = dev(xs), dev(mixed)
    tiles = basis.cut_frames(x, width, hop)
    N = tiles.shape[1]
    for t in range(3):
        gs = [flows[k].engine.log_prob_grad(tiles[k].unsqueeze(-1))[1] for k in range(3)]
        basis.langevin_update_frames(m, x, gs, width, hop, eta, lam, seed=4, step=t, tiles_out=tiles)
        for a in range(N - 1):                                                     # tile a + 1 starts hop frames into tile a
            assert torch.equal(tiles[:, a, :, hop:], tiles[:, a + 1, :, :width - hop])
        assert torch.equal(tiles[:, 0, :, :hop], x[:, :, :hop]) and torch.equal(tiles, basis.cut_frames(x, width, hop))
    assert float((x - dev(xs)).abs().max()) > 1e-3


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
N_LONG = 70001                                                                     # 138 frames, 143 samples of padding
SIGMAS = np.array([20.0, 5.0], np.float32)
KW = dict(T=2, delta=1e-4, seed=9, iters=20)


@pytest.fixture(scope="module")
def flows():
    """Two tiny calibrated K = 1 priors of tile shape [96, 64, 1], as tests/test_gpu_longform.py builds its own."""
    from audiosourcesep_amd.flow_models.flow_glow import GlowFlow
    from audiosourcesep_amd.synthetic import calibrated_engine
    cfg = GlowConfig(H=96, W=64, C=1, L=2, K=1, F=128)
    return [GlowFlow(calibrated_engine(cfg, device=0, init_tiles=8, seed=50 + k)[0]) for k in range(2)]


@functools.lru_cache(maxsize=None)
def excerpt():
    y = np.load(os.path.join(GOLDEN, "real_audio_excerpt.npz"))["pcm"].astype(np.float32).reshape(-1) / 32768.0
    y = np.stack([y[i * 50000:i * 50000 + N_LONG] for i in range(2)])
    y.setflags(write=False)
    return y


def test_separate_long_coupled_mono(flows):
    y = excerpt()[0].copy()
    ys, mixed, src = audio.separate_long(y, flows, SIGMAS, coupled=True, **KW)
    assert tuple(ys.shape) == (2, N_LONG) and tuple(mixed.shape) == (96, 138) and tuple(src.shape) == (2, 96, 138)
    assert bool(torch.isfinite(ys).all()) and bool(torch.isfinite(src).all()) and float(ys.abs().max()) > 0
    ys2, mixed2, src2 = audio.separate_long(y, flows, SIGMAS, coupled=True, **KW)
    assert torch.equal(ys, ys2) and torch.equal(src, src2) and torch.equal(mixed, mixed2)
    plain = audio.separate_long(y, flows, SIGMAS, **KW)
    off = audio.separate_long(y, flows, SIGMAS, coupled=False, **KW)
    assert all(torch.equal(a, b) for a, b in zip(plain, off))                      # the keyword's default is the path there was
    assert torch.equal(mixed, plain[1]) and not torch.equal(src, plain[2]) and not torch.equal(ys, plain[0])


def test_separate_long_coupled_stereo(flows):
    y = excerpt().copy()
    ys, mixed, src = audio.separate_long(y, flows, SIGMAS, coupled=True, **KW)
    assert tuple(ys.shape) == (2, 2, N_LONG) and tuple(mixed.shape) == (96, 138) and tuple(src.shape) == (2, 96, 138)
    assert bool(torch.isfinite(ys).all()) and bool(torch.isfinite(src).all())
    ys2, _, src2 = audio.separate_long(y, flows, SIGMAS, coupled=True, **KW)
    assert torch.equal(ys, ys2) and torch.equal(src, src2)
    _, _, plain = audio.separate_long(y, flows, SIGMAS, **KW)
    assert not torch.equal(src, plain)
