"""BASIS as one chain over a whole signal's frames, host side: the torch-formula loop (``basis.basis_inner_loop_frames`` /
``basis_outer_loop_frames`` on CPU tensors) with stand-in Gaussian priors against the fp64 restatement of tests/frames_chain_ref.py,
the case in which it must coincide with the per-tile chain, and the argument checks.  No GPU."""
import numpy as np
import pytest
import torch

from audiosourcesep_amd import audio, basis
from tests import frames_chain_ref as R

ROWS, W = 6, 8


class _StandInPrior:
    """A prior with a closed-form gradient (diagonal Gaussian in dB space), as in tests/test_basis_sources_cpu.py; the mean varies
    along the tile so that a frame's score depends on where in a tile it lies, and overlapping tiles disagree about it."""

    def __init__(self, mu, s, width=W, event_shape=None):
        self.mu = float(mu) + 3.0 * np.cos(np.arange(width) / 1.7)
        self.s = float(s)
        self.engine = self
        if event_shape is not None:
            self.event_shape = event_shape

    def log_prob_grad(self, x):                        # [N, rows, width, 1]
        d = (x - torch.as_tensor(self.mu, dtype=x.dtype)[:, None]) / self.s
        return -0.5 * (d * d).flatten(1).sum(1), -d / self.s

    def grad_np(self, tiles):                          # [N, rows, width] float64
        return -(tiles - self.mu) / self.s ** 2


def _problem(S, F, dtype=torch.float32):
    g = torch.Generator().manual_seed(5 + F)
    mus = [-40.0 - 5.0 * k for k in range(S)]
    truth = [mu + 8.0 * torch.randn(ROWS, F, generator=g) for mu in mus]
    mixed = basis.mixing(truth).to(dtype)
    x = torch.stack([-100.0 + 120.0 * torch.rand(ROWS, F, generator=g) for _ in range(S)]).to(dtype)
    return mixed, x, [_StandInPrior(mu, 8.0) for mu in mus], basis.get_sigmas(30.0, 1.2, 3)


def _noise(sig, t, k, shape, dtype=torch.float32):
    g = torch.Generator().manual_seed(1000 * sig + 10 * t + k)
    return torch.randn(tuple(shape), generator=g).to(dtype)


# a short last tile; a hop that does not divide the width (and frames under 2 and 3 tiles); one tile wider than the signal
@pytest.mark.parametrize("process", ["db", "mean"])
@pytest.mark.parametrize("F,hop", [(8, 4), (19, 4), (21, 3), (5, 4)])
def test_host_loop_against_the_restatement(F, hop, process):
    mixed, x, priors, sigmas = _problem(3, F)
    T, delta, sidx = 4, 0.05, 1
    seen = []

    def noise_fn(t, k, shape):
        seen.append(tuple(shape))
        return _noise(sidx, t, k, shape)

    got = basis.basis_inner_loop_frames(mixed, x, priors, sidx, sigmas, W, hop, delta=delta, T=T, noise_fn=noise_fn, debug=True, mixing=process)
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (3, ROWS, F) and set(seen) == {(ROWS, F)}
    noise = [[_noise(sidx, t, k, (ROWS, F)).numpy().astype(np.float64) for k in range(3)] for t in range(T)]
    want = R.inner_loop(mixed.numpy().astype(np.float64), list(x.numpy()), [p.grad_np for p in priors], W, hop, sidx, sigmas, noise,
                        delta=delta, T=T, process=process)
    for a, b, x0 in zip(got, want, x):
        # a float32 loop against float64: T steps of a state of magnitude <= 100 dB (the bar of tests/test_basis_sources_cpu.py)
        np.testing.assert_allclose(a.numpy(), b, rtol=1e-5, atol=1e-4)
        assert float((a - x0).abs().mean()) > 0.1                    # the chain moved
    assert torch.equal(x, _problem(3, F)[1])                         # and the inputs are left alone
    # the outer loop is the inner loops one after the other, and records the trajectory as frames
    out, arr = basis.basis_outer_loop_frames(mixed, x, priors, sigmas[:2], W, hop, T=2, delta=delta, mixing=process,
                                             noise_fn=lambda s, t, k, shape: _noise(s, t, k, shape))
    step = x
    for s in range(2):
        step = basis.basis_inner_loop_frames(mixed, step, priors, s, sigmas[:2], W, hop, delta=delta, T=2, mixing=process,
                                             noise_fn=lambda t, k, shape, s=s: _noise(s, t, k, shape))
    assert torch.equal(out, step) and sorted(arr) == ["x1", "x2", "x3"]
    assert all(len(v) == 3 and v[0].shape == (ROWS, F) for v in arr.values()) and np.array_equal(arr["x2"][-1], out[1].numpy())


def test_cut_and_stitched_score_on_the_host():
    rng = np.random.default_rng(0)
    for F, hop in [(8, 4), (19, 4), (21, 3), (5, 4), (24, 8)]:
        x = rng.uniform(-150.0, 50.0, (2, ROWS, F))
        tiles = basis.cut_frames(torch.from_numpy(x), W, hop, pad=-77.0)
        N = R.tile_count(F, W, hop)
        assert basis.tile_count(F, W, hop) == N == audio.tile_count(F, W, hop) and tuple(tiles.shape) == (2, N, ROWS, W)
        np.testing.assert_array_equal(tiles.numpy(), R.cut(x, W, hop, pad=-77.0))
        np.testing.assert_array_equal(basis.cut_frames(torch.from_numpy(x[0]), W, hop).numpy(), R.cut(x[0], W, hop))
        g = rng.normal(0.0, 5.0, (N, ROWS, W))
        s = basis.stitch_scores(torch.from_numpy(g), F, hop).numpy()
        np.testing.assert_allclose(s, R.stitched_score(g, F, hop), rtol=1e-12, atol=1e-12)
        # the weights of a frame sum to one: equal scores in every tile stitch to that score
        one = basis.stitch_scores(torch.ones(N, ROWS, W, dtype=torch.float64), F, hop).numpy()
        np.testing.assert_allclose(one, 1.0, rtol=1e-12)


@pytest.mark.parametrize("process", ["db", "mean"])
def test_disjoint_tiles_are_the_per_tile_chain(process):
    """hop = W and F a multiple of W: every frame lies under one tile, whose gradient it takes as it is, so the frame chain is
    ``basis_inner_loop_n`` on the cut tiles with the same noise permuted into the tile layout.  Both are the same float64 torch
    formulas on the same values; only the memory layout differs, which may change the last bits of a vectorised exp or log, so
    the bar is a few float64 roundings of a 100 dB state and not bitwise equality."""
    F, T, delta, sidx = 3 * W, 5, 0.05, 1
    mixed, x, priors, sigmas = _problem(3, F, torch.float64)
    to_tiles = lambda a: torch.from_numpy(np.ascontiguousarray(R.tiles_of_frames(a.numpy(), W)))[..., None]   # noqa: E731
    got = basis.basis_inner_loop_frames(mixed, x, priors, sidx, sigmas, W, W, delta=delta, T=T, mixing=process,
                                        noise_fn=lambda t, k, shape: _noise(sidx, t, k, shape, torch.float64))
    want = basis.basis_inner_loop_n(to_tiles(mixed), [to_tiles(x[k]) for k in range(3)], priors, sidx, sigmas, delta=delta, T=T, mixing=process,
                                    noise_fn=lambda t, k, shape: to_tiles(_noise(sidx, t, k, (ROWS, F), torch.float64)))
    for k in range(3):
        assert tuple(want[k].shape) == (3, ROWS, W, 1)
        np.testing.assert_allclose(to_tiles(got[k]).numpy(), want[k].numpy(), rtol=1e-13, atol=1e-11)
        assert float((got[k] - x[k]).abs().mean()) > 0.1
    # overlapping tiles give another chain
    other = basis.basis_inner_loop_frames(mixed, x, priors, sidx, sigmas, W, W // 2, delta=delta, T=T, mixing=process,
                                          noise_fn=lambda t, k, shape: _noise(sidx, t, k, shape, torch.float64))
    assert float((other - got).abs().max()) > 1e-3


def test_argument_checks():
    mixed, x, priors, sigmas = _problem(3, 19)
    run = lambda m=mixed, s=x, p=priors, width=W, hop=4, **kw: basis.basis_inner_loop_frames(m, s, p, 0, sigmas, width, hop, T=1, **kw)  # noqa: E731
    assert tuple(run().shape) == (3, ROWS, 19)
    assert tuple(run(s=list(x)).shape) == (3, ROWS, 19)              # a list of S frame tensors is stacked
    big = torch.zeros(17, ROWS, 19)
    for bad in (dict(s=x[:1], p=priors[:1]), dict(s=big, p=[priors[0]] * 17),          # S outside 2..16
                dict(hop=W + 1), dict(hop=0), dict(width=1, hop=1), dict(width=129, hop=4), dict(hop=4.0),
                dict(p=priors[:2]), dict(m=mixed[:, :18]), dict(m=mixed[None]), dict(s=x[0]),      # shapes that do not fit
                dict(p=[_StandInPrior(-40.0, 8.0, event_shape=(ROWS, W + 1, 1))] + priors[1:]),     # a prior of another tile width
                dict(p=[_StandInPrior(-40.0, 8.0, event_shape=(ROWS + 1, W, 1))] + priors[1:]),
                dict(mixing="power")):
        with pytest.raises(ValueError):
            run(**bad)
    assert tuple(run(p=[_StandInPrior(-40.0, 8.0, event_shape=(ROWS, W, 1))] + priors[1:]).shape) == (3, ROWS, 19)
    with pytest.raises(ValueError):
        basis.basis_outer_loop_frames(mixed, x, priors, sigmas, W, 4, restores=[None, None], T=1)
    with pytest.raises(ValueError):
        basis.basis_outer_loop_frames(mixed, x[:1], priors[:1], sigmas, W, 4, T=1)
    with pytest.raises(ValueError):
        basis.cut_frames(x, W, W + 1)
    with pytest.raises(ValueError):
        basis.cut_frames(x[0, 0], W, 4)
    g = [torch.zeros(4, ROWS, W) for _ in range(3)]
    basis.langevin_update_frames(mixed, x.clone(), g, W, 4, 1e-3, 1.0, eps=[torch.zeros(ROWS, 19)] * 3)
    for bad in (dict(g=g[:2]), dict(g=[torch.zeros(3, ROWS, W)] * 3), dict(hop=W + 1), dict(eps=[None, None]), dict(mixing="power"),
                dict(tiles_out=torch.zeros(3, 4, ROWS, W + 1))):
        kw = dict(g=g, hop=4, eps=None, mixing="db", tiles_out=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            basis.langevin_update_frames(mixed, x.clone(), kw["g"], W, kw["hop"], 1e-3, 1.0, eps=kw["eps"], mixing=kw["mixing"],
                                         tiles_out=kw["tiles_out"])


class _Flow:
    event_shape = (96, 64, 1)


@pytest.mark.parametrize("coupled", [1, 0, None, "yes", np.bool_(True)])
def test_separate_long_rejects_a_coupled_that_is_no_bool(coupled):
    with pytest.raises(ValueError, match="coupled"):
        audio.separate_long(np.zeros(4000, np.float32), [_Flow(), _Flow()], np.array([1.0], np.float32), coupled=coupled)
