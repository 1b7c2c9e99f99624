"""BASIS for any number of sources, host side: the mixing processes and their gradients, the torch-formula loop with stand-in
priors, the prior-parallel layout for S priors and its gloo run.  No GPU."""
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from audiosourcesep_amd import basis
from tests import basis_sources_ref as ref


class _StandInPrior:
    """A prior with a closed-form gradient (diagonal Gaussian in dB space): what compute_grad_logprob needs of a GlowFlow."""

    def __init__(self, mu, s):
        self.mu, self.s = float(mu), float(s)
        self.engine = self

    def log_prob_grad(self, x):
        d = (x - self.mu) / self.s
        return -0.5 * (d * d).flatten(1).sum(1), -d / self.s


@pytest.mark.parametrize("process", ["db", "mean"])
@pytest.mark.parametrize("S", [2, 3, 16])
def test_mixing_and_its_gradient_against_numpy(S, process):
    rng = np.random.default_rng(S)
    src = rng.uniform(-80, 10, (S, 5, 6, 4, 1))
    got = basis.mixing([torch.from_numpy(s) for s in src], process).numpy()
    np.testing.assert_allclose(got, ref.g(list(src), process), rtol=1e-12, atol=1e-12)
    grads = basis.grad_mixing([torch.from_numpy(s) for s in src], process)
    assert len(grads) == S
    for a, b in zip(grads, ref.grad_g(list(src), process)):
        np.testing.assert_allclose(a.numpy(), b, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(sum(a.numpy() for a in grads), 1.0, rtol=1e-12)
    # float32 tensors take the same formulas in float32
    got32 = basis.mixing([torch.from_numpy(s.astype(np.float32)) for s in src], process).numpy()
    np.testing.assert_allclose(got32, ref.g(list(src), process), rtol=2e-6, atol=2e-5)
    if process == "db":
        # equal sources mix to themselves, and S equal-power sources lose nothing to the -ln S term
        same = [torch.from_numpy(src[0])] * S
        np.testing.assert_allclose(basis.mixing(same).numpy(), src[0], rtol=1e-12, atol=1e-12)
        if S == 2:
            np.testing.assert_array_equal(basis.mixing([torch.from_numpy(s) for s in src]).numpy(),
                                          basis.mixing_db(*[torch.from_numpy(s) for s in src]).numpy())
    with pytest.raises(ValueError):
        basis.mixing([torch.from_numpy(s) for s in src], "power")
    with pytest.raises(ValueError):
        basis.grad_mixing([torch.from_numpy(s) for s in src], "power")


@pytest.mark.parametrize("process", ["db", "mean"])
@pytest.mark.parametrize("S", [2, 3, 16])
def test_grad_mixing_is_the_derivative_of_mixing(S, process):
    g = torch.Generator().manual_seed(S)
    src = [(-80.0 + 90.0 * torch.rand(4, 3, 2, 1, generator=g, dtype=torch.float64)).requires_grad_(True) for _ in range(S)]
    auto = torch.autograd.grad(basis.mixing(src, process).sum(), src)
    for a, b in zip(auto, basis.grad_mixing([s.detach() for s in src], process)):
        assert float((a - b).abs().max()) <= 1e-6


def _problem(S, n=9):
    g = torch.Generator().manual_seed(5)
    mus = [-40.0 - 5.0 * k for k in range(S)]
    truth = [mu + 8.0 * torch.randn(n, 6, 4, 1, generator=g) for mu in mus]
    mixed = basis.mixing(truth)
    xs = [-100.0 + 120.0 * torch.rand(n, 6, 4, 1, generator=g) for _ in range(S)]
    return mixed, xs, [_StandInPrior(mu, 8.0) for mu in mus], basis.get_sigmas(30.0, 1.2, 3)


def _noise(sig, t, k, shape, lo=0, n=9):
    """Injected Langevin noise, a pure function of (level, step, source, tile index): every rank draws the whole batch's noise and
    takes its tiles, as the device RNG does with its tile offset."""
    g = torch.Generator().manual_seed(1000 * sig + 10 * t + k)
    return torch.randn((n,) + tuple(shape[1:]), generator=g)[lo:lo + shape[0]]


@pytest.mark.parametrize("process", ["db", "mean"])
def test_host_loop_for_three_sources_against_the_update_written_out(process):
    mixed, xs, priors, sigmas = _problem(3)
    T, delta, sidx = 4, 0.05, 1
    got = basis.basis_inner_loop_n(mixed, xs, priors, sidx, sigmas, delta=delta, T=T, noise_fn=lambda t, k, shape: _noise(sidx, t, k, shape),
                                   debug=True, mixing=process)
    sigma, sigma_l = float(sigmas[sidx]), float(sigmas[-1])
    eta, lam = float(np.float32(delta * (sigma / sigma_l) ** 2)), 1.0 / sigma ** 2
    want = [x.numpy().astype(np.float64) for x in xs]
    m64 = mixed.numpy().astype(np.float64)
    for t in range(T):
        gs = [-(x - p.mu) / p.s ** 2 for x, p in zip(want, priors)]
        eps = [_noise(sidx, t, k, x.shape).numpy().astype(np.float64) for k, x in enumerate(want)]
        want = ref.update(m64, want, gs, eps, eta, lam, process)
    assert isinstance(got, list) and len(got) == 3
    for a, b, x in zip(got, want, xs):
        # float32 loop against float64: T steps of a state of magnitude <= 100 dB
        np.testing.assert_allclose(a.numpy(), b, rtol=1e-5, atol=1e-4)
        assert float((a - x).abs().mean()) > 0.1                     # the chain moved
    assert all(torch.equal(x, y) for x, y in zip(xs, _problem(3)[1]))  # and the inputs are left alone


def test_two_sources_agree_with_the_two_source_host_loop():
    mixed, xs, priors, sigmas = _problem(2)
    nf2 = lambda s, t, w, shape: _noise(s, t, w, shape)   # noqa: E731
    r1, r2, arr2 = basis.basis_outer_loop(mixed, xs[0], xs[1], priors[0], priors[1], sigmas, T=6, delta=0.05, noise_fn=nf2)
    ys, arr = basis.basis_outer_loop_n(mixed, xs, priors, sigmas, T=6, delta=0.05, noise_fn=nf2)
    np.testing.assert_allclose(ys[0].numpy(), r1.numpy(), rtol=1e-6)
    np.testing.assert_allclose(ys[1].numpy(), r2.numpy(), rtol=1e-6)
    assert sorted(arr) == ["x1", "x2"] and len(arr["x1"]) == len(arr2["x1"]) == len(sigmas) + 1
    a, b = basis.basis_inner_loop(mixed, xs[0], xs[1], priors[0], priors[1], 2, sigmas, delta=0.05, T=5, noise_fn=lambda t, w, s: _noise(2, t, w, s))
    c = basis.basis_inner_loop_n(mixed, xs, priors, 2, sigmas, delta=0.05, T=5, noise_fn=lambda t, w, s: _noise(2, t, w, s))
    np.testing.assert_allclose(c[0].numpy(), a.numpy(), rtol=1e-6)
    np.testing.assert_allclose(c[1].numpy(), b.numpy(), rtol=1e-6)


def test_argument_checks_of_the_loops():
    mixed, xs, priors, sigmas = _problem(3)
    with pytest.raises(ValueError):
        basis.basis_inner_loop_n(mixed, xs[:1], priors[:1], 0, sigmas, T=1)
    with pytest.raises(ValueError):
        basis.basis_inner_loop_n(mixed, xs, priors[:2], 0, sigmas, T=1)
    with pytest.raises(ValueError):
        basis.basis_inner_loop_n(mixed, xs, priors, 0, sigmas, T=1, mixing="power")
    with pytest.raises(ValueError):
        basis.basis_outer_loop_n(mixed, xs, priors, sigmas, restores=[None, None], T=1)
    with pytest.raises(ValueError):
        basis.basis_inner_loop_n(mixed, xs, priors, 0, sigmas, T=1, prior_group=object(), prior_index=3)


def test_prior_parallel_layout_for_three_priors():
    lays = [basis.prior_parallel_layout_n(30, 6, r, 3) for r in range(6)]
    assert [l["prior"] for l in lays] == [0, 1, 2, 0, 1, 2]
    assert [l["shard"] for l in lays] == [0, 0, 0, 1, 1, 1] and all(l["n_shards"] == 2 for l in lays)
    assert [l["bounds"] for l in lays] == [(0, 15)] * 3 + [(15, 30)] * 3
    assert [l["group"] for l in lays] == [(0, 1, 2)] * 3 + [(3, 4, 5)] * 3
    # two sources: the pair layout
    for r in range(4):
        a, b = basis.prior_parallel_layout_n(30, 4, r, 2), basis.prior_parallel_layout(30, 4, r)
        assert (a["prior"], a["shard"], a["n_shards"], a["bounds"], a["group"]) == (b["prior"], b["shard"], b["n_shards"], b["bounds"], b["pair"])
    for world, S in ((4, 3), (2, 3), (6, 4), (6, 1), (34, 17)):
        with pytest.raises(ValueError):
            basis.prior_parallel_layout_n(30, world, 0, S)
    with pytest.raises(ValueError):
        basis.prior_parallel_layout_n(30, 6, 6, 3)


def _pp_worker(rank, world, port, q):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    mixed, xs, priors, sigmas = _problem(3)
    lay = basis.prior_parallel_layout_n(mixed.shape[0], world, rank, 3)
    group = basis.make_prior_group(world, rank, 3)
    a, b = lay["bounds"]
    # this rank holds ONE prior: the other models are None and must never be asked
    models = [p if k == lay["prior"] else None for k, p in enumerate(priors)]
    ys, arr = basis.basis_outer_loop_n(mixed[a:b], [x[a:b] for x in xs], models, sigmas, T=6, delta=0.05,
                                       noise_fn=lambda s, t, k, shape: _noise(s, t, k, shape, lo=a), tile_offset=a,
                                       prior_group=group, prior_index=lay["prior"])
    q.put((rank, lay["prior"], a, b, [y.numpy() for y in ys], sorted(arr), len(arr["x3"])))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [3, 6])
def test_prior_parallel_three_priors_equal_the_one_process_chain(world):
    """world = 3 shards' worth of ranks: rank r owns prior r % 3 of tile shard r // 3, one all-gather of the three gradients per
    step.  Every rank ends with the state the one-process chain reaches for its tiles (the gradients are gathered, not reduced,
    and the update is the same arithmetic on the same numbers), and the ranks of a group hold identical copies."""
    mixed, xs, priors, sigmas = _problem(3)
    want, _ = basis.basis_outer_loop_n(mixed, xs, priors, sigmas, T=6, delta=0.05, noise_fn=lambda s, t, k, shape: _noise(s, t, k, shape))
    assert all(torch.isfinite(w).all() for w in want) and float((want[0] - xs[0]).abs().mean()) > 1.0          # the chain moved
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_pp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    covered = []
    for rank, prior, a, b, ys, keys, nlev in res:
        assert prior == rank % 3 and keys == ["x1", "x2", "x3"] and nlev == len(sigmas) + 1
        for y, w in zip(ys, want):
            np.testing.assert_array_equal(y, w[a:b].numpy())
        first = res[rank - prior]                                    # the group's rank of prior 0
        assert all(np.array_equal(y, z) for y, z in zip(ys, first[4]))
        if prior == 0:
            covered.append((a, b))
    assert covered[0][0] == 0 and covered[-1][1] == mixed.shape[0] and all(covered[i][1] == covered[i + 1][0] for i in range(len(covered) - 1))
