"""BASIS separation loop (annealed Langevin dynamics with flow priors) on top of the glowk log_prob + gradient path.

Mirrors the glow branch of the reference's ``run_basis_sep.py``: ``get_sigmas`` (ncsn/utils.py:7-14), the dB mixing
process ``g`` / ``grad_g`` (run_basis_sep.py:131-147), ``basis_inner_loop`` (:152-214) and ``basis_outer_loop`` (:217-260).
On the GPU the per-step arithmetic outside ``compute_grad_logprob`` -- the two noise draws, the dB mixture ``g``, its softmax
weights ``grad_g`` and every update -- is ONE HIP kernel (``glowk_basis_update_n``, csrc/glowk_basis.h) with the engine's
counter-based device RNG (Philox4x32-10: the draw of element e at step t is a pure function of (seed, t, e)); torch supplies
storage and streams only.  The noise source stays injectable so that tests can replay the oracle's draws (the reference draws
fresh ``tf.random.normal`` noise, unseeded).  CPU tensors (the host-side tests of ``g`` / ``grad_g``) take the torch formulas.

Convention: ``x1, x2, mixed`` live in the space the two flows were built for -- with
``build_glow(..., data_type='melspec')`` that is dB; the flows' own SpecPreprocessing maps it to the network's range.
Tiles are independent, so ``shard`` splits ``n_mixed`` over the ranks of a process group with no collective in the loop.
At the reference's 30 mixture tiles that alone cannot scale far (a step is a latency-bound chain of ~400 small launches per prior:
4 tiles per GPU take almost as long as 30), so the loop also runs PRIOR-PARALLEL (``prior_parallel_layout``): the two priors of a
tile shard live on two ranks, each evaluates its own prior's gradient, ONE all-gather of the two gradient tensors per Langevin
step (2 x 737 KB for 30 tiles of 96x64) makes both visible, and both ranks run the identical update kernel (same Philox counters:
the replicated state stays bit-identical without a broadcast).

Any number of sources: the ``*_n`` functions (``mixing`` / ``grad_mixing``, ``langevin_update_n``, ``basis_inner_loop_n``,
``basis_outer_loop_n``, ``prior_parallel_layout_n`` / ``make_prior_group`` / ``exchange_prior_gradients_n``) take lists of S
states, gradients and priors, S in [2, 16], and either mixing process of the reference (``"db"``: :131-147, ``"mean"``: :108-116;
its power-scale branch is not offered).  The update is still one kernel (``glowk_basis_update_n``); source k draws the device RNG
stream ``k & 1`` of source pair ``k >> 1``, so sources 0 and 1 see the two-source path's noise and no two sources share a draw.
The S gradient evaluations go to at most four side streams, round-robin.  The two-source functions (``mixing_db``,
``langevin_update``, ``basis_inner_loop``, ``basis_outer_loop``, ``prior_parallel_layout`` / ``make_pair_group`` /
``exchange_prior_gradients``) are these at S = 2 under their first signatures: the same kernel, the same loops.

One chain over a whole signal: the ``*_frames`` functions (``cut_frames``, ``langevin_update_frames``,
``basis_inner_loop_frames``, ``basis_outer_loop_frames``) keep the Langevin state as the signal's frames [S, rows, F].  The priors
see its overlapping tiles, and a frame's prior score is the cross-fade of the scores of the tiles that cover it, with weights that
sum to one, so overlapping tiles are coupled inside the loop (not in the reference, which cuts disjoint
extracts).  The update, the stitch in front of it and the next step's tiles are one kernel (``glowk_basis_update_frames``,
csrc/glowk_frames.h), which shares the update's device code with ``glowk_basis_update_n``.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .distributed import shard_bounds


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _s(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def get_sigmas(sigma1, sigmaL, num_classes, progression="geometric"):
    """ncsn/utils.py:7-14."""
    if progression == "geometric":
        sigmas = np.exp(np.linspace(np.log(sigma1), np.log(sigmaL), num=num_classes))
    elif progression == "logarithmic":
        sigmas = np.logspace(np.log(sigma1) / np.log(10), np.log(sigmaL) / np.log(10), num=num_classes)
    else:
        raise ValueError("progression should be geometric or logarithmic")
    return sigmas.astype(np.float32)


def mixing_db(*sources):
    """``g`` of the dB branch, sum in power (run_basis_sep.py:133-141): 10/ln10 * (logsumexp(s ln10/10) - ln K)."""
    return mixing(sources, "db")


def device_randn(shape, device, seed, step=0, which=0, uniform=False, offset=0, pair=0):
    """Standard-normal (or U(0, 1)) tensor from the engine's Philox stream (seed, step, which): the draws
    ``glowk_basis_update`` makes itself when no noise is injected.  ``offset``: position of element 0 in the stream (a
    multiple of 4) -- a rank holding tiles [a, b) of a batch passes ``a * H * W * C`` and gets the draws one process would have
    made for those tiles, so the noise a tile sees does not depend on how the batch is sharded.  ``pair``: the source pair of
    the S-source update (``glowk_random_source``: source k draws ``which = k & 1``, ``pair = k >> 1``); 0 is the stream above."""
    out = torch.empty(shape, device=device, dtype=torch.float32)
    if pair:
        _lib.check(_lib.load().glowk_random_source(_p(out), out.numel(), int(seed), int(step), int(which), int(pair), int(bool(uniform)),
                                                   int(offset), _s(out)))
        return out
    _lib.check(_lib.load().glowk_random(_p(out), out.numel(), int(seed), int(step), int(which), int(bool(uniform)), int(offset), _s(out)))
    return out


def add_device_noise(x, sigma, seed, step=0, which=2, offset=0):
    """x + sigma * N(0, I) as ONE kernel of the engine (``glowk_add_noise``; the draws are ``device_randn(seed, step, which,
    offset)``): train_noisy_glow.py:31."""
    x = x.contiguous()
    out = torch.empty_like(x)
    _lib.check(_lib.load().glowk_add_noise(_p(x), _p(out), x.numel(), float(sigma), int(seed), int(step), int(which), int(offset), _s(x)))
    return out


def langevin_update(mixed, x1, x2, g1, g2, eta, lambda_recon, eps1=None, eps2=None, seed=0, step=0, nonfinite=None, offset=0):
    """run_basis_sep.py:163-181 for two sources, IN PLACE on x1 / x2 (contiguous float32 CUDA tensors, distinct buffers): one
    kernel, the S = 2 instance behind ``langevin_update_n`` (``glowk_basis_update``)."""
    _lib.check(_lib.load().glowk_basis_update(_p(x1), _p(x2), _p(g1), _p(g2), _p(mixed), x1.numel(), float(eta), float(lambda_recon),
                                              _p(eps1), _p(eps2), int(seed), int(step), int(offset), _p(nonfinite), _s(x1)))


def grad_mixing_db(*sources):
    """``grad_g`` (run_basis_sep.py:143-147): softmax over the sources of s ln10/10."""
    return tuple(grad_mixing(sources, "db"))


def prior_parallel_layout(n_mixed, world_size, rank):
    """Prior-parallel BASIS over ``world_size`` = 2 S ranks: rank r holds prior ``r % 2`` (0: model1, 1: model2) of tile shard
    ``r // 2`` of S.  -> dict(prior, shard, n_shards, bounds=(a, b), pair=(rank of prior 0, rank of prior 1)):
    ``prior_parallel_layout_n`` for two priors, its ``group`` under the name ``pair``.  ``make_pair_group`` creates the groups."""
    if world_size < 2 or world_size % 2:
        raise ValueError("prior-parallel BASIS needs an even number of ranks (two priors per tile shard)")
    lay = prior_parallel_layout_n(n_mixed, world_size, rank, 2)
    lay["pair"] = lay.pop("group")
    return lay


def make_pair_group(world_size, rank):
    """The process group of this rank's prior pair (``make_prior_group`` for two priors: collective over the whole job)."""
    return make_prior_group(world_size, rank, 2)


def exchange_prior_gradients(g_mine, prior_index, pair_group):
    """-> (g1, g2): ``exchange_prior_gradients_n`` over the pair (rank order within the pair = prior order)."""
    g1, g2 = exchange_prior_gradients_n(g_mine, prior_index, pair_group)
    return g1, g2


def compute_grad_logprob(inputs, model):
    """run_basis_sep.py:73-79 -- d log_prob / d inputs through the engine (no autograd tape needed)."""
    _, g = model.engine.log_prob_grad(inputs)
    return g


def basis_inner_loop(mixed, x1, x2, model1, model2, sigma_idx, sigmas, delta=2e-5, T=100, noise_fn=None, debug=False,
                     streams="auto", seed=0, step0=0, offset=0, prior_group=None, prior_index=None):
    """run_basis_sep.py:152-214 (model_type == 'glow'): ``basis_inner_loop_n`` for two sources and the dB mixture -> (x1, x2).
    ``noise_fn(t, which, shape)``: ``which`` is the source, 0 or 1.  ``streams``: "auto", None, or (s1, s2)."""
    if prior_group is not None and prior_index not in (0, 1):
        raise ValueError("prior_index must be 0 or 1 in prior-parallel mode")
    x1, x2 = basis_inner_loop_n(mixed, [x1, x2], [model1, model2], sigma_idx, sigmas, delta=delta, T=T, noise_fn=noise_fn, debug=debug,
                                streams=streams, seed=seed, step0=step0, offset=offset, prior_group=prior_group, prior_index=prior_index)
    return x1, x2


def basis_outer_loop(mixed, x1, x2, model1, model2, sigmas, restore_1=None, restore_2=None, T=100, delta=2e-5, noise_fn=None,
                     debug=False, seed=0, tile_offset=0, prior_group=None, prior_index=None):
    """run_basis_sep.py:217-260: ``basis_outer_loop_n`` for two sources and the dB mixture -> (x1, x2, x_arr), the trajectory
    under the keys ``"x1"`` and ``"x2"``.  ``restore_k``: the restore map of model k (``restores[k - 1]`` there)."""
    (x1, x2), x_arr = basis_outer_loop_n(mixed, [x1, x2], [model1, model2], sigmas, restores=[restore_1, restore_2], T=T, delta=delta,
                                         noise_fn=noise_fn, debug=debug, seed=seed, tile_offset=tile_offset, prior_group=prior_group,
                                         prior_index=prior_index)
    return x1, x2, x_arr


def shard(tensor, world_size, rank):
    """This rank's contiguous slice of the ``n_mixed`` tiles (tiles are independent: no collective inside the loop)."""
    a, b = shard_bounds(tensor.shape[0], world_size, rank)
    return tensor[a:b]


# ---- any number of sources (run_basis_sep.py:106-149: g(*sources), grad_g(*sources) for K = len(sources)) -------------------------
MIXINGS = {"db": _lib.MIX_DB, "mean": _lib.MIX_MEAN}
MAX_SOURCES = 16
MAX_SIDE_STREAMS = 4


def _mixing_id(process):
    if process not in MIXINGS:
        raise ValueError("mixing process: expected one of %s, got %r" % (tuple(MIXINGS), process))
    return MIXINGS[process]


def _ptrs(tensors):
    """Host array of device pointers (None -> NULL) for the ``*_n`` entry points."""
    arr = (ctypes.c_void_p * len(tensors))()
    for k, t in enumerate(tensors):
        arr[k] = t.data_ptr() if t is not None else None
    return arr


def mixing(sources, process="db"):
    """``g(*sources)`` for S = len(sources): ``"db"`` sums in power (run_basis_sep.py:131-141), ``"mean"`` is the linear mean
    (:108-111).  2..16 CUDA float32 tensors go through ``glowk_basis_mix_n``; anything else takes the torch formula."""
    mid = _mixing_id(process)
    sources = list(sources)
    if not sources:
        raise ValueError("mixing: expected at least one source")
    if 2 <= len(sources) <= MAX_SOURCES and all(t.is_cuda and t.dtype == torch.float32 for t in sources):
        if any(t.shape != sources[0].shape for t in sources):
            raise ValueError("mixing: the sources must have one shape")
        src = [t.contiguous() for t in sources]
        out = torch.empty_like(src[0])
        _lib.check(_lib.load().glowk_basis_mix_n(_ptrs(src), len(src), _p(out), out.numel(), mid, _s(out)))
        return out
    s = torch.stack(sources, dim=0)
    if process == "mean":
        return s.mean(dim=0)
    return (10.0 / math.log(10.0)) * (torch.logsumexp(s * (math.log(10.0) / 10.0), dim=0) - math.log(float(len(sources))))


def grad_mixing(sources, process="db"):
    """``grad_g(*sources)`` -> list of S tensors: softmax over the sources of s ln10/10 (``"db"``, run_basis_sep.py:143-147) or
    1/S (``"mean"``, :113-116).  Torch formulas: the update kernel computes these weights itself."""
    _mixing_id(process)
    s = torch.stack(list(sources), dim=0)
    if process == "mean":
        return list(torch.unbind(torch.full_like(s, 1.0 / s.shape[0]), dim=0))
    return list(torch.unbind(torch.softmax(s * (math.log(10.0) / 10.0), dim=0), dim=0))


def langevin_update_n(mixed, xs, gs, eta, lambda_recon, eps=None, seed=0, step=0, nonfinite=None, offset=0, mixing="db"):
    """run_basis_sep.py:163-181 for S = len(xs) sources, IN PLACE on every xs[k] (contiguous float32 CUDA tensors, distinct
    buffers): one kernel.  ``eps``: None, or a list of S entries, each a standard-normal tensor or None (that source draws from
    the device RNG: stream ``k & 1`` of pair ``k >> 1`` at (seed, step), element ``offset`` onwards)."""
    mid = _mixing_id(mixing)
    S = len(xs)
    if len(gs) != S or (eps is not None and len(eps) != S):
        raise ValueError("langevin_update_n: %d states need %d gradients (and noise entries)" % (S, S))
    for t in xs:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("langevin_update_n: the states are updated in place and must be contiguous float32 CUDA tensors")
    n = xs[0].numel() if S else 0
    ro = [mixed] + list(gs) + [e for e in (eps or []) if e is not None]
    ro = [t.to(torch.float32).contiguous() for t in ro]
    if any(t.numel() != n for t in list(xs) + ro):
        raise ValueError("langevin_update_n: every tensor must hold as many elements as the states")
    mixed_c, gs_c = ro[0], ro[1:1 + S]
    eps_c, rest = None, iter(ro[1 + S:])
    if eps is not None:
        eps_c = [next(rest) if e is not None else None for e in eps]
    _lib.check(_lib.load().glowk_basis_update_n(_ptrs(xs), _ptrs(gs_c), _ptrs(eps_c) if eps_c is not None else None, S, _p(mixed_c), n, mid,
                                                float(eta), float(lambda_recon), int(seed), int(step), int(offset), _p(nonfinite),
                                                _s(mixed_c)))


def prior_parallel_layout_n(n_mixed, world_size, rank, n_sources):
    """Prior-parallel BASIS for ``n_sources`` priors over ``world_size`` = n_sources * shards ranks: rank r holds prior
    ``r % n_sources`` of tile shard ``r // n_sources``.  -> dict(prior, shard, n_shards, bounds=(a, b), group=(the ranks of this
    shard, in prior order)).  ``make_prior_group`` creates the groups."""
    if n_sources < 2 or n_sources > MAX_SOURCES:
        raise ValueError("prior-parallel BASIS: the number of sources must be 2..%d, got %d" % (MAX_SOURCES, n_sources))
    if world_size < n_sources or world_size % n_sources:
        raise ValueError("prior-parallel BASIS with %d priors needs a multiple of %d ranks, got %d" % (n_sources, n_sources, world_size))
    if not 0 <= rank < world_size:
        raise ValueError("rank %d is outside the world of %d" % (rank, world_size))
    shards = world_size // n_sources
    s = rank // n_sources
    return {"prior": rank % n_sources, "shard": s, "n_shards": shards, "bounds": shard_bounds(n_mixed, shards, s),
            "group": tuple(range(n_sources * s, n_sources * (s + 1)))}


def make_prior_group(world_size, rank, n_sources):
    """The process group of this rank's tile shard (its ``n_sources`` priors).  Collective over the whole job: every rank creates
    every group, in the same order, and keeps its own."""
    import torch.distributed as dist
    if world_size < n_sources or world_size % n_sources:
        raise ValueError("prior-parallel BASIS with %d priors needs a multiple of %d ranks, got %d" % (n_sources, n_sources, world_size))
    mine = None
    for s in range(world_size // n_sources):
        g = dist.new_group(list(range(n_sources * s, n_sources * (s + 1))))
        if rank // n_sources == s:
            mine = g
    return mine


def exchange_prior_gradients_n(g_mine, prior_index, group):
    """-> list of the S priors' gradients: ONE all-gather over the shard's group (rank order within the group = prior order).
    RCCL over xGMI when the backend is nccl; under gloo (CPU tests, one-GPU rehearsal) device tensors go through the host."""
    import torch.distributed as dist
    S = dist.get_world_size(group)
    g_mine = g_mine.contiguous()
    if g_mine.is_cuda and dist.get_backend(group) == "gloo":
        mine = g_mine.cpu()
        parts = [torch.empty_like(mine) for _ in range(S)]
        dist.all_gather(parts, mine, group=group)
        parts = [p.to(g_mine.device) for p in parts]
    else:
        parts = [torch.empty_like(g_mine) for _ in range(S)]
        dist.all_gather(parts, g_mine, group=group)
    parts[prior_index] = g_mine
    return parts


def _grad_n(xs, models, streams):
    """The S priors' gradients are independent, so their chains are enqueued on the given side streams, source k on the stream of
    its model -- distinct models take the streams round-robin, a model that serves several sources runs them one after the other
    on one stream (an engine is not re-entrant).  At BASIS batch sizes the deeper levels launch only tens of workgroups each, so
    the kernel sequences interleave on the 256 CUs.

    The range guard of the split arithmetics would make each call wait for its own stream before returning (policy "error" /
    "fallback"), i.e. serialise the models; so all calls run under "ignore" (fully asynchronous) and the flags are read once every
    sequence is enqueued: "fallback" re-runs that one model's gradients on the exact fp32 kernels, "error" raises."""
    if not streams or xs[0].device.type != "cuda":
        return [compute_grad_logprob(x, m) for x, m in zip(xs, models)]
    cur = torch.cuda.current_stream(xs[0].device)
    engines, of_engine = [], {}
    for m in models:
        if id(m.engine) not in of_engine:
            of_engine[id(m.engine)] = len(engines)
            engines.append(m.engine)
    stream_of = [streams[of_engine[id(m.engine)] % len(streams)] for m in models]
    used = list({id(st): st for st in stream_of}.values())
    for st in used:
        st.wait_stream(cur)
    guarded = [e.get_precision() != _lib.PREC_F32 for e in engines]
    saved = [int(e.lib.glowk_get_range_policy(e.h)) for e in engines]
    for e, gd in zip(engines, guarded):
        if gd:
            e.set_range_policy("ignore")
    try:
        out = []
        for x, m, st in zip(xs, models, stream_of):
            with torch.cuda.stream(st):
                out.append(compute_grad_logprob(x, m))
        for i, e in enumerate(engines):
            if not guarded[i] or saved[i] == _lib.RANGE_IGNORE:
                continue
            mine = [k for k, m in enumerate(models) if m.engine is e]
            with torch.cuda.stream(stream_of[mine[0]]):
                if e.range_status()[0]:       # the flag is sticky: one look covers every source this engine served
                    if saved[i] == _lib.RANGE_ERROR:
                        raise _lib.GlowkRangeError("BASIS: a prior's gradient left the fp16 range of the split arithmetic")
                    prec = e.get_precision()
                    e.set_precision(_lib.PREC_F32)
                    for k in mine:
                        out[k] = compute_grad_logprob(xs[k], models[k])
                    e.set_precision(prec)
    finally:
        for e, gd, pol in zip(engines, guarded, saved):
            if gd:
                e.set_range_policy(pol)
    for st in used:
        cur.wait_stream(st)
    for g in out:
        g.record_stream(cur)
    return out


def _side_streams(streams, models, device):
    """``streams`` of the loops: "auto" becomes one side stream per distinct engine on the GPU, at most four (None for one engine
    or CPU tensors); anything else is passed through."""
    if not (isinstance(streams, str) and streams == "auto"):
        return streams
    distinct = len({id(getattr(m, "engine", m)) for m in models})
    if device.type == "cuda" and distinct > 1:
        return [torch.cuda.Stream(device=device) for _ in range(min(distinct, MAX_SIDE_STREAMS))]
    return None


def _step_sizes(sigma_idx, sigmas, delta):
    """-> (eta, lambda_recon) of noise level ``sigma_idx`` (run_basis_sep.py:157-161)."""
    sigma = float(sigmas[sigma_idx])
    sigma_l = float(sigmas[-1])
    return float(np.float32(delta * (sigma / sigma_l) ** 2)), 1.0 / (sigma ** 2)


def basis_inner_loop_n(mixed, xs, models, sigma_idx, sigmas, delta=2e-5, T=100, noise_fn=None, debug=False, streams="auto", seed=0,
                       step0=0, offset=0, prior_group=None, prior_index=None, mixing="db"):
    """run_basis_sep.py:152-214 (model_type == 'glow') for S = len(xs) sources -> list of S tensors.  ``noise_fn(t, k, shape) ->
    standard normal tensor`` replays given draws for source k at step t; without it the update kernel draws from the device RNG
    at (seed, step0 + t), source k from stream ``k & 1`` of pair ``k >> 1``, element ``offset`` onwards (``offset`` = this shard's
    first tile * H * W * C: the draws of a tile are the same whatever the sharding).
    ``streams``: "auto" (on the GPU, one side stream per distinct engine, at most four), None, or a sequence of streams.
    ``debug``: the reference's NaN asserts (:183-191), from a flag the update kernel raises (one word read back per step).
    ``prior_group`` / ``prior_index``: prior-parallel mode -- this rank evaluates the gradient of prior ``prior_index`` only (the
    other models may be None), the group all-gathers the S gradients (``exchange_prior_gradients_n``) and every rank takes the
    same update; the noise must then be the same on all of them (the device RNG with equal seed / step0 / offset is; an injected
    ``noise_fn`` has to be)."""
    _mixing_id(mixing)
    xs, models = list(xs), list(models)
    S = len(xs)
    if S < 2 or S > MAX_SOURCES:
        raise ValueError("BASIS: the number of sources must be 2..%d, got %d" % (MAX_SOURCES, S))
    if len(models) != S:
        raise ValueError("BASIS: %d states need %d priors, got %d" % (S, S, len(models)))
    pp = prior_group is not None
    if pp and (not isinstance(prior_index, int) or not 0 <= prior_index < S):
        raise ValueError("prior_index must be 0..%d in prior-parallel mode" % (S - 1))
    on_gpu = xs[0].device.type == "cuda"
    streams = None if pp else _side_streams(streams, models, xs[0].device)
    eta, lambda_recon = _step_sizes(sigma_idx, sigmas, delta)

    def grads(cur):
        if not pp:
            return _grad_n(cur, models, streams)
        return exchange_prior_gradients_n(compute_grad_logprob(cur[prior_index], models[prior_index]), prior_index, prior_group)

    if not on_gpu:
        return _inner_loop_host_n(mixed, xs, grads, eta, lambda_recon, T, noise_fn, debug, mixing)
    mixed = mixed.to(torch.float32).contiguous()
    xs = [x.to(torch.float32).clone().contiguous() for x in xs]   # (the update is in place)
    flag = torch.zeros(1, dtype=torch.int32, device=xs[0].device) if debug else None
    for t in range(T):
        gs = grads(xs)
        eps = [noise_fn(t, k, xs[k].shape) for k in range(S)] if noise_fn is not None else None
        langevin_update_n(mixed, xs, gs, eta, lambda_recon, eps, seed=seed, step=step0 + t, nonfinite=flag, offset=offset, mixing=mixing)
        if debug:
            assert int(flag.item()) == 0, (float(sigmas[sigma_idx]), t)   # run_basis_sep.py:183-191
    return xs


def _inner_loop_host_n(mixed, xs, grads, eta, lambda_recon, T, noise_fn, debug, process):
    """The same loop on torch formulas (CPU tensors).  ``grads(xs) -> list of S gradients``."""
    if noise_fn is None:
        noise_fn = lambda t, k, shape: torch.randn(shape, dtype=torch.float32)  # noqa: E731
    for t in range(T):
        z = [noise_fn(t, k, x.shape) for k, x in enumerate(xs)]
        xs = _update_host_n(mixed, xs, grads(xs), z, eta, lambda_recon, process)
        if debug:
            assert all(torch.isfinite(x).all() for x in xs), t
    return xs


def _models_at_level(models, restores, sigma, prior_group=None, prior_index=None):
    """The S priors with their weights for noise level ``sigma`` (``restores`` as in ``basis_outer_loop_n``); None for a prior that
    another rank of ``prior_group`` owns."""
    current = []
    for k, (model, restore) in enumerate(zip(models, restores)):
        if prior_group is not None and k != prior_index:
            current.append(None)          # another rank of the group owns this prior
            continue
        if restore is not None:
            state = restore[float(sigma)] if float(sigma) in restore else restore[sigma]
            if hasattr(state, "log_prob"):      # a resident flow for this noise level: no weight swap at all
                model = state
            elif isinstance(state, str):
                model.restore(state)            # ~0.4 s for config B (host re-pack on 16 threads + 0.5 GB upload)
            else:
                model.load_state_dict(state)
        current.append(model)
    return current


def basis_outer_loop_n(mixed, xs, models, sigmas, restores=None, T=100, delta=2e-5, noise_fn=None, debug=False, seed=0, tile_offset=0,
                       prior_group=None, prior_index=None, mixing="db"):
    """run_basis_sep.py:217-260 for S sources.  ``restores``: None, or a list of S entries, each None or ``{sigma: state_dict |
    path | GlowFlow}`` with the noise-conditioned weights of that prior for each noise level (the per-sigma checkpoints of
    train_noisy_glow.py:309-358); a ``GlowFlow`` value is used as is (all ten noise levels of two priors resident: 2 x 10 x 0.5 GB
    of packed weights).  ``noise_fn(sigma_idx, t, k, shape)``.
    ``tile_offset``: index of ``mixed[0]`` in the whole set of mixture tiles (``shard_bounds(n_mixed, world, rank)[0]`` on a rank
    that holds a shard): folded into the device RNG's counter, so every tile sees the Langevin noise it would see in a
    one-process run -- ranks do not repeat each other's draws and the result does not depend on the world size.
    Returns ``(xs, x_arr)``: the list of S final states and the trajectory ``{"x1": [...], .., "xS": [...]}`` (start state and
    one entry per level).  In prior-parallel mode (``basis_inner_loop_n``) only the own prior's model and restore map are used;
    the others may be None."""
    xs, models = list(xs), list(models)
    S = len(xs)
    if len(models) != S or (restores is not None and len(restores) != S):
        raise ValueError("BASIS: %d states need %d priors (and restore maps)" % (S, S))
    restores = [None] * S if restores is None else list(restores)
    elems_per_tile = int(np.prod(mixed.shape[1:]))
    x_arr = {"x%d" % (k + 1): [x.cpu().numpy()] for k, x in enumerate(xs)}
    for sigma_idx, sigma in enumerate(sigmas):
        current = _models_at_level(models, restores, sigma, prior_group, prior_index)
        nf = None if noise_fn is None else (lambda t, k, shape, _s=sigma_idx: noise_fn(_s, t, k, shape))
        xs = basis_inner_loop_n(mixed, xs, current, sigma_idx, sigmas, delta=delta, T=T, noise_fn=nf, debug=debug, seed=seed,
                                step0=sigma_idx * T, offset=int(tile_offset) * elems_per_tile, prior_group=prior_group,
                                prior_index=prior_index, mixing=mixing)
        for k, x in enumerate(xs):
            x_arr["x%d" % (k + 1)].append(x.cpu().numpy())
    return xs, x_arr


# ---- one chain over a whole signal: the state is the signal's frames, the priors see its overlapping tiles -------------------------
MAX_TILE_WIDTH = 128
MAX_FRAMES = 1 << 20
MAX_ROWS = 1 << 16


def tile_count(n_frames, width, hop):
    """Tiles of ``width`` frames every ``hop`` frames that cover ``n_frames``: 1 if they fit one tile, else
    1 + ceil((n_frames - width) / hop)."""
    return 1 if n_frames <= width else 1 + -(-(n_frames - width) // hop)


def _check_frame_tiling(width, hop):
    for name, v in (("width", width), ("hop", hop)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s: expected an integer, got %r" % (name, v))
    if not 2 <= width <= MAX_TILE_WIDTH:
        raise ValueError("width: expected a tile width in [2, %d], got %d" % (MAX_TILE_WIDTH, width))
    if not 1 <= hop <= width:
        raise ValueError("hop: expected an integer in [1, width = %d], got %d" % (width, hop))


def stitch_window(width, dtype=torch.float32):
    """w[j] = sin^2(pi (j + 1/2) / width), built in float64 and rounded once: the cross-fade weights of ``glowk_tile_stitch``."""
    return (torch.sin(math.pi * (torch.arange(width, dtype=torch.float64) + 0.5) / width) ** 2).to(dtype)


def cut_frames(x, width, hop, pad=-100.0):
    """Frames [rows, F] or [nsig, rows, F] -> tiles [N, rows, width] ([nsig, N, rows, width]), N = ``tile_count(F, width, hop)``:
    tile t holds frames [t hop, t hop + width) and ``pad`` at and beyond F.  A raw gather (``glowk_frames_to_tiles``): no floor and
    no clip, unlike ``audio.frame_tiles`` -- BASIS states leave [-100, 20].  CPU tensors take the torch formula."""
    _check_frame_tiling(width, hop)
    if x.dim() not in (2, 3) or not 1 <= x.shape[-1] <= MAX_FRAMES or not 1 <= x.shape[-2] <= MAX_ROWS:
        raise ValueError("cut_frames: expected [rows, F] or [nsig, rows, F] frames with rows <= %d and 1 <= F <= %d, got %s"
                         % (MAX_ROWS, MAX_FRAMES, tuple(x.shape)))
    rows, F = x.shape[-2:]
    N = tile_count(F, width, hop)
    if not x.is_cuda:
        padded = torch.nn.functional.pad(x, (0, (N - 1) * hop + width - F), value=float(pad))
        return torch.stack([padded[..., t * hop:t * hop + width] for t in range(N)], dim=-3)
    x = x.to(torch.float32).contiguous()
    nsig = x.shape[0] if x.dim() == 3 else 1
    out = torch.empty(tuple(x.shape[:-2]) + (N, rows, width), device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().glowk_frames_to_tiles(_p(x), nsig, rows, F, int(width), int(hop), float(pad), _p(out), _s(x)))
    return out


def stitch_scores(g_tiles, n_frames, hop):
    """Gradient tiles [N, rows, width] -> the prior score of every frame [rows, n_frames]: the mean of the scores the covering tiles
    give it, weighted by ``stitch_window`` at the frame's place in each; gradients with respect to pad cells are dropped.  Torch
    formula in the tiles' dtype (the CPU loop; on the GPU ``glowk_basis_update_frames`` does this in front of its update)."""
    N, rows, width = g_tiles.shape
    w = stitch_window(width, g_tiles.dtype)
    span = (N - 1) * hop + width
    num, den = g_tiles.new_zeros((rows, span)), g_tiles.new_zeros(span)
    for t in range(N):
        num[:, t * hop:t * hop + width] += w * g_tiles[t]
        den[t * hop:t * hop + width] += w
    out = (num / den)[:, :n_frames]
    for f in range(n_frames):                           # a frame under exactly one tile takes that tile's gradient as it is
        t_hi, t_lo = min(N - 1, f // hop), 0 if f < width else (f - width) // hop + 1
        if t_lo == t_hi:
            out[:, f] = g_tiles[t_lo][:, f - t_lo * hop]
    return out


def _as_tiles(g, N, rows, width, what):
    if g.dim() == 4 and g.shape[3] == 1:
        g = g[..., 0]
    if tuple(g.shape) != (N, rows, width):
        raise ValueError("%s: expected [%d, %d, %d] or [%d, %d, %d, 1] tiles, got %s" % (what, N, rows, width, N, rows, width, tuple(g.shape)))
    return g


def langevin_update_frames(mixed, x, g_tiles, width, hop, eta, lambda_recon, eps=None, seed=0, step=0, nonfinite=None, mixing="db",
                           tiles_out=None, pad=-100.0):
    """run_basis_sep.py:163-181 on the frames of a whole signal, IN PLACE on ``x`` [S, rows, F] (contiguous float32), for S
    sources in one kernel (``glowk_basis_update_frames``).  ``g_tiles``: S gradient tensors [N, rows, width(, 1)], source k's the
    gradient of prior k at ``cut_frames(x[k], width, hop)``; frame f takes their cross-fade (``stitch_scores``) as its
    ``grad_logprob``.  ``mixed`` [rows, F].  ``eps``: None, or S entries, each None or [rows, F] standard-normal draws; a source
    without draws takes the device RNG's, stream ``k & 1`` of pair ``k >> 1`` at (seed, step), element b F + f at offset 0.
    ``tiles_out`` (optional, [S, N, rows, width] contiguous float32): receives ``cut_frames`` of the updated ``x``, pad cells
    included -- the tiles of the next step's gradient calls.  CPU tensors take the torch formulas."""
    mid = _mixing_id(mixing)
    _check_frame_tiling(width, hop)
    if x.dim() != 3:
        raise ValueError("langevin_update_frames: expected states [S, rows, F], got %s" % (tuple(x.shape),))
    S, rows, F = x.shape
    N = tile_count(F, width, hop)
    if len(g_tiles) != S or (eps is not None and len(eps) != S):
        raise ValueError("langevin_update_frames: %d states need %d gradients (and noise entries)" % (S, S))
    if tuple(mixed.shape) != (rows, F) or any(e is not None and tuple(e.shape) != (rows, F) for e in (eps or [])):
        raise ValueError("langevin_update_frames: the mixture and the noise must be [rows, F] = [%d, %d]" % (rows, F))
    gs = [_as_tiles(g, N, rows, width, "g_tiles[%d]" % k) for k, g in enumerate(g_tiles)]
    if tiles_out is not None and tuple(tiles_out.shape) != (S, N, rows, width):
        raise ValueError("tiles_out: expected [%d, %d, %d, %d], got %s" % (S, N, rows, width, tuple(tiles_out.shape)))
    if not x.is_cuda:
        xs = list(x)
        z = [e if e is not None else torch.randn((rows, F), dtype=x.dtype) for e in (eps or [None] * S)]
        new = _update_host_n(mixed, xs, [stitch_scores(g, F, hop) for g in gs], z, eta, lambda_recon, mixing)
        x.copy_(torch.stack(new))
        if tiles_out is not None:
            tiles_out.copy_(cut_frames(x, width, hop, pad))
        return
    for t, name in ((x, "x"), (tiles_out, "tiles_out")):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("langevin_update_frames: %s is written in place and must be a contiguous float32 CUDA tensor" % name)
    mixed_c = mixed.to(torch.float32).contiguous()
    gs_c = [g.to(torch.float32).contiguous() for g in gs]
    eps_c = None if eps is None else [e.to(torch.float32).contiguous() if e is not None else None for e in eps]
    _lib.check(_lib.load().glowk_basis_update_frames(_p(x), _ptrs(gs_c), _ptrs(eps_c) if eps_c is not None else None, S, _p(mixed_c),
                                                     rows, F, int(width), int(hop), mid, float(eta), float(lambda_recon), int(seed),
                                                     int(step), float(pad), _p(tiles_out), _p(nonfinite), _s(x)))


def _update_host_n(mixed, xs, gs, z, eta, lambda_recon, process):
    """One step on torch formulas: ``z[k]`` are standard-normal draws."""
    mix = mixing(xs, process)
    ms = grad_mixing(xs, process)
    return [x + eta * (g + lambda_recon * m * (mixed - mix)) + math.sqrt(2.0 * eta) * e for x, g, m, e in zip(xs, gs, ms, z)]


def _check_frames_problem(mixed, x, models, width, tile_hop):
    """The states as one [S, rows, F] tensor, checked against the mixture, the priors and the tiling."""
    x = torch.stack(list(x)) if isinstance(x, (list, tuple)) else x
    if x.dim() != 3:
        raise ValueError("BASIS on frames: expected states [S, rows, F], got %s" % (tuple(x.shape),))
    S, rows, F = x.shape
    if S < 2 or S > MAX_SOURCES:
        raise ValueError("BASIS: the number of sources must be 2..%d, got %d" % (MAX_SOURCES, S))
    if len(models) != S:
        raise ValueError("BASIS: %d states need %d priors, got %d" % (S, S, len(models)))
    _check_frame_tiling(width, tile_hop)
    if not 1 <= F <= MAX_FRAMES or not 1 <= rows <= MAX_ROWS:
        raise ValueError("BASIS on frames: expected rows <= %d and 1 <= F <= %d, got %s" % (MAX_ROWS, MAX_FRAMES, tuple(x.shape)))
    if tuple(mixed.shape) != (rows, F):
        raise ValueError("BASIS on frames: the mixture must be [rows, F] = [%d, %d], got %s" % (rows, F, tuple(mixed.shape)))
    for k, m in enumerate(models):
        shape = getattr(m, "event_shape", None)
        if shape is not None and tuple(int(d) for d in shape) != (rows, width, 1):
            raise ValueError("BASIS on frames: prior %d takes tiles %s, not [rows, width, 1] = [%d, %d, 1]"
                             % (k, tuple(int(d) for d in shape), rows, width))
    return x


def basis_inner_loop_frames(mixed, x, models, sigma_idx, sigmas, width, tile_hop, delta=2e-5, T=100, noise_fn=None, debug=False,
                            streams="auto", seed=0, step0=0, mixing="db"):
    """``basis_inner_loop_n`` as ONE chain over a whole signal -> x [S, rows, F].  The state is the signal's frames ``x`` [S, rows,
    F] (``mixed`` [rows, F]); prior k sees the N = ``tile_count(F, width, tile_hop)`` overlapping tiles of x[k] (``cut_frames``), and
    the score of a frame is the mean of the scores the tiles that cover it give it, weighted by w[j] = sin^2(pi (j + 1/2) / width)
    at the frame's place in each and divided by the weights' sum.  The weights of a frame thus sum to one: the prior pulls on a
    frame as hard as in a per-tile chain, two tiles never hold different values for one frame, and at tile_hop = width this is
    ``basis_inner_loop_n`` on the disjoint tiles.  A step on the GPU is the S gradient evaluations (``_grad_n``: ``streams`` and the
    range-guard handling as in ``basis_inner_loop_n``) and one launch of ``glowk_basis_update_frames``, which also writes the next
    step's tiles.  ``noise_fn(t, k, shape)`` gets the frame shape [rows, F]; without it the kernel draws at (seed, step0 + t).
    There is no prior-parallel mode."""
    _mixing_id(mixing)
    models = list(models)
    x = _check_frames_problem(mixed, x, models, width, tile_hop)
    S, rows, F = x.shape
    streams = _side_streams(streams, models, x.device)
    eta, lambda_recon = _step_sizes(sigma_idx, sigmas, delta)

    def tile_grads(tiles):
        return _grad_n([tiles[k].unsqueeze(-1) for k in range(S)], models, streams)

    if not x.is_cuda:
        def grads(xs):
            return [stitch_scores(g[..., 0], F, tile_hop) for g in tile_grads(cut_frames(torch.stack(xs), width, tile_hop))]
        return torch.stack(_inner_loop_host_n(mixed, list(x), grads, eta, lambda_recon, T, noise_fn, debug, mixing))
    mixed = mixed.to(torch.float32).contiguous()
    x = x.to(torch.float32).clone().contiguous()                  # (the update is in place)
    tiles = cut_frames(x, width, tile_hop)                        # [S, N, rows, width]: rewritten by every update
    flag = torch.zeros(1, dtype=torch.int32, device=x.device) if debug else None
    for t in range(T):
        gs = tile_grads(tiles)
        eps = [noise_fn(t, k, (rows, F)) for k in range(S)] if noise_fn is not None else None
        langevin_update_frames(mixed, x, gs, width, tile_hop, eta, lambda_recon, eps, seed=seed, step=step0 + t, nonfinite=flag,
                               mixing=mixing, tiles_out=tiles)
        if debug:
            assert int(flag.item()) == 0, (float(sigmas[sigma_idx]), t)   # run_basis_sep.py:183-191
    return x


def basis_outer_loop_frames(mixed, x, models, sigmas, width, tile_hop, restores=None, T=100, delta=2e-5, noise_fn=None, debug=False,
                            seed=0, mixing="db"):
    """``basis_outer_loop_n`` over ``basis_inner_loop_frames``: the annealing over ``sigmas`` with the per-level ``restores`` of
    ``basis_outer_loop_n``.  ``noise_fn(sigma_idx, t, k, shape)`` with the frame shape.  Returns ``(x [S, rows, F], x_arr)``, the
    trajectory ``{"x1": [...], .., "xS": [...]}`` of frame arrays (start state and one entry per level)."""
    models = list(models)
    x = _check_frames_problem(mixed, x, models, width, tile_hop)
    S = x.shape[0]
    if restores is not None and len(restores) != S:
        raise ValueError("BASIS: %d states need %d priors (and restore maps)" % (S, S))
    restores = [None] * S if restores is None else list(restores)
    x_arr = {"x%d" % (k + 1): [x[k].cpu().numpy()] for k in range(S)}
    for sigma_idx, sigma in enumerate(sigmas):
        current = _models_at_level(models, restores, sigma)
        nf = None if noise_fn is None else (lambda t, k, shape, _s=sigma_idx: noise_fn(_s, t, k, shape))
        x = basis_inner_loop_frames(mixed, x, current, sigma_idx, sigmas, width, tile_hop, delta=delta, T=T, noise_fn=nf, debug=debug,
                                    seed=seed, step0=sigma_idx * T, mixing=mixing)
        for k in range(S):
            x_arr["x%d" % (k + 1)].append(x[k].cpu().numpy())
    return x, x_arr
