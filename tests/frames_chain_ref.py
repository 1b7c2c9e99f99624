"""Test infrastructure: BASIS as one chain over a whole signal's frames, restated in NumPy (float64 unless a dtype is given) from the
formulas of include/glowk.h, with no code of the package: the cut of frames [rows, F] into overlapping tiles, the prior score of a
frame stitched from the scores of the tiles that cover it, one Langevin step on the frames and the loop.  The update itself and the
mixing processes are those of tests/basis_sources_ref.py, the window and the tile count those of tests/longform_ref.py."""
import numpy as np

from tests import basis_sources_ref as B
from tests import longform_ref as L

tile_count = L.tile_count


def cut(frames, width, hop, pad=-100.0, dtype=np.float64):
    """[..., rows, F] -> [..., N, rows, width]: tile t = frames [t hop, t hop + width), ``pad`` at and beyond F.  A gather: nothing
    is floored or clipped."""
    frames = np.asarray(frames, dtype=dtype)
    F = frames.shape[-1]
    N = tile_count(F, width, hop)
    padded = np.full(frames.shape[:-1] + ((N - 1) * hop + width,), pad, dtype=dtype)
    padded[..., :F] = frames
    return np.stack([padded[..., t * hop:t * hop + width] for t in range(N)], axis=-3)


def covering(f, N, width, hop):
    """The tiles t with 0 <= f - t hop < width, ascending."""
    return [t for t in range(N) if 0 <= f - t * hop < width]


def stitched_score(g_tiles, F, hop):
    """[N, rows, width] -> [rows, F]: s[b, f] = sum_t w[f - t hop] g_t[b, f - t hop] / sum_t w[f - t hop] over the tiles that cover
    f; a frame under one tile takes that tile's gradient itself.  Gradients of pad cells (f >= F) are dropped."""
    g_tiles = np.asarray(g_tiles, dtype=np.float64)
    N, rows, width = g_tiles.shape
    w = L.window(width)
    out = np.empty((rows, F))
    for f in range(F):
        ts = covering(f, N, width, hop)
        if len(ts) == 1:
            out[:, f] = g_tiles[ts[0]][:, f - ts[0] * hop]
        else:
            out[:, f] = sum(w[f - t * hop] * g_tiles[t][:, f - t * hop] for t in ts) / sum(w[f - t * hop] for t in ts)
    return out


def update(mixed, xs, g_tiles, eps, hop, eta, lam, process="db"):
    """One Langevin step on the frames: xs, eps lists of [rows, F]; g_tiles[k] [N, rows, width] the gradient tiles of source k."""
    F = xs[0].shape[1]
    return B.update(mixed, xs, [stitched_score(g, F, hop) for g in g_tiles], eps, eta, lam, process)


def step_sizes(sigma_idx, sigmas, delta):
    sigma, sigma_l = float(sigmas[sigma_idx]), float(sigmas[-1])
    return float(np.float32(delta * (sigma / sigma_l) ** 2)), 1.0 / sigma ** 2


def inner_loop(mixed, xs, grad_fns, width, hop, sigma_idx, sigmas, noise, delta=2e-5, T=100, process="db"):
    """The chain: ``grad_fns[k](tiles [N, rows, width]) -> gradient tiles`` of prior k; noise[t][k] standard-normal [rows, F]."""
    eta, lam = step_sizes(sigma_idx, sigmas, delta)
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    for t in range(T):
        gs = [fn(cut(x, width, hop)) for fn, x in zip(grad_fns, xs)]
        xs = update(mixed, xs, gs, noise[t], hop, eta, lam, process)
    return xs


def glow_grad_fn(params, cfg):
    """The fp64 autograd gradient of a flow prior (oracle.glowref_torch) on tiles [N, rows, width]."""
    from oracle import glowref_torch as RT
    return lambda tiles: RT.log_prob_and_grad(tiles[..., None], params, cfg)[1][..., 0]


def tiles_of_frames(a, width):
    """[..., rows, n width] -> [..., n, rows, width]: the disjoint tiles (hop = width) of frames, a permutation."""
    a = np.asarray(a)
    rows, F = a.shape[-2:]
    return np.moveaxis(a.reshape(a.shape[:-1] + (F // width, width)), -2, -3)
