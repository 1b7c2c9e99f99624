"""NumPy restatement of REPET-SIM's nearest-neighbour filter (a helper of the REPET tests, not a test module): the cosine
similarity of frames in fp64, the neighbour rule (candidates at least ``width`` frames away, the k most similar in decreasing
similarity, equal similarities to the lower index, -1 past the candidate count), the median over gathered columns by sorting,
``rep`` / ``res``, and the masks of tests/hpss_ref.py.  Written from the formulas of include/glowk.h and the documented semantics
of librosa.decompose.nn_filter / librosa.segment.recurrence_matrix, with no code of the package.  No sklearn at module level."""
import math

import numpy as np

from tests import hpss_ref as H

TINY = H.TINY                                            # FLT_MIN: the floor of the product of two norms


def default_k(F, width):
    return min(512, max(1, 2 * math.ceil(math.sqrt(max(F - 2 * width + 1, 1)))))


def similarity(S):
    """sim [F, F] in fp64 of one spectrum S [rows, F]: <S[:, i], S[:, j]> / max(|S[:, i]| |S[:, j]|, FLT_MIN)."""
    S = np.asarray(S, dtype=np.float64)
    norm = np.sqrt((S * S).sum(0))
    return (S.T @ S) / np.maximum(norm[:, None] * norm[None, :], TINY)


def select(sim, k, width):
    """The neighbour rule on a similarity matrix [F, F] -> idx [F, k] int32, sim [F, k], kth [F] (the k_i-th largest candidate
    similarity, +inf for a frame without candidates)."""
    F = sim.shape[0]
    idx, val, kth = np.full((F, k), -1, np.int32), np.zeros((F, k)), np.full(F, np.inf)
    j = np.arange(F)
    for i in range(F):
        cand = j[np.abs(j - i) >= width]
        order = cand[np.argsort(-sim[i, cand], kind="stable")][:k]                 # stable: equal similarities keep index order
        idx[i, :len(order)], val[i, :len(order)] = order, sim[i, order]
        if len(order):
            kth[i] = sim[i, order[-1]]
    return idx, val, kth


def neighbors(S, k, width):
    """idx [.., F, k], sim [.., F, k] of S [rows, F] or [N, rows, F]."""
    S = np.asarray(S)
    if S.ndim == 3:
        out = [neighbors(s, k, width) for s in S]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    return select(similarity(S), k, width)[:2]


def gather_median(S, idx):
    """filt [.., rows, F]: the median over the entries >= 0 of idx[i] of S[:, j], in S's dtype -- the middle of the sorted values, at
    an even count (a + b) * 0.5 of the two middle ones in S's arithmetic; a frame without neighbours stays."""
    S, idx = np.asarray(S), np.asarray(idx)
    if S.ndim == 3:
        return np.stack([gather_median(s, i) for s, i in zip(S, idx)])
    out = np.empty_like(S)
    half = S.dtype.type(0.5)
    for i in range(S.shape[1]):
        nb = idx[i][idx[i] >= 0]
        n = len(nb)
        if n == 0:
            out[:, i] = S[:, i]
            continue
        cols = np.sort(S[:, nb], axis=1)
        out[:, i] = cols[:, n // 2] if n % 2 else (cols[:, n // 2 - 1] + cols[:, n // 2]) * half
    return out


def nn_filter(S, k, width):
    return gather_median(S, neighbors(S, k, width)[0])


def rep_res(S, filt):
    """What repeats and what does not, in fp64: rep = min(S, filt), res = S - rep."""
    S, filt = np.asarray(S, dtype=np.float64), np.asarray(filt, dtype=np.float64)
    rep = np.minimum(S, filt)
    return rep, S - rep


def masks(S, filt, power=2.0, margin=(2.0, 10.0)):
    """(mask_background, mask_foreground) from a spectrum and its filtered version: the two softmasks of tests/hpss_ref.py."""
    rep, res = rep_res(S, filt)
    return H.masks(rep, res, power, margin)


def repet_sim(S, k=None, width=1, power=2.0, margin=(2.0, 10.0), mask=False):
    S = np.asarray(S)
    mag, phase = (np.abs(S), np.exp(1j * np.angle(S))) if np.iscomplexobj(S) else (S, 1.0)
    k = default_k(mag.shape[-1], width) if k is None else k
    mb, mf = masks(mag, nn_filter(mag, k, width), power, margin)
    return (mb, mf) if mask else (mag * mb * phase, mag * mf * phase)


def planted(rng, rows, patterns, copies, noise=0.02):
    """[rows, patterns * copies] float32: ``patterns`` random |N(0, 1)|^2 columns tiled ``copies`` times, every cell times
    1 + noise N(0, 1).  Frame f is a copy of pattern f mod patterns, so its copies sit multiples of ``patterns`` frames away."""
    base = np.abs(rng.standard_normal((rows, patterns))) ** 2
    S = np.tile(base, (1, copies)) * (1.0 + noise * rng.standard_normal((rows, patterns * copies)))
    return np.abs(S).astype(np.float32)


def copies_of(F, patterns):
    """The planted answer: for every frame the set of the other frames of its pattern."""
    return [set(range(i % patterns, F, patterns)) - {i} for i in range(F)]


def pattern_and_chirp(n=48000, sr=16000):
    """(pattern, chirp): a 0.5 s phrase of four 0.125 s notes (two partials each, Hann-faded) repeated to n samples, and a linear
    chirp from 500 Hz to 6 kHz over the whole signal that never repeats.  The mixture is their sum."""
    t = np.arange(n) / sr
    note = int(0.125 * sr)
    fade = np.sin(np.pi * (np.arange(note) + 0.5) / note) ** 0.5
    phrase = np.concatenate([(0.25 * np.sin(2 * np.pi * f * t[:note]) + 0.15 * np.sin(2 * np.pi * 2.5 * f * t[:note])) * fade
                             for f in (330.0, 440.0, 587.0, 392.0)])
    pattern = np.tile(phrase, -(-n // len(phrase)))[:n]
    f0, f1 = 500.0, 6000.0
    chirp = 0.3 * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / t[-1] * t * t))
    return pattern, chirp
