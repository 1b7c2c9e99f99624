"""fp64 NumPy restatement of the whole-signal path (a helper of the long-form tests, not a test module), built on tests/audio_ref.py:
the zero-pad to a hop multiple, the mel frames of a whole signal, the tile count, the cut into overlapping tiles, the cross-fade
window, the stitch, and the mask + iSTFT + trim.  Written from the formulas of include/glowk.h, with no code of the package."""
import numpy as np

from tests import audio_ref as A

HOP, NMEL, NBIN = A.HOP, A.NMEL, A.NBIN


def pad_hop(y):
    """[..., n] -> [..., ceil(n / 512) * 512], zeros appended."""
    y = np.asarray(y)
    return np.concatenate([y, np.zeros(y.shape[:-1] + (-y.shape[-1] % HOP,), y.dtype)], axis=-1)


def mel_frames(y, return_stft=False):
    """One signal [n] -> dB frames [96, F], F = 1 + ceil(n / 512), of the zero-padded signal: no top_db floor, clipped to [-100, 20]."""
    X = A.stft(pad_hop(np.asarray(y, dtype=np.float64)))
    L = np.clip(10.0 * np.log10(np.maximum(1e-10, A.mel_filterbank().astype(np.float64) @ (np.abs(X) ** 2))), -100.0, 20.0)
    return (L, X) if return_stft else L


def tile_count(F, width, hop):
    return 1 if F <= width else 1 + int(np.ceil((F - width) / hop))


def cut(frames, width, hop, top_db=None, dtype=np.float64):
    """[96, F] -> [N, 96, width] in ``dtype``: tile k = frames [k hop, k hop + width), -100 past F; the floor at the padded tile's
    max - top_db (one subtraction in ``dtype``), then the clip to [-100, 20]."""
    frames = np.asarray(frames, dtype=dtype)
    F = frames.shape[1]
    N = tile_count(F, width, hop)
    padded = np.full((NMEL, (N - 1) * hop + width), -100.0, dtype=dtype)
    padded[:, :F] = frames
    out = np.stack([padded[:, k * hop:k * hop + width] for k in range(N)])
    if top_db is not None and top_db > 0:
        floor = out.max(axis=(1, 2), keepdims=True) - dtype(top_db)
        out = np.maximum(out, floor)
    return np.clip(out, dtype(-100.0), dtype(20.0))


def window(width):
    """w[j] = sin^2(pi (j + 1/2) / width): strictly positive, w[j] + w[j + width / 2] = 1."""
    return np.sin(np.pi * (np.arange(width) + 0.5) / width) ** 2


def coverage(F, N, width, hop):
    """[F] the number of tiles that cover each frame."""
    c = np.zeros(F, dtype=np.int64)
    for k in range(N):
        c[k * hop:min(F, k * hop + width)] += 1
    return c


def stitch(tiles, F, hop):
    """[N, 96, width] -> [96, F]: the mean over the tiles that cover a frame, weighted by the window at the frame's place in each;
    a frame one tile covers is that tile's value itself."""
    tiles = np.asarray(tiles, dtype=np.float64)
    N, _, width = tiles.shape
    w = window(width)
    num, den = np.zeros((NMEL, (N - 1) * hop + width)), np.zeros((N - 1) * hop + width)
    for k in range(N):
        num[:, k * hop:k * hop + width] += w * tiles[k]
        den[k * hop:k * hop + width] += w
    out = (num / den)[:, :F]
    single = coverage(F, N, width, hop) == 1
    for f in np.nonzero(single)[0]:
        k = min(N - 1, f // hop)
        out[:, f] = tiles[k][:, f - k * hop]
    return out


def mask_istft(powers, X_mix, n, wiener=False):
    """powers [S, 1025, F] + the mixture's STFT [1025, F] -> [S, n]: audio_ref's mask and iSTFT, the first n samples."""
    return np.stack([y[:n] for y in A.masked_istft(list(powers), X_mix, wiener)])


def round_trip(y):
    """zero-pad, STFT, iSTFT, trim: the signal itself."""
    y = np.asarray(y, dtype=np.float64)
    return A.istft(A.stft(pad_hop(y)))[:len(y)]
