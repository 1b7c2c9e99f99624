"""NumPy restatement of kernel additive modelling (a helper of the KAM tests, not a test module): the kernel builders, the median over a
sparse kernel by a stable sort of the gathered neighbours, the back-fitting step in fp64, the loop, the audio pipeline on the STFT pair
of tests/audio_ref.py, and the launch-geometry and workspace rules of csrc/glowk_kam_index.h.  Written from the formulas of
include/glowk.h, with no code of the package."""
import numpy as np

from tests import audio_ref as A
from tests import longform_ref as L
from tests import repet_beat_ref as B
from tests import repet_ref as R

TINY = float(np.finfo(np.float32).tiny)                  # FLT_MIN
MAX_N, MAX_DROW, MAX_DFRAME = 127, 4095, 32767


# ---- kernels ---------------------------------------------------------------------------------------------------------------------------------
def harmonic(size):
    return np.array([(0, d) for d in range(-(size // 2), size // 2 + 1)], np.int32)


def percussive(size):
    return np.array([(d, 0) for d in range(-(size // 2), size // 2 + 1)], np.int32)


def periodic(period, repeats):
    return np.array([(0, i * period) for i in range(-repeats, repeats + 1)], np.int32)


def cross(rows, frames):
    return np.array([(0, d) for d in range(-(frames // 2), frames // 2 + 1)] + [(d, 0) for d in range(-(rows // 2), rows // 2 + 1) if d], np.int32)


def rectangle(rows, frames):
    return np.array([(dr, df) for dr in range(-(rows // 2), rows // 2 + 1) for df in range(-(frames // 2), frames // 2 + 1)], np.int32)


# ---- the median over a sparse kernel ---------------------------------------------------------------------------------------------------------
def gather(S, table):
    """(vals [n, rows, F] in S's dtype, +inf where the neighbour lies outside the plane; ok [n, rows, F])."""
    rows, F = S.shape
    n = len(table)
    vals = np.full((n, rows, F), np.inf, S.dtype)
    ok = np.zeros((n, rows, F), bool)
    for e, (dr, df) in enumerate(np.asarray(table).tolist()):
        r0, r1, t0, t1 = max(0, -dr), min(rows, rows - dr), max(0, -df), min(F, F - df)
        if r0 < r1 and t0 < t1:
            vals[e, r0:r1, t0:t1] = S[r0 + dr:r1 + dr, t0 + df:t1 + df]
            ok[e, r0:r1, t0:t1] = True
    return vals, ok


def median(S, table):
    """The median over the neighbours (r + d_row, t + d_frame) inside the plane, in S's dtype: m odd, the middle of the sorted values; m
    even, (a + b) * 0.5 of the two middle ones in S's arithmetic; m = 0, the cell itself.  Of values that compare equal (-0 and +0) the
    first in table order: a stable sort keeps table order inside a run of equal values, and the run of the element at position p
    starts at #(values < it)."""
    S = np.asarray(S)
    if S.ndim == 3:
        return np.stack([median(s, table) for s in S])
    vals, ok = gather(S, table)
    m = ok.sum(0)
    srt = np.take_along_axis(vals, np.argsort(vals, axis=0, kind="stable"), 0)

    def pick(p):
        x = np.take_along_axis(srt, p[None], 0)
        return np.take_along_axis(srt, (srt < x).sum(0)[None], 0)[0]

    m1 = np.maximum(m, 1)
    a, b = pick((m1 - 1) // 2), pick(m1 // 2)
    with np.errstate(invalid="ignore"):
        even = (a + b) * S.dtype.type(0.5)
    return np.where(m == 0, S, np.where(m % 2 == 1, a, even)).astype(S.dtype)


def median_brute(S, table):
    """The same, one cell at a time with Python lists: the check of ``median``."""
    S = np.asarray(S)
    rows, F = S.shape
    out = np.empty_like(S)
    half = S.dtype.type(0.5)
    for r in range(rows):
        for t in range(F):
            nb = [S[r + dr, t + df] for dr, df in np.asarray(table).tolist() if 0 <= r + dr < rows and 0 <= t + df < F]
            m = len(nb)
            if m == 0:
                out[r, t] = S[r, t]
                continue
            srt = sorted(nb)
            first = lambda x: next(v for v in nb if v == x)
            out[r, t] = first(srt[m // 2]) if m % 2 else (first(srt[m // 2 - 1]) + first(srt[m // 2])) * half
    return out


# ---- the back-fitting step ---------------------------------------------------------------------------------------------------------------------
def backfit(V, A, power=2.0):
    """fp64: A [.., J, rows, F], V [.., rows, F] -> (P, masks) shaped like A."""
    V, A = np.asarray(V, np.float64), np.asarray(A, np.float64)
    J = A.shape[-3]
    Z = A.max(axis=-3, keepdims=True)
    bad = Z < TINY
    r = (A / np.where(bad, 1.0, Z)) ** power
    total = np.zeros_like(Z)
    for j in range(J):                                   # ascending j
        total = total + r[..., j:j + 1, :, :]
    masks = np.where(bad, 1.0 / J, r / np.where(bad, 1.0, total))
    return V[..., None, :, :] * masks, masks


def filter_model(P, model):
    """One source's filter: an offset table, or ("index", idx [.., F, k])."""
    if isinstance(model, tuple) and model[0] == "index":
        return R.gather_median(P, model[1])
    return median(P, model)


def fit(V, models, n_iter=3, power=2.0, dtype=np.float64):
    """(P, masks) [.., J, rows, F]: P_j = V; n_iter times A_j = filter_j(P_j), then the back-fit.  The medians select, so they carry
    ``dtype``'s values; the masks are fp64."""
    V = np.asarray(V).astype(dtype)
    P = np.stack([V] * len(models), axis=-3)
    masks = None
    for _ in range(n_iter):
        Af = np.stack([filter_model(P[..., j, :, :], m) for j, m in enumerate(models)], axis=-3)
        P, masks = backfit(V, Af, power)
        P = P.astype(dtype)
    return P, masks


# ---- audio -------------------------------------------------------------------------------------------------------------------------------------
def models_of(mag, sources, kernel_size=31, period_sec=(0.8, 8.0), k=None, width_sec=2.0, sr=16000, hop=512):
    F = mag.shape[-1]
    out = []
    for s in sources:
        if isinstance(s, str) and s == "harmonic":
            out.append(harmonic(kernel_size))
        elif isinstance(s, str) and s == "percussive":
            out.append(percussive(kernel_size))
        elif isinstance(s, str) and s == "repeating":
            fps = sr / hop
            pmin, pmax = max(1, int(np.ceil(period_sec[0] * fps))), min(int(np.floor(period_sec[1] * fps)), F // 3)
            period = B.find_period(B.beat_spectrum(mag, pmax + 1), pmin, pmax)
            out.append(("index", B.period_neighbors(period, F, min(512, -(-F // pmin)))))
        elif isinstance(s, str) and s == "similar":
            width = max(1, int(width_sec * sr / hop))
            out.append(("index", R.neighbors(mag, R.default_k(F, width) if k is None else k, width)[0]))
        else:
            out.append(np.asarray(s, np.int32))
    return out


def kam_audio(y, sources=("harmonic", "percussive"), n_iter=3, power=2.0, kernel_size=31, **kw):
    """One signal [n] at 16 kHz -> the stems [J, n] in fp64: zero-pad to a hop multiple, STFT, ``fit`` on |X| (rounded to float32, as the
    device holds it), the masks times X, iSTFT, the first n samples."""
    y = np.asarray(y, dtype=np.float64)
    X = A.stft(L.pad_hop(y))
    mag = np.abs(X).astype(np.float32)
    P, _ = fit(mag, models_of(mag, sources, kernel_size, **kw), n_iter, power)
    phase = np.exp(1j * np.angle(X))
    return np.stack([A.istft(p * phase)[:len(y)] for p in P])


def scene(n=40000, sr=16000, period=8, hop=512):
    """(sines, clicks, motif), whose sum is the mixture:
    sines: two sine voices of amplitude 0.3 and 0.2 with continuous phase, the first stepping every 13 frames and the second every 11
      among the twelve semitones above 440 and 1320 Hz (a seeded draw).  A tone that never moves repeats at EVERY period and would
      belong to the harmonic and the periodic model alike; one that moves is horizontal but not periodic;
    clicks: 0.8 Hann(32) clicks of alternating sign every 5000 samples from sample 2300 (not a multiple of the period);
    motif: a chord of 2500, 3100 and 3700 Hz, 0.1 each, under a Hann window of 1536 samples, every ``period`` frames from sample 1024:
      three frames long, so neither a horizontal run of nine nor a vertical one holds it."""
    rng = np.random.default_rng(7)

    def voice(base, frames, amp):
        f = np.repeat(base * 2.0 ** (rng.integers(0, 12, -(-n // (frames * hop))) / 12.0), frames * hop)[:n]
        return amp * np.sin(2 * np.pi * np.cumsum(f) / sr)

    sines = voice(440.0, 13, 0.3) + voice(1320.0, 11, 0.2)
    clicks = np.zeros(n)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(32) / 32)
    for i, at in enumerate(range(2300, n - 32, 5000)):
        clicks[at:at + 32] += (0.8 if i % 2 == 0 else -0.8) * hann
    m = 1536
    u = np.arange(m) / sr
    chord = 0.1 * sum(np.sin(2 * np.pi * f * u) for f in (2500.0, 3100.0, 3700.0)) * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(m) / m))
    motif = np.zeros(n)
    for at in range(1024, n - m, period * hop):
        motif[at:at + m] += chord
    return sines, clicks, motif


def fractions(stems, components):
    """frac[c][j] = sum_tf |STFT stem_j| |STFT component_c|, divided by its sum over j: the share of component c's time-frequency
    support that stem j holds (fp64, on the host)."""
    S = np.stack([np.abs(A.stft(L.pad_hop(np.asarray(s, np.float64)))) for s in stems])
    C = np.stack([np.abs(A.stft(L.pad_hop(np.asarray(c, np.float64)))) for c in components])
    d = np.einsum("crt,jrt->cj", C, S)
    return d / d.sum(axis=1, keepdims=True)


# ---- the rules of csrc/glowk_kam_index.h -------------------------------------------------------------------------------------------------------
TILE_F, MAX_WAVES, LDS_LIMIT = 64, 4, 65536


def waves(n):
    return MAX_WAVES if MAX_WAVES * 256 * n <= LDS_LIMIT else 1


def lds_bytes(n):
    return 256 * n * waves(n)


def ftiles(frames):
    return -(-frames // TILE_F)


def units(nsig, rows, frames):
    return nsig * rows * ftiles(frames)


def blocks(nsig, rows, frames, n):
    return -(-units(nsig, rows, frames) // waves(n))


def round8(b):
    return (b + 7) // 8 * 8


def work_bytes(nsig, rows, frames, J, has_index):
    """A [nsig][J][rows][frames] float32 rounded up to 8, then glowk_nn_median's workspace for one signal when a source needs it."""
    return round8(4 * nsig * J * rows * frames) + (round8(4 * frames * (rows + 1)) if has_index else 0)
