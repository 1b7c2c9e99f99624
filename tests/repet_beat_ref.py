"""NumPy restatement of REPET's front end in fp64 (a helper of the REPET tests, not a test module): the windows of the beat
spectrogram, the beat value as a plain sum over the pairs of frames inside a window (slices, never a Gram matrix), its
normalisation, the period rule and the order of the periodic neighbours; then REPET itself with ``gather_median``, ``rep_res`` and
the masks of tests/repet_ref.py.  Written from the formulas of include/glowk.h, with no code of the package."""
import numpy as np

from tests import repet_ref as R


def windows(F, win, step):
    """[(first frame, frame count)] of the windows: win = 0 is the one window [0, F); else window t covers the frames
    [t step - win // 2, t step - win // 2 + win) that lie in [0, F), for t < ceil(F / step)."""
    if win == 0:
        return [(0, F)]
    out = []
    for t in range(-(-F // step)):
        lo = t * step - win // 2
        a, b = max(lo, 0), min(lo + win, F)
        out.append((a, b - a))
    return out


def beat_of_window(S, a, n, nlags):
    """beat [nlags] of frames [a, a + n) of one spectrum S [rows, F]: raw[l] = sum_r sum_j P[r, j] P[r, j + l] / (rows (n - l)) over
    the pairs inside the window, divided by raw[0]; 0 for l >= n; all zeros if raw[0] = 0."""
    P = (np.asarray(S, dtype=np.float64) ** 2)[:, a:a + n]                          # fp64 throughout: the bar covers the fp32 squares
    rows = P.shape[0]
    raw = np.zeros(nlags)
    for l in range(min(nlags, n)):
        raw[l] = (P[:, :n - l] * P[:, l:]).sum() / (rows * (n - l))
    return raw / raw[0] if raw[0] > 0 else np.zeros(nlags)


def beat_spectrogram(S, nlags, win, step):
    """[.., nwin, nlags] fp64 of S [rows, F] or [N, rows, F]."""
    S = np.asarray(S)
    if S.ndim == 3:
        return np.stack([beat_spectrogram(s, nlags, win, step) for s in S])
    return np.stack([beat_of_window(S, a, n, nlags) for a, n in windows(S.shape[1], win, step)])


def beat_spectrum(S, nlags):
    return beat_spectrogram(S, nlags, 0, 0)[..., 0, :]


def find_period(beat, pmin, pmax):
    """int32 [..]: the lag in [pmin, pmax] of largest value, the lowest of equal ones."""
    beat = np.asarray(beat)
    return (pmin + np.argmax(beat[..., pmin:pmax + 1], axis=-1)).astype(np.int32)  # argmax returns the first of equal maxima


def period_neighbors(period, frames, k, step=None):
    """idx int32 [.., frames, k]: period [..] (one per signal) or, with step, [.., nper]."""
    period = np.asarray(period)
    per = period.reshape(-1, 1) if step is None else period.reshape(-1, period.shape[-1])
    lead = period.shape if step is None else period.shape[:-1]
    out = np.full((per.shape[0], frames, k), -1, np.int32)
    for s in range(per.shape[0]):
        for j in range(frames):
            w = 0 if step is None else min((j + step // 2) // step, per.shape[1] - 1)
            p = max(1, int(per[s, w]))
            kept, i = [j], 1
            while len(kept) < k and (j - i * p >= 0 or j + i * p < frames):
                kept += [f for f in (j - i * p, j + i * p) if 0 <= f < frames]
                i += 1
            out[s, j, :min(k, len(kept))] = kept[:k]
    return out.reshape(tuple(lead) + (frames, k))


def masks(S, filt, power=1.0, margin=(1.0, 1.0)):
    return R.masks(S, filt, power, margin)


def best_and_second(beat, pmin, pmax):
    """(argmax lag, its value minus the largest other value in the range)."""
    seg = np.asarray(beat)[pmin:pmax + 1]
    order = np.argsort(-seg, kind="stable")
    return pmin + int(order[0]), float(seg[order[0]] - seg[order[1]]) if len(seg) > 1 else float("inf")


PLANTED = [(33, 12, 5, 0.02), (33, 12, 5, 0.3), (1025, 25, 8, 0.1), (2, 7, 4, 0.02), (1, 5, 6, 0.02)]


def planted_case(case):
    """(S, pmin, pmax) of a planted input: the range (patterns // 2 + 1, min(2 patterns - 1, F // 3)) holds exactly one multiple of
    the planted period."""
    rows, patterns, copies, noise = case
    S = R.planted(np.random.default_rng(rows + patterns), rows, patterns, copies, noise)
    F = S.shape[1]
    return S, patterns // 2 + 1, min(2 * patterns - 1, F // 3)


def bar(rows):
    """The accuracy bar of the device's beat values, relative per element: numerator and denominator each carry at most
    (rows + 2) 2^-24 (one fp32 square per operand, an fp32 chain of ``rows`` non-negative terms); fp64 and the final rounding are
    within the slack of 2 (rows + 8) 2^-24."""
    return 2.0 * (rows + 8) * 2.0 ** -24
