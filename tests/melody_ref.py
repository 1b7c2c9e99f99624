"""The melody separator of include/glowk.h restated in fp64 numpy, one operation at a time: the grid and the position table, the
salience, the emission, the Viterbi path with its order rule, the comb mask, the separator; and the synthetic scene the tests share.
Imports nothing from the package."""
import numpy as np

SR, N_FFT, HOP = 16000, 2048, 512
BIN_HZ = SR / N_FFT
FLOOR = 2.0 ** -40
FLT_MIN = 1.17549435e-38


# ---- section 1: the grid and the tables ------------------------------------------------------------------------------------------------
def f0_grid(fmin=55.0, n_octaves=5, bins_per_octave=60):
    return fmin * 2.0 ** (np.arange(n_octaves * bins_per_octave, dtype=np.float64) / bins_per_octave)


def weights(harmonics=8, decay=0.8):
    return np.float64(decay) ** np.arange(harmonics, dtype=np.float64)


def positions(f0, H, bin_hz, rows):
    """(i, a, live), each [B, H]: p = h f0_b / bin_hz, i = floor(p), a = p - i, live iff i + 1 <= rows - 1."""
    h = np.arange(1, H + 1, dtype=np.float64)
    p = h[None, :] * np.asarray(f0, np.float64)[:, None]
    p = p / np.float64(bin_hz)
    fl = np.floor(p)
    live = fl + 1.0 <= rows - 1
    return np.where(live, fl, 0).astype(np.int64), p - fl, live


# ---- section 2: the salience --------------------------------------------------------------------------------------------------------------
def salience(S, f0, w, bin_hz=BIN_HZ, return_weight=False):
    """S float32 [rows, T] -> sal float32 [B, T]; with ``return_weight`` also the fp64 sum and sum_h |term_h| (the bound's weight)."""
    S = np.asarray(S)
    assert S.dtype == np.float32 and S.ndim == 2
    S64 = S.astype(np.float64)
    w = np.asarray(w, np.float64)
    i, a, live = positions(f0, w.shape[0], bin_hz, S.shape[0])
    acc = np.zeros((len(f0), S.shape[1]))
    weight = np.zeros_like(acc)
    for h in range(w.shape[0]):
        on = live[:, h]
        s0, s1 = S64[i[on, h]], S64[i[on, h] + 1]
        ah = a[on, h][:, None]
        one_minus = 1.0 - ah
        left = one_minus * s0
        right = ah * s1
        both = left + right
        term = w[h] * both
        acc[on] = acc[on] + term
        weight[on] = weight[on] + np.abs(term)
    sal = acc.astype(np.float32)
    return (sal, acc, weight) if return_weight else sal


# ---- section 3: the emission ----------------------------------------------------------------------------------------------------------------
def emission(sal):
    sal = np.asarray(sal)
    assert sal.dtype == np.float32
    m = sal.max()
    den = max(np.float64(m), FLOOR)
    return sal.astype(np.float64) / den, m


# ---- section 4: the track ----------------------------------------------------------------------------------------------------------------------
def penalties(jump_penalty=0.02, max_jump=12):
    return np.float64(jump_penalty) * np.arange(max_jump + 1, dtype=np.float64)


def track(e, threshold=0.2, jump_penalty=0.02, voicing_penalty=0.5, max_jump=12):
    """e float64 [B, T] -> int32 [T] in [0, B].  np.argmax returns the first maximum: a later candidate replaces the best only if it is
    strictly greater.  Row b of the candidate table holds state B first, then b' = b - J .. b + J ascending (-inf outside the grid)."""
    e = np.asarray(e, np.float64)
    B, T = e.shape
    J, theta, nu = int(max_jump), np.float64(threshold), np.float64(voicing_penalty)
    pen = penalties(jump_penalty, J)
    pen_row = pen[np.abs(np.arange(-J, J + 1))]
    D = np.concatenate([e[:, 0], [theta]])
    back = np.zeros((T, B + 1), np.int64)
    padded = np.full(B + 2 * J, -np.inf)
    first_bin = np.arange(B) - J
    for t in range(1, T):
        padded[J:J + B] = D[:B]
        cand = np.empty((B, 2 * J + 2))
        cand[:, 0] = D[B] - nu
        cand[:, 1:] = np.lib.stride_tricks.sliding_window_view(padded, 2 * J + 1) - pen_row[None, :]
        k = np.argmax(cand, axis=1)
        best = cand[np.arange(B), k]
        back[t, :B] = np.where(k == 0, B, first_bin + k - 1)
        un = np.concatenate([[D[B]], D[:B] - nu])
        ku = int(np.argmax(un))
        back[t, B] = B if ku == 0 else ku - 1
        new = np.empty(B + 1)
        new[:B] = e[:, t] + best
        new[B] = theta + un[ku]
        D = new
    path = np.empty(T, np.int32)
    s = int(np.argmax(D))
    for t in range(T - 1, 0, -1):
        path[t] = s
        s = int(back[t, s])
    path[0] = s
    return path


def track_loops(e, threshold, jump_penalty, voicing_penalty, max_jump):
    """The same path by the plainest loops (small planes only): the check of ``track``'s candidate table."""
    e = np.asarray(e, np.float64)
    B, T = e.shape
    pen = penalties(jump_penalty, max_jump)
    D = [e[b, 0] for b in range(B)] + [np.float64(threshold)]
    back = []
    for t in range(1, T):
        new, arg = [], []
        for b in range(B):
            best, who = D[B] - voicing_penalty, B
            for c in range(max(0, b - max_jump), min(B - 1, b + max_jump) + 1):
                v = D[c] - pen[abs(b - c)]
                if v > best:
                    best, who = v, c
            new.append(e[b, t] + best)
            arg.append(who)
        best, who = D[B], B
        for c in range(B):
            v = D[c] - voicing_penalty
            if v > best:
                best, who = v, c
        new.append(threshold + best)
        arg.append(who)
        D = new
        back.append(arg)
    s = 0
    for c in range(B + 1):
        if D[c] > D[s]:
            s = c
    path = [s]
    for arg in reversed(back):
        s = arg[s]
        path.append(s)
    return np.array(path[::-1], np.int32)


# ---- section 5: the mask --------------------------------------------------------------------------------------------------------------------------
def harmonic_mask(path, f0, rows=1025, n_harmonics=20, width=40.0, bin_hz=BIN_HZ, as_float64=False):
    path = np.asarray(path)
    f0 = np.asarray(f0, np.float64)
    B, T = len(f0), path.shape[0]
    x = np.arange(rows, dtype=np.float64) * np.float64(bin_hz)
    out = np.zeros((rows, T))
    on = np.nonzero((path >= 0) & (path < B))[0]
    if len(on):
        g = f0[path[on]]
        d = np.full((rows, len(on)), np.inf)
        for h in range(1, n_harmonics + 1):
            d = np.minimum(d, np.abs(x[:, None] - np.float64(h) * g[None, :]))
        out[:, on] = np.maximum(0.0, 1.0 - d / np.float64(width))
    return out if as_float64 else out.astype(np.float32)


# ---- section 6: the separator ------------------------------------------------------------------------------------------------------------------------
def softmask(X, R, power):
    """glowk_hpss_mask's mask of X against R (librosa.util.softmask, split_zeros), in fp64."""
    X, R = np.asarray(X, np.float64), np.asarray(R, np.float64)
    if np.isinf(power):
        return (X > R).astype(np.float64)                  # the hard mask, zeros included
    Z = np.maximum(X, R)
    bad = Z < FLT_MIN
    Z = np.where(bad, 1.0, Z)
    m, r = (X / Z) ** power, (R / Z) ** power
    return np.where(bad, 0.5, m / np.where(bad, 1.0, m + r))


def melody(S, f0=None, w=None, bin_hz=BIN_HZ, threshold=0.2, jump_penalty=0.02, voicing_penalty=0.5, max_jump=12, n_harmonics=20,
           width=40.0, power=2.0):
    """|S| float32 [rows, T] -> (mask_lead, mask_accompaniment, path, f0 track): the final masks, to be multiplied with S."""
    S = np.asarray(S, np.float32)
    f0 = f0_grid() if f0 is None else np.asarray(f0, np.float64)
    w = weights() if w is None else w
    sal = salience(S, f0, w, bin_hz)
    e, _ = emission(sal)
    path = track(e, threshold, jump_penalty, voicing_penalty, max_jump)
    m = harmonic_mask(path, f0, S.shape[0], n_harmonics, width, bin_hz)
    if power == 1:
        ml, ma = m.astype(np.float64), (np.float32(1.0) - m).astype(np.float64)
    else:
        first_l, first_a = m * S, (np.float32(1.0) - m) * S
        ml, ma = softmask(first_l, first_a, power), softmask(first_a, first_l, power)
    return ml, ma, path, np.concatenate([f0, [0.0]])[path]


# ---- the scene ----------------------------------------------------------------------------------------------------------------------------------------
def scene(seconds=4.0, seed=0):
    """(lead, accompaniment, f0_true, lead_on): two float32 signals at 16 kHz and, per STFT frame (hop 512, centred), the lead's true
    fundamental and whether the lead sounds.  The lead is a vibrato glide from 440 to 622 Hz with 10 harmonics, on from 0.5 s to 3.6 s;
    the accompaniment is a decaying 8-harmonic note every 0.25 s, between 131 and 330 Hz, and a little noise.  Never modified."""
    n = int(seconds * SR)
    t = np.arange(n) / SR
    glide = 440.0 * (622.0 / 440.0) ** (t / seconds)
    f_lead = glide * (1.0 + 0.01 * np.sin(2 * np.pi * 5.5 * t))
    phase = 2 * np.pi * np.cumsum(f_lead) / SR
    env = np.clip((t - 0.5) / 0.02, 0, 1) * np.clip((3.6 - t) / 0.02, 0, 1)
    lead = sum(np.sin(h * phase) / h for h in range(1, 11)) * env * 0.3
    notes = [130.81, 164.81, 196.00, 261.63, 329.63, 220.00, 174.61, 146.83]
    acc = np.zeros(n)
    step = SR // 4
    for k in range(n // step):
        f = notes[k % len(notes)]
        tt = np.arange(n - k * step) / SR
        note = sum(np.sin(2 * np.pi * h * f * tt) / h for h in range(1, 9)) * np.exp(-tt / 0.4) * np.clip(tt / 0.005, 0, 1)
        acc[k * step:] += 0.25 * note
    acc += 0.003 * np.random.default_rng(seed).standard_normal(n)
    frames = 1 + n // HOP
    centre = np.arange(frames) * HOP
    f0_true = f_lead[np.minimum(centre, n - 1)]
    tc = centre / SR
    lead_on = (tc >= 0.5) & (tc <= 3.6)
    return lead.astype(np.float32), acc.astype(np.float32), f0_true, lead_on


def stft(y):
    """Centred STFT, periodic Hann window of 2048, hop 512, reflect padding: complex128 [1025, 1 + n // 512]."""
    y = np.asarray(y, np.float64)
    pad = np.pad(y, N_FFT // 2, mode="reflect")
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)
    frames = np.lib.stride_tricks.sliding_window_view(pad, N_FFT)[::HOP]
    return np.fft.rfft(frames * win, axis=1).T


def sdr(true, est):
    """10 log10 of |true|^2 over |true - est|^2, summed over the STFT plane."""
    return 10 * np.log10((np.abs(true) ** 2).sum() / (np.abs(true - est) ** 2).sum())


def scene_figures(X_lead, X_acc, X_mix, f0_true, lead_on, mask_l, mask_a, f0_hat):
    """(frames of the lead within 50 cents, lead frames, SDR gain of the lead, SDR gain of the accompaniment) of masks applied to X_mix."""
    voiced = f0_hat > 0
    cents = np.full(len(f0_hat), np.inf)
    cents[voiced] = 1200 * np.abs(np.log2(f0_hat[voiced] / f0_true[voiced]))
    hit = int((lead_on & (cents <= 50)).sum())
    gain_l = sdr(X_lead, mask_l * X_mix) - sdr(X_lead, X_mix)
    gain_a = sdr(X_acc, mask_a * X_mix) - sdr(X_acc, X_mix)
    return hit, int(lead_on.sum()), gain_l, gain_a
