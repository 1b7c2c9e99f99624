"""The NMF formulas of include/glowk.h restated in fp64 numpy, one operation at a time, and the derived error bars the GPU tests
hold the device to.  Nothing here imports the package: the restatement is the reference, not a copy of the code under test.

V [.., R, T] >= 0, W [.., R, K], H [.., K, T]; FLOOR = 2^-40; beta in {0, 1, 2}."""
import numpy as np

FLOOR = 2.0 ** -40
U = 2.0 ** -24

# (nsig, rows, frames, K): single and odd rows; K on both sides of an MFMA tile edge and at the limit; frame counts inside a tile
# and across several W-update chunks; the largest row count
SHAPES = [(1, 1, 1, 1), (1, 33, 95, 5), (3, 65, 33, 32), (2, 257, 130, 33), (1, 1025, 97, 128), (1, 2, 4500, 7), (1, 4096, 66, 2)]
BETAS = (0, 1, 2)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def qp(V, L, beta):
    Le = np.maximum(L, FLOOR)
    if beta == 2:
        return V, Le
    if beta == 1:
        return V / Le, np.ones_like(Le)
    return V / (Le * Le), 1.0 / Le


def g(x, beta):
    return np.sqrt(x) if beta == 0 else x


def update_h(V, W, H, beta):
    V, W, H = f64(V), f64(W), f64(H)
    Q, P = qp(V, W @ H, beta)
    Wt = np.swapaxes(W, -1, -2)
    return H * g((Wt @ Q) / np.maximum(Wt @ P, FLOOR), beta)


def update_w(V, W, H, beta):
    V, W, H = f64(V), f64(W), f64(H)
    Q, P = qp(V, W @ H, beta)
    Ht = np.swapaxes(H, -1, -2)
    return W * g((Q @ Ht) / np.maximum(P @ Ht, FLOOR), beta)


def iterate(V, W, H, beta, update_w_too=True):
    """One iteration: the W update with the old H, then the H update with the new W."""
    if update_w_too:
        W = update_w(V, W, H, beta)
    return W, update_h(V, W, H, beta)


def divergence_terms(V, L, beta):
    V, Le = f64(V), np.maximum(f64(L), FLOOR)
    if beta == 2:
        return 0.5 * (V - Le) ** 2
    if beta == 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(V > 0, V * np.log(np.where(V > 0, V, 1.0) / Le), 0.0)
        return t - V + Le
    q = np.maximum(V, FLOOR) / Le
    return q - np.log(q) - 1.0


def divergence(V, W, H, beta):
    """D_beta(V | W H) per signal."""
    return divergence_terms(V, f64(W) @ f64(H), beta).sum(axis=(-2, -1))


def divergence_weight(V, W, H, beta):
    """sum w of the divergence bar: w = (V + L)^2, V + L, q + 1."""
    V, L = f64(V), f64(W) @ f64(H)
    if beta == 2:
        w = (V + L) ** 2
    elif beta == 1:
        w = V + L
    else:
        w = np.maximum(V, FLOOR) / np.maximum(L, FLOOR) + 1.0
    return w.sum(axis=(-2, -1))


def masks(W, H, sizes, power=1):
    """[.., S, R, T]: m_s = (W_s H_s)^power, mask_s = m_s / sum m, 1 / S where the sum is below FLOOR."""
    W, H = f64(W), f64(H)
    b = np.cumsum([0] + list(sizes))
    m = np.stack([(W[..., :, b[s]:b[s + 1]] @ H[..., b[s]:b[s + 1], :]) ** power for s in range(len(sizes))], axis=-3)
    tot = m.sum(axis=-3, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tot < FLOOR, 1.0 / len(sizes), m / np.where(tot < FLOOR, 1.0, tot))


# ---- the bars: derived from the arithmetic, never from what the device gives ---------------------------------------------------------
def update_bar(K, n):
    """One update fed the device's own inputs: |dev - ref| <= (3 K + 2 n + 16) u ref per element, n = rows for H, frames for W.
    Lambda carries (K + 1) u; Q and P at most (2 K + 3) u and (K + 2) u; each outer chain of n non-negative terms (n + 1) u; the
    division, the square root and the product a few more."""
    return (3 * K + 2 * n + 16) * U


def divergence_bar(K, weight):
    return (K + 4) * U * weight


def mask_bar(K, S, power):
    return power * (2 * K + 2 * S + 8) * U


def mask_sum_bar(S):
    return S * U * 4


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def spectra(shape, seed, silent=0.05):
    """|N(0, 1)|^2 in float32 with about 5 % silent frames, none in a signal of fewer than 8 frames (tests/test_gpu_repet_beat.py's
    inputs)."""
    rng = np.random.default_rng(seed)
    V = (np.abs(rng.standard_normal(shape)) ** 2).astype(np.float32)
    V[..., (rng.random(shape[-1]) < silent) & (shape[-1] >= 8)] = 0.0
    return V


def ratio(err, bar):
    """The largest err / bar; an error of 0 counts as 0 whatever the bar, an error above a bar of 0 as inf."""
    err, bar = np.broadcast_arrays(f64(err), f64(bar))
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / bar).max())


def random_factors(nsig, rows, frames, K, seed):
    rng = np.random.default_rng(seed)
    lead = (nsig,) if nsig != 1 else ()
    return rng.random(lead + (rows, K)).astype(np.float32) + 0.01, rng.random(lead + (K, frames)).astype(np.float32) + 0.01


def two_sources(rows=65, frames=120, sizes=(5, 4), seed=11):
    """Two synthetic sources from disjoint random dictionaries (no atom is shared; every atom lives on a random half of the rows, so
    the sources overlap in most rows) with random sparse activations, and their sum with a random phase: (X complex64 [R, T],
    [W_0, W_1], [M_0, M_1] magnitudes)."""
    rng = np.random.default_rng(seed)
    K = sum(sizes)
    W = ((rng.random((rows, K)) + 0.5) * (rng.random((rows, K)) < 0.5)).astype(np.float32)
    H = (rng.random((K, frames)) * (rng.random((K, frames)) < 0.6)).astype(np.float32)
    b = np.cumsum([0] + list(sizes))
    mags = [W[:, b[s]:b[s + 1]] @ H[b[s]:b[s + 1]] for s in range(len(sizes))]
    phase = np.exp(2j * np.pi * rng.random((rows, frames)))
    X = (sum(mags) * phase).astype(np.complex64)
    return X, [W[:, b[s]:b[s + 1]].copy() for s in range(len(sizes))], mags
