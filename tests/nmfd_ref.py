"""The convolutive NMF formulas of include/glowk.h restated in fp64 numpy, one operation at a time, the derived error bars the GPU
tests hold the device to, and the glide scene.  Nothing here imports the package: the restatement is the reference, not a copy of
the code under test.

V [.., R, T] >= 0, W [.., R, K, Tw], H [.., K, T]; FLOOR = 2^-40; beta in {0, 1, 2}.  The model is written with the shifts
themselves (a loop over tau), never through the stacked NMF problem: that the two agree is a test (tests/test_nmfd_cpu.py)."""
import numpy as np

from tests import nmf_ref as N
from tests import rng_ref

FLOOR, U, BETAS = N.FLOOR, N.U, N.BETAS
f64 = N.f64
NMFD_STREAM = 11

# (nsig, rows, frames, K, Tw): everything degenerate; fewer frames than template frames; an odd stacked count 15 with every edge
# ragged; the largest Tw, a halo as long as a tile that runs past the end, stacked 128, a batch; K = 1 with the halo ending exactly on
# the last frame; stacked 128 over several frame tiles and chunks; the workload's rows with stacked 33 just over an accumulator tile;
# Tw = 1 at the largest K
SHAPES = [(1, 1, 1, 1, 1), (1, 5, 3, 2, 4), (1, 33, 95, 3, 5), (3, 65, 33, 4, 32), (1, 64, 64, 1, 32), (2, 257, 130, 16, 8), (1, 1025, 97, 11, 3),
          (1, 40, 70, 128, 1)]


def shift(A, tau):
    """A [.., n, T] moved tau frames later: out[.., t] = A[.., t - tau], 0 for t < tau."""
    out = np.zeros_like(A)
    if tau < A.shape[-1]:
        out[..., tau:] = A[..., :A.shape[-1] - tau]
    return out


def unshift(A, tau):
    """A [.., n, T] moved tau frames earlier: out[.., t] = A[.., t + tau], 0 for t + tau >= T."""
    out = np.zeros_like(A)
    if tau < A.shape[-1]:
        out[..., :A.shape[-1] - tau] = A[..., tau:]
    return out


def tap(W, tau):
    """W[.., :, :, tau] as a contiguous [.., R, K]."""
    return np.ascontiguousarray(f64(W)[..., tau])


def stack(H, Tw):
    """Hs [.., K Tw, T]: Hs[k Tw + tau, t] = H[k, t - tau], 0 for t < tau."""
    H = np.asarray(H)
    out = np.stack([shift(H, tau) for tau in range(Tw)], axis=-2)                      # [.., K, Tw, T]
    return out.reshape(H.shape[:-2] + (H.shape[-2] * Tw, H.shape[-1]))


def stacked(W):
    """Ws [.., R, K Tw]: W's own memory read as an NMF dictionary."""
    W = np.asarray(W)
    return W.reshape(W.shape[:-2] + (W.shape[-2] * W.shape[-1],))


def lam(W, H):
    """Lambda = sum_tau W[.., tau] shift(H, tau)."""
    H = f64(H)
    L = tap(W, 0) @ H
    for tau in range(1, np.shape(W)[-1]):
        L = L + tap(W, tau) @ shift(H, tau)
    return L


def update_h(V, W, H, beta):
    """The joint update: N[k, t] = sum_tau sum_f W[f, k, tau] Q[f, t + tau] over t + tau < T, D with P, H' = H g(N / max(D, FLOOR))."""
    V, H = f64(V), f64(H)
    Q, P = N.qp(V, lam(W, H), beta)
    Wt = np.swapaxes(tap(W, 0), -1, -2)
    num, den = Wt @ Q, Wt @ P
    for tau in range(1, np.shape(W)[-1]):
        Wt = np.swapaxes(tap(W, tau), -1, -2)
        num, den = num + Wt @ unshift(Q, tau), den + Wt @ unshift(P, tau)
    return H * N.g(num / np.maximum(den, FLOOR), beta)


def update_w(V, W, H, beta):
    """W'[.., tau] = W[.., tau] g(Q shift(H, tau)^T / max(P shift(H, tau)^T, FLOOR))."""
    V, W, H = f64(V), f64(W), f64(H)
    Q, P = N.qp(V, lam(W, H), beta)
    out = np.empty_like(W)
    for tau in range(W.shape[-1]):
        Ht = np.swapaxes(shift(H, tau), -1, -2)
        out[..., tau] = tap(W, tau) * N.g((Q @ Ht) / np.maximum(P @ Ht, FLOOR), beta)
    return out


def iterate(V, W, H, beta, update_w_too=True):
    """One iteration: the W update with the old H, then the H update with the new W."""
    if update_w_too:
        W = update_w(V, W, H, beta)
    return W, update_h(V, W, H, beta)


def divergence(V, W, H, beta):
    return N.divergence_terms(V, lam(W, H), beta).sum(axis=(-2, -1))


def divergence_weight(V, W, H, beta):
    """sum w of the divergence bar: w = (V + L)^2, V + L, q + 1."""
    V, L = f64(V), lam(W, H)
    if beta == 2:
        w = (V + L) ** 2
    elif beta == 1:
        w = V + L
    else:
        w = np.maximum(V, FLOOR) / np.maximum(L, FLOOR) + 1.0
    return w.sum(axis=(-2, -1))


def masks(W, H, sizes, power=1):
    """[.., S, R, T]: m_s = (the model of the components of source s)^power, mask_s = m_s / sum m, 1 / S where the sum is below FLOOR."""
    W, H = f64(W), f64(H)
    b = np.cumsum([0] + list(sizes))
    m = np.stack([lam(W[..., :, b[s]:b[s + 1], :], H[..., b[s]:b[s + 1], :]) ** power for s in range(len(sizes))], axis=-3)
    tot = m.sum(axis=-3, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tot < FLOOR, 1.0 / len(sizes), m / np.where(tot < FLOOR, 1.0, tot))


# ---- the bars: derived from the arithmetic, never from what the device gives ---------------------------------------------------------
def h_bar(K, Tw, rows):
    """nmf_ref.update_bar with a chain of K Tw terms and an outer sum of rows Tw non-negative terms in whatever order."""
    return (3 * K * Tw + 2 * rows * Tw + 16) * U


def w_bar(K, Tw, frames):
    return (3 * K * Tw + 2 * frames + 16) * U


def divergence_bar(K, Tw, weight):
    return N.divergence_bar(K * Tw, weight)


def mask_bar(K, Tw, S, power):
    return N.mask_bar(K * Tw, S, power)


mask_sum_bar = N.mask_sum_bar


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def start(V, K, Tw, seed):
    """``nmfd.init`` from the restated RNG: uniforms of stream 11, step 0 for W and 1 for H in array order, times
    sqrt(mean(V) / (K Tw)) per signal, the mean in float64 and the scale and the products in float32."""
    V = np.asarray(V, np.float32)
    lead, R, T = V.shape[:-2], V.shape[-2], V.shape[-1]
    nw, nh = int(np.prod(lead + (R, K, Tw))), int(np.prod(lead + (K, T)))
    scale = np.sqrt(V.astype(np.float64).mean(axis=(-2, -1), keepdims=True) / (K * Tw)).astype(np.float32)
    W = rng_ref.uniform(seed, step=0, which=NMFD_STREAM, n=nw).astype(np.float32).reshape(lead + (R, K, Tw)) * scale[..., None]
    H = rng_ref.uniform(seed, step=1, which=NMFD_STREAM, n=nh).astype(np.float32).reshape(lead + (K, T)) * scale
    return W, H


def random_problem(shape, seed):
    """(V, W, H) float32 for a shape (nsig, rows, frames, K, Tw): nmf_ref's spectra and plain numpy factors."""
    nsig, rows, frames, K, Tw = shape
    lead = (nsig,) if nsig != 1 else ()
    V = N.spectra(lead + (rows, frames), seed)
    rng = np.random.default_rng(seed + 1)
    s = np.sqrt(max(float(V.mean()), 1e-3) / (K * Tw))
    return V, (rng.random(lead + (rows, K, Tw)) * s).astype(np.float32) + 1e-6, (rng.random(lead + (K, frames)) * s).astype(np.float32) + 1e-6


# ---- the glide scene ----------------------------------------------------------------------------------------------------------------------
SCENE_ROWS, SCENE_FRAMES, SCENE_TW, SCENE_DENSITY, SCENE_FLOOR = 48, 400, 8, 0.04, 1e-3


def glide_patches():
    """[2, rows, Tw]: three partials that glide up one row per frame while they decay, and the time-reversed copy, which glides down
    while it swells.  Their long-term spectra (the sums over the patch's frames) are equal: only the motion tells them apart."""
    up = np.zeros((SCENE_ROWS, SCENE_TW))
    for base, amp in ((5, 1.0), (19, 0.7), (33, 0.5)):
        for tau in range(SCENE_TW):
            up[base + tau, tau] += amp * 0.85 ** tau
            up[base + tau + 1, tau] += 0.3 * amp * 0.85 ** tau
    return np.stack([up, up[:, ::-1]])


def onsets(seed):
    """[2, frames]: sparse onsets of random strength, density 0.04 per source."""
    rng = np.random.default_rng(seed)
    return (rng.random((2, SCENE_FRAMES)) < SCENE_DENSITY) * (0.5 + rng.random((2, SCENE_FRAMES)))


def glide_scene(train_seed=21, test_seed=22):
    """(isolated training material [2, rows, frames], the test sources [2, rows, frames], their mixture), float32; the training and
    the test activations come from different seeds.  Every source lies on a noise floor of 1e-3 (its patches peak at 1): a magnitude
    spectrogram has no exact zeros, and Itakura-Saito, which weighs a silent cell like a loud one, has no minimum with them."""
    P = glide_patches()
    render = lambda A: (np.stack([lam(P[j][:, None, :], A[j][None]) for j in range(2)]) + SCENE_FLOOR).astype(np.float32)
    train, test = render(onsets(train_seed)), render(onsets(test_seed))
    return train, test, (test[0].astype(np.float64) + test[1]).astype(np.float32)


def sdr(ref, est):
    ref, est = f64(ref), f64(est)
    return 10.0 * np.log10((ref ** 2).sum() / max(((ref - est) ** 2).sum(), 1e-300))


def scene_sdrs(Tw, beta, train, test, mix, learn_iter=200, n_iter=100, seed=3, fit=None):
    """Supervised separation of the scene with one component of Tw frames per source: each dictionary from ``learn_iter`` iterations on
    its isolated material from ``start(.., seed)``, then ``n_iter`` H-only iterations on the mixture from ``start(mix, 2, Tw, seed)``,
    and the SDR of the masked mixture magnitude per source.  ``fit(V, W, H, beta, n_iter, update_w)`` -> (W, H) replaces the
    restatement's loop (the GPU test passes the device's)."""
    def loop(V, W, H, beta, n, update_w_too):
        for _ in range(n):
            W, H = iterate(V, W, H, beta, update_w_too)
        return W, H
    fit = fit or loop
    dicts = []
    for j in range(2):
        W0, H0 = start(train[j], 1, Tw, seed)
        dicts.append(np.asarray(fit(train[j], W0, H0, beta, learn_iter, True)[0], dtype=np.float32))
    W = np.concatenate(dicts, axis=1)                                                   # [rows, 2, Tw]
    H0 = start(mix, 2, Tw, seed)[1]
    H = np.asarray(fit(mix, W, H0, beta, n_iter, False)[1])
    m = masks(W, H, (1, 1), 1)
    return [sdr(test[j], m[j] * mix) for j in range(2)]
