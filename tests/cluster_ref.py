"""fp64 numpy restatement of audiosourcesep_amd/cluster.py (csrc/glowk_cluster.h), written for clarity: one signal at a time, features
F [D, R, T] and weights w [R, T].  Every function takes ``dtype`` where the GPU tests need the np.longdouble variant.  Also the a-priori
bound of the statistics (include/glowk.h, "Since version 556"), the partition rules of csrc/glowk_cluster_index.h restated, and the
scene helpers (tests/projet_ref.scene and tests/melody_ref.scene by import)."""
import math
import statistics

import numpy as np

STATUS_ZERO_WEIGHT, STATUS_DEAD, STATUS_CHOLESKY = 1, 2, 4
DEAD = 2.0 ** -40
EPS = 2.0 ** -53
THREADS, WAVE, WAVES, MAX_GROUPS = 256, 64, 4, 1024


# ---- the partition of glowk_cluster_index.h ---------------------------------------------------------------------------------------------
def chunk_cells(cells):
    g = max(1, min(MAX_GROUPS, -(-cells // THREADS)))
    per = -(-cells // g)
    return -(-per // THREADS) * THREADS


def groups(cells):
    return max(1, -(-cells // chunk_cells(cells)))


def chain(R, T):
    cells = R * T
    return chunk_cells(cells) // THREADS * WAVE + WAVES + groups(cells)


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def quantiles(J):
    nd = statistics.NormalDist()
    return np.array([nd.inv_cdf((j + 0.5) / J) for j in range(J)], dtype=np.float64)


def tri_index(D):
    """The (a, b) pairs of the upper triangle in the statistics' order."""
    return [(a, b) for a in range(D) for b in range(a, D)]


def stat_size(D, J):
    return J * (1 + D + D * (D + 1) // 2) + 1


def _cells(F, w=None, dtype=np.float64):
    D = F.shape[0]
    x = np.asarray(F, dtype=np.float32).astype(dtype).reshape(D, -1)
    return x if w is None else (x, np.asarray(w, dtype=np.float32).astype(dtype).reshape(-1))


def _sum(a, reverse=False):
    """The sum over the last axis, cells in natural or reversed order."""
    return (a[..., ::-1] if reverse else a).sum(axis=-1)


def pass0(F, w, dtype=np.float64, reverse=False):
    """W = sum w, o = sum w x / W (0 for W == 0)."""
    x, ww = _cells(F, w, dtype)
    W = _sum(ww, reverse)
    o = _sum(ww * x, reverse) / W if W > 0 else np.zeros(x.shape[0], dtype)
    return W, o


def moments(F, w, o, dtype=np.float64, reverse=False):
    """sum w, sum w u, sum w u u^T of u = x - o."""
    x, ww = _cells(F, w, dtype)
    u = x - np.asarray(o, dtype)[:, None]
    return _sum(ww, reverse), _sum(ww * u, reverse), _sum(ww * u[:, None, :] * u[None, :, :], reverse)


def principal_axis(S0):
    D = S0.shape[0]
    v = np.ones(D)
    for _ in range(64):
        v = S0 @ v
        v = v / math.sqrt(float((v * v).sum()))
    big = int(np.argmax(np.abs(v)))                               # the earliest of equals
    if v[big] < 0:
        v = -v
    return v, float(v @ (S0 @ v))


def init(F, w, J, reg_covar=1e-6, reverse=False):
    """The principal-axis start -> the state dict (fp64) with ``status``."""
    D = F.shape[0]
    W, o = pass0(F, w, reverse=reverse)
    if not W > 0:
        return dict(weights=np.full(J, 1.0 / J), means=np.zeros((J, D)), covariances=np.tile(np.eye(D), (J, 1, 1)), origin=o, total=W,
                    status=STATUS_ZERO_WEIGHT)
    _, a, B = moments(F, w, o, reverse=reverse)
    m = a / W
    S0 = B / W - np.outer(m, m) + reg_covar * np.eye(D)
    v, lam = principal_axis(S0)
    means = (o + m)[None, :] + (quantiles(J) * math.sqrt(lam))[:, None] * v[None, :]
    return dict(weights=np.full(J, 1.0 / J), means=means, covariances=np.tile(S0, (J, 1, 1)), origin=o, total=W, status=0)


def constants(state, dtype=np.float64):
    """k [J] and Linv [J, D, D] of a state; raises np.linalg.LinAlgError on a covariance that is not positive definite."""
    pi, mu, Sg = (np.asarray(state[k], np.float64) for k in ("weights", "means", "covariances"))
    J, D = mu.shape
    k, Linv = np.empty(J, dtype), np.empty((J, D, D), dtype)
    for j in range(J):
        L = _cholesky(Sg[j].astype(dtype))
        Linv[j] = _tri_inverse(L)
        with np.errstate(divide="ignore"):
            k[j] = np.log(np.asarray(pi[j], dtype)) - np.log(np.diagonal(L)).sum() - D * np.log(np.asarray(2 * np.pi, dtype)) / 2
    return k, Linv


def _cholesky(S):
    D = S.shape[0]
    L = np.zeros_like(S)
    for a in range(D):
        for b in range(a + 1):
            s = S[a, b] - (L[a, :b] * L[b, :b]).sum()
            if a == b:
                if not s > 0:
                    raise np.linalg.LinAlgError("not positive definite")
                L[a, a] = np.sqrt(s)
            else:
                L[a, b] = s / L[b, b]
    return L


def _tri_inverse(L):
    D = L.shape[0]
    Li = np.zeros_like(L)
    for b in range(D):
        for a in range(b, D):
            s = (1.0 if a == b else 0.0) - (L[a, b:a] * Li[b:a, b]).sum()
            Li[a, b] = s / L[a, a]
    return Li


def estep(F, state, dtype=np.float64, with_abs=False):
    """-> (l [J, C], lse [C], r [J, C]) and, with_abs, q~ [J, C] and k [J]."""
    x = _cells(F, None, dtype)
    if not state["total"] > 0:
        J = len(state["weights"])
        C = x.shape[1]
        l = np.zeros((J, C), dtype)
        out = (l, np.full(C, math.log(J), dtype), np.full((J, C), 1.0 / J, dtype))
        return out + (np.zeros((J, C), dtype), np.zeros(J, dtype)) if with_abs else out
    k, Linv = constants(state, dtype)
    mu = np.asarray(state["means"], dtype)
    diff = x[None, :, :] - mu[:, :, None]                         # [J, D, C]
    y = np.einsum("jab,jbc->jac", Linv, diff)
    l = k[:, None] - (y * y).sum(axis=1) / 2
    m = l.max(axis=0)
    e = np.exp(l - m[None, :])
    s = e.sum(axis=0)
    out = (l, m + np.log(s), e / s[None, :])
    if with_abs:
        ya = np.einsum("jab,jbc->jac", np.abs(Linv), np.abs(diff))
        out = out + ((ya * ya).sum(axis=1), k)
    return out


def _phi(F, o, dtype):
    """The columns of Phi but lse: 1, u, the upper triangle of u u^T -> [1 + D + tri, C]."""
    x = _cells(F, None, dtype)
    D = x.shape[0]
    u = x - np.asarray(o, dtype)[:, None]
    return np.concatenate([np.ones((1, x.shape[1]), dtype), u, np.stack([u[a] * u[b] for a, b in tri_index(D)])])


def stats(F, w, state, dtype=np.float64, reverse=False):
    """The statistics vector [J (1 + D + tri) + 1]: per cluster N, a, the upper triangle of B; then LL."""
    _, ww = _cells(F, w, dtype)
    l, lse, r = estep(F, state, dtype)
    phi = _phi(F, state["origin"], dtype)
    S = _sum((ww[None, :] * r)[:, None, :] * phi[None, :, :], reverse)      # [J, 1 + D + tri]
    return np.concatenate([S.reshape(-1), [_sum(ww * lse, reverse)]])


def stats_longdouble(F, w, state):
    return stats(F, w, state, dtype=np.longdouble)


def stats_bound(F, w, state, chain_len=None):
    """The a-priori bound of every statistic (include/glowk.h): eps [chain sum w r_j |phi| + sum w |phi| r_j (e_j + sum_i r_i e_i + 4)]
    with e_j = 4 (D + 2)^2 (q~_j + |k_j| + 1); LL: eps [chain sum w |lse| + sum w (|lse| + max_j e_j)].  Dead clusters (pi == 0) have r =
    0 and take no part."""
    D, R, T = F.shape
    ch = chain(R, T) if chain_len is None else chain_len
    _, ww = _cells(F, w)
    l, lse, r, qa, k = estep(F, state, with_abs=True)
    alive = np.isfinite(k)
    e = 4.0 * (D + 2) ** 2 * (qa + np.where(alive, np.abs(k), 0.0)[:, None] + 1.0)
    e = np.where(alive[:, None], e, 0.0)
    mix = (r * e).sum(axis=0)
    phi = np.abs(_phi(F, state["origin"], np.float64))
    wr = ww[None, :] * r
    first = (wr[:, None, :] * phi[None]).sum(axis=-1)
    second = ((wr * (e + mix[None, :] + 4.0))[:, None, :] * phi[None]).sum(axis=-1)
    ll = ch * (ww * np.abs(lse)).sum() + (ww * (np.abs(lse) + e.max(axis=0))).sum()
    return EPS * np.concatenate([(ch * first + second).reshape(-1), [ll]])


def unpack(S, D, J):
    """The statistics vector -> N [J], a [J, D], B [J, D, D] (mirrored), LL."""
    S = np.asarray(S)
    body = S[:-1].reshape(J, -1)
    B = np.zeros((J, D, D), S.dtype)
    for i, (a, b) in enumerate(tri_index(D)):
        B[:, a, b] = B[:, b, a] = body[:, 1 + D + i]
    return body[:, 0], body[:, 1:1 + D], B, S[-1]


def update(S, state, reg_covar=1e-6):
    """The M-step -> (new state with ``status`` bits ORed in, ll)."""
    J, D = np.asarray(state["means"]).shape
    W, o = state["total"], np.asarray(state["origin"], np.float64)
    new = dict(state, weights=np.array(state["weights"], np.float64), means=np.array(state["means"], np.float64),
               covariances=np.array(state["covariances"], np.float64), status=int(state.get("status", 0)))
    if not W > 0:
        new["status"] |= STATUS_ZERO_WEIGHT
        return new, float("nan")
    N, a, B, LL = unpack(np.asarray(S, np.float64), D, J)
    dead = False
    for j in range(J):
        if N[j] < DEAD * W:
            new["weights"][j] = 0.0
            dead = True
            continue
        m = a[j] / N[j]
        new["weights"][j] = N[j] / W
        new["means"][j] = o + m
        new["covariances"][j] = B[j] / N[j] - np.outer(m, m) + reg_covar * np.eye(D)
    try:
        for j in range(J):
            np.linalg.cholesky(new["covariances"][j])
    except np.linalg.LinAlgError:
        old = dict(state, status=int(state.get("status", 0)) | STATUS_CHOLESKY)
        return old, LL / W
    if dead:
        new["status"] |= STATUS_DEAD
    return new, LL / W


def update_tolerance(state_new, D):
    """2^-53 64 D^2 (1 + cond(Sigma_j)) per cluster [J]."""
    return np.array([EPS * 64 * D * D * (1.0 + np.linalg.cond(S)) for S in state_new["covariances"]])


def fit(F, w, J, n_iter=50, tol=1e-6, reg_covar=1e-6, means=None, covariances=None, weights=None, reverse=False):
    """-> the state with ``log_likelihood`` [n_iter] (NaN after the stop), ``iterations`` and ``status``."""
    state = init(F, w, J, reg_covar, reverse=reverse)
    if means is not None:
        state["means"] = np.array(means, np.float64)
        if covariances is not None:
            state["covariances"] = np.array(covariances, np.float64)
        if weights is not None:
            state["weights"] = np.array(weights, np.float64)
    lls = np.full(n_iter, np.nan)
    iters, prev = 0, 0.0
    for k in range(n_iter):
        if not state["total"] > 0:
            break
        S = stats(F, w, state, reverse=reverse)
        state, ll = update(S, state, reg_covar)
        lls[k] = ll
        if state["status"] & STATUS_CHOLESKY:
            break
        iters = k + 1
        if tol > 0 and k >= 1 and ll - prev <= tol * abs(ll):
            break
        prev = ll
    return dict(state, log_likelihood=lls, iterations=iters)


def posteriors(F, state):
    """r [J, R, T] in fp64."""
    D, R, T = F.shape
    return estep(F, state)[2].reshape(-1, R, T)


def labels(F, state):
    r = posteriors(F, state)
    return (np.arange(r.shape[0])[:, None, None] == np.argmax(r, axis=0)[None]).astype(np.float32)


def posterior_bound(F, state):
    """|dr_j| <= eps r_j (e_j + sum_i r_i e_i + 4) per cluster and cell -> [J, R, T]."""
    D, R, T = F.shape
    l, lse, r, qa, k = estep(F, state, with_abs=True)
    alive = np.isfinite(k)
    e = np.where(alive[:, None], 4.0 * (D + 2) ** 2 * (qa + np.where(alive, np.abs(k), 0.0)[:, None] + 1.0), 0.0)
    return (EPS * r * (e + (r * e).sum(axis=0)[None, :] + 4.0)).reshape(-1, R, T)


def label_ties(F, state):
    """The cells whose two largest posteriors are within their bounds of each other -> (count, mask [R, T])."""
    r, b = posteriors(F, state), posterior_bound(F, state)
    if r.shape[0] == 1:
        return 0
    order = np.argsort(-r, axis=0, kind="stable")
    top, second = np.take_along_axis(r, order[:1], 0)[0], np.take_along_axis(r, order[1:2], 0)[0]
    bt, bs = np.take_along_axis(b, order[:1], 0)[0], np.take_along_axis(b, order[1:2], 0)[0]
    return int((top - second <= bt + bs + 2.0 ** -24).sum())


def spatial_features(X, delay=False, max_delay=3.0, p=1.0):
    """X [2, R, T] complex64 -> (F [1 or 2, R, T], w [R, T]) in fp64 (the device rounds them to float32)."""
    X = np.asarray(X, np.complex64)
    R = X.shape[1]
    a, b, c, d = (X[0].real.astype(np.float64), X[0].imag.astype(np.float64), X[1].real.astype(np.float64), X[1].imag.astype(np.float64))
    p1, p2 = a * a + b * b, c * c + d * d
    feats = [np.arctan2(np.sqrt(p2), np.sqrt(p1)) - math.pi / 4]
    rows = np.arange(R, dtype=np.float64)[:, None]
    if delay:
        omega = 2 * math.pi * rows / (2 * (R - 1))
        with np.errstate(divide="ignore", invalid="ignore"):
            dl = -np.arctan2(d * a - c * b, c * a + d * b) / omega
        dl = np.where((rows == 0) | (p1 == 0) | (p2 == 0), 0.0, np.clip(dl, -max_delay, max_delay))
        feats.append(dl)
    e = p1 + p2
    wv = np.sqrt(e) if p == 1.0 else e if p == 2.0 else e ** (p / 2)
    return np.stack(feats), np.where((rows == 0) | (e == 0), 0.0, wv)


# ---- inputs and scenes ------------------------------------------------------------------------------------------------------------------
GPU_SHAPES = [(1, 1, 1, 5, 7), (3, 5, 2, 17, 45), (1, 8, 8, 33, 64), (2, 3, 5, 64, 64), (1, 2, 3, 513, 515)]


def inputs(shape, seed=0):
    """(N, D, J, R, T) -> F float32 [N, D, R, T] drawn around J centres, w float32 [N, R, T]: gamma(0.5) draws, row 0 and a random 10 % of
    the cells exactly 0."""
    N, D, J, R, T = shape
    rng = np.random.default_rng([seed, N, D, J, R, T])
    centres = rng.normal(0.0, 2.0, (N, J, D)) + 3.0
    which = rng.integers(0, J, (N, R, T))
    F = np.take_along_axis(centres[:, :, :, None, None], which[:, None, None, :, :].repeat(D, axis=2), axis=1)[:, 0]
    F = (F + rng.normal(0.0, 0.5, (N, D, R, T))).astype(np.float32)
    w = rng.gamma(0.5, 1.0, (N, R, T))
    w[rng.random((N, R, T)) < 0.1] = 0.0
    w[:, 0, :] = 0.0
    return F, w.astype(np.float32)


def random_state(F, w, J, seed=0):
    """A valid state that is not a fixed point: the start, its means jittered and its weights made unequal."""
    D = F.shape[0]
    rng = np.random.default_rng([seed, D, J])
    st = init(F, w, J)
    st["means"] = st["means"] + rng.normal(0.0, 0.3, (J, D))
    p = rng.random(J) + 0.5
    st["weights"] = p / p.sum()
    A = rng.normal(0.0, 0.2, (J, D, D))
    st["covariances"] = st["covariances"] + A @ A.transpose(0, 2, 1)
    st["status"] = 0
    return st


def sdr(est, ref):
    e = np.asarray(est).astype(np.complex128) - np.asarray(ref).astype(np.complex128)
    return 10.0 * math.log10(float((np.abs(np.asarray(ref).astype(np.complex128)) ** 2).sum()) / max(float((np.abs(e) ** 2).sum()), 1e-300))


def spatial_scene(R, T, pans, density):
    from tests.projet_ref import scene
    return scene(R, T, pans, density)


def spatial_separate(X, J, n_iter=30, p=1.0, reverse=False):
    """The restatement of cluster.spatial with tol = 0 -> (stems [J, 2, R, T] complex128, state)."""
    F, w = spatial_features(X, p=p)
    F, w = F.astype(np.float32), w.astype(np.float32)
    st = fit(F, w, J, n_iter=n_iter, tol=0.0, reverse=reverse)
    r = posteriors(F, st).astype(np.float32)
    return r[:, None] * np.asarray(X)[None], st


def sdr_gains(Y, X, imgs):
    J = imgs.shape[0]
    base = np.asarray(X).astype(np.complex128) / J
    return np.array([sdr(Y[j], imgs[j]) - sdr(base, imgs[j]) for j in range(J)])


def melody_scene():
    """tests/melody_ref.scene() -> (X_lead, X_acc, X_mix) complex STFTs [rows, T] (melody_ref.stft)."""
    from tests import melody_ref
    lead, acc, f0_true, lead_on = melody_ref.scene()
    return melody_ref.stft(lead), melody_ref.stft(acc), melody_ref.stft(lead + acc)


def ensemble_separate(masks, mag, J=2, n_iter=30, power=1.0):
    """The restatement of cluster.ensemble on ready masks -> (r [J, R, T] float32, state)."""
    F = np.stack([np.asarray(m, np.float32) for m in masks])
    w = (np.asarray(mag, np.float64) ** power).astype(np.float32) if power != 1.0 else np.asarray(mag, np.float32)
    st = fit(F, w, J, n_iter=n_iter, tol=0.0)
    return posteriors(F, st).astype(np.float32), st
