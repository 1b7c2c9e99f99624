"""PROJET in plain fp64 numpy: the definitions of include/glowk.h (the PROJET section) restated without the package, for the CPU and
GPU tests.  Every sum over j, m and l is an explicit ascending loop of one product and one add, as the kernels do it; only the sums
over the cells (the outer sums and the divergence) use numpy's own order, or long double where a test asks for it.  Shapes: X [2, R, T]
complex, V [M, R, T], P [J, R, T], Q [L, J], G [M, J]."""
import math

import numpy as np

FLOOR = 2.0 ** -40


def tables(M=15, L=41, alpha=1.0):
    phi = np.arange(M, dtype=np.float64) * math.pi / (2 * (M - 1))
    theta = np.full(1, math.pi / 4) if L == 1 else np.arange(L, dtype=np.float64) * math.pi / (2 * (L - 1))
    U = np.stack([-np.sin(phi), np.cos(phi)], axis=1)
    K = np.abs(np.sin(theta[None, :] - phi[:, None])) ** alpha
    Up = np.linalg.solve(U.T @ U, U.T)
    return dict(U=U, K=K, Up=Up, phi=phi, theta=theta, alpha=float(alpha))


def proj(X, U):
    """c [M, R, T] complex128 as (re, im): two products and one add per component."""
    x = np.asarray(X).astype(np.complex128)
    re = U[:, 0, None, None] * x[0].real[None] + U[:, 1, None, None] * x[1].real[None]
    im = U[:, 0, None, None] * x[0].imag[None] + U[:, 1, None, None] * x[1].imag[None]
    return re, im


def power(p, alpha):
    return np.sqrt(p) if alpha == 1.0 else p if alpha == 2.0 else np.power(p, alpha / 2)


def projections(X, tab):
    re, im = proj(X, tab["U"])
    return power(re * re + im * im, tab["alpha"])


def gains(Q, K):
    G = K[:, 0, None] * Q[0][None, :]
    for l in range(1, K.shape[1]):
        G = G + K[:, l, None] * Q[l][None, :]
    return G


def sigma_raw(P, G):
    """[M, R, T]: sum_j P_j G[m][j], j ascending, before the floor."""
    s = P[0][None] * G[:, 0, None, None]
    for j in range(1, P.shape[0]):
        s = s + P[j][None] * G[:, j, None, None]
    return s


def weights(V, s, beta):
    if beta == 2:
        return V, s
    if beta == 1:
        return V / s, np.ones_like(s)
    return V / (s * s), 1.0 / s


def g_of(r, beta):
    return np.sqrt(r) if beta == 0 else r


def init(X, J, tab):
    x = np.asarray(X).astype(np.complex128)
    e = (x[0].real * x[0].real + x[0].imag * x[0].imag) + (x[1].real * x[1].real + x[1].imag * x[1].imag)
    P = np.repeat((power(e, tab["alpha"]) / J)[None], J, axis=0)
    w = math.pi / (2 * J)
    t = (np.arange(J, dtype=np.float64) + 0.5) * math.pi / (2 * J)
    Q = np.maximum(1.0 - np.abs(tab["theta"][:, None] - t[None, :]) / w, 0.0) + 0.05
    return P, Q / Q.sum(axis=0, keepdims=True)


def update_p(V, P, G, beta):
    s = np.maximum(sigma_raw(P, G), FLOOR)
    wn, wd = weights(V, s, beta)
    M, J = G.shape
    num, den = np.zeros_like(P), np.zeros_like(P)
    for m in range(M):
        for j in range(J):
            num[j] = num[j] + G[m, j] * wn[m]
            den[j] = den[j] + G[m, j] * wd[m]
    return P * g_of(num / np.maximum(den, FLOOR), beta)


def outer_sums(V, P, G, beta, wide=False):
    """An, Ad [M, J] from P as given (sigma from it and G).  wide: the products and the sums over the cells in numpy's long double
    (64 significant bits on x86), so that a one-step comparison sees the device's rounding and not the order of numpy's own sum."""
    s = np.maximum(sigma_raw(P, G), FLOOR)
    wn, wd = weights(V, s, beta)
    if not wide:
        return np.einsum("jrt,mrt->mj", P, wn), np.einsum("jrt,mrt->mj", P, wd)
    Pw, An, Ad = P.astype(np.longdouble), np.zeros(G.shape), np.zeros(G.shape)
    for m in range(G.shape[0]):
        for j in range(G.shape[1]):
            An[m, j] = float((Pw[j] * wn[m].astype(np.longdouble)).sum())
            Ad[m, j] = float((Pw[j] * wd[m].astype(np.longdouble)).sum())
    return An, Ad


def update_q(V, P, Q, K, beta, G=None, wide=False):
    G = gains(Q, K) if G is None else G
    An, Ad = outer_sums(V, P, G, beta, wide)
    M = K.shape[0]
    num, den = K[0][:, None] * An[0][None, :], K[0][:, None] * Ad[0][None, :]
    for m in range(1, M):
        num = num + K[m][:, None] * An[m][None, :]
        den = den + K[m][:, None] * Ad[m][None, :]
    return Q * g_of(num / np.maximum(den, FLOOR), beta)


def divergence_terms(V, P, G, beta):
    """(d, a) [M, R, T]: the terms of D and the sum of the magnitudes of each term's parts (the scale of its rounding error)."""
    s = np.maximum(sigma_raw(P, G), FLOOR)
    if beta == 2:
        return (V - s) ** 2 / 2.0, (V + s) ** 2 / 2.0
    if beta == 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            lg = np.where(V > 0, V * np.log(np.where(V > 0, V, 1.0) / s), 0.0)
        return lg - V + s, np.abs(lg) + V + s
    q = np.maximum(V, FLOOR) / s
    return q - np.log(q) - 1.0, q + np.abs(np.log(q)) + 1.0


def divergence(V, P, G, beta, wide=False):
    d = divergence_terms(V, P, G, beta)[0]
    return float(d.astype(np.longdouble).sum()) if wide else float(d.sum())


def separate(X, P, G, tab, dtype=np.complex64):
    """Y [J, 2, R, T]; dtype=None keeps complex128 (before the one rounding)."""
    re, im = proj(X, tab["U"])
    raw = sigma_raw(P, G)
    s = np.maximum(raw, FLOOR)
    M, J = G.shape
    Up = tab["Up"]
    yr, yi = np.zeros((J, 2) + re.shape[1:]), np.zeros((J, 2) + re.shape[1:])
    for m in range(M):
        for j in range(J):
            w = np.where(raw[m] >= FLOOR, P[j] * G[m, j] / s[m], 1.0 / J)
            for ch in range(2):
                t = Up[ch, m] * w
                yr[j, ch] = yr[j, ch] + t * re[m]
                yi[j, ch] = yi[j, ch] + t * im[m]
    Y = yr + 1j * yi
    return Y if dtype is None else Y.astype(dtype)


def separate_scale(X, tab):
    """sum_m |Up[ch][m]| |c_m| [2, R, T]: the scale of the separation's rounding error."""
    re, im = proj(X, tab["U"])
    return np.einsum("cm,mrt->crt", np.abs(tab["Up"]), np.sqrt(re * re + im * im))


def step(V, P, Q, K, beta):
    """One iteration -> (P', Q')."""
    G = gains(Q, K)
    P = update_p(V, P, G, beta)
    return P, update_q(V, P, Q, K, beta, G)


def fit(X, J, tab, beta, n_iter, trace=None):
    """init and n_iter iterations -> (P, Q).  trace: a list that receives D after every half step (P, then Q), D of the start first."""
    V = projections(X, tab)
    P, Q = init(X, J, tab)
    K = tab["K"]
    if trace is not None:
        trace.append(divergence(V, P, gains(Q, K), beta))
    for _ in range(n_iter):
        G = gains(Q, K)
        P = update_p(V, P, G, beta)
        if trace is not None:
            trace.append(divergence(V, P, G, beta))
        Q = update_q(V, P, Q, K, beta, G)
        if trace is not None:
            trace.append(divergence(V, P, gains(Q, K), beta))
    return P, Q


def projet(X, J, tab, beta=1, n_iter=100):
    P, Q = fit(X, J, tab, beta, n_iter)
    return separate(X, P, gains(Q, tab["K"]), tab), P, Q


def pan_estimates(Q, theta):
    return theta[np.argmax(Q, axis=0)]


def scene(R, T, pans, density, seed=1):
    """-> (X [2, R, T] complex64, images [J, 2, R, T] complex64): per source gamma(0.4, 1) magnitudes on a Bernoulli(density) support
    with uniform phases, panned by (cos theta, sin theta), each image rounded to complex64; the mixture is the sum of the rounded images."""
    rng = np.random.default_rng(seed)
    imgs = []
    for th in pans:
        mag = rng.gamma(0.4, 1.0, (R, T)) * (rng.random((R, T)) < density)
        s = mag * np.exp(2j * np.pi * rng.random((R, T)))
        imgs.append(np.stack([math.cos(th) * s, math.sin(th) * s]).astype(np.complex64))
    imgs = np.stack(imgs)
    return imgs.sum(axis=0).astype(np.complex64), imgs


def sdr(est, ref):
    """10 log10(|ref|^2 / |ref - est|^2) over everything."""
    e = np.asarray(est).astype(np.complex128) - np.asarray(ref).astype(np.complex128)
    return 10.0 * math.log10(float((np.abs(ref.astype(np.complex128)) ** 2).sum()) / max(float((np.abs(e) ** 2).sum()), 1e-300))


def sdr_gains(Y, X, imgs):
    """Per source: SDR of the stem over the SDR of X / J."""
    J = imgs.shape[0]
    base = np.asarray(X).astype(np.complex128) / J
    return np.array([sdr(Y[j], imgs[j]) - sdr(base, imgs[j]) for j in range(J)])
