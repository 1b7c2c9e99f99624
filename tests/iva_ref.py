"""The AuxIVA and ILRMA definitions of include/glowk.h restated in fp64 numpy, one operation at a time, with the costs, the synthetic
scenes and the interference ratio the tests use.  Nothing here imports the package: the restatement is the reference, not a copy of
the code under test.  ILRMA's NMF half is ``tests/nmf_ref.py``.

X [.., M, R, T] complex, W [.., R, M, M] complex128 with row k of W_f = w_{k,f}^H, phi [.., M, T] (AuxIVA) or [.., M, R, T] (ILRMA),
V [.., R, M(k), M, M]; FLOOR = 2^-40."""
import itertools

import numpy as np

from tests import nmf_ref

FLOOR = 2.0 ** -40
U = 2.0 ** -53
MODELS = ("laplace", "gauss")


def c128(a):
    return np.asarray(a, dtype=np.complex128)


def identity(X):
    M, R = X.shape[-3], X.shape[-2]
    return np.broadcast_to(np.eye(M, dtype=np.complex128), X.shape[:-3] + (R, M, M)).copy()


def demix(X, W):
    """y_k(f, t) = sum_m W_f[k, m] X[m, f, t] -> [.., M, R, T] complex128."""
    return np.einsum("...fkm,...mft->...kft", c128(W), c128(X))


def abs2(y):
    """|y|^2 = re^2 + im^2 (not hypot squared, which rounds twice more)."""
    return y.real * y.real + y.imag * y.imag


def _sum(a, axis):
    """A sum that is accurate to the last place of fp64 whatever the number of terms: numpy adds pairwise along the fastest axis only
    and one term after another across the others, which costs several ulp over a thousand rows; extended precision does not."""
    return np.sum(a, axis=axis, dtype=np.longdouble).astype(np.float64)


def norms(X, W):
    """r_k(t) = sum_f |y_k(f, t)|^2 -> [.., M, T]."""
    return _sum(abs2(demix(X, W)), -2)


def weights(X, W, model="laplace"):
    r = norms(X, W)
    R = X.shape[-2]
    return 1.0 / np.maximum(r / R if model == "gauss" else np.sqrt(r), FLOOR)


def factor_weights(basis, act):
    """ILRMA's phi [.., M, R, T] = 1 / max(basis act, FLOOR), fp64 from the float32 factors."""
    rho = np.asarray(basis, np.float32).astype(np.float64) @ np.asarray(act, np.float32).astype(np.float64)
    return 1.0 / np.maximum(rho, FLOOR)


def covariances(X, phi, order=None):
    """V_k(f) = (1/T) sum_t phi_k x x^H -> [.., R, M, M, M].  ``order``: a permutation of the frames to add them in (the restatement
    against itself)."""
    X = c128(X)
    M, R, T = X.shape[-3:]
    phi = np.asarray(phi, np.float64)
    if phi.ndim == X.ndim - 1:
        phi = np.broadcast_to(phi[..., :, None, :], X.shape[:-3] + (M, R, T))
    if order is not None:
        X, phi = X[..., order], phi[..., order]
    xx = np.einsum("...ift,...jft->...fijt", X, X.conj())                       # [.., R, M, M, T]
    return np.einsum("...kft,...fijt->...fkij", phi, xx) / T


def ip_update(W, V, return_cond=False):
    """The iterative projection -> W' (and c_f [.., R]: the largest 2-norm condition number of W_f V_k(f) over k, each taken with
    the rows < k already replaced)."""
    W = c128(W).copy()
    V = c128(V)
    M = W.shape[-1]
    cond = np.zeros(W.shape[:-2])
    for k in range(M):
        Vk = V[..., k, :, :]
        A = W @ Vk
        with np.errstate(all="ignore"):
            cond = np.maximum(cond, np.nan_to_num(np.linalg.cond(A), nan=np.inf))
            e = np.zeros(A.shape[:-1] + (1,), np.complex128)
            e[..., k, 0] = 1.0
            try:
                u = np.linalg.solve(A, e)[..., 0]
            except np.linalg.LinAlgError:
                u = np.full(A.shape[:-1], np.nan, np.complex128)
                for idx in np.ndindex(A.shape[:-2]):
                    try:
                        u[idx] = np.linalg.solve(A[idx], e[idx])[..., 0]
                    except np.linalg.LinAlgError:
                        pass
            d = np.einsum("...i,...ij,...j->...", u.conj(), Vk, u).real
            ok = np.isfinite(u).all(axis=-1) & np.isfinite(d) & (d > 0)
            new = (u / np.sqrt(np.where(ok, d, 1.0))[..., None]).conj()
        W[..., k, :] = np.where(ok[..., None], new, W[..., k, :])
    return (W, cond) if return_cond else W


def auxiva_step(X, W, model="laplace", order=None, return_cond=False):
    """One AuxIVA iteration: weights, covariances, iterative projection."""
    return ip_update(W, covariances(X, weights(X, W, model), order), return_cond)


def auxiva(X, n_iter, model="laplace", W=None):
    """The chain -> the list of iterates W_0 .. W_n."""
    out = [identity(X) if W is None else c128(W)]
    for _ in range(n_iter):
        out.append(auxiva_step(X, out[-1], model))
    return out


def power(X, W):
    """|y_k|^2 in fp64 (the device rounds it once to float32)."""
    return abs2(demix(X, W))


def lambdas(X, W):
    """lambda_k = sqrt(mean_{f,t} |y_k|^2) -> [.., M]."""
    P = power(X, W)
    return np.sqrt(_sum(P, (-2, -1)) / (P.shape[-2] * P.shape[-1]))


def normalize(X, W, basis):
    """Step 5: row k of every W_f / lambda_k, basis_k / lambda_k^2 rounded once to float32, where lambda_k is finite and positive."""
    lam = lambdas(X, W)
    ok = np.isfinite(lam) & (lam > 0)
    lam = np.where(ok, lam, 1.0)
    Wn = c128(W) / np.swapaxes(lam[..., None, :, None], -3, -3)                 # [.., 1, M, 1] over [.., R, M, M]
    bn = (np.asarray(basis, np.float32).astype(np.float64) / (lam ** 2)[..., None, None]).astype(np.float32)
    return Wn, bn


def ilrma_step(X, W, basis, act, return_cond=False):
    """One ILRMA iteration -> (W', basis', act'), the factors float32 (and step 4's c_f)."""
    P = power(X, W).astype(np.float32).astype(np.float64)
    b, a = nmf_ref.iterate(P, np.asarray(basis, np.float32), np.asarray(act, np.float32), 0)
    b, a = b.astype(np.float32), a.astype(np.float32)
    W, cond = ip_update(W, covariances(X, factor_weights(b, a)), True)
    W, b = normalize(X, W, b)
    return (W, b, a, cond) if return_cond else (W, b, a)


def inverse(W):
    """W_f^-1; all zero where it is not finite (or W_f is exactly singular)."""
    W = c128(W)
    out = np.zeros_like(W)
    for idx in np.ndindex(W.shape[:-2]):
        try:
            with np.errstate(all="ignore"):
                inv = np.linalg.inv(W[idx])
        except np.linalg.LinAlgError:
            continue
        if np.isfinite(inv).all():
            out[idx] = inv
    return out


def images(X, W, round_y=False):
    """img[k, m, f, t] = (W_f^-1)[m, k] y_k(f, t) -> [.., M, M, R, T] complex128; ``round_y`` rounds y to complex64 first, as the
    device does."""
    Y = demix(X, W)
    if round_y:
        Y = Y.astype(np.complex64).astype(np.complex128)
    return np.einsum("...fmk,...kft->...kmft", inverse(W), Y)


# ---- costs ---------------------------------------------------------------------------------------------------------------------------------
def _logdet(W):
    return np.log(np.abs(np.linalg.det(c128(W)))).sum(axis=-1)


def cost_iva(X, W):
    """J_IVA = sum_k mean_t sqrt(r_k(t)) - sum_f log |det W_f| (laplace)."""
    return np.sqrt(norms(X, W)).mean(axis=-1).sum(axis=-1) - _logdet(W)


def cost_ilrma(X, W, basis, act):
    """J_ILRMA = (1/T) sum_{k,f,t} (|y_k|^2 / rho_k + log rho_k) - 2 sum_f log |det W_f|."""
    rho = np.maximum(np.asarray(basis, np.float64) @ np.asarray(act, np.float64), FLOOR)
    T = X.shape[-1]
    return (power(X, W) / rho + np.log(rho)).sum(axis=(-3, -2, -1)) / T - 2.0 * _logdet(W)


# ---- the error bound of one step -----------------------------------------------------------------------------------------------------------
def step_bound(T, M, cond):
    """Per row: max |dW_f| / max |W_f| <= 2^-53 (T + 64 M) (1 + c_f)."""
    return U * (T + 64 * M) * (1.0 + cond)


def rows_left_out(T, M, cond):
    """How many rows the 1e-6 rule leaves out of a step."""
    return int((step_bound(T, M, cond) > 1e-6).sum())


def row_error(W_dev, W_ref):
    """max-abs over each row's matrix of the difference, relative to the reference's max-abs -> [.., R]."""
    num = np.abs(c128(W_dev) - c128(W_ref)).max(axis=(-2, -1))
    den = np.abs(c128(W_ref)).max(axis=(-2, -1))
    return num / np.where(den > 0, den, 1.0)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def stft(shape, seed=None):
    """tests/test_gpu_duet.stft for M channels: (N, M, R, T) complex Gaussian with about 5 % exact zeros, a random decade of scale,
    rounded to complex64; never modified."""
    N, M, R, T = shape
    rng = np.random.default_rng(100000 * M + 1000 * R + T if seed is None else seed)
    X = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    X *= rng.random(X.shape) >= 0.05
    X = (X * 10.0 ** rng.uniform(-3, 1)).astype(np.complex64)
    X.setflags(write=False)
    return X


def perturbed_identity(shape, seed=7, eps=0.3):
    """(N, M, R, T) -> W [N, R, M, M]: the identity plus eps times a complex Gaussian."""
    N, M, R, _ = shape
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((N, R, M, M)) + 1j * rng.standard_normal((N, R, M, M))
    return np.eye(M, dtype=np.complex128) + eps * G


def scene(M, R, T, components=2, seed=1):
    """A determined scene: M sources with NMF-structured variances, ``s_k(f, t) = sqrt((B_k A_k)(f, t))`` times a unit complex
    Gaussian, under a random complex mixing matrix per row -> (X [M, R, T] complex64, A_mix [R, M, M], S [M, R, T]).  (Seeds 1, 2, 3
    end within 2 dB of each other after 30 AuxIVA iterations at the tests' shapes; seed 0 at (4, 17, 400) is still descending there,
    at 19.6 dB.)"""
    rng = np.random.default_rng(1000003 * seed + 10007 * M + 101 * R + T)
    B = rng.random((M, R, components)) + 0.05
    A = rng.random((M, components, T)) ** 4 * (rng.random((M, components, T)) < 0.6) + 1e-3
    S = np.sqrt(B @ A) * (rng.standard_normal((M, R, T)) + 1j * rng.standard_normal((M, R, T))) / np.sqrt(2.0)
    mix = rng.standard_normal((R, M, M)) + 1j * rng.standard_normal((R, M, M))
    X = np.einsum("fmk,kft->mft", mix, S).astype(np.complex64)
    X.setflags(write=False)
    return X, mix, S


def interference_db(W, mix):
    """The global interference ratio of the overall system G_f = W_f A_f under the best global permutation: the power on the chosen
    source of every output over the power on the others, summed over the rows, in dB."""
    G = np.abs(c128(W) @ c128(mix)) ** 2                                         # [R, M(out), M(src)]
    P = G.sum(axis=0)
    M = P.shape[0]
    best = max(itertools.permutations(range(M)), key=lambda p: sum(P[k, p[k]] for k in range(M)))
    sig = sum(P[k, best[k]] for k in range(M))
    return 10.0 * np.log10(sig / (P.sum() - sig))


def init_factors(P, K, seed):
    """Random positive factors for the restatement's own ILRMA chains (the device's come from its RNG)."""
    rng = np.random.default_rng(seed)
    M, R, T = P.shape[-3:]
    scale = np.sqrt(P.mean(axis=(-2, -1), keepdims=True) / K)
    return ((rng.random(P.shape[:-2] + (R, K)) * 0.9 + 0.1) * scale).astype(np.float32), \
        ((rng.random(P.shape[:-2] + (K, T)) * 0.9 + 0.1) * scale).astype(np.float32)
