"""NumPy fp64 restatement of the stereo EM Wiener filter (``glowk_mwf_em`` / ``audio.multichannel_wiener``), written from the model's
formulas in 2 x 2 matrix form, its log-likelihood, and a generator of synthetic problems with known PSDs and spatial covariances.

A problem: the mixture STFT x [P, 2, B, T] (complex), S source PSDs v [S, P, B, T] >= 0, spatial covariances R [S, P, B, 2, 2]
(Hermitian), B bins, T frames.  eps = 1e-10, R = I at the start; one iteration, the old v, R on every right-hand side:

    Cx = sum_k v_k R_k + eps I,  W_j = v_j R_j Cx^-1,  y_j = W_j x,  C_j = y_j y_j^H + (I - W_j) v_j R_j,
    v_j' = max(0, Re tr(R_j^-1 C_j) / 2),  R_j' = mean_t C_j / (v_j' + eps) + eps I;   after n_iter: Y_j = v_j R_j Cx^-1 x.
"""
import numpy as np

EPS = 1e-10
I2 = np.eye(2)


def inv2(M):
    """Inverse of [..., 2, 2] matrices: the adjugate over the determinant."""
    det = M[..., 0, 0] * M[..., 1, 1] - M[..., 0, 1] * M[..., 1, 0]
    adj = np.empty_like(M)
    adj[..., 0, 0], adj[..., 1, 1] = M[..., 1, 1], M[..., 0, 0]
    adj[..., 0, 1], adj[..., 1, 0] = -M[..., 0, 1], -M[..., 1, 0]
    return adj / det[..., None, None]


def mixture_covariance(v, R):
    """Cx [P, B, T, 2, 2] = sum_k v_k R_k + eps I."""
    return np.einsum("kpbt,kpbij->pbtij", v, R) + EPS * I2


def _vec(x):
    return np.moveaxis(x, 1, -1)[..., None]                      # [P, B, T, 2, 1]


def filtered(x, v, R):
    """Y [S, P, 2, B, T] = v_j R_j Cx^-1 x."""
    z = inv2(mixture_covariance(v, R)) @ _vec(x)                 # Cx^-1 x
    Y = [(v[j][..., None, None] * R[j][:, :, None]) @ z for j in range(v.shape[0])]
    return np.moveaxis(np.stack(Y)[..., 0], -1, 2)


def em_step(x, v, R):
    """One iteration -> (v', R')."""
    Cxi = inv2(mixture_covariance(v, R))
    xv = _vec(x)
    v_new, R_new = np.empty_like(v), np.empty_like(R)
    for j in range(v.shape[0]):
        G = v[j][..., None, None] * R[j][:, :, None]             # [P, B, T, 2, 2]
        W = G @ Cxi
        y = W @ xv
        C = y @ np.conj(np.swapaxes(y, -1, -2)) + (I2 - W) @ G
        C[..., 0, 0], C[..., 1, 1] = C[..., 0, 0].real, C[..., 1, 1].real
        C[..., 1, 0] = np.conj(C[..., 0, 1])                     # Hermitian: c00, c11 real, c01 complex
        tr = np.trace(inv2(R[j])[:, :, None] @ C, axis1=-2, axis2=-1).real
        v_new[j] = np.maximum(0.0, tr / 2.0)
        R_new[j] = np.mean(C / (v_new[j] + EPS)[..., None, None], axis=2) + EPS * I2
    return v_new, R_new


def start(v):
    S, P, B, _ = v.shape
    return np.broadcast_to(I2.astype(np.complex128), (S, P, B, 2, 2)).copy()


def multichannel_wiener(x, v, n_iter, return_model=False):
    """x [P, 2, B, T], v [S, P, B, T] -> Y [S, P, 2, B, T] (and the fitted v, R)."""
    x, v = np.asarray(x, np.complex128), np.asarray(v, np.float64)
    R = start(v)
    for _ in range(n_iter):
        v, R = em_step(x, v, R)
    Y = filtered(x, v, R)
    return (Y, v, R) if return_model else Y


def single_channel_mask(x, v):
    """The n_iter = 0 output by its own formula: v_j / (sum_k v_k + eps) x per channel."""
    x, v = np.asarray(x, np.complex128), np.asarray(v, np.float64)
    return (v / (v.sum(0) + EPS))[:, :, None] * x[None]


def log_likelihood(x, v, R):
    """L = - sum_{f,t} [log det Cx + x^H Cx^-1 x]."""
    Cx = mixture_covariance(np.asarray(v, np.float64), np.asarray(R, np.complex128))
    det = (Cx[..., 0, 0] * Cx[..., 1, 1] - Cx[..., 0, 1] * Cx[..., 1, 0]).real
    xv = _vec(np.asarray(x, np.complex128))
    quad = (np.conj(np.swapaxes(xv, -1, -2)) @ inv2(Cx) @ xv)[..., 0, 0].real
    return float(-(np.log(det) + quad).sum())


def model_matrix(r):
    """(r00, r11, Re r01, Im r01) [..., 4] -> Hermitian [..., 2, 2]."""
    r = np.asarray(r, np.float64)
    R = np.empty(r.shape[:-1] + (2, 2), np.complex128)
    R[..., 0, 0], R[..., 1, 1] = r[..., 0], r[..., 1]
    R[..., 0, 1] = r[..., 2] + 1j * r[..., 3]
    R[..., 1, 0] = r[..., 2] - 1j * r[..., 3]
    return R


def sdr(sources, Y):
    """Mean over the sources of 10 log10(|s|^2 / |s - Y|^2), over every problem, channel, bin and frame."""
    s, Y = np.asarray(sources, np.complex128), np.asarray(Y, np.complex128)
    ax = tuple(range(1, s.ndim))
    return float(np.mean(10.0 * np.log10((np.abs(s) ** 2).sum(ax) / (np.abs(s - Y) ** 2).sum(ax))))


def problem(S, T, bins, P=1, seed=0, cond=100.0, perturb=1.0):
    """A synthetic problem: source j at (f, t) is sqrt(v_j) chol(R_j(f)) z with z ~ CN(0, I), v_j = exp(2 N(0, 1)) and R_j(f) =
    U diag(2 c, 2) U^H / (1 + c), c = ``cond``, U a random unitary (trace 2, condition number ``cond``); the mixture is their sum;
    the PSDs handed to the filter are v_j exp(perturb N(0, 1)).  Everything is rounded to fp32 (complex64) values, held in fp64, so
    a float32 implementation sees exactly these inputs.  Returns a dict: x [P, 2, B, T], v [S, P, B, T] (perturbed), sources
    [S, P, 2, B, T], v_true, R_true [S, P, B, 2, 2]."""
    rng = np.random.default_rng(seed)
    v_true = np.exp(2.0 * rng.standard_normal((S, P, bins, T)))
    A = rng.standard_normal((S, P, bins, 2, 2)) + 1j * rng.standard_normal((S, P, bins, 2, 2))
    U = np.linalg.qr(A)[0]
    d = np.array([2.0 * cond, 2.0]) / (1.0 + cond)
    R_true = (U * d) @ np.conj(np.swapaxes(U, -1, -2))
    L = U * np.sqrt(d)                                           # L L^H = R: any square root serves as the Cholesky factor does
    z = (rng.standard_normal((S, P, bins, T, 2, 1)) + 1j * rng.standard_normal((S, P, bins, T, 2, 1))) / np.sqrt(2.0)
    s = np.sqrt(v_true)[..., None, None] * (L[:, :, :, None] @ z)
    sources = np.moveaxis(s[..., 0], -1, 2).astype(np.complex64).astype(np.complex128)
    x = sources.sum(0).astype(np.complex64).astype(np.complex128)
    v = (v_true * np.exp(perturb * rng.standard_normal(v_true.shape))).astype(np.float32).astype(np.float64)
    return dict(x=x, v=v, sources=sources, v_true=v_true, R_true=R_true)
