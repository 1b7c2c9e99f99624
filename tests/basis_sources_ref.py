"""Test infrastructure: the BASIS update for any number of sources in float64 NumPy (run_basis_sep.py:106-181 with
``g(*sources)`` / ``grad_g(*sources)`` for K = len(sources)), with the noise supplied by the caller.  The dB formulas are the
oracle's (``oracle.basis_ref.g_db`` / ``grad_g_db``), the priors' gradients come from ``oracle.glowref_torch`` (fp64 autograd)."""
import numpy as np

from oracle import basis_ref


def g(sources, process="db"):
    if process == "mean":                                   # run_basis_sep.py:108-111
        return np.mean(np.stack(sources, axis=0), axis=0)
    return basis_ref.g_db(*sources)


def grad_g(sources, process="db"):
    if process == "mean":                                   # :113-116
        return [np.full_like(s, 1.0 / len(sources)) for s in sources]
    return basis_ref.grad_g_db(*sources)


def update(mixed, xs, gs, eps, eta, lam, process="db"):
    """One Langevin step (:163-181): eps[k] are standard-normal arrays."""
    mix = g(xs, process)
    ms = grad_g(xs, process)
    return [x + eta * (gk + lam * m * (mixed - mix)) + np.sqrt(2.0 * eta) * e for x, gk, m, e in zip(xs, gs, ms, eps)]


def inner_loop(mixed, xs, params, cfg, sigma_idx, sigmas, noise, delta=2e-5, T=100, process="db"):
    """run_basis_sep.py:152-181 for len(xs) flow priors; noise[t][k] are standard-normal arrays."""
    from oracle import glowref_torch as RT
    sigma, sigma_l = float(sigmas[sigma_idx]), float(sigmas[-1])
    eta = float(np.float32(delta * (sigma / sigma_l) ** 2))
    lam = 1.0 / sigma ** 2
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    for t in range(T):
        gs = [RT.log_prob_and_grad(x, p, cfg)[1] for x, p in zip(xs, params)]
        xs = update(mixed, xs, gs, noise[t], eta, lam, process)
    return xs
