"""fp64 NumPy / SciPy restatement of the sample-rate converter (a helper of the resampler tests, not a test module).

Written from the definition in include/glowk.h, not from the kernel: librosa 0.7's default filter design (resampy's kaiser_best: a
Kaiser-windowed sinc, Z = 64 zero crossings, P = 512 table points per zero crossing, beta and roll-off below), evaluated at the
exact position of every tap.  With a, b = sr_in, sr_out over their gcd, s = min(1, b / a) and t a = q b + r in integers:

    T[k] = rho sinc(rho k / P) I0(beta sqrt(1 - (k / (Z P))^2)) / I0(beta),  k = 0 .. Z P
    h(u) = 0 for p = |u| P > Z P, else T[k] + (p - k) (T[k + 1] - T[k]) with k = min(floor(p), Z P - 1)
    y[t] = s sum_m x[m] h(s ((q - m) + r / b)),  x zero outside [0, n_in),  n_out = ceil(n_in b / a)

All outputs with the same phase r share their weights, so ``resample`` works phase by phase, and on any subset of the outputs.
``emulate_fp32`` is a different thing: the kernel's own arithmetic (integer table positions, fp32 FMA chains outwards from the
centre), restated to measure how far fp32 in that order lands from the fp64 definition; the GPU tests take their bound from it.
"""
import math

import numpy as np
from scipy.special import i0

Z, P = 64, 512
ZP = Z * P
BETA, ROLLOFF = 14.769656459379492, 0.9475937167399596


def table():
    """T [32769] float64."""
    k = np.arange(ZP + 1, dtype=np.float64)
    return ROLLOFF * np.sinc(ROLLOFF * k / P) * i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (k / ZP) ** 2))) / i0(BETA)


def ratio(sr_in, sr_out):
    g = math.gcd(int(sr_in), int(sr_out))
    return int(sr_in) // g, int(sr_out) // g


def length(n_in, sr_in, sr_out):
    a, b = ratio(sr_in, sr_out)
    return -((-int(n_in) * b) // a)


def h(u, T):
    p = np.abs(u) * P
    k = np.minimum(np.floor(p), ZP - 1).astype(np.int64)
    return np.where(p > ZP, 0.0, T[k] + (p - k) * (T[k + 1] - T[k]))


def _positions(n_in, sr_in, sr_out, idx):
    a, b = ratio(sr_in, sr_out)
    t = np.arange(length(n_in, sr_in, sr_out), dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64)
    ta = t * a
    q = ta // b
    return a, b, q, ta - q * b


def resample(x, sr_in, sr_out, idx=None, T=None, chunk=1 << 22):
    """x [n_in] (any float type; the arithmetic is float64) -> y [n_out] float64, or only y[idx]."""
    x = np.asarray(x)
    T = table() if T is None else T
    a, b, q, r = _positions(len(x), sr_in, sr_out, idx)
    s = min(1.0, b / a)
    J = int(math.ceil(Z / s)) + 1                       # h vanishes beyond |q - m + r / b| = Z / s
    j = np.arange(-J, J + 1, dtype=np.int64)
    xp = np.concatenate([np.zeros(J, x.dtype), x, np.zeros(J, x.dtype)])       # xp[m + J] = x[m]
    y = np.zeros(len(q), dtype=np.float64)
    order = np.argsort(r, kind="stable")
    bounds = np.flatnonzero(np.diff(r[order])) + 1
    rows = max(1, chunk // len(j))
    for grp in np.split(order, bounds):
        if not len(grp):
            continue
        w = s * h(s * (j + float(r[grp[0]]) / b), T)    # the weights of this phase, tap m = q - j
        for i0_ in range(0, len(grp), rows):
            g = grp[i0_:i0_ + rows]
            y[g] = xp[(q[g] + J)[:, None] - j[None, :]].astype(np.float64) @ w
    return y


def _fma32(a, b, c):
    """fl32(a * b + c): the product of two float32 is exact in float64; the sum rounds to float64 first, which moves the float32
    result off the fused one in a negligible share of cases (double rounding)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_fp32(x, sr_in, sr_out, idx=None, T=None):
    """The kernel's arithmetic on the CPU: table pairs (T[k], T[k + 1] - T[k]) rounded to float32, the table position of tap i as
    the integer quotient and remainder of |j b + r| P / d (d = max(a, b)), the fraction as fl32(rem) * fl32(1 / d), one FMA
    chain over the taps m = q, q - 1, ..., one over m = q + 1, q + 2, ..., y = fl32(s) * (right + left).  -> float32."""
    x = np.asarray(x, dtype=np.float32)
    T = table() if T is None else T
    tab, dtab = T.astype(np.float32), np.append(np.diff(T), 0.0).astype(np.float32)
    a, b, q, r = _positions(len(x), sr_in, sr_out, idx)
    d = max(a, b)
    H = (Z * d) // b + 1
    stepk, stepr = divmod(b * P, d)
    inv_d = np.float32(1.0) / np.float32(d)
    xp = np.concatenate([np.zeros(H + 1, np.float32), x, np.zeros(H + 1, np.float32)])   # xp[m + H + 1] = x[m]
    acc = []
    for side in (0, 1):
        n0 = r if side == 0 else b - r
        k, rem = (n0 * P) // d, (n0 * P) % d
        s = np.zeros(len(q), np.float32)
        for i in range(H):
            on = (k < ZP) | ((k == ZP) & (rem == 0))
            if not on.any():
                break
            kk = np.minimum(k, ZP)
            w = _fma32(rem.astype(np.float32) * inv_d, dtab[kk], tab[kk])
            xv = xp[(q - i if side == 0 else q + 1 + i) + H + 1]
            s = np.where(on, _fma32(xv, w, s), s)
            k, rem = k + stepk, rem + stepr
            carry = rem >= d
            k, rem = k + carry, rem - d * carry
        acc.append(s)
    return np.float32(min(1.0, b / a)) * (acc[0] + acc[1])
