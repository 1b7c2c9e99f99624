"""The device RNG restated in NumPy, from its specification alone (include/glowk.h next to ``glowk_random``; Salmon et al.,
"Parallel random numbers: as easy as 1, 2, 3", SC'11).  Nothing here reads the package.

Philox4x32-10.  One round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to

    (hi32(M1 c2) ^ c1 ^ k0,  lo32(M1 c2),  hi32(M0 c0) ^ c3 ^ k1,  lo32(M0 c0)),    M0 = 0xD2511F53, M1 = 0xCD9E8D57,

and after every round the key grows by the Weyl increments (0x9E3779B9, 0xBB67AE85) modulo 2^32.  Ten rounds.

Counter layout.  Element e of the stream (seed, step, which, pair) starting at element ``offset`` sits in the quad
q = (offset + e) / 4 and takes word (offset + e) % 4 of the Philox output for

    c0 = lo32(q)
    c1 = hi32(q) ^ (which << 28)
    c2 = lo32(step)
    c3 = hi32(step) ^ (pair << 16)
    key = (lo32(seed), hi32(seed))

Uniform.  u = (top 24 bits of the word + 0.5) / 2^24 evaluated in float32: from 2^23 upwards the sum needs 25 bits and rounds to
even, so the largest word gives exactly 1.0; the U(0, 1) draws are clamped to the largest float below one, the u1 / u2 of the
normal draws are not.

Normal.  Words (0, 1) and (2, 3) of a quad are two Box-Muller pairs (u1, u2): theta = fl32(fl32(2 pi) u2) in float32 as the
kernel forms it, then r = sqrt(-2 ln u1), (r cos theta, r sin theta) in float64 -- what is left between this and the device is
the error of its float32 log, sqrt, sine and cosine.
"""
import functools

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SHIFT = np.uint64(32)
BELOW_ONE = np.float32(1.0) - np.float32(2.0 ** -24)          # 0x1.fffffep-1, the largest float below one
TWO_PI_F32 = np.float32(6.2831853071795865)


def philox4x32(counter, key, rounds=10, mult=(M0, M1), bump_first=False):
    """counter: four integer arrays (or ints) below 2^32, key: two ints below 2^32 -> four uint64 arrays of 32-bit words.
    ``rounds``, ``mult`` and ``bump_first`` (the key grows before a round instead of after it) exist for the tests that show the
    known answers tell a broken Philox from this one."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    m0, m1 = np.uint64(mult[0]), np.uint64(mult[1])
    for _ in range(rounds):
        if bump_first:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = m0 * c0, m1 * c2                              # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> SHIFT) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> SHIFT) ^ c3 ^ np.uint64(k1), p0 & MASK
        if not bump_first:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def quad_words(seed, step, which, pair, q):
    """The Philox output [len(q), 4] (uint32) of the quads ``q`` (Python ints or an integer array) of (seed, step, which, pair)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    q = np.atleast_1d(np.asarray(q, dtype=np.uint64))
    c0 = q & MASK
    c1 = (q >> SHIFT) ^ np.uint64((int(which) << 28) & 0xFFFFFFFF)
    c2 = np.uint64(step & 0xFFFFFFFF)
    c3 = np.uint64(((step >> 32) ^ (int(pair) << 16)) & 0xFFFFFFFF)
    out = philox4x32((c0, c1, np.full_like(q, c2), np.full_like(q, c3)), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=1).astype(np.uint32)


def _quads(offset, n):
    offset, n = int(offset), int(n)
    first, last = offset // 4, (offset + n + 3) // 4
    return np.array([first + i for i in range(last - first)], dtype=np.uint64), offset - 4 * first


def words(seed, step=0, which=0, pair=0, offset=0, n=4):
    """The 32-bit word of each of the n elements from element ``offset`` on."""
    q, lead = _quads(offset, n)
    return quad_words(seed, step, which, pair, q).reshape(-1)[lead:lead + int(n)]


def uniform_of_words(w, clamp=True):
    """float32, operation by operation as the kernel: ((float)(w >> 8) + 0.5f) * 2^-24, then min(u, largest float below 1)."""
    u = ((np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    assert u.dtype == np.float32
    return np.minimum(u, BELOW_ONE) if clamp else u


def uniform(seed, step=0, which=0, pair=0, offset=0, n=4, clamp=True):
    """The U(0, 1) draws (float32, bit for bit the device's)."""
    return uniform_of_words(words(seed, step, which, pair, offset, n), clamp)


def normal_of_quads(w4):
    """[nq, 4] words -> [nq, 4] float64 normals: (words 0, 1) -> elements (0, 1), (words 2, 3) -> elements (2, 3)."""
    u = uniform_of_words(w4, clamp=False)
    z = np.empty(u.shape, dtype=np.float64)
    for p in (0, 1):
        u1, u2 = u[:, 2 * p], u[:, 2 * p + 1]
        theta = TWO_PI_F32 * u2
        assert theta.dtype == np.float32
        r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
        z[:, 2 * p] = r * np.cos(theta.astype(np.float64))
        z[:, 2 * p + 1] = r * np.sin(theta.astype(np.float64))
    return z


def normal(seed, step=0, which=0, pair=0, offset=0, n=4):
    """The N(0, 1) draws in float64."""
    q, lead = _quads(offset, n)
    return normal_of_quads(quad_words(seed, step, which, pair, q)).reshape(-1)[lead:lead + int(n)]


@functools.lru_cache(maxsize=None)
def boundary_elements(seed, nquads=1 << 22):
    """Search the first ``nquads`` quads of (seed, step 0, which 0, pair 0) for the words whose top 24 bits are all ones or all
    zero -> (elements with all ones, elements with all zero), each a tuple of element indices."""
    ones, zero = [], []
    chunk = 1 << 20
    for a in range(0, nquads, chunk):
        top = quad_words(seed, 0, 0, 0, np.arange(a, min(a + chunk, nquads), dtype=np.uint64)).reshape(-1) >> np.uint32(8)
        ones += [4 * a + int(i) for i in np.flatnonzero(top == 0xFFFFFF)]
        zero += [4 * a + int(i) for i in np.flatnonzero(top == 0)]
    return tuple(ones), tuple(zero)
