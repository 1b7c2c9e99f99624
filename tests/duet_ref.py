"""DUET restated in fp64 numpy (include/glowk.h has the formulas; audiosourcesep_amd/duet.py the GPU path).  The definition the tests
hold the kernels to: features, the half-open binning, the exact integer histogram, binomial smoothing in int64, the greedy peaks and
the assignment, plus the crafted mixtures both test files share."""
import numpy as np

DEFAULT_GRID = (-3.0, 3.0, 50, -3.0, 3.0, 50)         # a_lo, a_hi, n_a, d_lo, d_hi, n_d
MAX_SHIFT = 40


def omega(rows):
    """omega_r = 2 pi r / n_fft, n_fft = 2 (rows - 1); 0 for row 0 (also when rows == 1)."""
    w = np.zeros(rows)
    if rows > 1:
        w[1:] = 2 * np.pi * np.arange(1, rows, dtype=np.float64) / float(2 * (rows - 1))
    return w


def features(X, p=1.0, q=0.0):
    """X [.., 2, R, T] complex -> alpha, delta, w, each [.., R, T] fp64."""
    X = np.asarray(X).astype(np.complex128)
    X1, X2 = X[..., 0, :, :], X[..., 1, :, :]
    om = omega(X.shape[-2])[:, None]
    m1, m2 = np.abs(X1), np.abs(X2)
    live = (m1 != 0) & (m2 != 0) & (om != 0)
    with np.errstate(all="ignore"):
        alpha = np.where(live, (m2 ** 2 - m1 ** 2) / (m1 * m2), 0.0)
        delta = np.where(live, -np.angle(X2 * np.conj(X1)) / om, 0.0)
        w = np.where(live, np.power(m1 * m2, p) * np.power(om, q), 0.0)
    return alpha, delta, w


def bin_of(v, lo, hi, n):
    """floor((v - lo) n / (hi - lo)) where it lies in [0, n), else -1."""
    with np.errstate(all="ignore"):
        f = np.floor((np.asarray(v, np.float64) - lo) * float(n) / (hi - lo))
    ok = (f >= 0) & (f < n)
    return np.where(ok, f, -1).astype(np.int64)


def counted_cells(alpha, delta, w, grid):
    """(flat indices of the counted points, their histogram cells)."""
    a_lo, a_hi, n_a, d_lo, d_hi, n_d = grid
    a, d, w = (np.asarray(t, np.float64).ravel() for t in (alpha, delta, w))
    i, j = bin_of(a, a_lo, a_hi, n_a), bin_of(d, d_lo, d_hi, n_d)
    ok = (i >= 0) & (j >= 0) & np.isfinite(w) & (w > 0)
    at = np.nonzero(ok)[0]
    return at, i[at] * n_d + j[at]


def histogram_float(alpha, delta, w, grid):
    """The weighted histogram of one signal in fp64 (its sums depend on the order; the integer form below does not)."""
    at, cell = counted_cells(alpha, delta, w, grid)
    return np.bincount(cell, weights=np.asarray(w, np.float64).ravel()[at], minlength=grid[2] * grid[5]).reshape(grid[2], grid[5])


def ceil_log2(n):
    return (int(n) - 1).bit_length()


def hist_shift(cells, smooth):
    return min(MAX_SHIFT, 62 - ceil_log2(max(cells, 2)) - 4 * smooth)


def histogram_int(alpha, delta, w, grid, smooth=1):
    """One signal -> (int64 plane [n_a, n_d], e, s): the sum of rint(w 2^(s - e)) per cell, wmax < 2^e, e = 0 without a counted weight."""
    wf = np.asarray(w, np.float64).ravel()
    s = hist_shift(wf.size, smooth)
    at, cell = counted_cells(alpha, delta, w, grid)
    plane = np.zeros(grid[2] * grid[5], np.int64)
    if at.size == 0:
        return plane.reshape(grid[2], grid[5]), 0, s
    e = int(np.frexp(wf[at].max())[1])
    np.add.at(plane, cell, np.rint(np.ldexp(wf[at], s - e)).astype(np.int64))
    return plane.reshape(grid[2], grid[5]), e, s


def smooth_plane(plane, passes):
    """`passes` of [1 2 1] x [1 2 1] in int64, zero beyond the edges."""
    a = np.asarray(plane, np.int64).copy()
    for _ in range(passes):
        b = np.pad(a, ((0, 0), (1, 1)))
        a = b[:, :-2] + 2 * b[:, 1:-1] + b[:, 2:]
        b = np.pad(a, ((1, 1), (0, 0)))
        a = b[:-2] + 2 * b[1:-1] + b[2:]
    return a


def find_peaks(plane, num_sources, smooth=1, min_distance=(5, 5), return_margins=False):
    """-> (peaks [S, 2] int32 with -1 where none, n_found, the smoothed plane[, the relative margin of every pick over the runner-up])."""
    sm = smooth_plane(plane, smooth)
    n_a, n_d = sm.shape
    free = np.ones(sm.shape, bool)
    peaks = np.full((num_sources, 2), -1, np.int32)
    margins = []
    found = 0
    ii, jj = np.meshgrid(np.arange(n_a), np.arange(n_d), indexing="ij")
    while found < num_sources:
        vals = np.where(free, sm, -1).ravel()
        at = int(np.argmax(vals))                        # the first of equal maxima: the lowest row-major index
        if vals[at] <= 0:
            break
        rest = np.delete(vals, at)
        second = max(int(rest.max()), 0) if rest.size else 0
        margins.append((int(vals[at]) - second) / float(vals[at]))
        i, j = divmod(at, n_d)
        peaks[found] = (i, j)
        found += 1
        free &= ~((np.abs(ii - i) <= min_distance[0]) & (np.abs(jj - j) <= min_distance[1]))
    return (peaks, found, sm, margins) if return_margins else (peaks, found, sm)


def centres(peaks, grid):
    """alpha_j, delta_j, a_j of peaks [n, 2]."""
    a_lo, a_hi, n_a, d_lo, d_hi, n_d = grid
    p = np.asarray(peaks, np.float64)
    al = a_lo + (p[:, 0] + 0.5) * (a_hi - a_lo) / float(n_a)
    de = d_lo + (p[:, 1] + 0.5) * (d_hi - d_lo) / float(n_d)
    return al, de, (al + np.sqrt(al * al + 4.0)) / 2.0


def costs(X, peaks, n_found, grid):
    """J [n_found, R, T] of X [2, R, T]."""
    X = np.asarray(X).astype(np.complex128)
    al, de, a = centres(np.asarray(peaks)[:n_found], grid)
    om = omega(X.shape[-2])[None, :, None]
    rot = a[:, None, None] * np.exp(-1j * de[:, None, None] * om)
    return np.abs(rot * X[0][None] - X[1][None]) ** 2 / (1.0 + a * a)[:, None, None]


def assign(X, peaks, n_found, grid, return_undecidable=False):
    """-> masks [S, R, T] float32 (S = len(peaks)); with return_undecidable also the cells whose two smallest J are within
    1e-9 (|X1|^2 + |X2|^2) of each other.  A cell where both channels are exactly 0 is not among them: every J there is an exact 0
    in any arithmetic, and the lowest index decides."""
    X = np.asarray(X)
    S = len(peaks)
    masks = np.zeros((S,) + X.shape[-2:], np.float32)
    und = np.zeros(X.shape[-2:], bool)
    if n_found:
        J = costs(X, peaks, n_found, grid)
        best = np.argmin(J, axis=0)                      # the first of equal minima
        for j in range(n_found):
            masks[j] = best == j
        if n_found > 1:
            two = np.sort(J, axis=0)[:2]
            Xc = X.astype(np.complex128)
            energy = np.abs(Xc[0]) ** 2 + np.abs(Xc[1]) ** 2
            und = (two[1] - two[0] <= 1e-9 * energy) & (energy > 0)
    return (masks, und) if return_undecidable else masks


# ---- the crafted mixtures of tests/test_duet_cpu.py and tests/test_gpu_duet.py ---------------------------------------------------------
CRAFT_GRID = (-3.0, 3.0, 35, -1.5, 1.5, 51)
CRAFT_A = (8, 17, 26, 13)
CRAFT_D = (13, 25, 37, 31)
CRAFT_SHAPES = [(33, 64), (65, 130), (129, 257), (1025, 96)]
CRAFT_CASES = [(S, shape) for S in (3, 4) for shape in CRAFT_SHAPES]
CRAFT_MIN_DISTANCE = (5, 5)                               # the default: no crafted cell lies in another's exclusion box


def crafted(S, shape, seed=7):
    """-> (X [2, R, T] complex64, images [S, 2, R, T] complex128 of the sources in the two channels).  Source j sits at the centre of
    attenuation cell CRAFT_A[j] and delay cell CRAFT_D[j]; each is complex Gaussian, active in a cell with probability 0.35."""
    R, T = shape
    rng = np.random.default_rng(seed)
    al, de, a = centres(np.stack([CRAFT_A[:S], CRAFT_D[:S]], 1), CRAFT_GRID)
    om = omega(R)[:, None]
    images = np.zeros((S, 2, R, T), np.complex128)
    for j in range(S):
        s = (rng.standard_normal((R, T)) + 1j * rng.standard_normal((R, T))) * (rng.random((R, T)) < 0.35)
        images[j, 0] = s
        images[j, 1] = a[j] * np.exp(-1j * de[j] * om) * s
    X = images.sum(0).astype(np.complex64)
    return X, images


def energy_shares(masks, images):
    """The share of each source's energy (both channels) that its mask keeps."""
    e = (np.abs(images) ** 2).sum(1)                     # [S, R, T]
    return np.array([(masks[j] * e[j]).sum() / e[j].sum() for j in range(len(images))])
