"""Melody separation by pitch: a harmonic salience function (Salamon & Gomez 2012, the surface of ``librosa.salience``), the predominant
f0 as a Viterbi path through it, and a harmonic comb mask around that path (Hsu & Jang 2010; nussl's ``Melodia`` separator).  The
prior-free baseline for one sustained, monophonic, harmonic voice over an accompaniment -- the violin over the piano of the BASIS
mixtures -- and the package's f0 tracker.  Not in the reference.

Kernels in ``csrc/glowk_melody.h`` (formulas in include/glowk.h, host-side rules in ``csrc/glowk_melody_index.h``):

* ``f0_grid``: the candidate fundamentals, ``fmin * 2 ** (b / bins_per_octave)``;
* ``salience``: ``sal[b, t] = sum_h w_h S(h f0_b, t)``, S interpolated linearly between the two rows around ``h f0_b``; the positions are
  computed on the host in IEEE fp64, the sum on the GPU in fp64, a thread per (bin, frame);
* ``emission``: the salience over its signal's maximum, float64;
* ``track``: the Viterbi path over the bins and one "unvoiced" state, with fp64 adds, subtractions and compares alone, so that it equals
  a plain numpy loop in every frame; one workgroup per signal;
* ``harmonic_mask``: the triangular comb of ``width`` Hz around the harmonics of the tracked f0;
* ``melody``: all of it in one library call (``glowk_melody_fit``), then the soft masks of ``hpss`` from ``m |S|`` and ``(1 - m) |S|``;
* ``melody_audio``, ``separate_wav_melody``: the audio and wav surfaces of ``hpss.hpss_audio`` and ``hpss.separate_wav_hpss``.

Conventions as in ``hpss.py``: numpy or torch in, tensors on the GPU the input lives on (the current one for host input) out, ValueError
for bad arguments before the library is loaded.  Results are bitwise reproducible and a batch gives what its signals give alone.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, audio
from .audio import _p, _s

MAX_SIGNALS, MIN_ROWS, MAX_ROWS, MAX_FRAMES = 65535, 2, 4096, 32768
MAX_BINS, MAX_HARMONICS, MAX_JUMP, MAX_MASK_HARMONICS = 1024, 32, 1023, 1024
MAX_ELEMENTS = (1 << 31) - 1
BIN_HZ = audio.SR / 2048                                  # the row spacing of audio.mel_frames' STFT
TRACK_KEYS = ("threshold", "jump_penalty", "voicing_penalty", "max_jump")
MELODY_KEYS = ("f0s", "harmonics", "decay", "weights", "bin_hz") + TRACK_KEYS + ("n_harmonics", "width", "power")


def _int(v, what, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError("%s: expected an integer in [%d, %d], got %r" % (what, lo, hi, v))
    return int(v)


def _number(v, what, positive=False):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or (positive and not v > 0):
        raise ValueError("%s: expected a finite%s number, got %r" % (what, " positive" if positive else "", v))
    return float(v)


def _flag(v, what):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("%s: expected True or False, got %r" % (what, v))
    return bool(v)


def f0_grid(fmin=55.0, n_octaves=5, bins_per_octave=60):
    """The candidate fundamentals: float64 [n_octaves * bins_per_octave], ``fmin * 2.0 ** (b / bins_per_octave)``."""
    fmin = _number(fmin, "fmin", positive=True)
    n_octaves = _int(n_octaves, "n_octaves", 1, MAX_BINS)
    bins_per_octave = _int(bins_per_octave, "bins_per_octave", 1, MAX_BINS)
    if n_octaves * bins_per_octave > MAX_BINS:
        raise ValueError("n_octaves * bins_per_octave: expected at most %d bins, got %d" % (MAX_BINS, n_octaves * bins_per_octave))
    return fmin * 2.0 ** (np.arange(n_octaves * bins_per_octave, dtype=np.float64) / bins_per_octave)


def _grid(f0s):
    """The grid as float64 [B]: 1 <= B <= 1024, finite, positive, strictly ascending."""
    if f0s is None:
        return f0_grid()
    g = np.asarray(f0s.detach().cpu() if torch.is_tensor(f0s) else f0s)
    if g.ndim != 1 or not 1 <= g.shape[0] <= MAX_BINS or g.dtype.kind not in "fiu":
        raise ValueError("f0s: expected a real vector of 1 to %d frequencies, got %s %s" % (MAX_BINS, g.dtype, g.shape))
    g = np.ascontiguousarray(g, dtype=np.float64)
    if not np.isfinite(g).all() or not (g > 0).all() or not (np.diff(g) > 0).all():
        raise ValueError("f0s: expected finite, positive, strictly ascending frequencies")
    return g


def _weights(harmonics, decay, weights):
    """The harmonic weights as float64 [H], 1 <= H <= 32: ``weights``, or ``decay ** (h - 1)`` for h = 1 .. harmonics."""
    if weights is None:
        H = _int(harmonics, "harmonics", 1, MAX_HARMONICS)
        return np.float64(_number(decay, "decay", positive=True)) ** np.arange(H, dtype=np.float64)
    w = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights)
    if w.ndim != 1 or not 1 <= w.shape[0] <= MAX_HARMONICS or w.dtype.kind not in "fiu":
        raise ValueError("weights: expected a real vector of 1 to %d harmonic weights, got %s %s" % (MAX_HARMONICS, w.dtype, w.shape))
    w = np.ascontiguousarray(w, dtype=np.float64)
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weights: expected finite, non-negative weights")
    return w


def _track_params(threshold, jump_penalty, voicing_penalty, max_jump):
    """(theta, pen [J + 1] float64, nu, J), checked; ``pen[d] = jump_penalty * d`` in fp64."""
    J = _int(max_jump, "max_jump", 0, MAX_JUMP)
    jp = _number(jump_penalty, "jump_penalty")
    if jp < 0:
        raise ValueError("jump_penalty: expected a number >= 0, got %r" % (jump_penalty,))
    return _number(threshold, "threshold"), np.float64(jp) * np.arange(J + 1, dtype=np.float64), _number(voicing_penalty, "voicing_penalty"), J


def _mask_params(n_harmonics, width, bin_hz):
    return _int(n_harmonics, "n_harmonics", 1, MAX_MASK_HARMONICS), _number(width, "width", positive=True), _number(bin_hz, "bin_hz", positive=True)


def _power(power):
    if isinstance(power, (bool, np.bool_)) or not isinstance(power, (int, float, np.integer, np.floating)) or not power > 0:
        raise ValueError("power: expected a number > 0 (inf: the hard mask), got %r" % (power,))
    return float(power)


def _planes(a, what, second, lo, hi, B=None, vector=False):
    """[.., second, T] (or [.., T] with ``vector``) within the library's ranges, as a tensor where it is; B: the bins that go with it."""
    x = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    nd = (1, 2) if vector else (2, 3)
    if x.dim() not in nd or x.dtype == torch.bool:
        raise ValueError("%s: expected %s, got %s %s" % (what, "[T] or [N, T]" if vector else "[%s, T] or [N, %s, T]" % (second, second), x.dtype,
                                                         tuple(x.shape)))
    N = x.shape[0] if x.dim() == nd[1] else 1
    T = x.shape[-1]
    A = 1 if vector else x.shape[-2]
    if N > MAX_SIGNALS:
        raise ValueError("%s: expected at most %d signals, got %d" % (what, MAX_SIGNALS, N))
    if not vector and not lo <= A <= hi:
        raise ValueError("%s: expected %d <= %s <= %d, got %s" % (what, lo, second, hi, tuple(x.shape)))
    if not 1 <= T <= MAX_FRAMES:
        raise ValueError("%s: expected 1 <= T (frames) <= %d, got %s" % (what, MAX_FRAMES, tuple(x.shape)))
    if N * A * T > MAX_ELEMENTS:
        raise ValueError("%s: expected at most 2^31 - 1 elements, got %s" % (what, tuple(x.shape)))
    if B is not None and N * (B + 1) * T > MAX_ELEMENTS:
        raise ValueError("%s, f0s: N * (B + 1) * T must be at most 2^31 - 1, got N = %d, B = %d, T = %d" % (what, N, B, T))
    return x, N


def _check_rows(rows, N, T, what="rows"):
    rows = _int(rows, what, MIN_ROWS, MAX_ROWS)
    if N * rows * T > MAX_ELEMENTS:
        raise ValueError("%s: N * rows * T must be at most 2^31 - 1, got N = %d, rows = %d, T = %d" % (what, N, rows, T))
    return rows


def _dev(a, dev, dtype):
    return torch.as_tensor(a, dtype=dtype).to(dev)


def _work(nbytes, dev):
    return torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)


def _positions(lib, grid, H, bin_hz, rows, dev):
    """(idx int32 [B, H], frac float64 [B, H]) on ``dev``: computed on the host by the library (``glowk_melody_positions``)."""
    idx, frac = np.empty((grid.shape[0], H), np.int32), np.empty((grid.shape[0], H), np.float64)
    as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(lib.glowk_melody_positions(as_p(grid), grid.shape[0], H, bin_hz, rows, as_p(idx), as_p(frac)))
    return _dev(idx, dev, torch.int32), _dev(frac, dev, torch.float64)


def salience(S, f0s, harmonics=8, decay=0.8, weights=None, bin_hz=BIN_HZ):
    """The harmonic salience of real, non-negative spectra S [rows, T] or [N, rows, T] (rows ``bin_hz`` apart) on the grid ``f0s`` [B]:
    ``sal[b, t] = sum_h w_h ((1 - a) S[i, t] + a S[i + 1, t])`` with ``i + a = h f0_b / bin_hz``, over the harmonics h = 1 .. H that lie
    below the last row; ``w_h = decay ** (h - 1)`` or ``weights`` [H].  fp64, h ascending, rounded once: float32 [.., B, T]
    (``glowk_melody_salience``, one launch)."""
    grid, w, bin_hz = _grid(f0s), _weights(harmonics, decay, weights), _number(bin_hz, "bin_hz", positive=True)
    B, H = grid.shape[0], w.shape[0]
    x, N = _planes(S, "S", "rows", MIN_ROWS, MAX_ROWS, B=B)
    if x.is_complex():
        raise ValueError("S: expected real spectra, got %s" % x.dtype)
    dev = audio._device(x)
    x = x.to(device=dev, dtype=torch.float32).contiguous()
    R, T = x.shape[-2], x.shape[-1]
    out = torch.empty(tuple(x.shape[:-2]) + (B, T), dtype=torch.float32, device=dev)
    if N == 0:
        return out
    lib = _lib.load()
    idx, frac = _positions(lib, grid, H, bin_hz, R, dev)
    wd = _dev(w, dev, torch.float64)
    _lib.check(lib.glowk_melody_salience(_p(x), N, R, T, _p(idx), _p(frac), _p(wd), B, H, _p(out), _s(x)))
    return out


def emission(sal, return_max=False):
    """The emission scores of a salience plane [B, T] or [N, B, T]: ``float64(sal) / max(float64(m), 2^-40)``, m the maximum of the
    signal's whole plane; float64, shaped like ``sal``; with ``return_max`` also m, float32 [N] (``glowk_melody_emission``)."""
    _flag(return_max, "return_max")
    x, N = _planes(sal, "sal", "B", 1, MAX_BINS)
    if x.is_complex():
        raise ValueError("sal: expected a real plane, got %s" % x.dtype)
    B, T = x.shape[-2], x.shape[-1]
    _planes(x, "sal", "B", 1, MAX_BINS, B=B)
    dev = audio._device(x)
    x = x.to(device=dev, dtype=torch.float32).contiguous()
    e = torch.empty(x.shape, dtype=torch.float64, device=dev)
    m = torch.empty(tuple(x.shape[:-2]), dtype=torch.float32, device=dev)
    if N:
        lib = _lib.load()
        nbytes = lib.glowk_melody_emission_workspace_bytes(N, B, T)
        work = _work(nbytes, dev)
        _lib.check(lib.glowk_melody_emission(_p(x), N, B, T, _p(e), _p(m), _p(work), nbytes, _s(x)))
    return (e, m) if return_max else e


def track(e, threshold=0.2, jump_penalty=0.02, voicing_penalty=0.5, max_jump=12, return_ticks=False):
    """The Viterbi path through emission scores e [B, T] or [N, B, T] (float64): int32 [.., T] with values in [0, B], B meaning
    "unvoiced".  Staying unvoiced scores ``threshold`` per frame, a jump of d <= ``max_jump`` bins costs ``jump_penalty * d``, a change of
    voicing ``voicing_penalty``; ties go to the earliest candidate (include/glowk.h states the order).  Only fp64 adds, subtractions and
    compares: the path equals a numpy loop's in every frame (``glowk_melody_track``: one launch, one workgroup per signal).  With
    ``return_ticks`` also int64 [.., 2]: the ticks of the device's 100 MHz clock the recursion and the back-trace took."""
    theta, pen, nu, J = _track_params(threshold, jump_penalty, voicing_penalty, max_jump)
    _flag(return_ticks, "return_ticks")
    x, N = _planes(e, "e", "B", 1, MAX_BINS)
    if x.is_complex():
        raise ValueError("e: expected a real plane, got %s" % x.dtype)
    B, T = x.shape[-2], x.shape[-1]
    _planes(x, "e", "B", 1, MAX_BINS, B=B)
    dev = audio._device(x)
    x = x.to(device=dev, dtype=torch.float64).contiguous()
    path = torch.empty(tuple(x.shape[:-2]) + (T,), dtype=torch.int32, device=dev)
    ticks = torch.zeros(tuple(x.shape[:-2]) + (2,), dtype=torch.int64, device=dev) if return_ticks else None
    if N:
        lib = _lib.load()
        nbytes = lib.glowk_melody_track_workspace_bytes(N, B, T)
        work = _work(nbytes, dev)
        pd = _dev(pen, dev, torch.float64)
        _lib.check(lib.glowk_melody_track(_p(x), N, B, T, _p(pd), J, theta, nu, _p(path), _p(ticks), _p(work), nbytes, _s(x)))
    return (path, ticks) if return_ticks else path


def harmonic_mask(path, f0s, rows=1025, n_harmonics=20, width=40.0, bin_hz=BIN_HZ):
    """The comb mask of a path [T] or [N, T] (integers in [0, B]) on the grid ``f0s`` [B]: float32 [.., rows, T], 0 where the path is
    unvoiced, else ``max(0, 1 - min_h |f bin_hz - h f0| / width)`` over h = 1 .. ``n_harmonics`` in fp64, rounded once
    (``glowk_melody_mask``, one launch)."""
    grid = _grid(f0s)
    Hm, width, bin_hz = _mask_params(n_harmonics, width, bin_hz)
    B = grid.shape[0]
    p, N = _planes(path, "path", "", 1, 1, B=B, vector=True)
    if p.is_complex() or p.is_floating_point():
        raise ValueError("path: expected integers, got %s" % p.dtype)
    T = p.shape[-1]
    rows = _check_rows(rows, N, T)
    dev = audio._device(p)
    p = p.to(device=dev, dtype=torch.int32).contiguous()
    out = torch.empty(tuple(p.shape[:-1]) + (rows, T), dtype=torch.float32, device=dev)
    if N:
        gd = _dev(grid, dev, torch.float64)
        _lib.check(_lib.load().glowk_melody_mask(_p(p), N, T, _p(gd), B, rows, Hm, width, bin_hz, _p(out), _s(p)))
    return out


def melody(S, f0s=None, harmonics=8, decay=0.8, weights=None, bin_hz=BIN_HZ, threshold=0.2, jump_penalty=0.02, voicing_penalty=0.5,
           max_jump=12, n_harmonics=20, width=40.0, power=2.0, mask=False, return_f0=False):
    """Spectra [rows, T] or [N, rows, T] -> ``(lead, accompaniment)`` shaped like S: the salience of |S| on ``f0s`` (default
    ``f0_grid()``), its emission, the Viterbi path and the comb mask m around it in one library call (``glowk_melody_fit``: bit for bit
    ``salience``, ``emission``, ``track`` and ``harmonic_mask``).  The first estimates m |S| and (1 - m) |S| become the final soft masks
    as in ``hpss.hpss``, ``librosa.util.softmask`` with exponent ``power`` and unit margins (``glowk_hpss_mask``); ``power = 1`` returns
    m and 1 - m themselves.  Complex S is split into magnitude and phase and the components come back complex64 with S's phase; real S
    gives float32 magnitudes.  ``mask=True`` returns the two masks instead.  ``return_f0`` adds the tracked fundamental, float64
    [.., T] in Hz, 0 where unvoiced."""
    grid, w, bin_hz = _grid(f0s), _weights(harmonics, decay, weights), _number(bin_hz, "bin_hz", positive=True)
    theta, pen, nu, J = _track_params(threshold, jump_penalty, voicing_penalty, max_jump)
    Hm, width, _ = _mask_params(n_harmonics, width, bin_hz)
    power, mask, return_f0 = _power(power), _flag(mask, "mask"), _flag(return_f0, "return_f0")
    B, H = grid.shape[0], w.shape[0]
    x, N = _planes(S, "S", "rows", MIN_ROWS, MAX_ROWS, B=B)
    dev = audio._device(x)
    phase = None
    if x.is_complex():
        x = x.to(device=dev, dtype=torch.complex64)
        phase = torch.polar(torch.ones_like(x.real), x.angle())                          # exp(i angle(S)), angle(0) = 0
        x = x.abs()
    x = x.to(device=dev, dtype=torch.float32).contiguous()
    R, T = x.shape[-2], x.shape[-1]
    lead = tuple(x.shape[:-2])
    path = torch.full(lead + (T,), B, dtype=torch.int32, device=dev)
    m = torch.zeros_like(x)
    if N:
        lib = _lib.load()
        idx, frac = _positions(lib, grid, H, bin_hz, R, dev)
        wd, gd, pd = _dev(w, dev, torch.float64), _dev(grid, dev, torch.float64), _dev(pen, dev, torch.float64)
        peak = torch.empty(lead, dtype=torch.float32, device=dev)
        nbytes = lib.glowk_melody_workspace_bytes(N, B, T)
        work = _work(nbytes, dev)
        _lib.check(lib.glowk_melody_fit(_p(x), N, R, T, _p(idx), _p(frac), _p(wd), _p(gd), B, H, _p(pd), J, theta, nu, Hm, width, bin_hz, _p(path),
                                        _p(m), _p(peak), _p(work), nbytes, _s(x)))
    if power == 1.0:
        out_l, out_a = (m, 1.0 - m) if mask else (m * x, (1.0 - m) * x)
    else:
        first_l, first_a = m * x, (1.0 - m) * x
        out_l, out_a = torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.load().glowk_hpss_mask(_p(first_l), _p(first_a), None if mask else _p(x), x.numel(), power, 1.0, 1.0, _p(out_l), _p(out_a),
                                               _s(x)))
    if not mask and phase is not None:
        out_l, out_a = out_l * phase, out_a * phase
    if not return_f0:
        return out_l, out_a
    table = torch.cat([_dev(grid, dev, torch.float64), torch.zeros(1, dtype=torch.float64, device=dev)])
    return out_l, out_a, table[path.long()]


def _check_melody_kwargs(kw):
    """Every keyword of ``melody`` that ``melody_audio`` passes on, checked without a device."""
    _grid(kw.get("f0s"))
    _weights(kw.get("harmonics", 8), kw.get("decay", 0.8), kw.get("weights"))
    _track_params(*(kw.get(k, d) for k, d in zip(TRACK_KEYS, (0.2, 0.02, 0.5, 12))))
    _mask_params(kw.get("n_harmonics", 20), kw.get("width", 40.0), kw.get("bin_hz", BIN_HZ))
    _power(kw.get("power", 2.0))


def melody_audio(y, **kwargs):
    """16 kHz audio [n] or [C, n], n > 1024 -> ``(lead, accompaniment)``, each shaped like y and aligned with it.  One STFT of the whole
    signal (``audio.mel_frames``), ``melody`` on |X| per channel, the masked magnitudes with the mixture's phase through one
    ``audio.griffinlim(n_iter=0)`` of all 2 C spectra, trimmed to n samples.  A channel's stems depend on that channel alone.
    ``kwargs`` are ``melody``'s keyword arguments but ``mask`` and ``return_f0``."""
    unknown = set(kwargs) - set(MELODY_KEYS)
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected melody's" % sorted(unknown))
    _check_melody_kwargs(kwargs)
    t = audio._tensor(y, "y")
    x = audio._long_audio(t)
    if x.shape[0] > MAX_SIGNALS:
        raise ValueError("y: expected at most %d channels, got %d" % (MAX_SIGNALS, x.shape[0]))
    lead, n = tuple(t.shape[:-1]), x.shape[1]
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [C, 1025, F]
    mags = torch.cat(melody(X.abs(), **kwargs))                                          # [2 C, 1025, F]
    phase = torch.polar(torch.ones_like(X.real), X.angle())
    stems = audio.griffinlim(mags, n_iter=0, init=torch.cat([phase, phase]))[:, :n].reshape((2,) + lead + (n,))
    return stems[0].contiguous(), stems[1].contiguous()


def separate_wav_melody(path, out_rate="input", mono=False, **kwargs):
    """``melody_audio`` for a PCM wav at any rate -> ``(stems, rate)``: stems [2, n'] (lead, accompaniment) of a one-channel file or
    with ``mono`` (the channels averaged), else [2, C, n'] with the file's C channels, at ``out_rate``: 'input' (the file's rate), an
    integer rate, or None (left at 16 kHz).  The file is resampled to 16 kHz on the GPU, the stems back in one launch; with
    ``out_rate='input'`` they have exactly the file's sample count.  ``kwargs`` are ``melody_audio``'s keyword arguments."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    _flag(mono, "mono")
    unknown = set(kwargs) - set(MELODY_KEYS)
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected melody_audio's" % sorted(unknown))
    _check_melody_kwargs(kwargs)
    y, native = audio.load_audio(path, sr=None, mono=False)
    n_file = y.shape[1]
    y = y.mean(0) if mono or y.shape[0] == 1 else y
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    stems = audio.resample(torch.stack(melody_audio(y, **kwargs)), audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate
