"""Kernel additive modelling (Liutkus, FitzGerald, Rafii, Pardo & Daudet, "Kernel additive models for source separation", IEEE TSP
2014; the light form, KAML, 2015): every source has a proximity kernel -- the set of time-frequency neighbours it is locally
constant over -- and the sources are estimated together by back-fitting: median-filter each source's estimate over its own kernel,
share the mixture out by the ratio of the results, repeat.  With two sources, a horizontal and a vertical kernel and one iteration it
is ``hpss.hpss``; with a periodic kernel, the adaptive REPET; several kernels and a few iterations separate what no single one of the
package's median-filter methods can: drums, a repeating accompaniment and a voice in one file.  ``cluster.ensemble`` combines the
separators' masks after the fact; this combines their models before any mask exists.  Not in the reference.

Kernels in ``csrc/glowk_kam.h`` (``glowk_kam_median``, ``glowk_kam_backfit``, ``glowk_kam_fit``; rules in include/glowk.h):

* kernel builders (host, int32 numpy ``[n, 2]`` tables of ``(d_row, d_frame)``): ``harmonic``, ``percussive``, ``periodic``, ``cross``,
  ``rectangle``; ``check_kernel`` applies the table's rules to a caller's own array;
* ``median``: the median of every cell's neighbours under a table -- those inside the plane; no reflection -- selected by compares;
* ``backfit``: the J soft masks of J filtered estimates and the mixture shared out by them (``hpss``'s mask from 2 to J sources);
* ``fit``: the loop in one library call.  A source's model is an offset table (a numpy array or a nested list) or a frame-neighbour
  tensor (a torch int32 tensor ``[.., F, k]``: what ``repet.neighbors`` and ``repet.period_neighbors`` return);
* ``kam``: spectra in, ``[.., J, rows, T]`` components (or masks) out; complex input keeps its phase;
* ``kam_audio`` / ``separate_wav_kam``: 16 kHz audio / a PCM wav in, one stem per source out, through the STFT, phase, inversion and
  trimming of ``hpss.hpss_audio`` / ``hpss.separate_wav_hpss``.  The stems add up to the input.

Conventions as in ``hpss.py``: numpy or torch in, float32 tensors on the GPU the input lives on (the current one for host input) out,
ValueError for bad arguments before the library is loaded.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, audio, repet
from .audio import _p, _s

MAX_N, MAX_DROW, MAX_DFRAME = 127, 4095, 32767          # glowk_kam_median: the offset table
MAX_ROWS, MAX_FRAMES, MAX_SIGNALS, MAX_SOURCES, MAX_ITER = 4096, 32768, 65535, 8, 100
MAX_ELEMENTS = (1 << 31) - 1
SOURCE_NAMES = ("harmonic", "percussive", "repeating", "similar")


# ---- kernel builders -----------------------------------------------------------------------------------------------------------------------
def _odd(v, what, top=MAX_N):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= v <= top or v % 2 == 0:
        raise ValueError("%s: expected an odd integer in [1, %d], got %r" % (what, top, v))
    return int(v)


def _table(pairs):
    return np.asarray(pairs, dtype=np.int32).reshape(-1, 2)


def harmonic(size):
    """``size`` (odd, in [1, 127]) cells along time: (0, -size // 2 .. size // 2)."""
    h = _odd(size, "size") // 2
    return _table([(0, d) for d in range(-h, h + 1)])


def percussive(size):
    """``size`` (odd, in [1, 127]) cells along frequency: (-size // 2 .. size // 2, 0)."""
    h = _odd(size, "size") // 2
    return _table([(d, 0) for d in range(-h, h + 1)])


def periodic(period, repeats):
    """The cells whole periods away in time, the cell itself included: (0, i period) for i = -repeats .. repeats.  ``period`` >= 1,
    ``repeats`` in [0, 63], ``repeats * period`` <= 32767."""
    for name, v, lo, hi in (("period", period, 1, MAX_DFRAME), ("repeats", repeats, 0, MAX_N // 2)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s: expected an integer in [%d, %d], got %r" % (name, lo, hi, v))
    if int(period) * int(repeats) > MAX_DFRAME:
        raise ValueError("periodic: repeats * period must be at most %d, got %d * %d" % (MAX_DFRAME, repeats, period))
    return _table([(0, i * int(period)) for i in range(-int(repeats), int(repeats) + 1)])


def cross(rows, frames):
    """A horizontal run of ``frames`` cells, then a vertical run of ``rows`` cells without its centre (the centre counts once).  Both
    odd, ``rows + frames - 1`` <= 127."""
    hr, hf = _odd(rows, "rows") // 2, _odd(frames, "frames") // 2
    if rows + frames - 1 > MAX_N:
        raise ValueError("cross: rows + frames - 1 must be at most %d, got %d" % (MAX_N, rows + frames - 1))
    return _table([(0, d) for d in range(-hf, hf + 1)] + [(d, 0) for d in range(-hr, hr + 1) if d])


def rectangle(rows, frames):
    """Every cell of a ``rows`` x ``frames`` box centred on the cell, row by row.  Both odd, ``rows * frames`` <= 127."""
    hr, hf = _odd(rows, "rows") // 2, _odd(frames, "frames") // 2
    if rows * frames > MAX_N:
        raise ValueError("rectangle: rows * frames must be at most %d, got %d" % (MAX_N, rows * frames))
    return _table([(dr, df) for dr in range(-hr, hr + 1) for df in range(-hf, hf + 1)])


def check_kernel(k, what="kernel"):
    """A caller's own table, checked -> int32 numpy [n, 2] (C-contiguous): integers ``[n, 2]`` of (d_row, d_frame) with 1 <= n <= 127,
    ``|d_row|`` <= 4095 and ``|d_frame|`` <= 32767.  Duplicates are allowed and count twice; (0, 0) need not be present."""
    if torch.is_tensor(k):
        raise ValueError("%s: expected a host array of offsets [n, 2], got a tensor (tensors are frame-neighbour models)" % what)
    try:
        a = np.asarray(k)
    except Exception:
        raise ValueError("%s: expected an integer array [n, 2], got %r" % (what, type(k).__name__))
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer) or a.ndim != 2 or a.shape[1] != 2 or not 1 <= a.shape[0] <= MAX_N:
        raise ValueError("%s: expected integers [n, 2] with 1 <= n <= %d, got %s %s" % (what, MAX_N, a.dtype, a.shape))
    a = a.astype(np.int64)
    if np.abs(a[:, 0]).max() > MAX_DROW or np.abs(a[:, 1]).max() > MAX_DFRAME:
        raise ValueError("%s: expected |d_row| <= %d and |d_frame| <= %d" % (what, MAX_DROW, MAX_DFRAME))
    return np.ascontiguousarray(a, dtype=np.int32)


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------
def _check_power(power):
    if isinstance(power, (bool, np.bool_)) or not isinstance(power, (int, float, np.integer, np.floating)) or not (math.isfinite(power) and power > 0):
        raise ValueError("power: expected a finite number > 0, got %r" % (power,))
    return float(power)


def _check_iter(n_iter):
    if isinstance(n_iter, (bool, np.bool_)) or not isinstance(n_iter, (int, np.integer)) or not 1 <= n_iter <= MAX_ITER:
        raise ValueError("n_iter: expected an integer in [1, %d], got %r" % (MAX_ITER, n_iter))
    return int(n_iter)


def _check_flag(v, what):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("%s: expected True or False, got %r" % (what, v))
    return bool(v)


def _spectra(S, what="S", J=1):
    """[rows, F] or [N, rows, F] within the kernels' ranges, as a tensor where it is."""
    x = S if torch.is_tensor(S) else torch.as_tensor(np.asarray(S))
    if x.dim() not in (2, 3) or not 1 <= x.shape[-2] <= MAX_ROWS or not 1 <= x.shape[-1] <= MAX_FRAMES \
            or (x.dim() == 3 and x.shape[0] > MAX_SIGNALS) or x.numel() * J > MAX_ELEMENTS:
        raise ValueError("%s: expected [rows, F] or [N, rows, F] with N <= %d, 1 <= rows <= %d, 1 <= F <= %d and at most 2^31 - 1 "
                         "elements (times the number of sources), got %s" % (what, MAX_SIGNALS, MAX_ROWS, MAX_FRAMES, tuple(x.shape)))
    return x


def _real(x, what="S"):
    if x.is_complex():
        raise ValueError("%s: expected real spectra, got %s" % (what, x.dtype))
    return x


def _check_models(models, lead, F):
    """-> [("offsets", table) or ("index", tensor)] for spectra with leading shape ``lead`` and F frames."""
    if isinstance(models, (np.ndarray, torch.Tensor)) or not isinstance(models, (tuple, list)) or not 1 <= len(models) <= MAX_SOURCES:
        raise ValueError("models: expected a sequence of 1 to %d models (offset arrays or int32 index tensors), got %r"
                         % (MAX_SOURCES, type(models).__name__ if not isinstance(models, (tuple, list)) else len(models)))
    out = []
    nsig = int(np.prod(lead)) if lead else 1
    for j, m in enumerate(models):
        if torch.is_tensor(m):
            if m.dtype != torch.int32 or m.dim() != len(lead) + 2 or tuple(m.shape[:-1]) != tuple(lead) + (F,) or not 1 <= m.shape[-1] <= repet.MAX_K:
                raise ValueError("models[%d]: expected an int32 index tensor %s with 1 <= k <= %d, got %s %s"
                                 % (j, tuple(lead) + (F, "k"), repet.MAX_K, m.dtype, tuple(m.shape)))
            if nsig * F * m.shape[-1] > MAX_ELEMENTS:
                raise ValueError("models[%d]: N * F * k must be at most 2^31 - 1, got %s" % (j, tuple(m.shape)))
            out.append(("index", m))
        else:
            out.append(("offsets", check_kernel(m, "models[%d]" % j)))
    return out


# ---- the calls -----------------------------------------------------------------------------------------------------------------------------
def _host(a):
    return ctypes.c_void_p(a.ctypes.data)


def _median(x, table):
    """x: float32 contiguous [.., rows, F] on the GPU."""
    out = torch.empty_like(x)
    nsig = x.numel() // (x.shape[-2] * x.shape[-1])
    _lib.check(_lib.load().glowk_kam_median(_p(x), nsig, x.shape[-2], x.shape[-1], _host(table), table.shape[0], _p(out), _s(x)))
    return out


def median(S, kernel):
    """The median over a sparse kernel of real spectra [rows, F] or [N, rows, F] -> float32, shaped like S.  ``kernel`` is a table of
    offsets (``check_kernel``).  The neighbours of cell (r, t) are the cells (r + d_row, t + d_frame) inside the plane; the others are
    skipped (no reflection).  With m of them: m odd, the middle element, the bits a sort gives; m even, ``(a + b) * 0.5f`` of the two
    middle ones; m = 0, the cell itself -- ``repet.nn_filter``'s rules.  ``glowk_kam_median``: one launch, bitwise reproducible, a batch
    gives what its signals give alone."""
    table = check_kernel(kernel)
    x = _real(_spectra(S))
    x = x.to(device=audio._device(x), dtype=torch.float32).contiguous()
    return _median(x, table)


def backfit(V, A, power=2.0, return_masks=False):
    """The back-fitting step: the mixture V [rows, F] or [N, rows, F] shared out over the J filtered estimates A [J, rows, F] or
    [N, J, rows, F] (>= 0) -> P shaped like A; with ``return_masks`` also the masks.  ``hpss``'s soft mask from 2 to J sources:
    ``Z = max_j A_j``, ``r_j = (A_j / Z)^power``, ``mask_j = r_j / sum_i r_i`` (1 / J where Z < FLT_MIN), ``P_j = V mask_j``, in fp32.
    ``glowk_kam_backfit``: one launch."""
    power, return_masks = _check_power(power), _check_flag(return_masks, "return_masks")
    a = A if torch.is_tensor(A) else torch.as_tensor(np.asarray(A))
    if a.dim() not in (3, 4) or not 1 <= a.shape[-3] <= MAX_SOURCES:
        raise ValueError("A: expected [J, rows, F] or [N, J, rows, F] with 1 <= J <= %d, got %s" % (MAX_SOURCES, tuple(a.shape)))
    J = a.shape[-3]
    v = _real(_spectra(V, "V", J), "V")
    _real(a, "A")
    if tuple(a.shape[:-3]) + tuple(a.shape[-2:]) != tuple(v.shape):
        raise ValueError("A: expected %s for V %s, got %s" % (tuple(v.shape[:-2]) + (J,) + tuple(v.shape[-2:]), tuple(v.shape), tuple(a.shape)))
    dev = audio._device(v, a)
    v = v.to(device=dev, dtype=torch.float32).contiguous()
    a = a.to(device=dev, dtype=torch.float32).contiguous()
    p = torch.empty_like(a)
    masks = torch.empty_like(a) if return_masks else None
    cells = v.shape[-2] * v.shape[-1]
    _lib.check(_lib.load().glowk_kam_backfit(_p(v), _p(a), v.numel() // cells, J, cells, power, _p(p), _p(masks), _s(v)))
    return (p, masks) if return_masks else p


def _fit(v, models, n_iter, power, want_masks):
    """v: float32 contiguous [.., rows, F] on the GPU; models: ``_check_models``' list."""
    lib = _lib.load()
    rows, F = v.shape[-2:]
    lead = tuple(v.shape[:-2])
    nsig, J = v.numel() // (rows * F), len(models)
    model_n = np.array([m.shape[0] if kind == "offsets" else 0 for kind, m in models], dtype=np.int32)
    model_k = np.array([m.shape[-1] if kind == "index" else 0 for kind, m in models], dtype=np.int32)
    tables = [m for kind, m in models if kind == "offsets"]
    offsets = np.ascontiguousarray(np.concatenate(tables)) if tables else np.zeros((1, 2), np.int32)
    idx = [m.to(device=v.device).contiguous() if kind == "index" else None for kind, m in models]
    ptrs = (ctypes.c_void_p * J)(*[None if t is None else t.data_ptr() for t in idx])
    p = torch.empty(lead + (J, rows, F), dtype=torch.float32, device=v.device)
    masks = torch.empty_like(p) if want_masks else None
    nbytes = lib.glowk_kam_work_bytes(nsig, rows, F, J, _host(model_k))
    work = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=v.device)
    _lib.check(lib.glowk_kam_fit(_p(v), nsig, rows, F, J, _host(model_n), _host(offsets), _host(model_k), ctypes.cast(ptrs, ctypes.c_void_p), n_iter,
                                 power, _p(p), _p(masks), _p(work), nbytes, _s(v)))
    return p, masks


def fit(V, models, n_iter=3, power=2.0, return_masks=False):
    """Back-fitting of the mixture magnitudes V [rows, F] or [N, rows, F] over ``models``, one per source -> P [.., J, rows, F]; with
    ``return_masks`` also the last iteration's masks.  A model is an offset table (a numpy array or a nested list, ``check_kernel``) or a
    frame-neighbour tensor (a torch int32 tensor [.., F, k], ``repet.neighbors`` / ``repet.period_neighbors``).  ``P_j = V`` to begin
    with; each of the ``n_iter`` iterations (in [1, 100]) filters every ``P_j`` with its own model (``median`` / ``repet.nn_filter``'s
    median) and applies ``backfit``.  One library call (``glowk_kam_fit``), bit for bit the staged rounds."""
    n_iter, power, return_masks = _check_iter(n_iter), _check_power(power), _check_flag(return_masks, "return_masks")
    if not isinstance(models, (tuple, list)):
        _check_models(models, (), 1)
    v = _real(_spectra(V, "V", max(len(models), 1)), "V")
    models = _check_models(models, tuple(v.shape[:-2]), v.shape[-1])
    dev = audio._device(v, *[m for kind, m in models if kind == "index"])
    v = v.to(device=dev, dtype=torch.float32).contiguous()
    p, masks = _fit(v, models, n_iter, power, return_masks)
    return (p, masks) if return_masks else p


def kam(S, models, n_iter=3, power=2.0, mask=False):
    """Kernel additive modelling of spectra [rows, T] or [N, rows, T] -> the J components [.., J, rows, T]: ``fit`` on |S|.  Complex S
    is split into magnitude and phase and the components come back complex64 with S's phase; real S (magnitudes) gives float32.
    ``mask=True`` returns the masks instead.  With ``models = (harmonic(31), percussive(31))`` and ``n_iter = 1`` this is
    ``hpss.hpss``."""
    n_iter, power, mask = _check_iter(n_iter), _check_power(power), _check_flag(mask, "mask")
    if not isinstance(models, (tuple, list)):
        _check_models(models, (), 1)
    x = _spectra(S, "S", max(len(models), 1))
    models = _check_models(models, tuple(x.shape[:-2]), x.shape[-1])
    dev = audio._device(x, *[m for kind, m in models if kind == "index"])
    phase = None
    if x.is_complex():
        x = x.to(device=dev, dtype=torch.complex64)
        phase = torch.polar(torch.ones_like(x.real), x.angle())                          # exp(i angle(S)), angle(0) = 0
        x = x.abs()
    x = x.to(device=dev, dtype=torch.float32).contiguous()
    p, masks = _fit(x, models, n_iter, power, mask)
    if mask:
        return masks
    return p if phase is None else p * phase.unsqueeze(-3)


# ---- audio ---------------------------------------------------------------------------------------------------------------------------------
_KAM_AUDIO_DEFAULTS = dict(sources=("harmonic", "percussive"), n_iter=3, power=2.0, kernel_size=31, period_sec=(0.8, 8.0), k=None, width_sec=2.0)


def _check_audio_params(sources, n_iter, power, kernel_size, period_sec, k, width_sec):
    """The arguments of ``kam_audio`` that do not depend on the signal, checked -> (sources with the arrays checked, (pmin, pmax) in
    frames, width in frames)."""
    _check_iter(n_iter)
    _check_power(power)
    _odd(kernel_size, "kernel_size")
    if isinstance(sources, (str, np.ndarray, torch.Tensor)) or not isinstance(sources, (tuple, list)) or not 1 <= len(sources) <= MAX_SOURCES:
        raise ValueError("sources: expected a sequence of 1 to %d sources (%s, or offset arrays), got %r" % (MAX_SOURCES, ", ".join(SOURCE_NAMES), sources))
    out = []
    for j, s in enumerate(sources):
        if isinstance(s, str):
            if s not in SOURCE_NAMES:
                raise ValueError("sources[%d]: expected one of %s or an offset array, got %r" % (j, SOURCE_NAMES, s))
            out.append(s)
        else:
            out.append(check_kernel(s, "sources[%d]" % j))
    pmin, pmax, _, _, _ = repet._check_repet_audio_params(False, period_sec, 10.0, 5.0, 5, 0.0, 1.0, 1.0, False)
    width = repet._check_audio_params(k, width_sec, 1.0, 1.0, False)
    return out, (pmin, pmax), width


def kam_audio(y, sources=("harmonic", "percussive"), n_iter=3, power=2.0, kernel_size=31, period_sec=(0.8, 8.0), k=None, width_sec=2.0):
    """Kernel additive modelling for 16 kHz audio [n] or [C, n], n > 1024 -> a tuple of one stem per source, each shaped like y and
    aligned with it.  ``hpss.hpss_audio``'s path: one STFT of the whole signal, ``fit`` on |X| with every channel a signal of its own,
    the shared-out magnitudes with the mixture's phase through one ``audio.griffinlim(n_iter=0)``, trimmed to n samples.  The masks
    add up to one, so the stems add up to y.

    A source is a name or an explicit offset array (``check_kernel``):

    * ``"harmonic"`` / ``"percussive"``: ``harmonic(kernel_size)`` / ``percussive(kernel_size)``;
    * ``"repeating"``: the frames whole periods away, the period from ``repet.beat_spectrum`` and ``repet.find_period`` as
      ``repet.repet_audio`` finds it (``period_sec``, the longest capped at a third of the signal), ``repet.period_neighbors`` with
      every repetition (at most 512);
    * ``"similar"``: ``repet.neighbors`` with ``k`` neighbours (default ``repet.default_k``) at least ``width_sec`` away, as
      ``repet.repet_sim_audio`` finds them."""
    srcs, (pmin, pmax), width = _check_audio_params(sources, n_iter, power, kernel_size, period_sec, k, width_sec)
    t = audio._tensor(y, "y")
    x = audio._long_audio(t)
    if x.shape[0] > MAX_SIGNALS:
        raise ValueError("y: expected at most %d channels, got %d" % (MAX_SIGNALS, x.shape[0]))
    lead, n = tuple(t.shape[:-1]), x.shape[1]
    F = 1 + -(-n // audio.HOP)
    if F > MAX_FRAMES:
        raise ValueError("y: expected at most %d frames (%d samples), got %d samples" % (MAX_FRAMES, (MAX_FRAMES - 2) * audio.HOP, n))
    if any(isinstance(s, str) and s == "repeating" for s in srcs):
        pmax = min(pmax, F // 3)
        if pmin > pmax:
            raise ValueError("period_sec: the shortest period, %d frames, is more than a third of the signal (%d frames)" % (pmin, F))
    J, C = len(srcs), x.shape[0]
    if C * J * audio.NBIN * F > MAX_ELEMENTS:
        raise ValueError("y: channels * sources * 1025 * frames must be at most 2^31 - 1, got %d channels, %d sources, %d frames" % (C, J, F))
    x = x.to(device=audio._device(x), dtype=torch.float32)
    _, X = audio.mel_frames(x, return_stft=True)                                         # [C, 1025, F]
    mag = X.abs().contiguous()
    models = []
    for s in srcs:
        if isinstance(s, str) and s == "repeating":
            period = repet.find_period(repet.beat_spectrum(mag, pmax + 1), pmin, pmax)
            models.append(("index", repet.period_neighbors(period, F, min(repet.MAX_K, -(-F // pmin)))))
        elif isinstance(s, str) and s == "similar":
            models.append(("index", repet.neighbors(mag, k, width)))
        else:
            models.append(("offsets", harmonic(kernel_size) if isinstance(s, str) and s == "harmonic" else percussive(kernel_size)
                           if isinstance(s, str) else s))
    p, _ = _fit(mag, models, n_iter, power, False)                                       # [C, J, 1025, F]
    mags = p.transpose(0, 1).reshape(J * C, audio.NBIN, F)
    phase = torch.polar(torch.ones_like(X.real), X.angle())
    stems = audio.griffinlim(mags, n_iter=0, init=torch.cat([phase] * J))[:, :n].reshape((J,) + lead + (n,))
    return tuple(stems[j].contiguous() for j in range(J))


def separate_wav_kam(path, out_rate="input", mono=False, **kwargs):
    """``kam_audio`` for a PCM wav at any rate -> ``(stems, rate)``: stems [J, n'] of a one-channel file or with ``mono`` (the channels
    averaged), else [J, C, n'] with the file's C channels, at ``out_rate``: 'input' (the file's rate and exactly its sample count), an
    integer rate, or None (left at 16 kHz).  The file is resampled to 16 kHz on the GPU, the stems back in one launch.  ``kwargs`` are
    ``kam_audio``'s keyword arguments; any other is refused before the file is opened."""
    if not (out_rate is None or (isinstance(out_rate, str) and out_rate == "input")):
        if isinstance(out_rate, str):
            raise ValueError("out_rate: expected 'input', None or an integer sampling rate, got %r" % (out_rate,))
        out_rate = audio._check_rate(out_rate, "out_rate")
    _check_flag(mono, "mono")
    unknown = set(kwargs) - set(_KAM_AUDIO_DEFAULTS)
    if unknown:
        raise ValueError("unexpected keyword arguments %s: expected kam_audio's" % sorted(unknown))
    _check_audio_params(**dict(_KAM_AUDIO_DEFAULTS, **kwargs))
    y, native = audio.load_audio(path, sr=None, mono=False)
    n_file = y.shape[1]
    y = y.mean(0) if mono or y.shape[0] == 1 else y
    if native != audio.SR:
        y = audio.resample(y, audio._check_rate(native, "%s: sampling rate" % (path,)), audio.SR)
    rate = audio.SR if out_rate is None else native if isinstance(out_rate, str) else out_rate
    stems = audio.resample(torch.stack(kam_audio(y, **kwargs)), audio.SR, rate)
    if isinstance(out_rate, str):
        stems = stems[..., :n_file].contiguous()
    return stems, rate
