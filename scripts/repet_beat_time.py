"""Times of REPET's front end (csrc/glowk_beat.h) on one GPU at 180 s of 16 kHz audio.

Shape 1 x 1025 x 5626, the |STFT| (``audio.mel_frames``) of tests/repet_ref.py's repeated phrase and chirp with a little noise.
HIP events around each C call on preallocated device tensors, median, minimum and spread of --reps runs after a warm-up:

* ``beat_spectrum_8s``: ``glowk_beat_spectrum`` at nlags = 251, the 8 s that ``repet_audio`` admits by default;
* ``beat_spectrum_full``: at nlags = F, every lag: rows F (F + 1) FLOP -- half the Gram matrix -- against the fp32-MFMA peak of
  DESIGN.md (``gram``; the time is k_beat_gram's from torch.profiler where that is available, else the entry's: a lower bound);
* ``beat_spectrogram``: 10 s windows every 5 s (win = 312, step = 156), nlags = 105;
* ``beat_period``, ``period_neighbors`` (k = ceil(F / 25) = 226: every frame a period of 25 or more away), and ``nn_median`` over
  that list, the filter of ``repet``; ``nn_median_order5`` over the 5 nearest repetitions, the filter of ``repet_adaptive``.

``host``: the fp64 restatement's time for the same shapes -- numpy's FFT autocorrelation for the whole-signal case, the sums over
pairs of tests/repet_beat_ref.py for the windows -- and the device's largest deviation from it in units of the tests' bar.

    python scripts/repet_beat_time.py --out profiles/repet_beat_time.json [--reps 10] [--no-cpu]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiosourcesep_amd import _lib, audio  # noqa: E402

FP32_MFMA_PEAK = 157.3e12                  # FLOP / s
SECONDS = 180
KERNELS = ("k_beat_gram", "k_beat_reduce", "k_beat_period", "k_period_neighbors", "k_nn_transpose", "k_nn_median")


def timed(call, reps):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), spread_ms=float(np.max(ms) - np.min(ms)), reps=reps)


def kernel_times(call):
    """{kernel name: ms} of one run of ``call`` from torch.profiler's device events."""
    from torch.profiler import ProfilerActivity, profile
    call()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        for short in KERNELS:
            if short in e.name:
                out[short] = out.get(short, 0.0) + float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0)) / 1e3
    if not out:
        raise RuntimeError("the profiler reported none of the kernels")
    return out


def spectrum():
    from tests import repet_ref as R
    n = SECONDS * audio.SR
    pattern, chirp = R.pattern_and_chirp(n)
    y = (pattern + chirp + 0.01 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)
    _, X = audio.mel_frames(y, return_stft=True)
    return X.abs().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true", help="leave out the restatement's time on the host")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("repet_beat_time.py measures on a GPU; none is visible")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    S = spectrum()
    nsig, rows, F = S.shape
    fps = audio.SR / audio.HOP
    pmin, pmax = 25, 250                                                            # 0.8 s .. 8 s
    win, step = int(10 * fps), int(5 * fps)
    res = dict(device=torch.cuda.get_device_name(0), build=os.environ.get("GLOWK_BUILD") or "unknown", fp32_mfma_peak_flops=FP32_MFMA_PEAK,
               seconds=SECONDS, shape=[nsig, rows, F], gram_matrix_bytes=4 * F * F)
    beats = {}

    def beat_entry(name, nlags, win, step):
        nwin = 1 if win == 0 else -(-F // step)
        beat = torch.empty((nsig, nwin, nlags), device="cuda")
        nbytes = lib.glowk_beat_workspace_bytes(nsig, rows, F, nlags, win, step)
        work = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")

        def call():
            _lib.check(lib.glowk_beat_spectrum(p(S), nsig, rows, F, nlags, win, step, p(beat), p(work), nbytes, stream))
        entry = dict(nlags=nlags, win=win, step=step, nwin=nwin, workspace_bytes=nbytes, **timed(call, args.reps))
        try:
            entry["kernels"] = kernel_times(call)
        except Exception as e:  # noqa: BLE001  (a machine without the profiler still gets the entry times)
            entry["kernels_error"] = "%s: %s" % (type(e).__name__, e)
        beats[name] = beat
        res[name] = entry
        return entry

    beat_entry("beat_spectrum_8s", pmax + 1, 0, 0)
    full = beat_entry("beat_spectrum_full", F, 0, 0)
    beat_entry("beat_spectrogram", win // 3 + 1, win, step)
    gram_ms, basis = full["median_ms"], "glowk_beat_spectrum entry (k_beat_reduce included): a lower bound"
    if "k_beat_gram" in full.get("kernels", {}):
        gram_ms, basis = full["kernels"]["k_beat_gram"], "k_beat_gram (Gram band + diagonal sums)"
    flop = float(rows) * F * (F + 1) * nsig
    full["gram"] = dict(flop=flop, ms=gram_ms, time_of=basis, flops_per_s=flop / (gram_ms * 1e-3),
                        fraction_of_fp32_mfma_peak=flop / (gram_ms * 1e-3) / FP32_MFMA_PEAK)

    b8 = beats["beat_spectrum_8s"].reshape(nsig, pmax + 1)
    period = torch.empty((nsig,), dtype=torch.int32, device="cuda")

    def per():
        _lib.check(lib.glowk_beat_period(p(b8), nsig, pmax + 1, pmin, pmax, p(period), stream))
    res["beat_period"] = dict(nseg=nsig, nlags=pmax + 1, pmin=pmin, pmax=pmax, **timed(per, args.reps))
    res["beat_period"]["period_frames"] = period.cpu().tolist()
    spec = beats["beat_spectrogram"]
    periods = torch.empty((nsig, spec.shape[1]), dtype=torch.int32, device="cuda")
    _lib.check(lib.glowk_beat_period(p(spec), nsig * spec.shape[1], spec.shape[2], pmin, win // 3, p(periods), stream))
    res["beat_spectrogram"]["period_frames"] = sorted(set(periods.cpu().ravel().tolist()))

    for name, k, per_t, nper, st in (("", -(-F // pmin), period, 1, 1), ("_order5", 5, periods, periods.shape[1], step)):
        idx = torch.empty((nsig, F, k), dtype=torch.int32, device="cuda")
        out = torch.empty_like(S)
        nbytes = lib.glowk_nn_workspace_bytes(nsig, rows, F, k)
        work = torch.empty(nbytes // 4, device="cuda")

        def nbr():
            _lib.check(lib.glowk_period_neighbors(p(per_t), nsig, F, nper, st, k, p(idx), stream))

        def med():
            _lib.check(lib.glowk_nn_median(p(S), p(idx), nsig, rows, F, k, p(out), p(work), nbytes, stream))
        res["period_neighbors" + name] = dict(k=k, nper=nper, step=st, **timed(nbr, args.reps))
        res["nn_median" + name] = dict(k=k, neighbours_per_frame=float((idx >= 0).sum(-1).float().mean().item()), workspace_bytes=nbytes,
                                       **timed(med, args.reps))

    if not args.no_cpu:
        from tests import repet_beat_ref as B
        host = S[0].cpu().numpy()
        t0 = time.perf_counter()
        P = host.astype(np.float64) ** 2
        acf = np.fft.irfft(np.abs(np.fft.rfft(P, 2 * F, axis=1)) ** 2, 2 * F, axis=1)[:, :F].sum(0)
        raw = acf / (rows * (F - np.arange(F)))
        fft_beat = raw / raw[0]
        t1 = time.perf_counter()
        ref8 = B.beat_spectrum(host, pmax + 1)                                      # the sums over pairs, 251 lags
        t2 = time.perf_counter()
        ref_spec = B.beat_spectrogram(host, win // 3 + 1, win, step)
        t3 = time.perf_counter()
        bar = B.bar(rows)
        dev8, dev_full, dev_spec = (beats[n][0].cpu().numpy().astype(np.float64) for n in ("beat_spectrum_8s", "beat_spectrum_full", "beat_spectrogram"))
        live = ref_spec > 0
        res["host"] = dict(fft_full_s=t1 - t0, pair_sums_251_lags_s=t2 - t1, pair_sums_spectrogram_s=t3 - t2, bar=bar,
                           worst_over_bar_8s=float((np.abs(dev8[0] - ref8) / (bar * ref8)).max()),
                           worst_over_bar_spectrogram=float((np.abs(dev_spec[live] - ref_spec[live]) / (bar * ref_spec[live])).max()),
                           worst_over_bar_full_vs_fft=float((np.abs(dev_full[0] - fft_beat) / (bar * fft_beat)).max()),
                           period_of_restatement=int(B.find_period(ref8, pmin, pmax)))
    res["note"] = ("HIP events around each C call on preallocated device tensors, median of reps after one warm-up call; kernels: device times "
                   "of one run from torch.profiler; gram: rows F (F + 1) FLOP over the time named in time_of against fp32_mfma_peak_flops; "
                   "host: fp64 numpy on the same input (the FFT form's own error is relative to lag 0, so worst_over_bar_full_vs_fft "
                   "measures the FFT as much as the device)")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
