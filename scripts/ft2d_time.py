"""Times of the 2DFT kernels (csrc/glowk_dft2.h) on one GPU.

``glowk_rdft2`` (with the magnitude plane), ``glowk_irdft2`` (with a mask), ``glowk_peak_mask`` at neighbourhood (1, 25),
``glowk_plane_std`` and ``ft2d.ft2d`` whole, on |STFT|-shaped float32 data at 1025 x 5626 (180 s of 16 kHz audio) and at the
30-extract shape 30 x 1025 x 64.  HIP events around each C call on preallocated device tensors, median, minimum and spread of
--reps runs after a warm-up.  ``numpy_s`` is the host's time for the fp64 restatement of the same array (numpy.fft, scipy.ndimage).

The two GEMM stages of each transform run inside one C call; their own durations come from the kernel records of one profiled
call (torch.profiler), and ``fraction_of_mfma_peak`` is the stage's useful flop -- 4 R fc T for a stage along frames (T, or 2 fc,
real terms for each of 2 R fc, or R T, real outputs), 8 R R fc along rows -- over its duration, against the 157.3 TFLOP/s of
v_mfma_f32_32x32x2_f32.  Where the profiler gives no kernel records the stage entries are null.

    python scripts/ft2d_time.py --out profiles/ft2d_time.json [--reps 20] [--no-cpu]
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
from audiosourcesep_amd import _lib, ft2d  # noqa: E402

MFMA_PEAK = 157.3e12                        # flop / s, fp32 matrix cores
SHAPES = [("180s", (1, 1025, 5626)), ("30_extracts", (30, 1025, 64))]
STAGES = ("k_rdft_frames", "k_cdft_rows", "k_irdft_frames")


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


def kernel_ms(call):
    """{kernel name: [durations in ms, in launch order]} of one call, or {} where the profiler records no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        call()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        out = {}
        for ev in sorted(prof.events(), key=lambda e: e.time_range.start):
            for name in STAGES:
                if name in ev.name:
                    out.setdefault(name, []).append((ev.time_range.end - ev.time_range.start) / 1e3)
        return out
    except Exception as e:                  # the timings above do not depend on it
        print("kernel records unavailable: %r" % (e,), file=sys.stderr)
        return {}


def stage(ms, flop):
    if ms is None:
        return None
    return dict(ms=ms, flop=flop, tflops=flop / ms / 1e9, fraction_of_mfma_peak=flop / (ms * 1e-3) / MFMA_PEAK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="leave out the host's time for the numpy restatement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ft2d_time.py measures on a GPU; none is visible")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = dict(device=torch.cuda.get_device_name(0), build=os.environ.get("GLOWK_BUILD") or "unknown", mfma_peak_flop_per_s=MFMA_PEAK)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for name, shape in SHAPES:
        nsig, rows, T = shape
        fc = T // 2 + 1
        S = (torch.randn(shape, device="cuda", generator=gen) ** 2).contiguous()
        spec = torch.empty((nsig, rows, fc), dtype=torch.complex64, device="cuda")
        mag, mask, out = torch.empty_like(S), torch.empty_like(S), torch.empty_like(S)
        std = torch.empty((nsig, 2), dtype=torch.float64, device="cuda")
        nb_dft, nb_std, nb_pk = lib.glowk_dft2_workspace_bytes(nsig, rows, T), lib.glowk_plane_std_workspace_bytes(nsig, rows * T), \
            lib.glowk_peak_workspace_bytes(nsig, rows, T)
        work = torch.empty(max(nb_dft, nb_std, nb_pk) // 8 + 1, dtype=torch.float64, device="cuda")

        def fwd():
            _lib.check(lib.glowk_rdft2(p(S), nsig, rows, T, p(spec), p(mag), p(work), nb_dft, stream))

        def sd():
            _lib.check(lib.glowk_plane_std(p(mag), nsig, rows * T, p(std), p(work), nb_std, stream))

        entry = dict(shape=list(shape), workspace_bytes=nb_dft)
        entry["rdft2_with_mag"] = timed(fwd, args.reps)
        entry["plane_std"] = timed(sd, args.reps)
        thr = std[:, 1].to(torch.float32).contiguous()

        def pk():
            _lib.check(lib.glowk_peak_mask(p(mag), nsig, rows, T, 1, 25, p(thr), p(mask), None, None, p(work), nb_pk, stream))

        def inv():
            _lib.check(lib.glowk_irdft2(p(spec), p(mask), nsig, rows, T, p(out), p(work), nb_dft, stream))

        entry["peak_mask_1x25"] = timed(pk, args.reps)
        entry["peaks"] = int(mask.sum().item())
        entry["irdft2_masked"] = timed(inv, args.reps)
        entry["ft2d_whole"] = timed(lambda: ft2d.ft2d(S), args.reps)
        kf, ki = kernel_ms(fwd), kernel_ms(inv)
        first = lambda d, k: d[k][0] if d.get(k) else None                             # noqa: E731
        f_frames, f_rows = 4.0 * nsig * rows * fc * T, 8.0 * nsig * rows * rows * fc
        entry["stages"] = dict(forward_frames=stage(first(kf, "k_rdft_frames"), f_frames), forward_rows=stage(first(kf, "k_cdft_rows"), f_rows),
                               inverse_rows=stage(first(ki, "k_cdft_rows"), f_rows), inverse_frames=stage(first(ki, "k_irdft_frames"), f_frames))
        both = [entry["stages"][k] for k in ("forward_frames", "forward_rows")]
        entry["forward_gemm_stages_ms"] = None if None in both else both[0]["ms"] + both[1]["ms"]
        if not args.no_cpu:
            from scipy import ndimage
            host = S[0].cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            F = np.fft.rfft2(host)
            t1 = time.perf_counter()
            full = np.abs(np.fft.fft2(host))
            thr64 = full.std()
            t2 = time.perf_counter()
            mx, mn = ndimage.maximum_filter(full, size=(1, 25), mode="wrap"), ndimage.minimum_filter(full, size=(1, 25), mode="wrap")
            M = (full == mx) & ((mx - mn) > thr64)
            t3 = time.perf_counter()
            np.fft.irfft2(F * M[:, :fc], s=(rows, T))
            t4 = time.perf_counter()
            entry["numpy_s"] = dict(signals=1, rfft2=t1 - t0, magnitude_and_std=t2 - t1, peak_mask=t3 - t2, irfft2=t4 - t3, whole=t4 - t0)
        res[name] = entry
    res["note"] = ("HIP events around each C call on preallocated device tensors, median of reps after one warm-up call; stages: kernel "
                   "durations of one profiled call; numpy_s: the fp64 restatement of ONE signal of the shape on the host")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
