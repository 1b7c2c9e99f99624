"""Times of the NMF kernels (csrc/glowk_nmf.h) on one GPU at 180 s of 16 kHz audio.

Shape 1 x 1025 x 5626, |N(0, 1)|^2 with about 5 % silent frames (tests/nmf_ref.py's inputs), K = 32, 64 and 128, beta = 0, 1, 2.
HIP events around each C call on preallocated device tensors, median, minimum and spread of --reps runs after a warm-up; one call
runs --iters iterations, the times are per iteration:

* ``iteration``: ``glowk_nmf_fit(update_w = 1)``, the W update and then the H update (three launches);
* ``h_update`` / ``w_update``: ``update_w = 0`` and ``2``.  One update is 6 rows frames K FLOP -- Lambda, and the numerator and the
  denominator chain, 2 rows frames K each -- against the fp32-MFMA peak of DESIGN.md (the MFMAs issued cover K padded to a multiple
  of 32; the fraction counts K);
* ``kernels``: device times of one call from torch.profiler, per iteration, where that is available;
* ``divergence`` and ``masks`` (two sources of K / 2 components, a one-channel complex spectrum, power 1) at each K.

``host``: the time of one iteration of the fp64 numpy restatement (tests/nmf_ref.py) at the same shape, and the device's largest
deviation from it after one update fed the same inputs, in units of the tests' bar.

    python scripts/nmf_time.py --out profiles/nmf_time.json [--reps 10] [--iters 10] [--no-cpu]
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
from audiosourcesep_amd import _lib, nmf  # noqa: E402

FP32_MFMA_PEAK = 157.3e12                  # FLOP / s
ROWS, FRAMES = 1025, 5626
KERNELS = ("k_nmf_update_h", "k_nmf_update_w", "k_nmf_w_finish", "k_nmf_divergence", "k_nmf_div_reduce", "k_nmf_masks")


def timed(call, reps, per=1):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / per)
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), spread_ms=float(np.max(ms) - np.min(ms)), reps=reps)


def kernel_times(call, per=1):
    """{kernel name: ms per iteration} of one run of ``call`` from torch.profiler's device events."""
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
                out[short] = out.get(short, 0.0) + float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0)) / 1e3 / per
    if not out:
        raise RuntimeError("the profiler reported none of the kernels")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true", help="leave out the restatement's time on the host")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nmf_time.py measures on a GPU; none is visible")
    from tests import nmf_ref as N
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Vh = N.spectra((ROWS, FRAMES), 1)
    V = torch.from_numpy(Vh).cuda()
    res = dict(device=torch.cuda.get_device_name(0), build=os.environ.get("GLOWK_BUILD") or "unknown", fp32_mfma_peak_flops=FP32_MFMA_PEAK,
               shape=[1, ROWS, FRAMES], iterations_per_call=args.iters, update_flop_per_K=6.0 * ROWS * FRAMES)
    for K in (32, 64, 128):
        W0, H0 = nmf.init(V, K, seed=0)
        nbytes = lib.glowk_nmf_workspace_bytes(1, ROWS, FRAMES, K)
        work = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
        flop = 6.0 * ROWS * FRAMES * K
        entry = dict(workspace_bytes=nbytes)
        for beta in (0, 1, 2):
            Vb = V.clamp_min(1e-3) if beta == 0 else V
            W, H = W0.clone(), H0.clone()

            def fit(mode, n=args.iters):
                _lib.check(lib.glowk_nmf_fit(p(Vb), 1, ROWS, FRAMES, p(W), 1, p(H), K, beta, n, mode, p(work), nbytes, stream))
            b = {}
            for name, mode, updates in (("iteration", 1, 2), ("h_update", 0, 1), ("w_update", 2, 1)):
                W.copy_(W0)
                H.copy_(H0)
                t = timed(lambda: fit(mode), args.reps, args.iters)
                t["fraction_of_fp32_mfma_peak"] = updates * flop / (t["median_ms"] * 1e-3) / FP32_MFMA_PEAK
                b[name] = t
            try:
                b["kernels"] = kernel_times(lambda: fit(1), args.iters)
                for kn, upd in (("k_nmf_update_h", "h"), ("k_nmf_update_w", "w")):
                    if kn in b["kernels"]:
                        b["kernel_fraction_of_peak_" + upd] = flop / (b["kernels"][kn] * 1e-3) / FP32_MFMA_PEAK
            except Exception as e:  # noqa: BLE001  (a machine without the profiler still gets the entry times)
                b["kernels_error"] = "%s: %s" % (type(e).__name__, e)
            out = torch.empty((1,), dtype=torch.float64, device="cuda")
            b["divergence"] = timed(lambda: _lib.check(lib.glowk_nmf_divergence(p(Vb), 1, ROWS, FRAMES, p(W), 1, p(H), K, beta, p(out), p(work), nbytes,
                                                                                stream)), args.reps)
            b["divergence"]["value_after_timing"] = float(out.item())
            if not args.no_cpu:
                W.copy_(W0)
                H.copy_(H0)
                vh, wh, hh = Vb.cpu().numpy(), W0.cpu().numpy(), H0.cpu().numpy()
                t0 = time.perf_counter()
                rw = N.update_w(vh, wh, hh, beta)
                rh = N.update_h(vh, rw, hh, beta)
                t1 = time.perf_counter()
                fit(2, 1)
                dw = W.cpu().numpy().astype(np.float64)
                W.copy_(W0)
                fit(0, 1)
                dh = H.cpu().numpy().astype(np.float64)
                rh0 = N.update_h(vh, wh, hh, beta)
                b["host"] = dict(fp64_iteration_s=t1 - t0, divergence_after_one_iteration=float(N.divergence(vh, rw, rh, beta)),
                                 worst_over_bar_w=N.ratio(np.abs(dw - rw), N.update_bar(K, FRAMES) * rw),
                                 worst_over_bar_h=N.ratio(np.abs(dh - rh0), N.update_bar(K, ROWS) * rh0))
            entry["beta%d" % beta] = b
        bounds = (ctypes.c_int32 * 3)(0, K // 2, K)
        X = torch.polar(V, torch.rand_like(V) * 6.2831853).contiguous()
        m = torch.empty((2, ROWS, FRAMES), device="cuda")
        spec = torch.empty((2, 1, ROWS, FRAMES), dtype=torch.complex64, device="cuda")
        entry["masks"] = timed(lambda: _lib.check(lib.glowk_nmf_masks(p(W0), 1, p(H0), 1, ROWS, FRAMES, K, bounds, 2, 1, p(X), 1, p(m), p(spec), stream)),
                               args.reps)
        entry["masks"]["bytes_moved"] = int(V.numel() * (8 + 2 * 4 + 2 * 8))
        entry["masks"]["bytes_per_s"] = entry["masks"]["bytes_moved"] / (entry["masks"]["median_ms"] * 1e-3)
        res["K%d" % K] = entry
    res["note"] = ("HIP events around each C call on preallocated device tensors, median of reps after one warm-up call, divided by the "
                   "iterations of a call; kernels: device times of one call from torch.profiler per iteration; fraction_of_fp32_mfma_peak: "
                   "6 rows frames K FLOP per update over the time against fp32_mfma_peak_flops; host: fp64 numpy on the same input")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
