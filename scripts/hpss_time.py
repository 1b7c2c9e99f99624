"""Times of the HPSS kernels (csrc/glowk_hpss.h) on one GPU and the largest mask error against the fp64 restatement.

Timing: ``glowk_median_filter`` along the frames and along the rows, and ``glowk_hpss_mask``, on |STFT|-shaped float32 data at
1025 x 5626 (180 s of 16 kHz audio) for sizes 31 and 127, and at the 30-extract shape 30 x 1025 x 64 for size 31.  HIP events
around each call on preallocated device tensors, median, minimum and spread of --reps runs after a warm-up.  ``hbm_floor_ms`` is
one read plus one write of the array (the mask with s: three reads, two writes) at the 8 TB/s peak; ``fraction_of_hbm_floor`` is the floor
over the median.  ``compares`` is size^2 per output, what rank counting performs at the most.  With scipy on the host,
``scipy_s`` is ``scipy.ndimage.median_filter`` on the same array, as context.

Accuracy (--accuracy-out): the device masks against tests/hpss_ref.py's fp64 ``masks`` of the device's own medians, for power in
{0.5, 1, 2, 10} and margins (1, 1), (2.5, 1), (1, 3), on continuous random spectra [1025, 256].

    python scripts/hpss_time.py --out profiles/hpss_time.json --accuracy-out profiles/hpss_accuracy.json [--reps 20] [--no-cpu]
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
from audiosourcesep_amd import _lib, hpss  # noqa: E402

HBM_PEAK = 8.0e12                          # bytes / s
SHAPES = [("180s", (1, 1025, 5626), (31, 127)), ("30_extracts", (30, 1025, 64), (31,))]


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


def with_floor(r, nbytes):
    floor_ms = nbytes / HBM_PEAK * 1e3
    r.update(bytes=nbytes, hbm_floor_ms=floor_ms, fraction_of_hbm_floor=floor_ms / r["median_ms"])
    return r


def accuracy():
    from tests import hpss_ref as R
    rng = np.random.default_rng(5)
    S = (np.abs(rng.standard_normal((1025, 256))) ** 3).astype(np.float32)
    harm, perc = hpss.median_filter(S, 31, 0).cpu().numpy(), hpss.median_filter(S, 31, 1).cpu().numpy()
    out = dict(shape=list(S.shape), kernel_size=31, bar=1e-6, cases=[])
    for power in (0.5, 1.0, 2.0, 10.0):
        for margin in ((1.0, 1.0), (2.5, 1.0), (1.0, 3.0)):
            got = hpss.hpss(S, kernel_size=31, power=power, mask=True, margin=margin)
            want = R.masks(harm, perc, power, margin)
            err = max(float(np.abs(g.cpu().numpy() - w).max()) for g, w in zip(got, want))
            out["cases"].append(dict(power=power, margin=list(margin), max_abs_error=err))
    out["max_abs_error"] = max(c["max_abs_error"] for c in out["cases"])
    out["note"] = "device masks (fp32) against the fp64 restatement of tests/hpss_ref.py fed the device's own medians"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--accuracy-out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="leave out scipy's time on the host")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hpss_time.py measures on a GPU; none is visible")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = dict(device=torch.cuda.get_device_name(0), build=os.environ.get("GLOWK_BUILD") or "unknown", hbm_peak_bytes_per_s=HBM_PEAK)
    ndimage = None
    if not args.no_cpu:
        try:
            from scipy import ndimage
        except ImportError:
            pass
    gen = torch.Generator(device="cuda").manual_seed(1)
    for name, shape, sizes in SHAPES:
        S = torch.randn(shape, device="cuda", generator=gen).abs().contiguous()
        out, out2 = torch.empty_like(S), torch.empty_like(S)
        nsig, rows, F = shape
        entry = dict(shape=list(shape))
        for size in sizes:
            for axis, label in ((0, "frames"), (1, "rows")):
                def call():
                    _lib.check(lib.glowk_median_filter(p(S), nsig, rows, F, size, axis, p(out), stream))
                r = with_floor(timed(call, args.reps), 2 * 4 * S.numel())
                r["compares"] = S.numel() * size * size
                if ndimage is not None:
                    host = S.cpu().numpy()
                    t0 = time.perf_counter()
                    want = ndimage.median_filter(host, size=(1, 1, size) if axis == 0 else (1, size, 1), mode="reflect")
                    r["scipy_s"] = time.perf_counter() - t0
                    r["equals_scipy_bitwise"] = bool(np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)))
                entry["median_%s_size%d" % (label, size)] = r
        harm, perc = out.clone(), S

        def mask():
            _lib.check(lib.glowk_hpss_mask(p(harm), p(perc), p(S), S.numel(), 2.0, 1.0, 1.0, p(out), p(out2), stream))
        entry["mask_power2"] = with_floor(timed(mask, args.reps), 5 * 4 * S.numel())
        res[name] = entry
    res["note"] = ("HIP events around each C call on preallocated device tensors, median of reps after one warm-up call; hbm_floor_ms: one read "
                   "and one write of the array per filter (three reads and two writes for the mask with s) at hbm_peak_bytes_per_s; the filters "
                   "are bound by the size^2 rank-counting compares, not by memory")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.accuracy_out:
        acc = accuracy()
        print(json.dumps(acc, indent=1))
        with open(args.accuracy_out, "w") as f:
            f.write(json.dumps(acc, indent=1) + "\n")


if __name__ == "__main__":
    main()
