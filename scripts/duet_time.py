"""Times of the DUET kernels (csrc/glowk_duet.h) on one GPU.

One stereo STFT of 2 x 1025 x 5626 (180 s of 16 kHz audio), four sources, the default 50 x 50 bins over [-3, 3) x [-3, 3), on two
inputs: ``crafted`` (four panned complex Gaussian sources, each active in 35 % of the cells: the weight piles onto four cells and
their neighbours, as DUET's data does by design) and ``one_cell`` (X2 = X1: every counted cell adds to the same bin, the most
contention the histogram can meet).  HIP events around each C call on preallocated device tensors: median, minimum and spread of
--reps runs after a warm-up.  ``bytes`` is what the stage must move (each pass over X reads 16 B per cell; the assignment also writes
20 B per cell and source) and ``gb_per_s`` that over the median.  The two passes of the fused histogram and the two launches of the
assignment run inside one C call each; their own durations come from the kernel records of one profiled call (torch.profiler; null
where it gives none).  ``numpy_s`` is the host's time for the fp64 restatement (tests/duet_ref.py) of the same array.

    python scripts/duet_time.py --out profiles/duet_time.json [--reps 20] [--no-cpu]
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
from audiosourcesep_amd import _lib, duet  # noqa: E402
from tests import duet_ref as D  # noqa: E402

ROWS, FRAMES, SOURCES = 1025, 5626, 4
GRID = D.DEFAULT_GRID
CELLS_A, CELLS_D = (10, 20, 30, 40), (20, 25, 30, 27)
KERNELS = ("k_duet_wmax", "k_duet_hist", "k_duet_table", "k_duet_assign")


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


def with_bytes(t, nbytes):
    return dict(t, bytes=int(nbytes), gb_per_s=nbytes / (t["median_ms"] * 1e-3) / 1e9)


def kernel_ms(call):
    """{kernel name: duration in ms of its first launch} of one call, or {} where the profiler records no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        call()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        out = {}
        for ev in sorted(prof.events(), key=lambda e: e.time_range.start):
            for name in KERNELS:
                if name in ev.name and name not in out:
                    out[name] = (ev.time_range.end - ev.time_range.start) / 1e3
        return out
    except Exception as e:                  # the timings above do not depend on it
        print("kernel records unavailable: %r" % (e,), file=sys.stderr)
        return {}


def crafted(gen):
    """[2, ROWS, FRAMES] complex64 on the GPU: SOURCES panned sources as tests/duet_ref.crafted makes them, drawn on the device."""
    _, de, a = D.centres(np.stack([CELLS_A, CELLS_D], 1), GRID)
    om = torch.from_numpy(D.omega(ROWS)).cuda()[:, None]
    X = torch.zeros((2, ROWS, FRAMES), dtype=torch.complex128, device="cuda")
    for j in range(SOURCES):
        s = torch.complex(torch.randn((ROWS, FRAMES), device="cuda", generator=gen, dtype=torch.float64),
                          torch.randn((ROWS, FRAMES), device="cuda", generator=gen, dtype=torch.float64))
        s = s * (torch.rand((ROWS, FRAMES), device="cuda", generator=gen) < 0.35)
        X[0] += s
        X[1] += float(a[j]) * torch.exp(-1j * float(de[j]) * om) * s
    return X.to(torch.complex64).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="leave out the host's time for the numpy restatement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("duet_time.py measures on a GPU; none is visible")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = dict(device=torch.cuda.get_device_name(0), build=os.environ.get("GLOWK_BUILD") or "unknown", shape=[2, ROWS, FRAMES], sources=SOURCES,
               bins=[GRID[2], GRID[5]])
    gen = torch.Generator(device="cuda").manual_seed(1)
    cells = ROWS * FRAMES
    first = crafted(gen)
    inputs = [("crafted", first), ("one_cell", torch.stack([first[0], first[0]]).contiguous())]
    fa, fd, fw = (torch.empty((ROWS, FRAMES), dtype=torch.float64, device="cuda") for _ in range(3))
    hist = torch.empty((GRID[2], GRID[5]), dtype=torch.int64, device="cuda")
    hist2 = torch.empty_like(hist)
    es = torch.empty(2, dtype=torch.int32, device="cuda")
    peaks = torch.empty((SOURCES, 2), dtype=torch.int32, device="cuda")
    found = torch.empty((), dtype=torch.int32, device="cuda")
    masks = torch.empty((SOURCES, ROWS, FRAMES), dtype=torch.float32, device="cuda")
    spec = torch.empty((SOURCES, 2, ROWS, FRAMES), dtype=torch.complex64, device="cuda")
    nb_h, nb_p, nb_a = lib.glowk_duet_hist_workspace_bytes(1, cells, GRID[2], GRID[5]), lib.glowk_duet_peaks_workspace_bytes(1, GRID[2], GRID[5]), \
        lib.glowk_duet_assign_workspace_bytes(1, ROWS, SOURCES)
    work = torch.empty(max(nb_h, nb_p, nb_a) // 8 + 2, dtype=torch.float64, device="cuda")
    for name, X in inputs:
        def feat():
            _lib.check(lib.glowk_duet_features(p(X), 1, ROWS, FRAMES, 1.0, 0.0, p(fa), p(fd), p(fw), stream))

        def fused():
            _lib.check(lib.glowk_duet_histogram_stft(p(X), 1, ROWS, FRAMES, 1.0, 0.0, *GRID, 1, p(hist), p(es), p(work), nb_h, stream))

        def staged():
            _lib.check(lib.glowk_duet_histogram(p(fa), p(fd), p(fw), 1, cells, *GRID, 1, p(hist2), p(es), p(work), nb_h, stream))

        def pk():
            _lib.check(lib.glowk_duet_peaks(p(hist), 1, GRID[2], GRID[5], 1, SOURCES, 5, 5, None, p(peaks), p(found), p(work), nb_p, stream))

        def asg():
            _lib.check(lib.glowk_duet_assign(p(X), 1, ROWS, FRAMES, p(peaks), p(found), SOURCES, *GRID, p(masks), p(spec), p(work), nb_a, stream))

        entry = dict(workspace_bytes=dict(histogram=nb_h, peaks=nb_p, assign=nb_a))
        entry["features"] = with_bytes(timed(feat, args.reps), cells * (16 + 24))
        entry["histogram_fused"] = with_bytes(timed(fused, args.reps), 2 * cells * 16)
        entry["histogram_staged"] = with_bytes(timed(staged, args.reps), 2 * cells * 24)
        entry["fused_equals_staged"] = bool(torch.equal(hist, hist2))
        entry["peaks"] = timed(pk, args.reps)
        entry["n_found"], entry["found_cells"] = int(found.item()), peaks.tolist()
        entry["largest_bin_share"] = float(hist.max().item() / max(hist.sum().item(), 1))
        entry["assign"] = with_bytes(timed(asg, args.reps), cells * (16 + 20 * SOURCES))
        entry["duet_whole"] = timed(lambda: duet.duet(X, SOURCES), args.reps)
        kh, ka = kernel_ms(fused), kernel_ms(asg)
        entry["kernels"] = {k: (None if v is None else dict(ms=v, gb_per_s=b / (v * 1e-3) / 1e9 if b else None)) for k, v, b in (
            ("k_duet_wmax", kh.get("k_duet_wmax"), cells * 16), ("k_duet_hist", kh.get("k_duet_hist"), cells * 16),
            ("k_duet_table", ka.get("k_duet_table"), 0), ("k_duet_assign", ka.get("k_duet_assign"), cells * (16 + 20 * SOURCES)))}
        if not args.no_cpu:
            host = X.cpu().numpy()
            t0 = time.perf_counter()
            alpha, delta, w = D.features(host)
            t1 = time.perf_counter()
            plane, _, _ = D.histogram_int(alpha, delta, w, GRID, 1)
            t2 = time.perf_counter()
            rp, rf, _ = D.find_peaks(plane, SOURCES, 1, (5, 5))
            t3 = time.perf_counter()
            D.assign(host, rp, rf, GRID)
            t4 = time.perf_counter()
            entry["numpy_s"] = dict(features=t1 - t0, histogram=t2 - t1, peaks=t3 - t2, assign=t4 - t3, whole=t4 - t0)
            entry["peaks_equal_numpy"] = bool(rf == entry["n_found"] and rp.tolist() == entry["found_cells"])
        res[name] = entry
    res["note"] = ("HIP events around each C call on preallocated device tensors, median of reps after one warm-up call; kernels: durations "
                   "of one profiled call; bytes: what the stage must move; numpy_s: the fp64 restatement of the same array on the host")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
