"""Times of the melody kernels (csrc/glowk_melody.h) on one GPU.

One spectrogram of 1 x 1025 x 5626 (180 s of 16 kHz audio) on the default grid of 300 fundamentals: a gliding ten-harmonic lead over
noise, built on the device.  HIP events around each C call on preallocated device tensors: median, minimum and spread of --reps runs
after a warm-up.  ``bytes`` is what a stage must move and ``gb_per_s`` that over the median, next to ``copy_gb_per_s``, the copy rate an
MI355X reaches from HBM; the spectrogram (23 MB) fits the 256 MiB Infinity Cache, so a pass may read faster than that.  ``track`` also
reports what the kernel's own stamps of the constant 100 MHz clock say of its two phases: the recursion (one barrier per frame) and
the back-trace.  ``numpy_s`` is the host's time for the fp64 restatement (tests/melody_ref.py) of each stage on the same arrays.

    python scripts/melody_time.py --out profiles/melody_time.json [--reps 20] [--no-cpu]
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
from audiosourcesep_amd import _lib, melody  # noqa: E402
from tests import melody_ref as M  # noqa: E402

ROWS, FRAMES, H, J, HM = 1025, 5626, 8, 12, 20
COPY_GB_PER_S = 6300.0
TICK_HZ = 100e6


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
    return dict(t, bytes=int(nbytes), gb_per_s=nbytes / (t["median_ms"] * 1e-3) / 1e9, copy_gb_per_s=COPY_GB_PER_S)


def scene(gen):
    """[ROWS, FRAMES] float32 on the GPU: ten harmonics of a slow glide from 220 to 440 Hz with vibrato, three rows wide, over noise."""
    t = torch.arange(FRAMES, device="cuda", dtype=torch.float64)
    f0 = 220.0 * 2.0 ** (t / FRAMES) * (1.0 + 0.01 * torch.sin(2 * np.pi * t / 6.0))
    rows = torch.arange(ROWS, device="cuda", dtype=torch.float64)[:, None] * M.BIN_HZ
    S = 0.02 * torch.rand((ROWS, FRAMES), device="cuda", generator=gen, dtype=torch.float64)
    for h in range(1, 11):
        S += torch.exp(-0.5 * ((rows - h * f0[None, :]) / 10.0) ** 2) / h
    S[:, FRAMES // 2:FRAMES // 2 + 400] *= 0.02                                          # a rest: the track has to leave and come back
    return S.to(torch.float32).contiguous(), f0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="leave out the host's time for the numpy restatement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("melody_time.py measures on a GPU; none is visible")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    grid, w, pen = melody.f0_grid(), M.weights(H, 0.8), M.penalties(0.02, J)
    B = grid.shape[0]
    res = dict(device=torch.cuda.get_device_name(0), build=os.environ.get("GLOWK_BUILD") or "unknown", shape=[1, ROWS, FRAMES], bins=B, harmonics=H,
               max_jump=J)
    S, f0_true = scene(torch.Generator(device="cuda").manual_seed(1))
    dev = S.device
    idx, frac = melody._positions(lib, grid, H, M.BIN_HZ, ROWS, dev)
    wd, gd, pd = (torch.as_tensor(a, dtype=torch.float64).to(dev) for a in (w, grid, pen))
    sal = torch.empty((B, FRAMES), dtype=torch.float32, device=dev)
    e = torch.empty((B, FRAMES), dtype=torch.float64, device=dev)
    peak = torch.empty(1, dtype=torch.float32, device=dev)
    path = torch.empty(FRAMES, dtype=torch.int32, device=dev)
    ticks = torch.zeros(2, dtype=torch.int64, device=dev)
    mask = torch.empty_like(S)
    nb = lib.glowk_melody_workspace_bytes(1, B, FRAMES)
    work = torch.empty(nb // 8 + 2, dtype=torch.float64, device=dev)
    theta, nu, width = 0.2, 0.5, 40.0

    def salience():
        _lib.check(lib.glowk_melody_salience(p(S), 1, ROWS, FRAMES, p(idx), p(frac), p(wd), B, H, p(sal), stream))

    def emission():
        _lib.check(lib.glowk_melody_emission(p(sal), 1, B, FRAMES, p(e), p(peak), p(work), nb, stream))

    def track(stamps=None):
        _lib.check(lib.glowk_melody_track(p(e), 1, B, FRAMES, p(pd), J, theta, nu, p(path), p(stamps), p(work), nb, stream))

    def comb():
        _lib.check(lib.glowk_melody_mask(p(path), 1, FRAMES, p(gd), B, ROWS, HM, width, M.BIN_HZ, p(mask), stream))

    def fit():
        _lib.check(lib.glowk_melody_fit(p(S), 1, ROWS, FRAMES, p(idx), p(frac), p(wd), p(gd), B, H, p(pd), J, theta, nu, HM, width, M.BIN_HZ, p(path), p(mask),
                                        p(peak), p(work), nb, stream))

    cells, plane = ROWS * FRAMES, B * FRAMES
    res["salience"] = with_bytes(timed(salience, args.reps), cells * 4 + plane * 4)
    res["salience"]["lds_reads"] = 2 * H * plane
    res["emission"] = with_bytes(timed(emission, args.reps), 2 * plane * 4 + plane * 8)
    res["track"] = with_bytes(timed(track, args.reps), plane * 8 + 2 * FRAMES * (B + 1) * 2)
    track(ticks)
    torch.cuda.synchronize()
    rec, back = (float(v) / TICK_HZ * 1e3 for v in ticks.tolist())
    res["track"].update(recursion_ms=rec, back_trace_ms=back, us_per_frame=rec * 1e3 / (FRAMES - 1),
                        stamps="the kernel's own stamps of the constant 100 MHz clock around its two phases, one run")
    res["mask"] = with_bytes(timed(comb, args.reps), cells * 4)
    res["fit"] = timed(fit, args.reps)
    res["fit"]["sum_of_stages_ms"] = sum(res[k]["median_ms"] for k in ("salience", "emission", "track", "mask"))
    whole = timed(lambda: melody.melody(S), max(3, args.reps // 4))
    res["melody_python"] = dict(whole, note="melody(S) with its table uploads, allocations, the first estimates and glowk_hpss_mask")
    f0_hat = np.concatenate([grid, [0.0]])[path.cpu().numpy()]
    truth = f0_true.cpu().numpy()
    voiced = f0_hat > 0
    res["frames_voiced"] = int(voiced.sum())
    res["frames_within_50_cents"] = int((1200 * np.abs(np.log2(f0_hat[voiced] / truth[voiced])) <= 50).sum())
    if not args.no_cpu:
        host = S.cpu().numpy()
        t = [time.perf_counter()]
        hs = M.salience(host, grid, w)
        t.append(time.perf_counter())
        he, _ = M.emission(hs)
        t.append(time.perf_counter())
        hp = M.track(he, theta, 0.02, nu, J)
        t.append(time.perf_counter())
        M.harmonic_mask(hp, grid, ROWS, HM, width)
        t.append(time.perf_counter())
        res["numpy_s"] = dict(zip(("salience", "emission", "track", "mask"), np.diff(t).tolist()), total=t[-1] - t[0])
        res["path_equals_numpy_fed_the_device_emission"] = bool(np.array_equal(M.track(e.cpu().numpy(), theta, 0.02, nu, J), path.cpu().numpy()))
    res["note"] = ("HIP events around each C call on preallocated device tensors, median of reps after one warm-up call; bytes: what the stage must "
                   "move; numpy_s: the fp64 restatement of the same arrays on the host, once")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
