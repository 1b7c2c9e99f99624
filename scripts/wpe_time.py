"""Times of the WPE kernels (csrc/glowk_wpe.h) on one GPU at 180 s of 16 kHz audio, beside the fp64 numpy restatement on the host.

Shapes 1 x 2 x 1025 x 5626 with K = 10, delay = 3 and 1 x 4 x 1025 x 5626 with K = 16 (D = 64).  HIP events around each C call on
preallocated device tensors, median, minimum and spread of --reps runs after a warm-up:

* ``power`` / ``correlations`` / ``solve`` / ``filter``: the four staged entries;
* ``iteration``: ``glowk_wpe_fit`` with --iters iterations, per iteration;
* ``correlations.flop``: what the matrix cores execute (the tile pairs of one triangle, four 16 x 16 x 4 products per pair and four
  frames), ``of_peak`` against 78.6 Tflop/s, the fp64 matrix peak;
* ``numpy``: one iteration of the restatement with BLAS products (tests/wpe_ref.py's steps, correlations in plain fp64) on --host-rows
  rows, scaled to all the rows.

    python scripts/wpe_time.py --out profiles/wpe_time.json [--reps 10] [--iters 3] [--host-rows 32]
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
from audiosourcesep_amd import _lib  # noqa: E402

ROWS, FRAMES = 1025, 5626
CASES = ((2, 10, 3), (4, 16, 3))
PEAK_FP64_MATRIX = 78.6e12


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


def scene(M, seed=0):
    """A reverberant-looking complex64 STFT [1, M, ROWS, FRAMES]: Gaussian cells under a slow envelope, smeared over later frames."""
    rng = np.random.default_rng(seed)
    t = np.arange(FRAMES)
    env = np.exp(1.2 * np.sin(2 * np.pi * (t / 29.0 + rng.uniform(size=(1, M, ROWS, 1))))).astype(np.float32)
    s = env * (rng.standard_normal((1, M, ROWS, FRAMES), np.float32) + 1j * rng.standard_normal((1, M, ROWS, FRAMES), np.float32))
    x = s.copy()
    for lag, g in ((1, 0.5), (2, 0.35 + 0.2j), (4, -0.25j), (7, 0.15)):
        x[..., lag:] += np.complex64(g) * s[..., :FRAMES - lag]
    return x.astype(np.complex64)


def host_iteration(X, K, delay, rows):
    """One iteration of the restatement on the first ``rows`` rows with BLAS products; seconds."""
    from tests import wpe_ref as W
    t0 = time.perf_counter()
    for r in range(rows):
        x = W.c128(X[0, :, r])
        w, _, _ = W.inv_power(x)
        xt = W.stacked(x, K, delay)
        R, P = (xt * w) @ xt.conj().T, (xt * w) @ x.conj().T
        G, _, _ = W.solve(R, P)
        (x - G.conj().T @ xt).astype(np.complex64)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wpe_time.py measures on a GPU; none is visible")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = dict(device=torch.cuda.get_device_name(0), build=os.environ.get("GLOWK_BUILD") or "unknown", iterations_per_call=args.iters)
    for M, K, delay in CASES:
        D = M * K
        Xh = scene(M)
        X = torch.from_numpy(Xh).cuda()
        Y = torch.empty_like(X)
        w = torch.empty((1, ROWS, FRAMES), dtype=torch.float64, device="cuda")
        Rm = torch.empty((1, ROWS, D, D), dtype=torch.complex128, device="cuda")
        P = torch.empty((1, ROWS, D, M), dtype=torch.complex128, device="cuda")
        G = torch.empty((1, ROWS, D, M), dtype=torch.complex128, device="cuda")
        status = torch.empty((1, ROWS), dtype=torch.int32, device="cuda")
        nbytes = lib.glowk_wpe_workspace_bytes(1, M, K, ROWS, FRAMES)
        work = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
        e = dict(shape=[1, M, ROWS, FRAMES], taps=K, delay=delay, D=D, workspace_bytes=nbytes)
        e["power"] = timed(lambda: _lib.check(lib.glowk_wpe_power(p(X), 1, M, ROWS, FRAMES, 0, 1e-10, p(w), p(None), stream)), args.reps)
        e["correlations"] = timed(lambda: _lib.check(lib.glowk_wpe_correlations(p(X), p(w), 1, M, ROWS, FRAMES, K, delay, p(Rm), p(P), stream)), args.reps)
        e["solve"] = timed(lambda: _lib.check(lib.glowk_wpe_solve(p(Rm), p(P), 1, ROWS, D, M, 1e-10, p(G), p(status), stream)), args.reps)
        e["filter"] = timed(lambda: _lib.check(lib.glowk_wpe_filter(p(X), p(G), 1, M, ROWS, FRAMES, K, delay, p(Y), stream)), args.reps)
        e["iteration"] = timed(lambda: _lib.check(lib.glowk_wpe_fit(p(X), 1, M, ROWS, FRAMES, K, delay, args.iters, 0, 1e-10, 1e-10, p(Y), p(G), p(status), p(work),
                                                                    nbytes, stream)), args.reps, args.iters)
        rt, ct = -(-D // 16), -(-(D + M) // 16)
        pairs = sum(ct - i for i in range(rt))
        flop = float(ROWS) * pairs * 4 * -(-FRAMES // 4) * (2 * 16 * 16 * 4)
        e["correlations"].update(tile_pairs=pairs, flop=flop, tflops=flop / (e["correlations"]["median_ms"] * 1e-3) / 1e12,
                                 of_peak=flop / (e["correlations"]["median_ms"] * 1e-3) / PEAK_FP64_MATRIX)
        e["flagged_rows"] = int(status.ne(0).sum())
        sec = host_iteration(Xh, K, delay, args.host_rows)
        e["numpy"] = dict(rows_timed=args.host_rows, seconds=sec, iteration_s_scaled_to_all_rows=sec * ROWS / args.host_rows,
                          threads=os.cpu_count())
        e["numpy_over_device"] = e["numpy"]["iteration_s_scaled_to_all_rows"] / (e["iteration"]["median_ms"] * 1e-3)
        res["M%d_K%d" % (M, K)] = e
    res["note"] = ("HIP events around each C call on preallocated device tensors, median of reps after one warm-up call; iteration: glowk_wpe_fit, per "
                   "iteration; flop: what the matrix cores execute; of_peak: against 78.6 Tflop/s; numpy: one iteration of the fp64 restatement with "
                   "BLAS products on rows_timed rows, scaled to 1025")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
