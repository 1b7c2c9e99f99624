"""Times of the REPET-SIM kernels (csrc/glowk_repet.h) on one GPU at 180 s of 16 kHz audio.

Shape 1 x 1025 x 5626, width = 62 frames (2 s), k = default_k = 150.  Two inputs: ``audio``, the |STFT| (``audio.mel_frames``) of
tests/repet_ref.py's repeated phrase and chirp with a little noise, and ``random``, |N(0, 1)|^2 -- the number of list insertions
of the selection depends on the data, nothing else does.

Per entry: HIP events around ``glowk_nn_neighbors`` (k_nn_norms + k_nn_topk) and ``glowk_nn_median`` (k_nn_transpose +
k_nn_median) and ``glowk_hpss_mask`` on preallocated device tensors, median, minimum and spread of --reps runs after a warm-up;
``nn_neighbors_k1`` is ``glowk_nn_neighbors`` with k = 1, where the lists cost next to nothing: the Gram loop and the scaling alone.
Per kernel: the device times torch.profiler reports for one more run of the two entries (``kernels``; ``kernels_error`` where the
profiler is unavailable).  ``gram``: 2 rows frames^2 FLOP (every product of the Gram matrix, the band included, as the kernel
computes them) over k_nn_topk's time -- the selection runs inside it -- as a fraction of the fp32-MFMA peak of DESIGN.md; without
per-kernel times the whole entry's time stands in and the figure is a lower bound.  ``host``: the fp64 restatement of
tests/repet_ref.py (similarity + selection, then gather + median) on the ``audio`` input, and whether the device's filter equals
its gather-median of the device's neighbours bit for bit.

    python scripts/repet_time.py --out profiles/repet_time.json [--reps 10] [--no-cpu]
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
from audiosourcesep_amd import _lib, audio, repet  # noqa: E402

FP32_MFMA_PEAK = 157.3e12                  # FLOP / s
SECONDS, WIDTH_SEC = 180, 2.0


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
        for short in ("k_nn_norms", "k_nn_topk", "k_nn_transpose", "k_nn_median", "k_hpss_mask"):
            if short in e.name:
                out[short] = out.get(short, 0.0) + float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0)) / 1e3
    if not out:
        raise RuntimeError("the profiler reported none of the kernels")
    return out


def inputs():
    from tests import repet_ref as R
    n = SECONDS * audio.SR
    pattern, chirp = R.pattern_and_chirp(n)
    y = (pattern + chirp + 0.01 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)
    _, X = audio.mel_frames(y, return_stft=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    return [("audio", X.abs().contiguous()), ("random", torch.randn(tuple(X.shape), device="cuda", generator=gen).square().contiguous())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true", help="leave out the restatement's time on the host")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("repet_time.py measures on a GPU; none is visible")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    width = max(1, int(WIDTH_SEC * audio.SR / audio.HOP))
    res = dict(device=torch.cuda.get_device_name(0), build=os.environ.get("GLOWK_BUILD") or "unknown", fp32_mfma_peak_flops=FP32_MFMA_PEAK,
               seconds=SECONDS, width=width)
    for name, S in inputs():
        nsig, rows, F = S.shape
        k = repet.default_k(F, width)
        idx = torch.empty((nsig, F, k), dtype=torch.int32, device="cuda")
        sim, out, out2 = torch.empty((nsig, F, k), device="cuda"), torch.empty_like(S), torch.empty_like(S)
        nbytes = lib.glowk_nn_workspace_bytes(nsig, rows, F, k)
        work = torch.empty(nbytes // 4, device="cuda")

        def nb():
            _lib.check(lib.glowk_nn_neighbors(p(S), nsig, rows, F, k, width, p(idx), p(sim), p(work), nbytes, stream))

        def med():
            _lib.check(lib.glowk_nn_median(p(S), p(idx), nsig, rows, F, k, p(out), p(work), nbytes, stream))

        def both():
            nb()
            med()
        idx1 = torch.empty((nsig, F, 1), dtype=torch.int32, device="cuda")

        def nb1():                                                                  # k = 1: next to no list work, the Gram loop alone
            _lib.check(lib.glowk_nn_neighbors(p(S), nsig, rows, F, 1, width, p(idx1), None, p(work), nbytes, stream))
        entry = dict(shape=[nsig, rows, F], k=k, workspace_bytes=nbytes, nn_neighbors=timed(nb, args.reps), nn_median=timed(med, args.reps),
                     nn_neighbors_k1=timed(nb1, args.reps))
        rep = torch.minimum(S, out)
        resid = S - rep

        fg = torch.empty_like(S)

        def mask():
            _lib.check(lib.glowk_hpss_mask(p(rep), p(resid), p(S), S.numel(), 2.0, 2.0, 10.0, p(out2), p(fg), stream))
        entry["hpss_mask"] = timed(mask, args.reps)
        gram_ms, basis = entry["nn_neighbors"]["median_ms"], "nn_neighbors entry (k_nn_norms included): a lower bound"
        try:
            entry["kernels"] = kernel_times(both)
            if "k_nn_topk" in entry["kernels"]:
                gram_ms, basis = entry["kernels"]["k_nn_topk"], "k_nn_topk (Gram + scaling + selection)"
        except Exception as e:  # noqa: BLE001  (a machine without the profiler still gets the entry times)
            entry["kernels_error"] = "%s: %s" % (type(e).__name__, e)
        flop = 2.0 * rows * F * F * nsig
        entry["gram"] = dict(flop=flop, ms=gram_ms, time_of=basis, flops_per_s=flop / (gram_ms * 1e-3),
                             fraction_of_fp32_mfma_peak=flop / (gram_ms * 1e-3) / FP32_MFMA_PEAK)
        gathered = 4.0 * nsig * rows * F * int((idx >= 0).sum(-1).float().mean().item())
        entry["median_traffic"] = dict(gathered_bytes=gathered, transpose_bytes=8.0 * S.numel(), out_bytes=4.0 * S.numel(),
                                       compares=float(S.numel()) * k * k)
        if name == "audio" and not args.no_cpu:
            from tests import repet_ref as R
            host = S[0].cpu().numpy()
            dev_idx = idx[0].cpu().numpy()
            t0 = time.perf_counter()
            want_idx, _ = R.neighbors(host, k, width)
            t1 = time.perf_counter()
            filt = R.gather_median(host, dev_idx)                                   # of the device's neighbours: the same work
            t2 = time.perf_counter()
            same = float(np.mean([set(a.tolist()) == set(b.tolist()) for a, b in zip(dev_idx, want_idx)]))
            bitwise = bool(np.array_equal(out[0].cpu().numpy().view(np.uint32), filt.view(np.uint32)))
            entry["host"] = dict(neighbors_s=t1 - t0, gather_median_s=t2 - t1, total_s=t2 - t0, frames_with_the_fp64_neighbour_set=same,
                                 filter_equals_gather_median_of_device_neighbours_bitwise=bitwise)
        res[name] = entry
    res["note"] = ("HIP events around each C call on preallocated device tensors, median of reps after one warm-up call; kernels: device times "
                   "of one run from torch.profiler; gram: 2 rows frames^2 FLOP over the time named in time_of against fp32_mfma_peak_flops; "
                   "host: tests/repet_ref.py in fp64 numpy on the audio input (frames whose fp64 neighbour set differs from the device's "
                   "differ in near-ties of the similarity)")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
