"""Times of the convolutive NMF kernels (csrc/glowk_nmfd.h) on one GPU at 180 s of 16 kHz audio, beside plain NMF at as many components.

Shape 1 x 1025 x 5626, |N(0, 1)|^2 with about 5 % silent frames (tests/nmf_ref.py's inputs), (K, Tw) = (16, 8), (4, 32), (32, 4) and
(128, 1) -- 128 stacked components each -- and beta = 0, 1, 2.  HIP events around each C call on preallocated device tensors, median,
minimum and spread of --reps runs after a warm-up; one call runs --iters iterations, the times are per iteration:

* ``iteration`` / ``h_update`` / ``w_update``: ``glowk_nmfd_fit`` with ``update_w`` = 1, 0, 2;
* ``nmf``: the same three of ``glowk_nmf_fit`` at K Tw plain components in the same run, and ``ratio`` = nmfd / nmf of the medians;
* ``kernels``: device times of one call from torch.profiler, per iteration, where that is available (the H update's two launches apart);
* ``divergence`` and ``masks`` (two sources of K / 2 components, a one-channel complex spectrum, power 1).

    python scripts/nmfd_time.py --out profiles/nmfd_time.json [--reps 10] [--iters 10]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiosourcesep_amd import _lib, nmf, nmfd  # noqa: E402

ROWS, FRAMES = 1025, 5626
CASES = ((16, 8), (4, 32), (32, 4), (128, 1))
KERNELS = ("k_nmfd_update_h", "k_nmfd_h_finish", "k_nmfd_update_w", "k_nmf_w_finish", "k_nmf_update_h", "k_nmf_update_w")


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
            if short + "<" in e.name or short + "(" in e.name or e.name.endswith(short):
                out[short] = out.get(short, 0.0) + float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0)) / 1e3 / per
    if not out:
        raise RuntimeError("the profiler reported none of the kernels")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nmfd_time.py measures on a GPU; none is visible")
    from tests import nmf_ref as N
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    V = torch.from_numpy(N.spectra((ROWS, FRAMES), 1)).cuda()
    res = dict(device=torch.cuda.get_device_name(0), build=os.environ.get("GLOWK_BUILD") or "unknown", shape=[1, ROWS, FRAMES],
               iterations_per_call=args.iters)
    modes = (("iteration", 1), ("h_update", 0), ("w_update", 2))
    for K, Tw in CASES:
        KS = K * Tw
        W0, H0 = nmfd.init(V, K, Tw, seed=0)
        Wp0, Hp0 = nmf.init(V, KS, seed=0)
        nbytes = lib.glowk_nmfd_workspace_bytes(1, ROWS, FRAMES, K, Tw)
        pbytes = lib.glowk_nmf_workspace_bytes(1, ROWS, FRAMES, KS)
        work = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
        entry = dict(workspace_bytes=nbytes, nmf_workspace_bytes=pbytes)
        for beta in (0, 1, 2):
            Vb = V.clamp_min(1e-3) if beta == 0 else V
            W, H, Wp, Hp = W0.clone(), H0.clone(), Wp0.clone(), Hp0.clone()

            def fit(mode, n=args.iters):
                _lib.check(lib.glowk_nmfd_fit(p(Vb), 1, ROWS, FRAMES, p(W), 1, p(H), K, Tw, beta, n, mode, p(work), nbytes, stream))

            def plain(mode, n=args.iters):
                _lib.check(lib.glowk_nmf_fit(p(Vb), 1, ROWS, FRAMES, p(Wp), 1, p(Hp), KS, beta, n, mode, p(work), pbytes, stream))
            b = dict(nmf={}, ratio={})
            for name, mode in modes:
                for t, t0 in ((W, W0), (H, H0), (Wp, Wp0), (Hp, Hp0)):
                    t.copy_(t0)
                b[name] = timed(lambda: fit(mode), args.reps, args.iters)
                b["nmf"][name] = timed(lambda: plain(mode), args.reps, args.iters)
                b["ratio"][name] = b[name]["median_ms"] / b["nmf"][name]["median_ms"]
            try:
                b["kernels"] = kernel_times(lambda: fit(1), args.iters)
                b["nmf"]["kernels"] = kernel_times(lambda: plain(1), args.iters)
            except Exception as e:  # noqa: BLE001  (a machine without the profiler still gets the entry times)
                b["kernels_error"] = "%s: %s" % (type(e).__name__, e)
            out = torch.empty((1,), dtype=torch.float64, device="cuda")
            b["divergence"] = timed(lambda: _lib.check(lib.glowk_nmfd_divergence(p(Vb), 1, ROWS, FRAMES, p(W), 1, p(H), K, Tw, beta, p(out), p(work), nbytes,
                                                                                 stream)), args.reps)
            b["nmf"]["divergence"] = timed(lambda: _lib.check(lib.glowk_nmf_divergence(p(Vb), 1, ROWS, FRAMES, p(Wp), 1, p(Hp), KS, beta, p(out), p(work),
                                                                                       pbytes, stream)), args.reps)
            b["ratio"]["divergence"] = b["divergence"]["median_ms"] / b["nmf"]["divergence"]["median_ms"]
            entry["beta%d" % beta] = b
        half, S = K // 2, 2
        bounds = (ctypes.c_int32 * 3)(0, half, K)
        X = torch.polar(V, torch.rand_like(V) * 6.2831853).contiguous()
        m = torch.empty((S, ROWS, FRAMES), device="cuda")
        spec = torch.empty((S, 1, ROWS, FRAMES), dtype=torch.complex64, device="cuda")
        entry["masks"] = timed(lambda: _lib.check(lib.glowk_nmfd_masks(p(W0), 1, p(H0), 1, ROWS, FRAMES, K, Tw, bounds, S, 1, p(X), 1, p(m), p(spec), stream)),
                               args.reps)
        pb = (ctypes.c_int32 * 3)(0, half * Tw, KS)
        entry["nmf_masks"] = timed(lambda: _lib.check(lib.glowk_nmf_masks(p(Wp0), 1, p(Hp0), 1, ROWS, FRAMES, KS, pb, S, 1, p(X), 1, p(m), p(spec), stream)),
                                   args.reps)
        entry["masks_ratio"] = entry["masks"]["median_ms"] / entry["nmf_masks"]["median_ms"]
        res["K%d_Tw%d" % (K, Tw)] = entry
    res["note"] = ("HIP events around each C call on preallocated device tensors, median of reps after one warm-up call, divided by the "
                   "iterations of a call; nmf: glowk_nmf_* at K Tw plain components in the same run; ratio: nmfd / nmf of the medians; kernels: "
                   "device times of one call from torch.profiler per iteration")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
