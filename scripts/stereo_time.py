"""Time of the stereo EM Wiener filter (``glowk_mwf_em``, csrc/glowk_stereo.h) on one GPU: one minute of stereo audio = 30
extracts, S = 2 and 4 sources, n_iter = 0 / 2 / 10, as 30 problems of 64 frames (``method='frame'``) and as one problem of 1920
frames (``'whole'``), on synthetic spectra (tests/stereo_ref.py's model, drawn in float32 on the device).  HIP events around the C
call on preallocated tensors (the PSDs restored before every run, outside the events), median of --reps runs after a warm-up.
``bytes`` is what the call has to move through HBM -- x read, v read (and written when n_iter > 0), y written -- and
``bytes_per_s`` that over the median time.  Prints one JSON object and writes it to --out.
    python scripts/stereo_time.py --out profiles/stereo_time.json [--reps 20]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def spectra(S, P, T, seed=0):
    """x [P, 2, 1025, T, 2], v [S, P, 1025, T]: diffuse sources sqrt(v_j) z with v_j = exp(2 N(0, 1)), PSDs perturbed by exp(N(0, 1))."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    v = torch.exp(2.0 * torch.randn((S, P, 1025, T), device="cuda", generator=g))
    z = torch.randn((S, P, 2, 1025, T, 2), device="cuda", generator=g) * (0.5 ** 0.5)
    x = (torch.sqrt(v)[:, :, None, :, :, None] * z).sum(0).contiguous()
    return x, (v * torch.exp(torch.randn(v.shape, device="cuda", generator=g))).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    graft.build()
    from audiosourcesep_amd import _lib
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    try:
        build = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        build = ""
    res = dict(device=torch.cuda.get_device_name(0), build=build or "unknown", reps=args.reps)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for method, (P, T) in dict(frame=(30, 64), whole=(1, 30 * 64)).items():
        for S in (2, 4):
            x, v0 = spectra(S, P, T)
            v, y = torch.empty_like(v0), torch.empty((S, P, 2, 1025, T, 2), device="cuda")
            for n_iter in (0, 2, 10):
                def call():
                    _lib.check(lib.glowk_mwf_em(p(x), p(v), S, P, T, n_iter, p(y), None, stream))
                v.copy_(v0)
                call()
                torch.cuda.synchronize()
                ms = []
                for _ in range(args.reps):
                    v.copy_(v0)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    call()
                    b.record()
                    b.synchronize()
                    ms.append(a.elapsed_time(b))
                nbytes = P * 1025 * T * (16 + 4 * S * (2 if n_iter else 1) + 16 * S)
                med = float(np.median(ms))
                res["%s_S%d_iter%d" % (method, S, n_iter)] = dict(
                    problems=P, frames=T, median_ms=med, min_ms=float(np.min(ms)), bytes=nbytes, bytes_per_s=nbytes / (med * 1e-3),
                    ms_per_iteration=None if n_iter == 0 else (med - res["%s_S%d_iter0" % (method, S)]["median_ms"]) / n_iter,
                    finite=bool(torch.isfinite(y).all()))
    res["note"] = ("HIP events around glowk_mwf_em (one launch, all iterations) on preallocated device tensors; ms_per_iteration: "
                   "(median - the n_iter = 0 median) / n_iter")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
