"""Wall time of the oracle separation systems (IBM, IRM, MWF) on one GPU against the fp64 NumPy restatement on the host, on
synthetic stereo audio (per channel, filtered noise with a shared and an independent part): 60 s at 16 kHz with 2 sources, and a 200 s track at
44.1 kHz with 4 sources.  GPU: HIP events around the whole call from float32 CUDA tensors to the estimates' tensor (host
validation, the STFT of every channel, masks / Wiener gains, iSTFT), median of --reps runs after a warm-up.  Prints one JSON
object and writes it to --out.
    python scripts/oracle_time.py --out profiles/oracle_time.json [--reps 5] [--no-cpu]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), wall_median_ms=float(np.median(wall)), reps=reps)


def signals(nsrc, n, seed=0):
    """Per channel: filtered (a shared signal + an independent one), as tests/test_gpu_oracle_systems.py's ``synthetic``."""
    rng = np.random.default_rng(seed)
    src = np.empty((nsrc, n, 2), dtype=np.float32)
    for j in range(nsrc):
        base = rng.standard_normal(n)
        for c in range(2):
            src[j, :, c] = np.convolve(base + rng.standard_normal(n), rng.standard_normal(8 + 4 * j) / (2 + j), mode="same")
    return src.sum(0), src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    graft.build()
    from audiosourcesep_amd import oracle_systems as O
    from tests import oracle_systems_ref as R
    try:
        build = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        build = ""
    res = dict(device=torch.cuda.get_device_name(0), build=build or "unknown")
    tracks = dict(s60_16k_2src=(2, 60 * 16000), s200_44k_4src=(4, 200 * 44100))
    for tname, (nsrc, n) in tracks.items():
        mix, src = signals(nsrc, n)
        tm, ts = torch.from_numpy(mix).cuda(), torch.from_numpy(src).cuda()
        res[tname] = dict(signal="%d s, %d sources, stereo, float32" % (n // (16000 if nsrc == 2 else 44100), nsrc))
        for name in ("IBM", "IRM", "MWF"):
            fn = getattr(O, name)
            r = timed(lambda: fn(tm, ts), args.reps)
            if not args.no_cpu and tname == "s60_16k_2src":
                t0 = time.perf_counter()
                want = getattr(R, name)(mix, src)
                r["numpy_restatement_s"] = time.perf_counter() - t0
                got = fn(tm, ts).cpu().numpy().astype(np.float64)
                r["max_rel_l2"] = float(max(np.linalg.norm(got[j] - want[j]) / np.linalg.norm(want[j]) for j in range(nsrc)))
            res[tname][name] = r
        del tm, ts
        torch.cuda.empty_cache()
    res["note"] = ("HIP-event and wall times per call from CUDA tensors (validation, STFT, masks or Wiener gains, iSTFT); "
                   "numpy_restatement_s: tests/oracle_systems_ref.py (fp64 numpy) on this host's CPU, one run; max_rel_l2: the "
                   "largest per-source relative L2 distance between the two")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
