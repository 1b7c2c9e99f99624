"""Wall time of the sample-rate converter on one GPU (HIP events, median of repeated runs): 44.1 kHz -> 16 kHz and 16 kHz -> 44.1 kHz
for three one-minute signals (a mixture and its two stems) in one launch, with the rates the call achieves: taps per second
(multiply-adds of the filter sum) and GB/s of signal read and written.  Input: the committed audio excerpt, tiled and resampled.
Prints one JSON object and writes it to --out.
    python scripts/resample_time.py --out profiles/resample_time.json [--reps 20]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

Z = 64      # zero crossings of the filter on each side


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), reps=reps)


def taps_per_output(sr_in, sr_out):
    """Mean taps of one output away from the signal's ends: the filter spans 2 Z / min(1, sr_out / sr_in) input samples."""
    return 2.0 * Z * max(1.0, sr_in / sr_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    graft.build()
    from audiosourcesep_amd import audio
    pcm = np.load(os.path.join(ROOT, "tests", "golden", "real_audio_excerpt.npz"))["pcm"].astype(np.float32).reshape(-1) / 32768.0
    minute16 = np.tile(pcm, 5)[:60 * 16000]
    x16 = torch.from_numpy(np.stack([minute16, 0.6 * minute16, 0.4 * minute16[::-1].copy()])).cuda()      # mixture + two stems
    x441 = audio.resample(x16, 16000, 44100)
    res = dict(device=torch.cuda.get_device_name(0))
    for name, x, sr_in, sr_out in (("44100_to_16000_3x60s", x441, 44100, 16000), ("16000_to_44100_3x60s", x16, 16000, 44100)):
        t = timed(lambda: audio.resample(x, sr_in, sr_out), args.reps)
        n_out = math.ceil(x.shape[1] * sr_out / sr_in)
        taps = 3 * n_out * taps_per_output(sr_in, sr_out)
        t.update(n_in=int(x.shape[1]), n_out=int(n_out), taps_per_output=taps_per_output(sr_in, sr_out),
                 gtaps_per_s=taps / t["median_ms"] / 1e6, signal_gb_per_s=3 * 4 * (x.shape[1] + n_out) / t["median_ms"] / 1e6)
        res[name] = t
    res["access_scheme"] = ("one 256-thread workgroup per 256 consecutive outputs of one signal; the input span staged in LDS; the filter "
                            "table as (T[k], T[k+1]-T[k]) float2 pairs gathered from global memory (256 KB, L2-resident), one 8-byte load "
                            "per tap; table positions by integer arithmetic")
    res["note"] = ("median of HIP-event wall times per audio.resample call on the current stream (the output allocation and the call's "
                   "host work included); taps = outputs x 2 Z max(1, sr_in / sr_out); GB/s counts the signals read and written once")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
