"""Wall time of Griffin-Lim on one GPU (HIP events, median of repeated runs): the Griffin-Lim inversion of 2 x 30 tiles (two sources
of one minute, as run_basis_sep.py --inverse inverts them) by the `frame` and the `whole` method at n_iter = 32, the time per
iteration, and the rate of the two DFT-GEMM kernels against the 157.3 TFLOP/s fp32-MFMA peak.  Input: the committed mel tiles,
tiled to 30 per source.  Prints one JSON object and writes it to --out.
    python scripts/griffin_time.py --out profiles/griffin_time.json [--reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

PEAK_TFLOPS = 157.3
# useful DFT work per frame: the STFT is 1025 complex bins x 2048 samples, the iSTFT 4 overlapping 512-sample quarters x 1025
# complex bins per hop block; 2 real multiply-adds per complex term, 2 FLOP each
STFT_FLOP = 1025 * 2048 * 2 * 2
ISTFT_FLOP = 4 * 512 * 1025 * 2 * 2


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    graft.build()
    from audiosourcesep_amd import audio
    t = np.load(os.path.join(ROOT, "tests", "golden", "real_mel_tiles.npz"))
    src = [torch.from_numpy(np.tile(t[k], (8, 1, 1))[:30]).cuda() for k in ("gt1", "gt2")]   # 2 sources x 30 tiles [30, 96, 64]
    res = dict(device=torch.cuda.get_device_name(0))
    for method in ("frame", "whole"):
        res["griffin_invert_2x30_%s_n32" % method] = timed(
            lambda: audio.invert(src, algorithm="griffin", method=method, n_iter=32), args.reps)
    for method in ("frame", "whole"):
        res["mel_to_audio_30_%s_n32" % method] = timed(lambda: audio.mel_to_audio(src[0], method=method, n_iter=32), args.reps)
    P = audio.mel_to_power(torch.cat(src), 200).reshape(2, 30, 1025, 64)
    res["mel_to_power_2x30"] = timed(lambda: audio.mel_to_power(torch.cat(src), 200), args.reps)
    shapes = dict(frame=torch.sqrt(P).reshape(60, 1025, 64).contiguous(),
                  whole=torch.sqrt(P).permute(0, 2, 1, 3).reshape(2, 1025, 1920).contiguous())
    for method, S in shapes.items():
        init = torch.ones(S.shape, dtype=torch.complex64, device=S.device)
        frames = S.shape[0] * S.shape[2]
        t0 = timed(lambda: audio.griffinlim(S, n_iter=0, init=init), args.reps)
        t32 = timed(lambda: audio.griffinlim(S, n_iter=32, init=init), args.reps)
        it_ms = (t32["median_ms"] - t0["median_ms"]) / 32
        istft_ms = t0["median_ms"]
        stft_ms = it_ms - istft_ms
        res["griffinlim_2x30_%s" % method] = dict(
            frames=frames, n_iter0=t0, n_iter32=t32, per_iteration_ms=it_ms, istft_ms=istft_ms, stft_ms=stft_ms,
            istft_tflops=ISTFT_FLOP * frames / istft_ms / 1e9, stft_tflops=STFT_FLOP * frames / stft_ms / 1e9,
            iteration_tflops=(ISTFT_FLOP + STFT_FLOP) * frames / it_ms / 1e9)
        r = res["griffinlim_2x30_%s" % method]
        for k in ("istft", "stft", "iteration"):
            r[k + "_pct_of_peak"] = 100.0 * r[k + "_tflops"] / PEAK_TFLOPS
    res["note"] = ("median of HIP-event wall times per call on the current stream.  griffin_invert = one NNLS launch over both "
                   "sources + sqrt + phases drawn on the device + Griffin-Lim (2 n_iter + 1 launches); griffinlim: magnitudes given, "
                   "ones as the start; per_iteration = (t(32) - t(0)) / 32; istft = t(0) (one k_istft launch, including the call's "
                   "host work), stft = per_iteration - istft; rates count the useful DFT FLOPs (%d per frame for the STFT, %d for "
                   "the iSTFT) against the %.1f TFLOP/s fp32-MFMA peak" % (STFT_FLOP, ISTFT_FLOP, PEAK_TFLOPS))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
