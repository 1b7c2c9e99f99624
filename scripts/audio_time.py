"""Wall time of the audio ends on one GPU (HIP events, median of repeated runs): the front end on 30 extracts (one minute of
audio) and on one hour (1765 extracts), mel_to_power + the Wiener iSTFT for 2 x 30 tiles, and separate_audio around a short
BASIS loop with small flows (96x64, L = 3, K = 2, n_filters 128; 2 sigmas x T = 4), with the share of its two audio ends.
Input: the committed audio excerpt, tiled.  Prints one JSON object and writes it to --out.
    python scripts/audio_time.py --out profiles/audio_time.json [--reps 10]
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
    from audiosourcesep_amd.flow_models.flow_builder import build_glow
    pcm = np.load(os.path.join(ROOT, "tests", "golden", "real_audio_excerpt.npz"))["pcm"].astype(np.float32) / 32768.0
    minute = torch.from_numpy(np.tile(pcm, (5, 1))).cuda()                     # 30 extracts
    hour = torch.from_numpy(np.tile(pcm, (295, 1))[:1765]).cuda()               # 1765 extracts
    res = dict(device=torch.cuda.get_device_name(0))
    res["front_end_30"] = timed(lambda: audio.mel_tiles(minute, return_stft=True), args.reps)
    res["front_end_1765"] = timed(lambda: audio.mel_tiles(hour, return_stft=True), max(3, args.reps // 2))
    mel, X = audio.mel_tiles(minute, return_stft=True)
    tiles = [mel, mel.flip(0).contiguous()]
    both = torch.cat(tiles)
    res["mel_to_power_2x30"] = timed(lambda: audio.mel_to_power(both, 200), args.reps)          # one launch, as invert makes it
    p = audio.mel_to_power(both, 200).reshape(2, 30, 1025, 64)
    res["wiener_istft_2x30"] = timed(lambda: audio.masked_istft(p, X, wiener=True), args.reps)
    res["invert_wiener_2x30"] = timed(lambda: audio.invert(tiles, X, wiener=True), args.reps)
    flows = [build_glow(mel[:8].contiguous(), [96, 64, 1], L=3, K=2, n_filters=128, learntop=True, seed=40 + i, data_type="melspec",
                        minval=-100.0, maxval=20.0, use_logit=False) for i in range(2)]
    y = minute.reshape(-1)
    sig = np.array([20.0, 5.0], np.float32)
    res["separate_audio_30_small_flows_2sigma_T4"] = timed(
        lambda: audio.separate_audio(y, flows[0], flows[1], sig, T=4, delta=1e-4, seed=9, wiener=True), max(3, args.reps // 2))
    res["note"] = ("median of HIP-event wall times per call on the current stream; front end includes the complex STFT output; "
                   "separate_audio = front end + BASIS loop (2 sigmas x 4 steps, small flows) + one mel_to_power launch over both sources + Wiener iSTFT")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
