"""Times of the whole-signal path (csrc/glowk_longform.h) on one GPU for a 180 s signal at 16 kHz: 2 880 000 samples, F = 5626
frames, 175 tiles of 64 frames every 32, S = 2 sources.  HIP events around each call on preallocated device tensors, median of
--reps runs after a warm-up:

* ``glowk_mel_frames`` with and without the complex STFT output, ``glowk_tile_cut`` (top_db 80), ``glowk_tile_stitch`` (S = 2);
* ``audio.invert_frames`` (200 NNLS iterations, single-channel Wiener; the Python call, its torch glue included);
* beside them ``glowk_mel_frontend`` (``audio.mel_tiles``' C call) on the same audio cut into its 88 whole extracts of 64 frames, the
  only front end there was before: ``us_per_frame`` compares the two.

``bytes`` is what a call has to move through HBM (inputs read once, outputs written once) and ``bytes_per_s`` that over the median.
Prints one JSON object and writes it to --out.  Needs a GPU and the built library; nothing is timed without them.
    python scripts/longform_time.py --out profiles/longform_time.json [--reps 20]
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
from audiosourcesep_amd import _lib, audio  # noqa: E402

SECONDS, S, WIDTH, TILE_HOP = 180, 2, 64, 32


def signal(n, seed=0):
    """Two chirps and noise, float32 on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(n, device="cuda", dtype=torch.float64) / audio.SR
    y = 0.3 * torch.sin(2 * np.pi * (220.0 * t + 3.0 * t * t)) + 0.2 * torch.sin(2 * np.pi * (1500.0 * t - 2.0 * t * t))
    return (y.float() + 0.05 * torch.randn(n, device="cuda", generator=g)).contiguous()


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
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    try:
        build = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        build = ""
    n = SECONDS * audio.SR
    F = 1 + n // audio.HOP
    N = audio.tile_count(F, WIDTH, TILE_HOP)
    res = dict(device=torch.cuda.get_device_name(0), build=build or "unknown", reps=args.reps, seconds=SECONDS, samples=n, frames=F, tiles=N,
               sources=S, width=WIDTH, tile_hop=TILE_HOP)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    y = signal(n)[None].contiguous()
    mel = torch.empty((1, 96, F), device="cuda")
    X = torch.empty((1, 1025, F, 2), device="cuda")

    def entry(key, call, nbytes, frames):
        med, lo = timed(call, args.reps)
        res[key] = dict(median_ms=med, min_ms=lo, bytes=nbytes, bytes_per_s=nbytes / (med * 1e-3), us_per_frame=1e3 * med / frames)

    entry("mel_frames_with_stft", lambda: _lib.check(lib.glowk_mel_frames(p(y), 1, n, p(mel), p(X), stream)), 4 * n + 8 * 1025 * F + 4 * 96 * F, F)
    entry("mel_frames", lambda: _lib.check(lib.glowk_mel_frames(p(y), 1, n, p(mel), None, stream)), 4 * n + 4 * 96 * F, F)
    mel_long = mel.clone()

    # the per-extract front end on the same audio: its 88 whole extracts (the last 7 680 samples are what it drops)
    ex = audio.extracts(y[0]).contiguous()
    E, Fe = ex.shape[0], 1 + audio.EXTRACT // audio.HOP
    mel_e = torch.empty((E, 96, Fe, 1), device="cuda")
    X_e = torch.empty((E, 1025, Fe, 2), device="cuda")
    res["extracts"] = E
    entry("mel_frontend_extracts_with_stft", lambda: _lib.check(lib.glowk_mel_frontend(p(ex), E, audio.EXTRACT, 80.0, p(mel_e), p(X_e), stream)),
          4 * ex.numel() + 8 * 1025 * E * Fe + 4 * 96 * E * Fe, E * Fe)
    entry("mel_frontend_extracts", lambda: _lib.check(lib.glowk_mel_frontend(p(ex), E, audio.EXTRACT, 80.0, p(mel_e), None, stream)),
          4 * ex.numel() + 4 * 96 * E * Fe, E * Fe)

    tiles = torch.empty((1, N, 96, WIDTH), device="cuda")
    entry("tile_cut", lambda: _lib.check(lib.glowk_tile_cut(p(mel_long), 1, F, WIDTH, TILE_HOP, 80.0, p(tiles), stream)),
          4 * 96 * F + 4 * tiles.numel(), F)
    g = torch.Generator(device="cuda").manual_seed(1)
    st = (tiles + 3.0 * torch.randn((S, N, 96, WIDTH), device="cuda", generator=g)).contiguous()
    frames = torch.empty((S, 96, F), device="cuda")
    entry("tile_stitch", lambda: _lib.check(lib.glowk_tile_stitch(p(st), S, N, WIDTH, TILE_HOP, F, p(frames), stream)),
          4 * st.numel() + 4 * frames.numel(), S * F)
    Xc = torch.view_as_complex(X)[0]
    out = []

    def inv():
        out[:] = [audio.invert_frames(frames, Xc, n, wiener=True, iters=200)]
    _lib.check(lib.glowk_mel_frames(p(y), 1, n, p(mel), p(X), stream))
    med, lo = timed(inv, args.reps)
    res["invert_frames"] = dict(median_ms=med, min_ms=lo, nnls_iters=200, wiener=True, us_per_frame=1e3 * med / (S * F),
                                finite=bool(torch.isfinite(out[0]).all()), shape=list(out[0].shape))
    res["finite"] = bool(torch.isfinite(mel_long).all() and torch.isfinite(tiles).all() and torch.isfinite(frames).all())
    res["note"] = ("HIP events around each call on preallocated device tensors, median of reps after one warm-up call; invert_frames is the "
                   "Python call (mel_to_power on 88 tiles of 128 frames, the Wiener mask in torch, one iSTFT launch, the trim); "
                   "us_per_frame: median over the frames the call produces")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
