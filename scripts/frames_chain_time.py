"""Time of the non-prior part of one Langevin step of the whole-signal chain (csrc/glowk_frames.h) on one GPU: a 180 s signal at
16 kHz, F = 5626 frames of 96 mel rows, 175 tiles of 64 frames every 32, S = 2 sources, the device RNG for the noise.  HIP events
around each call on preallocated device tensors, median, minimum and spread (max - min) of --reps runs after a warm-up:

* ``fused``: one ``glowk_basis_update_frames`` with ``tiles_out`` -- gather and stitch the gradient tiles, update the frames, write the
  next step's tiles;
* ``composed``: the same data movement from the entry points there were before it -- ``glowk_tile_stitch`` of the S gradient tensors,
  ``glowk_basis_update_n`` on the frames, ``glowk_tile_cut`` without a floor (three launches; the cut also clips, which the chain
  must not) -- and each of the three alone.  These entry points are the ones the commit before the fused kernel had (``baseline_commit``;
  their device code is unchanged), so both sides are timed in one process, on one device, on the same tensors;
* ``prior_gradient``: one ``log_prob_grad`` of a prior of the front end's geometry (configs/melspec_glow.yml: 96 x 64, L = 3, K = 40,
  512 filters, synthetic weights, f16x3) on 175 mel-like tiles, next to which the README states the update's share of a step.

Prints one JSON object and writes it to --out.  ``GLOWK_BUILD`` names the build where there is no git checkout to ask.
    python scripts/frames_chain_time.py --out profiles/frames_chain_time.json [--reps 20] [--no-prior]
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
from audiosourcesep_amd import _lib, audio, basis  # noqa: E402

SECONDS, S, ROWS, WIDTH, TILE_HOP = 180, 2, 96, 64, 32
BASELINE_COMMIT = "8934ace"                # the last commit without the fused kernel: the composed entry points are its, unchanged


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-prior", action="store_true", help="leave out the prior's gradient evaluation")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frames_chain_time.py measures on a GPU; none is visible")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
    try:
        build = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        build = ""
    build = os.environ.get("GLOWK_BUILD") or build or "unknown"
    F = 1 + SECONDS * audio.SR // audio.HOP
    N = audio.tile_count(F, WIDTH, TILE_HOP)
    n = ROWS * F
    res = dict(device=torch.cuda.get_device_name(0), baseline_commit=BASELINE_COMMIT, seconds=SECONDS, frames=F, rows=ROWS, tiles=N,
               sources=S, width=WIDTH, tile_hop=TILE_HOP)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(1)
    mk = lambda shape, lo, hi: (lo + (hi - lo) * torch.rand(shape, device="cuda", generator=gen)).contiguous()   # noqa: E731
    mixed = mk((ROWS, F), -80.0, 10.0)
    start = mk((S, ROWS, F), -80.0, 10.0)
    g = mk((S, N, ROWS, WIDTH), -5.0, 5.0)
    tiles = torch.empty((S, N, ROWS, WIDTH), device="cuda")
    eta, lam, step = 1e-9, 1.0, [0]                                # (eta tiny: the state stays in range over the run)
    tile_bytes, frame_bytes = 4 * g[0].numel(), 4 * n

    # (b) the composition: stitch the S gradient tensors, update the frames, cut them again
    x = start.clone()
    score = torch.empty((S, ROWS, F), device="cuda")
    xs_ptr, score_ptr = basis._ptrs(list(x)), basis._ptrs(list(score))

    def stitch():
        _lib.check(lib.glowk_tile_stitch(p(g), S, N, WIDTH, TILE_HOP, F, p(score), stream))

    def update():
        _lib.check(lib.glowk_basis_update_n(xs_ptr, score_ptr, None, S, p(mixed), n, _lib.MIX_DB, eta, lam, 1, step[0], 0, None, stream))
        step[0] += 1

    def cut():
        _lib.check(lib.glowk_tile_cut(p(x), S, F, WIDTH, TILE_HOP, 0.0, p(tiles), stream))

    def composed():
        stitch()
        update()
        cut()

    composed_bytes = S * (tile_bytes + frame_bytes) + (3 * S + 1) * frame_bytes + S * (frame_bytes + tile_bytes)
    entries = {"composed": (composed, composed_bytes), "composed_stitch": (stitch, S * (tile_bytes + frame_bytes)),
               "composed_update": (update, (3 * S + 1) * frame_bytes), "composed_cut": (cut, S * (frame_bytes + tile_bytes))}
    # (a) the fused step: S gradient tensors and the mixture read once, the frames read and written once, the tiles written once
    y = start.clone()
    g_ptr = basis._ptrs(list(g))

    def fused():
        _lib.check(lib.glowk_basis_update_frames(p(y), g_ptr, None, S, p(mixed), ROWS, F, WIDTH, TILE_HOP, _lib.MIX_DB, eta, lam, 1, step[0],
                                                 -100.0, p(tiles), None, stream))
        step[0] += 1
    entries["fused"] = (fused, S * tile_bytes + (2 * S + 1) * frame_bytes + S * tile_bytes)
    for call, _ in entries.values():
        call()
    torch.cuda.synchronize()
    for key, (call, nbytes) in entries.items():
        r = timed(call, args.reps)
        r.update(build=BASELINE_COMMIT if key.startswith("composed") else build, bytes=nbytes, bytes_per_s=nbytes / (r["median_ms"] * 1e-3))
        res[key] = r
    res["finite"] = bool(torch.isfinite(x).all() and torch.isfinite(y).all() and torch.isfinite(tiles).all())
    res["fused_not_slower"] = res["fused"]["median_ms"] <= res["composed"]["median_ms"] + res["composed"]["spread_ms"]
    if not args.no_prior:
        from audiosourcesep_amd.config import CONFIG_YAML
        from audiosourcesep_amd.synthetic import calibrated_engine, synthetic_mel_tiles
        eng, _ = calibrated_engine(CONFIG_YAML, device=0, init_tiles=8, seed=100)
        eng.set_precision(_lib.PREC_F16X3)
        eng.set_range_policy("fallback")
        batch = torch.from_numpy(synthetic_mel_tiles(N, CONFIG_YAML, seed=20)).cuda()
        r = timed(lambda: eng.log_prob_grad(batch), max(3, args.reps // 4))
        r.update(build=build, config="96x64 L=3 K=40 F=512", precision="f16x3", tiles=N, range_fallbacks=eng.range_status(sync=False)[1])
        res["prior_gradient"] = r
        res["update_share_of_step"] = res["fused"]["median_ms"] / (S * r["median_ms"] + res["fused"]["median_ms"])
    res["note"] = ("HIP events around each call on preallocated device tensors, device RNG, median / min / max - min of reps after a warm-up; "
                   "bytes: what a call has to move through HBM (inputs read once, outputs written once); update_share_of_step: fused over S "
                   "prior gradients plus fused")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
