"""Times of the S-source BASIS step on one GPU (HIP events), for S in {2, 3, 4} (the update kernel also for S = 16):
  * the update kernel alone (``glowk_basis_update_n``, device RNG) at 30 tiles of 96x64 and at 64 times as many, with the bandwidth
    its time implies against the (3 S + 1) * 4 bytes per element it has to move, and the two-source entry point
    (``glowk_basis_update``: the same S = 2 instance behind the two-source argument list) beside it;
  * one Langevin step (S gradient evaluations + the update) with config-B-geometry priors (64x64, L = 3, n_filters 512) of K = 32
    on 30 tiles, the gradients on side streams (created once; and "auto": created per call) and one after the other, alternated in
    one process; for S = 2 the same through the two-source signature (``basis_inner_loop``), an adapter over the same loop.
Synthetic weights and tiles.  Prints one JSON object and writes it to --out.
    python scripts/basis_sources_time.py --out profiles/basis_sources_time.json [--reps 7] [--K 32]
    rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/basis_sources_time.py --update-only    (kernel times)
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


def timed(fn, reps, inner=1):
    """Median / min over ``reps`` event-timed windows of ``inner`` calls each, per call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), reps=reps, calls_per_window=inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--tiles", type=int, default=30)
    ap.add_argument("--update-only", action="store_true", help="only the update kernels at --tiles (for a kernel trace)")
    args = ap.parse_args()
    from audiosourcesep_amd import _lib, basis
    if not os.path.exists(_lib.LIB_PATH):
        graft.build()
    from audiosourcesep_amd.config import GlowConfig
    from audiosourcesep_amd.flow_models.flow_glow import GlowFlow
    from audiosourcesep_amd.synthetic import calibrated_engine, synthetic_mel_tiles
    if not torch.cuda.is_available():
        raise SystemExit("basis_sources_time.py measures on a GPU; none is visible")
    res = dict(device=torch.cuda.get_device_name(0), tiles=args.tiles, K=args.K)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def update_times(n_tiles):
        shape = (n_tiles, 96, 64, 1)
        n = int(np.prod(shape))
        mk = lambda lo, hi: lo + (hi - lo) * torch.rand(shape, device="cuda", generator=gen)   # noqa: E731
        mixed, out = mk(-80.0, 10.0), {}
        for S in (2, 3, 4, 16):
            xs, gs = [mk(-80.0, 10.0) for _ in range(S)], [mk(-5.0, 5.0) for _ in range(S)]
            step = [0]

            def upd():
                basis.langevin_update_n(mixed, xs, gs, 1e-9, 1.0, seed=1, step=step[0])      # (eta tiny: the state stays in range over the run)
                step[0] += 1

            def upd2():
                basis.langevin_update(mixed, xs[0], xs[1], gs[0], gs[1], 1e-9, 1.0, seed=1, step=step[0])
                step[0] += 1
            for name, fn in (("S%d" % S, upd),) + ((("S2_two_source_entry", upd2),) if S == 2 else ()):
                r = timed(fn, args.reps, inner=200)
                nbytes = (3 * S + 1) * 4 * n
                r.update(bytes_per_call=nbytes, implied_GBps=nbytes / (r["median_ms"] * 1e-3) / 1e9)
                out[name] = r
        return out
    res["update_kernel"] = update_times(args.tiles)
    if args.update_only:
        print(json.dumps(res))
        return
    res["update_kernel_%d_tiles" % (64 * args.tiles)] = update_times(64 * args.tiles)     # large enough to be bound by HBM, not by the launch
    # one Langevin step around priors of the flagship geometry
    cfg = GlowConfig(H=64, W=64, C=1, L=3, K=args.K, F=512)
    flows = []
    for k in range(4):
        eng, _ = calibrated_engine(cfg, device=0, init_tiles=args.tiles, seed=100 + k)
        eng.set_precision(_lib.PREC_F16X3)
        eng.set_range_policy("fallback")
        flows.append(GlowFlow(eng))
    sig = basis.get_sigmas(1.0, 0.01, 10)
    tiles = lambda seed: torch.from_numpy(synthetic_mel_tiles(args.tiles, cfg, seed=seed)).cuda()   # noqa: E731
    res["langevin_step"] = {}
    for S in (2, 3, 4):
        m = basis.mixing([tiles(10 + k) for k in range(S)])
        start = [tiles(20 + k) for k in range(S)]          # every timed step starts here: synthetic weights give the chain nowhere to go
        side = [torch.cuda.Stream() for _ in range(min(S, basis.MAX_SIDE_STREAMS))]
        t, last = [0], {}

        def step_n(streams):
            out = basis.basis_inner_loop_n(m, start, flows[:S], 9, sig, T=1, seed=3, step0=t[0], streams=streams)
            t[0] += 1
            return out

        def step_2(streams):
            out = basis.basis_inner_loop(m, start[0], start[1], flows[0], flows[1], 9, sig, T=1, seed=3, step0=t[0], streams=streams)
            t[0] += 1
            return out
        variants = {"side_streams": lambda: step_n(side), "sequential": lambda: step_n(None), "auto_streams": lambda: step_n("auto")}
        if S == 2:   # the two-source signature beside it: the same stream objects, none, and "auto" (two new streams per call)
            variants.update({"two_source_path_side_streams": lambda: step_2(tuple(side)), "two_source_path_sequential": lambda: step_2(None),
                             "two_source_path_auto_streams": lambda: step_2("auto")})
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.reps):                      # the variants alternate inside one process
            for key, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(3):
                    last[key] = fn()
                b.record()
                b.synchronize()
                ms[key].append(a.elapsed_time(b) / 3)
        assert all(bool(torch.isfinite(x).all()) for out in last.values() for x in out)
        entry = {"streams": len(side)}
        for key, v in ms.items():
            entry[key + "_ms"] = float(np.median(v))
            entry[key + "_min_ms"] = float(np.min(v))
        res["langevin_step"]["S%d" % S] = entry
    res["range_fallbacks"] = [f.engine.range_status(sync=False)[1] for f in flows]
    res["note"] = ("median of HIP-event windows (update kernel: 200 calls per window; step: 3 steps per window, the variants "
                   "alternating); implied_GBps = (3 S + 1) * 4 bytes per element over the time per call of 200 back-to-back calls -- at 30 "
                   "tiles the working set is a few MB (it stays in the last-level cache) and the figure contains the launch, so it is not "
                   "an HBM figure; the 64x larger batch is; priors: synthetic weights, "
                   "f16x3, range policy fallback")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
