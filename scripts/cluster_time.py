"""Times of the clustering kernels (csrc/glowk_cluster.h) on one GPU.

Features of 1 x D x 1025 x 5626 (180 s of 16 kHz audio) for (D, J) = (1, 3), (4, 2) and (8, 8): float32 draws around J centres with
gamma(0.5) weights.  HIP events around the C entries on preallocated device tensors (no allocation, no copy in the timed region):
median, minimum and spread of --reps runs after a warm-up.  ``iteration`` is glowk_cluster_fit at 20 iterations over 20 (the statistics
pass and the per-signal kernel; pass 0 and the start amortised), ``stats`` the staged statistics (constants, the pass, the sum of the
partials), ``update`` the per-signal kernel alone, ``posteriors`` the masks.  ``spatial_features`` is on a stereo STFT of the same
size; ``ensemble`` is ``cluster.ensemble`` whole (its four default primitives included) and with ready masks (the clustering alone), at
--ensemble-iters iterations.  ``numpy_iteration_s`` is the host's time for one iteration of the fp64 restatement on the same input (where its [J, P, cells] array
fits in 2 GiB).

The byte floor of the statistics pass is 4 (D + 1) bytes per cell; ``copy_gb_per_s`` is a device-to-device copy of 256 MiB measured
here, and ``of_copy_rate`` the fraction of it the pass reaches.  HIP events cannot split the two launches of an iteration; the kernels'
own times come from a kernel trace of a run that does nothing but one fit, merged with --kernel-stats:

    rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -- python scripts/cluster_time.py --fit-only 8,8
    python scripts/cluster_time.py --out profiles/cluster_time.json [--kernel-stats D,J:file.csv ...] [--no-cpu]
"""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiosourcesep_amd import _lib, cluster  # noqa: E402
from tests import cluster_ref as R  # noqa: E402

ROWS, FRAMES = 1025, 5626
CASES = [(1, 3), (4, 2), (8, 8)]


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


def with_bytes(t, nbytes, copy_rate, key="median_ms"):
    rate = nbytes / (t[key] * 1e-3) / 1e9
    return dict(t, bytes=int(nbytes), gb_per_s=rate, of_copy_rate=rate / copy_rate)


def kernel_stats(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3)
    return out


def inputs(D, J):
    """Drawn on the device (tests/cluster_ref.inputs' recipe, not its numbers): features around J centres, gamma(0.5) weights with row 0
    and a tenth of the cells exactly 0."""
    g = torch.Generator(device="cuda").manual_seed(1000 * D + J)
    centres = torch.randn(J, D, device="cuda", generator=g) * 2 + 3
    which = torch.randint(0, J, (ROWS, FRAMES), device="cuda", generator=g)
    F = centres[which].permute(2, 0, 1) + 0.5 * torch.randn(D, ROWS, FRAMES, device="cuda", generator=g)
    w = torch._standard_gamma(torch.full((ROWS, FRAMES), 0.5, device="cuda"), generator=g)
    w[torch.rand(ROWS, FRAMES, device="cuda", generator=g) < 0.1] = 0
    w[0] = 0
    return F.float().contiguous(), w.float().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--ensemble-iters", type=int, default=30)
    ap.add_argument("--fit-only", default=None, metavar="D,J", help="one fit of 20 iterations and nothing else (for a kernel trace)")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="D,J:CSV")
    args = ap.parse_args()

    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cells = ROWS * FRAMES

    def setup(D, J):
        f, wt = inputs(D, J)
        F, w = f.cpu().numpy(), wt.cpu().numpy()
        f64 = dict(dtype=torch.float64, device="cuda")
        state = [torch.empty(J, **f64), torch.empty(J, D, **f64), torch.empty(J, D, D, **f64), torch.empty(D, **f64), torch.empty((), **f64)]
        z = torch.from_numpy(cluster.quantiles(J)).cuda()
        nbytes = lib.glowk_cluster_work_bytes(1, D, J, ROWS, FRAMES)
        work = torch.empty(nbytes // 8, **f64)
        ll = torch.empty(20, **f64)
        iters, status = torch.zeros((), dtype=torch.int32, device="cuda"), torch.zeros((), dtype=torch.int32, device="cuda")

        def fit(n):
            _lib.check(lib.glowk_cluster_fit(p(f), p(wt), 1, D, J, ROWS, FRAMES, p(z), 1e-6, n, 0.0, *[p(t) for t in state], p(ll), p(iters), p(status), p(work), nbytes, st))
        return F, w, f, wt, state, work, nbytes, status, fit

    if args.fit_only:
        D, J = (int(v) for v in args.fit_only.split(","))
        setup(D, J)[-1](20)
        torch.cuda.synchronize()
        return

    big = torch.empty(1 << 26, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(big)
    t = timed(lambda: dst.copy_(big), args.reps)
    copy_rate = 2 * big.numel() * 4 / (t["median_ms"] * 1e-3) / 1e9                       # read + write
    del big, dst
    out = dict(shape=[1, "D", ROWS, FRAMES], device=torch.cuda.get_device_name(0), copy_gb_per_s=copy_rate, workgroups=R.groups(cells))
    print("copy", copy_rate, "GB/s", flush=True)
    stats = dict((tuple(int(v) for v in s.split(":", 1)[0].split(",")), kernel_stats(s.split(":", 1)[1])) for s in args.kernel_stats)
    for D, J in CASES:
        F, w, f, wt, state, work, nbytes, status, fit = setup(D, J)
        r = dict(stats_floor_bytes_per_cell=4 * (D + 1))
        t = timed(lambda: fit(20), args.reps)
        r["iteration"] = dict((k, v / 20 if k.endswith("_ms") else v) for k, v in t.items())
        fit(3)
        S = torch.empty(cluster.stat_size(D, J), dtype=torch.float64, device="cuda")
        ll1 = torch.empty((), dtype=torch.float64, device="cuda")
        r["stats"] = with_bytes(timed(lambda: _lib.check(lib.glowk_cluster_stats(p(f), p(wt), 1, D, J, ROWS, FRAMES, *[p(t) for t in state], p(S), p(status), p(work),
                                                                                 nbytes, st)), args.reps), 4 * (D + 1) * cells, copy_rate)
        keep = [t.clone() for t in state]
        r["update"] = timed(lambda: _lib.check(lib.glowk_cluster_update(p(S), 1, D, J, 1e-6, p(keep[0]), p(keep[1]), p(keep[2]), p(state[3]), p(state[4]), p(ll1),
                                                                        p(status), p(work), nbytes, st)), args.reps)
        mask = torch.empty(J, ROWS, FRAMES, dtype=torch.float32, device="cuda")
        r["posteriors"] = with_bytes(timed(lambda: _lib.check(lib.glowk_cluster_posteriors(p(f), 1, D, J, ROWS, FRAMES, *[p(t) for t in state], None, 1, p(mask), None,
                                                                                           p(status), p(work), nbytes, st)), args.reps), 4 * (D + J) * cells, copy_rate)
        if (D, J) in stats:
            ks = [(n, v) for n, v in stats[(D, J)].items() if "k_cluster_stats" in n]
            ku = [(n, v) for n, v in stats[(D, J)].items() if "k_cluster_update" in n]
            em = max(ks, key=lambda nv: nv[1][0]) if ks else None                         # the E-step instance: the most calls
            if em and ku:
                us = em[1][1]
                r["stats_kernel"] = with_bytes(dict(average_us=us, calls=em[1][0], median_ms=us / 1e3, source="rocprofv3 --kernel-trace --stats of --fit-only"),
                                               4 * (D + 1) * cells, copy_rate)
                r["update_kernel"] = dict(average_us=ku[0][1][1], calls=ku[0][1][0])
        if not args.no_cpu and J * cluster.stat_size(D, 1) * cells * 8 < 2 << 30:     # the restatement holds [J, P, cells] at once
            ref = R.init(F, w, J)
            t0 = time.perf_counter()
            R.update(R.stats(F, w, ref), ref)
            r["numpy_iteration_s"] = time.perf_counter() - t0
        out["D%d_J%d" % (D, J)] = r
        print(D, J, r, flush=True)
        del f, wt, work, mask

    from tests import projet_ref
    X, _ = projet_ref.scene(ROWS, FRAMES, (0.2, 0.8, 1.4), 0.1)
    x = torch.from_numpy(X).cuda()
    Fs = torch.empty(1, ROWS, FRAMES, dtype=torch.float32, device="cuda")
    ws = torch.empty(ROWS, FRAMES, dtype=torch.float32, device="cuda")
    out["spatial_features"] = with_bytes(timed(lambda: _lib.check(lib.glowk_cluster_spatial_features(p(x), 1, ROWS, FRAMES, 0, 3.0, 1.0, p(Fs), p(ws), st)), args.reps),
                                         24 * cells, copy_rate)
    print("spatial_features", out["spatial_features"], flush=True)
    mag = x[0].abs().contiguous()
    names = ("melody", "repet_sim", "ft2d", "hpss")
    n = args.ensemble_iters
    out["ensemble"] = dict(timed(lambda: cluster.ensemble(mag, names, n_iter=n, tol=0.0), 3), n_iter=n, primitives=list(names))
    masks = [cluster._primitive_mask(name, {}, mag) for name in names]
    out["ensemble_without_primitives"] = dict(timed(lambda: cluster.ensemble(mag, masks, n_iter=n, tol=0.0), 3), n_iter=n)
    print("ensemble", out["ensemble"], out["ensemble_without_primitives"], flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
