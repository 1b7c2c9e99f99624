"""Times of the PROJET kernels (csrc/glowk_projet.h) on one GPU.

One stereo STFT of 1 x 2 x 1025 x 5626 (180 s of 16 kHz audio): four panned sources of tests/projet_ref.py's scene; J = 4, M = 15,
L = 41, alpha = 1, for beta 0, 1 and 2.  HIP events around the C entries on preallocated device tensors (no allocation, no copy in
the timed region): median, minimum and spread of --reps runs after a warm-up.  ``iteration`` is glowk_projet_fit at 20 iterations
over 20 (the fused pass and the Q kernel, the one launch of the gains amortised), ``update_p`` the P pass alone, ``update_q`` the
sums-only pass and the Q kernel, ``separate`` the filter, ``projet`` the whole of ``projet.projet`` at 100 iterations (start, fit,
filter, allocations included).  ``numpy_s`` is the host's time for the fp64 restatement of the same 100 iterations, measured on
--numpy-iters iterations and scaled.

HIP events cannot split the two launches of an iteration.  The kernels' own times come from a kernel trace of a run that does nothing
but one fit per beta; its summary is merged with --kernel-stats and gives ``fused_kernel``: microseconds, bytes per second over the
16 + 16 J bytes a cell moves, and the fraction of the HBM copy rate:

    rocprofv3 --kernel-trace --stats --output-format csv -d rocprof_out -- python scripts/projet_time.py --fit-only --beta 1
    python scripts/projet_time.py --out profiles/projet_time.json [--kernel-stats beta:file.csv ...] [--bounds file.json] [--no-cpu]

--bounds merges the largest measured fractions of the tests' bounds (tests/test_gpu_projet.py prints them).
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
from audiosourcesep_amd import _lib, projet  # noqa: E402
from tests import projet_ref as R  # noqa: E402

ROWS, FRAMES, J, M, L, ALPHA = 1025, 5626, 4, 15, 41, 1.0
PANS = (0.1, 0.5, 0.95, 1.4)
COPY_GB_PER_S = 6300.0            # what a device-to-device copy of this size reaches on the MI355X (profiles/README.md)
FP64_VALU_TFLOPS = 78.6           # the fp64 vector peak, a fused multiply-add counted as two


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


def with_bytes(t, nbytes, key="median_ms"):
    rate = nbytes / (t[key] * 1e-3) / 1e9
    return dict(t, bytes=int(nbytes), gb_per_s=rate, copy_gb_per_s=COPY_GB_PER_S, of_copy_rate=rate / COPY_GB_PER_S)


def kernel_stats(path):
    """name -> (calls, average microseconds) from a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projet_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--numpy-iters", type=int, default=1)
    ap.add_argument("--fit-only", action="store_true", help="one fit of 20 iterations and nothing else (for a kernel trace)")
    ap.add_argument("--beta", type=int, default=1, help="the beta of --fit-only")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="BETA:CSV")
    ap.add_argument("--bounds", default=None)
    args = ap.parse_args()

    X_host, _ = R.scene(ROWS, FRAMES, PANS, 0.25)
    x = torch.from_numpy(X_host).cuda()
    tab = projet.tables(M, L, ALPHA)
    lib = _lib.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    U, K, Up = dev(tab["U"]), dev(tab["K"]), dev(tab["Up"])
    P0, Q0 = projet.init(x, J, tab)
    P, Q = P0.clone(), Q0.clone()
    G = torch.empty((M, J), dtype=torch.float64, device="cuda")
    Y = torch.empty((J, 2, ROWS, FRAMES), dtype=torch.complex64, device="cuda")
    nbytes = lib.glowk_projet_workspace_bytes(1, M, J, ROWS, FRAMES)
    work = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cells = ROWS * FRAMES

    def fit(beta, n):
        _lib.check(lib.glowk_projet_fit(p(x), 1, ROWS, FRAMES, p(U), p(K), M, L, J, ALPHA, beta, n, p(P), p(Q), p(G), p(work), nbytes, st))

    if args.fit_only:
        fit(args.beta, 20)
        torch.cuda.synchronize()
        return

    out = dict(shape=[1, 2, ROWS, FRAMES], J=J, M=M, L=L, alpha=ALPHA, device=torch.cuda.get_device_name(0), workgroups=nbytes // (16 * M * J),
               fused_bytes_per_cell=16 + 16 * J, fp64_valu_peak_tflops=FP64_VALU_TFLOPS)
    stats = dict((int(s.split(":", 1)[0]), kernel_stats(s.split(":", 1)[1])) for s in args.kernel_stats)
    for beta in (0, 1, 2):
        r = {}

        def reset():
            P.copy_(P0)
            Q.copy_(Q0)

        reset()
        t = timed(lambda: fit(beta, 20), args.reps)
        r["iteration"] = dict((k, v / 20 if k.endswith("_ms") else v) for k, v in t.items())
        reset()
        fit(beta, 3)                                                                     # a state a few iterations in, for the staged calls
        r["update_p"] = with_bytes(timed(lambda: _lib.check(lib.glowk_projet_update_p(p(x), 1, ROWS, FRAMES, p(U), p(G), M, J, ALPHA, beta, p(P), st)), args.reps),
                                   (16 + 16 * J) * cells)
        reset()
        fit(beta, 3)
        r["update_q"] = with_bytes(timed(lambda: _lib.check(lib.glowk_projet_update_q(p(x), p(P), 1, ROWS, FRAMES, p(U), p(K), M, L, J, ALPHA, beta, p(Q), p(G), p(work),
                                                                                      nbytes, st)), args.reps), (16 + 8 * J) * cells)
        if beta in stats:
            fused = [(n, v) for n, v in stats[beta].items() if "k_projet_iterate" in n]
            qk = [(n, v) for n, v in stats[beta].items() if "k_projet_q" in n]
            if fused and qk:
                us = fused[0][1][1]
                r["fused_kernel"] = with_bytes(dict(average_us=us, calls=fused[0][1][0], median_ms=us / 1e3, source="rocprofv3 --kernel-trace --stats of --fit-only"),
                                               (16 + 16 * J) * cells)
                r["q_kernel"] = dict(average_us=qk[0][1][1], calls=qk[0][1][0])
        out["beta_%d" % beta] = r
        print("beta", beta, r, flush=True)
    reset()
    fit(1, 20)
    out["separate"] = with_bytes(timed(lambda: _lib.check(lib.glowk_projet_separate(p(x), p(P), 1, ROWS, FRAMES, p(U), p(Up), p(G), M, J, p(Y), st)), args.reps),
                                 (16 + 8 * J + 16 * J) * cells)
    print("separate", out["separate"], flush=True)
    whole = {}

    def run():
        whole["Y"], whole["model"] = projet.projet(x, J, M, L, ALPHA, 1, 100, return_model=True)

    out["projet"] = dict(timed(run, 3), n_iter=100)
    out["pans"] = whole["model"]["pans"].cpu().numpy().tolist()
    out["true_pans"] = list(PANS)
    print("projet", out["projet"], out["pans"], flush=True)
    if not args.no_cpu:
        rt = R.tables(M, L, ALPHA)
        Vr = R.projections(X_host, rt)
        Pr, Qr = R.init(X_host, J, rt)
        t0 = time.perf_counter()
        for _ in range(args.numpy_iters):
            Pr, Qr = R.step(Vr, Pr, Qr, rt["K"], 1)
        dt = time.perf_counter() - t0
        out["numpy_s"] = dt / args.numpy_iters * 100
        out["numpy_iterations_measured"] = args.numpy_iters
        print("numpy, 100 iterations (scaled)", out["numpy_s"], flush=True)
    if args.bounds:
        with open(args.bounds) as f:
            out["largest_fraction_of_each_bound"] = json.load(f)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
