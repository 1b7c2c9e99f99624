"""Times of the RPCA kernels (csrc/glowk_rpca.h) on one GPU.

One spectrogram of 1 x 1025 x 5626 (180 s of 16 kHz audio): the synthetic scene of tests/rpca_ref.py (rank 8 plus 6 % sparse).  HIP
events around each call of ``audiosourcesep_amd.rpca`` on device tensors (the calls allocate their workspace from torch's cache):
median, minimum and spread of --reps runs after a warm-up; the solve and the whole fit run --slow-reps times.  ``flop`` counts what a
product executes (the symmetric forms only their 64 x 64 tiles on and above the diagonal) and ``of_peak`` is that over the median
against the MI355X's fp64 matrix peak (78.6 Tflop/s).  ``round_us`` is the solve's time over its sweeps x rounds: two launches each.
``numpy_s`` is the host's time for the fp64 restatement (SVD route) of the same chain.

    python scripts/rpca_time.py --out profiles/rpca_time.json [--reps 10] [--slow-reps 2] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiosourcesep_amd import rpca  # noqa: E402
from tests import rpca_ref as R  # noqa: E402

ROWS, FRAMES, RANK = 1025, 5626, 8
FP64_MFMA_TFLOPS = 78.6
COPY_GB_PER_S = 6300.0


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


def with_flop(t, flop):
    return dict(t, flop=int(flop), tflops=flop / (t["median_ms"] * 1e-3) / 1e12, of_peak=flop / (t["median_ms"] * 1e-3) / 1e12 / FP64_MFMA_TFLOPS)


def with_bytes(t, nbytes):
    return dict(t, bytes=int(nbytes), gb_per_s=nbytes / (t["median_ms"] * 1e-3) / 1e9, copy_gb_per_s=COPY_GB_PER_S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rpca_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--slow-reps", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    Lt, St = R.scene(ROWS, FRAMES, rank=RANK)
    M_host = (Lt + St).astype(np.float32)
    M = torch.from_numpy(M_host).cuda()
    A = M.double()
    tiles = -(-ROWS // 64)
    upper = tiles * (tiles + 1) // 2 * 64 * 64
    out = dict(shape=[1, ROWS, FRAMES], rank=RANK, device=torch.cuda.get_device_name(0), fp64_mfma_peak_tflops=FP64_MFMA_TFLOPS)

    out["gram"] = with_flop(timed(lambda: rpca.gram(A), args.reps), 2 * upper * FRAMES)
    print("gram", out["gram"], flush=True)
    G = rpca.gram(A)
    solve = {}

    def run_solve():
        solve["l"], solve["V"], solve["sweeps"] = rpca.eigh(G)

    t = timed(run_solve, args.slow_reps)
    sweeps, rounds = int(solve["sweeps"]), ROWS + (ROWS & 1) - 1
    out["solve"] = dict(t, n=ROWS, sweeps=sweeps, rounds_per_sweep=rounds, launches=2 * sweeps * rounds, round_us=t["median_ms"] * 1e3 / (sweeps * rounds))
    print("solve", out["solve"], flush=True)
    g = torch.rand(ROWS, dtype=torch.float64, device="cuda")
    out["scaled_gram"] = with_flop(timed(lambda: rpca.scaled_gram(solve["V"], g), args.reps), 2 * upper * ROWS)
    P = rpca.scaled_gram(solve["V"], g)
    out["apply"] = with_flop(timed(lambda: rpca.matmul(P, A), args.reps), 2 * (tiles * 64) * (-(-FRAMES // 64) * 64) * ROWS)
    out["shrink"] = with_bytes(timed(lambda: rpca.shrink(A, 0.1), args.reps), 16 * ROWS * FRAMES)
    for k in ("scaled_gram", "apply", "shrink"):
        print(k, out[k], flush=True)
    out["svt"] = timed(lambda: rpca.svt(A, 1.0), args.slow_reps)
    print("svt", out["svt"], flush=True)

    fit = {}

    def run_fit():
        fit["L"], fit["S"], fit["it"], fit["status"] = rpca.rpca_fit(M, return_status=True)

    t = timed(run_fit, 1)
    L, S = fit["L"].cpu().numpy(), fit["S"].cpu().numpy()
    out["fit"] = dict(t, iterations=int(fit["it"]), status=int(fit["status"]), ms_per_iteration=t["median_ms"] / max(int(fit["it"]), 1),
                      rel_err_L=float(np.linalg.norm(L - Lt) / np.linalg.norm(Lt)), rel_err_S=float(np.linalg.norm(S - St) / np.linalg.norm(St)))
    print("fit", out["fit"], flush=True)
    if not args.no_cpu:
        t0 = time.perf_counter()
        Lr, Sr, itr = R.rpca(M_host.astype(np.float64))
        out["numpy_s"] = time.perf_counter() - t0
        out["numpy_iterations"] = itr
        out["fit_against_numpy"] = dict(L=float(np.abs(L - Lr).max() / np.abs(Lr).max()), S=float(np.abs(S - Sr).max() / np.abs(Lr).max()))
        print("numpy", out["numpy_s"], itr, out["fit_against_numpy"], flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
