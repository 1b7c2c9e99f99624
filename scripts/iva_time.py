"""Times of the AuxIVA / ILRMA kernels (csrc/glowk_iva.h) on one GPU.

One stereo STFT of 2 x 1025 x 5626 (180 s of 16 kHz audio): two sources with NMF-structured variances under a random complex mixing
matrix per row, drawn on the device.  HIP events around each C call on preallocated device tensors: median, minimum and spread of
--reps runs after a warm-up.  ``per_iteration_ms`` is a fit of ``--iters`` iterations over their number.  ``bytes`` is what a pass must
move (a pass over X reads 8 B per cell and channel; the weights, the covariances, the power planes and the images add what they
read and write) and ``gb_per_s`` that over the median, next to ``copy_gb_per_s``, the copy rate an MI355X reaches from HBM (6.3 TB/s of
its 8 TB/s peak); X (92 MB) fits the 256 MiB Infinity Cache, so a pass may read faster than that.  The launches inside one C call are timed from
the kernel records of one profiled call (torch.profiler; null where it gives none).  ``numpy_s`` is the host's time for one iteration
of the fp64 restatement (tests/iva_ref.py) on the same array.

    python scripts/iva_time.py --out profiles/iva_time.json [--reps 10] [--iters 10] [--no-cpu]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiosourcesep_amd import _lib, iva  # noqa: E402
from tests import iva_ref as I  # noqa: E402

M, ROWS, FRAMES, K = 2, 1025, 5626, 4
COPY_GB_PER_S = 6300.0
KERNELS = ("k_iva_norms", "k_iva_phi", "k_iva_cov", "k_iva_power", "k_nmf_update_w", "k_nmf_w_finish", "k_nmf_update_h", "k_iva_lambda", "k_iva_scale",
           "k_iva_inverse", "k_iva_demix")


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


def with_bytes(t, nbytes):
    return dict(t, bytes=int(nbytes), gb_per_s=nbytes / (t["median_ms"] * 1e-3) / 1e9, copy_gb_per_s=COPY_GB_PER_S)


def kernel_ms(call):
    """{kernel name: mean duration in ms over its launches} of one call, or {} where the profiler records no kernels."""
    try:
        from torch.profiler import ProfilerActivity, profile
        call()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            for name in KERNELS:
                if name in ev.name:
                    out.setdefault(name, []).append((ev.time_range.end - ev.time_range.start) / 1e3)
        return {k: float(np.mean(v)) for k, v in out.items()}
    except Exception as e:                  # the timings above do not depend on it
        print("kernel records unavailable: %r" % (e,), file=sys.stderr)
        return {}


def scene(gen):
    """[M, ROWS, FRAMES] complex64 on the GPU: tests/iva_ref.scene's construction, drawn on the device."""
    def rnd(*s):
        return torch.rand(s, device="cuda", generator=gen, dtype=torch.float64)

    def nrm(*s):
        return torch.randn(s, device="cuda", generator=gen, dtype=torch.float64)
    B = rnd(M, ROWS, 2) + 0.05
    A = rnd(M, 2, FRAMES) ** 4 * (rnd(M, 2, FRAMES) < 0.6) + 1e-3
    S = torch.sqrt(B @ A) * torch.complex(nrm(M, ROWS, FRAMES), nrm(M, ROWS, FRAMES)) / np.sqrt(2.0)
    mix = torch.complex(nrm(ROWS, M, M), nrm(ROWS, M, M))
    return torch.einsum("fmk,kft->mft", mix, S).to(torch.complex64).contiguous(), mix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true", help="leave out the host's time for the numpy restatement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("iva_time.py measures on a GPU; none is visible")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = dict(device=torch.cuda.get_device_name(0), build=os.environ.get("GLOWK_BUILD") or "unknown", shape=[M, ROWS, FRAMES], components=K,
               iters=args.iters)
    gen = torch.Generator(device="cuda").manual_seed(1)
    X, mix = scene(gen)
    cells = ROWS * FRAMES
    xb, wb = cells * M * 8, ROWS * M * M * 16
    w0 = iva.init(X)
    w = w0.clone()
    phi = torch.empty((M, FRAMES), dtype=torch.float64, device="cuda")
    V = torch.empty((ROWS, M, M, M), dtype=torch.complex128, device="cuda")
    P = torch.empty((M, ROWS, FRAMES), dtype=torch.float32, device="cuda")
    Y = torch.empty_like(X)
    img = torch.empty((M, M, ROWS, FRAMES), dtype=torch.complex64, device="cuda")
    winv = torch.empty_like(w0)
    nb_a, nb_i = lib.glowk_iva_workspace_bytes(1, M, ROWS, FRAMES), lib.glowk_ilrma_workspace_bytes(1, M, ROWS, FRAMES, K)
    work = torch.empty(max(nb_a, nb_i) // 8 + 2, dtype=torch.float64, device="cuda")
    b0, a0 = iva.init_factors(iva.power(X, w0), K, seed=0)
    b, a = b0.clone(), a0.clone()
    nrb = -(-ROWS // -(-ROWS // min(-(-ROWS // 32), 32)))

    def weights():
        _lib.check(lib.glowk_iva_weights(p(X), p(w), 1, M, ROWS, FRAMES, 0, p(phi), p(work), nb_a, stream))

    def cov():
        _lib.check(lib.glowk_iva_covariances(p(X), 1, M, ROWS, FRAMES, p(phi), None, None, 0, p(V), stream))

    def cov_factors():
        _lib.check(lib.glowk_iva_covariances(p(X), 1, M, ROWS, FRAMES, None, p(b), p(a), K, p(V), stream))

    def ip():
        _lib.check(lib.glowk_iva_ip_update(p(w), p(V), 1, M, ROWS, stream))

    def auxiva_fit(n):
        w.copy_(w0)
        _lib.check(lib.glowk_auxiva_fit(p(X), p(w), 1, M, ROWS, FRAMES, 0, n, p(work), nb_a, stream))

    def ilrma_fit(n):
        w.copy_(w0)
        b.copy_(b0)
        a.copy_(a0)
        _lib.check(lib.glowk_ilrma_fit(p(X), p(w), p(b), p(a), 1, M, ROWS, FRAMES, K, n, p(work), nb_i, stream))

    def power():
        _lib.check(lib.glowk_iva_power(p(X), p(w), 1, M, ROWS, FRAMES, p(P), stream))

    def normalize():
        _lib.check(lib.glowk_iva_normalize(p(X), p(w), p(b), 1, M, ROWS, FRAMES, K, p(work), nb_a, stream))

    def demix():
        _lib.check(lib.glowk_iva_demix(p(X), p(w), 1, M, ROWS, FRAMES, p(Y), stream))

    def images():
        _lib.check(lib.glowk_iva_inverse(p(w), 1, M, ROWS, p(winv), stream))
        _lib.check(lib.glowk_iva_images(p(X), p(w), p(winv), 1, M, ROWS, FRAMES, p(Y), p(img), stream))

    auxiva_fit(3)                                                # the stages are timed on a W that has moved off the identity
    part = nrb * M * FRAMES * 8
    res["weights"] = with_bytes(timed(weights, args.reps), xb + wb + 2 * part + M * FRAMES * 8)
    res["covariances"] = with_bytes(timed(cov, args.reps), xb + M * FRAMES * 8 + wb * M)
    res["covariances_factors"] = with_bytes(timed(cov_factors, args.reps), xb + M * K * (ROWS + FRAMES) * 4 + wb * M)
    res["ip_update"] = timed(ip, args.reps)
    res["power"] = with_bytes(timed(power, args.reps), xb + wb + cells * M * 4)
    res["normalize"] = with_bytes(timed(normalize, args.reps), xb + 2 * wb + 2 * part)
    res["demix"] = with_bytes(timed(demix, args.reps), 2 * xb + wb)
    res["images"] = with_bytes(timed(images, args.reps), 2 * xb + M * xb + 3 * wb)
    one, many = timed(lambda: auxiva_fit(1), args.reps), timed(lambda: auxiva_fit(1 + args.iters), args.reps)
    res["auxiva"] = dict(first_iteration=one, fit=many, per_iteration_ms=(many["median_ms"] - one["median_ms"]) / args.iters,
                         pass_bytes=3 * xb, launches_per_iteration=3)
    res["auxiva"]["gb_per_s"] = 2 * xb / (res["auxiva"]["per_iteration_ms"] * 1e-3) / 1e9          # two passes over X per iteration
    one, many = timed(lambda: ilrma_fit(1), args.reps), timed(lambda: ilrma_fit(1 + args.iters), args.reps)
    res["ilrma"] = dict(first_iteration=one, fit=many, per_iteration_ms=(many["median_ms"] - one["median_ms"]) / args.iters, launches_per_iteration=9)
    ka, ki = kernel_ms(lambda: auxiva_fit(2)), kernel_ms(lambda: ilrma_fit(2))
    kb = dict(k_iva_norms=xb + wb + part, k_iva_phi=part + M * FRAMES * 8, k_iva_cov=xb + M * FRAMES * 8 + 2 * wb, k_iva_power=xb + wb + cells * M * 4)
    res["kernels"] = dict(auxiva={k: dict(ms=v, gb_per_s=kb[k] / (v * 1e-3) / 1e9 if k in kb else None) for k, v in ka.items()},
                          ilrma={k: dict(ms=v, gb_per_s=kb[k] / (v * 1e-3) / 1e9 if k in kb and k != "k_iva_cov" else None) for k, v in ki.items()})
    auxiva_fit(30)
    res["interference_db_after_30_auxiva"] = float(I.interference_db(w.cpu().numpy(), mix.cpu().numpy()))
    if not args.no_cpu:
        host, Wh = X.cpu().numpy(), w.cpu().numpy()
        bh, ah = b0.cpu().numpy(), a0.cpu().numpy()
        t0 = time.perf_counter()
        I.auxiva_step(host, Wh)
        t1 = time.perf_counter()
        I.ilrma_step(host, Wh, bh, ah)
        t2 = time.perf_counter()
        res["numpy_s"] = dict(auxiva_iteration=t1 - t0, ilrma_iteration=t2 - t1)
    res["note"] = ("HIP events around each C call on preallocated device tensors, median of reps after one warm-up call; per_iteration_ms: the "
                   "fit of 1 + iters iterations minus the fit of one, over iters (the copies that reset the state cancel); kernels: mean "
                   "duration of the launches of one profiled two-iteration call; bytes: what the pass must move; numpy_s: one iteration of "
                   "the fp64 restatement of the same array on the host")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
