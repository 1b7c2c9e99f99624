"""Times of the kernel-additive-modelling kernels (csrc/glowk_kam.h) on one GPU and the back-fit's powf error against the fp64
restatement.

Timing, at 1 x 1025 x 5626 (180 s of 16 kHz audio), HIP events around each C call on preallocated device tensors, median, minimum and
spread of --reps runs after a warm-up:

* ``glowk_kam_median`` for ``harmonic(31)``, ``percussive(31)``, ``periodic(25, 8)``, ``cross(15, 15)``, ``harmonic(127)`` and n = 127
  random offsets drawn from 64 distinct pairs (duplicates tie, and ties keep the rank counting from leaving early);
* ``glowk_kam_backfit`` at J = 3 with masks, and one ``glowk_kam_fit`` iteration at J = 3 (harmonic, percussive, periodic);
* ``glowk_median_filter`` at sizes 31 and 127 along both axes, in the same run: the nearest existing yardstick.  ``over_median_filter``
  is the sparse-kernel time over the contiguous filter's of the same size and direction: what the per-lane gather costs over a shared
  staged window.

``hbm_floor_ms`` is one read plus one write of the plane (the back-fit: 1 + J reads, 2 J writes) at the 8 TB/s peak.  ``compares`` is
n^2 per output, what rank counting performs at the most; ``lds_reads`` is n^2 / c + n per output (c = 4 candidates share a read, 8 for n > 28);
``gather_loads`` is n per output.  With --cpu, ``ref_s`` is tests/kam_ref.py's ``median`` on the host for the kernels without row
offsets: timed on a band of 128 rows (its sort of all neighbours at once needs 12 n bytes per cell) and scaled to the plane.

Accuracy (--accuracy-out): the device masks against tests/kam_ref.py's fp64 ``backfit`` of the same inputs, for J in {1, 2, 3, 8} and
power in {0.5, 1, 2, 10}, on the inputs of tests/test_gpu_kam.py.

    python scripts/kam_time.py --out profiles/kam_time.json --accuracy-out profiles/kam_accuracy.json [--reps 20] [--cpu]
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
from audiosourcesep_amd import _lib, kam  # noqa: E402

HBM_PEAK = 8.0e12                          # bytes / s
SHAPE = (1, 1025, 5626)


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


def with_floor(r, nbytes):
    floor_ms = nbytes / HBM_PEAK * 1e3
    r.update(bytes=nbytes, hbm_floor_ms=floor_ms, fraction_of_hbm_floor=floor_ms / r["median_ms"])
    return r


def accuracy():
    from tests import kam_ref as R
    from tests import test_gpu_kam as T
    out = dict(shape=[2, "J", 33, 65], cases=[])
    for power in (0.5, 1.0, 2.0, 10.0):
        for J in (1, 2, 3, 8):
            V, A = T.backfit_inputs(J)
            P, M = kam.backfit(V, A, power, return_masks=True)
            wp, wm = R.backfit(V, A, power)
            out["cases"].append(dict(power=power, J=J, max_abs_mask_error=float(np.abs(M.cpu().numpy() - wm).max()),
                                     max_abs_p_error=float(np.abs(P.cpu().numpy() - wp).max()), derived_bar=(J + 4) * 2.0 ** -24 if power in (1.0, 2.0) else None))
    for power in (0.5, 10.0):
        out["powf_max_abs_mask_error_power_%g" % power] = max(c["max_abs_mask_error"] for c in out["cases"] if c["power"] == power)
    out["note"] = ("device masks (fp32) against the fp64 restatement of tests/kam_ref.py on the same inputs; for powers 1 and 2 the bar is derived, for "
                   "the others (powf) the test's bar is four times the figure here, and at most 1e-6")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--accuracy-out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu", action="store_true", help="also time tests/kam_ref.py's median on the host")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kam_time.py measures on a GPU; none is visible")
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)   # noqa: E731
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)                                            # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = dict(device=torch.cuda.get_device_name(0), build=os.environ.get("GLOWK_BUILD") or "unknown", hbm_peak_bytes_per_s=HBM_PEAK, shape=list(SHAPE))
    gen = torch.Generator(device="cuda").manual_seed(1)
    S = torch.randn(SHAPE, device="cuda", generator=gen).abs().contiguous()
    out = torch.empty_like(S)
    nsig, rows, F = SHAPE
    cells = S.numel()

    yard = {}
    for size in (31, 127):
        for axis, label in ((0, "frames"), (1, "rows")):
            def call():
                _lib.check(lib.glowk_median_filter(p(S), nsig, rows, F, size, axis, p(out), stream))
            yard["median_filter_%s_size%d" % (label, size)] = with_floor(timed(call, args.reps), 8 * cells)
    res["yardstick"] = yard

    rng = np.random.default_rng(127)
    tables = [("harmonic_31", kam.harmonic(31), "median_filter_frames_size31"), ("percussive_31", kam.percussive(31), "median_filter_rows_size31"),
              ("periodic_25_8", kam.periodic(25, 8), None), ("cross_15_15", kam.cross(15, 15), None),
              ("harmonic_127", kam.harmonic(127), "median_filter_frames_size127"),
              ("random_127", np.stack([rng.integers(-10, 11, 64), rng.integers(-20, 21, 64)], 1)[rng.integers(0, 64, 127)].astype(np.int32), "median_filter_frames_size127")]
    med = {}
    for name, table, against in tables:
        n = len(table)

        def call():
            _lib.check(lib.glowk_kam_median(p(S), nsig, rows, F, hp(table), n, p(out), stream))
        r = with_floor(timed(call, args.reps), 8 * cells)
        r.update(n=n, compares=cells * n * n, lds_reads=cells * (n * n // (8 if n > 28 else 4) + n), gather_loads=cells * n, waves_per_workgroup=4 if n <= 64 else 1, candidates_per_pass=8 if n > 28 else 4)
        if against:
            r["over_median_filter"] = r["median_ms"] / yard[against]["median_ms"]
            r["yardstick"] = against
        if args.cpu and n <= 31 and not table[:, 0].any():                               # no row offsets: a band of rows stands alone
            from tests import kam_ref as R
            band = 128                                                                   # the sort of [n, rows, F] at once needs 12 n bytes per cell
            host = S[0, :band].cpu().numpy()
            t0 = time.perf_counter()
            want = R.median(host, table)
            r["ref_s_of_%d_rows" % band] = time.perf_counter() - t0
            r["ref_s"] = r["ref_s_of_%d_rows" % band] * rows / band
            r["equals_ref_bitwise"] = bool(np.array_equal(out[0, :band].cpu().numpy().view(np.uint32), want.view(np.uint32)))
        med[name] = r
    res["median"] = med

    J = 3
    A = torch.randn((1, J) + SHAPE[1:], device="cuda", generator=gen).abs().contiguous()
    P, M = torch.empty_like(A), torch.empty_like(A)

    def backfit():
        _lib.check(lib.glowk_kam_backfit(p(S), p(A), nsig, J, rows * F, 2.0, p(P), p(M), stream))
    res["backfit_J3"] = with_floor(timed(backfit, args.reps), 4 * cells * (1 + J + 2 * J))

    models = (kam.harmonic(31), kam.percussive(31), kam.periodic(25, 8))
    model_n = np.array([len(m) for m in models], np.int32)
    model_k = np.zeros(J, np.int32)
    offsets = np.ascontiguousarray(np.concatenate(models))
    nbytes = lib.glowk_kam_work_bytes(nsig, rows, F, J, hp(model_k))
    work = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")

    def fit():
        _lib.check(lib.glowk_kam_fit(p(S), nsig, rows, F, J, hp(model_n), hp(offsets), hp(model_k), ctypes.c_void_p(0), 1, 2.0, p(P), p(M), p(work), nbytes, stream))
    r = with_floor(timed(fit, args.reps), 4 * cells * (2 * J + 1 + J + 2 * J))
    r.update(models=["harmonic_31", "percussive_31", "periodic_25_8"], work_bytes=nbytes,
             sum_of_parts_ms=sum(med[k]["median_ms"] for k in ("harmonic_31", "percussive_31", "periodic_25_8")) + res["backfit_J3"]["median_ms"])
    res["fit_one_iteration_J3"] = r
    res["note"] = ("HIP events around each C call on preallocated device tensors, median of reps after one warm-up call; hbm_floor_ms: one read and one "
                   "write of the plane per filter at hbm_peak_bytes_per_s.  Not measured: the split of a filter's time between the gather, the LDS "
                   "reads and the compares (no counters were collected); compares, lds_reads and gather_loads are counts from the kernel's structure")
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.accuracy_out:
        acc = accuracy()
        print(json.dumps(acc, indent=1))
        with open(args.accuracy_out, "w") as f:
            f.write(json.dumps(acc, indent=1) + "\n")


if __name__ == "__main__":
    main()
