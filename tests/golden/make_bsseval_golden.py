#!/usr/bin/env python3
"""Generate tests/golden/real_bsseval.npz (the real_ prefix keeps it out of the oracle-vector golden tests): BSS Eval outputs
of the reference's own ``bsseval_v4.py`` -- data only -- on

* a 2 s excerpt (int16, 16 kHz, from sample 64 000) of the ground truths and of both separations the reference ships with its
  BASIS result (basis_sep_results/beethoven_sonata_1_sep_1min/{gt1,gt2}.wav, reuse_phase/, swf/);
* synthetic cases from a fixed seed (float32): three sources, stereo, filters_len 64.

Inputs go to the reference as float64 (int16 / 32768), so that its FFTs run in double precision.  ``CASES`` (stored as JSON in
the file) says how tests/test_bsseval_cpu.py and tests/test_gpu_bsseval.py rebuild each case's inputs.  numpy 2 removed the
``np.float`` alias the reference uses, hence the shim.  Run from the repo root (needs the reference checkout and scipy):
    python tests/golden/make_bsseval_golden.py
"""
import json
import os
import sys
import wave

import numpy as np

REF = "/root/reference"
RES = os.path.join(REF, "basis_sep_results", "beethoven_sonata_1_sep_1min")
DST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "real_bsseval.npz")
START, LEN = 64000, 32000

# name -> (function, reference input, estimate input, keyword arguments); inputs name arrays of the file, with optional edits
CASES = [
    dict(name="v4_perm_swapped", fn="bss_eval", ref="gt", est="reuse", swap=True,
         kw=dict(window=8000, hop=6000, compute_permutation=True)),
    dict(name="sources", fn="bss_eval_sources", ref="gt", est="swf", kw={}),
    dict(name="images_framewise", fn="bss_eval_images_framewise", ref="gt", est="swf", kw=dict(window=15000, hop=15000)),
    dict(name="sources_framewise", fn="bss_eval_sources_framewise", ref="gt", est="reuse", kw=dict(window=12000, hop=9000)),
    dict(name="silent_window", fn="bss_eval", ref="gt", est="reuse", zero=[1, 8000, 16000], kw=dict(window=8000, hop=8000)),
    dict(name="one_window", fn="bss_eval", ref="gt", est="swf", kw=dict(window=40000, hop=40000)),
    dict(name="three_sources", fn="bss_eval", ref="syn3_ref", est="syn3_est",
         kw=dict(window=1200, hop=900, compute_permutation=True, framewise_filters=True)),
    dict(name="stereo", fn="bss_eval", ref="st_ref", est="st_est", kw=dict(window=1000, hop=500)),
    dict(name="filters_len_64", fn="bss_eval", ref="l64_ref", est="l64_est",
         kw=dict(window=900, hop=900, filters_len=64, framewise_filters=True, bsseval_sources_version=True)),
]


def read(path):
    with wave.open(path, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    return pcm[START:START + LEN]


def synthetic(rng, nsrc, n, nchan, alpha=0.15, noise=0.02):
    """Sources: white noise through random 24-tap FIRs per channel; estimates: a short FIR image of the source plus alpha times
    the next source plus white noise."""
    src = np.empty((nsrc, n, nchan))
    for j in range(nsrc):
        for c in range(nchan):
            src[j, :, c] = np.convolve(rng.standard_normal(n), rng.standard_normal(24) / 5.0, mode="same")
    est = np.empty_like(src)
    for j in range(nsrc):
        for c in range(nchan):
            est[j, :, c] = np.convolve(src[j, :, c], [1.0, 0.3, -0.1], mode="full")[:n] + alpha * src[(j + 1) % nsrc, :, c]
    est += noise * rng.standard_normal(est.shape)
    return src.astype(np.float32), est.astype(np.float32)


def inputs(data, case):
    """float64 (reference, estimate) of a case from the arrays of the file."""
    def conv(a):
        return a.astype(np.float64) / 32768.0 if a.dtype == np.int16 else a.astype(np.float64)
    ref, est = conv(data[case["ref"]]), conv(data[case["est"]])
    if case.get("swap"):
        est = est[::-1].copy()
    if "zero" in case:
        j, a, b = case["zero"]
        est[j, a:b] = 0.0
    return ref, est


if __name__ == "__main__":
    import scipy  # noqa: F401  (the reference needs it)
    np.float = float
    sys.path.insert(0, REF)
    import bsseval_v4 as B
    rng = np.random.default_rng(20261016)
    data = dict(gt=np.stack([read(os.path.join(RES, "gt1.wav")), read(os.path.join(RES, "gt2.wav"))]),
                reuse=np.stack([read(os.path.join(RES, "reuse_phase", "sep1.wav")), read(os.path.join(RES, "reuse_phase", "sep2.wav"))]),
                swf=np.stack([read(os.path.join(RES, "swf", "sep1.wav")), read(os.path.join(RES, "swf", "sep2.wav"))]))
    data["syn3_ref"], data["syn3_est"] = synthetic(rng, 3, 2500, 1)
    data["st_ref"], data["st_est"] = synthetic(rng, 2, 2500, 2)
    data["l64_ref"], data["l64_est"] = synthetic(rng, 2, 2500, 1)
    data["syn3_ref"], data["syn3_est"] = data["syn3_ref"][..., 0], data["syn3_est"][..., 0]
    data["l64_ref"], data["l64_est"] = data["l64_ref"][..., 0], data["l64_est"][..., 0]
    out = dict(data)
    for case in CASES:
        ref, est = inputs(data, case)
        res = getattr(B, case["fn"])(ref, est, **case["kw"])
        names = ("sdr", "isr", "sir", "sar", "perm") if len(res) == 5 else ("sdr", "sir", "sar", "perm")
        for k, v in zip(names, res):
            out["%s/%s" % (case["name"], k)] = np.asarray(v)
        print(case["name"], {k: np.round(np.asarray(v), 3).tolist() for k, v in zip(names, res)})
    out["cases"] = np.array(json.dumps(CASES))
    out["source"] = np.array(["SamArgt/AudioSourceSep bsseval_v4.py outputs; audio from basis_sep_results/beethoven_sonata_1_sep_1min "
                              "(gt1/gt2, reuse_phase/, swf/), samples %d..%d, int16" % (START, START + LEN)])
    np.savez_compressed(DST, **out)
    print(DST, os.path.getsize(DST), "bytes")
