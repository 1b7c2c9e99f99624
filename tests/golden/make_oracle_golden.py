#!/usr/bin/env python3
"""Generate tests/golden/real_oracle.npz (the real_ prefix keeps it out of the oracle-vector golden tests): outputs of the
reference's own ``oracle_systems.py`` (sigsep-mus-oracle's IBM / IRM / MWF and the two mel variants) -- data only -- on

* a 1 s excerpt (16 000 samples, not a multiple of 1024; int16, 16 kHz) of the ground truths the reference ships with its BASIS
  result (basis_sep_results/beethoven_sonata_1_sep_1min/gt1.wav, gt2.wav), mono, the mixture being their sum;
* a stereo case built from the same excerpt by ``stereo`` below: fixed dyadic pans (exact in float32) and integer
  inter-channel delays of 3 and 5 samples, which make each source's spatial covariance full rank;
* one dB tile of tests/golden/real_mel_tiles.npz (+ 100 dB, so that they are non-negative) for the mel variants.

The excerpt starts at the first whole second from sample 64 000 (the start of make_bsseval_golden.py) where no IBM bin of
either stored IBM case has its ratio within a relative 1e-4 of theta (``margin`` records the smallest |ratio - theta| / theta):
the GPU computes the spectra in fp32, which must not flip a mask bit of the fixture.  At 64 000 itself the margins are 4e-5
and 8e-5.

Inputs go to the reference as float64 (int16 / 32768); outputs are stored as float32.  Shims, all at generation time:
* numpy 2 removed the ``np.float`` alias the reference uses;
* the reference's IRM reads ``source.audio``: the sources go in as an ndarray subclass with an ``.audio`` property;
* the reference's MWF reuses its loop index ``i`` as the channel index, so every estimate lands in slot nchan - 1 = 1 and the
  last source's estimate wins: it is called once per source with that source moved to the last slot (with two sources, slot 1),
  so the reference itself computes every source's estimate.
Run from the repo root (needs the reference checkout and scipy):
    python tests/golden/make_oracle_golden.py
"""
import os
import sys
import wave

import numpy as np

REF = "/root/reference"
RES = os.path.join(REF, "basis_sep_results", "beethoven_sonata_1_sep_1min")
HERE = os.path.dirname(os.path.abspath(__file__))
DST = os.path.join(HERE, "real_oracle.npz")
START0, STEP, LEN, LEAD = 64000, 16000, 16000, 8      # LEAD samples before the excerpt feed the stereo delays
IBM_CASES = [(1, 0.5), (2, 0.3)]                      # (alpha, theta)
MARGIN = 1e-4
PANS = [(0.75, 0.5), (0.25, 0.875)]                   # source j: (left gain, right gain)
DELAYS = [(0, 3), (5, 0)]                             # source j: (left delay, right delay) in samples
MEL_TILES = 1


def stereo(gt):
    """int16 [2, LEAD + LEN] -> float64 stereo sources [2, LEN, 2] (the mixture is their sum)."""
    x = gt.astype(np.float64) / 32768.0
    out = np.empty((2, LEN, 2))
    for j in range(2):
        for c in range(2):
            d = DELAYS[j][c]
            out[j, :, c] = PANS[j][c] * x[j, LEAD - d:LEAD - d + LEN]
    return out


def mono(gt):
    return (gt[:, LEAD:].astype(np.float64) / 32768.0)[:, :, None]


def mel_inputs(tiles):
    """(mixture [2, 96, 64], sources [2, 2, 96, 64]) float32 from real_mel_tiles.npz."""
    off = np.float32(100.0)
    return tiles["mixed"][:MEL_TILES] + off, np.stack([tiles["gt1"][:MEL_TILES] + off, tiles["gt2"][:MEL_TILES] + off])


def read(path):
    with wave.open(path, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


def ibm_margin(mix, src, alpha, theta):
    from scipy.signal import stft
    X = stft(mix.T, nperseg=2048)[-1]
    Y = stft(src.transpose(0, 2, 1), nperseg=2048)[-1]
    ratio = np.abs(Y) ** alpha / (np.finfo(np.float64).eps + np.abs(X) ** alpha)
    return float(np.min(np.abs(ratio - theta) / theta))


class _Audio(np.ndarray):
    @property
    def audio(self):
        return np.asarray(self)


if __name__ == "__main__":
    np.float = float
    sys.path.insert(0, REF)
    import oracle_systems as O
    full = np.stack([read(os.path.join(RES, "gt1.wav")), read(os.path.join(RES, "gt2.wav"))])
    for start in range(START0, full.shape[1] - LEN, STEP):
        gt = full[:, start - LEAD:start + LEN].copy()
        s = mono(gt)
        margins = [ibm_margin(s.sum(0), s, a, t) for a, t in IBM_CASES]
        if min(margins) > MARGIN:
            break
    print("start", start, "IBM margins", margins)
    assert min(margins) > MARGIN
    out = dict(gt=gt, start=np.int64(start), margin=np.array(margins))
    ms = mono(gt)
    mm = ms.sum(0)
    for a, t in IBM_CASES:
        out["IBM_a%g_t%g" % (a, t)] = O.IBM(mm, ms, alpha=a, theta=t).astype(np.float32)
    ss = stereo(gt)
    sm = ss.sum(0)
    out["IRM"] = O.IRM(sm, ss.view(_Audio)).astype(np.float32)
    mwf = np.empty_like(ss)
    for j in range(2):
        order = [k for k in range(2) if k != j] + [j]
        mwf[j] = O.MWF(sm, ss[order])[1]
    out["MWF"] = mwf.astype(np.float32)
    mix_m, src_m = mel_inputs(np.load(os.path.join(HERE, "real_mel_tiles.npz")))
    out["IBM_melspec"] = O.IBM_melspec(mix_m, src_m)
    out["IRM_melspec"] = O.IRM_melspec(mix_m, src_m)
    assert out["IBM_melspec"].dtype == np.float32 and out["IRM_melspec"].dtype == np.float32
    out["source"] = np.array(["SamArgt/AudioSourceSep oracle_systems.py outputs; audio from basis_sep_results/beethoven_sonata_1_sep_1min "
                              "(gt1/gt2), samples %d..%d (with %d lead samples), int16; mel tiles from real_mel_tiles.npz + 100 dB"
                              % (start, start + LEN, LEAD)])
    np.savez_compressed(DST, **out)
    print(DST, os.path.getsize(DST), "bytes")
