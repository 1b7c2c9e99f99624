#!/usr/bin/env python3
"""Generate tests/golden/real_audio_excerpt.npz (the real_ prefix keeps it out of the oracle-vector golden tests): six 2.04 s
extracts (int16, 16 kHz) of the mixture wav the reference ships with its BASIS result (basis_sep_results/beethoven_sonata_1_sep_1min/mix.wav), starting after the two extracts get_song_extract skips --
data only, realistic test audio for the front end and the inversion (tests/test_gpu_audio.py).  That wav is itself a per-tile
inversion, not the original recording, so it is input for the tests, never a pin of the front end's output; only its length
(30 tiles x 32 256 samples) is recorded.  Run from the repo root (needs /root/reference):
    python tests/golden/make_audio_excerpt.py
"""
import os
import wave

import numpy as np

SRC = "/root/reference/basis_sep_results/beethoven_sonata_1_sep_1min/mix.wav"
DST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "real_audio_excerpt.npz")
EXTRACT, SKIP, COUNT = 32640, 2, 6

if __name__ == "__main__":
    with wave.open(SRC, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
        n = w.getnframes()
        pcm = np.frombuffer(w.readframes(n), dtype="<i2")
    cut = pcm[SKIP * EXTRACT:(SKIP + COUNT) * EXTRACT].reshape(COUNT, EXTRACT)
    np.savez_compressed(DST, pcm=cut, source_frames=np.array(n),
                        source=np.array(["SamArgt/AudioSourceSep basis_sep_results/beethoven_sonata_1_sep_1min/mix.wav "
                                         "(int16, extracts %d..%d of %d samples)" % (SKIP, SKIP + COUNT - 1, EXTRACT)]))
    print(DST, os.path.getsize(DST), "bytes,", n, "frames in the source")
