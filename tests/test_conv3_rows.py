"""The row order of conv3 in the forward image of the 16x16x32 kernels (audiosourcesep_amd/csrc/glowk_act_scale.h: glowk_conv3_row),
checked on the host: tests/conv3_rows_main.cpp verifies for c = 8 and 16 that the map is a bijection onto the 9 c (tap, channel)
pairs plus zero padding, that every (dx = -1, 0, +1) triplet sits in three consecutive registers of one lane group and one
accumulator group -- what lets the kernels add the horizontal taps before they store --, that the conv3 part of a packed image
(F = 128 and 512), read the way the kernels read it, is the split of the folded weights row by row, that the map for the device-side
refresh points at the same sources, and that c = 4 keeps the natural order half by half.
Built without HIP under AddressSanitizer + UndefinedBehaviorSanitizer, like tests/test_conv1_stacked.py."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "conv3_rows_main.cpp")


def test_conv3_rows_of_the_image_are_the_triplets_of_the_presum(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "conv3_rows")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "CONV3_ROWS_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
