"""The conv1 operands of the forward image of the 16x16x32 kernels, stacked along K (audiosourcesep_amd/csrc/glowk_act_scale.h:
glowk_conv1_stacked), checked on the host: tests/conv1_stacked_main.cpp packs the level shapes c = 4, 8, 16 at F = 128 and 512, reads
the image as the kernels read it and compares the fp64 sum over the slots with the fp64 convolution of the weights the packer split,
within 2^-20 * sum_k |w_k x_k| per output row (derived in the driver); the zero tail and the map for the device-side refresh too.
Built without HIP under AddressSanitizer + UndefinedBehaviorSanitizer, like tests/test_pack_sanitizers.py."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "conv1_stacked_main.cpp")


def test_conv1_image_against_fp64_convolution(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "conv1_stacked")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    print(r.stdout)
    assert r.returncode == 0 and "CONV1_STACKED_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
