"""The benchmark's plain run as a caller sees it: `bench.py --steps K --warmup W --dump-outputs DIR` in a fresh process prints ONE
line with the headline fields and nothing of what `--full` adds, times exactly K steps, and writes the last timed step's outputs --
the same log_prob the engine gives for the benchmark's seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from audiosourcesep_amd import _lib
from audiosourcesep_amd.config import CONFIG_B
from audiosourcesep_amd.synthetic import calibrated_engine, synthetic_mel_tiles

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dumped_outputs(repo_root, tmp_path):
    n, steps = 64, 3
    cmd = [sys.executable, os.path.join(repo_root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--batch", str(n), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=repo_root)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [s for s in r.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["unit"] == "passes/s" and out["higher_is_better"] is True and out["dtype"] == "f16x3"
    assert out["steps"] == steps and out["value"] > 0
    assert out["value"] == pytest.approx(n * 1e3 / out["ms_per_step"], rel=1e-9)
    for k in ("cpu_baseline", "config_A_32x32_K16_L2", "exact_fp32", "two_term_split_fp16", "accuracy", "log_prob_32", "train_32", "basis_30"):
        assert k not in out, k

    lp = np.load(tmp_path / "out" / "log_prob.npy")
    total = np.load(tmp_path / "out" / "log_prob_total.npy")
    assert lp.dtype == np.float32 and lp.shape == (n,) and np.isfinite(lp).all()
    assert total.dtype == np.float64 and total.shape == (1,)
    np.testing.assert_allclose(total[0], lp.astype(np.float64).sum(), rtol=1e-6)

    eng, _ = calibrated_engine(CONFIG_B, device=0, init_tiles=n)
    eng.set_precision(_lib.PREC_F16X3)
    ref = eng.log_prob(torch.from_numpy(synthetic_mel_tiles(n, CONFIG_B, seed=1234)).cuda()).cpu().numpy()
    eng.close()
    np.testing.assert_allclose(lp, ref, rtol=1e-6)
