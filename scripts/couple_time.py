"""Launches of the one-lane coupling kernel k_couple<C, false> (batches of >= 2 x compute units tiles) at 4, 8, 16 and 32 channels, for
a kernel trace:  rocprofv3 --kernel-trace --stats --output-format csv -- python scripts/couple_time.py
Exact fp32 (no fused level-0 kernel), 1024 tiles, log_prob and inverse: 64x64 C=1 L3 gives c = 4 / 8 / 16 at 1024 / 256 / 64 pixels a
tile, 32x32 C=2 L3 gives c = 8 / 16 / 32 at 256 / 64 / 16."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audiosourcesep_amd.config import GlowConfig                                        # noqa: E402
from audiosourcesep_amd.synthetic import calibrated_engine, synthetic_mel_tiles        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--tiles", type=int, default=1024)
args = ap.parse_args()
for cfg in (GlowConfig(H=64, W=64, C=1, L=3, K=2, F=128), GlowConfig(H=32, W=32, C=2, L=3, K=2, F=128)):
    eng, _ = calibrated_engine(cfg, device=0, init_tiles=8)
    x = torch.from_numpy(synthetic_mel_tiles(args.tiles, cfg, seed=3)).cuda()
    for _ in range(args.reps):
        lp, z = eng.log_prob(x, return_latent=True)
        xr = eng.inverse(z)
    torch.cuda.synchronize()
    print(cfg, "round trip %.1e dB" % float((xr - x).abs().max()))
