"""Case table of the inverse-direction oracle tests (tests/test_gpu_inverse_oracle.py on the GPU, tests/test_inverse_oracle_cpu.py
for the conditioning of the same inputs), with a restatement of the engine's launch rule for the coupling of a flow step
(launch_couple / net_and_couple in csrc/glowk.hip, launch_h3s in csrc/glowk_launch.h) so that the table can be checked to reach
every launch form of that direction.  NumPy only; nothing here needs a GPU."""
import numpy as np

from audiosourcesep_amd.config import GlowConfig
from audiosourcesep_amd.synthetic import synthetic_mel_tiles, synthetic_params
from oracle import glowref as R

ARITHMETICS = ("f32", "f16x3", "f16x2")


class Case:
    """cfg, tiles in the batch, seed of the tiles, tiles of the ActNorm calibration batch.  co_off: the split arithmetics are run
    with GLOWK_CO_OFF=1 as well -- on a device whose grid rule always prefers the co-resident (128-pixel) fused kernel that switch
    is the only way to the eight-wave 256-pixel fused kernel the case is about -- and the case's tile subset follows that form."""

    def __init__(self, cfg, n, seed, init_tiles=32, co_off=False):
        self.cfg, self.n, self.seed, self.init_tiles, self.co_off = cfg, n, seed, init_tiles, co_off


CASES = {
    # the smallest shapes that reach each k_couple form (what each reaches on 256 compute units: forms_of below)
    "16x16_L2_n3": Case(GlowConfig(H=16, W=16, C=1, L=2, K=2, F=128), 3, 21),
    "16x16_L3_n4": Case(GlowConfig(H=16, W=16, C=1, L=3, K=2, F=128), 4, 22),
    "32x32_L3_n5": Case(GlowConfig(H=32, W=32, C=1, L=3, K=2, F=128), 5, 23),
    "24x24_L2_F256_n7": Case(GlowConfig(H=24, W=24, C=1, L=2, K=2, F=256), 7, 24),
    "40x40_L2_n3": Case(GlowConfig(H=40, W=40, C=1, L=2, K=2, F=128), 3, 25),
    "8x8_L2_n515": Case(GlowConfig(H=8, W=8, C=1, L=2, K=2, F=128), 515, 26),
    "24x24_L2_F384_n515": Case(GlowConfig(H=24, W=24, C=1, L=2, K=2, F=384), 515, 27),
    "32x16_L4_n3": Case(GlowConfig(H=32, W=16, C=1, L=4, K=2, F=128), 3, 28),
    "16x16_C2_L3_n7": Case(GlowConfig(H=16, W=16, C=2, L=3, K=2, F=128), 7, 29),
    "8x16_C4_L2_n7": Case(GlowConfig(H=8, W=16, C=4, L=2, K=2, F=128), 7, 30),
    "8x8_logit_notop_n3": Case(GlowConfig(H=8, W=8, C=1, L=2, K=2, F=128, learntop=False, use_logit=True, alpha=1e-4), 3, 31),
    "16x16_L2_K8_n4": Case(GlowConfig(H=16, W=16, C=1, L=2, K=8, F=128), 4, 32),
    # the geometries of tests/test_gpu_fused_coupling.py (CASES / CO_CASES), there only compared form against form
    "32x32_L2_K3_F512_n300": Case(GlowConfig(H=32, W=32, C=1, L=2, K=3, F=512), 300, 33, co_off=True),
    "16x16_L2_n1031": Case(GlowConfig(H=16, W=16, C=1, L=2, K=2, F=128), 1031, 34, co_off=True),
    "64x64_L3_F512_n160": Case(GlowConfig(H=64, W=64, C=1, L=3, K=2, F=512), 160, 35, init_tiles=8),
    "96x64_L3_F512_n30": Case(GlowConfig(H=96, W=64, C=1, L=3, K=2, F=512), 30, 36, init_tiles=8),
}

# ---- the launch rule, restated ------------------------------------------------------------------------------------------------
FUSE_EW = 64           # csrc/glowk_kernels.h: widest row the fused kernels' edge buffer holds
ALL_FORMS = ("k_couple_flat<.,4>", "k_couple_flat<.,16>", "k_couple<.,true>@256", "k_couple<.,true>@512", "k_couple<.,true>@1024",
             "k_couple<.,false>", "fused_256", "fused_co_resident", "k_couple_edge")


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def couple_form(n, h, w, c, cus):
    """launch_couple with logdet == nullptr (the inverse direction asks for no log-det, so the flat grid needs no slots)."""
    hw, q = h * w, n * h * w
    if n < 2 * cus and hw % 64 == 0:
        wide = c >= 8 and (q + 15) // 16 <= 8 * cus
        return "k_couple_flat<.,16>" if wide else "k_couple_flat<.,4>"
    if n >= 2 * cus:
        return "k_couple<.,false>"
    return "k_couple<.,true>@%d" % (1024 if hw >= 256 else 512 if hw > 64 else 256)


def fuse_geometry_ok(h, w, pxw):
    hw = h * w
    if w < 4 or w > FUSE_EW or (w & (w - 1)) or pxw % w:
        return False
    if hw % pxw == 0:
        return True
    return 32 <= hw < pxw and (hw & (hw - 1)) == 0


def fused_px(n, h, w, c, F, split_arith, cus, co_off=False):
    """Pixels per workgroup of the fused network + coupling kernel that a plain forward network launch of the inverse direction takes
    (net_and_couple, then launch_h3s<.., NET_FWD or NET_FWD2>), or 0: P goes to memory and launch_couple follows.  Every n_filters
    has a fused instance of both kernels at the 4-channel level; n_filters >= 256 also has the four-pass instance that small grids
    prefer.  (Not restated: the scratch-size condition of net_and_couple and the occupancy query of the co-resident form -- the
    tests check this function's answer against the engine's own counters.)"""
    if not split_arith or c != 4 or not fuse_geometry_ok(h, w, 256):
        return 0
    q = n * h * w
    wgs, wgc = (q + 255) // 256, (q + 127) // 128
    if F >= 256 and 4 * wgs <= cus:
        return 0
    if not co_off and fuse_geometry_ok(h, w, 128) and wgc > cus:
        return 128
    return 256 if 2 * wgs > cus else 0


def forms_of(case, arith, cus, co_off=False):
    """The coupling launch forms that inverse() of the case's batch goes through, level by level."""
    cfg, out = case.cfg, set()
    for (h, w, c) in cfg.level_shapes():
        px = fused_px(case.n, h, w, c, cfg.F, arith != "f32", cus, co_off)
        if not px:
            out.add(couple_form(case.n, h, w, c, cus))
            continue
        out.add("fused_co_resident" if px == 128 else "fused_256")
        if h * w > px:
            out.add("k_couple_edge")
    return out


def level0_workgroup_pixels(case, cus):
    """Pixels per workgroup of the case's level-0 coupling launch: the fused form of the split arithmetics where it is taken (the
    256-pixel one for a co_off case), else launch_couple's."""
    h, w, c = case.cfg.level_shapes()[0]
    px = fused_px(case.n, h, w, c, case.cfg.F, True, cus, case.co_off)
    if px:
        return px
    form = couple_form(case.n, h, w, c, cus)
    return {"k_couple_flat<.,4>": 64, "k_couple_flat<.,16>": 16}.get(form, h * w)      # k_couple: one workgroup per tile


def tile_subset(case, cus):
    """The tiles the oracle evaluates: the first, the last, and those on either side of the first and of the last workgroup
    boundary of the level-0 grid (tiles are independent in this direction: the batch only selects the launch form).  ONE subset per
    case, shared by every run of it: the grid is that of level0_workgroup_pixels -- the fused form of the split arithmetics where
    the case has one (the 256-pixel one for a co_off case), else launch_couple's.  The other forms a case runs (exact fp32 always
    goes through launch_couple; the default co-resident run of a co_off case has 128-pixel workgroups) put their boundaries
    elsewhere -- 16x16_L2_n1031: tiles 1|2 and 1029|1030 co-resident, every tile for k_couple, against 3|4 and 1027|1028 here;
    the union would be nine tiles where six are allowed -- and are covered by the first and the last tile, which hold the first
    workgroup and the ragged last one of every form."""
    h, w, _ = case.cfg.level_shapes()[0]
    hw, q, p = h * w, case.n * h * w, level0_workgroup_pixels(case, cus)
    tiles = {0, case.n - 1}
    if q > p:
        first, last = p, (q - 1) // p * p
        for b in (first, last):
            tiles.update(((b - 1) // hw, b // hw))
    return sorted(tiles)


# ---- the references -----------------------------------------------------------------------------------------------------------
def latent_noise(case, n=None):
    """Seeded standard-normal eps of the latent's shape for the whole batch (float32: the common input of engine and oracle)."""
    n = case.n if n is None else n
    return np.random.default_rng(1000 + case.seed).standard_normal((n,) + case.cfg.latent_shape()).astype(np.float32)


def references(params, cfg, z, eps):
    """fp64 and float32 restatement of inverse(z) and sample_from_eps(eps) on float32 parameters / inputs, and the yardsticks
    max |ref32 - ref64| (dB) of both."""
    d, p64, p32 = cfg.as_dict(), R.cast_params(params, np.float64), R.cast_params(params, np.float32)
    z, eps = np.asarray(z, np.float32), np.asarray(eps, np.float32)
    x64 = R.bijector_inverse(z.astype(np.float64), p64, d)
    s64 = R.sample_from_eps(eps.astype(np.float64), p64, d)
    x32 = R.bijector_inverse(z, p32, d)
    s32 = R.sample_from_eps(eps, p32, d)
    assert x32.dtype == np.float32 and s32.dtype == np.float32
    return {"inverse": x64, "sample": s64, "y_inverse": float(np.abs(x32 - x64).max()), "y_sample": float(np.abs(s32 - s64).max())}


def cpu_calibrated_params(case):
    """The synthetic weights with ActNorm from the oracle's data-dependent init (run-time order, no raw-minibatch quirk: what
    synthetic.calibrated_engine asks of the GPU), rounded to the float32 an engine would hold."""
    cfg = case.cfg
    p = R.cast_params(synthetic_params(cfg), np.float64)
    mb = synthetic_mel_tiles(case.init_tiles, cfg, seed=77).astype(np.float64)
    R.actnorm_data_init(p, mb, cfg.as_dict(), runtime_order=True, raw_minibatch_quirk=False)
    return R.cast_params(p, np.float32)
