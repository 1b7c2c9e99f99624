"""ctypes binding of ``libglowk.so`` (the C ABI declared in ``include/glowk.h``).

The product path has no CPU fallback: if the HIP library has not been built (``__graft_entry__.build()``
or ``python -m audiosourcesep_amd.build``) importing a compute entry point raises ``GlowkLibraryMissing``.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GLOWK_LIB") or os.path.join(_HERE, "libglowk.so")   # GLOWK_LIB: A/B timing of two builds (scripts/ab.py)


class GlowkLibraryMissing(RuntimeError):
    pass


class GlowkError(RuntimeError):
    pass


class GlowkRangeError(GlowkError):
    """GLOWK_ERR_RANGE: a call in a split arithmetic (f16x3 / f16x2) left the fp16 range; its outputs are not usable."""


class GlowkConfigStruct(ctypes.Structure):
    """``glowk_config`` of include/glowk.h (field order and types must match)."""
    _fields_ = [
        ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("C", ctypes.c_int32),
        ("L", ctypes.c_int32), ("K", ctypes.c_int32), ("F", ctypes.c_int32),
        ("learntop", ctypes.c_int32), ("use_logit", ctypes.c_int32),
        ("minval", ctypes.c_float), ("maxval", ctypes.c_float), ("alpha", ctypes.c_float),
        ("bn_eps", ctypes.c_float),
    ]


class GlowkProfile(ctypes.Structure):
    """``glowk_profile`` of include/glowk.h."""
    _fields_ = [("net_ms", ctypes.c_double * 4), ("net_launches", ctypes.c_int64 * 4)]


class GlowkNetRecord(ctypes.Structure):
    """``glowk_net_record`` of include/glowk.h: one coupling-network launch of the launch trace."""
    _fields_ = [(n, ctypes.c_int32) for n in ("level", "dir", "arith", "store", "Q", "family", "passes", "split", "np", "co", "q",
                                              "fused_px", "presum")]


# tensor ids (enum glowk_tensor_id) keyed by the flat parameter names used across the repo
STEP_TENSOR_IDS = {
    "actnorm/log_scale": 0, "actnorm/shift": 1,
    "inv1x1/P": 2, "inv1x1/sign_S": 3, "inv1x1/L": 4, "inv1x1/log_S": 5, "inv1x1/U": 6,
    "nn/conv1/kernel": 7, "nn/conv1/bias": 8,
    "nn/bn1/gamma": 9, "nn/bn1/beta": 10, "nn/bn1/mean": 11, "nn/bn1/var": 12,
    "nn/conv2/kernel": 13, "nn/conv2/bias": 14,
    "nn/bn2/gamma": 15, "nn/bn2/beta": 16, "nn/bn2/mean": 17, "nn/bn2/var": 18,
    "nn/conv3/kernel": 19, "nn/conv3/bias": 20,
    "inv1x1/P_inv": 21,
}
PRIOR_TENSOR_IDS = {"prior/loc": 100, "prior/log_scale": 101}
PREC_F32, PREC_F16X3, PREC_F16X2 = 0, 1, 2
OK, ERR, ERR_RANGE = 0, 1, 2                       # enum glowk_status
RANGE_IGNORE, RANGE_ERROR, RANGE_FALLBACK = 0, 1, 2   # enum glowk_range_policy
MIX_DB, MIX_MEAN = 0, 1                            # enum glowk_mixing

_vp, _i, _fp, _d = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_double

# every symbol include/glowk.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "glowk_version": (_i, []),
    "glowk_last_error": (ctypes.c_char_p, []),
    "glowk_reload_env": (None, []),
    "glowk_create": (_i, [ctypes.POINTER(GlowkConfigStruct), _i, ctypes.POINTER(_vp)]),
    "glowk_destroy": (_i, [_vp]),
    "glowk_tensor_size": (ctypes.c_size_t, [_vp, _i, _i]),
    "glowk_set_tensor": (_i, [_vp, _i, _i, _i, _fp, ctypes.c_size_t]),
    "glowk_get_tensor": (_i, [_vp, _i, _i, _i, _fp, ctypes.c_size_t]),
    "glowk_finalize_weights": (_i, [_vp]),
    "glowk_actnorm_data_init": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "glowk_set_precision": (_i, [_vp, _i]),
    "glowk_get_precision": (_i, [_vp]),
    "glowk_set_range_policy": (_i, [_vp, _i]),
    "glowk_get_range_policy": (_i, [_vp]),
    "glowk_range_status": (_i, [_vp, ctypes.POINTER(_i), ctypes.POINTER(ctypes.c_int64), _vp]),
    "glowk_range_probe_begin": (_i, [_vp]),
    "glowk_range_probe_end": (_i, [_vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), _vp]),
    "glowk_split_probe": (_i, [_vp, _i, ctypes.c_float, _i, _vp, _vp, _vp]),
    "glowk_workspace_bytes": (ctypes.c_size_t, [_vp, _i, _i]),
    "glowk_reserve": (_i, [_vp, _i, _i]),
    "glowk_max_tiles": (_i, [_vp]),
    "glowk_forward": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "glowk_inverse": (_i, [_vp, _vp, _i, _vp, _vp]),
    "glowk_log_prob": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "glowk_log_prob_sum": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp]),
    "glowk_sum_f64": (_i, [_vp, ctypes.c_size_t, _vp, _i, ctypes.c_double, _vp]),
    "glowk_log_prob_grad": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "glowk_sample": (_i, [_vp, _vp, _i, _vp, _vp]),
    "glowk_prior_log_prob": (_i, [_vp, _vp, _i, _vp, _vp]),
    "glowk_fused_steps": (ctypes.c_int64, [_vp]),
    "glowk_kernel_families": (_i, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    "glowk_profile_begin": (_i, [_vp]),
    "glowk_profile_end": (_i, [_vp, ctypes.POINTER(GlowkProfile)]),
    "glowk_net_trace_begin": (_i, [_vp]),
    "glowk_net_trace_end": (_i, [_vp, ctypes.POINTER(GlowkNetRecord), _i, ctypes.POINTER(_i)]),
    "glowk_squeeze": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "glowk_unsqueeze": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "glowk_preprocess_forward": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "glowk_preprocess_inverse": (_i, [_vp, _vp, _i, _vp, _vp]),
    "glowk_step_forward": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "glowk_step_inverse": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp]),
    "glowk_coupling_net": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "glowk_param_vector_size": (ctypes.c_size_t, [_vp]),
    "glowk_param_offset": (_i, [_vp, _i, _i, _i, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]),
    "glowk_param_grad": (_i, [_vp, _vp, _i, ctypes.c_float, _vp, _vp, _vp]),
    "glowk_apply_gradients": (_i, [_vp, _vp, _i, ctypes.c_float, _vp]),
    "glowk_crc32c": (ctypes.c_uint32, [_vp, ctypes.c_size_t]),
    "glowk_basis_update": (_i, [_vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_float, ctypes.c_float, _vp, _vp,
                                ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, _vp, _vp]),
    "glowk_basis_mix": (_i, [_vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_basis_update_n": (_i, [_vp, _vp, _vp, _i, _vp, ctypes.c_size_t, _i, ctypes.c_float, ctypes.c_float,
                                  ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, _vp, _vp]),
    "glowk_basis_mix_n": (_i, [_vp, _i, _vp, ctypes.c_size_t, _i, _vp]),
    "glowk_random_source": (_i, [_vp, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64, _i, _i, _i, ctypes.c_uint64, _vp]),
    "glowk_random": (_i, [_vp, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64, _i, _i, ctypes.c_uint64, _vp]),
    "glowk_add_noise": (_i, [_vp, _vp, ctypes.c_size_t, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, _i, ctypes.c_uint64, _vp]),
    "glowk_mel_filterbank": (_i, [_fp]),
    "glowk_mel_frontend": (_i, [_vp, _i, _i, ctypes.c_float, _vp, _vp, _vp]),
    "glowk_mel_to_power": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "glowk_masked_istft": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp]),
    "glowk_griffinlim": (_i, [_vp, _vp, _i, _i, _i, ctypes.c_float, _vp, _vp]),
    "glowk_resample_length": (ctypes.c_int64, [ctypes.c_int64, _i, _i]),
    "glowk_resample_filter": (_i, [ctypes.POINTER(ctypes.c_double)]),
    "glowk_resample": (_i, [_vp, _i, ctypes.c_int64, _i, _i, _vp, _vp]),
    "glowk_bss_xcorr":(_i, [_vp, _i, ctypes.c_int64, _vp, _i, ctypes.c_int64, _vp, _i, _i, _vp, _vp]),
    "glowk_bss_solve": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "glowk_bss_project": (_i, [_vp, ctypes.c_int64, _i, _i, _i, _vp, _i, ctypes.c_int64, _vp, _i, _vp, _i, _vp, _vp]),
    "glowk_sp_stft": (_i, [_vp, _i, ctypes.c_int64, _vp, _vp]),
    "glowk_sp_istft": (_i, [_vp, _i, _i, ctypes.c_int64, _vp, _vp]),
    "glowk_oracle_mask": (_i, [_vp, _i, _i, _i, _i, ctypes.c_double, ctypes.c_double, _vp, _vp]),
    "glowk_mwf": (_i, [_vp, _i, _i, _vp]),
    "glowk_oracle_mel": (_i, [_vp, _vp, _i, ctypes.c_int64, _i, _i, ctypes.c_double, _vp, _vp]),
    "glowk_mwf_em": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "glowk_mel_frames": (_i, [_vp, _i, ctypes.c_int64, _vp, _vp, _vp]),
    "glowk_tile_cut": (_i, [_vp, _i, _i, _i, _i, ctypes.c_float, _vp, _vp]),
    "glowk_tile_stitch": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "glowk_frames_to_tiles": (_i, [_vp, _i, _i, _i, _i, _i, ctypes.c_float, _vp, _vp]),
    "glowk_basis_update_frames": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, ctypes.c_float, ctypes.c_float,
                                       ctypes.c_uint64, ctypes.c_uint64, ctypes.c_float, _vp, _vp, _vp]),
    "glowk_median_filter": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "glowk_hpss_mask": (_i, [_vp, _vp, _vp, ctypes.c_size_t, ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp]),
    "glowk_nn_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i]),
    "glowk_nn_neighbors": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_nn_median": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_beat_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i, _i, _i]),
    "glowk_beat_spectrum": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_beat_period": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "glowk_period_neighbors": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "glowk_dft2_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "glowk_rdft2": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_irdft2": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_plane_std_workspace_bytes": (ctypes.c_size_t, [_i, ctypes.c_int64]),
    "glowk_plane_std": (_i, [_vp, _i, ctypes.c_int64, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_peak_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "glowk_peak_mask": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_duet_features": (_i, [_vp, _i, _i, _i, _d, _d, _vp, _vp, _vp, _vp]),
    "glowk_duet_hist_workspace_bytes": (ctypes.c_size_t, [_i, ctypes.c_int64, _i, _i]),
    "glowk_duet_histogram": (_i, [_vp, _vp, _vp, _i, ctypes.c_int64, _d, _d, _i, _d, _d, _i, _i, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_duet_histogram_stft": (_i, [_vp, _i, _i, _i, _d, _d, _d, _d, _i, _d, _d, _i, _i, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_duet_peaks_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "glowk_duet_peaks": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_duet_assign_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "glowk_duet_assign": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _d, _d, _i, _d, _d, _i, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_nmf_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i]),
    "glowk_nmf_fit": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, ctypes.c_size_t, _vp]),
    "glowk_nmf_divergence": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _i, _i, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_nmf_masks": (_i, [_vp, _i, _vp, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int32), _i, _i, _vp, _i, _vp, _vp, _vp]),
    "glowk_iva_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i]),
    "glowk_iva_weights": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_iva_covariances": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "glowk_iva_ip_update": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "glowk_auxiva_fit": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, ctypes.c_size_t, _vp]),
    "glowk_ilrma_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i, _i]),
    "glowk_iva_power": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "glowk_iva_normalize": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, ctypes.c_size_t, _vp]),
    "glowk_ilrma_fit": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, ctypes.c_size_t, _vp]),
    "glowk_iva_inverse": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "glowk_iva_demix": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "glowk_iva_images": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "glowk_melody_positions": (_i, [_vp, _i, _i, _d, _i, _vp, _vp]),
    "glowk_melody_emission_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "glowk_melody_track_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "glowk_melody_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "glowk_melody_salience": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "glowk_melody_emission": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_melody_track": (_i, [_vp, _i, _i, _i, _vp, _i, _d, _d, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_melody_mask": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _d, _d, _vp, _vp]),
    "glowk_melody_fit": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _d, _d, _i, _d, _d, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_rpca_gemm_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i, _i]),
    "glowk_rpca_gemm": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_rpca_eigh_workspace_bytes": (ctypes.c_size_t, [_i, _i]),
    "glowk_rpca_eigh": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_rpca_shrink": (_i, [_vp, ctypes.c_size_t, _d, _vp, _vp]),
    "glowk_rpca_svt_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "glowk_rpca_svt": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_rpca_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i]),
    "glowk_rpca_fit": (_i, [_vp, _i, _i, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_rpca_binary_mask": (_i, [_vp, _vp, _vp, ctypes.c_size_t, _d, _vp, _vp, _vp, _vp]),
    "glowk_projet_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i, _i]),
    "glowk_projet_projections": (_i, [_vp, _i, _i, _i, _vp, _i, _d, _vp, _vp]),
    "glowk_projet_gains": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "glowk_projet_update_p": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _i, _d, _i, _vp, _vp]),
    "glowk_projet_update_q": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _d, _i, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_projet_fit": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _d, _i, _i, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_projet_divergence": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _d, _i, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_projet_separate": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "glowk_cluster_work_bytes": (ctypes.c_size_t, [_i, _i, _i, _i, _i]),
    "glowk_cluster_init": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_cluster_stats": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_cluster_update": (_i, [_vp, _i, _i, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_cluster_fit": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _d, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_cluster_posteriors": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_cluster_spatial_features": (_i, [_vp, _i, _i, _i, _i, _d, _d, _vp, _vp, _vp]),
    "glowk_kam_median": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "glowk_kam_backfit": (_i, [_vp, _vp, _i, _i, ctypes.c_size_t, ctypes.c_float, _vp, _vp, _vp]),
    "glowk_kam_work_bytes": (ctypes.c_size_t, [_i, _i, _i, _i, _vp]),
    "glowk_kam_fit": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, ctypes.c_float, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_nmfd_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i, _i]),
    "glowk_nmfd_fit": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, ctypes.c_size_t, _vp]),
    "glowk_nmfd_divergence": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _vp, _vp, ctypes.c_size_t, _vp]),
    "glowk_nmfd_masks": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int32), _i, _i, _vp, _i, _vp, _vp, _vp]),
    "glowk_wpe_workspace_bytes": (ctypes.c_size_t, [_i, _i, _i, _i, _i]),
    "glowk_wpe_power": (_i, [_vp, _i, _i, _i, _i, _i, _d, _vp, _vp, _vp]),
    "glowk_wpe_correlations": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "glowk_wpe_solve": (_i, [_vp, _vp, _i, _i, _i, _i, _d, _vp, _vp, _vp]),
    "glowk_wpe_filter": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "glowk_wpe_fit": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _d, _d, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
}

_lib = None


def load():
    """Load libglowk.so once and declare every prototype.  Fails loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GlowkLibraryMissing(
            "HIP library %s not found: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU fallback for the compute path." % LIB_PATH)
    # torch first: its wheel carries its own libamdhip64; if libglowk.so is loaded before it, the system HIP runtime gets
    # bound instead and the two runtimes in one process end in "no ROCm-capable device is detected" at the first hipSetDevice
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().glowk_last_error()
        raise (GlowkRangeError if rc == ERR_RANGE else GlowkError)(msg.decode() if msg else "glowk error %d" % rc)
