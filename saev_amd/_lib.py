"""ctypes binding of libsaev_amd.so (the C ABI declared in include/saev_amd.h).

The product path has no CPU fallback: if the shared library is missing or a HIP device is not
present, everything here raises.  Build the library with ``make`` (or ``__graft_entry__.build()``).
"""

from __future__ import annotations

import ctypes as C
import os
import pathlib

_HERE = pathlib.Path(__file__).resolve().parent
LIB_PATH = pathlib.Path(os.environ.get("SAEV_AMD_LIB", _HERE / "libsaev_amd.so"))

ABI_VERSION = 12


class SaevCfg(C.Structure):
    _fields_ = [
        ("d_model", C.c_int32), ("d_sae", C.c_int32), ("top_k", C.c_int32), ("k_aux", C.c_int32),
        ("alpha", C.c_float), ("dead_threshold_tokens", C.c_int64),
        ("normalize_w_dec", C.c_int32), ("remove_parallel_grads", C.c_int32),
        ("max_batch", C.c_int32), ("encoder_mode", C.c_int32), ("aux_dead_cap", C.c_int32),
        ("shard_world", C.c_int32), ("bound_mode", C.c_int32), ("max_backward_rows", C.c_int32),
        ("activation", C.c_int32),
    ]


class SaevDebugCfg(C.Structure):
    """Route switches (include/saev_amd.h: saev_debug_cfg); all zero = shipped defaults."""

    _fields_ = [(n, C.c_int32) for n in ("struct_size", "dw_route", "aux_small_max", "fwd_route", "csc_route", "fin_route", "prep_route", "aux_dense_route",
                                         "aux_small_route", "group_route", "aux_split_route", "aux_wide_route")]


class SaevLayout(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("off_W_dec", "off_b_dec", "off_W_enc", "off_b_enc", "n_total", "chunk_a", "chunk_b")]


class SaevStepStats(C.Structure):
    _fields_ = [
        ("mse", C.c_float), ("aux", C.c_float), ("l0", C.c_float), ("l1", C.c_float),
        ("grad_norm", C.c_float), ("upper", C.c_float), ("n_dead", C.c_int32),
        ("n_overflow_rows", C.c_int32), ("cand_max", C.c_int32), ("dense_route", C.c_int32), ("sse", C.c_double), ("sum_sq", C.c_double),
    ]


class SaevMuonCfg(C.Structure):
    """include/saev_amd.h: saev_muon_cfg (adjust_lr 0 = torch's "original", 1 = "match_rms_adamw", 2 = none)."""

    _fields_ = [(n, C.c_float) for n in ("momentum", "weight_decay", "a", "b", "c", "eps")] + \
               [(n, C.c_int32) for n in ("nesterov", "ns_steps", "adjust_lr")]


class SaevBatchAcc(C.Structure):
    """include/saev_amd.h: saev_batch_acc (output pointers of saev_batch_stats; NULL skips the output)."""

    _fields_ = [("struct_size", C.c_int32), ("flags", C.c_int32), ("live_eps", C.c_float), ("reserved", C.c_int32),
                ("col_sum", C.c_void_p), ("scalars", C.c_void_p), ("n_pos", C.c_void_p), ("value_sum", C.c_void_p),
                ("live", C.c_void_p)]


class SaevBatchTopKCfg(C.Structure):
    """include/saev_amd.h: saev_batch_topk_cfg (settings of a BatchTopK context beside saev_cfg; zeros = defaults)."""

    _fields_ = [("struct_size", C.c_int32), ("row_cap", C.c_int32), ("batch_momentum", C.c_double), ("list_cap", C.c_int32),
                ("reserved", C.c_int32)]


class SaevReluTrainCfg(C.Structure):
    """include/saev_amd.h: saev_relu_train_cfg (settings of a ReLU training context beside saev_cfg)."""

    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("l1_coeff", C.c_double)]


class SaevLatentTopKState(C.Structure):
    """include/saev_amd.h: saev_latent_topk_state (the caller's per-latent lists; zero-initialised before the first update)."""

    _fields_ = [("struct_size", C.c_int32), ("k", C.c_int32), ("top_val", C.c_void_p), ("top_row", C.c_void_p), ("top_cnt", C.c_void_p)]


class SaevLatentHistState(C.Structure):
    """include/saev_amd.h: saev_latent_hist_state (the caller's count table of one level; zero-initialised before the first update)."""

    _fields_ = [("struct_size", C.c_int32), ("level", C.c_int32), ("T", C.c_int32), ("reserved", C.c_int32), ("counts", C.c_void_p),
                ("n_rows", C.c_void_p), ("prefix", C.c_void_p)]


class SaevLatentExemplarsOut(C.Structure):
    """include/saev_amd.h: saev_latent_exemplars_out (where saev_latent_exemplars leaves its lists; device pointers)."""

    OUTPUTS = ("n_group_images", "n_fire", "top_val", "top_img", "top_patch", "bot_val", "bot_img", "bot_patch", "silent_img")
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32)] + [(name, C.c_void_p) for name in OUTPUTS]


class SaevLatentHistTargets(C.Structure):
    """include/saev_amd.h: saev_latent_hist_targets (the quantiles of saev_latent_hist_locate and what it leaves per target)."""

    _fields_ = [("struct_size", C.c_int32), ("Q", C.c_int32), ("over_rows", C.c_int32), ("reserved", C.c_int32), ("q", C.c_double * 8),
                ("prefix", C.c_void_p), ("rank", C.c_void_p), ("resolved", C.c_void_p), ("count", C.c_void_p), ("lower", C.c_void_p),
                ("higher", C.c_void_p), ("linear", C.c_void_p)]


class SaevProbe1DCfg(C.Structure):
    """include/saev_amd.h: saev_probe1d_cfg (the solver's hyper-parameters, the reference's names)."""

    _fields_ = [(n, C.c_int32) for n in ("struct_size", "max_iter", "class_slab_size", "poll_every", "out_dtype", "reserved")] + \
               [(n, C.c_double) for n in ("ridge", "tol", "lam_init", "lam_shrink", "lam_grow", "delta_logit")]


class SaevProbe1DLayout(C.Structure):
    """include/saev_amd.h: saev_probe1d_layout (byte offsets into the workspace of the probe1d entries)."""

    _fields_ = [("struct_size", C.c_int32), ("chunk", C.c_int32)] + \
               [(n, C.c_int64) for n in ("words", "max_chunks", "parts", "total_bytes", "off_err", "off_starts", "off_chunk_starts", "off_row",
                                         "off_val", "off_qx", "off_ybits", "off_pos", "off_cnt", "off_tot", "off_b", "off_w", "off_lam",
                                         "off_prev_pred", "off_prev_loss", "off_clipped", "off_sums", "off_part", "off_gmax", "off_done",
                                         "off_n_iter", "off_active")]


class SaevLatentAPLayout(C.Structure):
    """include/saev_amd.h: saev_latent_ap_layout (byte offsets into the workspace of saev_latent_ap)."""

    _fields_ = [("struct_size", C.c_int32), ("direct_max", C.c_int32)] + \
               [(n, C.c_int64) for n in ("parts", "part_len", "passes", "total_bytes", "off_err", "off_starts", "off_hist", "off_key",
                                         "off_latent", "off_row", "off_key2", "off_latent2", "off_row2")]


class SaevL1LogisticLayout(C.Structure):
    """include/saev_amd.h: saev_l1_logistic_layout (byte offsets into the workspace of the saev_l1_logistic entries)."""

    _fields_ = [("struct_size", C.c_int32), ("coef_rows", C.c_int32)] + \
               [(n, C.c_int64) for n in ("chunk_rows", "n_chunks", "col_blocks", "total_bytes", "off_err", "off_state", "off_w", "off_z",
                                         "off_g", "off_part", "off_r", "off_loss", "off_bp")]


class SaevEdit(C.Structure):
    """include/saev_amd.h: saev_edit (one edit of a latent; 16 bytes)."""

    _fields_ = [("latent", C.c_int32), ("op", C.c_int32), ("value", C.c_float), ("group", C.c_int32)]


EDIT_SET, EDIT_SCALE, EDIT_ADD, EDIT_IF_ACTIVE = 0, 1, 2, 4
ACT_TOPK, ACT_RELU, ACT_BATCHTOPK = 0, 1, 2
ROW_OVERFLOW = -7  # saev_status SAEV_ROW_OVERFLOW
BATCH_OVERWRITE = 1
OPERATING_SORTED = 1  # SAEV_OPERATING_SORTED
ROW_NORM_WORKSPACE_BYTES = 8192


class SaevError(RuntimeError):
    pass


P = C.c_void_p
_SIGNATURES = {
    "saev_abi_version": (C.c_int, []),
    "saev_last_error": (C.c_char_p, [P]),
    "saev_layout": (C.c_int, [C.POINTER(SaevCfg), C.POINTER(SaevLayout)]),
    "saev_create": (C.c_int, [C.POINTER(SaevCfg), C.c_int, C.POINTER(P)]),
    "saev_create_ex": (C.c_int, [C.POINTER(SaevCfg), C.POINTER(SaevDebugCfg), C.c_int, C.POINTER(P)]),
    "saev_create_batch_topk": (C.c_int, [C.POINTER(SaevCfg), C.POINTER(SaevDebugCfg), C.POINTER(SaevBatchTopKCfg), C.c_int, C.POINTER(P)]),
    "saev_create_relu_train": (C.c_int, [C.POINTER(SaevCfg), C.POINTER(SaevDebugCfg), C.POINTER(SaevReluTrainCfg), C.c_int, C.POINTER(P)]),
    "saev_copy_last_rows": (C.c_int, [P, C.c_int32, C.c_int32, P, P, P, P, P]),
    "saev_bind_threshold": (C.c_int, [P, P]),
    "saev_threshold_device": (P, [P]),
    "saev_row_cap": (C.c_int32, [P]),
    "saev_row_overflow_need": (C.c_int32, [P]),
    "saev_batch_topk_dense": (C.c_int, [P, P, C.c_int32, C.c_int32, P, P, P, P, P]),
    "saev_encode_batch_topk": (C.c_int, [P, P, C.c_int32, C.c_int32, P, P, P, P, P]),
    "saev_batch_topk_state": (C.c_int, [P, C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), P]),
    "saev_copy_last_row_nnz": (C.c_int, [P, C.c_int32, P, P]),
    "saev_destroy": (None, [P]),
    "saev_bind": (C.c_int, [P, P, P, P, P]),
    "saev_bind_tracker": (C.c_int, [P, P, P]),
    "saev_tracker_touched": (C.c_int, [P]),
    "saev_set_prefixes": (C.c_int, [P, P, C.c_int32]),
    "saev_share_x": (C.c_int, [P, P]),
    "saev_toks_since_active": (P, [P]),
    "saev_fired_flags": (P, [P]),
    "saev_stats_device": (P, [P]),
    "saev_read_stats": (C.c_int, [P, C.POINTER(SaevStepStats), P]),
    "saev_normalize_w_dec": (C.c_int, [P, P]),
    "saev_encode_dense": (C.c_int, [P, P, C.c_int32, P, P]),
    "saev_topk_dense": (C.c_int, [P, P, C.c_int32, C.c_int32, P, P, P, P]),
    "saev_encode_topk": (C.c_int, [P, P, C.c_int32, P, P, P]),
    "saev_scatter_dense": (C.c_int, [P, P, P, C.c_int32, C.c_int32, P, P]),
    "saev_decode_sparse": (C.c_int, [P, P, P, C.c_int32, C.c_int32, P, C.c_int32, P, P]),
    "saev_encode_relu": (C.c_int, [P, P, C.c_int32, C.c_int32, P, P, P, P, P]),
    "saev_decode_rows": (C.c_int, [P, P, P, P, C.c_int32, C.c_int32, P, C.c_int32, P, P]),
    "saev_scatter_rows": (C.c_int, [P, P, P, P, C.c_int32, C.c_int32, P, P]),
    "saev_remove_parallel_grads": (C.c_int, [P, P]),
    "saev_gather_rows": (C.c_int, [P, P, P, C.c_int32, P, P]),
    "saev_step_forward": (C.c_int, [P, P, C.c_int32, C.c_int64, C.c_int32, P]),
    "saev_step_dead": (C.c_int, [P, C.c_int64, P]),
    "saev_last_aux_route": (C.c_int, [P]),
    "saev_scratch_bytes": (C.c_int64, [P, C.c_int32]),
    "saev_dead_readbacks": (C.c_int64, [P]),
    "saev_step_backward": (C.c_int, [P, P]),
    "saev_backward_begin": (C.c_int, [P, P]),
    "saev_backward_rows": (C.c_int, [P, C.c_int32, C.c_int32, P]),
    "saev_backward_rows_part": (C.c_int, [P, C.c_int32, C.c_int32, C.c_int32, P]),
    "saev_backward_end": (C.c_int, [P, P]),
    "saev_copy_step_state": (C.c_int, [P, C.c_int32, P, P, P, P]),
    "saev_backward_override": (C.c_int, [P, P, P, P, P, C.c_int32]),
    "saev_aux_compact_rows": (C.c_int32, [P]),
    "saev_aux_compact_export": (C.c_int, [P, P, P]),
    "saev_aux_compact_import": (C.c_int, [P, P, P]),
    "saev_trust_gradients": (C.c_int, [P, C.c_int32]),
    "saev_grad_w_enc_t": (P, [P]),
    "saev_bind_w_enc_t": (C.c_int, [P, P]),
    "saev_step_tail": (C.c_int, [P, C.c_float, C.c_float, C.c_float, C.c_int64, P]),
    "saev_tail_prepare": (C.c_int, [P, C.c_int32, P]),
    "saev_tail_apply": (C.c_int, [P, C.c_float, C.c_float, C.c_float, C.c_int64, C.c_int32, P]),
    "saev_sumsq_device": (P, [P]),
    "saev_bind_sumsq": (C.c_int, [P, P]),
    "saev_wdec_ready_event": (C.c_int, [P, P]),
    "saev_wenc_ready_event": (C.c_int, [P, P]),
    "saev_train_step": (C.c_int, [P, P, C.c_int32, C.c_float, C.c_float, C.c_int64, P]),
    "saev_train_step_gather": (C.c_int, [P, P, P, P, C.c_int32, C.c_float, C.c_float, C.c_int64, P]),
    "saev_params_touched": (C.c_int, [P]),
    "saev_muon_default_cfg": (None, [C.POINTER(SaevMuonCfg)]),
    "saev_muon_tail": (C.c_int, [P, C.c_float, C.c_float, C.c_float, C.c_int64, C.POINTER(SaevMuonCfg), P]),
    "saev_muon_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "saev_muon_newton_schulz": (C.c_int, [P, C.c_int64, C.c_int64, P, C.POINTER(SaevMuonCfg), C.c_int32, P, C.c_int64, P]),
    "saev_coherence_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "saev_dictionary_coherence": (C.c_int, [P, C.c_int64, C.c_int64, C.c_int32, P, C.c_int64, P, P, P, P]),
    "saev_dictionary_match_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    "saev_dictionary_match": (C.c_int, [P, C.c_int64, P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, P, C.c_int64, P, P, P, P]),
    "saev_kmeans_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    "saev_kmeans_assign": (C.c_int, [P, C.c_int64, P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, P, C.c_int64, P, P, P, P]),
    "saev_kmeans_group": (C.c_int, [P, C.c_int64, C.c_int64, P, P, P, P]),
    "saev_kmeans_update": (C.c_int, [P, C.c_int64, C.c_int64, C.c_int64, P, P, P, P, P, P, P, P]),
    "saev_kmeans_collapsed": (C.c_int, [P, C.c_int64, C.c_int64, C.c_float, P, C.c_int32, P, C.c_int64, P, P, P]),
    "saev_batch_stats_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "saev_batch_stats": (C.c_int, [P, P, P, P, P, P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(SaevBatchAcc), P, C.c_int64, P]),
    "saev_row_norm_mean": (C.c_int, [P, C.c_int64, C.c_int64, P, P, C.c_int64, P]),
    "saev_latent_topk_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "saev_latent_topk_update": (C.c_int, [P, P, P, C.c_int64, P, P, P, C.c_int64, P, C.c_int64, C.c_int64, C.c_int64,
                                          C.POINTER(SaevLatentTopKState), P, C.c_int64, P]),
    "saev_latent_hist_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "saev_latent_hist_update": (C.c_int, [P, P, P, C.c_int64, P, P, P, C.c_int64, P, C.c_int64, C.c_int64, C.POINTER(SaevLatentHistState), P,
                                          C.c_int64, P]),
    "saev_latent_hist_locate": (C.c_int, [C.POINTER(SaevLatentHistState), C.POINTER(SaevLatentHistTargets), C.c_int64, P]),
    "saev_probe1d_workspace_bytes": (C.c_int64, [C.c_int64] * 4),
    "saev_probe1d_layout_of": (C.c_int, [C.c_int64] * 4 + [C.POINTER(SaevProbe1DLayout)]),
    "saev_probe1d_prepare": (C.c_int, [P, P, P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, P, P, P, P, C.c_int64, P]),
    "saev_probe1d_stats": (C.c_int, [C.c_int64] * 4 + [P, P, P, P, C.c_int64, P]),
    "saev_probe1d_init": (C.c_int, [C.c_int64] * 4 + [C.POINTER(SaevProbe1DCfg), P, C.c_int64, P]),
    "saev_probe1d_update": (C.c_int, [C.c_int64] * 4 + [C.POINTER(SaevProbe1DCfg), P, P, P, P, C.c_int64, P]),
    "saev_probe1d_fit": (C.c_int, [C.c_int64] * 4 + [C.POINTER(SaevProbe1DCfg), P, P, P, P, C.c_int64, P]),
    "saev_probe1d_evaluate": (C.c_int, [C.c_int64] * 4 + [P, P, C.c_double, C.c_int32, P, P, P, P, P, P, C.c_int64, P]),
    "saev_latent_ap_workspace_bytes": (C.c_int64, [C.c_int64] * 4),
    "saev_latent_ap_layout_of": (C.c_int, [C.c_int64] * 4 + [C.POINTER(SaevLatentAPLayout)]),
    "saev_latent_ap": (C.c_int, [P, P, P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, P, P, P, P, P, P, P, P, C.c_int64, P]),
    "saev_probe_ap": (C.c_int, [P, P, P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, P, P, P, P, P, C.c_int32, P, P, P, P, C.c_int32, P, P, C.c_int64, P]),
    "saev_latent_auroc_workspace_bytes": (C.c_int64, [C.c_int64] * 5),
    "saev_latent_auroc": (C.c_int, [P, P, P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, P, P, P, P, C.c_int64, P, P, P, P, P, P, P, P, P, P, C.c_int64, P]),
    "saev_latent_operating_workspace_bytes": (C.c_int64, [C.c_int64] * 5),
    "saev_latent_operating": (C.c_int, [P, P, P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, P, P, P, P, C.c_int64, C.c_int32] + [P] * 12 + [P, C.c_int64, P]),
    "saev_latent_spatial_workspace_bytes": (C.c_int64, [C.c_int64] * 5),
    "saev_latent_spatial": (C.c_int, [P, P, P] + [C.c_int64] * 6 + [P, C.c_int64, C.c_float] + [P] * 10 + [P, C.c_int64, P]),
    "saev_latent_exemplars_workspace_bytes": (C.c_int64, [C.c_int64] * 4),
    "saev_latent_exemplars": (C.c_int, [P, P, P, C.c_int64, P] + [C.c_int64] * 5 + [C.c_float, C.POINTER(SaevLatentExemplarsOut), P, C.c_int64, P]),
    "saev_latent_patch_rows": (C.c_int, [P, P, P] + [C.c_int64] * 4 + [P, P, C.c_int64, P, P, P]),
    "saev_pool_images_range": (C.c_int64, []),
    "saev_pool_images": (C.c_int, [P, P, P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, P, P, P]),
    "saev_pool_csr_range": (C.c_int64, []),
    "saev_pool_csr_workspace_bytes": (C.c_int64, [C.c_int64] * 4),
    "saev_pool_csr_count": (C.c_int, [P, P, P] + [C.c_int64] * 4 + [C.c_float, P, P, P, C.c_int64, P, P]),
    "saev_pool_csr_fill": (C.c_int, [P, P, P] + [C.c_int64] * 4 + [C.c_float, P] + [P] * 5 + [P, C.c_int64, P, P]),
    "saev_l1_logistic_workspace_bytes": (C.c_int64, [C.c_int64] * 3),
    "saev_l1_logistic_layout_of": (C.c_int, [C.c_int64] * 3 + [C.POINTER(SaevL1LogisticLayout)]),
    "saev_l1_logistic_init": (C.c_int, [P, P, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double, P, C.c_int64, P]),
    "saev_l1_logistic_iterate": (C.c_int, [P, P, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_int32, P, C.c_int64, P]),
    "saev_l1_logistic_result": (C.c_int, [P, P, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double, P, P, P, P, C.c_int64, P]),
    "saev_coactivation_chunk_rows": (C.c_int64, []),
    "saev_coactivation_window": (C.c_int64, []),
    "saev_coactivation_slots": (C.c_int64, []),
    "saev_coactivation_workspace_bytes": (C.c_int64, [C.c_int64] * 5),
    "saev_coactivation": (C.c_int, [P, P, P, C.c_int64, C.c_int64, P, P, P, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_int32,
                                    C.c_int32, P, P, P, P, P, P, C.c_int64, P]),
    "saev_edit_plan_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "saev_edit_plan_build": (C.c_int, [C.POINTER(SaevEdit), C.c_int64, C.c_int64, C.c_int64, P, C.c_int64, P]),
    "saev_intervene_rows": (C.c_int, [P, C.c_int64, C.c_int64, P, C.c_int64, P, P, P, C.c_int64, P, C.c_int64, C.c_int64, P, P, P, P, P]),
    "saev_class_fire_counts": (C.c_int, [P, P, P, C.c_int64, C.c_int64, P, P, C.c_int64, C.c_int64, C.POINTER(C.c_float), C.c_int32, P, P, P, P]),
    "saev_class_fire_f1": (C.c_int, [P, P, P, C.c_int64, C.c_int64, C.c_int32, P, P, P, P]),
    "saev_comm_unique_id": (C.c_int, [P]),
    "saev_comm_init": (C.c_int, [P, P, C.c_int32, C.c_int32]),
    "saev_comm_world": (C.c_int, [P]),
    "saev_comm_destroy": (C.c_int, [P]),
    "saev_train_step_dp": (C.c_int, [P, P, C.c_int32, C.c_float, C.c_float, C.c_int64, P]),
    "saev_last_idx": (P, [P]),
    "saev_last_val": (P, [P]),
    "saev_last_x_hat": (P, [P]),
    "saev_copy_last": (C.c_int, [P, C.c_int32, P, P, P, P]),
    "saev_bound_state": (C.c_int, [P, C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_float), P]),
    "saev_bound_ratio": (C.c_int, [P, C.POINTER(C.c_float), C.POINTER(C.c_int64), P]),
    "saev_enable_kernel_timing": (C.c_int, [P, C.c_int32]),
    "saev_last_encoder_ms": (C.c_float, [P]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def load() -> C.CDLL:
    """Load libsaev_amd.so and attach argument types.  Raises if the library is not built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise SaevError(
                f"{LIB_PATH} not found: build the HIP extension first (`make` in the repo root or "
                "`python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback."
            )
        # torch first: PyTorch-ROCm carries its own libamdhip64, and a process must hold ONE HIP runtime.  Loaded after torch, this
        # library's libamdhip64.so dependency resolves to the copy torch has mapped; loaded before it, the system's copy comes in
        # and torch's follows -- two runtimes, and every call here (hipSetDevice first of all) fails on pointers / devices of the
        # other one (`python __graft_entry__.py smoke`: build() loaded the library before smoke() imported torch).
        import torch  # noqa: F401

        lib = C.CDLL(str(LIB_PATH))
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        got = lib.saev_abi_version()
        if got != ABI_VERSION:
            raise SaevError(f"libsaev_amd.so ABI version {got} != expected {ABI_VERSION}")
        _lib = lib
    return _lib


def check(lib: C.CDLL, ctx, rc: int, what: str) -> None:
    if rc != 0:
        msg = lib.saev_last_error(ctx)
        raise SaevError(f"{what} failed (status {rc}): {msg.decode() if msg else '?'}")
