"""ctypes binding of libellc_hip.so (the C ABI declared in include/ellc_abi.h).

There is no fallback: if the HIP library is missing or a GPU call fails, an exception is raised.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.path.join(CSRC, "libellc_hip.so")   # the shipping loader reads nothing from the environment; diagnostic tools call use_library()
MAX_LEVELS = 8

# every symbol include/ellc_abi.h declares (checked by tests/test_abi_symbols.py against the header text)
ABI_SYMBOLS = [
    "ellc_abi_version", "ellc_device_count", "ellc_default_config", "ellc_ctx_create", "ellc_ctx_destroy", "ellc_last_error", "ellc_sync", "ellc_stream", "ellc_ctx_counters", "ellc_ctx_set_poll_timeout_us", "ellc_ctx_set_grid_batch", "ellc_ctx_set_dense_maps", "ellc_ctx_set_persistent_schedule",
    "ellc_frame_upload", "ellc_keyframe_upload", "ellc_keyframe_from_frame", "ellc_get_image_level", "ellc_get_gradient",
    "ellc_get_max_gradient", "ellc_keyframe_set_depth", "ellc_keyframe_set_depth_level", "ellc_keyframe_get_depth_level",
    "ellc_keyframe_set_weights", "ellc_keyframe_get_weights", "ellc_keyframe_finalise_weights", "ellc_align", "ellc_align_enqueue",
    "ellc_align_fetch", "ellc_align_quality_at", "ellc_gn_iterate", "ellc_gn_display_planes", "ellc_concatenate_relative_pose", "ellc_concatenate_origin_pose", "ellc_se3_exp",
    "ellc_se3_log", "ellc_depth_set_state", "ellc_depth_get_state", "ellc_depth_set_keyframe", "ellc_depth_propagate",
    "ellc_depth_observe", "ellc_depth_fill_holes", "ellc_depth_regularize", "ellc_depth_make_inv_depth_one", "ellc_depth_regularize_fill_regularize", "ellc_depth_do_regularization",
    "ellc_depth_update_depth_image", "ellc_depth_create_keyframe", "ellc_depth_seeds", "ellc_track_frame",
    "ellc_histogram", "ellc_kl_divergence", "ellc_copy_slot", "ellc_copy_slot_across", "ellc_keyframe_map_points", "ellc_keyframe_render_depth", "ellc_keyframe_fuse_depth",
    "ellc_depth_absorb_keyframes", "ellc_absorb_default_params", "ellc_keyframe_trial_propagate", "ellc_depth_restart_from_keyframes",
    "ellc_keyframe_depth_consistency", "ellc_keyframe_sim3_step", "ellc_keyframe_sim3_align", "ellc_sim3_default_params", "ellc_sim3_solve", "ellc_sim3_apply",
    "ellc_keyframe_light_step", "ellc_keyframe_sim3_step_lit", "ellc_keyframe_sim3_align_lit", "ellc_light_default_params", "ellc_light_solve",
    "ellc_keyframe_refine_depth", "ellc_refine_default_params", "ellc_sim3_invert",
    "ellc_keyframe_sweep_depth", "ellc_sweep_default_params",
    "ellc_keyframe_cull_depth", "ellc_cull_default_params",
    "ellc_keyframe_joint_step", "ellc_joint_solve", "ellc_keyframe_joint_apply", "ellc_keyframe_joint_refine", "ellc_joint_default_params",
    "ellc_depth_absorb_keyframes_lit", "ellc_depth_restart_from_keyframes_lit", "ellc_keyframe_trial_propagate_lit", "ellc_trial_light_solve",
    "ellc_ingest_configure", "ellc_frame_ingest_bgr",
    "ellc_shard_range", "ellc_comm_unique_id", "ellc_comm_init_rccl", "ellc_comm_init_tcp", "ellc_comm_info", "ellc_comm_destroy", "ellc_comm_last_error",
    "ellc_gather_start", "ellc_gather_finish", "ellc_gather_results",
]


# what include/ellc_abi_diag.h adds (measurement hooks, device self-tests, test hooks): exported by libellc_hip_diag.so only
DIAG_SYMBOLS = [
    "ellc_profile_gn_kernel", "ellc_profile_align", "ellc_profile_depth_stage", "ellc_profile_calibrate_read", "ellc_profile_stream_read",
    "ellc_selftest_div_pair", "ellc_selftest_lu", "ellc_debug_persist_delay", "ellc_debug_set_persist_epoch", "ellc_debug_persist_counters", "ellc_debug_set_eager_lists", "ellc_debug_set_hinv_cache", "ellc_debug_set_fold_staging",
    "ellc_debug_set_count_cache", "ellc_debug_count_cache_counters", "ellc_debug_set_packed_taps", "ellc_debug_row_tap_launches", "ellc_debug_get_packed_level",
    "ellc_debug_set_mask_scatter", "ellc_debug_mask_scatter_counters", "ellc_debug_get_valid_mask",
    "ellc_debug_schedule_sums", "ellc_profile_map_points", "ellc_profile_render_depth", "ellc_profile_fuse_depth", "ellc_profile_depth_absorb", "ellc_profile_trial_propagate", "ellc_profile_depth_consistency", "ellc_profile_sim3_step",
    "ellc_profile_light_step", "ellc_profile_sim3_step_lit", "ellc_profile_refine_depth", "ellc_profile_sweep_depth", "ellc_profile_cull_depth",
    "ellc_profile_joint_step", "ellc_profile_joint_apply",
]


class EllcConfig(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("levels", C.c_int),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("max_iter", C.c_int * MAX_LEVELS), ("early_exit", C.c_int),
                ("max_keyframes", C.c_int), ("max_frames", C.c_int), ("max_batch", C.c_int), ("device", C.c_int),
                ("concurrent_batches", C.c_int), ("arith", C.c_int), ("coalesce", C.c_int), ("cache_records", C.c_int), ("grid_batch", C.c_int)]


class EllcHypotheses(C.Structure):
    _fields_ = [("invDepth", C.c_void_p), ("invDepthSmoothed", C.c_void_p), ("variance", C.c_void_p), ("varianceSmoothed", C.c_void_p),
                ("validity_counter", C.c_void_p), ("blacklisted", C.c_void_p), ("isValid", C.c_void_p)]


class EllcAlignQuality(C.Structure):
    """ellc_align_quality: what ellc_align_quality_at returns per evaluation."""
    _fields_ = [("n_depth", C.c_int32), ("n_used", C.c_int32),
                ("sum_r2", C.c_double), ("sum_abs_r", C.c_double), ("sum_w", C.c_double), ("sum_wr2", C.c_double),
                ("H", C.c_float * 36), ("b", C.c_float * 6), ("Hinv", C.c_float * 36)]


class EllcMapPoint(C.Structure):
    """ellc_map_point: one record of ellc_keyframe_map_points (24 bytes)."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("var", C.c_float),
                ("px", C.c_uint16), ("py", C.c_uint16), ("intensity", C.c_uint8), ("support", C.c_uint8), ("source", C.c_uint16)]


class EllcMapFilter(C.Structure):
    """ellc_map_filter: which pixels ellc_keyframe_map_points keeps."""
    _fields_ = [("max_var", C.c_float), ("min_support", C.c_int), ("support_k2", C.c_float), ("stride", C.c_int)]


class EllcDepthConsistency(C.Structure):
    """ellc_depth_consistency: what ellc_keyframe_depth_consistency returns per request (72 bytes)."""
    _fields_ = [("sum_chi2", C.c_double), ("sum_w_ss", C.c_double), ("sum_w_st", C.c_double),
                ("sum_abs_di", C.c_int64), ("sum_di2", C.c_int64),
                ("n_kept", C.c_int32), ("n_in_view", C.c_int32), ("n_overlap", C.c_int32), ("n_agree", C.c_int32),
                ("n_in_front", C.c_int32), ("n_behind", C.c_int32), ("n_weighted", C.c_int32)]


class EllcSim3Params(C.Structure):
    """ellc_sim3_params: the weights and gates of ellc_keyframe_sim3_step."""
    _fields_ = [("sigma_i2", C.c_float), ("huber_k", C.c_float), ("gate_k2", C.c_float), ("depth_weight", C.c_float)]


class EllcSim3Normal(C.Structure):
    """ellc_sim3_normal: what ellc_keyframe_sim3_step returns per request (320 bytes)."""
    _fields_ = [("H", C.c_double * 28), ("b", C.c_double * 7), ("chi2_photo", C.c_double), ("chi2_depth", C.c_double),
                ("n_kept", C.c_int32), ("n_in_view", C.c_int32), ("n_photo", C.c_int32), ("n_photo_huber", C.c_int32),
                ("n_depth", C.c_int32), ("n_depth_gated", C.c_int32)]


class EllcLightNormal(C.Structure):
    """ellc_light_normal: what ellc_keyframe_light_step returns per request (72 bytes)."""
    _fields_ = [("sum_w", C.c_double), ("sum_w_s", C.c_double), ("sum_w_t", C.c_double), ("sum_w_ss", C.c_double), ("sum_w_st", C.c_double),
                ("sum_w_tt", C.c_double), ("chi2_photo", C.c_double),
                ("n_kept", C.c_int32), ("n_in_view", C.c_int32), ("n_photo", C.c_int32), ("n_photo_huber", C.c_int32)]


class EllcLightParams(C.Structure):
    """ellc_light_params: what ellc_light_solve accepts (12 bytes)."""
    _fields_ = [("gain_min", C.c_float), ("gain_max", C.c_float), ("min_pixels", C.c_int32)]


class EllcRefineParams(C.Structure):
    """ellc_refine_params: the weights, the step bound and the limits of ellc_keyframe_refine_depth (24 bytes)."""
    _fields_ = [("sigma_i2", C.c_float), ("huber_k", C.c_float), ("prior_weight", C.c_float), ("max_step_rel", C.c_float),
                ("n_iter", C.c_int), ("min_views", C.c_int)]


REFINE_STATUS = ("NOT_TAKING_PART", "REFINED", "TOO_FEW_VIEWS", "NO_INFORMATION", "BAD_STEP", "VIEWS_CHANGED", "COST_ROSE")


class EllcRefineStats(C.Structure):
    """ellc_refine_stats: what ellc_keyframe_refine_depth counts (64 bytes)."""
    _fields_ = [("n_kept", C.c_int32), ("n_taking_part", C.c_int32), ("n_refined", C.c_int32), ("n_too_few_views", C.c_int32),
                ("n_no_information", C.c_int32), ("n_bad_step", C.c_int32), ("n_views_changed", C.c_int32), ("n_cost_rose", C.c_int32),
                ("sum_views", C.c_int64), ("sum_cost_before", C.c_double), ("sum_cost_after", C.c_double), ("reserved", C.c_int32 * 2)]


class EllcSweepParams(C.Structure):
    """ellc_sweep_params: the weights, the inverse-depth range and the tests of ellc_keyframe_sweep_depth (40 bytes)."""
    _fields_ = [("sigma_i2", C.c_float), ("huber_k", C.c_float), ("d_min", C.c_float), ("d_max", C.c_float), ("min_grad2", C.c_float),
                ("max_cost", C.c_float), ("distinct_ratio", C.c_float), ("var_scale", C.c_float), ("n_samples", C.c_int), ("min_views", C.c_int)]


SWEEP_STATUS = ("NOT_SWEPT", "CREATED", "NO_VALID_SAMPLE", "AT_RANGE_END", "COST_TOO_HIGH", "NOT_DISTINCT", "FLAT")


class EllcSweepStats(C.Structure):
    """ellc_sweep_stats: what ellc_keyframe_sweep_depth counts (64 bytes)."""
    _fields_ = [("n_ok", C.c_int32), ("n_swept", C.c_int32), ("n_created", C.c_int32), ("n_no_valid_sample", C.c_int32),
                ("n_at_range_end", C.c_int32), ("n_cost_too_high", C.c_int32), ("n_not_distinct", C.c_int32), ("n_flat", C.c_int32),
                ("sum_views", C.c_int64), ("sum_cost", C.c_double), ("reserved", C.c_int32 * 4)]


SWEEP_STATS_FIELDS = tuple(f[0] for f in EllcSweepStats._fields_ if f[0] != "reserved")


class EllcCullParams(C.Structure):
    """ellc_cull_params: the agreement rule, the photometric bound and the four counts of ellc_keyframe_cull_depth (28 bytes)."""
    _fields_ = [("agree_k2", C.c_float), ("sigma_i2", C.c_float), ("photo_k", C.c_float), ("min_support", C.c_int), ("min_judged", C.c_int),
                ("min_in_front", C.c_int), ("min_photo", C.c_int)]


CULL_STATUS = ("NOT_TAKING_PART", "KEPT", "CULLED_FREE_SPACE", "CULLED_UNSUPPORTED", "CULLED_PHOTO", "UNSEEN")


class EllcCullStats(C.Structure):
    """ellc_cull_stats: what ellc_keyframe_cull_depth counts (64 bytes)."""
    _fields_ = [("n_kept", C.c_int32), ("n_retained", C.c_int32), ("n_unseen", C.c_int32), ("n_culled_free_space", C.c_int32),
                ("n_culled_unsupported", C.c_int32), ("n_culled_photo", C.c_int32),
                ("sum_agree", C.c_int64), ("sum_in_front", C.c_int64), ("sum_behind", C.c_int64), ("sum_photo", C.c_int64), ("sum_photo_bad", C.c_int64)]


CULL_STATS_FIELDS = tuple(f[0] for f in EllcCullStats._fields_)


JOINT_MAX_VIEWS = 8


class EllcJointParams(C.Structure):
    """ellc_joint_params: the weights, the step bound and the view limit of the joint refinement (20 bytes)."""
    _fields_ = [("sigma_i2", C.c_float), ("huber_k", C.c_float), ("prior_weight", C.c_float), ("max_step_rel", C.c_float), ("min_views", C.c_int)]


JOINT_STATUS = ("NOT_TAKING_PART", "STEPPED", "TOO_FEW_VIEWS", "NO_INFORMATION", "BAD_STEP")


class EllcJointNormal(C.Structure):
    """ellc_joint_normal: what ellc_keyframe_joint_step returns (11600 bytes)."""
    _fields_ = [("A", (C.c_double * 21) * JOINT_MAX_VIEWS), ("a", (C.c_double * 6) * JOINT_MAX_VIEWS), ("S", C.c_double * 1176), ("s", C.c_double * 48),
                ("chi2_photo", C.c_double), ("chi2_prior", C.c_double), ("n_terms", C.c_int64),
                ("n_kept", C.c_int32), ("n_taking_part", C.c_int32), ("n_used", C.c_int32), ("n_too_few_views", C.c_int32),
                ("n_no_information", C.c_int32), ("B", C.c_int32), ("n_view_terms", C.c_int32 * JOINT_MAX_VIEWS)]


class EllcJointApplyStats(C.Structure):
    """ellc_joint_apply_stats: what ellc_keyframe_joint_apply counts (32 bytes)."""
    _fields_ = [("n_kept", C.c_int32), ("n_taking_part", C.c_int32), ("n_stepped", C.c_int32), ("n_too_few_views", C.c_int32),
                ("n_no_information", C.c_int32), ("n_bad_step", C.c_int32), ("reserved", C.c_int32 * 2)]


class EllcAbsorbParams(C.Structure):
    """ellc_absorb_params: the gates and limits of ellc_depth_absorb_keyframes."""
    _fields_ = [("agree_k2", C.c_float), ("max_fold", C.c_int), ("photo_gate", C.c_int), ("src_validity", C.c_int), ("finalise", C.c_int)]


ABSORB_STATS_FIELDS = ("n_kept", "n_in_view", "n_interior", "n_candidates", "n_visited", "n_created", "n_merged", "n_replaced", "n_occluded",
                       "n_skipped", "targets_hit", "targets_touched", "targets_truncated", "n_valid_before", "n_valid_after", "reserved")


class EllcAbsorbStats(C.Structure):
    """ellc_absorb_stats: what ellc_depth_absorb_keyframes counts (64 bytes)."""
    _fields_ = [(name, C.c_int32) for name in ABSORB_STATS_FIELDS]


class EllcTrialPropagation(C.Structure):
    """ellc_trial_propagation: what ellc_keyframe_trial_propagate returns per request (48 bytes)."""
    _fields_ = [("sum_r2", C.c_double), ("sum_abs_r", C.c_double),
                ("n_kept", C.c_int32), ("n_in_view", C.c_int32), ("n_interior", C.c_int32), ("n_low_grad", C.c_int32),
                ("n_candidates", C.c_int32), ("n_targets", C.c_int32), ("reserved", C.c_int32 * 2)]


class EllcTrialPropagationLit(C.Structure):
    """ellc_trial_propagation_lit: what ellc_keyframe_trial_propagate_lit returns per request (96 bytes): an ellc_trial_propagation at
    the request's light, then the five sums of the fit of Iw on Is over the interior pixels and their number."""
    _fields_ = EllcTrialPropagation._fields_ + [("sum_s", C.c_double), ("sum_t", C.c_double), ("sum_ss", C.c_double), ("sum_st", C.c_double),
                                                ("sum_tt", C.c_double), ("n_fit", C.c_int32), ("reserved2", C.c_int32)]


class EllcError(RuntimeError):
    pass


def build(verbose=False):
    """Compile libellc_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC]
    if not verbose:
        args.insert(1, "-s")
    subprocess.check_call(args)


COMM_SO_PATH = os.path.join(CSRC, "libellc_comm.so")   # csrc/ellc_comm.cpp alone (TCP transport): loads without a GPU
COMM_SYMBOLS = ["ellc_shard_range", "ellc_comm_init_tcp", "ellc_comm_info", "ellc_comm_destroy", "ellc_comm_last_error", "ellc_gather_start", "ellc_gather_finish",
                "ellc_gather_results"]
_comm = None


def comm_lib():
    """The multi-GPU layer as a host-only library (no HIP, no RCCL): what the CPU tests of the sharded path drive."""
    global _comm
    if _comm is None:
        if not os.path.exists(COMM_SO_PATH):
            raise EllcError("libellc_comm.so is not built (%s). Run __graft_entry__.build() / make -C %s" % (COMM_SO_PATH, CSRC))
        _comm = C.CDLL(COMM_SO_PATH)
        _comm.ellc_comm_last_error.restype = C.c_char_p
        for name in COMM_SYMBOLS:
            getattr(_comm, name)
    return _comm


_lib = None
_diag = None
DIAG_SO_PATH = os.path.join(CSRC, "libellc_hip_diag.so")   # the same sources built with -DELLC_DIAG_ABI (csrc/Makefile)


def use_library(path):
    """Diagnostic tools only (tools/*.py with an A/B variant, build/libellc_hip_envdiag.so or ..._stamps.so — all built with the
    diagnostic ABI): load this build instead of the in-tree libraries, for the product entry points and the diagnostic ones
    alike. Must be called before the first lib() / diag_lib(); the path is explicit, never taken from the environment."""
    global SO_PATH, DIAG_SO_PATH, _external
    _external = True
    if _lib is not None or _diag is not None:
        raise EllcError("use_library: the library is already loaded")
    SO_PATH = DIAG_SO_PATH = os.path.abspath(path)


_external = False   # use_library(): an A/B build, possibly of an older revision that lacks the newest entry points


def _bind(path, symbols, what):
    if not os.path.exists(path):
        raise EllcError("%s is not built (%s). Run __graft_entry__.build() / make -C %s; "
                        "there is no CPU fallback for the product path." % (what, path, CSRC))
    h = C.CDLL(path)
    h.ellc_last_error.restype = C.c_char_p
    h.ellc_stream.restype = C.c_void_p
    h.ellc_kl_divergence.restype = C.c_double
    h.ellc_comm_last_error.restype = C.c_char_p
    if hasattr(h, "ellc_sim3_apply"):
        h.ellc_sim3_apply.restype = None
        h.ellc_sim3_default_params.restype = None
    if hasattr(h, "ellc_light_default_params"):
        h.ellc_light_default_params.restype = None
    if hasattr(h, "ellc_refine_default_params"):
        h.ellc_refine_default_params.restype = None
        h.ellc_sim3_invert.restype = None
    if hasattr(h, "ellc_sweep_default_params"):
        h.ellc_sweep_default_params.restype = None
    if hasattr(h, "ellc_cull_default_params"):
        h.ellc_cull_default_params.restype = None
    if hasattr(h, "ellc_joint_default_params"):
        h.ellc_joint_default_params.restype = None
    if hasattr(h, "ellc_absorb_default_params"):
        h.ellc_absorb_default_params.restype = None
    for name in symbols:
        if _external and not hasattr(h, name):
            continue          # (diagnostic A/B builds only; the in-tree libraries must export every symbol)
        getattr(h, name)  # raises AttributeError if the library does not export it
    return h


def diag_lib():
    """libellc_hip_diag.so: everything lib() has plus include/ellc_abi_diag.h (bench.py's roofline leg, tools/, self-tests)."""
    global _diag
    if _diag is None:
        if DIAG_SO_PATH == SO_PATH:   # use_library(): one build serves both (an A/B build of an older revision may lack the newer hooks)
            _diag = lib()
        else:
            _diag = _bind(DIAG_SO_PATH, ABI_SYMBOLS + DIAG_SYMBOLS, "libellc_hip_diag.so")
    return _diag


def lib():
    global _lib
    if _lib is None:
        _lib = _bind(SO_PATH, ABI_SYMBOLS, "libellc_hip.so")
    return _lib
