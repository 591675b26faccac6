"""ctypes binding of liblograst.so (C ABI: include/lograst.h).  Fails loudly when the library is
missing -- there is no CPU or PyTorch fallback for the product path."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LOGRAST_LIB") or os.path.join(_HERE, "lib", "liblograst.so")  # env: another build (variant, parent)

FILTER_NONE, FILTER_DILATE, FILTER_CLAMP = 0, 1, 2
FORM_AUTO, FORM_ROWS, FORM_QUADRANT = 0, 1, 2
GRAD_ROW_FLOATS = 16   # LOGRAST_GRAD_ROW_FLOATS
REC_FLOATS = 16
BWD_ROW_FLOATS = 16   # LOGRAST_BWD_ROW_FLOATS: the reverse walk's accumulator row (64 B per Gaussian)
NUM_KERNELS = 22          # the profiling slots version 4 started with (their order and count are pinned by the tests)
NUM_KERNEL_SLOTS = 23     # LOGRAST_NUM_KERNELS: + "recolor", appended within version 4 -- what lograst_profile_read fills

c_void_p, c_int32, c_uint32, c_float, c_size_t = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32,
                                                  ctypes.c_float, ctypes.c_size_t)


class LograstView(ctypes.Structure):
    """struct lograst_view (include/lograst.h)."""
    _fields_ = [
        ("width", c_int32), ("height", c_int32),
        ("tanfovx", c_float), ("tanfovy", c_float),
        ("scale_modifier", c_float),
        ("filter_mode", c_int32), ("ndc_cull", c_int32), ("extras", c_int32),
        ("viewmatrix", c_void_p), ("projmatrix", c_void_p), ("bg", c_void_p),
        ("tile_row_begin", c_int32), ("tile_row_end", c_int32),
        ("cov3d_precomp", c_void_p), ("dl_dcov3d", c_void_p),
        ("walk_form", c_int32),
        ("hit_masks", c_void_p), ("hit_mask_words", ctypes.c_uint64), ("hit_mask_form", c_int32),
    ]


class LograstAdamKey(ctypes.Structure):
    """struct lograst_adam_key (include/lograst.h)."""
    _fields_ = [("model_param", c_void_p), ("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p),
                ("exp_avg_sq", c_void_p), ("max_exp_avg_sq", c_void_p), ("width", c_int32), ("step_size", c_float)]


class LograstAccTarget(ctypes.Structure):
    """struct lograst_acc_target (include/lograst.h)."""
    _fields_ = [("base", c_void_p), ("row_stride_floats", c_int32)]


class LograstMoveKey(ctypes.Structure):
    """struct lograst_move_key (include/lograst.h)."""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("elem_size", c_int32), ("columns", c_int32),
                ("child_mode", c_int32)]


MOVE_COPY_PARENT, MOVE_ZERO, MOVE_SKIP = 0, 1, 2   # LOGRAST_MOVE_*


class LograstDecideStat(ctypes.Structure):
    """struct lograst_decide_stat (include/lograst.h)."""
    _fields_ = [("sum", ctypes.c_double), ("sumsq", ctypes.c_double), ("min", c_float), ("max", c_float),
                ("count", c_uint32), ("reserved", c_uint32)]


DECIDE_DEPTH_BINS = 256   # LOGRAST_DECIDE_DEPTH_BINS
EVAL_FIT_GAIN, EVAL_SSIM = 1, 2   # LOGRAST_EVAL_*


class LograstDecideRecord(ctypes.Structure):
    """struct lograst_decide_record (include/lograst.h)."""
    _fields_ = [("counts", c_uint32 * 8), ("need_cut", c_uint32), ("num_max_split", c_uint32), ("cut_value", c_int32),
                ("cut_thres", c_float), ("depth_all", c_uint32 * DECIDE_DEPTH_BINS),
                ("depth_split", c_uint32 * DECIDE_DEPTH_BINS), ("depth_remove", c_uint32 * DECIDE_DEPTH_BINS),
                ("stats", LograstDecideStat * 4)]


class LograstDecideDepthArgs(ctypes.Structure):
    """struct lograst_decide_depth_args (include/lograst.h)."""
    _fields_ = [(k, c_void_p) for k in ("opacity", "scaling", "node_index", "depth", "create_steps", "grad_sum", "area_sum",
                                        "radii_max_max", "weights_max", "visible_count")] + \
               [(k, c_int32) for k in ("current_depth", "max_level", "min_steps_split", "max_split_points")] + \
               [(k, c_float) for k in ("split_grad_thres", "radius2d_thres", "remove_weights_thres")] + \
               [("flag_split", c_void_p), ("flag_remove", c_void_p)]


class LograstDecideInitArgs(ctypes.Structure):
    """struct lograst_decide_init_args (include/lograst.h)."""
    _fields_ = [(k, c_void_p) for k in ("opacity", "create_steps", "grad_sum", "area_sum", "radii_max_max", "weights_max",
                                        "rand", "radius3d_min")] + \
               [("min_steps", c_int32), ("children", c_int32)] + \
               [(k, c_float) for k in ("init_weight_min", "small_thres", "split_thres_sq", "grad_thres", "radius_thres")] + \
               [("flag_split", c_void_p), ("flag_remove", c_void_p)]


class LograstError(RuntimeError):
    pass


_lib = None

_SIGNATURES = {
    "lograst_version": (ctypes.c_int, []),
    "lograst_last_error": (ctypes.c_char_p, []),
    "lograst_tile_state_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "lograst_geom_bytes": (c_size_t, [c_int32]),
    "lograst_record_bytes": (c_size_t, [c_int32]),
    "lograst_keys_bytes": (c_size_t, [c_uint32]),
    "lograst_hit_mask_bytes": (c_size_t, [c_uint32, c_int32, c_int32]),
    "lograst_forward_form": (ctypes.c_int, [ctypes.POINTER(LograstView)]),
    "lograst_backward_form": (ctypes.c_int, [ctypes.POINTER(LograstView), ctypes.c_int32]),
    "lograst_list_bytes": (c_size_t, [c_uint32]),
    "lograst_tile_offsets": (c_void_p, [c_void_p, c_int32, c_int32]),
    "lograst_ordered_lengths": (ctypes.c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "lograst_finish_lists": (ctypes.c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_uint32, c_void_p]),
    "lograst_compute_radius": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                              c_float, c_float, c_float, c_void_p, c_void_p]),
    "lograst_forward_project": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               ctypes.POINTER(c_uint32), ctypes.POINTER(c_uint32), c_void_p]),
    "lograst_forward_render": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "lograst_forward": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32] + [c_void_p] * 10 + [c_uint32, c_uint32]
                        + [c_void_p] * 7 + [c_int32, c_void_p, c_void_p]),
    "lograst_recomposite": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32] + [c_void_p] * 4 + [c_uint32, c_uint32]
                            + [c_void_p] * 10 + [c_int32, c_void_p, c_void_p]),
    "lograst_forward_speculative": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32] + [c_void_p] * 10
                                    + [c_uint32, c_uint32] + [c_void_p] * 7 + [c_int32, c_void_p]
                                    + [ctypes.POINTER(c_uint32), ctypes.POINTER(c_uint32), c_void_p]),
    # aux channels: the three forwards with (aux_colors, aux_image) behind `status`
    "lograst_forward_aux": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32] + [c_void_p] * 10 + [c_uint32, c_uint32]
                            + [c_void_p] * 7 + [c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lograst_forward_render_aux": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                                                  c_void_p]),
    "lograst_forward_speculative_aux": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32] + [c_void_p] * 10
                                        + [c_uint32, c_uint32] + [c_void_p] * 7 + [c_int32, c_void_p, c_void_p, c_void_p]
                                        + [ctypes.POINTER(c_uint32), ctypes.POINTER(c_uint32), c_void_p]),
    "lograst_tile_rows": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    "lograst_stream_copy": (ctypes.c_int, [c_void_p, c_void_p, c_size_t, c_int32, c_void_p]),
    "lograst_sparse_segment_floats": (c_size_t, [c_int32]),
    "lograst_pack_rows": (ctypes.c_int, [c_void_p, c_int32, ctypes.c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "lograst_pack_rows_clear": (ctypes.c_int, [c_void_p, c_int32, ctypes.c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    "lograst_pack_rows_hinted": (ctypes.c_int, [c_void_p, c_int32, ctypes.c_int64, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                                ctypes.c_int64, c_void_p]),
    "lograst_add_visible": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int64, c_void_p]),
    "lograst_add_visible_n": (ctypes.c_int, [c_void_p, c_void_p, c_int32, ctypes.c_int64, c_void_p]),
    "lograst_unpack_rows": (ctypes.c_int, [c_void_p, c_void_p, c_int32, c_int32, ctypes.c_int64, ctypes.c_int64, c_int32,
                                           c_void_p]),
    "lograst_read_state": (ctypes.c_int, [c_void_p, ctypes.POINTER(c_uint32), ctypes.POINTER(c_uint32),
                                          ctypes.POINTER(c_uint32), ctypes.POINTER(c_uint32), c_void_p]),
    "lograst_set_tile_cull": (ctypes.c_int, [ctypes.c_int]),
    "lograst_knob_count": (ctypes.c_int, []),
    "lograst_knob_info": (ctypes.c_int, [c_int32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_int32),
                                         ctypes.POINTER(c_int32), ctypes.POINTER(c_int32), ctypes.POINTER(ctypes.c_char_p)]),
    "lograst_set_knob": (ctypes.c_int, [ctypes.c_char_p, c_int32]),
    "lograst_get_knob": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(c_int32)]),
    "lograst_reset_knobs": (ctypes.c_int, []),
    "lograst_backward": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32] + [c_void_p] * 18 + [c_int32, c_void_p]),
    "lograst_backward_aux": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32] + [c_void_p] * 14 + [c_int32]
                             + [c_void_p] * 7 + [c_int32, c_void_p]),
    "lograst_project_backward": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32] + [c_void_p] * 10),
    # camera gradients: the two backwards with (dl_dviewmatrix, dl_dprojmatrix, scratch, scratch_bytes) in front of `stream`
    "lograst_camera_scratch_bytes": (c_size_t, [c_int32]),
    "lograst_backward_camera": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32] + [c_void_p] * 18 + [c_int32]
                                + [c_void_p] * 3 + [c_size_t, c_void_p]),
    "lograst_project_backward_camera": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32] + [c_void_p] * 12
                                        + [c_size_t, c_void_p]),
    # absolute screen-space gradients: the backward with dl_dmeans2d_abs in front of `stream`
    "lograst_backward_abs": (ctypes.c_int, [ctypes.POINTER(LograstView), c_int32] + [c_void_p] * 18 + [c_int32, c_void_p, c_void_p]),
    "lograst_pose_apply": (ctypes.c_int, [c_int32, c_int32] + [c_void_p] * 7),
    "lograst_pose_backward": (ctypes.c_int, [c_int32, c_int32] + [c_void_p] * 8),
    "lograst_sh_forward": (ctypes.c_int, [c_int32, c_int32, c_int32] + [c_void_p] * 6),
    "lograst_sh_backward": (ctypes.c_int, [c_int32, c_int32, c_int32] + [c_void_p] * 7 + [c_int32, c_void_p]),
    "lograst_knn_scratch_bytes": (c_size_t, [c_int32]),
    "lograst_knn_mean_dist2": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "lograst_lod_scratch_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "lograst_lod_traverse": (ctypes.c_int, [c_int32, c_int32, c_int32] + [c_void_p] * 6 + [c_int32, c_void_p, c_void_p,
                                            c_float, c_float, c_float, c_float, c_float, c_int32, c_void_p, c_uint32,
                                            c_void_p, c_size_t, c_void_p]),
    "lograst_lod_read": (ctypes.c_int, [c_void_p, ctypes.POINTER(c_uint32), ctypes.POINTER(c_uint32),
                                        ctypes.POINTER(c_uint32), c_void_p]),
    "lograst_frustum_scratch_bytes": (c_size_t, [c_int32]),
    "lograst_frustum_select": (ctypes.c_int, [c_int32, c_int32, c_void_p, c_void_p, c_void_p, ctypes.c_double]
                               + [c_void_p] * 11 + [c_size_t, c_void_p]),
    "lograst_frustum_read": (ctypes.c_int, [c_void_p, ctypes.POINTER(c_uint32), c_void_p]),
    "lograst_lod_select_scratch_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_uint32]),
    "lograst_lod_select": (ctypes.c_int, [c_int32, c_int32, c_int32] + [c_void_p] * 7 + [c_int32, c_void_p, c_void_p,
                                          c_void_p, c_int32, c_void_p, c_void_p] + [c_float] * 5 + [c_int32] * 3
                           + [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "lograst_lod_select_read": (ctypes.c_int, [c_void_p] + [ctypes.POINTER(c_uint32)] * 4 + [c_void_p]),
    "lograst_clamp_scale": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lograst_init_radius3d": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_int32] + [c_void_p] * 5),
    "lograst_id_histogram_scratch_bytes": (c_size_t, [c_int32]),
    "lograst_id_histogram": (ctypes.c_int, [c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "lograst_id_histogram_read": (ctypes.c_int, [c_void_p, ctypes.POINTER(c_uint32), c_void_p]),
    "lograst_counter_update": (ctypes.c_int, [c_int32] + [c_void_p] * 4 + [c_int32, c_void_p, c_void_p, c_int32]
                               + [c_void_p] * 10),
    "lograst_loss_scratch_bytes": (c_size_t, [c_int32] * 4),
    "lograst_loss_forward": (ctypes.c_int, [c_int32] * 4 + [c_void_p] * 6 + [c_float, c_float, c_void_p, c_void_p, c_void_p,
                                            c_size_t, c_void_p]),
    "lograst_loss_backward": (ctypes.c_int, [c_int32] * 4 + [c_void_p] * 6 + [c_float] + [c_void_p] * 5),
    "lograst_loss_gain_scratch_bytes": (c_size_t, [c_int32] * 4),
    "lograst_loss_forward_gain": (ctypes.c_int, [c_int32] * 4 + [c_void_p] * 5 + [c_float, c_float, c_void_p, c_void_p, c_void_p,
                                                 c_size_t, c_void_p]),
    "lograst_loss_backward_gain": (ctypes.c_int, [c_int32] * 4 + [c_void_p] * 5 + [c_float] + [c_void_p] * 5 + [c_size_t, c_void_p]),
    "lograst_loss_masked_scratch_bytes": (c_size_t, [c_int32] * 4),
    "lograst_loss_forward_masked": (ctypes.c_int, [c_int32] * 4 + [c_void_p] * 13 + [c_float, c_float, c_void_p, c_void_p,
                                                   c_void_p, c_size_t, c_void_p]),
    "lograst_loss_backward_masked": (ctypes.c_int, [c_int32] * 4 + [c_void_p] * 9 + [c_float] + [c_void_p] * 6
                                     + [c_size_t, c_void_p]),
    "lograst_mask_bounds_bytes": (c_size_t, [c_int32]),
    "lograst_mask_bounds": (ctypes.c_int, [c_int32] * 3 + [c_void_p, c_void_p, c_float, c_void_p, c_size_t, c_void_p]),
    "lograst_mask_bounds_read": (ctypes.c_int, [c_void_p, c_int32, c_void_p, c_void_p]),
    "lograst_corrector_step": (ctypes.c_int, [c_int32] * 4 + [ctypes.c_double, ctypes.c_double] + [c_void_p] * 7),
    "lograst_depth_loss_record_bytes": (c_size_t, [c_int32]),
    "lograst_depth_loss_forward": (ctypes.c_int, [c_int32, c_int32] + [c_void_p] * 6 + [c_int32, c_void_p, c_void_p,
                                                  ctypes.c_double, ctypes.c_double, ctypes.c_double, c_void_p, c_void_p,
                                                  c_size_t, c_void_p]),
    "lograst_depth_loss_backward": (ctypes.c_int, [c_int32, c_int32] + [c_void_p] * 6 + [c_int32] + [c_void_p] * 4),
    "lograst_eval_scratch_bytes": (c_size_t, [c_int32] * 3),
    "lograst_image_to_bgr8": (ctypes.c_int, [c_int32] * 3 + [c_void_p] * 4),
    "lograst_eval_metrics": (ctypes.c_int, [c_int32] * 3 + [c_void_p] * 4 + [c_int32, ctypes.c_double] + [c_void_p] * 4
                             + [c_size_t, c_void_p]),
    "lograst_eval_read": (ctypes.c_int, [c_void_p, ctypes.POINTER(ctypes.c_double), c_void_p]),
    "lograst_sparse_adam": (ctypes.c_int, [c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                           ctypes.POINTER(LograstAdamKey), ctypes.c_double, ctypes.c_double,
                                           ctypes.c_double, ctypes.c_double, c_void_p]),
    "lograst_densify_scratch_bytes": (c_size_t, [c_int32]),
    "lograst_densify_plan": (ctypes.c_int, [c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                            c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "lograst_densify_read": (ctypes.c_int, [c_void_p, ctypes.POINTER(c_uint32), ctypes.POINTER(c_uint32),
                                            ctypes.POINTER(c_uint32), c_void_p]),
    "lograst_densify_src_rows": (ctypes.c_int, [c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                                                c_void_p, c_void_p]),
    "lograst_densify_move_rows": (ctypes.c_int, [c_int32, c_int32, c_int32, c_void_p, c_int32,
                                                 ctypes.POINTER(LograstMoveKey), c_void_p]),
    "lograst_densify_split_uniform": (ctypes.c_int, [c_int32, c_int32, c_int32, c_float, c_int32] + [c_void_p] * 7),
    "lograst_densify_tree": (ctypes.c_int, [c_int32] * 5 + [c_void_p] * 14),
    "lograst_decide_scratch_bytes": (c_size_t, [c_int32]),
    "lograst_decide_depth": (ctypes.c_int, [c_int32, ctypes.POINTER(LograstDecideDepthArgs), c_void_p, c_size_t, c_void_p]),
    "lograst_decide_init": (ctypes.c_int, [c_int32, ctypes.POINTER(LograstDecideInitArgs), c_void_p, c_size_t, c_void_p]),
    "lograst_decide_read": (ctypes.c_int, [c_void_p, ctypes.POINTER(LograstDecideRecord), c_size_t, c_void_p]),
    "lograst_decide_child_radius_max": (ctypes.c_int, [c_int32, c_int32, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "lograst_activate_backward_adam": (ctypes.c_int, [c_int32] + [c_void_p] * 4 + [c_int32, c_int32] + [c_void_p] * 6 +
                                       [c_int32, c_void_p, c_void_p, ctypes.POINTER(LograstAdamKey), ctypes.c_double,
                                        ctypes.c_double, ctypes.c_double, ctypes.c_double, c_void_p]),
    "lograst_accumulate_target_floats": (c_size_t, [c_int32] * 3),
    "lograst_activate_backward_accumulate": (ctypes.c_int, [c_int32] + [c_void_p] * 4 + [c_int32, c_int32] + [c_void_p] * 6 +
                                             [c_int32, c_void_p, c_void_p, ctypes.POINTER(LograstAccTarget), c_void_p,
                                              c_void_p]),
    "lograst_accumulated_adam": (ctypes.c_int, [c_int32, c_void_p, ctypes.POINTER(LograstAdamKey),
                                                ctypes.POINTER(c_int32), ctypes.c_double, ctypes.c_double,
                                                ctypes.c_double, ctypes.c_double, c_void_p, c_void_p]),
    "lograst_gather_activate": (ctypes.c_int, [c_int32, c_int32] + [c_void_p] * 7 + [c_int32, c_int32] + [c_void_p] * 12),
    "lograst_activate_backward": (ctypes.c_int, [c_int32] + [c_void_p] * 4 + [c_int32, c_int32] + [c_void_p] * 11),
    "lograst_profile_enable": (None, [ctypes.c_int]),
    "lograst_profile_reset": (None, []),
    "lograst_profile_read": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)]),
    "lograst_kernel_name": (ctypes.c_char_p, [ctypes.c_int]),
}

EXPORTS = tuple(_SIGNATURES)


def lib():
    """Loads liblograst.so (after torch, so both share one HIP runtime).  Raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LograstError(
                f"{LIB_PATH} is missing: build it with `python -m log_amd.build` (hipcc, gfx950). "
                "log_amd has no CPU fallback.")
        import torch  # noqa: F401  -- loads libamdhip64 first so the .so binds to torch's runtime
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lograst_version() != 4:
            raise LograstError("liblograst.so version mismatch; rebuild")
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise LograstError(f"liblograst error {rc}: {lib().lograst_last_error().decode()}")


def profile_enable(on=True):
    lib().lograst_profile_enable(1 if on else 0)


def profile_reset():
    lib().lograst_profile_reset()


def profile_read():
    """-> {kernel_name: (total_ms, launches)} since the last reset (synchronises recorded events)."""
    ms = (ctypes.c_double * NUM_KERNEL_SLOTS)()
    cnt = (ctypes.c_int64 * NUM_KERNEL_SLOTS)()
    check(lib().lograst_profile_read(ms, cnt))
    return {lib().lograst_kernel_name(i).decode(): (ms[i], cnt[i]) for i in range(NUM_KERNEL_SLOTS) if cnt[i]}
