"""ctypes binding of libdqoraster.so (include/dqo_raster.h).  Shared by the drop-in packages in this directory.

There is NO CPU fallback: if the HIP library is missing or a tensor is not on the GPU the call raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdqoraster.so")

c_f, c_i32, c_vp = ctypes.c_float, ctypes.c_int32, ctypes.c_void_p


class DqoRastParams(ctypes.Structure):
    _fields_ = [("P", c_i32), ("D", c_i32), ("M", c_i32), ("W", c_i32), ("H", c_i32), ("prefiltered", c_i32), ("debug", c_i32),
                ("tanfovx", c_f), ("tanfovy", c_f), ("cx", c_f), ("cy", c_f), ("scale_modifier", c_f), ("color_sigma", c_f),
                ("opaque_threshold", c_f), ("depth_threshold", c_f), ("normal_threshold", c_f), ("T_threshold", c_f)]


class DqoRastInputs(ctypes.Structure):
    _fields_ = [(n, c_vp) for n in ("bg", "means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp",
                                    "viewmatrix", "projmatrix", "campos", "tile_mask", "row_flags")]


class DqoRastOutputs(ctypes.Structure):
    _fields_ = [(n, c_vp) for n in ("out_color", "out_depth", "out_hit_color", "out_hit_depth", "out_hit_color_weight",
                                    "out_hit_depth_weight", "out_T", "n_touched", "radii")]


class DqoLossTap(ctypes.Structure):
    _fields_ = [("gt_color", c_vp), ("gt_depth", c_vp), ("render_mask", c_vp), ("out_color", c_vp), ("out_depth", c_vp),
                ("color_weight", c_f), ("depth_weight", c_f), ("add_depth_thres", c_f), ("loss_out", c_vp), ("grad_scale", c_vp),
                ("per_object", c_i32)]


class DqoObjectGate(ctypes.Structure):
    _fields_ = [("gaussian_object", c_vp), ("pixel_object", c_vp), ("tile_objects", c_vp)]


class DqoRastCtx(ctypes.Structure):
    _fields_ = [("geom", c_vp), ("geom_bytes", ctypes.c_size_t), ("binning", c_vp), ("binning_bytes", ctypes.c_size_t),
                ("image", c_vp), ("image_bytes", ctypes.c_size_t), ("inst_capacity", ctypes.c_int64), ("tile_bucket_capacity", c_i32), ("keep_tile_order", c_i32), ("loss_tap", c_vp),
                ("object_gate", c_vp), ("list_split", c_i32), ("frame_prezeroed", c_i32)]


class DqoRastGrads(ctypes.Structure):
    _fields_ = [(n, c_vp) for n in ("dL_dmeans3D", "dL_dsh", "dL_dcolors", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dcov3D",
                                    "dL_dmeans2D")] + [("skip_culled_rows", c_i32)]


class DqoRastParamInputs(ctypes.Structure):
    """The parameter form's raw inputs (dqo_rast_*_params, ABI 5 symbols-only addition)."""
    _fields_ = [("features_dc", c_vp), ("features_rest", c_vp), ("rest", c_i32), ("opacity_raw", c_vp), ("scaling_raw", c_vp),
                ("rotation_raw", c_vp)]


class DqoRastParamGrads(ctypes.Structure):
    _fields_ = [(n, c_vp) for n in ("dL_dfeatures_dc", "dL_dfeatures_rest", "dL_dopacity_raw", "dL_dscaling_raw", "dL_drotation_raw")]


class DqoRastHeader(ctypes.Structure):
    _fields_ = [("num_rendered", ctypes.c_uint32), ("num_tiles", ctypes.c_uint32), ("overflow", ctypes.c_uint32),
                ("max_tile_count", ctypes.c_uint32), ("num_visible", ctypes.c_uint32), ("num_candidates", ctypes.c_uint32),
                ("stage", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class DqoProfileEntry(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("total_ms", ctypes.c_double), ("calls", ctypes.c_uint32)]


class DqoAdamStep(ctypes.Structure):
    _fields_ = ([("P", c_i32), ("M", c_i32), ("step", c_i32), ("beta1", c_f), ("beta2", c_f), ("eps", c_f), ("lr_xyz", c_f),
                 ("lr_f_dc", c_f), ("lr_f_rest", c_f), ("lr_opacity", c_f), ("lr_scaling", c_f), ("lr_rotation", c_f)] +
                [(n, c_vp) for n in ("xyz", "shs", "opacity_raw", "scaling_raw", "rotation_raw", "g_means3D", "g_sh", "g_opacity",
                                     "g_scales", "g_rotations", "m_xyz", "m_shs", "m_opacity", "m_scaling", "m_rotation", "v_xyz",
                                     "v_shs", "v_opacity", "v_scaling", "v_rotation", "act_opacity", "act_scales", "act_rotations", "radii", "step_dev", "moment_live",
                                     "attach_mask", "init_xyz", "init_scaling_raw", "init_rotation_raw")] +
                [("attach_count", c_i32), ("attach_partial", c_vp), ("frame_header", c_vp), ("block_ticket", c_vp), ("bias_table", c_vp), ("attach_gains", c_vp),
                 ("row_flags", c_vp), ("confidence", c_vp), ("lr_table", c_vp), ("record_ctx", c_vp), ("record_W", c_i32), ("record_H", c_i32)])

ROW_FROZEN, ROW_HIDDEN = 1, 2  # DQO_ROW_FROZEN / DQO_ROW_HIDDEN (include/dqo_raster.h)


class DqoAdamTensor(ctypes.Structure):
    _fields_ = [("p", c_vp), ("g", c_vp), ("m", c_vp), ("v", c_vp), ("n", ctypes.c_int64), ("lr", ctypes.c_double)]


class DqoLifecycle(ctypes.Structure):
    """dqo_map_lifecycle_vote / dqo_map_lifecycle_rows (ABI 5 symbols-only addition)."""
    _fields_ = ([(n, c_i32) for n in ("P", "W", "H", "tick", "unstable_time_window", "delete_thresh", "stable_oversized", "use_votes")] +
                [(n, c_f) for n in ("stable_confidence_thres", "add_color_thres", "add_depth_thres")] +
                [(n, c_vp) for n in ("xyz", "opacity_raw", "scaling_raw", "confidence", "alive", "row_flags", "stable", "add_tick",
                                     "depth_error_counter", "color_error_counter", "park", "vote", "workspace")] +
                [("workspace_bytes", ctypes.c_size_t), ("stats", c_vp), ("render_header", c_vp)])


class DqoGrowthSample(ctypes.Structure):
    """dqo_growth_sample (ABI 5 symbols-only addition)."""
    _fields_ = ([(n, c_i32) for n in ("W", "H", "first_frame", "uniform_sample_num", "capacity", "key_bits", "M", "identity_rotation")] +
                [("seed", ctypes.c_uint64)] +
                [(n, c_f) for n in ("add_transmission_thres", "add_depth_thres", "add_color_thres", "transmission_sample_ratio",
                                    "error_sample_ratio", "init_opacity")] +
                [(n, c_vp) for n in ("vertex", "normal", "color", "depth", "instance", "T", "render_depth", "render_color", "depth_index",
                                     "xyz", "scales", "rotations", "opacity", "shs", "obj_id", "out_normal", "pixel", "header", "workspace")] +
                [("workspace_bytes", ctypes.c_size_t)])


class DqoWindowBank(ctypes.Structure):
    """dqo_window_bank_select (ABI 5 symbols-only addition): the bank's parts, the destination a captured graph reads, the schedule, the
    state words, the lost-frame log and the render's header."""
    _fields_ = ([(n, c_i32) for n in ("W", "H", "K_cap", "n")] +
                [(n, c_vp) for n in ("camera", "gt_color", "gt_depth", "render_mask", "tile_mask", "pixel_object", "tile_objects", "dst_bg",
                                     "dst_viewmatrix", "dst_projmatrix", "dst_campos", "dst_gt_color", "dst_gt_depth", "dst_render_mask",
                                     "dst_tile_mask", "dst_pixel_object", "dst_tile_objects", "schedule", "state", "lost", "render_header")])


class DqoTrajRepose(ctypes.Structure):
    """dqo_traj_repose (ABI 5 symbols-only addition): the trajectory's store and header, the corrected poses, the target table
    (REPOSE_TARGET_FIELDS per entry), the projection, a keyframe bank's state words and the counts."""
    _fields_ = ([(n, c_i32) for n in ("cap", "n_new", "T", "flags")] +
                [(n, c_vp) for n in ("pose", "header", "new_pose", "targets", "projection", "bank_state", "stats")])


class DqoReposeTarget(ctypes.Structure):
    _fields_ = [("row", ctypes.c_int64)] + [(n, c_vp) for n in ("c2w", "w2c", "viewmatrix", "projmatrix", "campos")]


# a DqoReposeTarget as the columns of an int64 [T,6] device table, and DQO_REPOSE_HAS_PROJMATRIX
REPOSE_TARGET_FIELDS = ("row", "c2w", "w2c", "viewmatrix", "projmatrix", "campos")
REPOSE_HAS_PROJMATRIX = 1

TICKET_WORDS = 16 + 16 * 64  # DQO_TICKET_WORDS
# the state words of the keyframe bank behind its ticket (DQO_WINDOW_BANK_* of include/dqo_raster.h), in order, and the state's size
WINDOW_BANK_WORDS = ("cursor", "n", "prev_k", "prev_m", "force", "overrun", "lost_count")
WINDOW_BANK_STATE_WORDS = TICKET_WORDS + 48  # DQO_WINDOW_BANK_STATE_WORDS

EXPORTS = ("dqo_abi_version", "dqo_abi_sizeof", "dqo_last_error", "dqo_profile_enable", "dqo_profile_collect", "dqo_map_activate",
           "dqo_map_loss_workspace_bytes", "dqo_map_loss_fwd_bwd", "dqo_map_ssim_workspace_bytes", "dqo_map_ssim_fwd_bwd", "dqo_map_adam_step", "dqo_adam_multi_dev", "dqo_map_attach_workspace_bytes",
           "dqo_map_attach_loss_fwd_bwd", "dqo_adam_multi", "dqo_accumulate_gaussian_error", "dqo_accumulate_gaussian_confidence", "dqo_rast_geom_bytes", "dqo_rast_image_bytes",
           "dqo_rast_binning_bytes", "dqo_rast_binning_bytes_bucketed",
           "dqo_rast_backward_workspace_bytes", "dqo_rast_forward_prepare", "dqo_rast_read_header", "dqo_rast_forward_render",
           "dqo_rast_forward", "dqo_rast_forward_train", "dqo_rast_forward_async", "dqo_rast_backward", "dqo_rast_backward_adam", "dqo_mark_visible", "dqo_knn3_workspace_bytes", "dqo_knn3",
           "dqo_quadric_iou_fwd_bwd", "dqo_quadric_adam", "dqo_tile_count_mask", "dqo_transmission_mask", "dqo_tile_color_error", "dqo_knn3_query_workspace_bytes",
           "dqo_knn3_query", "dqo_knn3_query_within", "dqo_knn3_query_grouped", "dqo_icp_workspace_bytes", "dqo_icp_normal_equations",
           "dqo_attach_pixels", "dqo_attach_decide", "dqo_growth_scales", "dqo_growth_inside", "dqo_error_maps", "dqo_map_history_merge",
           "dqo_rast_forward_prepare_params", "dqo_rast_forward_render_params", "dqo_rast_forward_async_params", "dqo_rast_backward_params",
           "dqo_icp_gauss_newton", "dqo_track_preprocess_workspace_bytes", "dqo_track_preprocess", "dqo_track_pyramid_pixels",
           "dqo_track_pyramid_workspace_bytes", "dqo_track_pyramid", "dqo_track_fill_model_depth", "dqo_track_p2p_workspace_bytes",
           "dqo_track_p2p_loss", "dqo_map_lifecycle_workspace_bytes", "dqo_map_lifecycle_vote", "dqo_map_lifecycle_rows",
           "dqo_growth_sample_workspace_bytes", "dqo_growth_sample", "dqo_eval_picture_workspace_bytes", "dqo_eval_picture",
           "dqo_eval_ms_ssim_workspace_bytes", "dqo_eval_ms_ssim",
           "dqo_eval_lpips_weight_floats", "dqo_eval_lpips_workspace_bytes", "dqo_eval_lpips",
           "dqo_nn1_workspace_bytes", "dqo_nn1", "dqo_eval_pcd_workspace_bytes", "dqo_eval_pcd", "dqo_window_masks_workspace_bytes",
           "dqo_nn1_grouped_workspace_bytes", "dqo_nn1_grouped", "dqo_eval_pcd_grouped_workspace_bytes", "dqo_eval_pcd_grouped", "dqo_map_pack_rows_by_object",
           "dqo_window_masks", "dqo_surfel_densify_workspace_bytes", "dqo_surfel_densify", "dqo_map_pack_workspace_bytes",
           "dqo_map_pack_rows", "dqo_map_unpack_rows", "dqo_mesh_sample_workspace_bytes", "dqo_mesh_sample",
           "dqo_objmap_frame", "dqo_objmap_optimize", "dqo_objmap_mean_iou", "dqo_traj_append", "dqo_track_world_maps",
           "dqo_eval_ate_workspace_bytes", "dqo_eval_ate", "dqo_prune_workspace_bytes", "dqo_prune_cameras", "dqo_prune_touch",
           "dqo_prune_rows", "dqo_tsdf_workspace_bytes", "dqo_tsdf_clear", "dqo_tsdf_integrate", "dqo_tsdf_extract",
           "dqo_mesh_components_workspace_bytes", "dqo_mesh_smooth_workspace_bytes", "dqo_mesh_normals_workspace_bytes",
           "dqo_mesh_components", "dqo_mesh_smooth", "dqo_mesh_normals", "dqo_mesh_simplify_workspace_bytes", "dqo_mesh_simplify",
           "dqo_mesh_cull_workspace_bytes", "dqo_mesh_cull", "dqo_mesh_sample_counted_workspace_bytes", "dqo_mesh_sample_counted",
           "dqo_mesh_render_depth_workspace_bytes", "dqo_mesh_render_depth", "dqo_eval_depth_l1_workspace_bytes", "dqo_eval_depth_l1",
           "dqo_mesh_render_depth_clip", "dqo_mesh_cull_faces", "dqo_window_bank_arm", "dqo_window_bank_select", "dqo_traj_repose")

_lib = None


def lib():
    """Load libdqoraster.so (built by `make -C dqo-map_amd/csrc` / __graft_entry__.build()).  Fails loudly when absent."""
    global _lib
    if _lib is None:
        # torch first: it loads its bundled HIP runtime; libdqoraster.so then binds to that same copy (same SONAME).  The
        # other order puts two ROCr instances in one process and the second one sees "no ROCm-capable device".
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: the HIP extension is not built (run __graft_entry__.build()). "
                               "There is no CPU fallback for this operator.")
        L = ctypes.CDLL(LIB_PATH)
        c_sz, c_i64, c_u64, c_d = ctypes.c_size_t, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
        P = ctypes.POINTER
        # every size query returns size_t (ctypes' default c_int would cut it at 2 GiB): by rule, not per export
        for n in EXPORTS:
            if "_bytes" in n or n == "dqo_abi_sizeof":  # (*_bytes and dqo_rast_binning_bytes_bucketed)
                getattr(L, n).restype = c_sz
        L.dqo_last_error.restype = ctypes.c_char_p
        L.dqo_track_pyramid_pixels.restype = c_i64
        # argument types, grouped as the entry points are in csrc/ (a new operator adds one block).  dqo_capi.hip, rast_forward.hip:
        L.dqo_abi_sizeof.argtypes = [c_i32]
        L.dqo_profile_enable.argtypes = [ctypes.c_int]
        L.dqo_profile_collect.argtypes = [P(DqoProfileEntry), ctypes.c_int, ctypes.c_int]
        L.dqo_rast_geom_bytes.argtypes = [c_i32, c_i32, c_i32]
        L.dqo_rast_image_bytes.argtypes = [c_i32, c_i32]
        L.dqo_rast_binning_bytes.argtypes = [c_i64]
        L.dqo_rast_binning_bytes_bucketed.argtypes = [c_i64, c_i32, c_i32, c_i32]
        L.dqo_rast_backward_workspace_bytes.argtypes = [c_i64]
        L.dqo_rast_forward_prepare.argtypes = [P(DqoRastParams), P(DqoRastInputs), P(DqoRastOutputs), P(DqoRastCtx), c_vp]
        L.dqo_rast_forward_render.argtypes = L.dqo_rast_forward_prepare.argtypes
        L.dqo_rast_forward.argtypes = L.dqo_rast_forward_prepare.argtypes
        L.dqo_rast_forward_train.argtypes = L.dqo_rast_forward_prepare.argtypes
        L.dqo_rast_forward_async.argtypes = L.dqo_rast_forward_prepare.argtypes[:4] + [c_vp, c_vp, c_vp]
        L.dqo_rast_read_header.argtypes = [P(DqoRastCtx), P(DqoRastHeader), c_vp]
        L.dqo_rast_backward.argtypes = [P(DqoRastParams), P(DqoRastInputs), P(DqoRastCtx), c_vp, c_vp, c_vp, P(DqoRastGrads), c_vp, c_sz, c_vp]
        L.dqo_rast_backward_adam.argtypes = [P(DqoRastParams), P(DqoRastInputs), P(DqoRastCtx), c_vp, c_vp, P(DqoAdamStep), c_vp, c_sz, c_vp]
        L.dqo_rast_forward_prepare_params.argtypes = [P(DqoRastParams), P(DqoRastInputs), P(DqoRastParamInputs), P(DqoRastOutputs),
                                                      P(DqoRastCtx), c_vp]
        L.dqo_rast_forward_render_params.argtypes = L.dqo_rast_forward_prepare_params.argtypes
        L.dqo_rast_forward_async_params.argtypes = L.dqo_rast_forward_prepare_params.argtypes[:5] + [c_vp, c_vp, c_vp]
        L.dqo_rast_backward_params.argtypes = [P(DqoRastParams), P(DqoRastInputs), P(DqoRastParamInputs), P(DqoRastCtx), c_vp, c_vp, c_vp,
                                               P(DqoRastGrads), P(DqoRastParamGrads), c_vp, c_sz, c_vp]
        L.dqo_mark_visible.argtypes = [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]
        # knn.hip
        L.dqo_knn3_query_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_knn3_query.argtypes = [c_i32, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]
        L.dqo_knn3_query_within.argtypes = [c_i32, c_vp, c_i32, c_vp, c_f, c_vp, c_vp, c_vp, c_sz, c_vp]
        L.dqo_knn3_query_grouped.argtypes = [c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_f, c_vp, c_vp, c_vp, c_sz, c_vp]
        L.dqo_knn3_workspace_bytes.argtypes = [c_i32]
        L.dqo_knn3.argtypes = [c_i32, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]
        L.dqo_nn1_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_nn1.argtypes = [c_i32, c_vp, c_vp, c_i32] + [c_vp] * 7 + [c_sz, c_vp]
        L.dqo_nn1_grouped_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_nn1_grouped.argtypes = [c_i32, c_vp, c_vp, c_i32] + [c_vp] * 7 + [c_sz, c_vp]
        # quadric.hip
        L.dqo_quadric_iou_fwd_bwd.argtypes = [c_i32] + [c_vp] * 12
        L.dqo_quadric_adam.argtypes = [c_i32, c_i32] + [c_vp] * 9
        # map_fused.hip
        L.dqo_map_activate.argtypes = [c_i32] + [c_vp] * 7
        L.dqo_map_loss_fwd_bwd.argtypes = [c_i32, c_i32] + [c_vp] * 6 + [c_f, c_f, c_f] + [c_vp] * 4 + [c_sz, c_vp]
        L.dqo_map_attach_workspace_bytes.argtypes = [c_i32]
        L.dqo_map_history_merge.argtypes = [c_i32, c_i32, c_f, c_i32] + [c_vp] * 12
        L.dqo_map_attach_loss_fwd_bwd.argtypes = [c_i32] + [c_vp] * 7 + [c_i32] + [c_vp] * 5 + [c_sz, c_vp]
        L.dqo_adam_multi.argtypes = [c_vp, c_i32, c_i32, c_d, c_d, c_d, c_vp]
        L.dqo_adam_multi_dev.argtypes = [c_vp, c_i32, c_vp, c_i32, c_d, c_d, c_d, c_vp]
        L.dqo_map_adam_step.argtypes = [P(DqoAdamStep), c_vp]
        # map_ssim.hip
        L.dqo_map_ssim_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_map_ssim_fwd_bwd.argtypes = [c_i32, c_i32, c_vp, c_vp, c_f, c_vp, c_vp, c_i32, c_vp, c_vp, c_sz, c_vp]
        # map_error.hip
        L.dqo_accumulate_gaussian_error.argtypes = [c_i32] * 3 + [c_vp] * 5 + [c_f] * 3 + [c_i32] + [c_vp] * 6
        L.dqo_accumulate_gaussian_confidence.argtypes = [c_i32] * 3 + [c_vp] * 7
        # map_tilemask.hip
        L.dqo_tile_count_mask.argtypes = [c_i32, c_i32, c_vp, c_vp, c_vp]
        L.dqo_transmission_mask.argtypes = [c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]
        L.dqo_tile_color_error.argtypes = [c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]
        L.dqo_window_masks_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_window_masks.argtypes = [c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_f, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]
        # map_attach.hip
        L.dqo_attach_pixels.argtypes = [c_i32, c_vp, c_vp, c_f, c_f, c_f, c_f, c_i32, c_i32] + [c_vp] * 5
        L.dqo_attach_decide.argtypes = [c_i32] + [c_vp] * 10 + [c_f, c_f, c_vp, c_vp]
        # map_growth.hip
        L.dqo_growth_scales.argtypes = [c_i32] + [c_vp] * 7 + [c_f, c_f, c_f, c_vp, c_vp, c_vp]
        L.dqo_growth_inside.argtypes = [c_i32] + [c_vp] * 5
        L.dqo_error_maps.argtypes = [c_i32, c_i32] + [c_vp] * 9
        # map_lifecycle.hip
        L.dqo_map_lifecycle_workspace_bytes.argtypes = [c_i32]
        L.dqo_map_lifecycle_vote.argtypes = [P(DqoLifecycle)] + [c_vp] * 7
        L.dqo_map_lifecycle_rows.argtypes = [P(DqoLifecycle), c_vp]
        # map_sample.hip
        L.dqo_growth_sample_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_growth_sample.argtypes = [P(DqoGrowthSample), c_vp]
        # map_densify.hip, map_meshsample.hip
        L.dqo_surfel_densify_workspace_bytes.argtypes = [c_i32] * 4
        L.dqo_surfel_densify.argtypes = [c_i32] + [c_vp] * 4 + [c_i32] * 3 + [c_vp, c_i32, c_u64, c_i64] + [c_vp] * 6 + [c_sz, c_vp]
        L.dqo_mesh_sample_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_mesh_sample.argtypes = [c_i32, c_vp, c_i32, c_vp, c_i32, c_u64] + [c_vp] * 5 + [c_sz, c_vp]
        L.dqo_mesh_sample_counted_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_mesh_sample_counted.argtypes = [c_vp] * 3 + [c_i32] * 3 + [c_u64] + [c_vp] * 5 + [c_sz, c_vp]
        # map_eval.hip, map_msssim.hip
        L.dqo_eval_picture_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_eval_picture.argtypes = [c_i32, c_i32] + [c_vp] * 5 + [c_f, c_f, c_vp, c_vp, c_i32, c_vp, c_sz, c_vp]
        L.dqo_eval_pcd_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_eval_pcd.argtypes = [c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, P(c_f), c_vp, c_i32, c_vp, c_sz, c_vp]
        L.dqo_eval_pcd_grouped_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_eval_pcd_grouped.argtypes = [c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, P(c_f), c_vp, c_i64, c_i64, c_vp, c_sz, c_vp]
        L.dqo_eval_ms_ssim_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_eval_ms_ssim.argtypes = [c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_sz, c_vp]
        # map_lpips.hip
        L.dqo_eval_lpips_weight_floats.restype = c_sz
        L.dqo_eval_lpips_weight_floats.argtypes = [c_i32]
        L.dqo_eval_lpips_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_eval_lpips.argtypes = [c_i32, c_i32, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_sz, c_vp]
        # map_checkpoint.hip
        L.dqo_map_pack_workspace_bytes.argtypes = [c_i32]
        L.dqo_map_pack_rows.argtypes = [c_i32] * 3 + [c_vp] * 9 + [c_i64, c_vp, c_vp, c_sz, c_vp]
        L.dqo_map_pack_rows_by_object.argtypes = [c_i32] * 3 + [c_vp] * 10 + [c_i64, c_vp, c_vp, c_sz, c_vp]
        L.dqo_map_unpack_rows.argtypes = [c_i32] * 5 + [c_vp] * 8
        # map_objects.hip
        L.dqo_objmap_frame.argtypes = [c_i32] * 3 + [c_vp] * 9 + [c_i32] + [c_vp] * 7 + [c_i32] * 3 + [c_u64] + [c_vp] * 6
        L.dqo_objmap_optimize.argtypes = [c_i32] * 2 + [c_vp] * 9 + [c_i32, c_u64, c_vp, c_vp]
        L.dqo_objmap_mean_iou.argtypes = [c_i32] * 2 + [c_vp] * 9
        # map_traj.hip
        L.dqo_traj_append.argtypes = [c_i32] + [c_vp] * 14 + [c_i32, c_d, c_d, c_vp]
        L.dqo_track_world_maps.argtypes = [c_i32, c_i32] + [c_vp] * 6
        L.dqo_eval_ate_workspace_bytes.argtypes = [c_i32]
        L.dqo_eval_ate.argtypes = [c_i32, c_vp, c_i64, c_i64, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_sz, c_vp]
        # map_prune.hip
        L.dqo_prune_workspace_bytes.argtypes = [c_i32]
        L.dqo_prune_cameras.argtypes = [c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_d, c_d, c_vp, c_vp, c_vp, c_vp]
        L.dqo_prune_touch.argtypes = [c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]
        L.dqo_prune_rows.argtypes = [c_i32] + [c_vp] * 12 + [c_i32, c_i32, c_vp, c_sz, c_vp, c_vp]
        # map_tsdf.hip
        L.dqo_tsdf_workspace_bytes.argtypes = [c_i32] * 3
        L.dqo_tsdf_clear.argtypes = [c_i32] * 3 + [c_vp] * 5
        L.dqo_tsdf_integrate.argtypes = [c_i32] * 3 + [c_f] * 5 + [c_vp] * 4 + [c_i32, c_i32, c_vp, c_vp] + [c_f] * 4 + [c_vp, c_f, c_vp, c_vp]
        L.dqo_tsdf_extract.argtypes = [c_i32] * 3 + [c_f] * 4 + [c_vp] * 6 + [c_i32, c_i32, c_vp, c_vp, c_sz, c_vp]
        # map_meshops.hip
        for n in ("components", "smooth", "normals", "simplify"):
            getattr(L, f"dqo_mesh_{n}_workspace_bytes").argtypes = [c_i32, c_i32]
        L.dqo_mesh_components.argtypes = [c_vp] * 4 + [c_i32] * 4 + [c_vp] * 3 + [c_i32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]
        L.dqo_mesh_smooth.argtypes = [c_vp] * 4 + [c_i32] * 3 + [c_d, c_d, c_i32, c_vp, c_sz, c_vp]
        L.dqo_mesh_normals.argtypes = [c_vp] * 3 + [c_i32, c_i32, c_vp, c_vp, c_sz, c_vp]
        L.dqo_mesh_simplify.argtypes = [c_vp] * 4 + [c_i32, c_i32] + [c_d] * 4 + [c_vp] * 3 + [c_i32, c_i32, c_vp, c_vp, c_sz, c_vp]
        # map_meshcull.hip
        L.dqo_mesh_cull_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_mesh_cull.argtypes = ([c_vp] * 4 + [c_i32] * 3 + [c_vp] * 2 + [c_i32] * 2 + [c_f] * 4 + [c_vp] + [c_f] * 3 + [c_i32] + [c_vp] * 3 +
                                    [c_i32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp])
        L.dqo_mesh_cull_faces.argtypes = ([c_vp] * 4 + [c_i32] * 3 + [c_vp] + [c_i32] * 2 + [c_vp] * 3 + [c_f] * 2 + [c_i32] + [c_vp] * 3 +
                                          [c_i32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp])
        # map_meshrender.hip; map_eval.hip's depth L1
        L.dqo_mesh_render_depth_workspace_bytes.argtypes = [c_i32, c_i32, c_i32]
        L.dqo_mesh_render_depth.argtypes = ([c_vp] * 3 + [c_i32] * 3 + [c_vp] * 2 + [c_i32] * 2 + [c_f] * 6 + [c_vp] * 4 + [c_sz, c_vp])
        L.dqo_mesh_render_depth_clip.argtypes = L.dqo_mesh_render_depth.argtypes
        L.dqo_eval_depth_l1_workspace_bytes.argtypes = [c_i32, c_i32, c_i32]
        L.dqo_eval_depth_l1.argtypes = [c_i32] * 3 + [c_vp] * 3 + [c_f] + [c_vp] * 2 + [c_sz, c_vp]
        # map_window_bank.hip
        L.dqo_window_bank_arm.argtypes = [c_vp, c_i32, c_vp]
        L.dqo_window_bank_select.argtypes = [P(DqoWindowBank), c_vp]
        # map_repose.hip
        L.dqo_traj_repose.argtypes = [P(DqoTrajRepose), c_vp]
        # icp.hip, track.hip
        L.dqo_icp_normal_equations.argtypes = [c_i32, c_i32] + [c_vp] * 5 + [c_f] * 6 + [c_vp] * 4 + [c_sz, c_vp]
        L.dqo_icp_gauss_newton.argtypes = [c_i32, c_i32] + [c_vp] * 6 + [c_f] * 4 + [c_vp] * 2 + [c_sz, c_vp]
        L.dqo_track_preprocess_workspace_bytes.argtypes = [c_i32, c_i32]
        L.dqo_track_preprocess.argtypes = [c_i32, c_i32, c_vp, c_vp] + [c_f] * 3 + [c_i32] + [c_vp] * 6 + [c_sz, c_vp]
        L.dqo_track_pyramid_pixels.argtypes = [c_i32, c_i32, c_i32]
        L.dqo_track_pyramid.argtypes = [c_i32, c_i32, c_i32] + [c_vp] * 5 + [c_sz, c_vp]
        L.dqo_track_fill_model_depth.argtypes = [c_i32, c_i32] + [c_vp] * 4 + [c_f, c_f, c_vp]
        L.dqo_track_p2p_loss.argtypes = [c_i32, c_i32] + [c_vp] * 4 + [c_f] + [c_vp] * 5 + [c_sz, c_vp]
        if L.dqo_abi_version() != 5:
            raise RuntimeError("libdqoraster.so ABI version mismatch")
        for k, st in enumerate((DqoRastParams, DqoRastInputs, DqoRastOutputs, DqoRastCtx, DqoRastGrads, DqoRastHeader, DqoProfileEntry,
                                DqoAdamStep, DqoLossTap, DqoObjectGate, DqoAdamTensor, DqoRastParamInputs, DqoRastParamGrads, None,
                                DqoLifecycle, DqoGrowthSample, None, DqoWindowBank, DqoTrajRepose, DqoReposeTarget)):  # (None: indices 13 and 16 are unused)
            if st is not None and L.dqo_abi_sizeof(k) != ctypes.sizeof(st):
                raise RuntimeError(f"libdqoraster.so: struct {st.__name__} is {L.dqo_abi_sizeof(k)} bytes in the library, "
                                   f"{ctypes.sizeof(st)} in the binding")
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError(lib().dqo_last_error().decode() or f"libdqoraster error {rc}")


def ptr(t):
    """Raw device pointer of a torch tensor (None / empty tensor -> NULL, like an empty tensor's data_ptr in the reference)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and t.numel() > 0 and not t.is_cuda:
            raise RuntimeError("libdqoraster operators need GPU (ROCm) tensors; there is no CPU path. Got a tensor on "
                               f"{t.device}.")


def require_gpu_op(principal, *others):
    """The device rule of an operator's wrapper.  `principal` (a tensor, or a tuple of tensors) names the device the call runs on: it
    must be a GPU tensor even when it is empty.  `others` (None allowed) follow require_gpu's rule: an empty one may live anywhere."""
    principal = principal if isinstance(principal, tuple) else (principal,)
    require_gpu(*principal, *others)
    if not all(t.is_cuda for t in principal):
        raise RuntimeError("libdqoraster operators need GPU (ROCm) tensors; there is no CPU path.")


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def profile_enable(on):
    lib().dqo_profile_enable(1 if on else 0)


def profile_collect(reset=True):
    """{kernel name: (total_ms, calls)} of every launch bracketed since the last reset (synchronises)."""
    buf = (DqoProfileEntry * 64)()
    n = lib().dqo_profile_collect(buf, 64, 1 if reset else 0)
    return {buf[i].name.decode(): (buf[i].total_ms, buf[i].calls) for i in range(n)}
