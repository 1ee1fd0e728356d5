"""ctypes binding of the C ABI in include/karto_hip.h (libkartohip.so).

The library is the product: if it is missing or cannot be loaded this module raises -- there is
no Python / CPU fallback path."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KH_LIBRARY") or os.path.join(HERE, "libkartohip.so")     # KH_LIBRARY: another build of the same sources (measurements)

KH_OK, KH_ERR_INVALID_ARG, KH_ERR_NO_DEVICE, KH_ERR_HIP, KH_ERR_SEARCH, KH_ERR_NOT_FOUND, KH_ERR_SOLVER, KH_ERR_IO = range(8)
KH_GRAPH_TEXT, KH_GRAPH_BINARY = 0, 1

dptr = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
iptr = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
bptr = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")


class KhScan(C.Structure):
    _fields_ = [("n", C.c_int32), ("ranges", C.POINTER(C.c_double)), ("points_xy", C.POINTER(C.c_double)),
                ("sensor_pose", C.c_double * 3), ("device_points_xy", C.c_void_p)]


class KhMatchParams(C.Structure):
    _fields_ = [("coarse_search_angle_offset", C.c_double), ("coarse_angle_resolution", C.c_double),
                ("fine_search_angle_offset", C.c_double), ("use_response_expansion", C.c_int32),
                ("distance_variance_penalty", C.c_double), ("minimum_distance_penalty", C.c_double),
                ("angle_variance_penalty", C.c_double), ("minimum_angle_penalty", C.c_double)]


class KhGridInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("width", "height", "width_step", "data_size", "roi_x", "roi_y", "roi_w",
                                          "roi_h", "kernel_size", "search_side")] + \
               [(k, C.c_double) for k in ("offset_x", "offset_y", "scale")]


class KhMapView(C.Structure):
    """kh_map_view: a borrowed device view of a map's cell states (valid until its source is next updated, grown, cleared or destroyed)"""
    _fields_ = [("device_cells", C.c_void_p), ("device", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("width_step", C.c_int32), ("ox", C.c_int32), ("oy", C.c_int32), ("anchor", C.c_double * 2), ("scale", C.c_double)]


KH_LOSS_NONE, KH_LOSS_HUBER, KH_LOSS_CAUCHY = 0, 1, 2


class KhSpaOptions(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int32), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("min_relative_decrease", C.c_double), ("initial_trust_region_radius", C.c_double),
                ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("max_num_consecutive_invalid_steps", C.c_int32), ("use_nonmonotonic_steps", C.c_int32),
                ("max_consecutive_nonmonotonic_steps", C.c_int32), ("jacobi_scaling", C.c_int32),
                ("loss_function", C.c_int32), ("loss_scale", C.c_double)]


class KhSpaSummary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("successful_steps", C.c_int32), ("termination", C.c_int32),
                ("usable", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("linearize_ms", C.c_double), ("solve_ms", C.c_double), ("total_ms", C.c_double),
                ("nnz_factor", C.c_int64), ("factor_flops", C.c_int64), ("factorizations", C.c_int32),
                ("levels", C.c_int32), ("factor_gpu_ms", C.c_double), ("backward_gpu_ms", C.c_double),
                ("linearize_gpu_ms", C.c_double), ("symbolic_ms", C.c_double),
                ("worst_linear_residual", C.c_double), ("analysis", C.c_int32), ("analysis_pad", C.c_int32)]


class KhSpaCovSummary(C.Structure):
    _fields_ = [("n_free", C.c_int32), ("levels", C.c_int32), ("analysis", C.c_int32), ("pad", C.c_int32),
                ("linearize_ms", C.c_double), ("factor_ms", C.c_double), ("inverse_ms", C.c_double),
                ("gather_ms", C.c_double), ("total_ms", C.c_double), ("inverse_flops", C.c_int64)]


class KhSpaCovColumnsSummary(C.Structure):
    _fields_ = [("cov", KhSpaCovSummary), ("n_queries", C.c_int32), ("path_fronts", C.c_int32),
                ("forward_ms", C.c_double), ("backward_ms", C.c_double), ("total_ms", C.c_double), ("column_flops", C.c_int64)]


class KhSpaAudit(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("index", "id_a", "id_b", "verifiable")] + \
               [(k, C.c_double) for k in ("chi2", "redundancy", "min_pivot", "chi2_loo")]


# the records of kh_spa_audit_constraints as a structured array (same layout as KhSpaAudit)
AUDIT_DTYPE = np.dtype([(k, np.int32) for k in ("index", "id_a", "id_b", "verifiable")] +
                       [(k, np.float64) for k in ("chi2", "redundancy", "min_pivot", "chi2_loo")])


class KhSpaAuditSummary(C.Structure):
    _fields_ = [("cov", KhSpaCovSummary), ("n_constraints", C.c_int32), ("n_verifiable", C.c_int32),
                ("kernel_ms", C.c_double), ("total_ms", C.c_double)]


class KhRejectParams(C.Structure):
    _fields_ = [("chi2", C.c_double), ("min_redundancy", C.c_double), ("tie", C.c_double), ("min_id_gap", C.c_int32), ("max_rounds", C.c_int32)]


class KhRejectSummary(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("n_removed", C.c_int32), ("max_chi2_loo", C.c_double), ("solve_ms", C.c_double),
                ("audit_ms", C.c_double), ("total_ms", C.c_double)]


KH_SPA_MAX_COV_COLUMNS = 64


class KhMarginalizeSummary(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_marginalized", "n_plain", "n_rounds", "n_added", "n_fused", "max_degree")] + \
               [(k, C.c_double) for k in ("pack_ms", "kernel_ms", "apply_ms", "total_ms")]


KH_REMOVE_PLAIN, KH_REMOVE_MARGINALIZE = 0, 1


# every symbol include/karto_hip.h declares (tests check that the built library exports all of them)
SYMBOLS = [
    "kh_last_error", "kh_device_count", "kh_version", "kh_scan_points", "kh_match_params_default",
    "kh_matcher_create", "kh_matcher_destroy", "kh_matcher_set_params", "kh_matcher_match",
    "kh_matcher_match_batch", "kh_matcher_add_scans", "kh_matcher_correlate", "kh_matcher_correlate_batch",
    "kh_matcher_grid_info", "kh_matcher_read_grid", "kh_matcher_read_kernel", "kh_matcher_read_lookup",
    "kh_matcher_positional_covariance", "kh_matcher_angular_covariance",
    "kh_matcher_read_volume", "kh_matcher_read_search_probabilities", "kh_matcher_set_debug", "kh_matcher_stream", "kh_matcher_profile", "kh_matcher_score_loads", "kh_matcher_seq_stats", "kh_matcher_profile_side",
    "kh_matcher_group_create", "kh_matcher_group_destroy", "kh_matcher_group_set_params", "kh_matcher_group_size", "kh_matcher_group_member",
    "kh_matcher_group_device", "kh_matcher_group_match_batch", "kh_loop_closure_batch",
    "kh_spa_options_default", "kh_spa_create", "kh_spa_set_debug", "kh_spa_destroy", "kh_spa_set_options", "kh_spa_reset",
    "kh_spa_clear", "kh_spa_add_node", "kh_spa_add_constraint", "kh_spa_remove_node",
    "kh_spa_remove_constraint", "kh_spa_modify_node", "kh_spa_get_node", "kh_spa_num_nodes",
    "kh_spa_num_constraints", "kh_spa_compute", "kh_spa_iteration_log", "kh_spa_get_corrections", "kh_link_info", "kh_spa_set_sharding",
    "kh_spa_save", "kh_spa_load", "kh_spa_add_constraint_information", "kh_spa_get_node_at", "kh_spa_get_constraint", "kh_spa_get_nodes",
    "kh_graph_create", "kh_graph_destroy", "kh_graph_set", "kh_graph_set_positions", "kh_graph_find_loop_candidates",
    "kh_graph_last_kernel_ms", "kh_graph_find_near_chains", "kh_graph_closest_scan_to_pose", "kh_weighted_mean",
    "kh_occupancy_compute_dimensions", "kh_occupancy_create", "kh_occupancy_destroy", "kh_occupancy_clear",
    "kh_occupancy_add_scans", "kh_occupancy_update", "kh_occupancy_read", "kh_occupancy_info",
    "kh_decay_params_default", "kh_lifelong_scores", "kh_lifelong_scores_resident",
    "kh_spa_set_comm", "kh_comm_unique_id", "kh_comm_create", "kh_comm_destroy", "kh_comm_rank", "kh_comm_world", "kh_comm_device",
    "kh_comm_allreduce_sum_f64", "kh_comm_allgather_f64",
    "kh_device_malloc", "kh_device_free", "kh_device_upload", "kh_device_upload_on", "kh_device_download", "kh_selftest_lds_attr",
    "kh_graph_find_loop_candidates_from",
    "kh_mapper_params_default", "kh_mapper_create", "kh_mapper_create_on_devices", "kh_mapper_destroy", "kh_mapper_process", "kh_mapper_num_scans",
    "kh_mapper_num_edges", "kh_mapper_get_poses", "kh_mapper_get_scan", "kh_mapper_get_stats", "kh_mapper_solver",
    "kh_mapper_set_log", "kh_mapper_remove_node", "kh_mapper_get_adjacency", "kh_mapper_set_node_score", "kh_mapper_set_lifelong", "kh_mapper_num_alive", "kh_mapper_get_alive",
    "kh_graph_set_scan_limit", "kh_graph_find_near_linked", "kh_graph_append_scan", "kh_graph_add_edge", "kh_graph_set_position",
    "kh_graph_set_poses", "kh_graph_set_pose", "kh_graph_append_scan_with_pose", "kh_graph_find_near_by_scan", "kh_graph_find_near_by_vertices",
    "kh_graph_last_near_by_kernel_ms",
    "kh_mapper_process_localization", "kh_mapper_process_against_node", "kh_mapper_process_against_nodes_near_by",
    "kh_mapper_clear_localization_buffer", "kh_mapper_localization_buffer",
    "kh_mapper_save", "kh_mapper_load", "kh_session_info", "kh_session_last_load_ms", "kh_mapper_build_map", "kh_mapper_map_stats", "kh_occupancy_geometry",
    "kh_merge_create", "kh_merge_destroy", "kh_merge_add_mapper", "kh_merge_add_session", "kh_merge_remove_submap", "kh_merge_num_submaps",
    "kh_merge_submap_info", "kh_merge_set_transform", "kh_merge_get_transform", "kh_merge_move_submap", "kh_merge_get_location",
    "kh_merge_get_scan", "kh_merge_build_submap", "kh_merge_build", "kh_merge_stats",
    "kh_mapper_set_scan_pose", "kh_live_map_create", "kh_live_map_destroy", "kh_live_map_update", "kh_live_map_info", "kh_live_map_read",
    "kh_live_map_stats",
    "kh_occupancy_read_nav", "kh_map_feed_create", "kh_map_feed_destroy", "kh_map_feed_poll", "kh_map_feed_tiles", "kh_map_feed_read",
    "kh_map_feed_stats",
    "kh_graph_relocalize_candidates", "kh_graph_last_relocalize_kernel_ms", "kh_relocalize_params_default", "kh_mapper_relocalize", "kh_mapper_get_params",
    "kh_merge_fit", "kh_merge_fit_stats", "kh_merge_align_params_default", "kh_merge_align",
    "kh_spa_compute_covariances", "kh_spa_get_covariances", "kh_spa_get_joint_covariance", "kh_spa_covariance_device",
    "kh_mapper_get_covariances",
    "kh_spa_compute_covariance_columns", "kh_spa_get_covariance_column", "kh_spa_get_joint_covariance_any", "kh_spa_get_relative_covariances",
    "kh_mapper_get_relative_covariances",
    "kh_spa_marginalize_nodes", "kh_mapper_marginalize_nodes", "kh_mapper_set_removal_mode",
    "kh_spa_get_difference_covariances", "kh_mapper_get_difference_covariances", "kh_graph_find_loop_candidates_gated",
    "kh_loop_gate_params_default", "kh_mapper_set_loop_gate", "kh_mapper_get_loop_gate", "kh_mapper_get_loop_gate_stats",
    "kh_spa_audit_constraints", "kh_mapper_add_edge", "kh_mapper_remove_edge", "kh_mapper_correct_poses", "kh_mapper_audit",
    "kh_reject_params_default", "kh_mapper_reject_outliers",
    "kh_occupancy_view", "kh_occupancy_write_nav", "kh_live_map_view",
    "kh_matcher_add_map", "kh_matcher_match_map", "kh_matcher_match_map_batch", "kh_matcher_profile_map",
    "kh_map_seeds", "kh_map_fit", "kh_map_localizer_create", "kh_map_localizer_destroy", "kh_map_localizer_set_map",
    "kh_map_relocalize_params_default", "kh_map_localizer_relocalize", "kh_map_localizer_set_pose", "kh_map_localizer_get_pose",
    "kh_map_localizer_process", "kh_map_localizer_stats",
    "kh_map_changes_create", "kh_map_changes_destroy", "kh_map_changes_clear", "kh_map_changes_decay", "kh_map_changes_observe",
    "kh_map_changes_diff", "kh_map_changes_read", "kh_map_changes_view", "kh_map_changes_read_nav",
    "kh_map_raycast", "kh_map_align_params_default", "kh_map_align",
    "kh_map_merge_params_default", "kh_map_merge_create", "kh_map_merge_destroy", "kh_map_merge_stats_get", "kh_map_merge_view",
    "kh_map_merge_read", "kh_map_merge_read_nav",
    "kh_map_field_params_default", "kh_map_field_create", "kh_map_field_destroy", "kh_map_field_stats_get", "kh_map_field_read",
    "kh_inflation_params_default", "kh_inflation_table", "kh_map_field_costs", "kh_map_field_clearance", "kh_map_field_score",
    "kh_field_refine_params_default", "kh_map_field_refine",
    "kh_map_field_update", "kh_map_field_set_band_rows", "kh_map_field_read_rect", "kh_map_field_costs_rect",
    "kh_live_map_field_create", "kh_live_map_field_sync",
    "kh_map_regions_params_default", "kh_map_regions_create", "kh_map_regions_recompute", "kh_map_regions_destroy", "kh_map_regions_stats_get",
    "kh_map_regions_read", "kh_map_regions_get", "kh_map_regions_lookup",
    "kh_map_travel_params_default", "kh_map_travel_create", "kh_map_travel_recompute", "kh_map_travel_destroy", "kh_map_travel_solve",
    "kh_map_travel_stats_get", "kh_map_travel_read", "kh_map_travel_lookup", "kh_map_travel_paths", "kh_map_travel_set_rounds_per_check",
    "kh_map_visibility_params_default", "kh_map_visibility_create", "kh_map_visibility_destroy", "kh_map_visibility_set_map", "kh_map_visibility_clear",
    "kh_map_visibility_commit", "kh_map_visibility_gain", "kh_map_visibility_select", "kh_map_visibility_read_mask", "kh_map_visibility_stats_get",
    "kh_map_visibility_set_skip",
    "kh_map_footprint_create", "kh_map_footprint_recompute", "kh_map_footprint_destroy", "kh_map_footprint_stats_get", "kh_map_footprint_check",
    "kh_map_footprint_layer",
]


class KhScanBox(C.Structure):
    _fields_ = [("barycenter", C.c_double * 2), ("bbox_size", C.c_double * 2), ("unique_id", C.c_int32),
                ("n_edges", C.c_int32), ("score", C.c_double), ("n_points", C.c_int32),
                ("points_xy", C.POINTER(C.c_double))]


class KhDecayParams(C.Structure):
    _fields_ = [("iou_thresh", C.c_double), ("iou_match", C.c_double), ("removal_score", C.c_double),
                ("overlap_scale", C.c_double), ("constraint_scale", C.c_double), ("nearby_penalty", C.c_double),
                ("candidates_scale", C.c_double), ("scan_buffer_size", C.c_int32)]


class KhLaser(C.Structure):
    _fields_ = [("n_beams", C.c_int32), ("minimum_angle", C.c_double), ("angular_resolution", C.c_double),
                ("minimum_range", C.c_double), ("maximum_range", C.c_double), ("range_threshold", C.c_double),
                ("offset_x", C.c_double), ("offset_y", C.c_double), ("offset_heading", C.c_double)]


class KhMapperParams(C.Structure):
    _fields_ = [("use_scan_matching", C.c_int32), ("use_scan_barycenter", C.c_int32),
                ("minimum_time_interval", C.c_double), ("minimum_travel_distance", C.c_double),
                ("minimum_travel_heading", C.c_double), ("scan_buffer_size", C.c_int32),
                ("scan_buffer_maximum_scan_distance", C.c_double), ("link_match_minimum_response_fine", C.c_double),
                ("link_scan_maximum_distance", C.c_double), ("loop_search_maximum_distance", C.c_double),
                ("do_loop_closing", C.c_int32), ("loop_match_minimum_chain_size", C.c_int32),
                ("loop_match_maximum_variance_coarse", C.c_double), ("loop_match_minimum_response_coarse", C.c_double),
                ("loop_match_minimum_response_fine", C.c_double), ("correlation_search_space_dimension", C.c_double),
                ("correlation_search_space_resolution", C.c_double), ("correlation_search_space_smear_deviation", C.c_double),
                ("loop_search_space_dimension", C.c_double), ("loop_search_space_resolution", C.c_double),
                ("loop_search_space_smear_deviation", C.c_double), ("match", KhMatchParams)]


class KhMapperStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("scans_processed", "matches", "loop_candidates", "loop_closures", "speculation_discarded", "nodes_removed")] + \
               [(k, C.c_double) for k in ("process_ms", "match_ms", "solver_ms", "update_ms", "lifelong_ms")] + \
               [(k, C.c_int64) for k in ("fused_declined", "fused_declined_reason", "fused_matches", "fused_fine_passes",
                                           "decay_calls_resident", "decay_calls_packed", "marginalize_fallbacks")]


class KhLoopGateParams(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("refresh_scans", C.c_int32), ("chi2_position", C.c_double), ("chi2_jump", C.c_double),
                ("covariance_scale", C.c_double), ("max_reach", C.c_double)]


class KhLoopGateStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("column_passes", "ungated_searches", "jump_rejected")] + \
               [(k, C.c_double) for k in ("column_ms", "max_semi_axis")]


class KhSessionInfo(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("version", "file_bytes", "n_beams", "n_scan_slots", "n_alive", "n_edges", "n_running", "last_scan",
                                         "n_localization_buffer", "lifelong", "n_solver_nodes", "n_solver_constraints", "n_supernodes")]


class KhLiveMapInfo(C.Structure):
    _fields_ = [("anchor", C.c_double * 2), ("resolution", C.c_double), ("rebuild_fraction", C.c_double)] + \
               [(k, C.c_int32) for k in ("ox", "oy", "width", "height", "width_step", "reach")]


class KhLiveMapCounts(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("scans_added", "scans_removed", "scans_moved", "beams_traced", "beams_skipped", "cells_updated",
                                         "relayouts", "rebuilds")] + [("trace_ms", C.c_double)]


class KhLiveMapStats(C.Structure):
    _fields_ = [("last", KhLiveMapCounts), ("total", KhLiveMapCounts)] + [(k, C.c_int64) for k in ("updates", "scans_in_map", "log_bytes")]


KH_MAP_TILE = 16


class KhMapFeedDelta(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_tiles", "tiles_scanned", "bytes_downloaded")] + \
               [(k, C.c_int32) for k in ("ox", "oy", "width", "height", "x", "y", "w", "h")] + [("kernel_ms", C.c_double)]


class KhMapFeedStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("polls", "n_tiles", "tiles_scanned", "bytes_downloaded")] + [("kernel_ms", C.c_double)]


class KhRelocalizeParams(C.Structure):
    _fields_ = [("seed_spacing", C.c_double), ("n_headings", C.c_int32), ("max_base", C.c_int32), ("top_k", C.c_int32), ("pad", C.c_int32),
                ("center_xy", C.c_double * 2), ("radius", C.c_double)]


class KhRelocalizeHyp(C.Structure):
    _fields_ = [("index", C.c_int32), ("seed_scan", C.c_int32), ("heading", C.c_double),
                ("coarse_mean", C.c_double * 3), ("coarse_cov", C.c_double * 9), ("coarse_response", C.c_double),
                ("fine_mean", C.c_double * 3), ("fine_cov", C.c_double * 9), ("fine_response", C.c_double),
                ("robot_pose", C.c_double * 3)]


class KhRelocalizeSummary(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_seeds", "n_headings", "n_hypotheses", "n_passed", "n_accepted", "n_returned")] + \
               [(k, C.c_double) for k in ("kernel_ms", "candidates_ms", "scans_ms", "batch_ms", "total_ms")]


class KhMergeFit(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("pass_unknown", "pass_occupied", "pass_free", "hits_unknown", "hits_occupied", "hits_free",
                                          "agree", "conflict", "known")] + [("score", C.c_double)]


class KhMapRelocalizeParams(C.Structure):
    _fields_ = [("seed_spacing", C.c_double), ("n_headings", C.c_int32), ("top_k", C.c_int32), ("center_xy", C.c_double * 2),
                ("radius", C.c_double), ("minimum_response_coarse", C.c_double), ("maximum_variance_coarse", C.c_double),
                ("minimum_response_fine", C.c_double), ("min_fit_score", C.c_double), ("merge_distance", C.c_double),
                ("merge_heading", C.c_double)]


class KhMapHyp(C.Structure):
    _fields_ = [("index", C.c_int32), ("seed_cell", C.c_int32 * 2), ("pad", C.c_int32), ("heading", C.c_double),
                ("coarse_mean", C.c_double * 3), ("coarse_cov", C.c_double * 9), ("coarse_response", C.c_double),
                ("fine_mean", C.c_double * 3), ("fine_cov", C.c_double * 9), ("fine_response", C.c_double),
                ("robot_pose", C.c_double * 3), ("fit", KhMergeFit)]


class KhMapRelocalizeSummary(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_seeds", "n_headings", "n_hypotheses", "n_passed", "n_accepted", "n_rejected_fit", "n_duplicates",
                                         "n_returned")] + \
               [(k, C.c_double) for k in ("seed_kernel_ms", "fit_kernel_ms", "coarse_ms", "fine_ms", "total_ms")]


class KhMapTrack(C.Structure):
    _fields_ = [("predicted_pose", C.c_double * 3), ("robot_pose", C.c_double * 3), ("sensor_pose", C.c_double * 3),
                ("covariance", C.c_double * 9), ("response", C.c_double), ("fit", KhMergeFit)]


class KhMapLocalizerStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("relocalizations", "hypotheses", "steps", "poses_fitted")] + \
               [(k, C.c_double) for k in ("relocalize_ms", "process_ms", "match_ms", "seed_kernel_ms", "fit_kernel_ms")]


class KhMapChangesSummary(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_unobserved", "n_confirmed", "n_appeared", "n_vanished", "n_discovered_occupied", "n_discovered_free",
                                           "n_changed", "n_listed", "scans_observed", "beams_observed")] + \
               [(k, C.c_double) for k in ("observe_kernel_ms", "diff_kernel_ms", "list_kernel_ms", "download_ms")]


KH_BEAM_DROPPED, KH_BEAM_EXPLAINED, KH_BEAM_NOVEL, KH_BEAM_UNKNOWN, KH_BEAM_THROUGH, KH_BEAM_CLEAR = range(6)
KH_CELL_UNOBSERVED, KH_CELL_CONFIRMED, KH_CELL_APPEARED, KH_CELL_VANISHED, KH_CELL_DISCOVERED_OCCUPIED, KH_CELL_DISCOVERED_FREE = range(6)


KH_RAY_FREE, KH_RAY_HIT, KH_RAY_UNKNOWN = range(3)


class KhRay(C.Structure):
    _fields_ = [("range", C.c_double), ("cell", C.c_int32 * 2), ("steps", C.c_int32), ("code", C.c_int32)]


RAY_DTYPE = np.dtype([("range", np.float64), ("cell", np.int32, (2,)), ("steps", np.int32), ("code", np.int32)])


class KhMapAlignParams(C.Structure):
    _fields_ = [("probe_spacing", C.c_double), ("n_probes", C.c_int32), ("top_k", C.c_int32), ("max_unknown", C.c_int32), ("pad", C.c_int32),
                ("min_known", C.c_uint64), ("initial", C.c_double * 3), ("relocalize", KhMapRelocalizeParams)]


class KhMapAlignCand(C.Structure):
    _fields_ = [("correction", C.c_double * 3), ("probe_seed", C.c_int32), ("hypothesis", C.c_int32), ("fine_response", C.c_double),
                ("index", C.c_int32), ("enough", C.c_int32), ("fit", KhMergeFit)]


KH_MERGED_NEITHER, KH_MERGED_TARGET_ONLY, KH_MERGED_MOVING_ONLY, KH_MERGED_AGREE, KH_MERGED_MOVING_OCCUPIED, KH_MERGED_MOVING_FREE = range(6)
KH_MERGE_CONFLICT_TARGET, KH_MERGE_CONFLICT_MOVING, KH_MERGE_CONFLICT_OCCUPIED, KH_MERGE_CONFLICT_UNKNOWN = range(4)


class KhMapMergeParams(C.Structure):
    _fields_ = [("correction", C.c_double * 3), ("footprint", C.c_int32), ("conflict", C.c_int32), ("grow", C.c_int32), ("pad", C.c_int32)]


class KhMapMergeStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("ox", "oy", "width", "height", "width_step", "footprint")] + [("known_box", C.c_int32 * 4)] + \
               [(k, C.c_uint64) for k in ("target_only", "moving_only", "agree_free", "agree_occupied", "conflict_moving_occupied",
                                           "conflict_moving_free", "overlap")] + \
               [("agreement", C.c_double), ("times_ms", C.c_double * 3)]


KH_FIELD_FAR = 0xFFFFFFFF
KH_FIELD_OBSTACLE_OCCUPIED, KH_FIELD_OBSTACLE_NOT_FREE = 0, 1
KH_CLEAR_OK, KH_CLEAR_FAR, KH_CLEAR_OUTSIDE = range(3)
KH_REFINE_CONVERGED, KH_REFINE_MAX_ROUNDS, KH_REFINE_LEFT_LATTICE = range(3)


class KhMapFieldParams(C.Structure):
    _fields_ = [("max_distance", C.c_double), ("obstacles", C.c_int32), ("pad", C.c_int32)]


class KhMapFieldStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("ox", "oy", "width", "height", "radius_cells")] + [("max_d2", C.c_uint32)] + \
               [("n_obstacles", C.c_uint64), ("n_far", C.c_uint64), ("times_ms", C.c_double * 3)]


class KhInflationParams(C.Structure):
    _fields_ = [("inscribed_radius", C.c_double), ("inflation_radius", C.c_double), ("cost_scaling_factor", C.c_double),
                ("track_unknown", C.c_int32), ("inflate_unknown", C.c_int32)]


class KhFieldScore(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_kept", "n_hit", "n_inside", "n_near")] + [("sum_d2", C.c_uint64), ("cost", C.c_uint64), ("score", C.c_double)]


class KhFieldRefineParams(C.Structure):
    _fields_ = [("step_xy", C.c_double), ("step_heading", C.c_double)] + [(k, C.c_int32) for k in ("n_halvings", "max_rounds", "truncate_cells", "pad")]


class KhFieldRefined(C.Structure):
    _fields_ = [("pose", C.c_double * 3), ("cost_start", C.c_uint64), ("cost", C.c_uint64)] + \
               [(k, C.c_int32) for k in ("n_hit", "rounds", "halvings", "status")]


class KhFieldUpdate(C.Structure):
    _fields_ = [("cells_box", C.c_int32 * 4), ("values_box", C.c_int32 * 4), ("rebuilt", C.c_int32), ("relayout", C.c_int32),
                ("cells_compared", C.c_int64), ("cells_recomputed", C.c_int64), ("times_ms", C.c_double * 4)]


KH_REGION_NONE, KH_REGION_DROPPED = 0xFFFFFFFF, 0xFFFFFFFE
KH_REGIONS, KH_FRONTIERS = 0, 1
KH_REGION_AT_OK, KH_REGION_AT_NONE, KH_REGION_AT_DROPPED, KH_REGION_OUTSIDE = range(4)


class KhMapRegionsParams(C.Structure):
    _fields_ = [("min_clearance", C.c_double)] + \
               [(k, C.c_int32) for k in ("connectivity", "min_region_cells", "max_regions", "min_frontier_cells", "max_frontiers", "pad")]


class KhRegion(C.Structure):
    _fields_ = [("root", C.c_uint32), ("n_cells", C.c_uint32), ("box", C.c_int32 * 4), ("sum_i", C.c_uint64), ("sum_j", C.c_uint64)] + \
               [(k, C.c_uint32) for k in ("max_d2", "n_other", "link", "anchor_cell")] + [("centroid", C.c_double * 2), ("anchor_xy", C.c_double * 2)]


class KhMapRegionsStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("ox", "oy", "width", "height", "clearance_cells", "connectivity")] + \
               [("n_traversable", C.c_uint64), ("n_frontier_cells", C.c_uint64), ("n_total", C.c_uint32 * 2), ("n_kept", C.c_uint32 * 2),
                ("truncated", C.c_int32 * 2), ("times_ms", C.c_double * 7)]


KH_TRAVEL_FAR = 0xFFFFFFFF
KH_TRAVEL_GOAL_OK, KH_TRAVEL_GOAL_BLOCKED, KH_TRAVEL_GOAL_OUTSIDE = range(3)
KH_TRAVEL_AT_OK, KH_TRAVEL_AT_UNREACHED, KH_TRAVEL_AT_OUTSIDE = range(3)
KH_TRAVEL_PATH_OK, KH_TRAVEL_PATH_TRUNCATED, KH_TRAVEL_PATH_UNREACHED, KH_TRAVEL_PATH_OUTSIDE = range(4)


class KhMapTravelParams(C.Structure):
    _fields_ = [("min_clearance", C.c_double), ("inflation", KhInflationParams)] + \
               [(k, C.c_int32) for k in ("connectivity", "cut_corners", "neutral_cost", "cost_weight", "goal_snap_cells", "pad")]


class KhMapTravelStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("ox", "oy", "width", "height", "clearance_cells", "inflation_cells", "connectivity", "pad")] + \
               [("n_traversable", C.c_uint64), ("n_reached", C.c_uint64)] + \
               [(k, C.c_uint32) for k in ("max_value", "rounds", "launches", "pad2")] + [("tile_runs", C.c_uint64), ("times_ms", C.c_double * 4)]


class KhTravelPath(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_cells", C.c_int32), ("cost", C.c_uint32), ("start_cell", C.c_uint32)]


class KhVisibilityParams(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("max_unknown", "w_unknown", "w_free", "w_occupied")]


class KhVisibility(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("seen_free", "seen_occupied", "seen_unknown", "new_free", "new_occupied", "new_unknown", "gain", "beams_free",
                                          "beams_hit", "beams_unknown")]


class KhMapVisibilityStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("ox", "oy", "width", "height", "reach", "bitmap_bytes", "n_poses", "pad")] + \
               [("rounds", C.c_uint32), ("launches", C.c_uint32), ("kernel_ms", C.c_double), ("call_ms", C.c_double)]


KH_FOOTPRINT_FREE, KH_FOOTPRINT_UNKNOWN, KH_FOOTPRINT_OUTSIDE, KH_FOOTPRINT_COLLISION, KH_FOOTPRINT_LATTICE = range(5)
KH_FOOTPRINT_LAYER_REACH = 64


class KhFootprint(C.Structure):
    _fields_ = [("status", C.c_int32)] + [(k, C.c_uint32) for k in ("n_cells", "n_free", "n_occupied", "n_unknown", "n_outside", "min_d2", "pad")]


class KhFootprintLayer(C.Structure):
    _fields_ = [("n_fit", C.c_uint64 * 32), ("n_any", C.c_uint64), ("n_all", C.c_uint64)]


class KhMapFootprintStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("ox", "oy", "width", "height", "n_vertices", "reach", "layer_rows", "pad")] + [("times_ms", C.c_double * 3)]


class KhMergeAlignParams(C.Structure):
    _fields_ = [("n_probes", C.c_int32), ("top_k", C.c_int32), ("min_known", C.c_uint64), ("min_pass_through", C.c_uint32), ("pad", C.c_uint32),
                ("occupancy_threshold", C.c_double), ("relocalize", KhRelocalizeParams)]


class KhMergeAlignCand(C.Structure):
    _fields_ = [("correction", C.c_double * 3), ("probe_scan", C.c_int32), ("hypothesis", C.c_int32), ("fine_response", C.c_double),
                ("index", C.c_int32), ("enough", C.c_int32), ("fit", KhMergeFit)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)

_lib = None


class KartoHipError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = ""
        try:
            msg = lib().kh_last_error().decode()
        except Exception:
            pass
        super().__init__(f"{where}: status {code} {msg}")


def lib():
    """Loads libkartohip.so; raises if it has not been built (run `python -m slam_toolbox_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m slam_toolbox_amd.build` "
                          "(the HIP extension is the product; there is no fallback)")
    L = C.CDLL(LIB_PATH)
    vp, i32, dbl = C.c_void_p, C.c_int32, C.c_double
    L.kh_last_error.restype = C.c_char_p
    L.kh_version.restype = C.c_char_p
    L.kh_device_count.restype = C.c_int
    L.kh_scan_points.argtypes = [dptr, i32, dptr, dbl, dbl, dptr]
    L.kh_match_params_default.argtypes = [C.POINTER(KhMatchParams)]
    L.kh_matcher_create.argtypes = [dbl, dbl, dbl, dbl, i32, i32, C.POINTER(vp)]
    L.kh_matcher_destroy.argtypes = [vp]
    L.kh_matcher_destroy.restype = None
    L.kh_matcher_set_params.argtypes = [vp, C.POINTER(KhMatchParams)]
    L.kh_matcher_match.argtypes = [vp, C.POINTER(KhScan), C.POINTER(KhScan), i32, i32, i32, dptr, dptr, C.POINTER(dbl)]
    L.kh_matcher_match_batch.argtypes = [vp, i32, C.POINTER(KhScan), C.POINTER(KhScan), iptr, i32, i32, dptr, dptr, dptr, iptr]
    if hasattr(L, "kh_matcher_group_create"):
        L.kh_matcher_group_create.argtypes = [dbl, dbl, dbl, dbl, iptr, i32, i32, C.POINTER(vp)]
        L.kh_matcher_group_destroy.argtypes = [vp]
        L.kh_matcher_group_destroy.restype = None
        L.kh_matcher_group_set_params.argtypes = [vp, C.POINTER(KhMatchParams)]
        L.kh_matcher_group_size.argtypes = [vp]
        L.kh_matcher_group_member.argtypes = [vp, i32]
        L.kh_matcher_group_member.restype = vp
        L.kh_matcher_group_device.argtypes = [vp, i32]
        L.kh_matcher_group_match_batch.argtypes = [vp, i32, C.POINTER(KhScan), C.POINTER(KhScan), iptr, vp, i32, i32, dptr, dptr, dptr, iptr]
        L.kh_loop_closure_batch.argtypes = [vp, vp, i32, C.POINTER(KhScan), C.POINTER(KhScan), iptr, dbl, dbl, dbl, dbl, i32,
                                            dptr, dptr, dptr, iptr, dptr, dptr, dptr]
    L.kh_matcher_add_scans.argtypes = [vp, i32, C.POINTER(KhScan), C.POINTER(KhScan), i32]
    L.kh_matcher_correlate.argtypes = [vp, i32, C.POINTER(KhScan), dptr, dptr, dptr, dbl, dbl, i32, i32, dptr, dptr, C.POINTER(dbl)]
    L.kh_matcher_correlate_batch.argtypes = [vp, i32, C.POINTER(KhScan), dptr, dptr, dptr, dbl, dbl, i32, i32, dptr, dptr, dptr, iptr]
    L.kh_matcher_positional_covariance.argtypes = [vp, i32, dptr, dbl, dptr, dptr, dptr, dbl, dptr]
    L.kh_matcher_angular_covariance.argtypes = [vp, i32, C.POINTER(KhScan), dptr, dbl, dptr, dbl, dbl, dptr]
    L.kh_matcher_grid_info.argtypes = [vp, i32, C.POINTER(KhGridInfo)]
    L.kh_matcher_read_grid.argtypes = [vp, i32, bptr]
    L.kh_matcher_read_kernel.argtypes = [vp, bptr]
    L.kh_matcher_read_lookup.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), vp]
    L.kh_matcher_read_volume.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), vp, vp]
    if hasattr(L, "kh_matcher_read_search_probabilities"):      # (KH_LIBRARY may name a build from before the call existed: A/B runs)
        L.kh_matcher_read_search_probabilities.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), vp]
    L.kh_matcher_set_debug.argtypes = [vp, i32]
    L.kh_matcher_stream.argtypes = [vp]
    L.kh_matcher_stream.restype = vp
    L.kh_matcher_profile.argtypes = [vp, i32, C.POINTER(dbl), C.POINTER(C.c_int64), C.POINTER(dbl), C.POINTER(C.c_int64)]
    L.kh_matcher_score_loads.argtypes = [vp, C.POINTER(C.c_int64), i32]
    L.kh_matcher_seq_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    L.kh_matcher_profile_side.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(L, "kh_matcher_add_map"):      # (KH_LIBRARY may name a build from before the map entry points existed)
        L.kh_occupancy_view.argtypes = [vp, C.POINTER(KhMapView)]
        L.kh_occupancy_write_nav.argtypes = [vp, vp]
        L.kh_live_map_view.argtypes = [vp, C.POINTER(KhMapView)]
        L.kh_matcher_add_map.argtypes = [vp, i32, C.POINTER(KhScan), C.POINTER(KhMapView)]
        L.kh_matcher_match_map.argtypes = [vp, C.POINTER(KhScan), C.POINTER(KhMapView), i32, i32, dptr, dptr, C.POINTER(dbl)]
        L.kh_matcher_match_map_batch.argtypes = [vp, i32, C.POINTER(KhScan), C.POINTER(KhMapView), i32, i32, dptr, dptr, dptr, iptr]
        L.kh_matcher_profile_map.argtypes = [vp, C.POINTER(dbl), C.POINTER(C.c_int64)]
    if hasattr(L, "kh_map_localizer_create"):      # (KH_LIBRARY may name a build from before the map localizer existed)
        L.kh_map_seeds.argtypes = [C.POINTER(KhMapView), dbl, vp, dbl, vp, vp, i32, C.POINTER(i32)]
        L.kh_map_fit.argtypes = [C.POINTER(KhMapView), C.POINTER(KhLaser), vp, i32, vp, C.POINTER(KhMergeFit)]
        L.kh_map_localizer_create.argtypes = [C.POINTER(KhMapperParams), C.POINTER(KhLaser), i32, i32, C.POINTER(vp)]
        L.kh_map_localizer_destroy.argtypes = [vp]
        L.kh_map_localizer_destroy.restype = None
        L.kh_map_localizer_set_map.argtypes = [vp, C.POINTER(KhMapView)]
        L.kh_map_relocalize_params_default.argtypes = [C.POINTER(KhMapperParams), C.POINTER(KhMapRelocalizeParams)]
        L.kh_map_relocalize_params_default.restype = None
        L.kh_map_localizer_relocalize.argtypes = [vp, vp, C.POINTER(KhMapRelocalizeParams), C.POINTER(KhMapHyp), i32,
                                                  C.POINTER(KhMapRelocalizeSummary)]
        L.kh_map_localizer_set_pose.argtypes = [vp, vp, vp]
        L.kh_map_localizer_get_pose.argtypes = [vp, vp, vp]
        L.kh_map_localizer_process.argtypes = [vp, vp, vp, C.POINTER(KhMapTrack)]
        L.kh_map_localizer_stats.argtypes = [vp, C.POINTER(KhMapLocalizerStats)]
    if hasattr(L, "kh_map_changes_create"):      # (KH_LIBRARY may name a build from before the change layer existed)
        L.kh_map_changes_create.argtypes = [C.POINTER(KhMapView), C.POINTER(vp)]
        L.kh_map_changes_destroy.argtypes = [vp]
        L.kh_map_changes_destroy.restype = None
        L.kh_map_changes_clear.argtypes = [vp]
        L.kh_map_changes_decay.argtypes = [vp, i32]
        L.kh_map_changes_observe.argtypes = [vp, C.POINTER(KhLaser), i32, vp, vp, i32, vp]
        L.kh_map_changes_diff.argtypes = [vp, C.c_uint32, dbl, vp, i32, C.POINTER(KhMapChangesSummary)]
        L.kh_map_changes_read.argtypes = [vp, vp, vp, vp, vp]
        L.kh_map_changes_view.argtypes = [vp, C.POINTER(KhMapView)]
        L.kh_map_changes_read_nav.argtypes = [vp, vp]
    if hasattr(L, "kh_map_raycast"):      # (KH_LIBRARY may name a build from before the ray cast existed)
        L.kh_map_raycast.argtypes = [C.POINTER(KhMapView), C.POINTER(KhLaser), i32, vp, i32, dbl, vp, C.POINTER(dbl)]
        L.kh_map_align_params_default.argtypes = [vp, C.POINTER(KhMapAlignParams)]
        L.kh_map_align_params_default.restype = None
        L.kh_map_align.argtypes = [vp, C.POINTER(KhMapView), C.POINTER(KhMapAlignParams), C.POINTER(KhMapAlignCand), i32, C.POINTER(i32), vp]
    if hasattr(L, "kh_map_merge_create"):      # (KH_LIBRARY may name a build from before the map merge existed)
        L.kh_map_merge_params_default.argtypes = [C.POINTER(KhMapMergeParams)]
        L.kh_map_merge_params_default.restype = None
        L.kh_map_merge_create.argtypes = [C.POINTER(KhMapView), C.POINTER(KhMapView), C.POINTER(KhMapMergeParams), C.POINTER(vp)]
        L.kh_map_merge_destroy.argtypes = [vp]
        L.kh_map_merge_destroy.restype = None
        L.kh_map_merge_stats_get.argtypes = [vp, C.POINTER(KhMapMergeStats)]
        L.kh_map_merge_view.argtypes = [vp, C.POINTER(KhMapView)]
        L.kh_map_merge_read.argtypes = [vp, vp, vp]
        L.kh_map_merge_read_nav.argtypes = [vp, vp]
    if hasattr(L, "kh_map_field_create"):      # (KH_LIBRARY may name a build from before the distance field existed)
        L.kh_map_field_params_default.argtypes = [C.POINTER(KhMapFieldParams)]
        L.kh_map_field_params_default.restype = None
        L.kh_map_field_create.argtypes = [C.POINTER(KhMapView), C.POINTER(KhMapFieldParams), C.POINTER(vp)]
        L.kh_map_field_destroy.argtypes = [vp]
        L.kh_map_field_destroy.restype = None
        L.kh_map_field_stats_get.argtypes = [vp, C.POINTER(KhMapFieldStats)]
        L.kh_map_field_read.argtypes = [vp, vp, vp]
        L.kh_inflation_params_default.argtypes = [C.POINTER(KhInflationParams)]
        L.kh_inflation_params_default.restype = None
        L.kh_inflation_table.argtypes = [C.POINTER(KhInflationParams), dbl, vp, i32, C.POINTER(i32)]
        L.kh_map_field_costs.argtypes = [vp, C.POINTER(KhInflationParams), vp]
        L.kh_map_field_clearance.argtypes = [vp, i32, vp, vp, vp, vp]
        L.kh_map_field_score.argtypes = [vp, C.POINTER(KhLaser), vp, i32, vp, i32, C.POINTER(KhFieldScore)]
        L.kh_field_refine_params_default.argtypes = [C.POINTER(KhFieldRefineParams), dbl]
        L.kh_field_refine_params_default.restype = None
        L.kh_map_field_refine.argtypes = [vp, C.POINTER(KhLaser), vp, i32, vp, C.POINTER(KhFieldRefineParams), C.POINTER(KhFieldRefined), vp]
    if hasattr(L, "kh_map_field_update"):      # (KH_LIBRARY may name a build from before a field could follow its map)
        L.kh_map_field_update.argtypes = [vp, C.POINTER(KhMapView), C.POINTER(i32 * 4), C.POINTER(KhFieldUpdate)]
        L.kh_map_field_set_band_rows.argtypes = [vp, i32]
        L.kh_map_field_read_rect.argtypes = [vp, i32, i32, i32, i32, vp]
        L.kh_map_field_costs_rect.argtypes = [vp, C.POINTER(KhInflationParams), i32, i32, i32, i32, vp]
        L.kh_live_map_field_create.argtypes = [vp, C.POINTER(KhMapFieldParams), C.POINTER(vp)]
        L.kh_live_map_field_sync.argtypes = [vp, C.POINTER(KhFieldUpdate)]
    if hasattr(L, "kh_map_regions_create"):    # (KH_LIBRARY may name a build from before the region analysis existed)
        L.kh_map_regions_params_default.argtypes = [C.POINTER(KhMapRegionsParams)]
        L.kh_map_regions_params_default.restype = None
        L.kh_map_regions_create.argtypes = [vp, C.POINTER(KhMapRegionsParams), C.POINTER(vp)]
        L.kh_map_regions_recompute.argtypes = [vp, vp]
        L.kh_map_regions_destroy.argtypes = [vp]
        L.kh_map_regions_destroy.restype = None
        L.kh_map_regions_stats_get.argtypes = [vp, C.POINTER(KhMapRegionsStats)]
        L.kh_map_regions_read.argtypes = [vp, i32, vp]
        L.kh_map_regions_get.argtypes = [vp, i32, C.POINTER(KhRegion), i32, C.POINTER(i32)]
        L.kh_map_regions_lookup.argtypes = [vp, i32, vp, vp, vp]
    if hasattr(L, "kh_map_travel_create"):     # (KH_LIBRARY may name a build from before the travel costs existed)
        L.kh_map_travel_params_default.argtypes = [C.POINTER(KhMapTravelParams)]
        L.kh_map_travel_params_default.restype = None
        L.kh_map_travel_create.argtypes = [vp, C.POINTER(KhMapTravelParams), C.POINTER(vp)]
        L.kh_map_travel_recompute.argtypes = [vp, vp]
        L.kh_map_travel_destroy.argtypes = [vp]
        L.kh_map_travel_destroy.restype = None
        L.kh_map_travel_solve.argtypes = [vp, i32, vp, vp]
        L.kh_map_travel_stats_get.argtypes = [vp, C.POINTER(KhMapTravelStats)]
        L.kh_map_travel_read.argtypes = [vp, vp, vp]
        L.kh_map_travel_lookup.argtypes = [vp, i32, vp, i32, vp, vp, vp]
        L.kh_map_travel_paths.argtypes = [vp, i32, vp, i32, i32, C.POINTER(KhTravelPath), vp]
        L.kh_map_travel_set_rounds_per_check.argtypes = [vp, i32]
    if hasattr(L, "kh_map_visibility_create"):     # (KH_LIBRARY may name a build from before the visibility analysis existed)
        L.kh_map_visibility_params_default.argtypes = [C.POINTER(KhVisibilityParams)]
        L.kh_map_visibility_params_default.restype = None
        L.kh_map_visibility_create.argtypes = [C.POINTER(KhMapView), C.POINTER(KhLaser), C.POINTER(KhVisibilityParams), C.POINTER(vp)]
        L.kh_map_visibility_destroy.argtypes = [vp]
        L.kh_map_visibility_destroy.restype = None
        L.kh_map_visibility_set_map.argtypes = [vp, C.POINTER(KhMapView)]
        L.kh_map_visibility_clear.argtypes = [vp]
        L.kh_map_visibility_commit.argtypes = [vp, i32, vp]
        L.kh_map_visibility_gain.argtypes = [vp, i32, vp, vp, C.POINTER(dbl)]
        L.kh_map_visibility_select.argtypes = [vp, i32, vp, i32, C.c_uint32, vp, vp, C.POINTER(i32)]
        L.kh_map_visibility_read_mask.argtypes = [vp, vp]
        L.kh_map_visibility_stats_get.argtypes = [vp, C.POINTER(KhMapVisibilityStats)]
        L.kh_map_visibility_set_skip.argtypes = [vp, i32]
    if hasattr(L, "kh_map_footprint_create"):     # (KH_LIBRARY may name a build from before the footprint analysis existed)
        L.kh_map_footprint_create.argtypes = [vp, i32, vp, C.POINTER(vp)]
        L.kh_map_footprint_recompute.argtypes = [vp, vp]
        L.kh_map_footprint_destroy.argtypes = [vp]
        L.kh_map_footprint_destroy.restype = None
        L.kh_map_footprint_stats_get.argtypes = [vp, C.POINTER(KhMapFootprintStats)]
        L.kh_map_footprint_check.argtypes = [vp, i32, vp, vp]
        L.kh_map_footprint_layer.argtypes = [vp, i32, i32, vp, C.POINTER(KhFootprintLayer)]
    if hasattr(L, "kh_spa_create"):
        L.kh_spa_options_default.argtypes = [C.POINTER(KhSpaOptions)]
        L.kh_spa_create.argtypes = [i32, C.POINTER(vp)]
        L.kh_spa_destroy.argtypes = [vp]
        L.kh_spa_destroy.restype = None
        L.kh_spa_set_debug.argtypes = [vp, i32]
        L.kh_spa_set_options.argtypes = [vp, C.POINTER(KhSpaOptions)]
        L.kh_spa_reset.argtypes = [vp]
        L.kh_spa_clear.argtypes = [vp]
        L.kh_spa_add_node.argtypes = [vp, i32, dptr]
        L.kh_spa_add_constraint.argtypes = [vp, i32, i32, dptr, dptr]
        L.kh_spa_remove_node.argtypes = [vp, i32]
        L.kh_spa_remove_constraint.argtypes = [vp, i32, i32]
        L.kh_spa_modify_node.argtypes = [vp, i32, dptr]
        L.kh_spa_get_node.argtypes = [vp, i32, dptr]
        L.kh_spa_num_nodes.argtypes = [vp]
        L.kh_spa_num_constraints.argtypes = [vp]
        L.kh_spa_compute.argtypes = [vp, C.POINTER(KhSpaSummary)]
        L.kh_spa_iteration_log.argtypes = [vp, C.c_int32, vp, C.POINTER(C.c_int32)]
        L.kh_spa_get_corrections.argtypes = [vp, C.POINTER(i32), vp, vp]
        L.kh_link_info.argtypes = [dptr, dptr, dptr, dptr, dptr]
        L.kh_spa_set_sharding.argtypes = [vp, i32, i32, ALLREDUCE_FN, vp]
        L.kh_spa_save.argtypes = [vp, C.c_char_p, i32]
        L.kh_spa_load.argtypes = [vp, C.c_char_p]
        L.kh_spa_add_constraint_information.argtypes = [vp, i32, i32, dptr, dptr]
        L.kh_spa_get_node_at.argtypes = [vp, i32, C.POINTER(i32), dptr]
        L.kh_spa_get_nodes.argtypes = [vp, vp, vp]
        L.kh_spa_get_constraint.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), dptr, dptr]
        L.kh_spa_compute_covariances.argtypes = [vp, C.POINTER(KhSpaCovSummary)]
        L.kh_spa_get_covariances.argtypes = [vp, i32, vp, vp]
        L.kh_spa_get_joint_covariance.argtypes = [vp, i32, i32, vp]
        L.kh_spa_covariance_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64)]
    if hasattr(L, "kh_spa_compute_covariance_columns"):
        L.kh_spa_compute_covariance_columns.argtypes = [vp, i32, vp, C.POINTER(KhSpaCovColumnsSummary)]
        L.kh_spa_get_covariance_column.argtypes = [vp, i32, i32, vp, vp]
        L.kh_spa_get_joint_covariance_any.argtypes = [vp, i32, i32, vp]
        L.kh_spa_get_relative_covariances.argtypes = [vp, i32, i32, vp, vp]
    if hasattr(L, "kh_graph_find_loop_candidates_gated"):
        L.kh_spa_get_difference_covariances.argtypes = [vp, i32, i32, vp, vp]
        L.kh_mapper_get_difference_covariances.argtypes = [vp, i32, i32, vp, vp, C.POINTER(KhSpaCovColumnsSummary)]
        L.kh_graph_find_loop_candidates_gated.argtypes = [vp, i32, vp, vp, dbl, i32, dbl, vp, vp, vp, i32, C.POINTER(i32)]
        L.kh_loop_gate_params_default.argtypes = [C.POINTER(KhMapperParams), C.POINTER(KhLoopGateParams)]
        L.kh_loop_gate_params_default.restype = None
        L.kh_mapper_set_loop_gate.argtypes = [vp, C.POINTER(KhLoopGateParams)]
        L.kh_mapper_get_loop_gate.argtypes = [vp, C.POINTER(KhLoopGateParams)]
        L.kh_mapper_get_loop_gate_stats.argtypes = [vp, C.POINTER(KhLoopGateStats)]
    if hasattr(L, "kh_spa_audit_constraints"):
        L.kh_spa_audit_constraints.argtypes = [vp, dbl, vp, C.POINTER(KhSpaAuditSummary)]
        L.kh_mapper_add_edge.argtypes = [vp, i32, i32, vp, vp, i32]
        L.kh_mapper_remove_edge.argtypes = [vp, i32, i32]
        L.kh_mapper_correct_poses.argtypes = [vp]
        L.kh_mapper_audit.argtypes = [vp, dbl, vp, i32, C.POINTER(i32), C.POINTER(KhSpaAuditSummary)]
        L.kh_reject_params_default.argtypes = [C.POINTER(KhRejectParams)]
        L.kh_reject_params_default.restype = None
        L.kh_mapper_reject_outliers.argtypes = [vp, C.POINTER(KhRejectParams), vp, i32, C.POINTER(KhRejectSummary)]
    if hasattr(L, "kh_spa_marginalize_nodes"):
        L.kh_spa_marginalize_nodes.argtypes = [vp, i32, vp, C.POINTER(KhMarginalizeSummary)]
        L.kh_mapper_marginalize_nodes.argtypes = [vp, i32, vp]
        L.kh_mapper_set_removal_mode.argtypes = [vp, i32]
    if hasattr(L, "kh_comm_create"):
        L.kh_comm_unique_id.argtypes = [bptr]
        L.kh_comm_create.argtypes = [i32, i32, i32, bptr, C.POINTER(vp)]
        L.kh_comm_destroy.argtypes = [vp]
        L.kh_comm_destroy.restype = None
        L.kh_comm_rank.argtypes = [vp]
        L.kh_comm_world.argtypes = [vp]
        L.kh_comm_device.argtypes = [vp]
        L.kh_comm_allreduce_sum_f64.argtypes = [vp, vp, C.c_int64, vp]
        L.kh_comm_allgather_f64.argtypes = [vp, vp, vp, C.c_int64, vp]
        L.kh_spa_set_comm.argtypes = [vp, vp]
        L.kh_device_malloc.argtypes = [i32, C.c_int64, C.POINTER(vp)]
        L.kh_device_free.argtypes = [vp]
        L.kh_device_free.restype = None
        L.kh_device_upload.argtypes = [vp, vp, C.c_int64]
        L.kh_device_upload_on.argtypes = [vp, vp, C.c_int64, vp]
        L.kh_device_download.argtypes = [vp, vp, C.c_int64]
        L.kh_selftest_lds_attr.argtypes = []
        L.kh_selftest_lds_attr.restype = C.c_int
    if hasattr(L, "kh_graph_create"):
        L.kh_graph_create.argtypes = [i32, C.POINTER(vp)]
        L.kh_graph_destroy.argtypes = [vp]
        L.kh_graph_destroy.restype = None
        L.kh_graph_set.argtypes = [vp, i32, dptr, iptr, iptr]
        L.kh_graph_set_positions.argtypes = [vp, i32, dptr]
        L.kh_graph_find_loop_candidates.argtypes = [vp, i32, iptr, dbl, i32, iptr, iptr, i32, C.POINTER(i32)]
        L.kh_graph_last_kernel_ms.argtypes = [vp]
        L.kh_graph_find_near_chains.argtypes = [vp, i32, dbl, iptr, i32, C.POINTER(i32)]
        L.kh_graph_closest_scan_to_pose.argtypes = [vp, iptr, i32, dptr, C.POINTER(i32)]
        L.kh_weighted_mean.argtypes = [i32, dptr, dptr, dptr]
        L.kh_graph_last_kernel_ms.restype = dbl
    if hasattr(L, "kh_mapper_create"):
        L.kh_graph_find_loop_candidates_from.argtypes = [vp, i32, iptr, vp, dbl, i32, iptr, iptr, i32, C.POINTER(i32)]
        L.kh_mapper_params_default.argtypes = [C.POINTER(KhMapperParams)]
        L.kh_mapper_params_default.restype = None
        L.kh_mapper_create.argtypes = [C.POINTER(KhMapperParams), C.POINTER(KhLaser), i32, i32, C.POINTER(vp)]
        L.kh_mapper_get_adjacency.argtypes = [vp, i32, iptr, i32, C.POINTER(i32)]
        L.kh_mapper_set_node_score.argtypes = [vp, i32, dbl]
        L.kh_mapper_create_on_devices.argtypes = [C.POINTER(KhMapperParams), C.POINTER(KhLaser), iptr, i32, i32, C.POINTER(vp)]
        L.kh_mapper_destroy.argtypes = [vp]
        L.kh_mapper_destroy.restype = None
        L.kh_mapper_process.argtypes = [vp, dptr, dptr, dbl, C.POINTER(i32), dptr, dptr]
        L.kh_mapper_num_scans.argtypes = [vp]
        L.kh_mapper_num_edges.argtypes = [vp]
        L.kh_mapper_num_edges.restype = C.c_int64
        L.kh_mapper_get_poses.argtypes = [vp, dptr]
        L.kh_mapper_get_scan.argtypes = [vp, i32, C.POINTER(KhScan), C.POINTER(KhScanBox)]
        L.kh_mapper_get_stats.argtypes = [vp, C.POINTER(KhMapperStats)]
        L.kh_mapper_solver.argtypes = [vp]
        L.kh_mapper_solver.restype = vp
        L.kh_mapper_get_covariances.argtypes = [vp, i32, vp, vp, C.POINTER(KhSpaCovSummary)]
        if hasattr(L, "kh_mapper_get_relative_covariances"):
            L.kh_mapper_get_relative_covariances.argtypes = [vp, i32, i32, vp, vp, C.POINTER(KhSpaCovColumnsSummary)]
        L.kh_mapper_set_log.argtypes = [vp, C.c_char_p]
        L.kh_mapper_remove_node.argtypes = [vp, i32]
        L.kh_mapper_set_lifelong.argtypes = [vp, C.POINTER(KhDecayParams)]
        L.kh_mapper_num_alive.argtypes = [vp]
        L.kh_mapper_get_alive.argtypes = [vp, iptr]
        L.kh_graph_set_scan_limit.argtypes = [vp, i32]
        L.kh_graph_append_scan.argtypes = [vp, dptr]
        L.kh_graph_add_edge.argtypes = [vp, i32, i32]
        L.kh_graph_set_position.argtypes = [vp, i32, dptr]
        L.kh_graph_find_near_linked.argtypes = [vp, i32, dbl, iptr, i32, C.POINTER(i32)]
    if hasattr(L, "kh_graph_find_near_by_scan"):
        L.kh_graph_set_poses.argtypes = [vp, i32, vp]
        L.kh_graph_set_pose.argtypes = [vp, i32, vp]
        L.kh_graph_append_scan_with_pose.argtypes = [vp, vp, vp]
        L.kh_graph_find_near_by_scan.argtypes = [vp, i32, vp, vp, vp]
        L.kh_graph_find_near_by_vertices.argtypes = [vp, vp, dbl, vp, i32, C.POINTER(i32)]
        L.kh_graph_last_near_by_kernel_ms.argtypes = [vp]
        L.kh_graph_last_near_by_kernel_ms.restype = dbl
        L.kh_mapper_process_localization.argtypes = [vp, vp, vp, dbl, C.POINTER(i32), vp, vp]
        L.kh_mapper_process_against_node.argtypes = [vp, vp, vp, dbl, i32, C.POINTER(i32), vp, vp]
        L.kh_mapper_process_against_nodes_near_by.argtypes = [vp, vp, vp, dbl, i32, C.POINTER(i32), vp, vp]
        L.kh_mapper_clear_localization_buffer.argtypes = [vp]
        L.kh_mapper_localization_buffer.argtypes = [vp, vp, i32, C.POINTER(i32)]
    if hasattr(L, "kh_mapper_save"):
        L.kh_mapper_save.argtypes = [vp, C.c_char_p]
        L.kh_mapper_load.argtypes = [C.c_char_p, iptr, i32, i32, C.POINTER(vp)]
        L.kh_session_info.argtypes = [C.c_char_p, C.POINTER(KhSessionInfo)]
        L.kh_session_last_load_ms.argtypes = [dptr]
        L.kh_mapper_build_map.argtypes = [vp, dbl, C.c_uint32, dbl, C.POINTER(vp)]
        L.kh_occupancy_geometry.argtypes = [vp, dptr, C.POINTER(dbl)]
        L.kh_mapper_map_stats.argtypes = [vp, np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")]
    if hasattr(L, "kh_merge_create"):
        L.kh_merge_create.argtypes = [i32, dbl, C.POINTER(vp)]
        L.kh_merge_destroy.argtypes = [vp]
        L.kh_merge_destroy.restype = None
        L.kh_merge_add_mapper.argtypes = [vp, vp, C.POINTER(i32)]
        L.kh_merge_add_session.argtypes = [vp, C.c_char_p, C.POINTER(i32)]
        L.kh_merge_remove_submap.argtypes = [vp, i32]
        L.kh_merge_num_submaps.argtypes = [vp]
        L.kh_merge_submap_info.argtypes = [vp, i32, iptr]
        L.kh_merge_set_transform.argtypes = [vp, i32, dptr]
        L.kh_merge_get_transform.argtypes = [vp, i32, dptr]
        L.kh_merge_move_submap.argtypes = [vp, i32, dptr]
        L.kh_merge_get_location.argtypes = [vp, i32, dptr]
        L.kh_merge_get_scan.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
        L.kh_merge_build_submap.argtypes = [vp, i32, C.c_uint32, dbl, C.POINTER(vp)]
        L.kh_merge_build.argtypes = [vp, C.c_uint32, dbl, C.POINTER(vp)]
        L.kh_merge_stats.argtypes = [vp, np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")]
    if hasattr(L, "kh_merge_fit"):
        L.kh_merge_fit.argtypes = [vp, i32, i32, vp, C.c_uint32, dbl, C.POINTER(KhMergeFit)]
        L.kh_merge_fit_stats.argtypes = [vp, np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")]
        L.kh_merge_align_params_default.argtypes = [vp, i32, C.POINTER(KhMergeAlignParams)]
        L.kh_merge_align_params_default.restype = None
        L.kh_merge_align.argtypes = [vp, i32, i32, C.POINTER(KhMergeAlignParams), C.POINTER(KhMergeAlignCand), i32, C.POINTER(i32), vp]
    if hasattr(L, "kh_live_map_create"):
        L.kh_mapper_set_scan_pose.argtypes = [vp, i32, dptr]
        L.kh_live_map_create.argtypes = [vp, dbl, vp, dbl, C.POINTER(vp)]
        L.kh_live_map_destroy.argtypes = [vp]
        L.kh_live_map_destroy.restype = None
        L.kh_live_map_update.argtypes = [vp, C.c_uint32, dbl]
        L.kh_live_map_info.argtypes = [vp, C.POINTER(KhLiveMapInfo)]
        L.kh_live_map_read.argtypes = [vp, vp, vp, vp]
        L.kh_live_map_stats.argtypes = [vp, C.POINTER(KhLiveMapStats)]
    if hasattr(L, "kh_map_feed_create"):
        L.kh_map_feed_create.argtypes = [vp, C.POINTER(vp)]
        L.kh_map_feed_destroy.argtypes = [vp]
        L.kh_map_feed_destroy.restype = None
        L.kh_map_feed_poll.argtypes = [vp, C.POINTER(KhMapFeedDelta)]
        L.kh_map_feed_tiles.argtypes = [vp, vp, vp]
        L.kh_map_feed_read.argtypes = [vp, i32, i32, i32, i32, vp]
        L.kh_map_feed_stats.argtypes = [vp, C.POINTER(KhMapFeedStats)]
    if hasattr(L, "kh_mapper_relocalize"):
        L.kh_graph_relocalize_candidates.argtypes = [vp, dbl, dbl, i32, vp, dbl, vp, i32, C.POINTER(i32), vp, vp, i32, C.POINTER(i32)]
        L.kh_graph_last_relocalize_kernel_ms.argtypes = [vp]
        L.kh_graph_last_relocalize_kernel_ms.restype = dbl
        L.kh_relocalize_params_default.argtypes = [C.POINTER(KhMapperParams), C.POINTER(KhRelocalizeParams)]
        L.kh_relocalize_params_default.restype = None
        L.kh_mapper_get_params.argtypes = [vp, C.POINTER(KhMapperParams)]
        L.kh_mapper_relocalize.argtypes = [vp, vp, C.POINTER(KhRelocalizeParams), C.POINTER(KhRelocalizeHyp), i32, C.POINTER(KhRelocalizeSummary)]
    if hasattr(L, "kh_lifelong_scores"):
        L.kh_decay_params_default.argtypes = [C.POINTER(KhDecayParams)]
        L.kh_decay_params_default.restype = None
        L.kh_lifelong_scores.argtypes = [i32, C.POINTER(KhScanBox), i32, C.POINTER(KhScanBox), C.POINTER(KhDecayParams),
                                         vp, vp, vp, vp, vp]
        L.kh_lifelong_scores_resident.argtypes = [i32, C.POINTER(KhScanBox), i32, C.POINTER(KhScanBox), C.POINTER(vp), C.POINTER(vp), i32,
                                                  C.POINTER(KhDecayParams), vp, vp, vp, vp, vp]
    if hasattr(L, "kh_occupancy_create"):
        L.kh_occupancy_compute_dimensions.argtypes = [i32, C.POINTER(KhScan), dbl, dbl, dbl, C.POINTER(i32), C.POINTER(i32), dptr]
        L.kh_occupancy_create.argtypes = [i32, i32, dbl, dbl, dbl, i32, C.POINTER(vp)]
        L.kh_occupancy_destroy.argtypes = [vp]
        L.kh_occupancy_destroy.restype = None
        L.kh_occupancy_clear.argtypes = [vp]
        L.kh_occupancy_add_scans.argtypes = [vp, i32, C.POINTER(KhScan), dbl, dbl, dbl]
        L.kh_occupancy_update.argtypes = [vp, C.c_uint32, dbl]
        L.kh_occupancy_read.argtypes = [vp, vp, vp, vp]
        if hasattr(L, "kh_occupancy_read_nav"):
            L.kh_occupancy_read_nav.argtypes = [vp, vp]
        L.kh_occupancy_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(dbl), C.POINTER(C.c_int64)]
    _lib = L
    return L


def audit_summary_dict(s):
    out = {k: getattr(s, k) for k, _ in KhSpaAuditSummary._fields_ if k != "cov"}
    out["cov"] = {k: getattr(s.cov, k) for k, _ in KhSpaCovSummary._fields_ if k != "pad"}
    return out


def check(code, where):
    if code != KH_OK:
        raise KartoHipError(code, where)
