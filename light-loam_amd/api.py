"""ctypes binding of the C ABI (include/lightloam_hip.h) -- plumbing for tests, smoke and bench.

Fails loudly when the HIP library is missing or no gfx950 device is usable: there is no CPU fallback.
"""
import ctypes as C
import os
import weakref

import numpy as np

from .build import lib_path

POINT = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("intensity", "f4")])

LL_OK = 0
STATUS = {0: "LL_OK", -1: "LL_ERR_DEVICE", -2: "LL_ERR_ARG", -3: "LL_ERR_BAD_RINGS", -4: "LL_ERR_CAPACITY",
          -5: "LL_ERR_EMPTY", -6: "LL_ERR_HIP", -7: "LL_ERR_STATE"}

EXPORTS = [
    "ll_default_params", "ll_create", "ll_destroy", "ll_last_error", "ll_abi_version", "ll_stream", "ll_synchronize",
    "ll_upload_scan", "ll_extract_batch", "ll_get_scan_info", "ll_download_cloud", "ll_download_labels",
    "ll_download_features", "ll_set_target", "ll_upload_features", "ll_set_target_from_slot", "ll_associate_batch", "ll_get_pair_info",
    "ll_download_edge_corr", "ll_download_plane_corr", "ll_vote_batch", "ll_download_vote",
    "ll_normal_equations_batch", "ll_download_normal_equations", "ll_gn_step_batch", "ll_download_pose",
    "ll_residual_jacobian", "ll_hot_path_batch", "ll_algorithmic_bytes", "ll_profile_enable", "ll_profile_read", "ll_set_pose_guess", "ll_debug_counters", "ll_vote_host", "ll_debug_calibration_copy", "ll_debug_launch_stage", "ll_debug_exact_math", "ll_upload_scan_async", "ll_upload_scans_async", "ll_upload_scans_async_strided", "ll_stream_record", "ll_stream_wait", "ll_hot_path_chain", "ll_synchronize_copy", "ll_host_alloc", "ll_host_free",
    "ll_lm_default_options", "ll_lm_solve_batch", "ll_odometry_frames", "ll_odometry_sequences", "ll_set_two_stream",
    "ll_map_create", "ll_map_destroy", "ll_map_last_error", "ll_map_set_map", "ll_map_set_scan", "ll_map_associate",
    "ll_map_residual_jacobian", "ll_map_get_counts", "ll_map_get_map_sizes", "ll_map_download_edges", "ll_map_download_planes", "ll_map_normal_equations", "ll_map_optimize",
    "ll_cubemap_create", "ll_cubemap_destroy", "ll_cubemap_last_error", "ll_cubemap_prepare", "ll_cubemap_optimize", "ll_cubemap_update",
    "ll_cubemap_process", "ll_cubemap_process_slot", "ll_cubemap_info", "ll_cubemap_download_cloud", "ll_cubemap_download_cube",
    "ll_map_set_map_ids", "ll_map_knn_partial", "ll_map_associate_merged", "ll_map_solve", "ll_map_set_row_shard", "ll_cubemap_set_shard", "ll_cubemap_map",
    "ll_factor_blocks_set", "ll_factor_blocks_set_s", "ll_factor_blocks_evaluate",
    "ll_map_evaluate_dev", "ll_map_lm_begin_dev", "ll_map_lm_propose_dev", "ll_map_lm_accept_dev", "ll_map_knn_partial_dev",
    "ll_map_associate_merged_dev", "ll_map_solve_dev",
    "ll_voxel_grid", "ll_map_set_pose", "ll_map_get_pose", "ll_map_evaluate", "ll_map_lm_begin", "ll_map_lm_propose", "ll_map_lm_accept",
    "ll_cubemaps_create", "ll_cubemaps_destroy", "ll_cubemaps_last_error", "ll_cubemaps_process_slots", "ll_cubemaps_process",
    "ll_cubemaps_info", "ll_cubemaps_download_cloud", "ll_cubemaps_download_cube", "ll_cubemaps_stats",
    "ll_cubemaps_reset", "ll_drives_create", "ll_drives_destroy", "ll_drives_last_error", "ll_drives_slots", "ll_drives_step",
    "ll_drives_registered", "ll_drives_stats", "ll_drives_cubemaps",
    "ll_cubemaps_export_sizes", "ll_cubemaps_export", "ll_cubemaps_export_timing", "ll_cubemap_export",
    "ll_cubemaps_layout", "ll_cubemaps_import", "ll_cubemap_layout", "ll_cubemap_import",
    "ll_drives_save_size", "ll_drives_save", "ll_drives_restore", "ll_checkpoint_describe",
    "ll_cubemaps_localize_slots", "ll_drives_set_localize", "ll_drives_fit",
    "ll_cubemaps_localize_slots_info", "ll_cubemaps_align_info", "ll_drives_set_info", "ll_drives_info", "ll_pg_edge_from_info",
    "ll_posegraphs_evaluate6", "ll_posegraphs_solve6",
    "ll_cubemaps_merge", "ll_cubemaps_merge_timing",
    "ll_cubemaps_align", "ll_cubemaps_align_timing",
    "ll_debug_sort_pairs", "ll_debug_exscan", "ll_debug_voxel_segments",
    "ll_set_deskew", "ll_deskew_slots",
    "ll_map_set_vote", "ll_map_download_vote", "ll_map_vote_host", "ll_cubemap_set_vote", "ll_cubemaps_set_vote", "ll_drives_set_map_vote",
    "ll_places_default_params", "ll_places_create", "ll_places_destroy", "ll_places_last_error", "ll_places_size", "ll_places_reset",
    "ll_places_add_slots", "ll_places_add_points", "ll_places_upload", "ll_places_download", "ll_places_distances", "ll_places_match",
    "ll_places_timing",
    "ll_pg_default_options", "ll_posegraphs_create", "ll_posegraphs_destroy", "ll_posegraphs_last_error", "ll_posegraphs_evaluate",
    "ll_posegraphs_solve", "ll_posegraphs_timing",
    "ll_posegraphs_set_preconditioner", "ll_posegraphs_preconditioner", "ll_posegraphs_precond_stats", "ll_posegraphs_chain_solve",
    "ll_pg_cov_default_options", "ll_posegraphs_covariances", "ll_posegraphs_covariances6", "ll_posegraphs_cov_timing", "ll_pg_edge_gate",
    "ll_keyframes_create", "ll_keyframes_destroy", "ll_keyframes_last_error", "ll_keyframes_size", "ll_keyframes_reset", "ll_keyframes_info",
    "ll_keyframes_add_cubemaps", "ll_keyframes_add_points", "ll_keyframes_export",
    "ll_cubemaps_insert_keyframes", "ll_cubemaps_insert_timing", "ll_drives_set_keyframes", "ll_drives_correct",
    "ll_visibility_default_params", "ll_visibility_create", "ll_visibility_destroy", "ll_visibility_last_error", "ll_visibility_run",
    "ll_visibility_counts", "ll_visibility_images", "ll_visibility_reset", "ll_visibility_timing", "ll_cubemaps_insert_keyframes_filtered",
    "ll_bev_default_params", "ll_bev_create", "ll_bev_destroy", "ll_bev_last_error", "ll_bev_match", "ll_bev_volume", "ll_bev_grid", "ll_bev_reset",
    "ll_bev_timing", "ll_bev_guess",
    "ll_entropy_default_params", "ll_entropy_create", "ll_entropy_destroy", "ll_entropy_last_error", "ll_entropy_run", "ll_entropy_values",
    "ll_entropy_reset", "ll_entropy_timing",
    "ll_pcm_default_params", "ll_pcm_create", "ll_pcm_destroy", "ll_pcm_last_error", "ll_pcm_run", "ll_pcm_select", "ll_pcm_adjacency",
    "ll_pcm_timing", "ll_pcm_host",
]

MAP_NONE, MAP_SURROUND, MAP_ALL = -1, 0, 1
N_CUBES = 4851                  # laserCloudNum: 21 x 21 x 11


class Params(C.Structure):
    _fields_ = [("n_scans", C.c_int), ("ring_model", C.c_int), ("minimum_range", C.c_float),
                ("lower_bound", C.c_float), ("up_bound", C.c_float), ("max_points", C.c_int),
                ("max_ring_points", C.c_int), ("batch", C.c_int), ("curv_threshold", C.c_float),
                ("gap_sq_threshold", C.c_float), ("leaf_size", C.c_float), ("nn_dist_sq_max", C.c_float),
                ("nearby_scan", C.c_float), ("huber_delta", C.c_float), ("write_curvature", C.c_int),
                ("chunk", C.c_int), ("distortion", C.c_int), ("voxel_sort_ranks", C.c_int), ("input_stride_floats", C.c_int)]


class ScanInfo(C.Structure):
    _fields_ = [("status", C.c_int), ("n_in", C.c_int), ("n", C.c_int), ("n_sharp", C.c_int),
                ("n_less_sharp", C.c_int), ("n_flat", C.c_int), ("n_less_flat", C.c_int), ("max_ring", C.c_int)]


class LmOptions(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int), ("initial_radius", C.c_double), ("max_radius", C.c_double),
                ("min_radius", C.c_double), ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
                ("max_lm_diagonal", C.c_double), ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double), ("jacobi_scaling", C.c_int)]


class PairInfo(C.Structure):
    _fields_ = [("n_edge", C.c_int), ("n_plane", C.c_int), ("n_plane_selected", C.c_int)]


class LocalizeFit(C.Structure):
    """ll_localize_fit: how a localised pose fits the frozen map (residual blocks, Huber cost, sums of squared residuals)"""
    _fields_ = [("n_edge", C.c_int), ("n_plane", C.c_int), ("cost", C.c_double), ("sq_edge", C.c_double), ("sq_plane", C.c_double)]


class PoseInfo(C.Structure):
    """ll_pose_info: the Gauss-Newton information of a scan-to-map solve at its final pose (H 6 x 6 row-major and g over the
    increment (half-angle vector, translation), its eigenvalues ascending, the residual variance, rows, flags)"""
    _fields_ = [("H", C.c_double * 36), ("g", C.c_double * 6), ("eig", C.c_double * 6), ("sigma2", C.c_double), ("rows", C.c_int), ("flags", C.c_int)]


class MergeOp(C.Structure):
    """ll_merge_op: map src goes into map dst under the pose T_w7 (qx, qy, qz, qw, tx, ty, tz)"""
    _fields_ = [("dst", C.c_int), ("src", C.c_int), ("T_w7", C.c_double * 7)]


class KeyframesParams(C.Structure):
    _fields_ = [("max_frames", C.c_int), ("cap_corner", C.c_longlong), ("cap_surf", C.c_longlong)]


class KeyframeInfo(C.Structure):
    """ll_keyframe_info: n, offset per cloud type (corner, surf); offset in points into the type's pool"""
    _fields_ = [("lane", C.c_int), ("frame_index", C.c_int), ("n", C.c_int * 2), ("offset", C.c_longlong * 2), ("pose_w7", C.c_double * 7)]


class InsertOp(C.Structure):
    """ll_insert_op: the listed frames of a Keyframes store go into map dst, frame k under poses_w7[k] (NULL: its stored pose)"""
    _fields_ = [("dst", C.c_int), ("n_frames", C.c_int), ("frames", C.c_void_p), ("poses_w7", C.c_void_p), ("reset", C.c_int), ("cen", C.c_int * 3)]


class VisibilityParams(C.Structure):
    """ll_visibility_params: the range image (width x height over el_min_deg .. el_max_deg, ranges min_range .. max_range), the vote
    (margin_abs + margin_rel * r, observers within radius) and how many frames one run may list"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("el_min_deg", C.c_float), ("el_max_deg", C.c_float), ("min_range", C.c_float),
                ("max_range", C.c_float), ("margin_abs", C.c_float), ("margin_rel", C.c_float), ("radius", C.c_float), ("max_images", C.c_int)]


class VisibilityOp(C.Structure):
    """ll_visibility_op: the listed frames of one drive observe each other, frame k under poses_w7[k] (NULL: its stored pose)"""
    _fields_ = [("n_frames", C.c_int), ("frames", C.c_void_p), ("poses_w7", C.c_void_p)]


class VisibilityRule(C.Structure):
    """ll_visibility_rule: a point is removed iff through >= min_through and hit <= max_hit"""
    _fields_ = [("min_through", C.c_int), ("max_hit", C.c_int)]


class BevParams(C.Structure):
    """ll_bev_params: the grid (cell metres, 2 half cells a side about the anchor's sensor, eight layers of z_layer from z_min), the
    search (shifts -shift_half .. shift_half - 1), the exclusion window of `second`, and the limits of one call"""
    _fields_ = [("cell", C.c_float), ("half", C.c_int), ("shift_half", C.c_int), ("z_min", C.c_float), ("z_layer", C.c_float), ("excl_yaw", C.c_int),
                ("excl_shift", C.c_int), ("max_ops", C.c_int), ("max_yaws", C.c_int), ("max_points", C.c_longlong)]


class BevOp(C.Structure):
    """ll_bev_op: the query frames against the target frames (the first of a list is its anchor; frame k under its row of the poses,
    NULL: its stored pose) over the yaws yaw0 + j * yaw_step, j < n_yaws"""
    _fields_ = [("n_target", C.c_int), ("target", C.c_void_p), ("target_poses_w7", C.c_void_p), ("n_query", C.c_int), ("query", C.c_void_p),
                ("query_poses_w7", C.c_void_p), ("yaw0", C.c_double), ("yaw_step", C.c_double), ("n_yaws", C.c_int)]


class BevResult(C.Structure):
    """ll_bev_result: the best hypothesis (iyaw, sx, sy) and its score, the best score outside the exclusion window (-1: none), the
    query points with a layer, the yaw and D_w7 with p_target ~ D p_query"""
    _fields_ = [("score", C.c_int), ("second", C.c_int), ("iyaw", C.c_int), ("sx", C.c_int), ("sy", C.c_int), ("n_query", C.c_int), ("yaw", C.c_double),
                ("D_w7", C.c_double * 7)]


class EntropyParams(C.Structure):
    """ll_entropy_params: the neighbourhood (radius, at least min_neighbours points), the floor under an eigenvalue inside the
    logarithm, and how many points one run may list"""
    _fields_ = [("radius", C.c_float), ("min_neighbours", C.c_int), ("lambda_floor", C.c_float), ("max_points", C.c_longlong)]


class EntropyOp(C.Structure):
    """ll_entropy_op: the cloud of the listed frames, frame k under poses_w7[k] (NULL: its stored pose)"""
    _fields_ = [("n_frames", C.c_int), ("frames", C.c_void_p), ("poses_w7", C.c_void_p)]


class EntropyRec(C.Structure):
    """ll_entropy_rec: an op's points by kind, the neighbour pairs, the sums of the stored h and pv of the valid points, their means"""
    _fields_ = [("n_points", C.c_longlong), ("n_valid", C.c_longlong), ("n_sparse", C.c_longlong), ("n_outside", C.c_longlong),
                ("n_pairs", C.c_longlong), ("sum_h", C.c_double), ("sum_pv", C.c_double), ("mme", C.c_double), ("mpv", C.c_double)]


class PcmParams(C.Structure):
    """ll_pcm_params: a pair of candidates is consistent if its cycle closes within rot_tol + rot_rate * L radians and trans_tol +
    trans_rate * L metres, L the path length between the two candidates' endpoints"""
    _fields_ = [("rot_tol", C.c_double), ("trans_tol", C.c_double), ("rot_rate", C.c_double), ("trans_rate", C.c_double)]


class PcmRecord(C.Structure):
    """ll_pcm_record: a graph's candidates, the size of the selected set, the start it grew from (original index, -1: none), the largest
    degree and the consistent pairs"""
    _fields_ = [("n_candidates", C.c_int), ("n_selected", C.c_int), ("start", C.c_int), ("max_degree", C.c_int),
                ("n_consistent_pairs", C.c_longlong)]


class SeqLayout(C.Structure):
    """ll_seq_layout: S sequences side by side in a ring of `ring_rows` rows of S contiguous slots from slot `base`"""
    _fields_ = [("base", C.c_int), ("n_seq", C.c_int), ("ring_rows", C.c_int)]


def sequence_slot(layout, row, q):
    """the slot of frame row `row` of sequence `q`: base + (row mod ring_rows) * n_seq + q"""
    return layout.base + (row % layout.ring_rows) * layout.n_seq + q


class LightLoamError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


_lib = None


def load_library():
    """dlopen the in-tree HIP library.  Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        _lib = C.CDLL(path)
        _lib.ll_last_error.restype = C.c_char_p
        _lib.ll_last_error.argtypes = [C.c_void_p]
        _lib.ll_stream.restype = C.c_void_p
        _lib.ll_stream.argtypes = [C.c_void_p]
        _lib.ll_create.argtypes = [C.c_int, C.POINTER(Params), C.POINTER(C.c_void_p)]
        _lib.ll_destroy.argtypes = [C.c_void_p]
        _lib.ll_host_alloc.restype = C.c_void_p
        _lib.ll_host_alloc.argtypes = [C.c_size_t]
        _lib.ll_host_free.argtypes = [C.c_void_p]
        _lib.ll_cubemaps_export_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ll_cubemaps_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
        _lib.ll_cubemaps_export_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ll_cubemap_export.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
        _lib.ll_cubemaps_layout.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ll_cubemaps_import.argtypes = [C.c_void_p] * 8
        _lib.ll_cubemap_layout.argtypes = [C.c_void_p] * 5
        _lib.ll_cubemap_import.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _lib.ll_drives_save_size.restype = C.c_longlong
        _lib.ll_drives_save_size.argtypes = [C.c_void_p, C.c_void_p]
        _lib.ll_drives_save.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
        _lib.ll_drives_restore.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
        _lib.ll_cubemaps_localize_slots.argtypes = [C.c_void_p] * 6
        _lib.ll_cubemaps_localize_slots_info.argtypes = [C.c_void_p] * 7
        _lib.ll_cubemaps_align_info.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        _lib.ll_drives_set_info.argtypes = [C.c_void_p, C.c_int]
        _lib.ll_drives_info.argtypes = [C.c_void_p] * 2
        _lib.ll_pg_edge_from_info.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p]
        _lib.ll_posegraphs_evaluate6.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
        _lib.ll_posegraphs_solve6.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
        _lib.ll_drives_set_localize.argtypes = [C.c_void_p] * 3
        _lib.ll_drives_fit.argtypes = [C.c_void_p] * 2
        _lib.ll_checkpoint_describe.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
        _lib.ll_cubemaps_last_error.restype = C.c_char_p             # a borrowed CubeMaps (Drives.cubemaps) runs no CubeMaps.__init__
        _lib.ll_cubemaps_last_error.argtypes = [C.c_void_p]
        _lib.ll_cubemaps_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ll_cubemaps_merge_timing.argtypes = [C.c_void_p] * 3
        _lib.ll_cubemaps_align.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ll_cubemaps_align_timing.argtypes = [C.c_void_p] * 3
        _lib.ll_set_deskew.argtypes = [C.c_void_p, C.c_int]
        _lib.ll_deskew_slots.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        _lib.ll_map_set_vote.argtypes = [C.c_void_p, C.c_int]
        _lib.ll_map_download_vote.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ll_map_vote_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ll_cubemap_set_vote.argtypes = [C.c_void_p, C.c_int]
        _lib.ll_cubemaps_set_vote.argtypes = [C.c_void_p, C.c_void_p]
        _lib.ll_drives_set_map_vote.argtypes = [C.c_void_p, C.c_int]
        _lib.ll_places_default_params.restype = None
        _lib.ll_places_default_params.argtypes = [C.c_void_p, C.c_int]
        _lib.ll_places_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ll_places_destroy.restype = None
        _lib.ll_places_destroy.argtypes = [C.c_void_p]
        _lib.ll_places_last_error.restype = C.c_char_p
        _lib.ll_places_last_error.argtypes = [C.c_void_p]
        _lib.ll_places_size.argtypes = [C.c_void_p]
        _lib.ll_places_reset.argtypes = [C.c_void_p]
        _lib.ll_places_add_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ll_places_add_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ll_places_upload.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib.ll_places_download.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _lib.ll_places_distances.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ll_places_match.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ll_places_timing.argtypes = [C.c_void_p] * 3
        _lib.ll_pg_default_options.restype = None
        _lib.ll_pg_default_options.argtypes = [C.c_void_p]
        _lib.ll_posegraphs_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.ll_posegraphs_destroy.restype = None
        _lib.ll_posegraphs_destroy.argtypes = [C.c_void_p]
        _lib.ll_posegraphs_last_error.restype = C.c_char_p
        _lib.ll_posegraphs_last_error.argtypes = [C.c_void_p]
        _lib.ll_posegraphs_evaluate.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
        _lib.ll_posegraphs_solve.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
        _lib.ll_posegraphs_timing.argtypes = [C.c_void_p] * 3
        _lib.ll_posegraphs_set_preconditioner.argtypes = [C.c_void_p, C.c_int]
        _lib.ll_posegraphs_preconditioner.argtypes = [C.c_void_p]
        _lib.ll_posegraphs_precond_stats.argtypes = [C.c_void_p] * 2
        _lib.ll_posegraphs_chain_solve.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
        _lib.ll_pg_cov_default_options.restype = None
        _lib.ll_pg_cov_default_options.argtypes = [C.c_void_p]
        _lib.ll_posegraphs_covariances.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4
        _lib.ll_posegraphs_covariances6.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4
        _lib.ll_posegraphs_cov_timing.argtypes = [C.c_void_p] * 3
        _lib.ll_pg_edge_gate.argtypes = [C.c_void_p] * 7
        _lib.ll_keyframes_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ll_keyframes_destroy.restype = None
        _lib.ll_keyframes_destroy.argtypes = [C.c_void_p]
        _lib.ll_keyframes_last_error.restype = C.c_char_p
        _lib.ll_keyframes_last_error.argtypes = [C.c_void_p]
        _lib.ll_keyframes_size.argtypes = [C.c_void_p]
        _lib.ll_keyframes_reset.argtypes = [C.c_void_p]
        _lib.ll_keyframes_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.ll_keyframes_add_cubemaps.argtypes = [C.c_void_p] * 7
        _lib.ll_keyframes_add_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ll_keyframes_export.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ll_cubemaps_insert_keyframes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ll_cubemaps_insert_timing.argtypes = [C.c_void_p] * 3
        _lib.ll_drives_set_keyframes.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _lib.ll_drives_correct.argtypes = [C.c_void_p] * 3
        _lib.ll_visibility_default_params.restype = None
        _lib.ll_visibility_default_params.argtypes = [C.c_void_p]
        _lib.ll_visibility_create.argtypes = [C.c_void_p] * 3
        _lib.ll_visibility_destroy.restype = None
        _lib.ll_visibility_destroy.argtypes = [C.c_void_p]
        _lib.ll_visibility_last_error.restype = C.c_char_p
        _lib.ll_visibility_last_error.argtypes = [C.c_void_p]
        _lib.ll_visibility_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ll_visibility_counts.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.ll_visibility_images.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ll_visibility_reset.argtypes = [C.c_void_p]
        _lib.ll_visibility_timing.argtypes = [C.c_void_p] * 3
        _lib.ll_bev_default_params.restype = None
        _lib.ll_bev_default_params.argtypes = [C.c_void_p]
        _lib.ll_bev_create.argtypes = [C.c_void_p] * 3
        _lib.ll_bev_destroy.restype = None
        _lib.ll_bev_destroy.argtypes = [C.c_void_p]
        _lib.ll_bev_last_error.restype = C.c_char_p
        _lib.ll_bev_last_error.argtypes = [C.c_void_p]
        _lib.ll_bev_match.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ll_bev_volume.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.ll_bev_grid.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.ll_bev_reset.argtypes = [C.c_void_p]
        _lib.ll_bev_timing.argtypes = [C.c_void_p] * 3
        _lib.ll_bev_guess.argtypes = [C.c_void_p] * 4
        _lib.ll_entropy_default_params.restype = None
        _lib.ll_entropy_default_params.argtypes = [C.c_void_p]
        _lib.ll_entropy_create.argtypes = [C.c_void_p] * 3
        _lib.ll_entropy_destroy.restype = None
        _lib.ll_entropy_destroy.argtypes = [C.c_void_p]
        _lib.ll_entropy_last_error.restype = C.c_char_p
        _lib.ll_entropy_last_error.argtypes = [C.c_void_p]
        _lib.ll_entropy_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ll_entropy_values.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ll_entropy_reset.argtypes = [C.c_void_p]
        _lib.ll_entropy_timing.argtypes = [C.c_void_p] * 3
        _lib.ll_pcm_default_params.restype = None
        _lib.ll_pcm_default_params.argtypes = [C.c_void_p]
        _lib.ll_pcm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.ll_pcm_destroy.restype = None
        _lib.ll_pcm_destroy.argtypes = [C.c_void_p]
        _lib.ll_pcm_last_error.restype = C.c_char_p
        _lib.ll_pcm_last_error.argtypes = [C.c_void_p]
        _lib.ll_pcm_run.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
        _lib.ll_pcm_select.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        _lib.ll_pcm_adjacency.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.ll_pcm_timing.argtypes = [C.c_void_p] * 3
        _lib.ll_pcm_host.argtypes = [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
        _lib.ll_cubemaps_insert_keyframes_filtered.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


class _Handle:
    """what the classes over one of the library's handles share.  _DESTROY, _ERROR: the names of the handle's destroy and last-error
    functions; a class with a real difference (a borrowed handle, children to close first) overrides close"""
    _DESTROY = _ERROR = None

    def close(self):
        if getattr(self, "h", None):
            getattr(self.lib, self._DESTROY)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != LL_OK:
            raise LightLoamError(rc, getattr(self.lib, self._ERROR)(self.h).decode())

    def _timing(self, fn, n_ms, n_counts):
        """a *_timing function of the library as ((ms, ...), (counts, ...))"""
        ms = np.zeros(n_ms); cnt = np.zeros(n_counts, np.int64)
        self._ck(fn(self.h, ms.ctypes.data, cnt.ctypes.data))
        return tuple(ms), tuple(int(c) for c in cnt)


def _struct_params(struct, default_fn, kw):
    """a parameter struct as the library's default function fills it, with the given fields replaced"""
    p = struct()
    default_fn(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _frame_list(ids, poses):
    """(ids int32 [n], poses float64 [n, 7] or None) of one list of frames of a Keyframes store, as the library takes it; the caller
    keeps both alive over the call"""
    f = np.ascontiguousarray(ids, np.int32).reshape(-1)
    p = None if poses is None else np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
    if p is not None and len(p) != len(f):
        raise ValueError("poses must have one row per listed frame")
    return f, p


class PinnedStaging:
    """`count` scan slots of `stride_points` points each in ONE page-locked area: what an ingest thread fills and
    ll_upload_scans_async_strided copies with two enqueues"""

    def __init__(self, count, stride_points, floats_per_point=4):
        self.lib = load_library()
        self.fpp = int(floats_per_point)             # the context's resident layout (Params.input_stride_floats): 4, or 3 = x, y, z packed
        self.count, self.stride = int(count), int(stride_points) * 4 * self.fpp
        self.ptr = self.lib.ll_host_alloc(self.count * self.stride)
        if not self.ptr:
            raise MemoryError("ll_host_alloc failed")
        self.n = (C.c_int * self.count)()

    def put(self, i, xyz4):
        a = np.ascontiguousarray(np.asarray(xyz4, np.float32)[:, :self.fpp])   # an ingest thread's repack (KITTI .bin records carry a 4th float)
        assert a.ndim == 2 and a.shape[1] == self.fpp and a.nbytes <= self.stride
        C.memmove(self.ptr + i * self.stride, a.ctypes.data, a.nbytes)
        self.n[i] = len(a)

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.ll_host_free(C.c_void_p(self.ptr)); self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinnedScan:
    """an (n, 4) float32 scan in page-locked host memory (ll_host_alloc): the source of ll_upload_scan_async"""

    def __init__(self, xyz4, floats_per_point=4):
        a = np.ascontiguousarray(np.asarray(xyz4, np.float32)[:, :int(floats_per_point)])
        assert a.ndim == 2 and a.shape[1] == int(floats_per_point)
        self.n = len(a)
        self.lib = load_library()
        self.ptr = self.lib.ll_host_alloc(max(a.nbytes, 16))
        if not self.ptr:
            raise MemoryError("ll_host_alloc failed")
        C.memmove(self.ptr, a.ctypes.data, a.nbytes)

    def close(self):
        if getattr(self, "ptr", None):
            self.lib.ll_host_free(C.c_void_p(self.ptr)); self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_params(n_scans=64, **kw):
    p = Params()
    load_library().ll_default_params(C.byref(p), n_scans)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Context(_Handle):
    """One ll_ctx: `batch` scan slots resident in HBM on one GPU."""
    _DESTROY, _ERROR = "ll_destroy", "ll_last_error"

    def __init__(self, params, device=0):
        self.lib = load_library()
        self.params = params
        h = C.c_void_p()
        rc = self.lib.ll_create(device, C.byref(params), C.byref(h))
        if rc != LL_OK:
            raise LightLoamError(rc, self.lib.ll_last_error(None).decode())
        self.h = h
        self.R = params.n_scans
        self._children = weakref.WeakSet()      # Map / CubeMap objects living on this context: destroyed before it

    def close(self):
        if getattr(self, "h", None):
            for child in list(getattr(self, "_children", ())):   # a map outliving its context would free through a dangling pointer
                try:
                    child.close()
                except Exception:
                    pass
        super().close()

    @property
    def stream(self):
        return self.lib.ll_stream(self.h)

    def synchronize(self):
        self._ck(self.lib.ll_synchronize(self.h))

    # ---- input
    def upload_scan(self, slot, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        n, stride = (0, 4) if xyz.size == 0 else xyz.shape
        self._ck(self.lib.ll_upload_scan(self.h, slot, _ptr(xyz), stride, n))

    def upload_scan_async(self, slot, pinned):
        """enqueue the host -> device copy of a PinnedScan on the copy stream (ll_upload_scan_async)"""
        self._ck(self.lib.ll_upload_scan_async(self.h, slot, C.c_void_p(pinned.ptr), pinned.n))

    def upload_scans_async(self, first, pinned_list):
        """one call for a run of slots (the loop is in C: a Python call per scan would cost more than the copy's enqueue)"""
        k = len(pinned_list)
        ptrs = (C.c_void_p * k)(*[p.ptr for p in pinned_list]); ns = (C.c_int * k)(*[p.n for p in pinned_list])
        self._ck(self.lib.ll_upload_scans_async(self.h, first, k, ptrs, ns))

    def upload_staging_async(self, first, staging, i0=0, count=None):
        """slots first .. from entries i0 .. of a PinnedStaging (ll_upload_scans_async_strided)"""
        count = staging.count - i0 if count is None else count
        n = (C.c_int * count).from_buffer(staging.n, i0 * 4)
        self._ck(self.lib.ll_upload_scans_async_strided(self.h, first, count, C.c_void_p(staging.ptr + i0 * staging.stride), C.c_size_t(staging.stride), n))

    def stream_record(self, stream, ev):
        """mark "everything enqueued so far" on the compute (0) / copy (1) stream as event ev (0 .. 7)"""
        self._ck(self.lib.ll_stream_record(self.h, int(stream), int(ev)))

    def stream_wait(self, stream, ev):
        """what is enqueued on `stream` from now on waits for event ev"""
        self._ck(self.lib.ll_stream_wait(self.h, int(stream), int(ev)))

    def hot_path_chain(self, first, count, vote=True):
        """hot_path continuing a batch: slot `first` is matched against slot first - 1"""
        self._ck(self.lib.ll_hot_path_chain(self.h, first, count, int(bool(vote))))

    def synchronize_copy(self):
        self._ck(self.lib.ll_synchronize_copy(self.h))

    # ---- stages
    def extract(self, first=0, count=1):
        self._ck(self.lib.ll_extract_batch(self.h, first, count))

    def scan_info(self, slot=0):
        info = ScanInfo()
        self._ck(self.lib.ll_get_scan_info(self.h, slot, C.byref(info)))
        return info

    def cloud(self, slot=0):
        info = self.scan_info(slot)
        cloud = np.zeros((max(info.n, 1), 4), np.float32)
        ss = np.zeros(self.R, np.int32); se = np.zeros(self.R, np.int32)
        self._ck(self.lib.ll_download_cloud(self.h, slot, _ptr(cloud), len(cloud), _ptr(ss), _ptr(se)))
        return cloud[:info.n], ss, se

    def labels(self, slot=0, curvature=False):
        info = self.scan_info(slot)
        lab = np.zeros(max(info.n, 1), np.int8)
        cv = np.zeros(max(info.n, 1), np.float32) if curvature else None
        self._ck(self.lib.ll_download_labels(self.h, slot, _ptr(lab), _ptr(cv), len(lab)))
        return (lab[:info.n], cv[:info.n]) if curvature else lab[:info.n]

    def features(self, slot=0):
        info = self.scan_info(slot)
        arr = lambda n: np.zeros((max(n, 1), 4), np.float32)
        sh, ls, fl, lf = arr(info.n_sharp), arr(info.n_less_sharp), arr(info.n_flat), arr(info.n_less_flat)
        self._ck(self.lib.ll_download_features(self.h, slot, _ptr(sh), len(sh), _ptr(ls), len(ls), _ptr(fl), len(fl),
                                               _ptr(lf), len(lf)))
        return dict(sharp=sh[:info.n_sharp], less_sharp=ls[:info.n_less_sharp], flat=fl[:info.n_flat],
                    less_flat=lf[:info.n_less_flat])

    def set_target(self, corner_last, surf_last):
        c = np.ascontiguousarray(corner_last, np.float32).reshape(-1, 4)
        s = np.ascontiguousarray(surf_last, np.float32).reshape(-1, 4)
        self._ck(self.lib.ll_set_target(self.h, _ptr(c), len(c), _ptr(s), len(s)))

    def upload_features(self, slot, sharp, less_sharp, flat, less_flat):
        """the four feature clouds of a scan from host arrays into a slot (what a separate odometry process gets by topic)"""
        a = [np.ascontiguousarray(x, np.float32).reshape(-1, 4) for x in (sharp, less_sharp, flat, less_flat)]
        self._ck(self.lib.ll_upload_features(self.h, slot, _ptr(a[0]), len(a[0]), _ptr(a[1]), len(a[1]), _ptr(a[2]), len(a[2]),
                                             _ptr(a[3]), len(a[3])))

    def set_target_from_slot(self, slot):
        self._ck(self.lib.ll_set_target_from_slot(self.h, slot))

    @staticmethod
    def _poses(pose, count):
        if pose is None:
            return None
        p = np.ascontiguousarray(pose, np.float64).reshape(-1, 7)
        if len(p) == 1 and count > 1:
            p = np.repeat(p, count, axis=0)
        assert len(p) == count
        return np.ascontiguousarray(p)

    def associate(self, first=0, count=1, pose=None):
        p = self._poses(pose, count)
        self._ck(self.lib.ll_associate_batch(self.h, first, count, _ptr(p)))

    def set_pose_guess(self, first, count, pose):
        p = self._poses(pose, count)
        self._ck(self.lib.ll_set_pose_guess(self.h, first, count, _ptr(p)))

    def vote(self, first=0, count=1, enable=True):
        self._ck(self.lib.ll_vote_batch(self.h, first, count, int(bool(enable))))

    def pair_info(self, slot=0):
        info = PairInfo()
        self._ck(self.lib.ll_get_pair_info(self.h, slot, C.byref(info)))
        return info

    def edge_corr(self, slot=0):
        n = self.pair_info(slot).n_edge
        a = [np.zeros(max(n, 1), np.int32) for _ in range(3)]
        self._ck(self.lib.ll_download_edge_corr(self.h, slot, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), len(a[0])))
        return tuple(x[:n] for x in a)

    def plane_corr(self, slot=0):
        n = self.pair_info(slot).n_plane
        a = [np.zeros(max(n, 1), np.int32) for _ in range(4)]
        self._ck(self.lib.ll_download_plane_corr(self.h, slot, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), len(a[0])))
        return tuple(x[:n] for x in a)

    def vote_result(self, slot=0):
        n = self.pair_info(slot).n_plane
        cnt = np.zeros(max(n, 1), np.int32); sel = np.zeros(max(n, 1), np.uint8); w = np.zeros(max(n, 1), np.float32)
        self._ck(self.lib.ll_download_vote(self.h, slot, _ptr(cnt), _ptr(sel), _ptr(w), len(cnt)))
        return cnt[:n], sel[:n].astype(bool), w[:n]

    def vote_points(self, src, tgt, corner_case=False):
        """graph_based_correspondence_vote_simple on caller-supplied correspondences (ll_vote_host): src / tgt (n, 4) float32,
        5 regions for the corner case, else 10 -> (count int32[n], selected bool[n], weight float32[n])"""
        s = np.ascontiguousarray(src, np.float32).reshape(-1, 4); t = np.ascontiguousarray(tgt, np.float32).reshape(-1, 4)
        assert len(s) == len(t)
        n = len(s)
        cnt = np.zeros(max(n, 1), np.int32); sel = np.zeros(max(n, 1), np.uint8); w = np.zeros(max(n, 1), np.float32)
        self._ck(self.lib.ll_vote_host(self.h, _ptr(s), _ptr(t), n, int(bool(corner_case)), _ptr(cnt), _ptr(sel), _ptr(w)))
        return cnt[:n], sel[:n].astype(bool), w[:n]

    def normal_equations(self, first=0, count=1, pose=None):
        p = self._poses(pose, count)
        self._ck(self.lib.ll_normal_equations_batch(self.h, first, count, _ptr(p)))

    def normal_equations_result(self, slot=0):
        H = np.zeros((6, 6)); g = np.zeros(6); cost = C.c_double(0)
        self._ck(self.lib.ll_download_normal_equations(self.h, slot, _ptr(H), _ptr(g), C.byref(cost)))
        return H, g, cost.value

    def gn_step(self, first=0, count=1):
        self._ck(self.lib.ll_gn_step_batch(self.h, first, count))

    def pose(self, slot=0):
        p = np.zeros(7)
        self._ck(self.lib.ll_download_pose(self.h, slot, _ptr(p)))
        return p

    def residual_jacobian(self, slot=0, pose=None):
        pi = self.pair_info(slot)
        rows = 3 * pi.n_edge + pi.n_plane_selected
        r = np.zeros(max(rows, 1)); Jq = np.zeros((max(rows, 1), 4)); Jt = np.zeros((max(rows, 1), 3))
        p = None if pose is None else np.ascontiguousarray(pose, np.float64)
        self._ck(self.lib.ll_residual_jacobian(self.h, slot, _ptr(p), _ptr(r), _ptr(Jq), _ptr(Jt), len(r)))
        return r[:rows], Jq[:rows], Jt[:rows]

    def lm_solve(self, first=0, count=1, opt=None):
        """ceres::Solve (LM, max 4 iterations) on the slot's current residual blocks, from the slot's current pose."""
        self._ck(self.lib.ll_lm_solve_batch(self.h, first, count, None if opt is None else C.byref(opt)))

    def odometry_frames(self, first, count, pose0=None, n_outer=3, first_frame_index=1, opt=None):
        """laserOdometry's frame loop over consecutive slots; returns the (count, 7) relative poses (q_last_curr, t_last_curr)."""
        out = np.zeros((count, 7))
        p0 = None if pose0 is None else np.ascontiguousarray(pose0, np.float64)
        self._ck(self.lib.ll_odometry_frames(self.h, first, count, _ptr(p0), n_outer, first_frame_index,
                                             None if opt is None else C.byref(opt), _ptr(out)))
        return out

    def odometry_sequences(self, n_seq, ring_rows, row0, n_rows, base=0, seq_rows=None, frame_index0=1, pose0=None, n_outer=3, opt=None):
        """the frame loop of n_seq sequences side by side (ll_odometry_sequences); returns the (n_rows, n_seq, 7) relative poses,
        NaN for the rows a sequence did not run.  frame_index0: one int or one per sequence; pose0: None (continue from the poses
        on the device), one pose or (n_seq, 7)."""
        L = SeqLayout(base, n_seq, ring_rows)
        rows = None if seq_rows is None else np.ascontiguousarray(np.broadcast_to(np.asarray(seq_rows, np.int32), (n_seq,)))
        fidx = np.ascontiguousarray(np.broadcast_to(np.asarray(frame_index0, np.int32), (n_seq,)))
        p0 = self._poses(pose0, n_seq)
        out = np.zeros((n_rows, n_seq, 7))
        self._ck(self.lib.ll_odometry_sequences(self.h, C.byref(L), int(row0), int(n_rows), _ptr(rows), _ptr(fidx), _ptr(p0), int(n_outer),
                                                None if opt is None else C.byref(opt), _ptr(out)))
        return out

    def set_deskew(self, mode):
        """TransformToEnd in the frame loops (ll_set_deskew): 0 off, 1 the solved slots' less-sharp / less-flat clouds are re-projected
        to the end of their sweep in place, 2 also laserCloud.  Needs Params.distortion = 1 (LL_ERR_STATE otherwise)."""
        self._ck(self.lib.ll_set_deskew(self.h, int(mode)))

    def deskew_slots(self, first, count, poses=None, mode=1):
        """the stage on its own (ll_deskew_slots): slots [first, first + count) with `poses` ((count, 7) or one pose; None = the poses
        the slots hold on the device), then their search grids anew.  A slot takes it once per extraction / upload."""
        p = self._poses(poses, count)
        self._ck(self.lib.ll_deskew_slots(self.h, int(first), int(count), _ptr(p), int(mode)))

    def hot_path(self, first=0, count=1, pose=None, vote=True):
        p = self._poses(pose, count)
        self._ck(self.lib.ll_hot_path_batch(self.h, first, count, _ptr(p), int(bool(vote))))

    def set_two_stream(self, on=True):
        """association stage of hot_path on two streams (default) or kernel after kernel (ll_set_two_stream)"""
        self._ck(self.lib.ll_set_two_stream(self.h, int(bool(on))))

    def profile_enable(self, on=True):
        self._ck(self.lib.ll_profile_enable(self.h, int(bool(on))))

    def profile_read(self, reset=True):
        """{kernel name: (total_ms, launches)} measured with HIP events on the ctx stream."""
        n = C.c_int(16)
        names = (C.c_char_p * 16)(); ms = (C.c_double * 16)(); launches = (C.c_int * 16)()
        self._ck(self.lib.ll_profile_read(self.h, C.byref(n), names, ms, launches, int(bool(reset))))
        return {names[i].decode(): (ms[i], launches[i]) for i in range(n.value)}

    def voxel_grid(self, points, leaf):
        """pcl::VoxelGrid on a whole cloud (N x 4 float32) -> filtered cloud"""
        pts = np.ascontiguousarray(points, np.float32)
        out = np.zeros((max(len(pts), 1), 4), np.float32); n = C.c_int(0)
        self._ck(self.lib.ll_voxel_grid(self.h, _ptr(pts), len(pts), C.c_float(leaf), _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def factor_blocks_set(self, edge9=None, plane13=None, pnorm7=None):
        """lidarFactor.hpp blocks of one problem: edge [n, 9], plane [n, 13], plane-norm [n, 7] (f64)."""
        e = np.ascontiguousarray(edge9 if edge9 is not None else np.zeros((0, 9)), np.float64).reshape(-1, 9)
        p = np.ascontiguousarray(plane13 if plane13 is not None else np.zeros((0, 13)), np.float64).reshape(-1, 13)
        n = np.ascontiguousarray(pnorm7 if pnorm7 is not None else np.zeros((0, 7)), np.float64).reshape(-1, 7)
        self._fb_rows = 3 * len(e) + len(p) + len(n)
        self._ck(self.lib.ll_factor_blocks_set(self.h, len(e), _ptr(e), len(p), _ptr(p), len(n), _ptr(n)))

    def factor_blocks_set_s(self, edge_s=None, plane_s=None):
        """the functors' s_ of every edge / plane block (DISTORTION 1); None = all ones"""
        e = None if edge_s is None else np.ascontiguousarray(edge_s, np.float64)
        p = None if plane_s is None else np.ascontiguousarray(plane_s, np.float64)
        self._ck(self.lib.ll_factor_blocks_set_s(self.h, _ptr(e), _ptr(p)))

    def factor_blocks_evaluate(self, q, t):
        q = np.ascontiguousarray(q, np.float64); t = np.ascontiguousarray(t, np.float64)
        rows = self._fb_rows
        r = np.zeros(max(rows, 1)); Jq = np.zeros((max(rows, 1), 4)); Jt = np.zeros((max(rows, 1), 3))
        self._ck(self.lib.ll_factor_blocks_evaluate(self.h, _ptr(q), _ptr(t), _ptr(r), _ptr(Jq), _ptr(Jt), len(r)))
        return r[:rows], Jq[:rows], Jt[:rows]

    def exact_math(self, op, a, b=None, c=None):
        """the DEVICE's bit-exact libm restatements over float32 arrays (ll_debug_exact_math); ops 5 / 6 return int32 ring ids"""
        a = np.ascontiguousarray(a, np.float32)
        b = None if b is None else np.ascontiguousarray(b, np.float32)
        c = None if c is None else np.ascontiguousarray(c, np.float32)
        out = np.zeros(len(a), np.int32 if op >= 5 else np.float32)
        self._ck(self.lib.ll_debug_exact_math(self.h, int(op), _ptr(a), _ptr(b), _ptr(c), len(a), _ptr(out)))
        return out

    def debug_sort_pairs(self, keys, vals, seg_off=None):
        """the stable (u64 key, i32 value) pair sort on its own (ll_debug_sort_pairs): over all pairs, or over every
        segment [seg_off[s], seg_off[s + 1]) separately -> (sorted keys, values carried along)"""
        k = np.array(keys, np.uint64).ravel(); v = np.array(vals, np.int32).ravel()       # copies: the call sorts in place
        assert len(k) == len(v)
        so = None if seg_off is None else np.ascontiguousarray(seg_off, np.int32)
        self._ck(self.lib.ll_debug_sort_pairs(self.h, _ptr(k), _ptr(v), len(k), _ptr(so), 0 if so is None else len(so) - 1))
        return k, v

    def debug_exscan(self, data):
        """the device's exclusive prefix sum of an int32 array (ll_debug_exscan)"""
        d = np.array(data, np.int32).ravel()
        self._ck(self.lib.ll_debug_exscan(self.h, _ptr(d), len(d)))
        return d

    def debug_voxel_segments(self, points, seg_off, leaf, max_seg_len=0, cap=None):
        """pcl::VoxelGrid of the clouds [seg_off[s], seg_off[s + 1]) of `points` in one call (ll_debug_voxel_segments) ->
        (filtered clouds back to back, points per filtered cloud).  On LL_ERR_CAPACITY the error carries n_out."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        so = np.ascontiguousarray(seg_off, np.int32)
        cap = len(pts) if cap is None else int(cap)
        out = np.zeros((max(cap, 1), 4), np.float32); cnt = np.zeros(max(len(so) - 1, 1), np.int32); n = C.c_int(0)
        rc = self.lib.ll_debug_voxel_segments(self.h, _ptr(pts), len(pts), _ptr(so), len(so) - 1, C.c_float(leaf), int(max_seg_len),
                                              _ptr(out), cap, _ptr(cnt), C.byref(n))
        if rc != LL_OK:
            err = LightLoamError(rc, self.lib.ll_last_error(self.h).decode())
            err.n_out = n.value
            raise err
        return out[:n.value].copy(), cnt[:len(so) - 1].copy()

    def posegraphs(self, max_graphs, max_nodes_total, max_edges_total):
        """a PoseGraphs solver on this context for calls of at most these totals (ll_posegraphs_create)"""
        return PoseGraphs(self, max_graphs, max_nodes_total, max_edges_total)

    def places(self, capacity, max_radius=None, z_offset=None):
        """a Places database of `capacity` Scan Context descriptors on this context (ll_places_create)"""
        return Places(self, capacity, max_radius, z_offset)

    def keyframes(self, max_frames, cap_corner, cap_surf):
        """a Keyframes store on this context: up to max_frames frames, cap_corner / cap_surf points per cloud type (ll_keyframes_create)"""
        return Keyframes(self, max_frames, cap_corner, cap_surf)

    def visibility(self, kf, **params):
        """a Visibility object over the Keyframes store kf (ll_visibility_create); params: fields of visibility_params()"""
        return Visibility(self, kf, **params)

    def bev(self, kf, **params):
        """a Bev object over the Keyframes store kf (ll_bev_create); params: fields of bev_params()"""
        return Bev(self, kf, **params)

    def entropy(self, kf, **params):
        """an Entropy object over the Keyframes store kf (ll_entropy_create); params: fields of entropy_params()"""
        return Entropy(self, kf, **params)

    def pcm(self, max_graphs, max_nodes_total, max_candidates_total):
        """a Pcm object on this context (ll_pcm_create): pairwise-consistent sets of loop-closure candidates"""
        return Pcm(self, max_graphs, max_nodes_total, max_candidates_total)

    def algorithmic_bytes(self, first=0, count=1):
        b = [C.c_double(0) for _ in range(4)]
        self._ck(self.lib.ll_algorithmic_bytes(self.h, first, count, *[C.byref(x) for x in b]))
        return dict(ext=b[0].value, assoc=b[1].value, vote=b[2].value, rj=b[3].value)


class Map(_Handle):
    """One ll_map: laserMapping's scan-to-submap optimisation (laserMapping.cpp:1822-2095) on the device of `ctx`."""
    _DESTROY, _ERROR = "ll_map_destroy", "ll_map_last_error"

    def __init__(self, ctx, max_map_corner, max_map_surf, max_scan_corner, max_scan_surf, _borrowed=None):
        self.ctx = ctx; self.lib = ctx.lib
        self.lib.ll_map_last_error.restype = C.c_char_p
        self.lib.ll_map_last_error.argtypes = [C.c_void_p]
        self.lib.ll_map_destroy.argtypes = [C.c_void_p]
        self._owned = _borrowed is None
        if _borrowed is not None:                      # the inner map of a CubeMap: the cube map destroys it
            self.h = _borrowed
            return
        self.h = C.c_void_p()
        rc = self.lib.ll_map_create(ctx.h, int(max_map_corner), int(max_map_surf), int(max_scan_corner), int(max_scan_surf), C.byref(self.h))
        if rc != LL_OK:
            raise LightLoamError(rc, ctx.lib.ll_last_error(ctx.h).decode())
        ctx._children.add(self)

    def close(self):
        if getattr(self, "h", None) and not self._owned:
            self.h = None
        super().close()

    @staticmethod
    def _pts(a):
        a = np.ascontiguousarray(a, np.float32)
        assert a.ndim == 2 and a.shape[1] == 4
        return a

    def set_map(self, corner_from_map, surf_from_map):
        c, s_ = self._pts(corner_from_map), self._pts(surf_from_map)
        self._ck(self.lib.ll_map_set_map(self.h, _ptr(c), len(c), _ptr(s_), len(s_)))

    def set_scan(self, corner_stack, surf_stack):
        c, s_ = self._pts(corner_stack), self._pts(surf_stack)
        self._n_stack = (len(c), len(s_))
        self._ck(self.lib.ll_map_set_scan(self.h, _ptr(c), len(c), _ptr(s_), len(s_)))

    def associate(self, pose_w=None):
        p = None if pose_w is None else np.ascontiguousarray(pose_w, np.float64)
        self._ck(self.lib.ll_map_associate(self.h, _ptr(p)))

    def counts(self):
        ne, npl = C.c_int(0), C.c_int(0)
        self._ck(self.lib.ll_map_get_counts(self.h, C.byref(ne), C.byref(npl)))
        return ne.value, npl.value

    def map_sizes(self):
        """(laserCloudCornerFromMap, laserCloudSurfFromMap) sizes: what laserMapping.cpp:1822 tests before it optimises."""
        nc, ns = C.c_int(0), C.c_int(0)
        self._ck(self.lib.ll_map_get_map_sizes(self.h, C.byref(nc), C.byref(ns)))
        return nc.value, ns.value

    def edges(self):
        ne, _ = self.counts()
        src = np.zeros(max(ne, 1), np.int32); a = np.zeros((max(ne, 1), 3)); b = np.zeros((max(ne, 1), 3))
        self._ck(self.lib.ll_map_download_edges(self.h, _ptr(src), _ptr(a), _ptr(b), len(src)))
        return src[:ne], a[:ne], b[:ne]

    def planes(self):
        _, npl = self.counts()
        src = np.zeros(max(npl, 1), np.int32); n = np.zeros((max(npl, 1), 3)); d = np.zeros(max(npl, 1))
        self._ck(self.lib.ll_map_download_planes(self.h, _ptr(src), _ptr(n), _ptr(d), len(src)))
        return src[:npl], n[:npl], d[:npl]

    def normal_equations(self, pose_w=None):
        p = None if pose_w is None else np.ascontiguousarray(pose_w, np.float64)
        H = np.zeros((6, 6)); g = np.zeros(6); cost = C.c_double(0)
        self._ck(self.lib.ll_map_normal_equations(self.h, _ptr(p), _ptr(H), _ptr(g), C.byref(cost)))
        return H, g, cost.value

    def residual_jacobian(self, pose_w=None):
        ne, npl = self.counts()
        rows = 3 * ne + npl
        p = None if pose_w is None else np.ascontiguousarray(pose_w, np.float64)
        r = np.zeros(max(rows, 1)); Jq = np.zeros((max(rows, 1), 4)); Jt = np.zeros((max(rows, 1), 3))
        self._ck(self.lib.ll_map_residual_jacobian(self.h, _ptr(p), _ptr(r), _ptr(Jq), _ptr(Jt), len(r)))
        return r[:rows], Jq[:rows], Jt[:rows]

    def set_vote(self, on):
        """the graph-based correspondence vote on the plane blocks (ll_map_set_vote, laserMapping.cpp:836-1030): associate / optimize
        then keep the selected blocks only, in stack order; off (the default) changes nothing by a bit"""
        self._ck(self.lib.ll_map_set_vote(self.h, int(bool(on))))

    def download_vote(self):
        """the candidates of the last voted association, in stack order (ll_map_download_vote) ->
        (stack index int32[n], count int32[n], selected bool[n], tgt float32[n, 3])"""
        n = C.c_int(0)
        cap = max(getattr(self, "_n_stack", (0, 0))[1], 1)
        while True:
            src = np.zeros(cap, np.int32); cnt = np.zeros(cap, np.int32); sel = np.zeros(cap, np.uint8); tgt = np.zeros((cap, 3), np.float32)
            rc = self.lib.ll_map_download_vote(self.h, _ptr(src), _ptr(cnt), _ptr(sel), _ptr(tgt), cap, C.byref(n))
            if rc == -4 and cap < (1 << 24):
                cap *= 4
                continue
            self._ck(rc)
            k = n.value
            return src[:k], cnt[:k], sel[:k].astype(bool), tgt[:k]

    def optimize(self, pose_w, n_outer=2, opt=None):
        p = np.ascontiguousarray(pose_w, np.float64).copy()
        ran = C.c_int(0)
        self._ck(self.lib.ll_map_optimize(self.h, _ptr(p), n_outer, None if opt is None else C.byref(opt), C.byref(ran)))
        return p, bool(ran.value)

    # ---- tile-parallel search: this map holds a shard of the cubes, the candidates are all-gathered
    def set_map_ids(self, corner_gid, surf_gid):
        c = None if corner_gid is None else np.ascontiguousarray(corner_gid, np.int32)
        s_ = None if surf_gid is None else np.ascontiguousarray(surf_gid, np.int32)
        self._ck(self.lib.ll_map_set_map_ids(self.h, _ptr(c), _ptr(s_)))

    def knn_partial(self, pose_w=None, n_stack=None):
        """-> corner_nn [n, 5, 4] f32 (x, y, z, d2), corner_id [n, 5] i32, surf_nn, surf_id of this rank's points."""
        nc, ns = n_stack if n_stack is not None else self._n_stack
        p = None if pose_w is None else np.ascontiguousarray(pose_w, np.float64)
        cn = np.zeros((nc, 5, 4), np.float32); ci = np.zeros((nc, 5), np.int32)
        sn = np.zeros((ns, 5, 4), np.float32); si = np.zeros((ns, 5), np.int32)
        self._ck(self.lib.ll_map_knn_partial(self.h, _ptr(p), _ptr(cn), _ptr(ci), _ptr(sn), _ptr(si)))
        return cn, ci, sn, si

    def associate_merged(self, corner_nn, corner_id, surf_nn, surf_id, pose_w=None):
        """The candidates of all parts, arrays [parts, n, 5(, 4)] -> the residual blocks of the whole map."""
        cn = np.ascontiguousarray(corner_nn, np.float32); ci = np.ascontiguousarray(corner_id, np.int32)
        sn = np.ascontiguousarray(surf_nn, np.float32); si = np.ascontiguousarray(surf_id, np.int32)
        assert cn.ndim == 4 and sn.ndim == 4 and cn.shape[0] == sn.shape[0] == ci.shape[0] == si.shape[0]
        p = None if pose_w is None else np.ascontiguousarray(pose_w, np.float64)
        self._ck(self.lib.ll_map_associate_merged(self.h, _ptr(p), int(cn.shape[0]), _ptr(cn), _ptr(ci), _ptr(sn), _ptr(si)))

    def set_row_shard(self, rank, world):
        """evaluate() / normal_equations() sum the residual blocks i with i % world == rank ((0, 1): all of them)."""
        self._ck(self.lib.ll_map_set_row_shard(self.h, int(rank), int(world)))

    def solve(self, pose_w, opt=None):
        p = np.ascontiguousarray(pose_w, np.float64).copy()
        self._ck(self.lib.ll_map_solve(self.h, _ptr(p), None if opt is None else C.byref(opt)))
        return p

    # ---- row-parallel stepping: the caller sums `evaluate()` over ranks between the LM stages
    def set_pose(self, pose_w):
        p = np.ascontiguousarray(pose_w, np.float64)
        self._ck(self.lib.ll_map_set_pose(self.h, _ptr(p)))

    def pose(self):
        p = np.zeros(7)
        self._ck(self.lib.ll_map_get_pose(self.h, _ptr(p)))
        return p

    def evaluate(self):
        v = np.zeros(44)
        self._ck(self.lib.ll_map_evaluate(self.h, _ptr(v)))
        return v

    def lm_begin(self, neq44, opt=None):
        v = np.ascontiguousarray(neq44, np.float64)
        self._ck(self.lib.ll_map_lm_begin(self.h, _ptr(v), None if opt is None else C.byref(opt)))

    def lm_propose(self, opt=None):
        self._ck(self.lib.ll_map_lm_propose(self.h, None if opt is None else C.byref(opt)))

    def lm_accept(self, neq44, opt=None):
        v = np.ascontiguousarray(neq44, np.float64)
        self._ck(self.lib.ll_map_lm_accept(self.h, _ptr(v), None if opt is None else C.byref(opt)))

    # ---- device-resident variants: raw DEVICE pointers (ints), enqueue only -- for RCCL collectives on ll_stream(ctx)
    def evaluate_dev(self, neq44_ptr):
        self._ck(self.lib.ll_map_evaluate_dev(self.h, C.c_void_p(neq44_ptr)))

    def lm_begin_dev(self, neq44_ptr, opt=None):
        self._ck(self.lib.ll_map_lm_begin_dev(self.h, C.c_void_p(neq44_ptr), None if opt is None else C.byref(opt)))

    def lm_propose_dev(self, opt=None):
        self._ck(self.lib.ll_map_lm_propose_dev(self.h, None if opt is None else C.byref(opt)))

    def lm_accept_dev(self, neq44_ptr, opt=None):
        self._ck(self.lib.ll_map_lm_accept_dev(self.h, C.c_void_p(neq44_ptr), None if opt is None else C.byref(opt)))

    def knn_partial_dev(self, cn_ptr, ci_ptr, sn_ptr, si_ptr):
        self._ck(self.lib.ll_map_knn_partial_dev(self.h, C.c_void_p(cn_ptr), C.c_void_p(ci_ptr), C.c_void_p(sn_ptr), C.c_void_p(si_ptr)))

    def associate_merged_dev(self, n_parts, cn_ptr, ci_ptr, sn_ptr, si_ptr):
        self._ck(self.lib.ll_map_associate_merged_dev(self.h, int(n_parts), C.c_void_p(cn_ptr), C.c_void_p(ci_ptr), C.c_void_p(sn_ptr), C.c_void_p(si_ptr)))

    def solve_dev(self, opt=None):
        self._ck(self.lib.ll_map_solve_dev(self.h, None if opt is None else C.byref(opt)))


def map_vote_host(ctx, src, tgt):
    """laserMapping's graph_based_correspondence_vote_simple (:836-1030) on caller-supplied correspondences through k_map_vote
    (ll_map_vote_host): src / tgt (n, 4) float32 -> (count int32[n], selected bool[n])"""
    s = np.ascontiguousarray(src, np.float32).reshape(-1, 4); t = np.ascontiguousarray(tgt, np.float32).reshape(-1, 4)
    assert len(s) == len(t)
    n = len(s)
    cnt = np.zeros(max(n, 1), np.int32); sel = np.zeros(max(n, 1), np.uint8)
    ctx._ck(ctx.lib.ll_map_vote_host(ctx.h, _ptr(s), _ptr(t), n, _ptr(cnt), _ptr(sel)))
    return cnt[:n], sel[:n].astype(bool)


class CubeMap(_Handle):
    """One ll_cubemap: laserMapping's cube map + per-frame body (laserMapping.cpp:1584-2165) on the device of `ctx`."""
    _DESTROY, _ERROR = "ll_cubemap_destroy", "ll_cubemap_last_error"

    def __init__(self, ctx, max_scan_corner, max_scan_surf, pool_points=1 << 20, line_res=0.4, plane_res=0.8):
        self.ctx = ctx; self.lib = ctx.lib
        self.lib.ll_cubemap_last_error.restype = C.c_char_p
        self.lib.ll_cubemap_last_error.argtypes = [C.c_void_p]
        self.lib.ll_cubemap_destroy.argtypes = [C.c_void_p]
        self.h = C.c_void_p()
        rc = self.lib.ll_cubemap_create(ctx.h, C.c_float(line_res), C.c_float(plane_res), int(max_scan_corner), int(max_scan_surf),
                                        int(pool_points), C.byref(self.h))
        if rc != LL_OK:
            raise LightLoamError(rc, ctx.lib.ll_last_error(ctx.h).decode())
        ctx._children.add(self)

    def set_shard(self, rank, world):
        """Keep only the cubes of `rank` out of `world` (tile-parallel mapping); before the first scan."""
        self._ck(self.lib.ll_cubemap_set_shard(self.h, int(rank), int(world)))

    def set_vote(self, on):
        """vote the plane blocks in optimize / process* (ll_cubemap_set_vote: the inner map's Map.set_vote)"""
        self._ck(self.lib.ll_cubemap_set_vote(self.h, int(bool(on))))

    def map(self):
        """The inner Map (borrowed): knn_partial / associate_merged / solve / edges / planes on the gathered clouds."""
        self.lib.ll_cubemap_map.restype = C.c_void_p
        self.lib.ll_cubemap_map.argtypes = [C.c_void_p]
        return Map(self.ctx, 0, 0, 0, 0, _borrowed=C.c_void_p(self.lib.ll_cubemap_map(self.h)))

    def prepare(self, t_w, corner_last, surf_last):
        t = np.ascontiguousarray(t_w, np.float64)
        c = np.ascontiguousarray(corner_last, np.float32); s_ = np.ascontiguousarray(surf_last, np.float32)
        self._ck(self.lib.ll_cubemap_prepare(self.h, _ptr(t), _ptr(c), len(c), _ptr(s_), len(s_)))

    def optimize(self, pose_w, n_outer=2, opt=None):
        p = np.ascontiguousarray(pose_w, np.float64).copy(); ran = C.c_int(0)
        self._ck(self.lib.ll_cubemap_optimize(self.h, _ptr(p), n_outer, None if opt is None else C.byref(opt), C.byref(ran)))
        return p, bool(ran.value)

    def update(self, pose_w):
        p = np.ascontiguousarray(pose_w, np.float64)
        self._ck(self.lib.ll_cubemap_update(self.h, _ptr(p)))

    def process(self, pose_w, corner_last, surf_last):
        p = np.ascontiguousarray(pose_w, np.float64).copy(); ran = C.c_int(0)
        c = np.ascontiguousarray(corner_last, np.float32); s_ = np.ascontiguousarray(surf_last, np.float32)
        self._ck(self.lib.ll_cubemap_process(self.h, _ptr(p), _ptr(c), len(c), _ptr(s_), len(s_), C.byref(ran)))
        return p, bool(ran.value)

    def process_slot(self, pose_w, slot):
        p = np.ascontiguousarray(pose_w, np.float64).copy(); ran = C.c_int(0)
        self._ck(self.lib.ll_cubemap_process_slot(self.h, _ptr(p), int(slot), C.byref(ran)))
        return p, bool(ran.value)

    def info(self):
        cen = (C.c_int * 3)(); cnt = (C.c_int * 4)()
        self._ck(self.lib.ll_cubemap_info(self.h, cen, cnt))
        return tuple(cen), tuple(cnt)

    def cloud(self, which):
        _, cnt = self.info()
        out = np.zeros((max(cnt[which], 1), 4), np.float32); n = C.c_int(0)
        self._ck(self.lib.ll_cubemap_download_cloud(self.h, which, _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def cube(self, surf, index, cap=1 << 18):
        out = np.zeros((cap, 4), np.float32); n = C.c_int(0)
        self._ck(self.lib.ll_cubemap_download_cube(self.h, int(surf), int(index), _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def export(self, which):
        """laserCloudSurround (MAP_SURROUND) or laserCloudMap (MAP_ALL) of this map: (n, 4) float32, per cube corner then surf;
        one gather, one copy, one synchronisation"""
        n = C.c_longlong(0); out = np.zeros((1, 4), np.float32)
        rc = self.lib.ll_cubemap_export(self.h, int(which), out.ctypes.data, 0, C.byref(n))   # the size: nothing is launched
        if rc not in (LL_OK, -4):
            self._ck(rc)
        if n.value > 0:
            out = np.empty((n.value, 4), np.float32)
            self._ck(self.lib.ll_cubemap_export(self.h, int(which), out.ctypes.data, len(out), C.byref(n)))
        return out[:n.value]


    def layout(self):
        """(cen (3,), counts [2, 4851] int32, valid [n_valid] int32): with export(MAP_ALL) the complete state of the map"""
        cen = np.zeros(3, np.int32); counts = np.zeros((2, N_CUBES), np.int32); valid = np.zeros(125, np.int32); n = C.c_int(0)
        self._ck(self.lib.ll_cubemap_layout(self.h, cen.ctypes.data, counts.ctypes.data, valid.ctypes.data, C.addressof(n)))
        return cen, counts, valid[:n.value].copy()

    def import_map(self, points, layout):
        """replace the map by an export(MAP_ALL) cloud and its layout (cen, counts, valid): one upload, one scatter, one synchronisation"""
        cen, counts, valid = layout
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        cen = np.ascontiguousarray(cen, np.int32); counts = np.ascontiguousarray(counts, np.int32); valid = np.ascontiguousarray(valid, np.int32)
        if cen.shape != (3,) or counts.shape != (2, N_CUBES) or len(valid) > 125:
            raise ValueError("layout must be (cen [3], counts [2, 4851], valid [<= 125])")
        v = np.zeros(125, np.int32); v[:len(valid)] = valid
        self._ck(self.lib.ll_cubemap_import(self.h, pts.ctypes.data, len(pts), cen.ctypes.data, counts.ctypes.data, v.ctypes.data, len(valid)))


class CubeMaps(_Handle):
    """One ll_cubemaps: n_seq cube maps side by side, frame k of every running sequence in one set of launches per stage.
    Sequence q equals a CubeMap with the same parameters driven by process_slot / process with the same frames, bit for bit."""
    _DESTROY, _ERROR = "ll_cubemaps_destroy", "ll_cubemaps_last_error"

    def __init__(self, ctx, n_seq, max_scan_corner, max_scan_surf, pool_points=1 << 20, line_res=0.4, plane_res=0.8):
        self.ctx = ctx; self.lib = ctx.lib; self.n_seq = int(n_seq)
        self.lib.ll_cubemaps_last_error.restype = C.c_char_p
        self.lib.ll_cubemaps_last_error.argtypes = [C.c_void_p]
        self.lib.ll_cubemaps_destroy.argtypes = [C.c_void_p]
        self.h = C.c_void_p()
        rc = self.lib.ll_cubemaps_create(ctx.h, int(n_seq), C.c_float(line_res), C.c_float(plane_res), int(max_scan_corner),
                                         int(max_scan_surf), int(pool_points), C.byref(self.h))
        if rc != LL_OK:
            raise LightLoamError(rc, ctx.lib.ll_last_error(ctx.h).decode())
        ctx._children.add(self)

    def _poses(self, pose_w):
        p = np.ascontiguousarray(pose_w, np.float64).reshape(self.n_seq, 7).copy()
        return p, np.zeros(self.n_seq, np.int32)

    def process_slots(self, pose_w, slots):
        """pose_w [S, 7], slots [S] (-1: the sequence does not run) -> (poses [S, 7], ran [S] bool)"""
        p, ran = self._poses(pose_w)
        s = np.ascontiguousarray(slots, np.int32)
        if s.shape != (self.n_seq,):
            raise ValueError("slots must have one entry per sequence")
        self._ck(self.lib.ll_cubemaps_process_slots(self.h, _ptr(s), _ptr(p), _ptr(ran)))
        return p, ran.astype(bool)

    def localize_slots(self, pose_w, slots, map_of=None, fit=True, info=False):
        """A read-only frame: sequence q localises the extracted slot slots[q] (-1: it sits out) against map map_of[q] (None: its
        own) from the guess pose_w[q]; no map changes -> (poses [S, 7], ran [S] bool, fit: a LocalizeFit array [S], or None with
        fit=False -- then the extra association pass and the reduction are not launched).  info=True appends a PoseInfo array [S]:
        the information of every solve at its final pose (edge_from_info turns a record into a pose-graph edge's weight)"""
        p, ran = self._poses(pose_w)
        s = np.ascontiguousarray(slots, np.int32)
        if s.shape != (self.n_seq,):
            raise ValueError("slots must have one entry per sequence")
        m = None if map_of is None else np.ascontiguousarray(map_of, np.int32)
        if m is not None and m.shape != (self.n_seq,):
            raise ValueError("map_of must have one entry per sequence")
        rec = (LocalizeFit * self.n_seq)() if fit else None
        if info:
            return self._localize_slots_info(s, m, p, ran, rec)
        self._ck(self.lib.ll_cubemaps_localize_slots(self.h, s.ctypes.data, None if m is None else m.ctypes.data, p.ctypes.data,
                                                     ran.ctypes.data, C.addressof(rec) if fit else None))
        return p, ran.astype(bool), rec

    def _localize_slots_info(self, s, m, p, ran, rec):
        inf = (PoseInfo * self.n_seq)()
        self._ck(self.lib.ll_cubemaps_localize_slots_info(self.h, s.ctypes.data, None if m is None else m.ctypes.data, p.ctypes.data,
                                                          ran.ctypes.data, None if rec is None else C.addressof(rec), C.addressof(inf)))
        return p, ran.astype(bool), rec, inf

    def process(self, pose_w, corners, surfs):
        """corners / surfs: one (n, 4) float32 cloud per sequence, None for a sequence that does not run"""
        p, ran = self._poses(pose_w)
        keep = []
        cp = (C.c_void_p * self.n_seq)(); sp = (C.c_void_p * self.n_seq)()
        nc = np.zeros(self.n_seq, np.int32); ns = np.zeros(self.n_seq, np.int32)
        for q in range(self.n_seq):
            if corners[q] is None and surfs[q] is None:
                continue
            c = np.ascontiguousarray(np.zeros((0, 4)) if corners[q] is None else corners[q], np.float32).reshape(-1, 4)
            s_ = np.ascontiguousarray(np.zeros((0, 4)) if surfs[q] is None else surfs[q], np.float32).reshape(-1, 4)
            keep += [c, s_]
            cp[q] = c.ctypes.data if c.size else C.addressof(_EMPTY)
            sp[q] = s_.ctypes.data if s_.size else C.addressof(_EMPTY)
            nc[q] = len(c); ns[q] = len(s_)
        self._ck(self.lib.ll_cubemaps_process(self.h, cp, _ptr(nc), sp, _ptr(ns), _ptr(p), _ptr(ran)))
        return p, ran.astype(bool)

    def info(self, q):
        cen = (C.c_int * 3)(); cnt = (C.c_int * 4)()
        self._ck(self.lib.ll_cubemaps_info(self.h, int(q), cen, cnt))
        return tuple(cen), tuple(cnt)

    def cloud(self, q, which):
        _, cnt = self.info(q)
        out = np.zeros((max(cnt[which], 1), 4), np.float32); n = C.c_int(0)
        self._ck(self.lib.ll_cubemaps_download_cloud(self.h, int(q), which, _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def cube(self, q, surf, index, cap=1 << 18):
        out = np.zeros((cap, 4), np.float32); n = C.c_int(0)
        self._ck(self.lib.ll_cubemaps_download_cube(self.h, int(q), int(surf), int(index), _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def _which(self, which):
        w = np.full(self.n_seq, which, np.int32) if np.ndim(which) == 0 else np.ascontiguousarray(which, np.int32)
        if w.shape != (self.n_seq,):
            raise ValueError("which must be one value or one per sequence")
        return w

    def export_sizes(self, which):
        """offset [S + 1] int64 of export(which): host bookkeeping, no launch, no synchronisation"""
        w = self._which(which)
        off = np.zeros(self.n_seq + 1, np.int64)
        self._ck(self.lib.ll_cubemaps_export_sizes(self.h, w.ctypes.data, off.ctypes.data))
        return off

    def export(self, which, out=None):
        """which: MAP_NONE / MAP_SURROUND / MAP_ALL, one for all sequences or one per sequence -> (points [N, 4] float32,
        offset [S + 1] int64); sequence q is points[offset[q]:offset[q + 1]], per cube corner then surf.  One gather, one copy,
        one synchronisation.  out: a preallocated (n, 4) float32 array to fill instead (page-locked memory copies faster)"""
        w = self._which(which)
        off = self.export_sizes(w)
        n = int(off[-1])
        if out is None:
            out = np.empty((max(n, 1), 4), np.float32)
        if out.dtype != np.float32 or not out.flags.c_contiguous or out.size < 4 * n:
            raise ValueError("out must be a C-contiguous float32 array of at least N x 4")
        self._ck(self.lib.ll_cubemaps_export(self.h, w.ctypes.data, out.ctypes.data, out.size // 4, off.ctypes.data))
        return out.reshape(-1, 4)[:n], off

    def export_timing(self):
        """the last export: ((table build ms, gather ms, copy ms), (points, segments, tiles))"""
        return self._timing(self.lib.ll_cubemaps_export_timing, 3, 3)

    def layout(self, q):
        """(cen (3,), counts [2, 4851] int32, valid [n_valid] int32) of map q: host bookkeeping, no launch, no synchronisation.
        With export(MAP_ALL) the complete state of the map"""
        cen = np.zeros(3, np.int32); counts = np.zeros((2, N_CUBES), np.int32); valid = np.zeros(125, np.int32); n = C.c_int(0)
        self._ck(self.lib.ll_cubemaps_layout(self.h, int(q), cen.ctypes.data, counts.ctypes.data, valid.ctypes.data, C.addressof(n)))
        return cen, counts, valid[:n.value].copy()

    def import_maps(self, points, offset, layouts, device_ptr=None):
        """put maps back: points [N, 4] float32 in the layout export(MAP_ALL) writes, offset [S + 1], layouts: per sequence
        None (the map is left alone) or (cen, counts, valid) as layout() gives it.  One upload, one scatter kernel, one
        synchronisation.  device_ptr: the address of the same cloud in device memory (points is then not read)"""
        S = self.n_seq
        if len(layouts) != S:
            raise ValueError("layouts must have one entry per sequence")
        off = np.ascontiguousarray(offset, np.int64)
        if off.shape != (S + 1,):
            raise ValueError("offset must have S + 1 entries")
        sel = np.zeros(S, np.int32); cen = np.zeros((S, 3), np.int32); counts = np.zeros((S, 2, N_CUBES), np.int32)
        valid = np.zeros((S, 125), np.int32); nv = np.zeros(S, np.int32)
        for q, lay in enumerate(layouts):
            if lay is None:
                continue
            c, k, v = lay
            sel[q] = 1; cen[q] = c; counts[q] = k; nv[q] = len(v); valid[q, :len(v)] = v
        if device_ptr is None:
            pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
            if len(pts) < int(off[-1]):
                raise ValueError("points is shorter than offset[S]")
            ptr = pts.ctypes.data
        else:
            ptr = int(device_ptr)
        self._ck(self.lib.ll_cubemaps_import(self.h, sel.ctypes.data, ptr, off.ctypes.data, cen.ctypes.data, counts.ctypes.data,
                                             valid.ctypes.data, nv.ctypes.data))

    def merge(self, ops):
        """ops: a list of (dst, src, pose_w7) -- map src, taken through pointAssociateToMap with the pose, is binned into map dst and
        every cube that received a point is voxel-filtered -> (added [n_ops, 2], dropped [n_ops, 2]) int64: per op and cloud type
        the points that entered a cube (before the filter) and those that fell outside the cube array.  Everything on the device;
        three synchronisations whatever len(ops) is, plus the voxel filter's read-back above 65 536 points"""
        rec = (MergeOp * max(len(ops), 1))()
        for i, (dst, src, pose) in enumerate(ops):
            p = np.ascontiguousarray(pose, np.float64).reshape(7)
            rec[i].dst = int(dst); rec[i].src = int(src)
            for k in range(7):
                rec[i].T_w7[k] = p[k]
        added = np.zeros((len(ops), 2), np.int64); dropped = np.zeros((len(ops), 2), np.int64)
        self._ck(self.lib.ll_cubemaps_merge(self.h, C.addressof(rec), len(ops), added.ctypes.data, dropped.ctypes.data))
        return added, dropped

    def merge_timing(self):
        """the last merge: ((assign ms, sort + gather ms, filter ms, commit ms), (points in, touched cubes, points out))"""
        return self._timing(self.lib.ll_cubemaps_merge_timing, 4, 3)

    def insert_keyframes(self, kf, ops, visibility=None, rule=None):
        """ops: a list of (dst, frames, poses, reset, cen) -- the frames (ids of the Keyframes store kf, in this order; they may repeat)
        go into map dst, frame k under poses[k] ([n, 7]; None: the poses the store holds); reset: dst is first emptied and given the
        centre cen (ignored without reset; None: (10, 10, 5)).  Every cube that received a point is voxel-filtered ONCE over its old
        cloud and all new points (the merge's semantics, not frame-by-frame mapping) -> (added [n_ops, 2], dropped [n_ops, 2]) int64.
        Everything on the device; three synchronisations whatever len(ops) and the number of frames are.
        visibility: a Visibility object of kf -- the points its counters and rule ((min_through, max_hit); None: (2, 255)) remove are
        left out (ll_cubemaps_insert_keyframes_filtered) -> (added, dropped, removed [n_ops, 2])"""
        rec = (InsertOp * max(len(ops), 1))()
        keep = []
        for i, (dst, frames, poses, reset, cen) in enumerate(ops):
            f, p = _frame_list(frames, poses)
            keep += [f, p]
            rec[i].dst = int(dst); rec[i].n_frames = len(f); rec[i].frames = f.ctypes.data
            rec[i].poses_w7 = None if p is None else p.ctypes.data
            rec[i].reset = int(reset)
            for k, v in enumerate((10, 10, 5) if cen is None else cen):
                rec[i].cen[k] = int(v)
        added = np.zeros((len(ops), 2), np.int64); dropped = np.zeros((len(ops), 2), np.int64)
        if visibility is None:
            if rule is not None:
                raise ValueError("a rule needs a Visibility object")
            self._ck(self.lib.ll_cubemaps_insert_keyframes(self.h, kf.h, C.addressof(rec), len(ops), added.ctypes.data, dropped.ctypes.data))
            return added, dropped
        visibility._live()
        r = VisibilityRule(*((2, 255) if rule is None else (int(rule[0]), int(rule[1]))))
        removed = np.zeros((len(ops), 2), np.int64)
        self._ck(self.lib.ll_cubemaps_insert_keyframes_filtered(self.h, kf.h, visibility.h, C.addressof(r), C.addressof(rec), len(ops),
                                                                added.ctypes.data, dropped.ctypes.data, removed.ctypes.data))
        return added, dropped, removed

    def insert_timing(self):
        """the last insert_keyframes: ((assign ms, sort + gather ms, filter ms, commit ms), (points in, touched cubes, points out))"""
        return self._timing(self.lib.ll_cubemaps_insert_timing, 4, 3)

    def align(self, ops, n_outer=2, opt=None, fit=True, info=False):
        """ops: a list of (dst, src, guess_w7) -- the rigid transform that takes map src's world frame into map dst's, by
        laserMapping's scan-to-map optimisation over the whole of both maps from the guess (local registration: the guess must lie
        inside the basin of the 1 m association radius) -> (T [n_ops, 7], ran [n_ops] bool, fit: a LocalizeFit array [n_ops], or
        None with fit=False -- then the extra pass at the final poses is not launched).  n_outer = 0 scores the guess.  No map
        changes; everything on the device; one synchronisation whatever len(ops) and n_outer are.  info=True appends a PoseInfo
        array [n_ops]: the information of every op at its final T"""
        rec = (MergeOp * max(len(ops), 1))()
        for i, (dst, src, pose) in enumerate(ops):
            p = np.ascontiguousarray(pose, np.float64).reshape(7)
            rec[i].dst = int(dst); rec[i].src = int(src)
            for k in range(7):
                rec[i].T_w7[k] = p[k]
        T = np.zeros((len(ops), 7)); ran = np.zeros(len(ops), np.int32)
        out = (LocalizeFit * max(len(ops), 1))() if fit else None
        if info:
            inf = (PoseInfo * max(len(ops), 1))()
            self._ck(self.lib.ll_cubemaps_align_info(self.h, C.addressof(rec), len(ops), int(n_outer), None if opt is None else C.addressof(opt),
                                                     T.ctypes.data, ran.ctypes.data, C.addressof(out) if fit else None, C.addressof(inf)))
            return T, ran.astype(bool), out, inf
        self._ck(self.lib.ll_cubemaps_align(self.h, C.addressof(rec), len(ops), int(n_outer), None if opt is None else C.addressof(opt),
                                            T.ctypes.data, ran.ctypes.data, C.addressof(out) if fit else None))
        return T, ran.astype(bool), out

    def align_timing(self):
        """the last align: ((build ms, search + fit ms, evaluate + solve ms, fit record ms), (stack points, map points, residual blocks))"""
        return self._timing(self.lib.ll_cubemaps_align_timing, 4, 3)

    def stats(self):
        """(host synchronisations, frames) since create"""
        s = C.c_longlong(0); f = C.c_longlong(0)
        self._ck(self.lib.ll_cubemaps_stats(self.h, C.byref(s), C.byref(f)))
        return s.value, f.value

    def set_vote(self, on):
        """on [S] of 0 / 1: the sequences whose plane blocks are voted in process / process_slots from now on (ll_cubemaps_set_vote);
        localize_slots never votes"""
        o = np.ascontiguousarray(on).astype(np.int32)
        if o.shape != (self.n_seq,):
            raise ValueError("on must have one entry per sequence")
        self._ck(self.lib.ll_cubemaps_set_vote(self.h, o.ctypes.data))

    def reset(self, q):
        """sequence q back to a freshly created cube map; the others are untouched"""
        self._ck(self.lib.ll_cubemaps_reset(self.h, int(q)))


class Keyframes(_Handle):
    """One ll_keyframes: the stack clouds (down-sized corner and surf features, sensor frame) and mapped poses of frames, on the device;
    frame ids are 0 .. len(self) - 1 in the order they were added.  CubeMaps.insert_keyframes rebuilds maps from them"""
    _DESTROY, _ERROR = "ll_keyframes_destroy", "ll_keyframes_last_error"

    def __init__(self, ctx, max_frames, cap_corner, cap_surf):
        self.ctx = ctx; self.lib = ctx.lib
        self.params = KeyframesParams(int(max_frames), int(cap_corner), int(cap_surf))
        self.h = C.c_void_p()
        rc = self.lib.ll_keyframes_create(ctx.h, C.byref(self.params), C.byref(self.h))
        if rc != LL_OK:
            raise LightLoamError(rc, ctx.lib.ll_last_error(ctx.h).decode())
        ctx._children.add(self)

    def __len__(self):
        return self.lib.ll_keyframes_size(self.h)

    size = __len__

    def reset(self):
        self._ck(self.lib.ll_keyframes_reset(self.h))

    def info(self, i):
        """frame i: {"lane", "frame_index", "n": (corner, surf), "offset": (corner, surf), "pose": [7]}; host only"""
        e = KeyframeInfo()
        self._ck(self.lib.ll_keyframes_info(self.h, int(i), C.byref(e)))
        return {"lane": e.lane, "frame_index": e.frame_index, "n": tuple(e.n), "offset": tuple(e.offset), "pose": np.array(e.pose_w7[:])}

    def add_cubemaps(self, cms, sel, poses, lane_tag=None, frame_tag=None):
        """one keyframe per sequence with sel[q] = 1 from the stack clouds of its last frame (CubeMaps.cloud(q, 2 / 3)) and poses[q]
        -> the first new id (-1: none selected).  One copy launch, no synchronisation"""
        S = cms.n_seq
        s = np.ascontiguousarray(sel).astype(np.int32)
        if s.shape != (S,):
            raise ValueError("sel must have one entry per sequence")
        p = np.ascontiguousarray(poses, np.float64).reshape(S, 7)
        lt = None if lane_tag is None else np.ascontiguousarray(lane_tag, np.int32).reshape(S)
        ft = None if frame_tag is None else np.ascontiguousarray(frame_tag, np.int32).reshape(S)
        first = C.c_int(-1)
        self._ck(self.lib.ll_keyframes_add_cubemaps(self.h, cms.h, s.ctypes.data, p.ctypes.data, None if lt is None else lt.ctypes.data,
                                                    None if ft is None else ft.ctypes.data, C.addressof(first)))
        return first.value

    def add_points(self, corner, surf, pose):
        """one keyframe from host clouds (n, 4) float32 -> its id"""
        c = np.ascontiguousarray(corner, np.float32).reshape(-1, 4); s = np.ascontiguousarray(surf, np.float32).reshape(-1, 4)
        p = np.ascontiguousarray(pose, np.float64).reshape(7)
        i = C.c_int(-1)
        self._ck(self.lib.ll_keyframes_add_points(self.h, c.ctypes.data if len(c) else None, len(c), s.ctypes.data if len(s) else None, len(s),
                                                  p.ctypes.data, C.addressof(i)))
        return i.value

    def export(self, first=0, count=None):
        """(points [N, 4] float32, offsets [count, 2] + total as int64 [2 count + 1]): frames first .. back to back, per frame the
        corner cloud and then the surf cloud; cloud w of frame first + f is points[offsets[2 f + w]:offsets[2 f + w + 1]].  One gather,
        one copy, one synchronisation"""
        count = len(self) - int(first) if count is None else int(count)
        off = np.zeros(2 * max(count, 0) + 1, np.int64)
        self._ck(self.lib.ll_keyframes_export(self.h, int(first), count, None, off.ctypes.data))
        out = np.zeros((max(int(off[-1]), 1), 4), np.float32)
        self._ck(self.lib.ll_keyframes_export(self.h, int(first), count, out.ctypes.data, off.ctypes.data))
        return out[:int(off[-1])], off


class _StoreReader(_Handle):
    """what the classes over an object that follows one Keyframes store share.  _CREATE: the name of the create function, which
    reports through the store's last error"""
    _CREATE = None

    def _follow(self, ctx, kf, params):
        self.ctx = ctx; self.lib = ctx.lib; self.kf = kf
        self.params = params
        self.h = C.c_void_p()
        rc = getattr(self.lib, self._CREATE)(kf.h, C.byref(self.params), C.byref(self.h))
        if rc != LL_OK:
            raise LightLoamError(rc, self.lib.ll_keyframes_last_error(kf.h).decode())
        ctx._children.add(self)           # destroy reads nothing of the store: the order in which a Context closes its children is free

    def _live(self):
        if not getattr(self, "h", None) or not getattr(self.kf, "h", None):
            raise LightLoamError(-7, "the %s object or its Keyframes store is closed" % type(self).__name__)


def visibility_params(**kw):
    """ll_visibility_default_params with the given fields replaced"""
    return _struct_params(VisibilityParams, load_library().ll_visibility_default_params, kw)


class Visibility(_StoreReader):
    """One ll_visibility over a Keyframes store: per stored point how many other frames of its drive saw THROUGH it and how many HIT
    it (range images of the frames' own clouds, a 3 x 3 minimum, a margin); CubeMaps.insert_keyframes(..., visibility=self) leaves
    the points out that a rule over the two counters removes"""
    _CREATE, _DESTROY, _ERROR = "ll_visibility_create", "ll_visibility_destroy", "ll_visibility_last_error"

    def __init__(self, ctx, kf, **params):
        self._follow(ctx, kf, visibility_params(**params))

    def run(self, ops):
        """ops: a list of (frames, poses) -- the frames of one drive (ids of the store, each at most once per call) observe each other,
        frame k under poses[k] ([n, 7]; None: the stored poses) -> pairs [n_ops] int64, the ordered (subject, observer) frame pairs.
        The listed frames' counters are made anew, the others keep theirs.  Three launches, one synchronisation"""
        self._live()
        rec = (VisibilityOp * max(len(ops), 1))()
        keep = []
        for i, (frames, poses) in enumerate(ops):
            f, p = _frame_list(frames, poses)
            keep += [f, p]
            rec[i].n_frames = len(f); rec[i].frames = f.ctypes.data
            rec[i].poses_w7 = None if p is None else p.ctypes.data
        pairs = np.zeros(max(len(ops), 1), np.int64)
        self._ck(self.lib.ll_visibility_run(self.h, C.addressof(rec), len(ops), pairs.ctypes.data))
        return pairs[:len(ops)]

    def counts(self, frame):
        """(corner [n_corner, 2], surf [n_surf, 2]) uint8: (through, hit) of every point of the frame, each saturating at 255"""
        self._live()
        e = self.kf.info(frame)
        out = np.zeros((max(e["n"][0] + e["n"][1], 1), 2), np.uint8)
        self._ck(self.lib.ll_visibility_counts(self.h, int(frame), out.ctypes.data))
        return out[:e["n"][0]], out[e["n"][0]:e["n"][0] + e["n"][1]]

    def images(self, k):
        """(raw, img) [height, width] float32 of the k-th listed frame, counted across ops, of the last run; +inf: empty"""
        shape = (self.params.height, self.params.width)
        raw = np.zeros(shape, np.float32); img = np.zeros(shape, np.float32)
        self._ck(self.lib.ll_visibility_images(self.h, int(k), raw.ctypes.data, img.ctypes.data))
        return raw, img

    def reset(self):
        """all counters zero; needed after Keyframes.reset before the object is used again"""
        self._live()
        self._ck(self.lib.ll_visibility_reset(self.h))

    def timing(self):
        """the last run: ((images ms, erode ms, vote ms), (listed frames, their points, frame pairs))"""
        return self._timing(self.lib.ll_visibility_timing, 3, 3)


def bev_params(**kw):
    """ll_bev_default_params with the given fields replaced"""
    return _struct_params(BevParams, load_library().ll_bev_default_params, kw)


def bev_guess(Pc, D, Pq):
    """ll_bev_guess: T0 = P_c o D o P_q^-1 [7], the guess of CubeMaps.align((dst = the candidate's map, src = the query's map, T0));
    P_c, P_q: the anchors' poses in their maps, D: BevResult.D_w7.  Host arithmetic: needs no device"""
    a = [np.ascontiguousarray(x, np.float64).reshape(7) for x in (Pc, D, Pq)]
    T = np.zeros(7)
    rc = load_library().ll_bev_guess(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, T.ctypes.data)
    if rc != LL_OK:
        raise LightLoamError(rc, "bev_guess: a NULL pointer")
    return T


class Bev(_StoreReader):
    """One ll_bev over a Keyframes store: correlative matching of bird's-eye occupancy grids, from a place match (the revisited
    frame and a heading good to a sector) to the 3-DoF transform that starts CubeMaps.align or a localising lane"""
    _CREATE, _DESTROY, _ERROR = "ll_bev_create", "ll_bev_destroy", "ll_bev_last_error"

    def __init__(self, ctx, kf, **params):
        self._n_yaws = []
        self._follow(ctx, kf, bev_params(**params))

    def match(self, ops):
        """ops: a list of (target, target_poses, query, query_poses, yaw0, yaw_step, n_yaws) -- frame ids of the store, the first of a
        list is its anchor; poses [n, 7] or None for the stored ones -> a BevResult array [n_ops].  One upload, one fill, three launches,
        one synchronisation whatever len(ops) is"""
        self._live()
        rec = (BevOp * max(len(ops), 1))()
        keep = []
        for i, (target, tposes, query, qposes, yaw0, yaw_step, n_yaws) in enumerate(ops):
            for side, ids, poses in (("target", target, tposes), ("query", query, qposes)):
                f, p = _frame_list(ids, poses)
                keep += [f, p]
                setattr(rec[i], "n_" + side, len(f)); setattr(rec[i], side, f.ctypes.data if len(f) else None)
                setattr(rec[i], side + "_poses_w7", None if p is None else p.ctypes.data)
            rec[i].yaw0 = float(yaw0); rec[i].yaw_step = float(yaw_step); rec[i].n_yaws = int(n_yaws)
        out = (BevResult * max(len(ops), 1))()
        self._ck(self.lib.ll_bev_match(self.h, C.addressof(rec), len(ops), C.addressof(out)))
        self._n_yaws = [int(o[6]) for o in ops]
        return out

    def volume(self, op):
        """the scores [n_yaws, 2 sh, 2 sh] int32 of op `op` of the last match (index: yaw, sy + sh, sx + sh)"""
        self._live()
        S = 2 * self.params.shift_half
        n = self._n_yaws[op] if 0 <= int(op) < len(self._n_yaws) else 1
        out = np.zeros((n, S, S), np.int32)
        self._ck(self.lib.ll_bev_volume(self.h, int(op), out.ctypes.data))
        return out

    def grid(self, op):
        """the target grid [2 half, 2 half] uint8 of op `op` of the last match: bit l of cell (fy + half, fx + half) is layer l"""
        self._live()
        G = 2 * self.params.half
        out = np.zeros((G, G), np.uint8)
        self._ck(self.lib.ll_bev_grid(self.h, int(op), out.ctypes.data))
        return out

    def reset(self):
        """the last match forgotten; needed after Keyframes.reset before the object is used again"""
        self._live()
        self._ck(self.lib.ll_bev_reset(self.h))
        self._n_yaws = []

    def timing(self):
        """the last match: ((prepare ms, score ms, peak ms), (ops, listed points, hypotheses))"""
        return self._timing(self.lib.ll_bev_timing, 3, 3)


def entropy_params(**kw):
    """ll_entropy_default_params with the given fields replaced"""
    return _struct_params(EntropyParams, load_library().ll_entropy_default_params, kw)


class Entropy(_StoreReader):
    """One ll_entropy over a Keyframes store: mean map entropy and mean plane variance of the cloud that listed frames make under
    listed poses, from the covariance of every point's fixed-radius neighbourhood.  It rewards any thinning: compare trajectories over
    the same points only"""
    _CREATE, _DESTROY, _ERROR = "ll_entropy_create", "ll_entropy_destroy", "ll_entropy_last_error"

    def __init__(self, ctx, kf, **params):
        self._sizes = []
        self._follow(ctx, kf, entropy_params(**params))

    def run(self, ops):
        """ops: a list of (frames, poses) -- the cloud of the listed frames (ids of the store, each at most once per op; the same id may
        stand in several ops), frame k under poses[k] ([n, 7]; None: the stored poses) -> a list of EntropyRec, one per op.  Two
        synchronisations, plus the sort's read-back above 65536 points"""
        self._live()
        rec = (EntropyOp * max(len(ops), 1))()
        keep = []; sizes = []
        for i, (frames, poses) in enumerate(ops):
            f, p = _frame_list(frames, poses)
            keep += [f, p]
            rec[i].n_frames = len(f); rec[i].frames = f.ctypes.data
            rec[i].poses_w7 = None if p is None else p.ctypes.data
        out = (EntropyRec * max(len(ops), 1))()
        self._ck(self.lib.ll_entropy_run(self.h, C.addressof(rec), len(ops), C.addressof(out)))
        for i, (frames, _) in enumerate(ops):
            sizes += [self.kf.info(int(f))["n"] for f in np.asarray(frames, np.int64).reshape(-1)]
        self._sizes = sizes
        return [out[i] for i in range(len(ops))]

    def values(self, k):
        """(h, pv, nn) of the k-th listed frame, counted across ops, of the last run: float32, float32, uint16 [n_corner + n_surf],
        corner first; NaN where a point is sparse (nn < min_neighbours) or outside (nn == 0)"""
        self._live()
        n = sum(self._sizes[k]) if 0 <= int(k) < len(self._sizes) else 0
        h = np.zeros(max(n, 1), np.float32); pv = np.zeros(max(n, 1), np.float32); nn = np.zeros(max(n, 1), np.uint16)
        self._ck(self.lib.ll_entropy_values(self.h, int(k), h.ctypes.data, pv.ctypes.data, nn.ctypes.data))
        return h[:n], pv[:n], nn[:n]

    def reset(self):
        """the last run forgotten; needed after Keyframes.reset before the object is used again"""
        self._live()
        self._ck(self.lib.ll_entropy_reset(self.h))
        self._sizes = []

    def timing(self):
        """the last run: ((keys, sort + cells, rows, moments, sums) ms, (listed frames, their points, occupied cells, neighbour pairs,
        host synchronisations))"""
        return self._timing(self.lib.ll_entropy_timing, 5, 5)


PCM_CANDIDATE = np.dtype([("i", "i4"), ("j", "i4"), ("Z_w7", "f8", (7,))])       # ll_pcm_candidate as a numpy record
PCM_MAX_CANDIDATES = 4096


def pcm_params(**kw):
    """ll_pcm_default_params (0.05 rad, 0.5 m, 2e-4 rad/m, 0.02: conventions, not measurements) with the given fields replaced"""
    return _struct_params(PcmParams, load_library().ll_pcm_default_params, kw)


def pcm_candidates(cands):
    """a PCM_CANDIDATE record array from one, or from tuples starting with (i, j, Z[7], ...): a pose-graph edge tuple passes as it is"""
    if isinstance(cands, np.ndarray) and cands.dtype == PCM_CANDIDATE:
        return np.ascontiguousarray(cands).reshape(-1)
    if isinstance(cands, np.ndarray) and cands.dtype in (PG_EDGE, PG_EDGE6):
        out = np.zeros(len(cands), PCM_CANDIDATE)
        out["i"] = cands["i"]; out["j"] = cands["j"]; out["Z_w7"] = cands["Z_w7"]
        return out
    out = np.zeros(len(cands), PCM_CANDIDATE)
    for k, e in enumerate(cands):
        out[k] = (int(e[0]), int(e[1]), np.asarray(e[2], np.float64).reshape(7))
    return out


def pcm_words(C_):
    """words per row of a graph's bit matrix"""
    return (int(C_) + 63) // 64


def pcm_pack_bits(adj):
    """a bool [C, C] matrix as the uint64 [C, ceil(C / 64)] bit matrix of ll_pcm_select (bit d % 64 of word d // 64 stands for d)"""
    a = np.asarray(adj, bool)
    n = len(a); W = pcm_words(n)
    pad = np.zeros((n, W * 64), np.uint8); pad[:, :n] = a
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little")).view("<u8").reshape(n, W)


def pcm_unpack_bits(words, C_):
    """the bool [C, C] matrix of a uint64 [C, W] bit matrix"""
    w = np.ascontiguousarray(words, "<u8").reshape(int(C_), -1)
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :int(C_)].astype(bool)


def pcm_host(poses, candidates, params=None):
    """ll_pcm_host: one graph entirely on the host, no device -> (words uint64 [C, W], selected bool [C], degree int32 [C], PcmRecord)"""
    p = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
    c = pcm_candidates(candidates)
    n = len(c); W = pcm_words(n)
    words = np.zeros((n, W), np.uint64); sel = np.zeros(max(n, 1), np.uint8); deg = np.zeros(max(n, 1), np.int32)
    rec = PcmRecord()
    rc = load_library().ll_pcm_host(len(p), p.ctypes.data, n, c.ctypes.data, None if params is None else C.addressof(params),
                                    words.ctypes.data, sel.ctypes.data, deg.ctypes.data, C.addressof(rec))
    if rc != LL_OK:
        raise LightLoamError(rc, "pcm_host: a NULL or non-finite input, an index outside the graph, i == j, a zero quaternion, a negative "
                                 "parameter, or more than 4096 candidates")
    return words, sel[:n].astype(bool), deg[:n], rec


class Pcm(_Handle):
    """One ll_pcm: the pairwise-consistent set of loop-closure candidates of many graphs side by side.  A graph is (poses [N, 7] in
    trajectory order, candidates); a candidate is any tuple starting with (i, j, Z[7], ...), i and j local to the graph, Z measuring
    P_i^-1 P_j.  Thresholds, not a Mahalanobis test; a greedy clique, not the maximum one"""
    _DESTROY, _ERROR = "ll_pcm_destroy", "ll_pcm_last_error"

    def __init__(self, ctx, max_graphs, max_nodes_total, max_candidates_total):
        self.ctx = ctx; self.lib = ctx.lib
        self.h = C.c_void_p()
        self._sizes = []
        rc = self.lib.ll_pcm_create(ctx.h, int(max_graphs), int(max_nodes_total), int(max_candidates_total), C.byref(self.h))
        if rc != LL_OK:
            raise LightLoamError(rc, ctx.lib.ll_last_error(ctx.h).decode())
        ctx._children.add(self)

    def _split(self, off, sel, deg, rec):
        G = len(off) - 1
        return ([sel[off[g]:off[g + 1]].astype(bool) for g in range(G)], [deg[off[g]:off[g + 1]].copy() for g in range(G)], [rec[g] for g in range(G)])

    def run(self, graphs, params=None):
        """(selected [bool [C_g]], degree [int32 [C_g]], records [PcmRecord]) per graph.  params: a PcmParams (pcm_params(...)).  ONE
        synchronisation"""
        node_off = [0]; cand_off = [0]; poses = []; cands = []
        for g in graphs:
            p = np.ascontiguousarray(g[0], np.float64).reshape(-1, 7); c = pcm_candidates(g[1])
            poses.append(p); cands.append(c)
            node_off.append(node_off[-1] + len(p)); cand_off.append(cand_off[-1] + len(c))
        no = np.array(node_off, np.int32); co = np.array(cand_off, np.int32)
        P = np.ascontiguousarray(np.concatenate(poses)) if poses else np.zeros((0, 7))
        Cd = np.ascontiguousarray(np.concatenate(cands)) if cands else np.zeros(0, PCM_CANDIDATE)
        n = int(co[-1])
        sel = np.zeros(max(n, 1), np.uint8); deg = np.zeros(max(n, 1), np.int32); rec = (PcmRecord * max(len(graphs), 1))()
        self._ck(self.lib.ll_pcm_run(self.h, len(graphs), _ptr(no), _ptr(co), _ptr(P), _ptr(Cd), None if params is None else C.addressof(params),
                                     _ptr(sel), _ptr(deg), C.addressof(rec)))
        self._sizes = [int(co[g + 1] - co[g]) for g in range(len(graphs))]
        return self._split(co, sel, deg, rec)

    def select(self, matrices):
        """the selection alone on supplied adjacency matrices, each a bool [C, C] array or a uint64 [C, ceil(C / 64)] bit matrix -> what
        run returns"""
        words = []; cand_off = [0]
        for m in matrices:
            m = np.asarray(m)
            w = pcm_pack_bits(m) if m.dtype != np.uint64 else np.ascontiguousarray(m).reshape(len(m), -1)
            if len(w) and w.shape[1] != pcm_words(len(w)):
                raise ValueError("a bit matrix of C rows has ceil(C / 64) words per row")
            words.append(w.reshape(-1)); cand_off.append(cand_off[-1] + len(w))
        co = np.array(cand_off, np.int32)
        Wd = np.ascontiguousarray(np.concatenate(words)) if words else np.zeros(0, np.uint64)
        n = int(co[-1])
        sel = np.zeros(max(n, 1), np.uint8); deg = np.zeros(max(n, 1), np.int32); rec = (PcmRecord * max(len(matrices), 1))()
        self._ck(self.lib.ll_pcm_select(self.h, len(matrices), _ptr(co), _ptr(Wd) if len(Wd) else None, _ptr(sel), _ptr(deg), C.addressof(rec)))
        self._sizes = [int(co[g + 1] - co[g]) for g in range(len(matrices))]
        return self._split(co, sel, deg, rec)

    def adjacency_words(self, g):
        """the uint64 [C, ceil(C / 64)] bit matrix of graph g of the last run or select, in original candidate order"""
        n = self._sizes[g] if 0 <= int(g) < len(self._sizes) else 0
        w = np.zeros((n, pcm_words(n)), np.uint64)
        self._ck(self.lib.ll_pcm_adjacency(self.h, int(g), w.ctypes.data if w.size else None))
        return w

    def adjacency(self, g):
        """the consistency matrix of graph g of the last run or select as bool [C, C]"""
        w = self.adjacency_words(g)
        return pcm_unpack_bits(w, len(w)) if len(w) else np.zeros((0, 0), bool)

    def timing(self):
        """the last call: {"ms": [prepare, adjacency, order, clique, pick] (device events), "graphs", "candidates", "pairs", "clique_steps"}"""
        ms = np.zeros(5); cnt = np.zeros(4, np.int64)
        self._ck(self.lib.ll_pcm_timing(self.h, ms.ctypes.data, cnt.ctypes.data))
        return {"ms": ms.tolist(), "graphs": int(cnt[0]), "candidates": int(cnt[1]), "pairs": int(cnt[2]), "clique_steps": int(cnt[3])}


class PlacesParams(C.Structure):
    _fields_ = [("capacity", C.c_int), ("max_radius", C.c_float), ("z_offset", C.c_float)]


class Places(_Handle):
    """One ll_places: Scan Context descriptors (20 rings x 60 sectors) of resident or uploaded scans in HBM, and the exact search of
    every query against every stored place.  Place ids are 0 .. size - 1 in the order they were added."""
    _DESTROY, _ERROR = "ll_places_destroy", "ll_places_last_error"

    DESC = (20, 60)

    def __init__(self, ctx, capacity, max_radius=None, z_offset=None):
        self.ctx = ctx; self.lib = ctx.lib
        self.params = PlacesParams()
        self.lib.ll_places_default_params(C.byref(self.params), int(capacity))
        if max_radius is not None:
            self.params.max_radius = max_radius
        if z_offset is not None:
            self.params.z_offset = z_offset
        self.h = C.c_void_p()
        rc = self.lib.ll_places_create(ctx.h, C.byref(self.params), C.byref(self.h))
        if rc != LL_OK:
            raise LightLoamError(rc, ctx.lib.ll_last_error(ctx.h).decode())
        ctx._children.add(self)

    def __len__(self):
        return self.lib.ll_places_size(self.h)

    def reset(self):
        self._ck(self.lib.ll_places_reset(self.h))

    def add_slots(self, slots):
        """one place per slot from the slots' resident laserCloud -> the first new id.  With Drives: the values slots() returned
        BEFORE the step"""
        s = np.ascontiguousarray(slots, np.int32).reshape(-1)
        first = C.c_int(-1)
        self._ck(self.lib.ll_places_add_slots(self.h, _ptr(s), len(s), C.byref(first)))
        return first.value

    def add_points(self, points):
        """one place from a host cloud (n, 4) float32 -> its id"""
        a = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        pid = C.c_int(-1)
        self._ck(self.lib.ll_places_add_points(self.h, _ptr(a), len(a), C.byref(pid)))
        return pid.value

    def upload(self, first, desc):
        """descriptors [count, 20, 60] float32 to ids first .. (first <= len(self): overwrites or extends)"""
        d = np.ascontiguousarray(desc, np.float32).reshape(-1, 1200)
        self._ck(self.lib.ll_places_upload(self.h, int(first), len(d), _ptr(d)))

    def download(self, first=0, count=None):
        count = len(self) - int(first) if count is None else int(count)
        out = np.zeros((max(count, 0), 20, 60), np.float32)
        self._ck(self.lib.ll_places_download(self.h, int(first), count, _ptr(out)))
        return out

    def distances(self, q0, nq, c0, nc):
        """(dist [nq, nc] float32, shift [nq, nc] uint8): queries q0 .. against candidates c0 .."""
        dist = np.zeros((max(nq, 0), max(nc, 0)), np.float32); shift = np.zeros(dist.shape, np.uint8)
        self._ck(self.lib.ll_places_distances(self.h, int(q0), int(nq), int(c0), int(nc), _ptr(dist), _ptr(shift)))
        return dist, shift

    def match(self, q0, nq, c0, nc, K=1, c_end=None):
        """(id [nq, K] int32, dist [nq, K] float32, shift [nq, K] uint8): per query its K best candidates by (distance, id); ranks
        without a candidate hold (-1, inf, 0).  c_end [nq]: query q only sees candidate ids below c_end[q]"""
        shape = (max(nq, 0), int(K))
        pid = np.zeros(shape, np.int32); dist = np.zeros(shape, np.float32); shift = np.zeros(shape, np.uint8)
        ce = None if c_end is None else np.ascontiguousarray(c_end, np.int32).reshape(-1)
        if ce is not None and len(ce) != nq:
            raise ValueError("c_end must have one entry per query")
        self._ck(self.lib.ll_places_match(self.h, int(q0), int(nq), int(c0), int(nc), _ptr(ce), int(K), _ptr(pid), _ptr(dist), _ptr(shift)))
        return pid, dist, shift

    def timing(self):
        """{"ms": [describe, gram, select], "places": of the last add / upload, "pairs": of the last search} (device events)"""
        ms = np.zeros(3); cnt = np.zeros(2, np.int64)
        self._ck(self.lib.ll_places_timing(self.h, _ptr(ms), _ptr(cnt)))
        return {"ms": ms.tolist(), "places": int(cnt[0]), "pairs": int(cnt[1])}


class PgEdge(C.Structure):
    """ll_pg_edge: Z_w7 measures P_i^-1 P_j (i, j local to the graph); sqrt_info: diagonal, rotation first; huber <= 0: no loss"""
    _fields_ = [("i", C.c_int), ("j", C.c_int), ("Z_w7", C.c_double * 7), ("sqrt_info", C.c_double * 6), ("huber", C.c_double)]


class PgEdge6(C.Structure):
    """ll_pg_edge6: the same edge with a full square-root information: r = S e, S 6 x 6 row-major, any finite matrix"""
    _fields_ = [("i", C.c_int), ("j", C.c_int), ("Z_w7", C.c_double * 7), ("S", C.c_double * 36), ("huber", C.c_double)]


class PgOptions(C.Structure):
    _fields_ = [("max_lm_iterations", C.c_int), ("max_pcg_iterations", C.c_int), ("eta", C.c_double), ("initial_radius", C.c_double),
                ("max_radius", C.c_double), ("min_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double)]


class PgRecord(C.Structure):
    _fields_ = [("cost0", C.c_double), ("cost", C.c_double), ("grad_max", C.c_double), ("lm_iterations", C.c_int),
                ("lm_successes", C.c_int), ("pcg_iterations", C.c_int), ("termination", C.c_int)]


class PgCovQuery(C.Structure):
    """ll_pg_cov_query: the joint covariance of nodes a and b of a graph of the call (local indices); b < 0: node a alone"""
    _fields_ = [("graph", C.c_int), ("a", C.c_int), ("b", C.c_int)]


class PgCovOptions(C.Structure):
    _fields_ = [("max_pcg_iterations", C.c_int), ("tolerance", C.c_double)]


class PgCovRecord(C.Structure):
    """ll_pg_cov_record: status 0 converged, 1 some column hit max_pcg_iterations, 2 breakdown (the blocks are zeros)"""
    _fields_ = [("status", C.c_int), ("pcg_iterations", C.c_int), ("residual", C.c_double)]


PG_COV_QUERY = np.dtype([("graph", "i4"), ("a", "i4"), ("b", "i4")])                                                   # PgCovQuery as a numpy record
PG_COV_STATUS = {0: "converged", 1: "iterations", 2: "breakdown"}
PG_EDGE = np.dtype([("i", "i4"), ("j", "i4"), ("Z_w7", "f8", (7,)), ("sqrt_info", "f8", (6,)), ("huber", "f8")])     # PgEdge as a numpy record
PG_EDGE6 = np.dtype([("i", "i4"), ("j", "i4"), ("Z_w7", "f8", (7,)), ("S", "f8", (6, 6)), ("huber", "f8")])          # PgEdge6 as a numpy record
PG_TERMINATION = {0: "gradient", 1: "function", 2: "parameter", 3: "iterations", 4: "radius", 5: "non-finite"}
PG_PRECOND_BLOCK_JACOBI, PG_PRECOND_CHAIN = 0, 1                    # LL_PG_PRECOND_*: the preconditioner of a PoseGraphs' solves
PG_PRECOND_NAMES = {"jacobi": PG_PRECOND_BLOCK_JACOBI, "chain": PG_PRECOND_CHAIN}


def pg_options(**kw):
    """ll_pg_default_options with the given fields replaced"""
    o = PgOptions()
    load_library().ll_pg_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def pg_cov_options(**kw):
    """ll_pg_cov_default_options (1000 PCG iterations per column, tolerance 1e-10) with the given fields replaced"""
    o = PgCovOptions()
    load_library().ll_pg_cov_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                     a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def relative_pose(Pi, Pj):
    """P_i^-1 P_j in the pose_w7 layout: the measurement of an odometry edge between two poses of a chain"""
    Pi = np.asarray(Pi, np.float64); Pj = np.asarray(Pj, np.float64)
    qi = Pi[:4] / np.linalg.norm(Pi[:4])
    ci = qi * np.array([-1.0, -1.0, -1.0, 1.0])
    v = np.concatenate([Pj[4:] - Pi[4:], [0.0]])
    return np.concatenate([_quat_mul(ci, Pj[:4]), _quat_mul(_quat_mul(ci, v), qi)[:3]])


def pg_edges(edges):
    """a PG_EDGE record array from one, or from a list of (i, j, Z[7], sqrt_info[6] or scalar, huber) tuples.  If the sqrt_info of
    any tuple is a 6 x 6 array, a PG_EDGE6 record array comes back, the diagonal weights of the others promoted to diag(sqrt_info)"""
    if isinstance(edges, np.ndarray) and edges.dtype in (PG_EDGE, PG_EDGE6):
        return np.ascontiguousarray(edges).reshape(-1)
    if any(np.ndim(e[3]) == 2 for e in edges):
        out = np.zeros(len(edges), PG_EDGE6)
        for k, e in enumerate(edges):
            w = np.asarray(e[3], np.float64)
            S = w.reshape(6, 6) if w.ndim == 2 else np.diag(np.broadcast_to(w, (6,)))
            out[k] = (int(e[0]), int(e[1]), np.asarray(e[2], np.float64), S, float(e[4]) if len(e) > 4 else 0.0)
        return out
    out = np.zeros(len(edges), PG_EDGE)
    for k, e in enumerate(edges):
        out[k] = (int(e[0]), int(e[1]), np.asarray(e[2], np.float64), np.broadcast_to(np.asarray(e[3], np.float64), (6,)), float(e[4]) if len(e) > 4 else 0.0)
    return out


def pg_edges6(edges):
    """a PG_EDGE6 record array from what pg_edges gives: full edges as they are, diagonal ones with S = diag(sqrt_info)"""
    e = pg_edges(edges)
    if e.dtype == PG_EDGE6:
        return e
    out = np.zeros(len(e), PG_EDGE6)
    out["i"] = e["i"]; out["j"] = e["j"]; out["Z_w7"] = e["Z_w7"]; out["huber"] = e["huber"]
    for k in range(6):
        out["S"][:, k, k] = e["sqrt_info"][:, k]
    return out


def edge_from_info(info, X, sigma=0.0, floor=0.0):
    """ll_pg_edge_from_info: the upper-triangular S [6, 6] with S^T S = the information, in the tangent of a pose-graph edge
    (i, j, Z = relative_pose(P_i, X)), of the solve the PoseInfo record describes; X: the localised pose or the aligned T.
    sigma: the residual standard deviation in metres (<= 0: sqrt(info.sigma2)); floor: added to the information's diagonal.
    Host arithmetic: needs no device"""
    x = np.ascontiguousarray(X, np.float64).reshape(7)
    S = np.zeros((6, 6))
    rc = load_library().ll_pg_edge_from_info(C.addressof(info), x.ctypes.data, float(sigma), float(floor), S.ctypes.data)
    if rc != LL_OK:
        raise LightLoamError(rc, "edge_from_info: the record is not finite, sigma2 is 0 with sigma <= 0, or the information is not positive definite"
                             if rc == -7 else "edge_from_info: a non-finite argument, a negative floor or a zero quaternion")
    return S


def edge_gate(Pa, Pb, Z, S, joint, with_cov=False):
    """ll_pg_edge_gate: chi2 = e^T C^-1 e of the candidate edge a -> b with measurement Z [7] and square-root information S ([6, 6], [6]
    for a diagonal one, or None) against the joint covariance [12, 12] of the two poses (PoseGraphs.covariances), C = J Sigma J^T +
    (S^T S)^-1; 6 degrees of freedom.  with_cov: (chi2, C [6, 6]).  A chi-square only for an edge that is NOT in the graph.
    Host arithmetic: needs no device"""
    pa = np.ascontiguousarray(Pa, np.float64).reshape(7); pb = np.ascontiguousarray(Pb, np.float64).reshape(7)
    z = np.ascontiguousarray(Z, np.float64).reshape(7); jt = np.ascontiguousarray(joint, np.float64).reshape(144)
    s = None
    if S is not None:
        s = np.asarray(S, np.float64)
        s = np.ascontiguousarray(s.reshape(6, 6) if s.size == 36 else np.diag(np.broadcast_to(s, (6,))))
    chi2 = C.c_double(0.0); cov = np.zeros((6, 6))
    rc = load_library().ll_pg_edge_gate(pa.ctypes.data, pb.ctypes.data, z.ctypes.data, None if s is None else s.ctypes.data, jt.ctypes.data,
                                        C.addressof(chi2), cov.ctypes.data if with_cov else None)
    if rc != LL_OK:
        raise LightLoamError(rc, "edge_gate: a non-finite input, a zero quaternion, or a covariance or information that is not positive definite")
    return (chi2.value, cov) if with_cov else chi2.value


class PoseGraphs(_Handle):
    """One ll_posegraphs: many independent SE(3) pose graphs optimised side by side on the device, one workgroup per graph.  A graph
    is the tuple (poses [N, 7], edges, fixed): poses in the pose_w7 layout (world from body), edges as pg_edges takes them (i, j local to
    the graph, Z measures P_i^-1 P_j), fixed None (node 0 is fixed) or N flags."""
    _DESTROY, _ERROR = "ll_posegraphs_destroy", "ll_posegraphs_last_error"

    def __init__(self, ctx, max_graphs, max_nodes_total, max_edges_total):
        self.ctx = ctx; self.lib = ctx.lib
        self.h = C.c_void_p()
        rc = self.lib.ll_posegraphs_create(ctx.h, int(max_graphs), int(max_nodes_total), int(max_edges_total), C.byref(self.h))
        if rc != LL_OK:
            raise LightLoamError(rc, ctx.lib.ll_last_error(ctx.h).decode())
        ctx._children.add(self)

    @staticmethod
    def _pack(graphs):
        """the ragged packing: (node_off, edge_off, poses [Nt, 7], fixed [Nt] uint8, edges [Et] PG_EDGE -- or PG_EDGE6, the diagonal
        edges promoted, if any edge of the call has a 6 x 6 sqrt_info)"""
        node_off = [0]; edge_off = [0]; poses = []; fixed = []; edges = []
        for g in graphs:
            p = np.ascontiguousarray(g[0], np.float64).reshape(-1, 7)
            e = pg_edges(g[1])
            f = g[2] if len(g) > 2 else None
            if f is None:
                f = np.zeros(len(p), np.uint8); f[:1] = 1
            f = (np.asarray(f).reshape(-1) != 0).astype(np.uint8)
            if len(f) != len(p):
                raise ValueError("fixed must have one entry per node")
            poses.append(p); fixed.append(f); edges.append(e)
            node_off.append(node_off[-1] + len(p)); edge_off.append(edge_off[-1] + len(e))
        if any(e.dtype == PG_EDGE6 for e in edges):
            edges = [pg_edges6(e) for e in edges]
        cat = lambda parts, empty: np.ascontiguousarray(np.concatenate(parts)) if parts else empty
        return (np.array(node_off, np.int32), np.array(edge_off, np.int32), cat(poses, np.zeros((0, 7))), cat(fixed, np.zeros(0, np.uint8)),
                cat(edges, np.zeros(0, PG_EDGE)))

    def evaluate(self, graphs):
        """(cost [G], [grad [N_g, 6] per graph]): the robustified cost and its gradient per increment (zeros at fixed nodes)"""
        no, eo, poses, fixed, edges = self._pack(graphs)
        cost = np.zeros(len(graphs)); grad = np.zeros((len(poses), 6))
        fn = self.lib.ll_posegraphs_evaluate6 if edges.dtype == PG_EDGE6 else self.lib.ll_posegraphs_evaluate
        self._ck(fn(self.h, len(graphs), _ptr(no), _ptr(eo), _ptr(poses), _ptr(fixed), _ptr(edges), _ptr(cost), _ptr(grad)))
        return cost, [grad[no[g]:no[g + 1]].copy() for g in range(len(graphs))]

    def solve(self, graphs, options=None):
        """([poses [N_g, 7] per graph], records [G] of PgRecord): the inputs are not modified.  options: a PgOptions (pg_options(...))"""
        no, eo, poses, fixed, edges = self._pack(graphs)
        rec = (PgRecord * max(len(graphs), 1))()
        fn = self.lib.ll_posegraphs_solve6 if edges.dtype == PG_EDGE6 else self.lib.ll_posegraphs_solve
        self._ck(fn(self.h, len(graphs), _ptr(no), _ptr(eo), _ptr(poses), _ptr(fixed), _ptr(edges),
                    None if options is None else C.addressof(options), C.addressof(rec)))
        return [poses[no[g]:no[g + 1]].copy() for g in range(len(graphs))], list(rec)[:len(graphs)]

    def timing(self):
        """{"ms": [evaluate, solve] of the last such calls (device events), "graphs", "lm_iterations", "pcg_iterations": of the last call}"""
        ms = np.zeros(2); cnt = np.zeros(3, np.int64)
        self._ck(self.lib.ll_posegraphs_timing(self.h, _ptr(ms), _ptr(cnt)))
        return {"ms": ms.tolist(), "graphs": int(cnt[0]), "lm_iterations": int(cnt[1]), "pcg_iterations": int(cnt[2])}

    def covariances(self, graphs, queries, options=None):
        """(joint [Q, 12, 12], records [Q] of PgCovRecord): ll_posegraphs_covariances at the graphs' poses.  queries: (graph, a, b) tuples
        or a PG_COV_QUERY record array, a and b local to the graph, b < 0 (or left out): node a alone.  joint[q] = [[S_aa, S_ab], [S_ba,
        S_bb]] of Sigma = H^-1 in the increments' tangent (half-angle vector, translation); zeros at fixed nodes.  options: a PgCovOptions
        (pg_cov_options(...)).  The object's preconditioner applies"""
        no, eo, poses, fixed, edges = self._pack(graphs)
        if isinstance(queries, np.ndarray) and queries.dtype == PG_COV_QUERY:
            q = np.ascontiguousarray(queries).reshape(-1)
        else:
            q = np.zeros(len(queries), PG_COV_QUERY)
            for k, t in enumerate(queries):
                q[k] = (int(t[0]), int(t[1]), int(t[2]) if len(t) > 2 else -1)
        joint = np.zeros((len(q), 12, 12)); rec = (PgCovRecord * max(len(q), 1))()
        fn = self.lib.ll_posegraphs_covariances6 if edges.dtype == PG_EDGE6 else self.lib.ll_posegraphs_covariances
        self._ck(fn(self.h, len(graphs), _ptr(no), _ptr(eo), _ptr(poses), _ptr(fixed), _ptr(edges), len(q), _ptr(q),
                    None if options is None else C.addressof(options), _ptr(joint), C.addressof(rec)))
        return joint, list(rec)[:len(q)]

    def cov_timing(self):
        """{"ms": [prepare, columns] of the last covariances call (device events), "queries", "sources", "pcg_iterations": of that call}"""
        ms = np.zeros(2); cnt = np.zeros(3, np.int64)
        self._ck(self.lib.ll_posegraphs_cov_timing(self.h, _ptr(ms), _ptr(cnt)))
        return {"ms": ms.tolist(), "queries": int(cnt[0]), "sources": int(cnt[1]), "pcg_iterations": int(cnt[2])}

    def set_preconditioner(self, kind):
        """PG_PRECOND_BLOCK_JACOBI (0, the default) or PG_PRECOND_CHAIN (1: the block-tridiagonal chain, by cyclic reduction), or the
        names "jacobi" / "chain"; applies to the solves from the next call on, evaluate does not change"""
        self._ck(self.lib.ll_posegraphs_set_preconditioner(self.h, int(PG_PRECOND_NAMES.get(kind, kind))))

    @property
    def preconditioner(self):
        return int(self.lib.ll_posegraphs_preconditioner(self.h))

    def precond_stats(self):
        """{"factorisations", "fallbacks"}: factorisations of the chain matrix and LM iterations that fell back to block-Jacobi, summed
        over the graphs of the last solve"""
        cnt = np.zeros(2, np.int64)
        self._ck(self.lib.ll_posegraphs_precond_stats(self.h, _ptr(cnt)))
        return {"factorisations": int(cnt[0]), "fallbacks": int(cnt[1])}

    def chain_solve(self, systems):
        """ll_posegraphs_chain_solve: the chain preconditioner's solver alone.  systems: a list of (diag [N, 6, 6], upper [N, 6, 6] or
        [N - 1, 6, 6] -- M[n][n+1] --, rhs [N, 6]) -> ([x [N, 6] per system], status [S] int32: 1 where a pivot failed, x zeros then)"""
        node_off = [0]; diag = []; upper = []; rhs = []
        for d, u, r in systems:
            d = np.ascontiguousarray(d, np.float64).reshape(-1, 36)
            u = np.asarray(u, np.float64).reshape(-1, 36)
            if len(u) == len(d) - 1:
                u = np.concatenate([u, np.zeros((1, 36))])
            r = np.ascontiguousarray(r, np.float64).reshape(-1, 6)
            if len(u) != len(d) or len(r) != len(d):
                raise ValueError("diag, upper and rhs must have one block per node (upper may leave out the last)")
            diag.append(d); upper.append(u); rhs.append(r); node_off.append(node_off[-1] + len(d))
        cat = lambda parts, w: np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, w))
        no = np.array(node_off, np.int32); diag = cat(diag, 36); upper = cat(upper, 36); rhs = cat(rhs, 6)
        out = np.zeros_like(rhs); status = np.zeros(max(len(systems), 1), np.int32)
        self._ck(self.lib.ll_posegraphs_chain_solve(self.h, len(systems), _ptr(no), _ptr(diag), _ptr(upper), _ptr(rhs), _ptr(out), _ptr(status)))
        return [out[no[g]:no[g + 1]].copy() for g in range(len(systems))], status[:len(systems)]


class DrivesParams(C.Structure):
    _fields_ = [("n_lanes", C.c_int), ("base", C.c_int), ("line_res", C.c_float), ("plane_res", C.c_float),
                ("max_scan_corner", C.c_int), ("max_scan_surf", C.c_int), ("pool_points", C.c_int), ("n_outer", C.c_int),
                ("keep_registered", C.c_int)]


IDLE, RUN, START = 0, 1, 2


class Drives(_Handle):
    """One ll_drives: n_lanes lanes, each running one drive at a time through registration -> odometry -> mapping.  Upload lane q's
    raw scan into slots()[q], then step(cmd): IDLE (0), RUN (1: the next frame, only after a step the lane ran) or START (2: frame 0
    of a new drive).  Lane q equals its drive run alone through ll_odometry_frames, WorldPose and a CubeMap, bit for bit."""
    _DESTROY, _ERROR = "ll_drives_destroy", "ll_drives_last_error"

    def __init__(self, ctx, n_lanes, max_scan_corner, max_scan_surf, pool_points=1 << 20, base=0, line_res=0.4, plane_res=0.8,
                 n_outer=3, keep_registered=False):
        self.ctx = ctx; self.lib = ctx.lib; self.n_lanes = int(n_lanes)
        self.lib.ll_drives_last_error.restype = C.c_char_p
        self.lib.ll_drives_last_error.argtypes = [C.c_void_p]
        self.lib.ll_drives_destroy.argtypes = [C.c_void_p]
        self.lib.ll_drives_cubemaps.restype = C.c_void_p
        self.lib.ll_drives_cubemaps.argtypes = [C.c_void_p]
        self.params = DrivesParams(self.n_lanes, int(base), line_res, plane_res, int(max_scan_corner), int(max_scan_surf),
                                   int(pool_points), int(n_outer), int(bool(keep_registered)))
        self.h = C.c_void_p()
        rc = self.lib.ll_drives_create(ctx.h, C.byref(self.params), C.byref(self.h))
        if rc != LL_OK:
            raise LightLoamError(rc, ctx.lib.ll_last_error(ctx.h).decode())
        ctx._children.add(self)
        self._cms_h = C.c_void_p(self.lib.ll_drives_cubemaps(self.h))

    @property
    def cubemaps(self):
        """the lanes' cube maps (borrowed CubeMaps: info / cloud / cube per lane)"""
        return _BorrowedCubeMaps(self._cms_h, self)

    def export_maps(self, which):
        """CubeMaps.export of the lanes' maps: (points [N, 4], offset [S + 1]); between any two steps"""
        return self.cubemaps.export(which)

    def slots(self):
        """[S]: the slot the next step reads each lane's raw scan from"""
        s = np.zeros(self.n_lanes, np.int32)
        self._ck(self.lib.ll_drives_slots(self.h, _ptr(s)))
        return s

    def step(self, cmd, pose0=None):
        """cmd [S] of IDLE / RUN / START; pose0: None or [S, 7] (the rows of START lanes are read) -> (odom [S, 7], mapped [S, 7],
        ran [S] bool); rows of lanes that did not run are NaN / False"""
        c = np.ascontiguousarray(cmd, np.int32)
        if c.shape != (self.n_lanes,):
            raise ValueError("cmd must have one entry per lane")
        p0 = None if pose0 is None else np.ascontiguousarray(pose0, np.float64).reshape(self.n_lanes, 7)
        odom = np.zeros((self.n_lanes, 7)); mapped = np.zeros((self.n_lanes, 7)); ran = np.zeros(self.n_lanes, np.int32)
        self._ck(self.lib.ll_drives_step(self.h, _ptr(c), _ptr(p0), _ptr(odom), _ptr(mapped), _ptr(ran)))
        return odom, mapped, ran.astype(bool)

    def set_localize(self, map_of, start=None):
        """map_of [S]: -1 = the lane maps into its own map, m >= 0 = it localises against lane m's map, from the next step on;
        start: None or [S, 7], the map-to-odom pose START gives a localising lane (where its drive begins in the map)"""
        m = np.ascontiguousarray(map_of, np.int32)
        if m.shape != (self.n_lanes,):
            raise ValueError("map_of must have one entry per lane")
        st = None if start is None else np.ascontiguousarray(start, np.float64).reshape(self.n_lanes, 7)
        self._ck(self.lib.ll_drives_set_localize(self.h, m.ctypes.data, None if st is None else st.ctypes.data))

    def set_map_vote(self, from_frame):
        """the mapping lanes vote their plane blocks in frames whose per-lane index is > from_frame (the reference's gate: 20); negative:
        off, the default (ll_drives_set_map_vote).  Not part of a checkpoint: set it again after restore"""
        self._ck(self.lib.ll_drives_set_map_vote(self.h, int(from_frame)))

    def set_keyframes(self, kf, every=1):
        """from the next step on every lane that ran a frame whose per-lane index is a multiple of `every` is captured into the
        Keyframes store kf (its stack clouds and mapped pose, tagged with lane and frame index); None: off, the default"""
        self._kf = kf                                                # keeps the store alive while the drives object points at it
        self._ck(self.lib.ll_drives_set_keyframes(self.h, None if kf is None else kf.h, int(every)))

    def correct(self, lanes, C_w7):
        """left-multiplies the map-to-odom pose of every lane with lanes[q] = 1 by C_w7[q] ([S, 7]): with C = P'_last o P_last^-1 the
        lane's drive continues in a map rebuilt under corrected poses.  Between any two steps"""
        sel = self._lanes(lanes)
        c = np.ascontiguousarray(C_w7, np.float64).reshape(self.n_lanes, 7)
        self._ck(self.lib.ll_drives_correct(self.h, sel.ctypes.data, c.ctypes.data))

    def fit(self):
        """the last step's LocalizeFit records [S]: zeros for lanes that mapped, sat out or did not optimise"""
        rec = (LocalizeFit * self.n_lanes)()
        self._ck(self.lib.ll_drives_fit(self.h, C.addressof(rec)))
        return rec

    def set_info(self, on=True):
        """the localising lanes' steps also fill PoseInfo records (info()); off after create, not part of a checkpoint"""
        self._ck(self.lib.ll_drives_set_info(self.h, 1 if on else 0))

    def info(self):
        """the last step's PoseInfo records [S]: zeros for lanes that mapped, sat out or did not optimise, and while set_info is off"""
        rec = (PoseInfo * self.n_lanes)()
        self._ck(self.lib.ll_drives_info(self.h, C.addressof(rec)))
        return rec

    def registered(self, lane):
        """the last step's registered full-resolution cloud of `lane` ((n, 4) float32, laserCloud order; empty if it did not run)"""
        n = C.c_int(0)
        self._ck(self.lib.ll_drives_registered(self.h, int(lane), None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 4), np.float32)
        self._ck(self.lib.ll_drives_registered(self.h, int(lane), _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def _lanes(self, lanes):
        sel = np.ascontiguousarray(lanes).astype(np.int32)
        if sel.shape != (self.n_lanes,):
            raise ValueError("lanes must be a 0 / 1 mask with one entry per lane")
        return sel

    def save_size(self, lanes):
        """bytes of save(lanes): host bookkeeping, no launch, no synchronisation.  lanes: a 0 / 1 mask [S]"""
        n = self.lib.ll_drives_save_size(self.h, self._lanes(lanes).ctypes.data)
        if n < 0:
            self._ck(int(n))
        return int(n)

    def save(self, lanes, out=None):
        """the checkpoint of the selected lanes: bytes, or the filled uint8 array `out`.  One pack launch, one copy, one
        synchronisation; the run goes on as if it had not saved"""
        sel = self._lanes(lanes)
        n = self.save_size(sel)
        buf = np.empty(n, np.uint8) if out is None else out
        if buf.dtype != np.uint8 or not buf.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous uint8 array")
        got = C.c_longlong(0)
        self._ck(self.lib.ll_drives_save(self.h, sel.ctypes.data, buf.ctypes.data, buf.size, C.addressof(got)))
        return buf[:got.value].tobytes() if out is None else buf[:got.value]

    def restore(self, blob, into):
        """record r of the checkpoint goes into lane into[r] (-1: skipped); the lane may then RUN on"""
        raw = np.frombuffer(blob, np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, np.uint8)
        dst = np.ascontiguousarray(into, np.int32)
        n = _checkpoint_records(raw)                                 # the header's count: the library validates the blob itself, once
        if n is not None and dst.shape != (n,):
            raise ValueError(f"into must have one entry per record ({n})")
        self._ck(self.lib.ll_drives_restore(self.h, dst.ctypes.data, raw.ctypes.data, raw.size))

    def stats(self):
        """(host synchronisations inside steps, steps that ran at least one lane) since create"""
        s = C.c_longlong(0); f = C.c_longlong(0)
        self._ck(self.lib.ll_drives_stats(self.h, C.byref(s), C.byref(f)))
        return s.value, f.value


class _BorrowedCubeMaps(CubeMaps):
    """the CubeMaps interface over the handle an ll_drives owns; closing it does nothing"""

    def __init__(self, handle, owner):
        self.ctx = owner.ctx; self.lib = owner.lib; self.n_seq = owner.n_lanes; self.h = handle
        self._owner = owner                           # keeps the drives object (and so the handle) alive

    def close(self):
        self.h = None


class CheckpointRecord(C.Structure):
    _fields_ = [("lane", C.c_int), ("frame_index", C.c_int), ("n_corner", C.c_longlong), ("n_surf", C.c_longlong),
                ("n_features", C.c_int * 4), ("offset", C.c_longlong), ("bytes", C.c_longlong)]


class CheckpointInfo(C.Structure):
    _fields_ = [("version", C.c_int), ("n_records", C.c_int), ("total_bytes", C.c_longlong), ("n_scans", C.c_int),
                ("distortion", C.c_int), ("voxel_sort_ranks", C.c_int), ("line_res", C.c_float), ("plane_res", C.c_float),
                ("need_features", C.c_int * 4), ("records", C.POINTER(CheckpointRecord)), ("cap_records", C.c_int)]


def _checkpoint_records(raw):
    """n_records as the header states it (bytes 24..28), None for a blob too short or too large to be believed"""
    if raw.size < 28:
        return None
    n = int(raw[24:28].view("<u4")[0])
    return n if n <= 4096 else None


def describe_checkpoint(blob, lib=None):
    """validate a checkpoint (bytes or uint8 array) on the host -- no device, no context -- and return its header fields and
    per-record sizes as a dict; LightLoamError(LL_ERR_ARG) for a blob this library cannot read"""
    lib = lib or load_library()
    raw = np.frombuffer(blob, np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, np.uint8)
    info = CheckpointInfo()
    recs = (CheckpointRecord * max(_checkpoint_records(raw) or 0, 1))()
    info.records = C.cast(recs, C.POINTER(CheckpointRecord)); info.cap_records = len(recs)
    rc = lib.ll_checkpoint_describe(raw.ctypes.data if raw.size else None, raw.size, C.addressof(info))
    if rc != LL_OK:
        raise LightLoamError(rc, "not a readable checkpoint")
    out = {k: getattr(info, k) for k in ("version", "n_records", "total_bytes", "n_scans", "distortion", "voxel_sort_ranks", "line_res", "plane_res")}
    out["need_features"] = tuple(info.need_features)
    out["records"] = [dict(lane=r.lane, frame_index=r.frame_index, n_corner=r.n_corner, n_surf=r.n_surf, n_features=tuple(r.n_features),
                           offset=r.offset, bytes=r.bytes) for r in recs[:info.n_records]]
    return out


_EMPTY = (C.c_float * 4)()      # a non-NULL address for an empty cloud of a running sequence
