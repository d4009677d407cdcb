"""ctypes binding of liborbx.so (include/orbx.h).  This is the ONLY way Python reaches the HIP path;
there is no CPU fallback: a missing library or a missing GPU raises."""
from __future__ import annotations
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# ORBX_LIB: another build of the same library (kernel-variant sweeps in tools/); never a different implementation
LIB_PATH = os.environ.get("ORBX_LIB") or os.path.join(HERE, "lib", "liborbx.so")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28

OK, EMPTY_IMAGE, BAD_ARGUMENT, BAD_ASPECT, CAPACITY, HIP_ERROR, NO_DEVICE, UNSUPPORTED = range(8)
FP_GCC_FMA, FP_STRICT = 0, 1
PYRAMID_FORK_PADDED, PYRAMID_UPSTREAM = 0, 1   # orbx_params.pyramid_mode: what mvImagePyramid[level] is (include/orbx.h)
FMT_GRAY8, FMT_RGB8, FMT_BGR8, FMT_RGBA8, FMT_BGRA8 = range(5)
DEPTH_U16, DEPTH_F32 = 0, 1
K_NAMES = ("k_pyr_l0", "k_pyr_resize", "k_fast_rows", "k_quadtree", "k_orient", "k_blur", "k_describe",
           "k_match", "misc")
K_COUNT = len(K_NAMES)


class Params(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("pyramid_mode", C.c_int32),
                ("fp_mode", C.c_int32), ("device", C.c_int32), ("max_batch", C.c_int32),
                ("max_cand_per_cell", C.c_int32)]


class FrameView(C.Structure):
    _fields_ = [("keys_un", C.c_void_p), ("desc", C.c_void_p), ("u_right", C.c_void_p), ("n", C.c_int32),
                ("Tcw", C.c_float * 16), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("mb", C.c_float), ("mbf", C.c_float)]


class LastFrameView(C.Structure):
    _fields_ = [("keys_un", C.c_void_p), ("n", C.c_int32), ("has_map_point", C.c_void_p), ("world_pos", C.c_void_p),
                ("mp_desc", C.c_void_p), ("observations", C.c_void_p), ("Tcw", C.c_float * 16)]


class MapPointView(C.Structure):
    _fields_ = [("n", C.c_int32), ("in_view", C.c_void_p), ("proj", C.c_void_p), ("level", C.c_void_p),
                ("view_cos", C.c_void_p), ("desc", C.c_void_p), ("observations", C.c_void_p)]


class TrackFrameProblem(C.Structure):   # orbx_track_frame_problem
    _fields_ = [("frame", C.c_int32), ("th", C.c_float), ("mono", C.c_int32), ("Tcw", C.c_float * 16),
                ("last", LastFrameView)]


class TrackPointsProblem(C.Structure):   # orbx_track_points_problem
    _fields_ = [("frame", C.c_int32), ("th", C.c_float), ("frame_observations", C.c_void_p), ("points", MapPointView)]


class LocalMapView(C.Structure):   # orbx_local_map_view
    _fields_ = [("n", C.c_int32), ("world_pos", C.c_void_p), ("normal", C.c_void_p), ("min_distance", C.c_void_p),
                ("max_distance", C.c_void_p), ("desc", C.c_void_p), ("observations", C.c_void_p)]


class TrackLocalProblem(C.Structure):   # orbx_track_local_problem
    _fields_ = [("frame", C.c_int32), ("th", C.c_float), ("viewing_cos_limit", C.c_float), ("Tcw", C.c_float * 16),
                ("Ow", C.c_float * 3), ("npoints", C.c_int32), ("point_index", C.c_void_p), ("skip", C.c_void_p),
                ("frame_observations", C.c_void_p)]


class PoseProblem(C.Structure):   # orbx_pose_problem
    _fields_ = [("frame", C.c_int32), ("Tcw", C.c_float * 16), ("point_index", C.c_void_p), ("npoints", C.c_int32)]


class Sim3Problem(C.Structure):   # orbx_sim3_problem
    _fields_ = [("n", C.c_int32), ("x1c", C.c_void_p), ("x2c", C.c_void_p), ("max_err1", C.c_void_p), ("max_err2", C.c_void_p),
                ("camera1", C.c_float * 4), ("camera2", C.c_float * 4), ("fix_scale", C.c_int32), ("min_inliers", C.c_int32),
                ("iterations", C.c_int32), ("sets", C.c_void_p)]


class Sim3OptProblem(C.Structure):   # orbx_sim3opt_problem
    _fields_ = [("n", C.c_int32), ("x1c", C.c_void_p), ("x2c", C.c_void_p), ("obs1", C.c_void_p), ("obs2", C.c_void_p),
                ("inv_sigma2_1", C.c_void_p), ("inv_sigma2_2", C.c_void_p), ("camera1", C.c_float * 4), ("camera2", C.c_float * 4),
                ("R", C.c_float * 9), ("t", C.c_float * 3), ("s", C.c_float), ("th2", C.c_float), ("fix_scale", C.c_int32),
                ("keep", C.c_void_p)]


SIM3OPT_RESULT_DTYPE = np.dtype([("r", "<f8", 4), ("t", "<f8", 3), ("s", "<f8"), ("T12", "<f4", 16), ("ninliers", "<i4"),
                                 ("nbad", "<i4"), ("ncorr", "<i4"), ("written", "<i4")])   # orbx_sim3opt_result
assert SIM3OPT_RESULT_DTYPE.itemsize == 144


class LocalBAProblem(C.Structure):   # orbx_localba_problem
    _fields_ = [("nlocal", C.c_int32), ("nfixed", C.c_int32), ("npoints", C.c_int32), ("second_round", C.c_int32),
                ("Tcw", C.c_void_p), ("local_fixed", C.c_void_p), ("camera", C.c_float * 4), ("bf", C.c_float),
                ("world", C.c_void_p), ("obs_begin", C.c_void_p), ("obs_kf", C.c_void_p), ("obs", C.c_void_p),
                ("inv_sigma2", C.c_void_p), ("Tcw_out", C.c_void_p), ("world_out", C.c_void_p), ("erase", C.c_void_p)]


class LocalBADebug(C.Structure):   # orbx_localba_debug
    _fields_ = [("Tcw_est", C.c_void_p), ("world_est", C.c_void_p), ("Tcw_last", C.c_void_p), ("world_last", C.c_void_p)]


LOCALBA_RESULT_DTYPE = np.dtype([("iters", "<i4", 2), ("nflagged", "<i4"), ("nerase", "<i4"), ("chi2", "<f8", 4)])   # orbx_localba_result
assert LOCALBA_RESULT_DTYPE.itemsize == 48


class EssGraphProblem(C.Structure):   # orbx_essgraph_problem
    _fields_ = [("nvertices", C.c_int32), ("nedges", C.c_int32), ("npoints", C.c_int32), ("fix_scale", C.c_int32),
                ("Scw", C.c_void_p), ("fixed", C.c_void_p), ("non_corrected", C.c_void_p), ("has_non_corrected", C.c_void_p),
                ("edges", C.c_void_p), ("world", C.c_void_p), ("ref", C.c_void_p), ("Siw_out", C.c_void_p),
                ("Tiw_out", C.c_void_p), ("world_out", C.c_void_p)]


ESSGRAPH_RESULT_DTYPE = np.dtype([("iters", "<i4"), ("nactive", "<i4"), ("nfailed", "<i4"), ("nrounds", "<i4"), ("nlblocks", "<i4"),
                                  ("pad", "<i4"), ("chi2", "<f8", 2), ("lambda", "<f8")])   # orbx_essgraph_result
assert ESSGRAPH_RESULT_DTYPE.itemsize == 48
ESSGRAPH_MAX_LBLOCKS = 32768   # ORBX_ESSGRAPH_MAX_LBLOCKS


class PnpProblem(C.Structure):   # orbx_pnp_problem
    _fields_ = [("n", C.c_int32), ("p3dw", C.c_void_p), ("p2d", C.c_void_p), ("max_err", C.c_void_p), ("camera", C.c_double * 4),
                ("min_inliers", C.c_int32), ("iterations", C.c_int32), ("sets", C.c_void_p)]


class InitProblem(C.Structure):   # orbx_init_problem
    _fields_ = [("n1", C.c_int32), ("n2", C.c_int32), ("keys1", C.c_void_p), ("keys2", C.c_void_p), ("n", C.c_int32),
                ("matches", C.c_void_p), ("sigma", C.c_float), ("iterations", C.c_int32), ("sets", C.c_void_p),
                ("models", C.c_int32)]


class ReconProblem(C.Structure):   # orbx_recon_problem
    _fields_ = [("n1", C.c_int32), ("n2", C.c_int32), ("keys1", C.c_void_p), ("keys2", C.c_void_p), ("n", C.c_int32),
                ("matches", C.c_void_p), ("inliers", C.c_void_p), ("model", C.c_int32), ("M", C.c_float * 9), ("K", C.c_float * 4),
                ("sigma", C.c_float), ("min_parallax", C.c_float), ("min_triangulated", C.c_int32)]


class InitCamera(C.Structure):   # orbx_init_camera
    _fields_ = [("K", C.c_float * 4), ("min_parallax", C.c_float), ("min_triangulated", C.c_int32)]


INIT_NONE, INIT_H, INIT_F = 0, 1, 2


class NewPointsKeyFrame(C.Structure):   # orbx_newpoints_keyframe
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float), ("mb", C.c_float),
                ("mbf", C.c_float), ("nlevels", C.c_int32), ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p),
                ("n", C.c_int32), ("keys_un", C.c_void_p), ("keys", C.c_void_p), ("u_right", C.c_void_p), ("depth", C.c_void_p)]


class NewPointsProblem(C.Structure):   # orbx_newpoints_problem
    _fields_ = [("kf1", NewPointsKeyFrame), ("kf2", NewPointsKeyFrame), ("scale_factor", C.c_float), ("nmatches", C.c_int32),
                ("matches", C.c_void_p)]


# orbx_create_new_map_points_batch's status bytes (ORBX_NEWPOINT_*); 1..3 accept
(NEWPOINT_TRIANGULATED, NEWPOINT_STEREO1, NEWPOINT_STEREO2, NEWPOINT_LOW_PARALLAX, NEWPOINT_ZERO_W, NEWPOINT_DEPTH1,
 NEWPOINT_DEPTH2, NEWPOINT_REPROJ1, NEWPOINT_REPROJ2, NEWPOINT_ZERO_DIST, NEWPOINT_SCALE, NEWPOINT_NO_DEPTH) = range(1, 13)

class Sim3SearchKeyFrame(C.Structure):   # orbx_sim3_search_keyframe
    _fields_ = [("n", C.c_int32), ("keys_un", C.c_void_p), ("desc", C.c_void_p), ("Tcw", C.c_float * 16), ("has_point", C.c_void_p),
                ("world_pos", C.c_void_p), ("min_distance", C.c_void_p), ("max_distance", C.c_void_p), ("point_desc", C.c_void_p)]


class Sim3SearchProblem(C.Structure):   # orbx_sim3_search_problem
    _fields_ = [("kf1", C.c_int32), ("kf2", C.c_int32), ("s12", C.c_float), ("R12", C.c_float * 9), ("t12", C.c_float * 3),
                ("th", C.c_float), ("matched1", C.c_void_p), ("matched2", C.c_void_p)]


class Sim3SearchDebug(C.Structure):   # orbx_sim3_search_debug
    _fields_ = [("status1", C.c_void_p), ("status2", C.c_void_p), ("best1", C.c_void_p), ("best2", C.c_void_p),
                ("level1", C.c_void_p), ("level2", C.c_void_p), ("uv1", C.c_void_p), ("uv2", C.c_void_p)]


# orbx_search_by_sim3_batch's status bytes (ORBX_SIM3S_*)
(SIM3S_NOT_SEARCHED, SIM3S_BEHIND, SIM3S_OUTSIDE, SIM3S_DISTANCE, SIM3S_NO_CANDIDATE, SIM3S_TOO_FAR, SIM3S_MATCH) = range(7)

TRACK_STATE_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"),
                              ("level", "<i4")])   # orbx_track_state
assert TRACK_STATE_DTYPE.itemsize == 20


class FeatVecView(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("node_id", C.c_void_p), ("begin", C.c_void_p), ("index", C.c_void_p)]


class KeyFrameView(C.Structure):
    _fields_ = [("keys_un", C.c_void_p), ("desc", C.c_void_p), ("n", C.c_int32), ("has_map_point", C.c_void_p),
                ("u_right", C.c_void_p), ("feat_vec", FeatVecView), ("scale_factors", C.c_void_p),
                ("level_sigma2", C.c_void_p)]


class ProjectedPoints(C.Structure):
    _fields_ = [("n", C.c_int32), ("valid", C.c_void_p), ("uv", C.c_void_p), ("u_right", C.c_void_p), ("level", C.c_void_p),
                ("desc", C.c_void_p), ("angle", C.c_void_p)]


class TargetView(C.Structure):
    _fields_ = [("keys_un", C.c_void_p), ("desc", C.c_void_p), ("u_right", C.c_void_p), ("n", C.c_int32),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("scale_factors", C.c_void_p), ("inv_level_sigma2", C.c_void_p)]


class VocabularyView(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("k", C.c_int32), ("L", C.c_int32), ("weighting", C.c_int32), ("scoring", C.c_int32),
                ("child_begin", C.c_void_p), ("child_ids", C.c_void_p), ("desc", C.c_void_p), ("weight", C.c_void_p),
                ("word_id", C.c_void_p)]


class OrbxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"orbx status {status}: {msg}")
        self.status = status


# every symbol include/orbx.h declares (tests/test_abi.py checks the header against this list)
SYMBOLS = [
    "orbx_create", "orbx_destroy", "orbx_default_params", "orbx_last_error", "orbx_status_string",
    "orbx_abi_version", "orbx_get_levels", "orbx_get_scale_factor", "orbx_get_scale_tables",
    "orbx_get_features_per_level", "orbx_get_umax", "orbx_max_keypoints", "orbx_extract", "orbx_extract_batch",
    "orbx_extract_batch_device", "orbx_pyramid_level_info", "orbx_pyramid_level_device",
    "orbx_pyramid_level_copy", "orbx_match_bruteforce_device", "orbx_match_bruteforce", "orbx_hamming_matrix",
    "orbx_get_stream", "orbx_set_stream", "orbx_synchronize", "orbx_profile_enable", "orbx_profile_read",
    "orbx_kernel_name", "orbx_debug_candidates", "orbx_debug_level_keypoints", "orbx_debug_blur_copy", "orbx_debug_fast_groups",
    "orbx_debug_describe_pattern", "orbx_debug_match_plan", "orbx_debug_fast_gpw",
    "orbx_grid_create", "orbx_grid_destroy", "orbx_grid_query", "orbx_three_maxima",
    "orbx_search_for_initialization", "orbx_stereo_match", "orbx_search_by_projection_frame",
    "orbx_search_by_projection_mappoints", "orbx_search_by_projection_frame_batch_device",
    "orbx_search_by_projection_mappoints_batch_device", "orbx_predict_scale_table", "orbx_predict_scale",
    "orbx_search_local_points_batch_device", "orbx_set_input_format", "orbx_search_by_bow_keyframe_frame",
    "orbx_search_by_bow_keyframes", "orbx_search_by_bow_keyframe_frame_batch", "orbx_search_by_bow_keyframes_batch", "orbx_search_for_triangulation", "orbx_triangulation_batch_create", "orbx_triangulation_batch_select", "orbx_triangulation_batch_destroy", "orbx_fuse", "orbx_fuse_sim3", "orbx_fuse_batch", "orbx_fuse_sim3_batch",
    "orbx_search_by_projection_sim3", "orbx_search_by_sim3", "orbx_search_by_projection_keyframe",
    "orbx_stereo_match_batch_device", "orbx_host_alloc", "orbx_host_free", "orbx_set_rectification", "orbx_undistort_keypoints_device",
    "orbx_grid_build_device", "orbx_gated_candidates",
    "orbx_undistort_keypoints", "orbx_image_bounds", "orbx_rgbd_depth_device", "orbx_rgbd_depth", "orbx_extract_rgbd_batch",
    "orbx_vocabulary_create", "orbx_vocabulary_destroy", "orbx_bow_transform", "orbx_bow_transform_device", "orbx_bow_vectors",
    "orbx_vocabulary_scoring", "orbx_bow_score", "orbx_kfdb_create", "orbx_kfdb_destroy", "orbx_kfdb_clear", "orbx_kfdb_size",
    "orbx_kfdb_add", "orbx_kfdb_erase", "orbx_kfdb_score_entries", "orbx_kfdb_query_reloc", "orbx_kfdb_query_loop",
    "orbx_kfdb_query_matches", "orbx_kfdb_query_touched", "orbx_kfdb_select_groups", "orbx_kfdb_state",
    "orbx_distinctive_descriptors_batch", "orbx_distinctive_descriptors_batch_device", "orbx_update_normal_and_depth_batch",
    "orbx_pose_optimization_batch_device", "orbx_pose_optimization", "orbx_pose_sin_cos",
    "orbx_debug_pose_inlier_test",
    "orbx_sim3_ransac_iterations", "orbx_sim3_ransac_batch_create", "orbx_sim3_batch_iterate", "orbx_sim3_batch_best",
    "orbx_sim3_batch_counts", "orbx_sim3_batch_hypothesis", "orbx_sim3_batch_destroy", "orbx_sim3_atan2",
    "orbx_optimize_sim3_batch", "orbx_debug_sim3opt_inlier_test", "orbx_sim3opt_exp",
    "orbx_local_bundle_adjustment_batch", "orbx_debug_localba_classify",
    "orbx_optimize_essential_graph_batch", "orbx_essgraph_log", "orbx_essgraph_sim3_log", "orbx_essgraph_sim3_from_tcw",
    "orbx_pnp_ransac_parameters", "orbx_pnp_ransac_batch_create", "orbx_pnp_batch_iterate", "orbx_pnp_batch_append",
    "orbx_pnp_batch_best", "orbx_pnp_batch_counts", "orbx_pnp_batch_hypothesis", "orbx_pnp_batch_destroy",
    "orbx_init_ransac_batch_create", "orbx_init_batch_result", "orbx_init_batch_scores", "orbx_init_batch_hypothesis",
    "orbx_init_batch_normalization", "orbx_init_batch_destroy",
    "orbx_init_reconstruct_batch_create", "orbx_recon_batch_result", "orbx_recon_batch_hypothesis", "orbx_recon_batch_destroy",
    "orbx_initialize_batch_create",
    "orbx_create_new_map_points_batch", "orbx_newpoints_stereo_cos",
    "orbx_search_by_sim3_batch",
    "orbx_debug_rect_digest",
]

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OrbxError(NO_DEVICE, f"{LIB_PATH} is missing: build it with "
                        "`python -m orb_slam2_detailed_comments_amd.build` (hipcc, gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_float
    L.orbx_create.restype = i32; L.orbx_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    L.orbx_destroy.restype = None; L.orbx_destroy.argtypes = [vp]
    L.orbx_default_params.restype = None; L.orbx_default_params.argtypes = [C.POINTER(Params)]
    L.orbx_last_error.restype = C.c_char_p; L.orbx_last_error.argtypes = []
    L.orbx_status_string.restype = C.c_char_p; L.orbx_status_string.argtypes = [i32]
    L.orbx_abi_version.restype = i32
    L.orbx_get_levels.restype = i32; L.orbx_get_levels.argtypes = [vp]
    L.orbx_get_scale_factor.restype = f32; L.orbx_get_scale_factor.argtypes = [vp]
    L.orbx_get_scale_tables.restype = i32; L.orbx_get_scale_tables.argtypes = [vp, vp, vp, vp, vp]
    L.orbx_get_features_per_level.restype = i32; L.orbx_get_features_per_level.argtypes = [vp, vp]
    L.orbx_get_umax.restype = i32; L.orbx_get_umax.argtypes = [vp, vp]
    L.orbx_max_keypoints.restype = i32; L.orbx_max_keypoints.argtypes = [vp, i32, i32]
    L.orbx_extract.restype = i32; L.orbx_extract.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, C.POINTER(i32)]
    L.orbx_extract_batch.restype = i32
    L.orbx_extract_batch.argtypes = [vp, i32, vp, i32, i32, i32, i64, vp, vp, vp, i32]
    L.orbx_extract_batch_device.restype = i32
    L.orbx_extract_batch_device.argtypes = [vp, i32, vp, i32, i32, i32, i64, vp, vp, vp, vp, i32]
    L.orbx_pyramid_level_info.restype = i32
    L.orbx_pyramid_level_info.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.orbx_pyramid_level_device.restype = i32; L.orbx_pyramid_level_device.argtypes = [vp, i32, i32, C.POINTER(vp)]
    L.orbx_pyramid_level_copy.restype = i32; L.orbx_pyramid_level_copy.argtypes = [vp, i32, i32, vp, i32]
    L.orbx_match_bruteforce_device.restype = i32
    L.orbx_match_bruteforce_device.argtypes = [vp, i32, vp, vp, i64, vp, vp, i64, vp, vp, vp, i32]
    L.orbx_match_bruteforce.restype = i32; L.orbx_match_bruteforce.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp]
    L.orbx_hamming_matrix.restype = i32; L.orbx_hamming_matrix.argtypes = [vp, vp, i32, vp, i32, vp]
    L.orbx_distinctive_descriptors_batch.restype = i32
    L.orbx_distinctive_descriptors_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.orbx_distinctive_descriptors_batch_device.restype = i32
    L.orbx_distinctive_descriptors_batch_device.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp, vp]
    L.orbx_update_normal_and_depth_batch.restype = i32
    L.orbx_update_normal_and_depth_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbx_pose_optimization_batch_device.restype = i32
    L.orbx_pose_optimization_batch_device.argtypes = [vp, i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, f32, vp, i32, vp, vp, vp]
    L.orbx_pose_optimization.restype = i32
    L.orbx_pose_optimization.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp, vp, f32, vp, i32, vp, C.POINTER(i32)]
    L.orbx_debug_pose_inlier_test.restype = i32
    L.orbx_debug_pose_inlier_test.argtypes = [vp, i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, f32, vp, i32, vp, vp, vp, vp]
    L.orbx_pose_sin_cos.restype = None
    L.orbx_pose_sin_cos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.orbx_sim3_ransac_iterations.restype = i32; L.orbx_sim3_ransac_iterations.argtypes = [i32, C.c_double, i32, i32]
    L.orbx_sim3_ransac_batch_create.restype = i32; L.orbx_sim3_ransac_batch_create.argtypes = [vp, i32, vp, C.POINTER(vp)]
    L.orbx_sim3_batch_iterate.restype = i32
    L.orbx_sim3_batch_iterate.argtypes = [vp, i32, i32, C.POINTER(i32), vp, C.POINTER(i32), vp]
    L.orbx_sim3_batch_best.restype = i32; L.orbx_sim3_batch_best.argtypes = [vp, i32, vp, vp, C.POINTER(f32)]
    L.orbx_sim3_batch_counts.restype = i32; L.orbx_sim3_batch_counts.argtypes = [vp, i32, vp, C.POINTER(i32)]
    L.orbx_sim3_batch_hypothesis.restype = i32; L.orbx_sim3_batch_hypothesis.argtypes = [vp, i32, i32, vp, vp]
    L.orbx_sim3_batch_destroy.restype = None; L.orbx_sim3_batch_destroy.argtypes = [vp]
    L.orbx_sim3_atan2.restype = C.c_double; L.orbx_sim3_atan2.argtypes = [C.c_double, C.c_double]
    if hasattr(L, "orbx_optimize_sim3_batch"):   # (absent from an ORBX_LIB build older than the symbols: A/B runs against it)
        L.orbx_optimize_sim3_batch.restype = i32; L.orbx_optimize_sim3_batch.argtypes = [vp, i32, vp, vp]
        L.orbx_debug_sim3opt_inlier_test.restype = i32; L.orbx_debug_sim3opt_inlier_test.argtypes = [vp, i32, vp, vp, vp]
        L.orbx_sim3opt_exp.restype = C.c_double; L.orbx_sim3opt_exp.argtypes = [C.c_double]
    if hasattr(L, "orbx_local_bundle_adjustment_batch"):
        L.orbx_local_bundle_adjustment_batch.restype = i32; L.orbx_local_bundle_adjustment_batch.argtypes = [vp, i32, vp, vp]
        L.orbx_debug_localba_classify.restype = i32; L.orbx_debug_localba_classify.argtypes = [vp, i32, vp, vp, vp]
    if hasattr(L, "orbx_optimize_essential_graph_batch"):
        L.orbx_optimize_essential_graph_batch.restype = i32; L.orbx_optimize_essential_graph_batch.argtypes = [vp, i32, vp, vp]
        L.orbx_essgraph_log.restype = C.c_double; L.orbx_essgraph_log.argtypes = [C.c_double]
        L.orbx_essgraph_sim3_log.restype = None; L.orbx_essgraph_sim3_log.argtypes = [vp, vp]
        L.orbx_essgraph_sim3_from_tcw.restype = None; L.orbx_essgraph_sim3_from_tcw.argtypes = [vp, vp]
    L.orbx_pnp_ransac_parameters.restype = None
    L.orbx_pnp_ransac_parameters.argtypes = [i32, C.c_double, i32, i32, i32, f32, C.POINTER(i32), C.POINTER(i32)]
    L.orbx_pnp_ransac_batch_create.restype = i32; L.orbx_pnp_ransac_batch_create.argtypes = [vp, i32, vp, C.POINTER(vp)]
    L.orbx_pnp_batch_iterate.restype = i32
    L.orbx_pnp_batch_iterate.argtypes = [vp, i32, i32, C.POINTER(i32), vp, C.POINTER(i32), vp]
    L.orbx_pnp_batch_append.restype = i32; L.orbx_pnp_batch_append.argtypes = [vp, i32, i32, vp]
    L.orbx_pnp_batch_best.restype = i32; L.orbx_pnp_batch_best.argtypes = [vp, i32, vp, C.POINTER(i32), C.POINTER(i32)]
    L.orbx_pnp_batch_counts.restype = i32; L.orbx_pnp_batch_counts.argtypes = [vp, i32, vp, C.POINTER(i32)]
    L.orbx_pnp_batch_hypothesis.restype = i32; L.orbx_pnp_batch_hypothesis.argtypes = [vp, i32, i32, vp, vp, C.POINTER(i32), vp]
    L.orbx_pnp_batch_destroy.restype = None; L.orbx_pnp_batch_destroy.argtypes = [vp]
    if hasattr(L, "orbx_init_ransac_batch_create"):   # (absent from an ORBX_LIB build older than the symbols: A/B runs against it)
        L.orbx_init_ransac_batch_create.restype = i32; L.orbx_init_ransac_batch_create.argtypes = [vp, i32, vp, C.POINTER(vp)]
        L.orbx_init_batch_result.restype = i32
        L.orbx_init_batch_result.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.orbx_init_batch_scores.restype = i32; L.orbx_init_batch_scores.argtypes = [vp, i32, i32, vp, C.POINTER(i32)]
        L.orbx_init_batch_hypothesis.restype = i32; L.orbx_init_batch_hypothesis.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
        L.orbx_init_batch_normalization.restype = i32; L.orbx_init_batch_normalization.argtypes = [vp, i32, vp, vp]
        L.orbx_init_batch_destroy.restype = None; L.orbx_init_batch_destroy.argtypes = [vp]
    if hasattr(L, "orbx_init_reconstruct_batch_create"):
        L.orbx_init_reconstruct_batch_create.restype = i32; L.orbx_init_reconstruct_batch_create.argtypes = [vp, i32, vp, C.POINTER(vp)]
        L.orbx_recon_batch_result.restype = i32; L.orbx_recon_batch_result.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.orbx_recon_batch_hypothesis.restype = i32
        L.orbx_recon_batch_hypothesis.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        L.orbx_recon_batch_destroy.restype = None; L.orbx_recon_batch_destroy.argtypes = [vp]
        L.orbx_initialize_batch_create.restype = i32
        L.orbx_initialize_batch_create.argtypes = [vp, i32, vp, vp, C.POINTER(vp), C.POINTER(vp)]
    if hasattr(L, "orbx_create_new_map_points_batch"):   # (absent from an ORBX_LIB build older than the symbols: A/B runs against it)
        L.orbx_create_new_map_points_batch.restype = i32; L.orbx_create_new_map_points_batch.argtypes = [vp, i32, vp, vp, vp]
        L.orbx_newpoints_stereo_cos.restype = f32; L.orbx_newpoints_stereo_cos.argtypes = [f32, f32]
    if hasattr(L, "orbx_search_by_sim3_batch"):   # (absent from an ORBX_LIB build older than the symbol: A/B runs against it)
        L.orbx_search_by_sim3_batch.restype = i32
        L.orbx_search_by_sim3_batch.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.orbx_get_stream.restype = vp; L.orbx_get_stream.argtypes = [vp]
    L.orbx_set_stream.restype = i32; L.orbx_set_stream.argtypes = [vp, vp]
    L.orbx_synchronize.restype = i32; L.orbx_synchronize.argtypes = [vp]
    L.orbx_profile_enable.restype = i32; L.orbx_profile_enable.argtypes = [vp, C.c_uint32]
    L.orbx_profile_read.restype = i32; L.orbx_profile_read.argtypes = [vp, vp, vp, i32]
    L.orbx_kernel_name.restype = C.c_char_p; L.orbx_kernel_name.argtypes = [i32]
    L.orbx_debug_candidates.restype = i32; L.orbx_debug_candidates.argtypes = [vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.orbx_debug_level_keypoints.restype = i32
    L.orbx_debug_level_keypoints.argtypes = [vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.orbx_debug_blur_copy.restype = i32; L.orbx_debug_blur_copy.argtypes = [vp, i32, i32, vp, i32]
    L.orbx_debug_fast_groups.restype = i32; L.orbx_debug_fast_groups.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    if hasattr(L, "orbx_debug_describe_pattern"):   # (absent from an ORBX_LIB build older than the symbol: A/B runs against it)
        L.orbx_debug_describe_pattern.restype = i32; L.orbx_debug_describe_pattern.argtypes = [vp, vp]
    if hasattr(L, "orbx_debug_match_plan"):   # (absent from an ORBX_LIB build older than the symbols: A/B runs against it)
        L.orbx_debug_match_plan.restype = i32; L.orbx_debug_match_plan.argtypes = [vp, i32, i32, C.POINTER(i32), C.POINTER(i32)]
        L.orbx_debug_fast_gpw.restype = i32; L.orbx_debug_fast_gpw.argtypes = [vp, i32, i32, C.POINTER(i32)]
    L.orbx_grid_create.restype = vp; L.orbx_grid_create.argtypes = [vp, i32, f32, f32, f32, f32]
    L.orbx_grid_destroy.restype = None; L.orbx_grid_destroy.argtypes = [vp]
    L.orbx_grid_query.restype = i32; L.orbx_grid_query.argtypes = [vp, f32, f32, f32, i32, i32, vp, i32]
    L.orbx_three_maxima.restype = None
    L.orbx_three_maxima.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.orbx_search_for_initialization.restype = i32
    L.orbx_search_for_initialization.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, f32, i32, vp, C.POINTER(i32)]
    L.orbx_stereo_match.restype = i32
    L.orbx_stereo_match.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, i32, f32, f32, vp, vp, C.POINTER(i32)]
    L.orbx_search_by_projection_frame.restype = i32
    L.orbx_search_by_projection_frame.argtypes = [vp, C.POINTER(FrameView), C.POINTER(LastFrameView), f32, i32, i32, vp,
                                                  C.POINTER(i32)]
    L.orbx_search_by_projection_mappoints.restype = i32
    L.orbx_search_by_projection_mappoints.argtypes = [vp, C.POINTER(FrameView), vp, C.POINTER(MapPointView), f32, f32, vp,
                                                      C.POINTER(i32)]
    L.orbx_search_by_projection_frame_batch_device.restype = i32
    L.orbx_search_by_projection_frame_batch_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, f32, f32,
                                                               i32, vp, vp]
    L.orbx_search_by_projection_mappoints_batch_device.restype = i32
    L.orbx_search_by_projection_mappoints_batch_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, f32, vp, vp]
    L.orbx_predict_scale_table.restype = i32; L.orbx_predict_scale_table.argtypes = [vp, vp, i32]
    L.orbx_predict_scale.restype = i32; L.orbx_predict_scale.argtypes = [vp, f32, f32]
    L.orbx_search_local_points_batch_device.restype = i32
    L.orbx_search_local_points_batch_device.argtypes = [vp, i32, vp, C.POINTER(LocalMapView), i32, vp, vp, vp, vp, i32, vp, vp,
                                                        vp, vp, f32, f32, vp, vp, vp, vp]
    L.orbx_set_input_format.restype = i32; L.orbx_set_input_format.argtypes = [vp, i32]
    L.orbx_search_by_bow_keyframe_frame.restype = i32
    L.orbx_search_by_bow_keyframe_frame.argtypes = [vp, C.POINTER(KeyFrameView), vp, vp, i32, C.POINTER(FeatVecView), f32,
                                                    i32, vp, C.POINTER(i32)]
    L.orbx_search_by_bow_keyframes.restype = i32
    L.orbx_search_by_bow_keyframes.argtypes = [vp, C.POINTER(KeyFrameView), C.POINTER(KeyFrameView), f32, i32, vp,
                                               C.POINTER(i32)]
    L.orbx_search_by_bow_keyframe_frame_batch.restype = i32   # arrays of pointers to the views / output arrays
    L.orbx_search_by_bow_keyframe_frame_batch.argtypes = [vp, i32, vp, vp, vp, i32, C.POINTER(FeatVecView), f32, i32, vp, vp]
    L.orbx_search_by_bow_keyframes_batch.restype = i32
    L.orbx_search_by_bow_keyframes_batch.argtypes = [vp, C.POINTER(KeyFrameView), i32, vp, f32, i32, vp, vp]
    L.orbx_search_for_triangulation.restype = i32
    L.orbx_search_for_triangulation.argtypes = [vp, C.POINTER(KeyFrameView), C.POINTER(KeyFrameView), vp, f32, f32, i32,
                                                i32, vp, C.POINTER(i32)]
    L.orbx_triangulation_batch_create.restype = i32
    L.orbx_triangulation_batch_create.argtypes = [vp, C.POINTER(KeyFrameView), i32, vp, C.POINTER(vp)]
    L.orbx_triangulation_batch_select.restype = i32
    L.orbx_triangulation_batch_select.argtypes = [vp, i32, C.POINTER(KeyFrameView), C.POINTER(KeyFrameView), vp, f32, f32, i32, i32, vp, C.POINTER(i32)]
    L.orbx_triangulation_batch_destroy.restype = None; L.orbx_triangulation_batch_destroy.argtypes = [vp]
    PT, TV = C.POINTER(ProjectedPoints), C.POINTER(TargetView)
    L.orbx_fuse.restype = i32; L.orbx_fuse.argtypes = [vp, TV, PT, f32, vp, C.POINTER(i32)]
    L.orbx_fuse_sim3.restype = i32; L.orbx_fuse_sim3.argtypes = [vp, TV, PT, f32, vp, C.POINTER(i32)]
    for fn in (L.orbx_fuse_batch, L.orbx_fuse_sim3_batch):   # arrays of pointers to the views / output arrays
        fn.restype = i32; fn.argtypes = [vp, i32, vp, vp, f32, vp, vp]
    L.orbx_search_by_projection_sim3.restype = i32
    L.orbx_search_by_projection_sim3.argtypes = [vp, TV, PT, i32, vp, vp, C.POINTER(i32)]
    L.orbx_search_by_sim3.restype = i32; L.orbx_search_by_sim3.argtypes = [vp, TV, TV, PT, PT, f32, vp, C.POINTER(i32)]
    L.orbx_search_by_projection_keyframe.restype = i32
    L.orbx_search_by_projection_keyframe.argtypes = [vp, TV, PT, f32, i32, i32, vp, vp, C.POINTER(i32)]
    L.orbx_vocabulary_create.restype = i32; L.orbx_vocabulary_create.argtypes = [vp, C.POINTER(VocabularyView), C.POINTER(vp)]
    L.orbx_vocabulary_destroy.restype = None; L.orbx_vocabulary_destroy.argtypes = [vp]
    L.orbx_bow_transform.restype = i32; L.orbx_bow_transform.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    L.orbx_bow_transform_device.restype = i32
    L.orbx_bow_transform_device.argtypes = [vp, vp, i32, vp, vp, i64, i32, i32, vp, vp, i32]
    L.orbx_bow_vectors.restype = i32
    L.orbx_bow_vectors.argtypes = [vp, vp, vp, vp, i32, vp, vp, C.POINTER(i32), vp, vp, vp, C.POINTER(i32)]
    L.orbx_stereo_match_batch_device.restype = i32
    L.orbx_stereo_match_batch_device.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, f32, f32, vp, vp, vp]
    L.orbx_undistort_keypoints_device.restype = i32
    L.orbx_undistort_keypoints_device.argtypes = [vp, i32, vp, vp, i32, vp, vp, i32, vp]
    L.orbx_grid_build_device.restype = i32
    L.orbx_grid_build_device.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp]
    L.orbx_gated_candidates.restype = i32
    L.orbx_gated_candidates.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp]
    L.orbx_undistort_keypoints.restype = i32; L.orbx_undistort_keypoints.argtypes = [vp, vp, i32, vp, vp, i32, vp]
    L.orbx_image_bounds.restype = i32; L.orbx_image_bounds.argtypes = [vp, i32, i32, vp, vp, i32, vp]
    L.orbx_set_rectification.restype = i32; L.orbx_set_rectification.argtypes = [vp, vp, vp, i32, i32]
    if hasattr(L, "orbx_debug_rect_digest"):   # (absent from an ORBX_LIB build older than the symbol: A/B runs against it)
        L.orbx_debug_rect_digest.restype = i32; L.orbx_debug_rect_digest.argtypes = [vp, vp, i64, vp, vp]
    L.orbx_rgbd_depth_device.restype = i32
    L.orbx_rgbd_depth_device.argtypes = [vp, i32, vp, vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, i64, f32, f32, vp, vp, vp]
    L.orbx_rgbd_depth.restype = i32
    L.orbx_rgbd_depth.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, i32, f32, f32, vp, vp]
    L.orbx_extract_rgbd_batch.restype = i32
    L.orbx_extract_rgbd_batch.argtypes = [vp, i32, vp, i32, i32, i32, i64, vp, i32, i32, i64, f32, vp, vp, i32, f32,
                                          vp, vp, vp, vp, vp, vp, i32]
    L.orbx_vocabulary_scoring.restype = i32; L.orbx_vocabulary_scoring.argtypes = [vp]
    L.orbx_bow_score.restype = i32; L.orbx_bow_score.argtypes = [vp, i32, vp, vp, i32, vp, vp, i32, C.POINTER(C.c_double)]
    L.orbx_kfdb_create.restype = i32; L.orbx_kfdb_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.orbx_kfdb_destroy.restype = None; L.orbx_kfdb_destroy.argtypes = [vp]
    L.orbx_kfdb_clear.restype = i32; L.orbx_kfdb_clear.argtypes = [vp]
    L.orbx_kfdb_size.restype = i32; L.orbx_kfdb_size.argtypes = [vp]
    L.orbx_kfdb_add.restype = i32; L.orbx_kfdb_add.argtypes = [vp, i64, vp, vp, i32]
    L.orbx_kfdb_erase.restype = i32; L.orbx_kfdb_erase.argtypes = [vp, i64]
    L.orbx_kfdb_score_entries.restype = i32; L.orbx_kfdb_score_entries.argtypes = [vp, vp, vp, i32, vp, i32, vp]
    L.orbx_kfdb_query_reloc.restype = i32; L.orbx_kfdb_query_reloc.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.orbx_kfdb_query_loop.restype = i32; L.orbx_kfdb_query_loop.argtypes = [vp, i64, vp, vp, i32, vp, i32, f32, vp, vp]
    L.orbx_kfdb_query_matches.restype = i32; L.orbx_kfdb_query_matches.argtypes = [vp, i32, vp, vp, i32, C.POINTER(i32)]
    L.orbx_kfdb_query_touched.restype = i32; L.orbx_kfdb_query_touched.argtypes = [vp, i32, vp, i32, C.POINTER(i32)]
    L.orbx_kfdb_select_groups.restype = i32
    L.orbx_kfdb_select_groups.argtypes = [vp, i32, vp, vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.orbx_kfdb_state.restype = i32
    L.orbx_kfdb_state.argtypes = [vp, i64, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(f32), C.POINTER(i32)]
    L.orbx_host_alloc.restype = vp; L.orbx_host_alloc.argtypes = [C.c_size_t]
    L.orbx_host_free.restype = None; L.orbx_host_free.argtypes = [vp]
    _lib = L
    return L


def check(status, allow=()):
    if status != OK and status not in allow:
        raise OrbxError(status, lib().orbx_last_error().decode(errors="replace"))
    return status


def ptr(a):
    """numpy array -> void*, torch tensor / int -> device address"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if isinstance(a, int):
        return C.c_void_p(a)
    return C.c_void_p(a.data_ptr())


class PinnedArray:
    """numpy view of page-locked host memory (orbx_host_alloc); keep the object alive as long as the array is used"""

    def __init__(self, shape, dtype=np.uint8):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._p = lib().orbx_host_alloc(self.nbytes)
        if not self._p:
            raise MemoryError("orbx_host_alloc failed")
        self.array = np.frombuffer((C.c_uint8 * self.nbytes).from_address(self._p), dtype=dtype).reshape(shape)

    def __del__(self):
        if getattr(self, "_p", None):
            try:
                lib().orbx_host_free(self._p)
            except Exception:
                pass
            self._p = None
