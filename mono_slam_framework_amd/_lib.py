"""ctypes view of include/msf_abi.h, include/msf_initializer.h, include/msf_local_mapping.h, include/msf_pnp.h, include/msf_pose.h, include/msf_ba.h, include/msf_global_ba.h, include/msf_tracking.h and include/msf_frame_tracking.h.  Loading fails loudly when libmsf.so is missing: there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import build as _build
from . import results

MSF_OK = 0
MSF_ERR_INVALID_ARG = -1
MSF_ERR_HIP = -2
MSF_ERR_UNSUPPORTED = -3
MSF_ERR_CAPACITY = -4
MSF_ERR_IO = -5

MSF_KIND_ORB = 0
MSF_KIND_LOFTR = 1

MSF_FLAG_BLUR_TIE_HALF_UP = 1
MSF_FLAG_PROFILE = 2
MSF_FLAG_KEEP_DEBUG = 4
MSF_FLAG_FAST_DENSE = 8
MSF_FLAG_NO_FRAME_CACHE = 16
MSF_FLAG_LEVEL_SIZE_MUL_INV = 32
MSF_FLAG_FAST_STREAM = 64
MSF_FLAG_LOFTR_F32 = 128
MSF_FLAG_BLUR_SUM256 = 256

(DBG_LEVEL_SIZES, DBG_LEVEL_PIXELS, DBG_FAST_CANDS, DBG_KEYPOINTS, DBG_DESCRIPTORS, DBG_STAGE1,
 DBG_LOFTR_CONF, DBG_LOFTR_FEAT, DBG_FAST_TAU, DBG_LOFTR_ACT, DBG_WALK_MODE, DBG_LOFTR_TOK,
 DBG_ORB_MATCH_FORM, DBG_WALK_FINISHED) = range(14)

# every symbol include/msf_abi.h declares
ABI_SYMBOLS = ["msf_abi_version", "msf_default_config", "msf_create", "msf_destroy", "msf_set_threshold",
               "msf_last_error", "msf_match_pair", "msf_match_batch", "msf_match_batch_device",
               "msf_extract_device", "msf_match_slots_device", "msf_pack_matches_device", "msf_debug_get",
               "msf_debug_loftr_head", "msf_debug_loftr_transformer", "msf_debug_loftr_backbone",
               "msf_debug_orb_set_features", "msf_debug_orb_tail",
               "msf_stage_times", "msf_set_mappoints", "msf_count_mappoint_matches_device",
               "msf_store_frame", "msf_match_one_to_many", "msf_check_hypotheses",
               "msf_find_models", "msf_find_models_device",
               "msf_render_match_image", "msf_weights_info", "msf_convert_weights",
               "msf_frame_cache_stats", "msf_multi_create", "msf_multi_destroy", "msf_multi_device_count",
               "msf_multi_handle", "msf_multi_set_threshold", "msf_multi_last_error", "msf_multi_shard_range",
               "msf_multi_match_batch", "msf_multi_match_batch_device",
               "msf_gather_unique_id", "msf_gather_create", "msf_gather_destroy", "msf_gather_last_error",
               "msf_gather_plan", "msf_gather_matches_device"]

# every symbol include/msf_initializer.h declares (a header and a version of its own: MSF_ABI_VERSION stays what it is)
INITIALIZER_SYMBOLS = ["msf_initializer_version", "msf_reconstruct", "msf_reconstruct_device"]

# every symbol include/msf_local_mapping.h declares (again a header and a version of its own)
LOCAL_MAPPING_SYMBOLS = ["msf_local_mapping_version", "msf_new_points", "msf_new_points_device", "msf_create_map_points"]

# every symbol include/msf_pnp.h declares (again a header and a version of its own)
PNP_SYMBOLS = ["msf_pnp_version", "msf_pnp_ransac", "msf_pnp_ransac_device"]

# every symbol include/msf_pose.h declares (again a header and a version of its own)
POSE_SYMBOLS = ["msf_pose_version", "msf_pose_optimize", "msf_pose_optimize_device"]

# every symbol include/msf_ba.h declares (again a header and a version of its own)
BA_SYMBOLS = ["msf_ba_version", "msf_bundle_adjust", "msf_bundle_adjust_device"]

# every symbol include/msf_global_ba.h declares (again a header and a version of its own)
GLOBAL_BA_SYMBOLS = ["msf_global_ba_version", "msf_global_ba_tile_rows", "msf_global_bundle_adjust",
                     "msf_global_bundle_adjust_device"]
GBA_MAX_FREE_CAMS = 1024

# every symbol include/msf_tracking.h declares (again a header and a version of its own)
TRACKING_SYMBOLS = ["msf_tracking_version", "msf_frustum", "msf_frustum_device", "msf_claim_points_device",
                    "msf_search_local_points"]
MSF_POINT_BAD, MSF_POINT_SEEN = 1, 2
MSF_SEARCH_KEEP_ON_DEVICE = 1

# every symbol include/msf_frame_tracking.h declares.  The msf_ names are closed with msf_tracking.h: the entry points of
# every later header carry the prefix msfx_
FRAME_TRACKING_SYMBOLS = ["msfx_frame_tracking_version", "msfx_carry_points_device", "msfx_track_list_device",
                          "msfx_track_frame"]
MSFX_TRACK_MAX_CANDIDATES = 8192
MSFX_TRACK_KEEP_ON_DEVICE = 1


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("device", C.c_int32), ("threshold", C.c_float),
                ("image_width", C.c_int32), ("image_height", C.c_int32), ("max_batch_pairs", C.c_int32),
                ("flags", C.c_uint32), ("weights_path", C.c_char_p)]


class Image(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int64)]


# msf_ransac_result's arrays in declaration order (rows as in the tables below): the homography's result has no fn, the
# fundamental's no m12; best starts at -1
RANSAC_ARRAYS = [("m21", "float32", "hyp", (3, 3)), ("m12", "float32", "hyp", (3, 3)), ("fn", "float32", "hyp", (3, 3)),
                 ("null_vec", "float32", "hyp", (3, 3)), ("scores", "float32", "hyp", ()), ("best", "int32", "list", ()),
                 ("best_inliers", "uint8", "list", ("cap",)), ("T1", "float32", "list", (3, 3)),
                 ("T2", "float32", "list", (3, 3))]


class RansacResult(C.Structure):
    """msf_ransac_result: host pointers for msf_find_models, device pointers inside a RansacBatch"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(a[0], C.c_void_p) for a in RANSAC_ARRAYS]


def ransac_shapes(lists, n_hyp, cap):
    """-> {name: (shape, dtype name)} of msf_ransac_result's arrays"""
    return results.shapes(RANSAC_ARRAYS, {"list": (lists,), "hyp": (lists, n_hyp)}, cap)


class RansacBatch(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("sets", C.c_void_p),
                ("homography", RansacResult), ("fundamental", RansacResult)]


class MotionParams(C.Structure):
    """msf_motion_params: Initializer(K, sigma) + Initialize(..., minTriangulated, minParallax)"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("K", C.c_float * 9), ("sigma", C.c_float),
                ("min_triangulated", C.c_int32), ("min_parallax", C.c_float)]


# The result structs' arrays in declaration order: (name, dtype, per, trailing shape) with `per` the leading unit after
# [n_lists] ("list": none) and "cap" the lists' stride; csrc/result_arrays.h holds the same tables for the library
# (tests/test_result_arrays_host.py compares them).  A 3 x 3 matrix is (3, 3) here and nine floats there.
MOTION_ARRAYS = [("ok", "int32", "list", ()), ("model", "int32", "list", ()), ("R21", "float32", "list", (3, 3)),
                 ("t21", "float32", "list", (3,)), ("points", "float32", "list", ("cap", 3)),
                 ("triangulated", "uint8", "list", ("cap",)), ("n_cand", "int32", "list", ()),
                 ("cand_R", "float32", "list", (8, 3, 3)), ("cand_t", "float32", "list", (8, 3)),
                 ("cand_good", "int32", "list", (8,)), ("cand_parallax", "float32", "list", (8,)),
                 ("winner", "int32", "list", ())]


class MotionResult(C.Structure):
    """msf_motion_result: host pointers for msf_reconstruct, device pointers [n_lists] for msf_reconstruct_device"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(a[0], C.c_void_p) for a in MOTION_ARRAYS]


def list_shapes(table, lists, cap):
    """-> {name: (shape, dtype)} of msf_motion_result's (MOTION_ARRAYS) or msf_new_points_result's (NEW_POINTS_ARRAYS) arrays"""
    return results.shapes(table, {"list": (lists,)}, cap)


class View(C.Structure):
    """msf_view: a key frame's pose and intrinsics"""
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float)]


class NewPointsParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("max_cos_parallax", C.c_double),
                ("chi2", C.c_double)]


NEW_POINT_DTYPE = np.dtype([("match", "<i4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
NEW_POINTS_ARRAYS = [("n_new", "int32", "list", ()), ("packed", NEW_POINT_DTYPE, "list", ("cap",)),
                     ("status", "uint8", "list", ("cap",)), ("points", "float32", "list", ("cap", 3)),
                     ("hom", "float32", "list", ("cap", 4)), ("cos_parallax", "float64", "list", ("cap",))]


class NewPointsResult(C.Structure):
    """msf_new_points_result: host pointers for msf_new_points / msf_create_map_points, device pointers for
    msf_new_points_device"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(a[0], C.c_void_p) for a in NEW_POINTS_ARRAYS]


class PnpParams(C.Structure):
    """msf_pnp_params: the current frame's intrinsics and SetRansacParameters' values after its adjustment"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("th2", C.c_float), ("min_inliers", C.c_int32),
                ("n_iterations", C.c_int32), ("max_records", C.c_int32), ("seed", C.c_uint64)]


# msf_pnp_result's arrays in declaration order: name -> (dtype, per "hyp" / "rec" / "list", trailing shape; "cap" = the lists' stride)
PNP_ARRAYS = [("n_records", "int32", "list", ()), ("counts", "int32", "hyp", ()),
              ("iteration", "int32", "rec", ()), ("n_inliers", "int32", "rec", ()), ("refined_ok", "int32", "rec", ()),
              ("n_refined", "int32", "rec", ()), ("Tcw_best", "float32", "rec", (12,)), ("Tcw_refined", "float32", "rec", (12,)),
              ("inliers_best", "uint8", "rec", ("cap",)), ("inliers_refined", "uint8", "rec", ("cap",)),
              ("sets", "int32", "hyp", (4,)), ("pose_f64", "float64", "hyp", (12,)), ("cws", "float64", "hyp", (4, 3)),
              ("ut_tail", "float64", "hyp", (4, 12)), ("betas", "float64", "hyp", (3, 4)), ("rep_errors", "float64", "hyp", (3,)),
              ("pca", "float64", "hyp", (3, 3)),
              ("rec_pose_f64", "float64", "rec", (12,)), ("rec_cws", "float64", "rec", (4, 3)),
              ("rec_ut_tail", "float64", "rec", (4, 12)), ("rec_betas", "float64", "rec", (3, 4)),
              ("rec_rep_errors", "float64", "rec", (3,)), ("rec_pca", "float64", "rec", (3, 3))]


class PnpResult(C.Structure):
    """msf_pnp_result: host pointers for msf_pnp_ransac, device pointers for msf_pnp_ransac_device"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(a[0], C.c_void_p) for a in PNP_ARRAYS]


def pnp_shapes(lists, n_iterations, max_records, cap):
    """-> {name: (shape, dtype name)} of msf_pnp_result's arrays"""
    return results.shapes(PNP_ARRAYS, {"list": (lists,), "hyp": (lists, n_iterations), "rec": (lists, max_records)}, cap)


class PoseParams(C.Structure):
    """msf_pose_params: the frame's intrinsics and chi2Mono"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("chi2", C.c_float)]


# msf_pose_result's arrays in declaration order: name -> (dtype, per "list" / "round" / "it", trailing shape; "cap" = the lists' stride)
POSE_ARRAYS = [("n_good", "int32", "list", ()), ("Tcw", "float32", "list", (12,)), ("outliers", "uint8", "list", ("cap",)),
               ("n_edges", "int32", "list", ()), ("rounds_run", "int32", "list", ()), ("pose_f64", "float64", "list", (12,)),
               ("round_pose_f64", "float64", "round", (12,)), ("round_n_bad", "int32", "round", ()),
               ("round_iterations", "int32", "round", ()),
               ("it_trials", "int32", "it", ()), ("it_lambda_in", "float64", "it", ()), ("it_lambda_out", "float64", "it", ()),
               ("it_cost_in", "float64", "it", ()), ("it_cost_out", "float64", "it", ()), ("it_H", "float64", "it", (21,)),
               ("it_b", "float64", "it", (6,)), ("it_pose_out", "float64", "it", (7,))]


class PoseResult(C.Structure):
    """msf_pose_result: host pointers for msf_pose_optimize, device pointers for msf_pose_optimize_device"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(a[0], C.c_void_p) for a in POSE_ARRAYS]


def pose_shapes(lists, cap):
    """-> {name: (shape, dtype name)} of msf_pose_result's arrays"""
    return results.shapes(POSE_ARRAYS, {"list": (lists,), "round": (lists, 4), "it": (lists, 4, 10)}, cap)


class BaParams(C.Structure):
    """msf_ba_params: the intrinsics and the schedule of up to two rounds"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("n_rounds", C.c_int32), ("iterations", C.c_int32 * 2),
                ("robust", C.c_int32 * 2), ("huber_delta2", C.c_double), ("chi2", C.c_double)]


BA_SLOTS = 64
BA_PROBLEM_DTYPE = np.dtype([("n_cams", "<i4"), ("n_points", "<i4"), ("n_edges", "<i4"), ("cam0", "<i4"), ("point0", "<i4"),
                             ("edge0", "<i4")])
# msf_ba_result's arrays in declaration order: name -> (dtype, per "problem" / "cam" / "point" / "edge" / "round" / "it" /
# "it_cam" / "it_point", trailing shape)
BA_ARRAYS = [("status", "int32", "problem", ()), ("cam_Tcw", "float32", "cam", (12,)), ("points", "float32", "point", (3,)),
             ("outliers", "uint8", "edge", ()), ("cam_pose_f64", "float64", "cam", (12,)), ("points_f64", "float64", "point", (3,)),
             ("round_flags", "uint8", "edge", (2,)), ("round_iterations", "int32", "round", ()),
             ("it_trials", "int32", "it", ()), ("it_lambda_in", "float64", "it", ()), ("it_lambda_out", "float64", "it", ()),
             ("it_cost_in", "float64", "it", ()), ("it_cost_out", "float64", "it", ()),
             ("it_cam_in", "float64", "it_cam", (7,)), ("it_point_in", "float64", "it_point", (3,)),
             ("it_cam_out", "float64", "it_cam", (7,)), ("it_point_out", "float64", "it_point", (3,)),
             ("it_Hcc", "float64", "it_cam", (21,)), ("it_bc", "float64", "it_cam", (6,)),
             ("it_Hpp", "float64", "it_point", (6,)), ("it_bp", "float64", "it_point", (3,))]


class BaResult(C.Structure):
    """msf_ba_result: host pointers for msf_bundle_adjust, device pointers for msf_bundle_adjust_device"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(a[0], C.c_void_p) for a in BA_ARRAYS]


def ba_shapes(problems, cams, points, edges):
    """-> {name: (shape, dtype name)} of msf_ba_result's arrays for a call of `problems` problems with `cams`, `points`
    and `edges` rows in all.  A problem's block of a per-iteration array starts at row 64 * cam0 (64 * point0) of the
    flat [64 * cams] ([64 * points]) rows and is [64][n_cams] ([64][n_points])."""
    lead = {"problem": (problems,), "cam": (cams,), "point": (points,), "edge": (edges,), "round": (problems, 2),
            "it": (problems, BA_SLOTS), "it_cam": (BA_SLOTS * cams,), "it_point": (BA_SLOTS * points,)}
    return results.shapes(BA_ARRAYS, lead)


class LocalMap(C.Structure):
    """msf_local_map: host pointers for msf_frustum / msf_search_local_points, device pointers for the *_device calls"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_points", C.c_int32), ("n_kf", C.c_int32),
                ("n_entries", C.c_int32), ("n_cur", C.c_int32), ("points", C.c_void_p), ("kf_start", C.c_void_p),
                ("kf_key", C.c_void_p), ("kf_point", C.c_void_p), ("cur_key", C.c_void_p), ("cur_point", C.c_void_p)]


class FrustumParams(C.Structure):
    """msf_frustum_params: the current frame's view, camera centre, image bounds and viewing-cosine limit"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("view", View), ("Ow", C.c_float * 3),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("viewing_cos_limit", C.c_float)]


class DeviceCorr(C.Structure):
    """msf_device_corr: where msf_search_local_points left the correspondences with MSF_SEARCH_KEEP_ON_DEVICE"""
    _fields_ = [("struct_size", C.c_uint32), ("corr_cap", C.c_int32), ("d_corr_p3d", C.c_void_p),
                ("d_corr_p2d", C.c_void_p), ("d_corr_point", C.c_void_p), ("d_n_corr", C.c_void_p)]


MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("max_distance", "<f4"), ("flags", "<u4")])
LOCAL_CLAIM_DTYPE = np.dtype([("key", "<i4"), ("point", "<i4"), ("kf", "<i4"), ("match", "<i4")])
# msf_frustum_result's / msf_claim_result's arrays in declaration order: (name, dtype, per "call" / "point" / "kf" /
# "corr", trailing shape; "cap" = the lists' stride); csrc/tracking_arrays.h holds the same tables
# (tests/test_tracking_arrays_host.py compares them)
FRUSTUM_ARRAYS = [("status_word", "int32", "call", ()), ("n_to_match", "int32", "kf", ()), ("status", "uint8", "point", ()),
                  ("visible", "uint8", "point", ()), ("owner_kf", "int32", "point", ()), ("u", "float32", "point", ()),
                  ("v", "float32", "point", ()), ("dist", "float32", "point", ()), ("view_cos", "float32", "point", ())]
CLAIM_ARRAYS = [("status_word", "int32", "call", ()), ("n_claims", "int32", "call", ()), ("n_claimed", "int32", "kf", ()),
                ("claims", LOCAL_CLAIM_DTYPE, "kf", ("cap",)), ("claim_status", "uint8", "kf", ("cap",)),
                ("n_corr", "int32", "call", ()), ("corr_p3d", "float32", "corr", (3,)), ("corr_p2d", "float32", "corr", (2,)),
                ("corr_point", "int32", "corr", ())]


class FrustumResult(C.Structure):
    """msf_frustum_result: host pointers for msf_frustum / msf_search_local_points, device pointers for msf_frustum_device"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(a[0], C.c_void_p) for a in FRUSTUM_ARRAYS]


class ClaimResult(C.Structure):
    """msf_claim_result: device pointers for msf_claim_points_device, host pointers for msf_search_local_points"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(a[0], C.c_void_p) for a in CLAIM_ARRAYS]


def tracking_shapes(table, points, kfs, cap, corr_cap):
    """-> {name: (shape, dtype)} of msf_frustum_result's (FRUSTUM_ARRAYS) or msf_claim_result's (CLAIM_ARRAYS) arrays"""
    return results.shapes(table, {"call": (1,), "point": (points,), "kf": (kfs,), "corr": (corr_cap,)}, cap)


class FrameMap(C.Structure):
    """msfx_frame_map: host pointers for msfx_track_frame, device pointers for the *_device calls"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_points", C.c_int32), ("n_ref", C.c_int32),
                ("n_cur", C.c_int32), ("reserved2", C.c_int32), ("points", C.c_void_p), ("observed", C.c_void_p),
                ("ref_key", C.c_void_p), ("ref_point", C.c_void_p), ("cur_key", C.c_void_p), ("cur_point", C.c_void_p)]


class TrackParams(C.Structure):
    """msfx_track_params: the optimiser's parameters, the entry pose and the two thresholds"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("pose", PoseParams), ("Tcw0", C.c_float * 12),
                ("min_matches", C.c_int32), ("min_map_matches", C.c_int32)]


FRAME_POINT_DTYPE = np.dtype([("key", "<i4"), ("point", "<i4"), ("match", "<i4"), ("flags", "<i4")])
REMOVED_POINT_DTYPE = np.dtype([("key", "<i4"), ("point", "<i4")])
# msfx_track_result's arrays in declaration order: (name, dtype, per "call" / "match" / "cur" / "corr", trailing shape);
# csrc/frame_tracking_arrays.h holds the same table (tests/test_frame_tracking_arrays_host.py compares them)
TRACK_ARRAYS = [("track_status", "int32", "call", ()), ("n_map", "int32", "call", ()), ("map", FRAME_POINT_DTYPE, "corr", ()),
                ("carry_status", "uint8", "match", ()), ("cur_status", "uint8", "cur", ()),
                ("corr_p3d", "float32", "corr", (3,)), ("corr_p2d", "float32", "corr", (2,)), ("corr_point", "int32", "corr", ()),
                ("Tcw", "float32", "call", (12,)), ("n_good", "int32", "call", ()), ("n_kept", "int32", "call", ()),
                ("kept_key", "int32", "corr", ()), ("kept_point", "int32", "corr", ()), ("n_removed", "int32", "call", ()),
                ("removed", REMOVED_POINT_DTYPE, "corr", ()), ("n_matches_map", "int32", "call", ())]
CARRY_NAMES = tuple(a[0] for a in TRACK_ARRAYS[:8])   # what msfx_carry_points_device writes


class TrackResult(C.Structure):
    """msfx_track_result: device pointers for the *_device calls, host pointers for msfx_track_frame"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(a[0], C.c_void_p) for a in TRACK_ARRAYS]


class DeviceTrack(C.Structure):
    """msfx_device_track: where msfx_track_frame left its results with MSFX_TRACK_KEEP_ON_DEVICE"""
    _fields_ = [("struct_size", C.c_uint32), ("corr_cap", C.c_int32)] + [(n, C.c_void_p) for n in (
        "d_track_status", "d_n_kept", "d_kept_key", "d_kept_point", "d_n_map", "d_corr_p3d", "d_corr_p2d", "d_corr_point",
        "d_outliers", "d_Tcw")]


def track_shapes(cap, n_cur, corr_cap):
    """-> {name: (shape, dtype)} of msfx_track_result's arrays; "call" arrays are [1, ...]"""
    return results.shapes(TRACK_ARRAYS, {"call": (1,), "match": (cap,), "cur": (n_cur,), "corr": (corr_cap,)})


VIEW_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4")])
MATCH_DTYPE = np.dtype([("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4")])
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("angle", "<f4"),
                     ("octave", "<i4"), ("lx", "<i4"), ("ly", "<i4"), ("fast_score", "<i4")])

_lib = None


def load():
    """Loads libmsf.so (after torch, if torch is importable, so both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  (torch bundles its own libamdhip64.so.7; load it first)
    except Exception:  # pragma: no cover
        pass
    path = _build.lib_path()
    L = C.CDLL(path, mode=C.RTLD_GLOBAL if hasattr(C, "RTLD_GLOBAL") else 0)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    L.msf_abi_version.restype = C.c_int
    L.msf_default_config.argtypes = [C.POINTER(Config), C.c_int]
    L.msf_default_config.restype = None
    L.msf_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.msf_destroy.argtypes = [vp]
    L.msf_destroy.restype = None
    L.msf_set_threshold.argtypes = [vp, f32]
    L.msf_last_error.argtypes = [vp]
    L.msf_last_error.restype = C.c_char_p
    L.msf_match_pair.argtypes = [vp, C.POINTER(Image), C.POINTER(Image), vp, i32, C.POINTER(i32)]
    L.msf_match_batch.argtypes = [vp, i32, C.POINTER(Image), C.POINTER(Image), vp, i32, vp]
    L.msf_match_batch_device.argtypes = [vp, i32, vp, vp, i64, i64, vp, i32, vp, vp]
    L.msf_extract_device.argtypes = [vp, i32, vp, i64, i64, i32, vp]
    L.msf_match_slots_device.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp]
    L.msf_pack_matches_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp]
    L.msf_debug_get.argtypes = [vp, i32, i32, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.msf_debug_loftr_head.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp]
    L.msf_debug_loftr_transformer.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.msf_debug_loftr_backbone.argtypes = [vp, i32, vp, vp, i64, i64, i32, vp, vp, vp]
    L.msf_debug_orb_set_features.argtypes = [vp, i32, i32, vp, vp]
    L.msf_debug_orb_tail.argtypes = [vp, i32, vp, i64, i64, i32, vp, vp, i32]
    L.msf_set_mappoints.argtypes = [vp, i32, vp, i32]
    L.msf_count_mappoint_matches_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.msf_store_frame.argtypes = [vp, i32, C.POINTER(Image)]
    L.msf_match_one_to_many.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32]
    L.msf_check_hypotheses.argtypes = [vp, i32, i32, vp, vp, i32, vp, f32, vp, C.POINTER(i32), vp]
    L.msf_find_models.argtypes = [vp, i32, vp, i32, vp, f32, C.POINTER(RansacResult), C.POINTER(RansacResult)]
    L.msf_find_models_device.argtypes = [vp, i32, vp, i32, vp, i32, C.c_uint64, f32, C.POINTER(RansacBatch), vp]
    L.msf_initializer_version.restype = C.c_int
    L.msf_reconstruct.argtypes = [vp, i32, vp, i32, vp, vp, C.POINTER(MotionParams), C.POINTER(MotionResult)]
    L.msf_reconstruct_device.argtypes = [vp, i32, vp, i32, vp, i32, C.POINTER(RansacBatch), C.POINTER(MotionParams),
                                         C.POINTER(MotionResult), vp]
    L.msf_local_mapping_version.restype = C.c_int
    L.msf_new_points.argtypes = [vp, i32, vp, vp, vp, C.POINTER(NewPointsParams), C.POINTER(NewPointsResult)]
    L.msf_new_points_device.argtypes = [vp, i32, vp, i32, vp, vp, vp, C.POINTER(NewPointsParams),
                                        C.POINTER(NewPointsResult), vp]
    L.msf_create_map_points.argtypes = [vp, i32, vp, i32, vp, vp, C.POINTER(NewPointsParams), vp, vp, i32,
                                        C.POINTER(NewPointsResult)]
    L.msf_pnp_version.restype = C.c_int
    L.msf_pnp_ransac.argtypes = [vp, i32, vp, vp, C.POINTER(PnpParams), vp, C.POINTER(PnpResult)]
    L.msf_pnp_ransac_device.argtypes = [vp, i32, vp, vp, i32, vp, C.POINTER(PnpParams), vp, C.POINTER(PnpResult), vp]
    L.msf_pose_version.restype = C.c_int
    L.msf_pose_optimize.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(PoseParams), C.POINTER(PoseResult)]
    L.msf_pose_optimize_device.argtypes = [vp, i32, vp, vp, i32, vp, vp, i64, vp, i64, C.POINTER(PoseParams),
                                           C.POINTER(PoseResult), vp]
    L.msf_ba_version.restype = C.c_int
    L.msf_bundle_adjust.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, C.POINTER(BaParams), C.POINTER(BaResult)]
    L.msf_bundle_adjust_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, vp,
                                           C.POINTER(BaParams), C.POINTER(BaResult), vp]
    L.msf_global_ba_version.restype = C.c_int
    L.msf_global_ba_tile_rows.restype = C.c_int
    L.msf_global_bundle_adjust.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, C.POINTER(BaParams), C.POINTER(BaResult)]
    L.msf_global_bundle_adjust_device.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, C.POINTER(BaParams),
                                                  C.POINTER(BaResult), vp]
    L.msf_tracking_version.restype = C.c_int
    L.msf_frustum.argtypes = [vp, C.POINTER(LocalMap), C.POINTER(FrustumParams), C.POINTER(FrustumResult)]
    L.msf_frustum_device.argtypes = [vp, C.POINTER(LocalMap), C.POINTER(FrustumParams), C.POINTER(FrustumResult), vp]
    L.msf_claim_points_device.argtypes = [vp, C.POINTER(LocalMap), vp, i32, vp, vp, i32, C.POINTER(ClaimResult), vp]
    L.msf_search_local_points.argtypes = [vp, i32, vp, C.POINTER(LocalMap), C.POINTER(FrustumParams), C.c_uint32, vp, vp,
                                          i32, C.POINTER(FrustumResult), C.POINTER(ClaimResult), C.POINTER(DeviceCorr)]
    L.msfx_frame_tracking_version.restype = C.c_int
    L.msfx_carry_points_device.argtypes = [vp, C.POINTER(FrameMap), vp, i32, vp, i32, C.POINTER(TrackResult), vp]
    L.msfx_track_list_device.argtypes = [vp, C.POINTER(FrameMap), vp, i32, vp, i32, C.POINTER(TrackParams),
                                         C.POINTER(TrackResult), C.POINTER(PoseResult), vp]
    L.msfx_track_frame.argtypes = [vp, i32, i32, C.POINTER(FrameMap), C.POINTER(TrackParams), C.c_uint32, vp, vp, i32,
                                   C.POINTER(TrackResult), C.POINTER(PoseResult), C.POINTER(DeviceTrack)]
    L.msf_render_match_image.argtypes = [vp, C.POINTER(Image), C.POINTER(Image), vp, i32, vp, vp, vp, i64]
    L.msf_weights_info.argtypes = [C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(i32), C.POINTER(i64)]
    L.msf_convert_weights.argtypes = [C.c_char_p, C.c_char_p]
    L.msf_frame_cache_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(i32)]
    L.msf_stage_times.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(f32), i32]
    L.msf_multi_create.argtypes = [C.POINTER(Config), i32, C.POINTER(i32), C.POINTER(vp)]
    L.msf_multi_destroy.argtypes = [vp]
    L.msf_multi_destroy.restype = None
    L.msf_multi_device_count.argtypes = [vp]
    L.msf_multi_device_count.restype = i32
    L.msf_multi_handle.argtypes = [vp, i32]
    L.msf_multi_handle.restype = vp
    L.msf_multi_set_threshold.argtypes = [vp, f32]
    L.msf_multi_last_error.argtypes = [vp]
    L.msf_multi_last_error.restype = C.c_char_p
    L.msf_multi_shard_range.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.msf_multi_shard_range.restype = None
    L.msf_multi_match_batch.argtypes = [vp, i32, C.POINTER(Image), C.POINTER(Image), vp, i32, vp]
    L.msf_multi_match_batch_device.argtypes = [vp, C.POINTER(i32), C.POINTER(vp), C.POINTER(vp), i64, i64, C.POINTER(vp), i32,
                                               C.POINTER(vp)]
    L.msf_gather_unique_id.argtypes = [vp]
    L.msf_gather_create.argtypes = [i32, i32, i32, vp, i32, i64, C.POINTER(vp)]
    L.msf_gather_destroy.argtypes = [vp]
    L.msf_gather_destroy.restype = None
    L.msf_gather_last_error.argtypes = [vp]
    L.msf_gather_last_error.restype = C.c_char_p
    L.msf_gather_plan.argtypes = [i32, i32, vp, i64, vp, vp]
    L.msf_gather_matches_device.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    _lib = L
    return L


def default_weights_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "weights", "loftr_teacher.bin")
