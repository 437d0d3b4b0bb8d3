"""ctypes binding of the C-ABI in include/mld.h (libmld_hip.so).

The library is built in-tree by `mono_lidar_depth_amd/csrc/Makefile` (see `__graft_entry__.build`).
There is no fallback: if the shared library is missing, importing the symbols raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "lib" / "libmld_hip.so"

MLD_ABI_VERSION = 8  # include/mld.h
MLD_OK = 0
MLD_ERR_INVALID_ARG = -1
MLD_ERR_NOT_INITIALIZED = -2
MLD_ERR_UNSUPPORTED_MODE = -3
MLD_ERR_NO_ROAD_ESTIMATOR = -4
MLD_ERR_NO_GROUND_PLANE = -5
MLD_ERR_CLOUD_TOO_SMALL = -6
MLD_ERR_HIP = -7
MLD_ERR_CAPACITY = -8
MLD_RESULT_TYPE_COUNT = 21

# eDepthResultType.h:8-30
RESULT_TYPE_NAMES = {
    0: "Unspecified", 1: "Success", 2: "RadiusSearchInsufficientPoints", 3: "HistogramNoLocalMax",
    4: "TresholdDepthGlobalGreaterMax", 5: "TresholdDepthGlobalSmallerMin", 6: "TresholdDepthLocalGreaterMax",
    7: "TresholdDepthLocalSmallerMin", 8: "TriangleNotPlanar", 9: "TriangleNotPlanarInsufficientPoints",
    10: "CornerBehindCamera", 11: "PlaneViewrayNotOrthogonal", 12: "PcaIsPoint", 13: "PcaIsLine",
    14: "PcaIsCubic", 15: "InsufficientRoadPoints", 16: "SuccessRoad",
    17: "RegionGrowingNearestSeedNotAvailable", 18: "RegionGrowingSeedsOutOfRange",
    19: "RegionGrowingInsufficientPoints", 20: "SuccessRegionGrowing",
}


class MldCamera(C.Structure):
    _fields_ = [
        ("focal_length", C.c_double),
        ("principal_point_x", C.c_double),
        ("principal_point_y", C.c_double),
        ("width", C.c_int32),
        ("height", C.c_int32),
    ]


class MldParams(C.Structure):
    _fields_ = [
        ("histogram_segmentation_bin_witdh", C.c_double),
        ("treshold_depth_local_value", C.c_double),
        ("pca_treshold_3_abs_min", C.c_double),
        ("pca_treshold_3_2_rel_max", C.c_double),
        ("pca_treshold_2_1_rel_min", C.c_double),
        ("ransac_plane_point_distance_treshold", C.c_double),
        ("ransac_plane_distance_treshold", C.c_double),
        ("ransac_plane_min_z", C.c_double),
        ("ransac_plane_max_z", C.c_double),
        ("ransac_plane_refinement_treshold", C.c_double),
        ("ransac_plane_probability", C.c_double),
        ("plane_estimator_z_x_min_relation", C.c_double),
        ("triangleplanar_crossnorm_treshold", C.c_double),
        ("viewray_plane_orthoganality_treshold", C.c_double),
        ("ransac_plane_treshold_camx", C.c_double),
        ("neighbor_search_mode", C.c_int32),
        ("pixelarea_search_witdh", C.c_int32),
        ("pixelarea_search_height", C.c_int32),
        ("radiusSearch_count_min", C.c_int32),
        ("do_use_histogram_segmentation", C.c_int32),
        ("histogram_segmentation_min_pointcount", C.c_int32),
        ("do_use_depth_segmentation", C.c_int32),
        ("treshold_depth_enabled", C.c_int32),
        ("treshold_depth_mode", C.c_int32),
        ("treshold_depth_max", C.c_int32),
        ("treshold_depth_min", C.c_int32),
        ("treshold_depth_local_enabled", C.c_int32),
        ("treshold_depth_local_mode", C.c_int32),
        ("treshold_depth_local_valuetype", C.c_int32),
        ("do_use_PCA", C.c_int32),
        ("do_use_ransac_plane", C.c_int32),
        ("plane_estimator_use_triangle_maximation", C.c_int32),
        ("plane_estimator_use_leastsquares", C.c_int32),
        ("plane_estimator_use_mestimator", C.c_int32),
        ("do_use_cut_behind_camera", C.c_int32),
        ("do_use_triangle_size_maximation", C.c_int32),
        ("do_check_triangleplanar_condition", C.c_int32),
        ("set_all_depths_to_zero", C.c_int32),
        ("ransac_plane_max_iterations", C.c_int32),
        ("ransac_plane_use_refinement", C.c_int32),
        ("ransac_plane_use_camx_treshold", C.c_int32),
    ]

    def copy(self) -> "MldParams":
        out = MldParams()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(MldParams))
        return out

    def replace(self, **kw) -> "MldParams":
        out = self.copy()
        for k, v in kw.items():
            if not hasattr(out, k):
                raise AttributeError(k)
            setattr(out, k, v)
        return out


MLD_PLANE_RANSAC, MLD_PLANE_SEMANTIC = 0, 1


class MldPlaneRequest(C.Structure):
    """mld_plane_request (include/mld.h): how the not-yet-segmented plane of a one-frame call is estimated."""
    _fields_ = [
        ("kind", C.c_int32),
        ("seed", C.c_uint32),
        ("label_image", C.c_void_p),
        ("rows", C.c_int32),
        ("cols", C.c_int32),
        ("row_stride_bytes", C.c_int32),
        ("n_labels", C.c_int32),
        ("ground_labels", C.c_void_p),
        ("inlier_threshold", C.c_double),
    ]


class MldPlaneResult(C.Structure):
    _fields_ = [("coeffs", C.c_float * 4), ("n_inliers", C.c_int64), ("status", C.c_int32), ("iterations", C.c_int32)]


class MldSemanticPlaneResult(C.Structure):
    """mld_semantic_plane_result (include/mld.h): one sequence of mld_semantic_planes_estimate_device, 32 bytes."""
    _fields_ = [("coeffs", C.c_float * 4), ("n_candidates", C.c_int32), ("n_inliers", C.c_int32), ("status", C.c_int32),
                ("reserved", C.c_int32)]


class MldRansacPlaneResult(C.Structure):
    """mld_ransac_plane_result (include/mld.h): one sequence of mld_ransac_planes_estimate_device, 32 bytes."""
    _fields_ = [("coeffs", C.c_float * 4), ("n_inliers", C.c_int32), ("iterations", C.c_int32), ("status", C.c_int32),
                ("n_candidates", C.c_int32)]


class MldDepthReport(C.Structure):
    """mld_depth_report (include/mld.h): one sequence of mld_depth_reports_collect_*_device, 192 bytes = 24 int64."""
    _fields_ = [("counts", C.c_int64 * MLD_RESULT_TYPE_COUNT), ("other", C.c_int64), ("point_count", C.c_int64), ("n_interpolated", C.c_int64)]


class MldLeavingRecord(C.Structure):
    """mld_leaving_record (include/mld.h): one sequence of mld_tracks_export_leaving_device, 32 bytes = 4 int64."""
    _fields_ = [("n_ended", C.c_int64), ("n_ended_entries", C.c_int64), ("n_spilled", C.c_int64), ("reserved", C.c_int64)]


class MldPlaneInlierCounts(C.Structure):
    """mld_plane_inlier_counts (include/mld.h): one sequence of mld_plane_inliers_export_device, 16 bytes = 2 int64."""
    _fields_ = [("n_inliers", C.c_int64), ("n_cloud", C.c_int64)]


# mld_feature_trace::road_state and ::flags (include/mld.h)
MLD_TRACE_ROAD_NOT_REACHED, MLD_TRACE_ROAD_FEW_NEIGHBOURS, MLD_TRACE_ROAD_FAR_NEIGHBOUR = 0, 1, 2
MLD_TRACE_ROAD_FEW_INLIERS, MLD_TRACE_ROAD_FIT = 3, 4
MLD_TRACE_FLAG_BAD_INPUT, MLD_TRACE_FLAG_NONFINITE_FEATURE = 1, 2


class MldFeatureTrace(C.Structure):
    """mld_feature_trace (include/mld.h): one feature of mld_feature_traces_collect_*_device, 184 bytes."""
    _fields_ = [("main_type", C.c_int32), ("road_state", C.c_int32), ("n_nb", C.c_int32), ("n_seg", C.c_int32),
                ("n_road", C.c_int32), ("n_road_inl", C.c_int32), ("corner_pos", C.c_int32 * 3), ("corner_vis", C.c_int32 * 3),
                ("flags", C.c_int32), ("pad_", C.c_int32), ("main_depth", C.c_double), ("hist_lower", C.c_double),
                ("hist_higher", C.c_double), ("plane_n", C.c_double * 3), ("plane_offset", C.c_double),
                ("corners", C.c_double * 9)]


# mld_coverage_maps: the bits of reach_out and mld_coverage_record::flags (include/mld.h)
MLD_COVERAGE_REACH_MAIN, MLD_COVERAGE_REACH_ROAD = 1, 2
MLD_COVERAGE_FLAG_BAD_INPUT, MLD_COVERAGE_FLAG_HAS_PLANE = 1, 2


class MldCoverageRecord(C.Structure):
    """mld_coverage_record (include/mld.h): one sequence of mld_coverage_maps_collect_device, 64 bytes = 8 int64."""
    _fields_ = [("n_reach", C.c_int64), ("n_reach_road", C.c_int64), ("n_occupied", C.c_int64), ("n_inlier", C.c_int64),
                ("n_far", C.c_int64), ("max_nb", C.c_int32), ("flags", C.c_int32), ("n_buckets", C.c_int32),
                ("pad_", C.c_int32 * 3)]


# mld_depth_images: the bits of mld_depth_image_record::flags (include/mld.h)
MLD_DEPTH_IMAGE_FLAG_BAD_INPUT, MLD_DEPTH_IMAGE_FLAG_HAS_PLANE = 1, 2


class MldDepthImageRecord(C.Structure):
    """mld_depth_image_record (include/mld.h): one sequence of mld_depth_images_render_device, 200 bytes = 25 int64."""
    _fields_ = [("counts", C.c_int64 * 21), ("n_pixels", C.c_int64), ("n_depth", C.c_int64), ("n_cooperative", C.c_int64),
                ("flags", C.c_int32), ("pad_", C.c_int32)]


# mld_region_depths: the bits of mld_region_depth::flags and the two capacities of the kernel (include/mld.h)
(MLD_REGION_FLAG_BAD_INPUT, MLD_REGION_FLAG_EMPTY_BOX, MLD_REGION_FLAG_HIST_FOUND, MLD_REGION_FLAG_HIST_CAPPED,
 MLD_REGION_FLAG_HAS_MASK) = 1, 2, 4, 8, 16
MLD_REGION_LIST_CAPACITY, MLD_REGION_HIST_BINS = 2048, 512


class MldRegionDepth(C.Structure):
    """mld_region_depth (include/mld.h): one box of mld_region_depths_collect_device, 80 bytes = 10 int64."""
    _fields_ = [("n_points", C.c_int32), ("n_ground", C.c_int32), ("n_seg", C.c_int32), ("flags", C.c_int32),
                ("nearest_orig", C.c_int32), ("clip", C.c_int32 * 4), ("pad_", C.c_int32), ("z_min", C.c_double),
                ("z_max", C.c_double), ("z_median", C.c_double), ("hist_lower", C.c_double), ("hist_higher", C.c_double)]


# mld_nearest_depths: the bits of mld_nearest_depth::flags and the limits of radius and count (include/mld.h)
MLD_NEAREST_FLAG_BAD_INPUT, MLD_NEAREST_FLAG_NONFINITE_FEATURE = 1, 2
MLD_NEAREST_MAX_RADIUS, MLD_NEAREST_MAX_COUNT = 64, 256


class MldNearestDepth(C.Structure):
    """mld_nearest_depth (include/mld.h): one feature of mld_nearest_depths_collect_*_device, 64 bytes = 8 int64."""
    _fields_ = [("type", C.c_int32), ("n_in_radius", C.c_int32), ("n_nb", C.c_int32), ("n_seg", C.c_int32),
                ("d2_first", C.c_int32), ("d2_last", C.c_int32), ("nearest_orig", C.c_int32), ("flags", C.c_int32),
                ("depth", C.c_double), ("nearest_z", C.c_double), ("corner_vis", C.c_int32 * 3), ("pad_", C.c_int32)]


# mld_row_growth: the bits of mld_row_growth::flags (the third also of mld_row_growth_cloud::flags) and the limits of the
# count, the kept list and the row capacity (include/mld.h)
(MLD_ROW_GROWTH_FLAG_BAD_INPUT, MLD_ROW_GROWTH_FLAG_NONFINITE_FEATURE, MLD_ROW_GROWTH_FLAG_ROWS_TRUNCATED,
 MLD_ROW_GROWTH_FLAG_LIST_CAPPED) = 1, 2, 4, 8
MLD_ROW_GROWTH_MAX_COUNT, MLD_ROW_GROWTH_MAX_LIST, MLD_ROW_GROWTH_MAX_ROWS = 256, 1024, 65536


class MldRowGrowthParams(C.Structure):
    """mld_row_growth_params (include/mld.h): the depth_segmentation_* values of DepthEstimatorParameters.h:52-60, 64 bytes."""
    _fields_ = [("depth_segmentation_max_treshold_gradient", C.c_double),
                ("depth_segmentation_max_neighbor_distance", C.c_double),
                ("depth_segmentation_max_neighbor_distance_gradient", C.c_double),
                ("depth_segmentation_max_neighbor_to_seedpoint_distance", C.c_double),
                ("depth_segmentation_max_seedpoint_to_seedpoint_distance_gradient", C.c_double),
                ("depth_segmentation_max_seedpoint_to_seedpoint_distance", C.c_double),
                ("depth_segmentation_max_neighbor_to_seedpoint_distance_gradient", C.c_double),
                ("depth_segmentation_max_pointcount", C.c_int32), ("pad_", C.c_int32)]

    def replace(self, **kw) -> "MldRowGrowthParams":
        out = MldRowGrowthParams.from_buffer_copy(self)
        for k, v in kw.items():
            if not hasattr(out, k):
                raise AttributeError(k)
            setattr(out, k, v)
        return out


class MldRowGrowthCloud(C.Structure):
    """mld_row_growth_cloud (include/mld.h): one sequence of mld_row_growth_segment_device, 16 bytes."""
    _fields_ = [("n_rows", C.c_int32), ("n_vis", C.c_int32), ("longest_row", C.c_int32), ("flags", C.c_int32)]


class MldRowGrowth(C.Structure):
    """mld_row_growth (include/mld.h): one feature of mld_row_growth_collect_*_device, 72 bytes = 9 int64."""
    _fields_ = [("type", C.c_int32), ("state", C.c_int32), ("grown_type", C.c_int32), ("flags", C.c_int32),
                ("n_nb", C.c_int32), ("seed_vis", C.c_int32), ("second_vis", C.c_int32), ("seed_row", C.c_int32),
                ("second_row", C.c_int32), ("n_first", C.c_int32), ("n_grown", C.c_int32), ("corner_vis", C.c_int32 * 3),
                ("depth", C.c_double), ("seed_z", C.c_double)]


# mld_sweep_merge: the bit of mld_sweep_merge_record::flags and the limit of max_sweeps (include/mld.h)
MLD_SWEEP_FLAG_TRUNCATED = 1
MLD_SWEEP_MAX_SWEEPS = 16


class MldSweepMergeRecord(C.Structure):
    """mld_sweep_merge_record (include/mld.h): one sequence of mld_sweep_merge_run_device, 112 bytes = 14 int64."""
    _fields_ = [("n_in", C.c_int64), ("n_kept", C.c_int64), ("n_written", C.c_int64), ("n_nonfinite", C.c_int64),
                ("n_out_of_range", C.c_int64), ("kept", C.c_int32 * MLD_SWEEP_MAX_SWEEPS), ("flags", C.c_int32),
                ("pad_", C.c_int32)]


# Every symbol include/mld.h declares: (name, restype, argtypes)
_P = C.POINTER
_SIGNATURES = [
    ("mld_params_default", None, [_P(MldParams)]),
    ("mld_params_c0", None, [_P(MldParams)]),
    ("mld_params_from_file", C.c_int, [_P(MldParams), C.c_char_p, C.c_char_p, C.c_int]),
    ("mld_abi_version", C.c_int, []),
    ("mld_create", C.c_void_p, [_P(MldParams), _P(MldCamera), _P(C.c_double), C.c_int, C.c_int, C.c_int64,
                                C.c_int64, _P(C.c_int)]),
    ("mld_create_error", C.c_char_p, []),
    ("mld_destroy", None, [C.c_void_p]),
    ("mld_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_get_stream", C.c_void_p, [C.c_void_p]),
    ("mld_synchronize", C.c_int, [C.c_void_p]),
    ("mld_order_after", C.c_int, [C.c_void_p, C.c_void_p]),
    ("mld_order_after_classify", C.c_int, [C.c_void_p, C.c_void_p]),
    ("mld_pair_contexts", C.c_int, [C.c_void_p, C.c_void_p]),
    ("mld_set_shared_gpu", C.c_int, [C.c_void_p, C.c_int]),
    ("mld_set_list_capacity", C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    ("mld_set_list_budget", C.c_int, [C.c_void_p, C.c_int]),
    ("mld_contexts_concurrent", C.c_int, [C.c_void_p, C.c_void_p]),
    ("mld_get_path_counts", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("mld_set_cloud", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int]),
    ("mld_set_cloud_device", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int]),
    ("mld_set_clouds_device", C.c_int, [C.c_void_p, C.c_int, _P(C.c_void_p), _P(C.c_int64), C.c_int]),
    ("mld_set_clouds_planes_device", C.c_int, [C.c_void_p, C.c_int, _P(C.c_void_p), _P(C.c_int64), C.c_int,
                                               _P(C.c_float), _P(C.c_void_p)]),
    ("mld_set_clouds_estimate_planes_device", C.c_int, [C.c_void_p, C.c_int, _P(C.c_void_p), _P(C.c_int64), C.c_int,
                                                        _P(C.c_uint32)]),
    ("mld_get_estimated_planes", C.c_int, [C.c_void_p, C.c_int, _P(C.c_float), _P(C.c_int64), _P(C.c_int32)]),
    ("mld_set_ground_plane", C.c_int, [C.c_void_p, C.c_int, _P(C.c_float), C.c_void_p, C.c_int64]),
    ("mld_set_ground_plane_device", C.c_int, [C.c_void_p, C.c_int, _P(C.c_float), C.c_void_p, C.c_int64]),
    ("mld_estimate_ground_plane", C.c_int, [C.c_void_p, C.c_int, C.c_uint32, _P(C.c_float), _P(C.c_int64)]),
    ("mld_estimate_semantic_plane", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_int, C.c_double, _P(C.c_float), _P(C.c_int64)]),
    ("mld_estimate_semantic_plane_device", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                     C.c_void_p, C.c_int, C.c_double, _P(C.c_float), _P(C.c_int64)]),
    ("mld_get_ground_plane_inliers", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("mld_set_ground_plane_mask_device", C.c_int, [C.c_void_p, C.c_int, _P(C.c_float), C.c_void_p]),
    ("mld_set_ground_planes_mask_device", C.c_int, [C.c_void_p, C.c_int, _P(C.c_float), _P(C.c_void_p)]),
    ("mld_calculate_depth", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("mld_calculate_depth_opts", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint32]),
    ("mld_calculate_depth_frame", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, _P(C.c_float), C.c_void_p,
                                            C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("mld_calculate_depth_frame_estimate", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int,
                                                     _P(MldPlaneRequest), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                     _P(MldPlaneResult)]),
    ("mld_frame_timing", C.c_int, [C.c_void_p, _P(C.c_double)]),
    ("mld_pack_points_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int]),
    ("mld_calculate_depth_device", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("mld_calculate_depths_device", C.c_int, [C.c_void_p, C.c_int, _P(C.c_void_p), _P(C.c_int64),
                                              _P(C.c_void_p), _P(C.c_void_p)]),
    ("mld_tracklets_depth_device", C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int64] +
     [C.c_void_p] * 4 + [_P(C.c_int64)]),
    ("mld_tracklets_depth", C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int64] +
     [C.c_void_p] * 4 + [_P(C.c_int64)]),
    ("mld_tracklets_frame", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, _P(MldPlaneRequest),
                                      _P(C.c_float), C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64] +
     [C.c_void_p] * 4 + [_P(C.c_int64), _P(MldPlaneResult)]),
    ("mld_set_clouds_planes_range_device", C.c_int, [C.c_void_p, C.c_int, C.c_int, _P(C.c_void_p), _P(C.c_int64), C.c_int,
                                                     _P(C.c_float), _P(C.c_void_p)]),
    ("mld_tracklets_depths_device", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [_P(C.c_void_p)] * 5 +
     [_P(C.c_int64)] + [_P(C.c_void_p)] * 4),
    ("mld_tracklets_depths_lanes_device", C.c_int, [C.c_void_p, C.c_int, C.c_int, _P(C.c_uint8)] + [_P(C.c_void_p)] * 5 +
     [_P(C.c_int64)] + [_P(C.c_void_p)] * 4),
    ("mld_tracks_create", C.c_void_p, [C.c_void_p, C.c_int, C.c_int64, C.c_int, _P(C.c_int)]),
    ("mld_tracks_destroy", None, [C.c_void_p]),
    ("mld_tracks_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_tracks_begin_device", C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64), _P(C.c_void_p)]),
    ("mld_tracks_commit_device", C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 6),
    ("mld_tracks_export_device", C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p)]),
    ("mld_tracks_export_packed_device", C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64), _P(C.c_void_p)]),
    ("mld_tracks_import_packed_device", C.c_int, [C.c_void_p, _P(C.c_uint8), _P(C.c_void_p), _P(C.c_int64), _P(C.c_void_p),
                                                  _P(C.c_void_p), _P(C.c_int64)]),
    ("mld_tracks_reset_device", C.c_int, [C.c_void_p, _P(C.c_uint8)]),
    ("mld_tracks_export_leaving_device", C.c_int, [C.c_void_p, _P(C.c_uint8)] + [_P(C.c_void_p)] * 5 + [_P(C.c_int64)] * 3 +
     [C.c_void_p]),
    ("mld_tracks_set_leaving_sink", C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 5 + [_P(C.c_int64)] * 3 + [C.c_void_p]),
    ("mld_tracks_counts", C.c_int, [C.c_void_p, _P(C.c_int64)]),
    ("mld_tracklets_step_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [_P(C.c_void_p)] * 5 +
     [_P(C.c_int64)] + [_P(C.c_void_p)] * 4),
    ("mld_tracklets_step_lanes_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_uint8), _P(C.c_uint8)] +
     [_P(C.c_void_p)] * 5 + [_P(C.c_int64)] + [_P(C.c_void_p)] * 4),
    ("mld_labels_create", C.c_void_p, [C.c_void_p, C.c_int, _P(C.c_int)]),
    ("mld_labels_destroy", None, [C.c_void_p]),
    ("mld_labels_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_labels_assign_device", C.c_int, [C.c_void_p, _P(C.c_void_p)] + [C.c_int] * 5 + [_P(C.c_void_p)] * 2 +
     [_P(C.c_int64)] + [_P(C.c_void_p)] * 2),
    ("mld_semantic_planes_create", C.c_void_p, [C.c_void_p, C.c_int, C.c_int64, _P(MldCamera), _P(C.c_double), _P(C.c_int)]),
    ("mld_semantic_planes_destroy", None, [C.c_void_p]),
    ("mld_semantic_planes_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_semantic_planes_estimate_device", C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64), C.c_int, _P(C.c_void_p)] +
     [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_double, C.c_void_p, _P(C.c_void_p)]),
    ("mld_ransac_planes_create", C.c_void_p, [C.c_void_p, C.c_int, C.c_int64, _P(MldParams), _P(C.c_int)]),
    ("mld_ransac_planes_destroy", None, [C.c_void_p]),
    ("mld_ransac_planes_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_ransac_planes_estimate_device", C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64), C.c_int, _P(C.c_uint32),
                                                    C.c_void_p, _P(C.c_void_p)]),
    ("mld_projected_clouds_create", C.c_void_p, [C.c_void_p, C.c_int, C.c_int64, _P(MldCamera), _P(C.c_double), _P(C.c_int)]),
    ("mld_projected_clouds_destroy", None, [C.c_void_p]),
    ("mld_projected_clouds_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_projected_clouds_export_device", C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64), C.c_int, _P(C.c_int64),
                                                     C.c_void_p] + [_P(C.c_void_p)] * 5),
    ("mld_depth_reports_create", C.c_void_p, [C.c_void_p, C.c_int, C.c_int64, _P(MldCamera), _P(C.c_int)]),
    ("mld_depth_reports_destroy", None, [C.c_void_p]),
    ("mld_depth_reports_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_depth_reports_collect_device", C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 3 + [_P(C.c_int64)] * 2 +
     [C.c_void_p] + [_P(C.c_void_p)] * 2),
    ("mld_depth_reports_collect_tracks_device", C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 4 + [_P(C.c_int64)] * 2 +
     [C.c_void_p] + [_P(C.c_void_p)] * 2),
    ("mld_plane_inliers_create", C.c_void_p, [C.c_void_p, C.c_int, C.c_int64, _P(MldParams), _P(C.c_double), _P(C.c_int)]),
    ("mld_plane_inliers_destroy", None, [C.c_void_p]),
    ("mld_plane_inliers_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_plane_inliers_export_device", C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64), C.c_int, _P(C.c_void_p),
                                                  _P(C.c_int64), C.c_void_p] + [_P(C.c_void_p)] * 3),
    ("mld_feature_traces_create", C.c_void_p, [C.c_void_p, C.c_int, C.c_int64, _P(MldParams), _P(MldCamera), _P(C.c_double),
                                               _P(C.c_int)]),
    ("mld_feature_traces_destroy", None, [C.c_void_p]),
    ("mld_feature_traces_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_feature_traces_collect_device", C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)] + [_P(C.c_void_p)] * 2 +
     [_P(C.c_int64), _P(C.c_void_p), _P(C.c_int64), _P(C.c_float), _P(C.c_void_p), C.c_int] + [_P(C.c_void_p)] * 5),
    ("mld_feature_traces_collect_tracks_device", C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 2 + [_P(C.c_int64)] +
     [_P(C.c_void_p)] * 2 + [_P(C.c_int64), _P(C.c_void_p), _P(C.c_int64), _P(C.c_float), _P(C.c_void_p), C.c_int] +
     [_P(C.c_void_p)] * 5),
    ("mld_coverage_maps_create", C.c_void_p, [C.c_void_p, C.c_int, _P(MldParams), _P(MldCamera), _P(C.c_double), _P(C.c_int)]),
    ("mld_coverage_maps_destroy", None, [C.c_void_p]),
    ("mld_coverage_maps_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_coverage_maps_collect_device", C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 2 + [_P(C.c_int64), _P(C.c_void_p),
                                                   _P(C.c_int64), _P(C.c_float)] + [_P(C.c_void_p)] * 6 +
     [C.c_void_p, C.c_int, C.c_int, _P(C.c_int64), _P(C.c_void_p)]),
    ("mld_depth_images_create", C.c_void_p, [C.c_void_p, C.c_int, _P(MldParams), _P(MldCamera), _P(C.c_double), _P(C.c_int)]),
    ("mld_depth_images_destroy", None, [C.c_void_p]),
    ("mld_depth_images_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_depth_images_render_device", C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 2 + [_P(C.c_int64), _P(C.c_void_p),
                                                 _P(C.c_int64), _P(C.c_float), _P(C.c_void_p)] + [C.c_int] * 6 +
     [_P(C.c_void_p)] * 3 + [C.c_void_p]),
    ("mld_region_depths_create", C.c_void_p, [C.c_void_p, C.c_int, C.c_int64, _P(MldParams), _P(MldCamera), _P(C.c_int)]),
    ("mld_region_depths_destroy", None, [C.c_void_p]),
    ("mld_region_depths_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_region_depths_collect_device", C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 2 + [_P(C.c_int64), _P(C.c_void_p),
                                                   _P(C.c_int64)] + [_P(C.c_void_p)] * 2 + [_P(C.c_int64), _P(C.c_void_p)]),
    ("mld_nearest_depths_create", C.c_void_p, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, _P(MldParams), _P(MldCamera),
                                               _P(C.c_int)]),
    ("mld_nearest_depths_destroy", None, [C.c_void_p]),
    ("mld_nearest_depths_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_nearest_depths_collect_device", C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)] + [_P(C.c_void_p)] * 2 +
     [_P(C.c_int64), _P(C.c_void_p), _P(C.c_int64), C.c_int] + [_P(C.c_void_p)] * 2),
    ("mld_nearest_depths_collect_tracks_device", C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 2 + [_P(C.c_int64)] +
     [_P(C.c_void_p)] * 2 + [_P(C.c_int64), _P(C.c_void_p), _P(C.c_int64), C.c_int] + [_P(C.c_void_p)] * 2),
    ("mld_row_growth_params_default", None, [_P(MldRowGrowthParams)]),
    ("mld_row_growth_params_yaml", None, [_P(MldRowGrowthParams)]),
    ("mld_row_growth_create", C.c_void_p, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, _P(MldParams),
                                           _P(MldRowGrowthParams), _P(MldCamera), _P(C.c_double), _P(C.c_int)]),
    ("mld_row_growth_destroy", None, [C.c_void_p]),
    ("mld_row_growth_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_row_growth_segment_device", C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64), C.c_void_p, _P(C.c_void_p),
                                                C.c_void_p]),
    ("mld_row_growth_collect_device", C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_int64)] + [_P(C.c_void_p)] * 2 +
     [_P(C.c_int64), _P(C.c_void_p), _P(C.c_int64)] + [_P(C.c_void_p)] * 2 + [C.c_void_p, C.c_int] + [_P(C.c_void_p)] * 4),
    ("mld_row_growth_collect_tracks_device", C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 2 + [_P(C.c_int64)] +
     [_P(C.c_void_p)] * 2 + [_P(C.c_int64), _P(C.c_void_p), _P(C.c_int64)] + [_P(C.c_void_p)] * 2 + [C.c_void_p, C.c_int] +
     [_P(C.c_void_p)] * 4),
    ("mld_sweep_merge_create", C.c_void_p, [C.c_void_p, C.c_int, C.c_int, C.c_int64, _P(C.c_int)]),
    ("mld_sweep_merge_destroy", None, [C.c_void_p]),
    ("mld_sweep_merge_last_error", C.c_char_p, [C.c_void_p]),
    ("mld_sweep_merge_run_device", C.c_int, [C.c_void_p, C.c_int, _P(C.c_void_p), _P(C.c_int64), C.c_int, _P(C.c_void_p),
                                             C.c_float, C.c_float, _P(C.c_int64)] + [_P(C.c_void_p)] * 3 + [C.c_void_p]),
    ("mld_get_visible_count", C.c_int, [C.c_void_p, C.c_int, _P(C.c_int64)]),
    ("mld_get_visible_image_points", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    ("mld_get_point_index", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    ("mld_get_cloud_camera_cs", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    ("mld_get_pixel_map", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    ("mld_get_point_depth_cam_visible", C.c_int, [C.c_void_p, C.c_int, C.c_int64, _P(C.c_double)]),
    ("mld_calculate_depth_debug", C.c_int,
     [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("mld_get_ground_plane_cloud", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("mld_result_histogram", C.c_int, [C.c_void_p, C.c_int64, _P(C.c_int64)]),
    ("mld_timing_enable", C.c_int, [C.c_void_p, C.c_int]),
    ("mld_timing_reset", C.c_int, [C.c_void_p]),
    ("mld_kernel_time_ms", C.c_int, [C.c_void_p, C.c_int, _P(C.c_double), _P(C.c_int64)]),
]
EXPORTED_SYMBOLS = [s[0] for s in _SIGNATURES]

_lib = None
_lib_ab = None
LIB_AB_PATH = _HERE / "lib" / "libmld_hip_ab.so"


def _bind(path: Path) -> C.CDLL:
    # PyTorch ships its own libamdhip64 (same SONAME as /opt/rocm's).  Two HIP runtimes in one process cannot
    # both own the GPU, so when torch is installed it is imported FIRST: the dynamic loader then resolves this
    # library's libamdhip64.so.7 dependency to the runtime torch already loaded.  (A C++ caller without torch
    # simply gets /opt/rocm's runtime.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not path.exists():
        raise RuntimeError(
            f"{path} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C mono_lidar_depth_amd/csrc`). There is no CPU fallback for this path.")
    lib = C.CDLL(str(path))
    for name, restype, argtypes in _SIGNATURES:
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


def load() -> C.CDLL:
    """Load libmld_hip.so.  Raises (never falls back) when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        _lib = _bind(Path(os.environ.get("MLD_HIP_LIBRARY", LIB_PATH)))
    return _lib


def load_ab() -> C.CDLL:
    """The test / measurement build of the same sources (-DMLD_AB_SWITCHES, see csrc/Makefile): its mld_create reads
    MLD_FORCE_WAVE_PATH etc. from the environment.  Used by the GPU parity suite and the A/B tools, never by the
    product path."""
    global _lib_ab
    if _lib_ab is None:
        _lib_ab = _bind(Path(os.environ.get("MLD_HIP_AB_LIBRARY") or LIB_AB_PATH))  # (the override: A/B tools only)
    return _lib_ab


def params_c0() -> MldParams:
    p = MldParams()
    load().mld_params_c0(C.byref(p))
    return p


def params_default() -> MldParams:
    p = MldParams()
    load().mld_params_default(C.byref(p))
    return p


def row_growth_params_default() -> MldRowGrowthParams:
    """The depth_segmentation_* defaults of DepthEstimatorParameters.h:52-60."""
    g = MldRowGrowthParams()
    load().mld_row_growth_params_default(C.byref(g))
    return g


def row_growth_params_yaml() -> MldRowGrowthParams:
    """The depth_segmentation_* values of the shipped parameters.yaml:77-91."""
    g = MldRowGrowthParams()
    load().mld_row_growth_params_yaml(C.byref(g))
    return g


def params_from_file(path: str) -> MldParams:
    p = MldParams()
    err = C.create_string_buffer(2048)
    rc = load().mld_params_from_file(C.byref(p), str(path).encode(), err, 2048)
    if rc != MLD_OK:
        raise RuntimeError(err.value.decode())
    # mirrored keys the file lacks (they read as 0, as cv::FileStorage reads them in the reference)
    note = err.value.decode()
    p.absent_keys = [k.strip() for k in note.split(":", 1)[1].split(",")] if note.startswith("absent") else []
    return p
