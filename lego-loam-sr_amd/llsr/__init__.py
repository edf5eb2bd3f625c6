"""Python host binding of the MI355X LeGO-LOAM-SR hot path (ctypes over include/llsr.h).

Mirrors the reference's node-level interface for this path:

* `ImageProjection.cloud_handler(points)` ~ ImageProjection::cloudHandler (imageProjection.cpp:189)
  -> a ProjectionOut-like dict (segmented / outlier clouds + CloudInfo fields).
* `FeatureAssociation.extract(...)` ~ the feature stage of runFeatureAssociation
  (featureAssociation.cpp:2766-2775).
* `MapOptimization.scan2map_optimization(...)` ~ MapOptimization::scan2MapOptimization
  (mapOptmization.cpp:1572-1610): kNN-5 correspondences + the 6x6 LM against a local map.
* `Pipeline.process_scan` runs both for one scan; `Pipeline.process_batch` runs B scans that are
  already resident in HBM (device pointers, e.g. from torch tensors).

There is no CPU fallback: if libllsr.so (the HIP build) is missing or no HIP device is present,
construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import Config, config_for  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("LLSR_LIB") or os.path.join(_PKG, "libllsr.so")  # override: A/B builds
_LIB = None

EXPORTS = [
    "llsr_abi_version", "llsr_build_id", "llsr_config_default", "llsr_get_config", "llsr_create", "llsr_destroy", "llsr_last_error", "llsr_query_sizes",
    "llsr_reset_state", "llsr_process_scan", "llsr_process_batch", "llsr_fetch_scan", "llsr_fetch_vis_clouds",
    "llsr_batch_counts", "llsr_kernel_times_ms", "llsr_kernel_name", "llsr_set_profiling",
    "llsr_scan2map_reserve", "llsr_scan2map_batch", "llsr_scan2map", "llsr_scan2map_stats",
    "llsr_shadow_points", "llsr_scan2scan_reserve", "llsr_scan2scan_batch", "llsr_scan2scan_check",
    "llsr_scan2scan", "llsr_scan2map_shard_begin", "llsr_scan2map_shard_partial",
    "llsr_scan2map_shard_step", "llsr_scan2map_shard_end", "llsr_odometry_batch", "llsr_odometry_fetch",
    "llsr_odometry_reset", "llsr_map_config_default", "llsr_map_config_lidar", "llsr_map_create", "llsr_map_destroy",
    "llsr_map_last_error", "llsr_map_reset", "llsr_map_voxel_grid", "llsr_map_downsample_scan",
    "llsr_map_add_keyframe", "llsr_map_num_keyframes", "llsr_map_extract", "llsr_map_keyframe_ids",
    "llsr_decode_pointcloud2", "llsr_kitti_count", "llsr_kitti_read", "llsr_kitti_load",
    "llsr_mapping_init", "llsr_mapping_batch", "llsr_mapping_fetch", "llsr_mapping_keyposes", "llsr_mapping_reset",
    "llsr_mapping_associate", "llsr_set_voxel_order", "llsr_scan2scan_stats", "llsr_fusion_init",
    "llsr_pose_to_odometry", "llsr_odometry_to_transform", "llsr_fusion_laser_odometry", "llsr_fusion_aft_mapped",
    "llsr_integrate_transformation", "llsr_transform_to_end", "llsr_odom_init", "llsr_odom_callback",
    "llsr_update_initial_guess", "llsr_odometry_batch_odom", "llsr_odometry_fetch_lm", "llsr_mapping_batch_odom",
    "llsr_global_map_config_default", "llsr_map_global", "llsr_map_save", "llsr_keypose_radius_sorted",
    "llsr_mapping_global_map", "llsr_mapping_save_map", "llsr_row_bins",
    "llsr_loop_config_lidar", "llsr_map_set_keyframe_time", "llsr_map_keyframe_times",
    "llsr_map_set_key_poses", "llsr_loop_candidate", "llsr_umeyama3", "llsr_loop_constraint",
    "llsr_icp_align_host", "llsr_icp_create", "llsr_icp_destroy", "llsr_icp_last_error", "llsr_icp_align",
    "llsr_icp_last_times", "llsr_map_loop_submaps", "llsr_map_loop_closure",
    "llsr_icp_align_batch", "llsr_icp_last_passes", "llsr_mapping_stage_times", "llsr_mapping_keyframe_times",
    "llsr_mapping_loop_closure", "llsr_mapping_set_key_poses",
    "llsr_pg_create", "llsr_pg_destroy", "llsr_pg_last_error", "llsr_pg_config_default", "llsr_pg_reset",
    "llsr_pg_append", "llsr_pg_add_loop", "llsr_pg_optimize", "llsr_pg_poses",
    "llsr_mapping_enable_pose_graph", "llsr_mapping_close_loops", "llsr_mapping_pose_graph_poses",
    "llsr_imu_init", "llsr_imu_callback", "llsr_imu_scan_window", "llsr_imu_deskew_host", "llsr_stage_imu",
    "llsr_fetch_imu_report", "llsr_set_imu_undistortion", "llsr_integrate_transformation_imu",
    "llsr_transform_to_end_imu", "llsr_first_scan_imu",
    "llsr_prior_config_default", "llsr_prior_create", "llsr_prior_destroy", "llsr_prior_last_error",
    "llsr_prior_load", "llsr_prior_info", "llsr_prior_points", "llsr_prior_tile_starts", "llsr_prior_crop_batch",
    "llsr_prior_last_crop", "llsr_mapping_set_prior", "llsr_mapping_set_pose",
]


class LlsrError(RuntimeError):
    pass


def build_id() -> str:
    """The loaded library's llsr_build_id() (hash of the kernel sources it was built from)."""
    return lib().llsr_build_id().decode()


def lib():
    """Load libllsr.so (raises if it has not been built)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise LlsrError(f"{LIB_PATH} missing: build it with `make -C lego-loam-sr_amd` "
                            "(there is no CPU fallback for the HIP path)")
        L = C.CDLL(LIB_PATH)
        L.llsr_abi_version.restype = C.c_int32
        L.llsr_abi_version.argtypes = []
        if L.llsr_abi_version() != _abi.ABI_VERSION:
            raise LlsrError(f"{LIB_PATH} has ABI version {L.llsr_abi_version()}, the bindings expect "
                            f"{_abi.ABI_VERSION}: rebuild with `make -C lego-loam-sr_amd`")
        L.llsr_build_id.restype = C.c_char_p
        L.llsr_build_id.argtypes = []
        L.llsr_config_default.argtypes = [C.POINTER(Config), C.c_int32]
        L.llsr_create.argtypes = [C.POINTER(Config), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.llsr_destroy.argtypes = [C.c_void_p]
        L.llsr_last_error.restype = C.c_char_p
        L.llsr_last_error.argtypes = [C.c_void_p]
        L.llsr_query_sizes.argtypes = [C.c_void_p, C.POINTER(_abi.Sizes)]
        L.llsr_reset_state.argtypes = [C.c_void_p]
        L.llsr_process_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(_abi.ScanOut)]
        L.llsr_process_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.llsr_fetch_scan.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_abi.ScanOut)]
        L.llsr_fetch_vis_clouds.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_abi.VisOut)]
        L.llsr_batch_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.llsr_kernel_times_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.llsr_kernel_name.restype = C.c_char_p
        L.llsr_kernel_name.argtypes = [C.c_int32]
        L.llsr_row_bins.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_int32]
        L.llsr_set_profiling.argtypes = [C.c_void_p, C.c_int32]
        L.llsr_scan2map_reserve.argtypes = [C.c_void_p] + [C.c_int32] * 5
        L.llsr_scan2map_batch.argtypes = [C.c_void_p, C.POINTER(_abi.S2MBatch), C.c_void_p]
        L.llsr_scan2map_stats.argtypes = [C.c_void_p, C.POINTER(_abi.S2MStats)]
        L.llsr_scan2scan_stats.argtypes = [C.c_void_p, C.POINTER(_abi.S2SStats)]
        L.llsr_fusion_init.argtypes = [C.POINTER(_abi.FusionState)]
        L.llsr_pose_to_odometry.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.OdometryMsg)]
        L.llsr_odometry_to_transform.argtypes = [C.POINTER(_abi.OdometryMsg), C.c_void_p]
        L.llsr_fusion_laser_odometry.argtypes = [C.POINTER(_abi.FusionState), C.POINTER(_abi.OdometryMsg),
                                                 C.POINTER(_abi.OdometryMsg)]
        L.llsr_fusion_aft_mapped.argtypes = [C.POINTER(_abi.FusionState), C.POINTER(_abi.OdometryMsg)]
        L.llsr_shadow_points.argtypes = [C.c_void_p]
        L.llsr_integrate_transformation.argtypes = [C.c_void_p, C.c_void_p]
        L.llsr_transform_to_end.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.llsr_scan2scan_reserve.argtypes = [C.c_void_p] + [C.c_int32] * 5
        L.llsr_scan2scan_batch.argtypes = [C.c_void_p, C.POINTER(_abi.S2SBatch), C.c_void_p]
        L.llsr_scan2scan_check.argtypes = [C.c_void_p]
        L.llsr_scan2scan.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                     C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.POINTER(_abi.S2SReport)]
        L.llsr_scan2map.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                    C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(_abi.LmReport)]
        L.llsr_scan2map_shard_begin.argtypes = [C.c_void_p, C.POINTER(_abi.S2MBatch), C.c_void_p]
        L.llsr_scan2map_shard_partial.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.llsr_scan2map_shard_step.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
        L.llsr_scan2map_shard_end.argtypes = [C.c_void_p, C.c_void_p]
        L.llsr_odometry_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.llsr_odometry_fetch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_abi.OdomSlot)] + [C.c_void_p] * 4
        L.llsr_odometry_reset.argtypes = [C.c_void_p]
        L.llsr_odometry_batch_odom.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        L.llsr_odometry_fetch_lm.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.llsr_mapping_batch_odom.argtypes = L.llsr_odometry_batch_odom.argtypes
        L.llsr_odom_init.argtypes = [C.POINTER(_abi.OdomState)]
        L.llsr_odom_callback.argtypes = [C.POINTER(_abi.OdomState), C.POINTER(_abi.OdometryMsg)]
        L.llsr_update_initial_guess.argtypes = [C.POINTER(_abi.OdomSample), C.c_void_p, C.c_void_p]
        L.llsr_imu_init.argtypes = [C.POINTER(_abi.ImuStateStruct)]
        L.llsr_imu_callback.argtypes = [C.POINTER(_abi.ImuStateStruct), C.POINTER(_abi.ImuMsg), C.c_float]
        L.llsr_imu_scan_window.argtypes = [C.POINTER(_abi.ImuStateStruct), C.c_void_p, C.POINTER(C.c_int32)]
        L.llsr_imu_deskew_host.argtypes = [C.POINTER(Config), C.c_int32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p,
                                           C.c_int32, C.c_void_p, C.POINTER(_abi.ImuCarry), C.c_void_p,
                                           C.POINTER(_abi.ImuReport)]
        L.llsr_stage_imu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.llsr_fetch_imu_report.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_abi.ImuReport)]
        L.llsr_set_imu_undistortion.argtypes = [C.c_void_p, C.c_int32]
        L.llsr_integrate_transformation_imu.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_abi.ImuReport)]
        L.llsr_transform_to_end_imu.argtypes = [C.c_void_p, C.POINTER(_abi.ImuReport), C.c_void_p, C.c_int32,
                                                C.c_void_p]
        L.llsr_first_scan_imu.argtypes = [C.c_void_p, C.POINTER(_abi.ImuReport)]
        L.llsr_map_config_default.argtypes = [C.POINTER(_abi.MapConfig)]
        L.llsr_map_config_lidar.argtypes = [C.POINTER(_abi.MapConfig), C.c_int32]
        L.llsr_map_create.argtypes = [C.POINTER(_abi.MapConfig), C.c_int32]
        L.llsr_map_destroy.argtypes = [C.c_void_p]
        L.llsr_map_last_error.argtypes = [C.c_void_p]
        L.llsr_map_reset.argtypes = [C.c_void_p]
        L.llsr_map_voxel_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
        L.llsr_map_downsample_scan.argtypes = [C.c_void_p] + [C.c_void_p, C.c_int32] * 5 + [C.c_void_p] * 3
        L.llsr_map_add_keyframe.argtypes = [C.c_void_p, C.c_void_p] + [C.c_void_p, C.c_int32] * 3 + [C.c_void_p]
        L.llsr_map_num_keyframes.argtypes = [C.c_void_p]
        L.llsr_map_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                       C.POINTER(_abi.MapReport), C.c_void_p]
        L.llsr_map_keyframe_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.llsr_global_map_config_default.argtypes = [C.POINTER(_abi.GlobalMapConfig)]
        _gm_out = [C.c_void_p, C.c_int64] * 3 + [C.POINTER(_abi.GlobalMapReport), C.c_void_p]
        L.llsr_map_global.argtypes = [C.c_void_p, C.POINTER(_abi.GlobalMapConfig), C.c_void_p] + _gm_out
        L.llsr_mapping_global_map.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_abi.GlobalMapConfig)] + _gm_out
        _save = [C.c_void_p, C.c_int64] * 2 + [C.POINTER(C.c_int64)] * 2 + [C.c_void_p]
        L.llsr_map_save.argtypes = [C.c_void_p] + _save
        L.llsr_mapping_save_map.argtypes = [C.c_void_p, C.c_int32] + _save
        L.llsr_keypose_radius_sorted.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_void_p]
        L.llsr_loop_config_lidar.argtypes = [C.POINTER(_abi.LoopConfig), C.c_int32]
        L.llsr_map_set_keyframe_time.argtypes = [C.c_void_p, C.c_int32, C.c_double]
        L.llsr_map_keyframe_times.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.llsr_map_set_key_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.llsr_loop_candidate.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_float,
                                          C.c_double]
        L.llsr_umeyama3.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.llsr_loop_constraint.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                           C.c_void_p]
        L.llsr_icp_align_host.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(_abi.LoopConfig),
                                          C.POINTER(_abi.IcpResult), C.c_void_p]
        L.llsr_icp_create.argtypes = [C.c_int32]
        L.llsr_icp_destroy.argtypes = [C.c_void_p]
        L.llsr_icp_last_error.argtypes = [C.c_void_p]
        L.llsr_icp_align.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(_abi.LoopConfig),
                                     C.POINTER(_abi.IcpResult), C.c_void_p, C.c_void_p]
        L.llsr_icp_last_times.argtypes = [C.c_void_p] + [C.POINTER(C.c_float)] * 3
        L.llsr_icp_align_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.llsr_icp_last_passes.argtypes = [C.c_void_p]
        L.llsr_mapping_stage_times.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.llsr_mapping_keyframe_times.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.llsr_mapping_loop_closure.argtypes = [C.c_void_p, C.POINTER(_abi.LoopConfig), C.c_int32, C.c_void_p,
                                                C.c_void_p]
        L.llsr_mapping_set_key_poses.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        L.llsr_pg_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64]
        L.llsr_pg_destroy.argtypes = [C.c_void_p]
        L.llsr_pg_last_error.argtypes = [C.c_void_p]
        L.llsr_pg_config_default.argtypes = [C.POINTER(_abi.PgConfig)]
        L.llsr_pg_reset.argtypes = [C.c_void_p, C.c_int32]
        L.llsr_pg_append.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.llsr_pg_add_loop.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_float]
        L.llsr_pg_optimize.argtypes = [C.c_void_p, C.POINTER(_abi.PgConfig), C.c_void_p, C.c_void_p]
        L.llsr_pg_poses.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.llsr_mapping_enable_pose_graph.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.llsr_mapping_close_loops.argtypes = [C.c_void_p, C.POINTER(_abi.LoopConfig), C.POINTER(_abi.PgConfig),
                                               C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.llsr_mapping_pose_graph_poses.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.llsr_prior_config_default.argtypes = [C.POINTER(_abi.PriorConfig)]
        L.llsr_prior_create.argtypes = [C.POINTER(_abi.PriorConfig), C.c_int32]
        L.llsr_prior_destroy.argtypes = [C.c_void_p]
        L.llsr_prior_last_error.argtypes = [C.c_void_p]
        L.llsr_prior_load.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        L.llsr_prior_info.argtypes = [C.c_void_p, C.POINTER(_abi.PriorReport)]
        L.llsr_prior_points.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        L.llsr_prior_tile_starts.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
        L.llsr_prior_crop_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
        L.llsr_prior_last_crop.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_int64)]
        L.llsr_mapping_set_prior.argtypes = [C.c_void_p, C.c_void_p]
        L.llsr_mapping_set_pose.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        _loop = [C.POINTER(_abi.LoopConfig), C.c_void_p, C.c_double, C.POINTER(_abi.LoopReport)]
        L.llsr_map_loop_submaps.argtypes = [C.c_void_p] + _loop + [C.c_void_p, C.c_int64] * 4 + [C.c_void_p]
        L.llsr_map_loop_closure.argtypes = [C.c_void_p, C.c_void_p] + _loop + [C.c_void_p, C.c_int64] * 2 + [C.c_void_p]
        L.llsr_mapping_init.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_abi.MapConfig)]
        L.llsr_mapping_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.llsr_mapping_fetch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_abi.MappingSlot)]
        L.llsr_mapping_keyposes.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.llsr_mapping_reset.argtypes = [C.c_void_p]
        L.llsr_mapping_associate.argtypes = [C.c_void_p] * 6
        L.llsr_set_voxel_order.argtypes = [C.c_void_p, C.c_int32]
        L.llsr_decode_pointcloud2.argtypes = [C.POINTER(_abi.Pc2Layout), C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.llsr_kitti_count.argtypes = [C.c_char_p]
        L.llsr_kitti_read.argtypes = [C.c_char_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
        L.llsr_kitti_load.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_void_p, C.c_void_p]
        for fn in EXPORTS:
            if fn not in ("llsr_last_error", "llsr_kernel_name", "llsr_destroy", "llsr_map_create",
                          "llsr_map_destroy", "llsr_map_last_error", "llsr_build_id", "llsr_icp_create",
                          "llsr_icp_destroy", "llsr_icp_last_error", "llsr_pg_create", "llsr_pg_destroy",
                          "llsr_pg_last_error", "llsr_prior_create", "llsr_prior_destroy", "llsr_prior_last_error",
                          "llsr_prior_points", "llsr_prior_tile_starts"):
                getattr(L, fn).restype = C.c_int32
        L.llsr_prior_create.restype = C.c_void_p
        L.llsr_prior_destroy.restype = None
        L.llsr_prior_last_error.restype = C.c_char_p
        L.llsr_prior_points.restype = C.c_int64
        L.llsr_prior_tile_starts.restype = C.c_int64
        L.llsr_destroy.restype = None
        L.llsr_map_create.restype = C.c_void_p
        L.llsr_map_destroy.restype = None
        L.llsr_map_last_error.restype = C.c_char_p
        L.llsr_icp_create.restype = C.c_void_p
        L.llsr_icp_destroy.restype = None
        L.llsr_icp_last_error.restype = C.c_char_p
        L.llsr_pg_create.restype = C.c_void_p
        L.llsr_pg_destroy.restype = None
        L.llsr_pg_last_error.restype = C.c_char_p
        _LIB = L
    return _LIB


def default_config(lidar: str, horizontal: int | None = None) -> Config:
    c = Config()
    code = {"vlp16": _abi.LLSR_LIDAR_VLP16, "vlp32c": _abi.LLSR_LIDAR_VLP32C,
            "hdl64e": _abi.LLSR_LIDAR_HDL64E}[lidar]
    rc = lib().llsr_config_default(C.byref(c), code)
    if rc != 0:
        raise LlsrError(f"llsr_config_default: {rc}")
    if horizontal is not None:
        c.num_horizontal_scans = horizontal
    return c


class Pipeline:
    """One llsr handle: ImageProjection + FeatureAssociation feature stage on a HIP device."""

    def __init__(self, cfg: Config, device: int = 0, max_batch: int = 1, max_points: int | None = None):
        self.cfg = cfg
        H, W = cfg.num_vertical_scans, cfg.num_horizontal_scans
        self.max_points = max_points or 2 * H * W
        self.max_batch = max_batch
        self.device = device
        self._gm_caps = {}  # mapping_global_map's output capacities per slot
        h = C.c_void_p()
        rc = lib().llsr_create(C.byref(cfg), device, max_batch, self.max_points, C.byref(h))
        if rc != 0:
            raise LlsrError(f"llsr_create failed ({rc}): no HIP device or invalid config")
        self._h = h
        self.out = _abi.OutBuffers(H, W)

    def close(self):
        if getattr(self, "_h", None):
            lib().llsr_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc, what):
        if rc != 0:
            e = LlsrError(f"{what} failed ({rc}): {lib().llsr_last_error(self._h).decode()}")
            e.code = rc
            raise e

    def reset(self):
        self._check(lib().llsr_reset_state(self._h), "llsr_reset_state")

    def set_voxel_order(self, order: int):
        """_abi.LLSR_VOXEL_ORDER_PCL (default: the reference's std::sort order) or LLSR_VOXEL_ORDER_INPUT
        (ring order inside each voxel) for the less-flat VoxelGrid."""
        self._check(lib().llsr_set_voxel_order(self._h, order), "llsr_set_voxel_order")

    def set_imu_undistortion(self, on: bool):
        """llsr_set_imu_undistortion: the reference's use_imu_undistortion switch for this handle's
        odometry (default off; takes effect at the next batch, kept across the reset calls)."""
        self._check(lib().llsr_set_imu_undistortion(self._h, 1 if on else 0), "llsr_set_imu_undistortion")

    def process_scan(self, xyzi: np.ndarray) -> dict:
        xyzi = np.ascontiguousarray(xyzi, dtype=np.float32).reshape(-1, 4)
        self._check(lib().llsr_process_scan(self._h, xyzi.ctypes.data, xyzi.shape[0], C.byref(self.out.struct)),
                    "llsr_process_scan")
        return self.out.result()

    def process_batch(self, d_xyzi: int, d_offsets: int, B: int, stream: int = 0):
        """Enqueue B device-resident scans (raw device pointers) on a hipStream_t (0 = own)."""
        self._check(lib().llsr_process_batch(self._h, C.c_void_p(d_xyzi), C.c_void_p(d_offsets), B,
                                             C.c_void_p(stream)), "llsr_process_batch")

    def fetch(self, b: int) -> dict:
        self._check(lib().llsr_fetch_scan(self._h, b, C.byref(self.out.struct)), "llsr_fetch_scan")
        return self.out.result()

    def stage_imu(self, scan_stamps, windows):
        """llsr_stage_imu: arm this handle's next batch call with the slots' IMU windows. scan_stamps:
        B (sec, nanosec) pairs of the segmented clouds' headers; windows: B entries, each None / empty
        (slot without IMU) or ImuState.scan_window()'s structured array (n + 1 samples)."""
        B = len(scan_stamps)
        sec = np.array([s[0] for s in scan_stamps], np.int32)
        nsec = np.array([s[1] for s in scan_stamps], np.uint32)
        ws = [np.zeros(0, IMU_SAMPLE_DTYPE) if w is None else np.ascontiguousarray(w, IMU_SAMPLE_DTYPE) for w in windows]
        if len(ws) != B:
            raise ValueError("one window per scan stamp")
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum([len(w) for w in ws])
        samples = np.concatenate(ws) if B else np.zeros(0, IMU_SAMPLE_DTYPE)
        self._check(lib().llsr_stage_imu(self._h, sec.ctypes.data, nsec.ctypes.data, samples.ctypes.data,
                                         off.ctypes.data, B), "llsr_stage_imu")

    def fetch_imu_report(self, b: int) -> dict:
        """llsr_fetch_imu_report: slot b's IMU members after the last batch, {field: float32 [3]}."""
        r = _abi.ImuReport()
        self._check(lib().llsr_fetch_imu_report(self._h, b, C.byref(r)), "llsr_fetch_imu_report")
        return imu_report_dict(r)

    def fetch_vis_clouds(self, b: int) -> dict:
        """publishClouds' visualization clouds of slot b (llsr_fetch_vis_clouds): {name: float32 [n, 4]}."""
        HW = self.cfg.num_vertical_scans * self.cfg.num_horizontal_scans
        bufs = {name: np.zeros((HW, 4), np.float32) for name, _ in _abi.VIS_CLOUDS}
        v = _abi.VisOut(*(bufs[name].ctypes.data for name, _ in _abi.VIS_CLOUDS))
        self._check(lib().llsr_fetch_vis_clouds(self._h, b, C.byref(v)), "llsr_fetch_vis_clouds")
        return {name: bufs[name][: (HW if cnt is None else getattr(v, cnt))].copy() for name, cnt in _abi.VIS_CLOUDS}

    def batch_counts(self, B: int) -> np.ndarray:
        buf = np.zeros((B, 8), dtype=np.int32)
        self._check(lib().llsr_batch_counts(self._h, buf.ctypes.data), "llsr_batch_counts")
        return buf

    def set_profiling(self, on: bool):
        self._check(lib().llsr_set_profiling(self._h, 1 if on else 0), "llsr_set_profiling")

    def debug_phase_ms(self, kernel: int, phase: int, reps: int = 5) -> float:
        """Diagnostics: mean ms of kernel `kernel` re-launched with an early exit at `phase`."""
        f = lib().llsr_debug_phase_ms
        f.restype, f.argtypes = C.c_float, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        return float(f(self._h, kernel, phase, reps))

    def debug_s2s_prof(self, out: np.ndarray) -> int:
        """Diagnostics build (libllsr_prof.so): the last scan-to-scan launch's per-problem phase ticks
        into out (float32 [P, 8]); returns the number of problems copied."""
        f = lib().llsr_debug_s2s_prof
        f.restype, f.argtypes = C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32]
        n = f(self._h, out.ctypes.data, out.shape[0])
        if n < 0:
            raise LlsrError(f"llsr_debug_s2s_prof: {n}")
        return n

    def kernel_times(self) -> dict:
        buf = np.zeros(32, dtype=np.float32)
        n = lib().llsr_kernel_times_ms(self._h, buf.ctypes.data, 32)
        if n < 0:
            self._check(n, "llsr_kernel_times_ms")
        return {lib().llsr_kernel_name(k).decode(): float(buf[k]) for k in range(n)}

    def row_bins(self, b: int = 0) -> np.ndarray:
        """use_vlp32c handles: slot b's vertical_raw2 of the last batch (llsr_row_bins), the ascending
        distinct elevation bins observed in the scan; more than num_vertical_scans of them means
        the scan overflowed and its points of rank >= H were dropped."""
        bins = np.zeros(512, dtype=np.int32)
        n = C.c_int32(0)
        self._check(lib().llsr_row_bins(self._h, b, C.byref(n), bins.ctypes.data, bins.size), "llsr_row_bins")
        return bins[: n.value].copy()

    # ---- scan-to-map (MapOptimization) -------------------------------------------------------
    def scan2map_reserve(self, problems: int, corner_map: int, surf_map: int, corner_q: int, surf_q: int):
        self._check(lib().llsr_scan2map_reserve(self._h, problems, corner_map, surf_map, corner_q, surf_q),
                    "llsr_scan2map_reserve")

    def scan2map(self, corner_q, surf_q, corner_map, surf_map, pose) -> dict:
        """One problem from host arrays ((n, 4) float32 clouds, pose[6]); returns the report."""
        arrs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4) for a in (corner_q, surf_q, corner_map, surf_map)]
        pose = np.ascontiguousarray(pose, dtype=np.float32).copy()
        rep = _abi.LmReport()
        args = []
        for a in arrs:
            args += [C.c_void_p(a.ctypes.data if len(a) else None), len(a)]
        self._check(lib().llsr_scan2map(self._h, *args, pose.ctypes.data, C.byref(rep)), "llsr_scan2map")
        d = rep.as_dict()
        d["pose"] = pose
        return d

    @staticmethod
    def _s2m_batch(ptrs: dict, P: int) -> _abi.S2MBatch:
        b = _abi.S2MBatch()
        b.n_problems = P
        for k, v in ptrs.items():
            setattr(b, k, v)
        return b

    def scan2map_batch(self, ptrs: dict, P: int, stream: int = 0):
        """Device-resident batch: ptrs maps the llsr_s2m_batch field names to device pointers."""
        b = self._s2m_batch(ptrs, P)
        self._check(lib().llsr_scan2map_batch(self._h, C.byref(b), C.c_void_p(stream)), "llsr_scan2map_batch")

    # split-correspondence mode (llsr_scan2map_shard_*): the LM loop is the caller's (llsr.dist)
    def scan2map_shard_begin(self, ptrs: dict, P: int, stream: int = 0):
        b = self._s2m_batch(ptrs, P)
        self._check(lib().llsr_scan2map_shard_begin(self._h, C.byref(b), C.c_void_p(stream)),
                    "llsr_scan2map_shard_begin")

    def scan2map_shard_partial(self, rank: int, world: int, d_ne: int, stream: int = 0):
        self._check(lib().llsr_scan2map_shard_partial(self._h, rank, world, C.c_void_p(d_ne), C.c_void_p(stream)),
                    "llsr_scan2map_shard_partial")

    def scan2map_shard_step(self, d_ne: int, poll: bool, stream: int = 0) -> int:
        """Solve from the summed words; with poll, sync and return the problems still active
        (else -1)."""
        n = C.c_int32(-1)
        self._check(lib().llsr_scan2map_shard_step(self._h, C.c_void_p(d_ne), C.byref(n) if poll else None,
                                                    C.c_void_p(stream)), "llsr_scan2map_shard_step")
        return int(n.value)

    def scan2map_shard_end(self, stream: int = 0):
        self._check(lib().llsr_scan2map_shard_end(self._h, C.c_void_p(stream)), "llsr_scan2map_shard_end")


    def scan2map_stats(self) -> dict:
        st = _abi.S2MStats()
        self._check(lib().llsr_scan2map_stats(self._h, C.byref(st)), "llsr_scan2map_stats")
        return {k: getattr(st, k) for k, _ in st._fields_}


    def scan2scan_stats(self) -> dict:
        st = _abi.S2SStats()
        self._check(lib().llsr_scan2scan_stats(self._h, C.byref(st)), "llsr_scan2scan_stats")
        return {k: getattr(st, k) for k, _ in st._fields_}

    # ---- scan-to-scan (FeatureAssociation::updateTransformation) ------------------------------
    def scan2scan_reserve(self, problems: int, sharp: int, flat: int, corner_last: int, surf_last: int):
        self._check(lib().llsr_scan2scan_reserve(self._h, problems, sharp, flat, corner_last, surf_last),
                    "llsr_scan2scan_reserve")

    def scan2scan(self, sharp, flat, corner_last, surf_last, transform_cur, is_degenerate: int = 0) -> dict:
        """One scan from host arrays; returns the report (+ transform_cur, is_degenerate)."""
        arrs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4) for a in (sharp, flat, corner_last, surf_last)]
        t = np.ascontiguousarray(transform_cur, dtype=np.float32).copy()
        deg = C.c_int32(is_degenerate)
        rep = _abi.S2SReport()
        args = []
        for a in arrs:
            args += [C.c_void_p(a.ctypes.data if len(a) else None), len(a)]
        self._check(lib().llsr_scan2scan(self._h, *args, t.ctypes.data, C.byref(deg), C.byref(rep)), "llsr_scan2scan")
        d = rep.as_dict()
        d["transform_cur"] = t
        d["is_degenerate"] = deg.value
        return d

    def scan2scan_batch(self, ptrs: dict, P: int, stream: int = 0):
        b = _abi.S2SBatch()
        b.n_problems = P
        for k, v in ptrs.items():
            setattr(b, k, v)
        self._check(lib().llsr_scan2scan_batch(self._h, C.byref(b), C.c_void_p(stream)), "llsr_scan2scan_batch")

    def scan2scan_check(self):
        self._check(lib().llsr_scan2scan_check(self._h), "llsr_scan2scan_check")


    # ---- end-to-end odometry (runFeatureAssociation) -------------------------------------------
    def odometry_batch(self, d_xyzi: int, d_offsets: int, B: int, stream: int = 0):
        """One device-resident scan per slot through features + scan-to-scan LM + last clouds."""
        self._check(lib().llsr_odometry_batch(self._h, C.c_void_p(d_xyzi), C.c_void_p(d_offsets), B,
                                              C.c_void_p(stream)), "llsr_odometry_batch")

    def odometry_fetch(self, b: int, clouds: bool = False) -> dict:
        st = _abi.OdomSlot()
        cap = self.cfg.num_vertical_scans * self.cfg.num_horizontal_scans + 160
        bufs = [np.zeros((cap, 4), np.float32) for _ in range(4)] if clouds else [None] * 4
        ptrs = [C.c_void_p(a.ctypes.data) if a is not None else None for a in bufs]
        self._check(lib().llsr_odometry_fetch(self._h, b, C.byref(st), *ptrs), "llsr_odometry_fetch")
        d = {k: getattr(st, k) for k in ("frames", "n_corner_last", "n_surf_last", "n_corner_scan", "n_surf_scan")}
        d["transform_cur"] = np.array(st.transform_cur[:], np.float32)
        d["transform_sum"] = np.array(st.transform_sum[:], np.float32)
        d["lm"] = st.lm.as_dict()
        if clouds:
            for name, a, n in zip(("corner_last", "surf_last", "corner_scan", "surf_scan"), bufs,
                                  (st.n_corner_last, st.n_surf_last, st.n_corner_scan, st.n_surf_scan)):
                d[name] = a[:n].copy()
        return d

    @staticmethod
    def _odom_args(samples, overwrite, B: int):
        """samples: B sequences of roll, pitch, yaw, x, y, z (or _abi.OdomSample); overwrite: B flags or None."""
        if isinstance(samples, C.Array) and samples._type_ is _abi.OdomSample and len(samples) >= B:
            arr = samples  # a caller-built llsr_odom_sample[B] goes through as it is
        else:
            arr = (_abi.OdomSample * B)()
            for b in range(B):
                v = samples[b]
                arr[b] = v if isinstance(v, _abi.OdomSample) else _abi.OdomSample(*(float(x) for x in v))
        flags = None if overwrite is None else np.ascontiguousarray(overwrite, np.uint8).reshape(B)
        return arr, flags

    def odometry_batch_odom(self, d_xyzi: int, d_offsets: int, B: int, samples, overwrite=None, stream: int = 0):
        """odometry_batch with updateInitialGuess after the LM (FA:2790): samples[b] is slot b's latest
        /odom2 sample, overwrite[b] selects the slots it applies to (None: every slot)."""
        arr, flags = self._odom_args(samples, overwrite, B)
        self._check(lib().llsr_odometry_batch_odom(self._h, C.c_void_p(d_xyzi), C.c_void_p(d_offsets), B, arr,
                                                   None if flags is None else flags.ctypes.data,
                                                   C.c_void_p(stream)), "llsr_odometry_batch_odom")

    def odometry_fetch_lm(self, b: int) -> np.ndarray:
        """The LM's own transformCur of slot b's last scan (before updateInitialGuess replaced it)."""
        out = np.zeros(6, np.float32)
        self._check(lib().llsr_odometry_fetch_lm(self._h, b, out.ctypes.data), "llsr_odometry_fetch_lm")
        return out

    def odometry_reset(self):
        self._check(lib().llsr_odometry_reset(self._h), "llsr_odometry_reset")

    # ---- mapping chain (FeatureAssociation -> MapOptimization::run) ----------------------------
    def mapping_init(self, mo_mode: int = _abi.LLSR_MODE_LM_APPLIED, map_cfg: _abi.MapConfig | None = None):
        """Per-slot MapOptimization state; mo_mode is MapOptimization's LM mode."""
        self._check(lib().llsr_mapping_init(self._h, mo_mode, C.byref(map_cfg) if map_cfg is not None else None),
                    "llsr_mapping_init")

    def mapping_batch(self, d_xyzi: int, d_offsets: int, B: int, stream: int = 0):
        """One device-resident scan per slot through IP + FA + odometry + MapOptimization."""
        self._check(lib().llsr_mapping_batch(self._h, C.c_void_p(d_xyzi), C.c_void_p(d_offsets), B,
                                             C.c_void_p(stream)), "llsr_mapping_batch")

    def mapping_batch_odom(self, d_xyzi: int, d_offsets: int, B: int, samples, overwrite=None, stream: int = 0):
        """mapping_batch over odometry_batch_odom (same samples / overwrite arguments)."""
        arr, flags = self._odom_args(samples, overwrite, B)
        self._check(lib().llsr_mapping_batch_odom(self._h, C.c_void_p(d_xyzi), C.c_void_p(d_offsets), B, arr,
                                                  None if flags is None else flags.ctypes.data,
                                                  C.c_void_p(stream)), "llsr_mapping_batch_odom")

    def mapping_fetch(self, b: int) -> dict:
        st = _abi.MappingSlot()
        self._check(lib().llsr_mapping_fetch(self._h, b, C.byref(st)), "llsr_mapping_fetch")
        d = {k: getattr(st, k) for k in ("frames", "mo_frames", "keyframes", "lm_ran", "n_corner_q", "n_surf_q")}
        for k in ("transform_sum", "transform_tobe_mapped", "transform_bef_mapped", "transform_aft_mapped"):
            d[k] = np.array(getattr(st, k)[:], np.float32)
        d["lm"] = st.lm.as_dict()
        d["map"] = st.map.as_dict()
        return d

    def mapping_keyposes(self, b: int) -> np.ndarray:
        n = lib().llsr_mapping_keyposes(self._h, b, None, 0)
        if n < 0:
            self._check(n, "llsr_mapping_keyposes")
        out = np.zeros((max(n, 1), 6), np.float32)
        lib().llsr_mapping_keyposes(self._h, b, out.ctypes.data, n)
        return out[:n].copy()

    def mapping_reset(self):
        self._check(lib().llsr_mapping_reset(self._h), "llsr_mapping_reset")

    def mapping_global_map(self, b: int, cfg: _abi.GlobalMapConfig | None = None, edge: bool = True,
                           planar: bool = True, stream: int = 0) -> dict:
        """publishGlobalMap on slot b's keyframes (llsr_mapping_global_map), around the slot's
        transformAftMapped position: as LocalMap.global_map."""
        import torch
        caps = self._gm_caps.setdefault(b, [1, 1, 1])
        call = lambda *out: lib().llsr_mapping_global_map(  # noqa: E731
            self._h, b, C.byref(cfg) if cfg is not None else None, *out, C.c_void_p(stream))
        r = _global_map(torch, torch.device("cuda", self.device), call, caps, edge, planar)
        self._check(r.pop("rc"), "llsr_mapping_global_map")
        return r

    def mapping_save_map(self, b: int, stream: int = 0):
        """saveMapService's (cornerMap, surfaceMap) of slot b (llsr_mapping_save_map)."""
        import torch
        call = lambda *out: lib().llsr_mapping_save_map(self._h, b, *out, C.c_void_p(stream))  # noqa: E731
        rc, c, su = _save_map(torch, torch.device("cuda", self.device), call)
        self._check(rc, "llsr_mapping_save_map")
        return c, su

    def mapping_stage_times(self, seconds):
        """timeLaserOdometry.seconds() of each slot's scan in the next mapping_batch / _batch_odom call
        (llsr_mapping_stage_times): stamps the keyframes that call saves."""
        t = np.ascontiguousarray(seconds, np.float64).reshape(-1)
        self._check(lib().llsr_mapping_stage_times(self._h, t.ctypes.data, len(t)), "llsr_mapping_stage_times")

    def mapping_keyframe_times(self, b: int) -> np.ndarray:
        """cloudKeyPoses6D[*].time of slot b (llsr_mapping_keyframe_times): NaN where none was staged."""
        n = lib().llsr_mapping_keyframe_times(self._h, b, None, 0)
        if n < 0:
            self._check(n, "llsr_mapping_keyframe_times")
        out = np.zeros(max(n, 1), np.float64)
        lib().llsr_mapping_keyframe_times(self._h, b, out.ctypes.data, n)
        return out[:n].copy()

    def mapping_loop_closure(self, B: int, cfg: _abi.LoopConfig | None = None, stream: int = 0) -> list:
        """detectLoopClosure + performLoopClosure of slots 0 .. B - 1 with one batched alignment
        (llsr_mapping_loop_closure): one llsr_loop_report dict per slot."""
        reps = (_abi.LoopReport * B)()
        self._check(lib().llsr_mapping_loop_closure(self._h, C.byref(cfg) if cfg is not None else None, B, reps,
                                                    C.c_void_p(stream)), "llsr_mapping_loop_closure")
        return [r.as_dict() for r in reps]

    def mapping_set_key_poses(self, b: int, poses6, latest_estimate=None):
        """correctPoses on slot b (llsr_mapping_set_key_poses): the first len(poses6) key poses (x, y, z,
        roll, pitch, yaw) and, when given, iSAM2's latestEstimate in transform_aft_mapped's layout."""
        p = np.ascontiguousarray(poses6, np.float32).reshape(-1, 6)
        e = None if latest_estimate is None else np.ascontiguousarray(latest_estimate, np.float32).reshape(6)
        self._check(lib().llsr_mapping_set_key_poses(self._h, b, p.ctypes.data, len(p),
                                                     None if e is None else e.ctypes.data),
                    "llsr_mapping_set_key_poses")


    def mapping_set_prior(self, prior: "PriorMap | None"):
        """Localisation mode (llsr_mapping_set_prior): every slot's local map becomes the crop of
        `prior` (a PriorMap on this device; None detaches). Only directly after mapping_init or
        mapping_reset. The Pipeline keeps a reference: the prior outlives the attachment."""
        self._check(lib().llsr_mapping_set_prior(self._h, prior._w if prior is not None else None),
                    "llsr_mapping_set_prior")
        self._prior = prior

    def mapping_set_pose(self, b: int, pose6):
        """The /initialpose of slot b (llsr_mapping_set_pose): pose6 in transform_aft_mapped's layout."""
        p = np.ascontiguousarray(pose6, np.float32).reshape(6)
        self._check(lib().llsr_mapping_set_pose(self._h, b, p.ctypes.data), "llsr_mapping_set_pose")

    def mapping_enable_pose_graph(self, on: bool = True, max_loops: int = 16):
        """Keep a pose graph per slot (llsr_mapping_enable_pose_graph): every keyframe a slot saves from
        now on is appended to it; mapping_close_loops optimises the graphs."""
        self._check(lib().llsr_mapping_enable_pose_graph(self._h, int(bool(on)), max_loops),
                    "llsr_mapping_enable_pose_graph")

    def mapping_close_loops(self, B: int, cfg: _abi.LoopConfig | None = None, pg_cfg: _abi.PgConfig | None = None,
                            stream: int = 0):
        """The loop closure of slots 0 .. B - 1 through to the corrected key poses
        (llsr_mapping_close_loops): the loop reports and the pose-graph reports, one dict per slot each."""
        reps, pg = (_abi.LoopReport * B)(), (_abi.PgReport * B)()
        self._check(lib().llsr_mapping_close_loops(self._h, C.byref(cfg) if cfg is not None else None,
                                                   C.byref(pg_cfg) if pg_cfg is not None else None, B, reps, pg,
                                                   C.c_void_p(stream)), "llsr_mapping_close_loops")
        return [r.as_dict() for r in reps], [r.as_dict() for r in pg]

    def mapping_pose_graph_poses(self, b: int) -> np.ndarray:
        """Slot b's graph estimate, (K, 6) x, y, z, roll, pitch, yaw (llsr_mapping_pose_graph_poses)."""
        n = lib().llsr_mapping_pose_graph_poses(self._h, b, None, 0)
        if n < 0:
            self._check(n, "llsr_mapping_pose_graph_poses")
        out = np.zeros((max(n, 1), 6), np.float32)
        lib().llsr_mapping_pose_graph_poses(self._h, b, out.ctypes.data, n)
        return out[:n].copy()


def mapping_associate(transform_sum_fa, bef, aft):
    """Host-only pose glue of the mapping chain (llsr_mapping_associate): OdometryToTransform then
    transformAssociateToMap; returns (transform_sum, transform_tobe_mapped, transform_incre)."""
    a = [np.ascontiguousarray(x, np.float32) for x in (transform_sum_fa, bef, aft)]
    out = [np.zeros(6, np.float32) for _ in range(3)]
    rc = lib().llsr_mapping_associate(*(x.ctypes.data for x in a), *(x.ctypes.data for x in out))
    if rc != 0:
        raise LlsrError(f"llsr_mapping_associate: {rc}")
    return tuple(out)


def _msg_to_array(m: "_abi.OdometryMsg") -> np.ndarray:
    return np.array(list(m.orientation) + list(m.position) + list(m.twist_angular) + list(m.twist_linear),
                    np.float64)


def _array_to_msg(a) -> "_abi.OdometryMsg":
    a = np.asarray(a, np.float64)
    m = _abi.OdometryMsg()
    m.orientation[:] = a[0:4].tolist()
    m.position[:] = a[4:7].tolist()
    m.twist_angular[:] = a[7:10].tolist()
    m.twist_linear[:] = a[10:13].tolist()
    return m


def pose_to_odometry(pose, twist=None) -> np.ndarray:
    """The publishers' pose -> nav_msgs/Odometry encoding (llsr_pose_to_odometry: FA:2612-2625,
    MO:704-723, TF:193-206), as 13 doubles: orientation xyzw, position, twist angular, twist linear."""
    p = np.ascontiguousarray(pose, np.float32)
    t = None if twist is None else np.ascontiguousarray(twist, np.float32)
    m = _abi.OdometryMsg()
    rc = lib().llsr_pose_to_odometry(p.ctypes.data, None if t is None else t.ctypes.data, C.byref(m))
    if rc != 0:
        raise LlsrError(f"llsr_pose_to_odometry: {rc}")
    return _msg_to_array(m)


def odometry_to_transform(msg) -> np.ndarray:
    """OdometryToTransform (UT:99-113) of a 13-double odometry message."""
    out = np.zeros(6, np.float32)
    m = _array_to_msg(msg)
    rc = lib().llsr_odometry_to_transform(C.byref(m), out.ctypes.data)
    if rc != 0:
        raise LlsrError(f"llsr_odometry_to_transform: {rc}")
    return out


class TransformFusion:
    """The TransformFusion node's arithmetic (transformFusion.cpp) over the C-ABI's host entry points:
    `laser_odometry_handler(msg)` takes /laser_odom_to_init and returns /integrated_to_init (TF:188-280),
    `odom_aft_mapped_handler(msg)` takes /aft_mapped_to_init (TF:282-304). Messages are 13 doubles."""

    def __init__(self):
        self.state = _abi.FusionState()
        rc = lib().llsr_fusion_init(C.byref(self.state))
        if rc != 0:
            raise LlsrError(f"llsr_fusion_init: {rc}")

    def laser_odometry_handler(self, msg) -> np.ndarray:
        m, out = _array_to_msg(msg), _abi.OdometryMsg()
        rc = lib().llsr_fusion_laser_odometry(C.byref(self.state), C.byref(m), C.byref(out))
        if rc != 0:
            raise LlsrError(f"llsr_fusion_laser_odometry: {rc}")
        return _msg_to_array(out)

    def odom_aft_mapped_handler(self, msg):
        m = _array_to_msg(msg)
        rc = lib().llsr_fusion_aft_mapped(C.byref(self.state), C.byref(m))
        if rc != 0:
            raise LlsrError(f"llsr_fusion_aft_mapped: {rc}")

    def state_array(self) -> np.ndarray:
        """transformSum, transformIncre, transformMapped, transformBefMapped, transformAftMapped."""
        st = self.state
        return np.concatenate([np.array(getattr(st, f), np.float32) for f, _ in st._fields_])


IMU_SAMPLE_DTYPE = np.dtype([("time", np.float64), ("roll", np.float32), ("pitch", np.float32), ("yaw", np.float32),
                             ("velo", np.float32, 3), ("shift", np.float32, 3),
                             ("angular_rotation", np.float32, 3)])
assert IMU_SAMPLE_DTYPE.itemsize == C.sizeof(_abi.ImuSample)


def imu_report_dict(r: "_abi.ImuReport") -> dict:
    return {f: np.array(getattr(r, f), np.float32) for f, _ in _abi.ImuReport._fields_}


class ImuState:
    """FeatureAssociation's IMU queue (llsr_imu_state): feed every /imu_type message to callback(),
    take scan_window() once per scan, where adjustDistortion would run."""

    def __init__(self, scan_period: float = 0.1):
        self.scan_period = float(scan_period)
        self.state = _abi.ImuStateStruct()
        rc = lib().llsr_imu_init(C.byref(self.state))
        if rc != 0:
            raise LlsrError(f"llsr_imu_init: {rc}")

    def callback(self, sec: int, nanosec: int, orientation, angular_velocity, linear_acceleration):
        """imuHandler + AccumulateIMUShiftAndRotation (FA:315-351, 452-489) of one message."""
        m = _abi.ImuMsg(int(sec), int(nanosec), (C.c_double * 4)(*map(float, orientation)),
                        (C.c_double * 3)(*map(float, angular_velocity)),
                        (C.c_double * 3)(*map(float, linear_acceleration)))
        rc = lib().llsr_imu_callback(C.byref(self.state), C.byref(m), self.scan_period)
        if rc != 0:
            raise LlsrError(f"llsr_imu_callback: {rc}")

    def scan_window(self) -> np.ndarray:
        """llsr_imu_scan_window: the n + 1 ring entries this scan's de-skew can read (empty: no IMU
        yet), as IMU_SAMPLE_DTYPE records; then imuPointerLastIteration = imuPointerLast (FA:788)."""
        out = np.zeros(_abi.IMU_WINDOW_MAX, IMU_SAMPLE_DTYPE)
        n = C.c_int32(0)
        rc = lib().llsr_imu_scan_window(C.byref(self.state), out.ctypes.data, C.byref(n))
        if rc != 0:
            raise LlsrError(f"llsr_imu_scan_window: {rc}")
        return out[: n.value + 1].copy() if n.value > 0 else out[:0].copy()

    def arrays(self) -> dict:
        """Every ring array and both pointers (for comparisons)."""
        st = self.state
        d = {"pointer_last": int(st.pointer_last), "pointer_last_iteration": int(st.pointer_last_iteration)}
        for f, _ in st._fields_[2:]:
            d[f] = np.ctypeslib.as_array(getattr(st, f)).copy()
        return d


def imu_deskew_host(cfg, scan_stamp, window, seg_xyzi, orientation, carry: "_abi.ImuCarry"):
    """llsr_imu_deskew_host: adjustDistortion (FA:565-690) of one scan on the host. Returns (loam_xyzi
    float32 [S, 4], report dict); `carry` is updated in place."""
    w = np.zeros(0, IMU_SAMPLE_DTYPE) if window is None else np.ascontiguousarray(window, IMU_SAMPLE_DTYPE)
    n = max(len(w) - 1, 0)
    seg = np.ascontiguousarray(seg_xyzi, np.float32).reshape(-1, 4)
    ori = np.ascontiguousarray(orientation, np.float32).reshape(3)
    out = np.zeros_like(seg)
    rep = _abi.ImuReport()
    rc = lib().llsr_imu_deskew_host(C.byref(cfg), int(scan_stamp[0]), int(scan_stamp[1]), w.ctypes.data, n,
                                    seg.ctypes.data, seg.shape[0], ori.ctypes.data, C.byref(carry), out.ctypes.data,
                                    C.byref(rep))
    if rc != 0:
        raise LlsrError(f"llsr_imu_deskew_host: {rc}")
    return out, imu_report_dict(rep)


def odom_init() -> "_abi.OdomState":
    """llsr_odom_init: FeatureAssociation's /odom2 members before any message (the zero sample)."""
    st = _abi.OdomState()
    rc = lib().llsr_odom_init(C.byref(st))
    if rc != 0:
        raise LlsrError(f"llsr_odom_init: {rc}")
    return st


def odom_callback(state: "_abi.OdomState", msg) -> np.ndarray:
    """odomCallback (FA:354-383) of a 13-double odometry message (orientation xyzw, position, twist;
    7 doubles are enough); updates `state` and returns its latest sample roll, pitch, yaw, x, y, z."""
    a = np.zeros(13, np.float64)
    m = np.asarray(msg, np.float64).reshape(-1)
    a[:len(m)] = m
    rc = lib().llsr_odom_callback(C.byref(state), C.byref(_array_to_msg(a)))
    if rc != 0:
        raise LlsrError(f"llsr_odom_callback: {rc}")
    return state.last.as_array()


def update_initial_guess(sample, transform_sum) -> np.ndarray:
    """updateInitialGuess (FA:2370-2402): the transformCur it builds from the /odom2 sample (roll,
    pitch, yaw, x, y, z or _abi.OdomSample) and transformSum."""
    smp = sample if isinstance(sample, _abi.OdomSample) else _abi.OdomSample(*(float(x) for x in sample))
    ts = np.ascontiguousarray(transform_sum, np.float32).reshape(6)
    out = np.zeros(6, np.float32)
    rc = lib().llsr_update_initial_guess(C.byref(smp), ts.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise LlsrError(f"llsr_update_initial_guess: {rc}")
    return out


def shadow_points() -> np.ndarray:
    """GenerateShadowPoint (FA:412-439): the 160 virtual points appended to the flat / surf-last clouds."""
    out = np.zeros((160, 4), np.float32)
    rc = lib().llsr_shadow_points(out.ctypes.data)
    if rc != 0:
        raise LlsrError(f"llsr_shadow_points: {rc}")
    return out


def _imu_report(imu) -> "_abi.ImuReport":
    """An _abi.ImuReport from one, or from a {field: [3]} mapping as fetch_imu_report returns it
    (missing fields are zero; the use_imu_undistortion branches read `start` and `cur`)."""
    if isinstance(imu, _abi.ImuReport):
        return imu
    r = _abi.ImuReport()
    for f, _ in _abi.ImuReport._fields_:
        if f in imu:
            v = np.asarray(imu[f], np.float32).reshape(3)
            setattr(r, f, (C.c_float * 3)(*(float(x) for x in v)))
    return r


def integrate_transformation(transform_sum, transform_cur, imu=None) -> np.ndarray:
    """integrateTransformation (FA:2537-2568) on the host side of the library: the new transformSum.
    imu: the scan's IMU report (use_imu_undistortion == true: PluginIMURotation at the end)."""
    ts = np.array(transform_sum, np.float32).reshape(6).copy()
    tc = np.ascontiguousarray(transform_cur, np.float32).reshape(6)
    if imu is None:
        rc = lib().llsr_integrate_transformation(ts.ctypes.data, tc.ctypes.data)
    else:
        rc = lib().llsr_integrate_transformation_imu(ts.ctypes.data, tc.ctypes.data, C.byref(_imu_report(imu)))
    if rc != 0:
        raise LlsrError(f"llsr_integrate_transformation: {rc}")
    return ts


def first_scan_imu(transform_sum, imu) -> np.ndarray:
    """checkSystemInitialization's use_imu_undistortion add (FA:2329-2332): the new transformSum."""
    ts = np.array(transform_sum, np.float32).reshape(6).copy()
    rc = lib().llsr_first_scan_imu(ts.ctypes.data, C.byref(_imu_report(imu)))
    if rc != 0:
        raise LlsrError(f"llsr_first_scan_imu: {rc}")
    return ts


def transform_to_end(transform_cur, xyzi, imu=None, out=None) -> np.ndarray:
    """TransformToEnd (FA:1414-1490) of float4 rows on the host side of the library. imu: the scan's
    IMU report (use_imu_undistortion == true: the tail at FA:1456-1483); out: the array to write
    (may be xyzi itself when that is a contiguous float32 array)."""
    tc = np.ascontiguousarray(transform_cur, np.float32).reshape(6)
    a = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    if out is None:
        out = np.empty_like(a)
    elif out.dtype != np.float32 or not out.flags.c_contiguous or out.size != a.size:
        raise ValueError("out: a contiguous float32 array of the input's size")
    if imu is None:
        rc = lib().llsr_transform_to_end(tc.ctypes.data, a.ctypes.data, len(a), out.ctypes.data)
    else:
        rc = lib().llsr_transform_to_end_imu(tc.ctypes.data, C.byref(_imu_report(imu)), a.ctypes.data, len(a),
                                             out.ctypes.data)
    if rc != 0:
        raise LlsrError(f"llsr_transform_to_end: {rc}")
    return out


class FeatureAssociation:
    """Drop-in for FeatureAssociation::updateTransformation's arithmetic (FA:2505-2535)."""

    def __init__(self, pipeline: Pipeline):
        self.p = pipeline
        self.transform_cur = np.zeros(6, np.float32)
        self.is_degenerate = 0

    def update_transformation(self, corner_points_sharp, surf_points_flat, laser_cloud_corner_last,
                              laser_cloud_surf_last) -> dict:
        r = self.p.scan2scan(corner_points_sharp, surf_points_flat, laser_cloud_corner_last,
                             laser_cloud_surf_last, self.transform_cur, self.is_degenerate)
        self.transform_cur = r["transform_cur"]
        self.is_degenerate = r["is_degenerate"]
        return r


class MapOptimization:
    """Drop-in for MapOptimization::scan2MapOptimization's arithmetic (MO:1572-1610)."""

    def __init__(self, pipeline: Pipeline):
        self.p = pipeline

    def scan2map_optimization(self, laser_cloud_corner_scan_ds, laser_cloud_surf_total_last_ds,
                              laser_cloud_corner_from_map_ds, laser_cloud_surf_from_map_ds,
                              transform_tobe_mapped) -> dict:
        return self.p.scan2map(laser_cloud_corner_scan_ds, laser_cloud_surf_total_last_ds,
                               laser_cloud_corner_from_map_ds, laser_cloud_surf_from_map_ds,
                               transform_tobe_mapped)


class ImageProjection:
    """Drop-in for ImageProjection::cloudHandler's arithmetic (IP:189-222)."""

    def __init__(self, pipeline: Pipeline):
        self.p = pipeline

    def cloud_handler(self, xyzi: np.ndarray) -> dict:
        r = self.p.process_scan(xyzi)
        return {
            "segmented_cloud": r["seg_xyzi"], "outlier_cloud": r["outlier_xyzi"],
            "seg_msg": {
                "start_ring_index": r["start_ring_index"], "end_ring_index": r["end_ring_index"],
                "start_orientation": float(r["orientation"][0]), "end_orientation": float(r["orientation"][1]),
                "orientation_diff": float(r["orientation"][2]),
                "segmented_cloud_ground_flag": r["seg_ground_flag"].astype(bool),
                "segmented_cloud_col_ind": r["seg_col_ind"], "segmented_cloud_range": r["seg_range"],
            },
            "outlierCloud_Intensity": r["outlier_intensity"].astype(np.float64),
            "segmentedCloud_Intensity": r["seg_intensity"].astype(np.float64),
            "_full": r,
        }


def map_config(lidar: str | None = None, **kw) -> _abi.MapConfig:
    """llsr_map_config_default (lidar None) or the loam_config.yaml block of `lidar`
    (llsr_map_config_lidar: "vlp32c" and "hdl64e" enable the loop-closure local map), then the overrides."""
    c = _abi.MapConfig()
    if lidar is None:
        lib().llsr_map_config_default(C.byref(c))
    else:
        code = {"vlp16": _abi.LLSR_LIDAR_VLP16, "vlp32c": _abi.LLSR_LIDAR_VLP32C,
                "hdl64e": _abi.LLSR_LIDAR_HDL64E}[lidar]
        if lib().llsr_map_config_lidar(C.byref(c), code) != 0:
            raise LlsrError("llsr_map_config_lidar failed")
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def global_map_config(**kw) -> _abi.GlobalMapConfig:
    """llsr_global_map_config_default (radius 5000, leaves 1.0 / 0.4, the reference's first-call
    behaviour), then the overrides."""
    c = _abi.GlobalMapConfig()
    if lib().llsr_global_map_config_default(C.byref(c)) != 0:
        raise LlsrError("llsr_global_map_config_default failed")
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def keypose_radius_sorted(poses4, pos, radius: float) -> np.ndarray:
    """publishGlobalMap's sorted radius search (llsr_keypose_radius_sorted, host only): indices of
    the key poses with d^2 < float(radius^2) by ascending d^2, equal d^2 by ascending index."""
    p = np.ascontiguousarray(poses4, np.float32).reshape(-1, 4)
    q = np.ascontiguousarray(pos, np.float32)
    out = np.zeros(max(len(p), 1), np.int32)
    n = lib().llsr_keypose_radius_sorted(p.ctypes.data, len(p), q.ctypes.data, radius, out.ctypes.data)
    if n < 0:
        raise LlsrError(f"llsr_keypose_radius_sorted: {n}")
    return out[:n].copy()


def loop_config(lidar: str = "hdl64e", **kw) -> _abi.LoopConfig:
    """llsr_loop_config_lidar: the loop-closure parameters of the loam_config.yaml block of `lidar`
    (history_keyframe_search_radius / _search_num / _fitness_score) with the constants of
    performLoopClosure (MO:97, 912, 1001-1008), then the overrides."""
    c = _abi.LoopConfig()
    code = {"vlp16": _abi.LLSR_LIDAR_VLP16, "vlp32c": _abi.LLSR_LIDAR_VLP32C, "hdl64e": _abi.LLSR_LIDAR_HDL64E}[lidar]
    if lib().llsr_loop_config_lidar(C.byref(c), code) != 0:
        raise LlsrError("llsr_loop_config_lidar failed")
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def loop_candidate(poses4, times, pos, now: float, radius: float, gap: float = 30.0) -> int:
    """detectLoopClosure's candidate (llsr_loop_candidate, host only): the first key pose of the
    sorted radius search with fabs(time - now) > gap, or -1."""
    p = np.ascontiguousarray(poses4, np.float32).reshape(-1, 4)
    t = np.ascontiguousarray(times, np.float64).reshape(-1)
    if len(t) != len(p):
        raise ValueError("one time per pose")
    q = np.ascontiguousarray(pos, np.float32)
    r = lib().llsr_loop_candidate(p.ctypes.data, t.ctypes.data, len(p), q.ctypes.data, now, radius, gap)
    if r < -1:
        raise LlsrError(f"llsr_loop_candidate: {r}")
    return r


def umeyama3(src_xyz, dst_xyz) -> np.ndarray:
    """One ICP iteration's rigid estimate (llsr_umeyama3, host only): the 4x4 float32 T with
    dst ~ T src, Eigen::umeyama without scaling in the order DESIGN.md §16 fixes."""
    a = np.ascontiguousarray(src_xyz, np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(dst_xyz, np.float32).reshape(-1, 3)
    if len(a) != len(b):
        raise ValueError("one destination per source point")
    T = np.zeros(16, np.float32)
    rc = lib().llsr_umeyama3(a.ctypes.data, b.ctypes.data, len(a), T.ctypes.data)
    if rc != 0:
        raise LlsrError(f"llsr_umeyama3: {rc}")
    return T.reshape(4, 4)


def loop_constraint(T, pose_latest, pose_closest, fitness: float):
    """performLoopClosure's pose constraint (llsr_loop_constraint, host only; MO:1056-1081):
    (pose_from, pose_to, noise_variance) for BetweenFactor(latest, closest, from.between(to))."""
    t = np.ascontiguousarray(T, np.float32).reshape(16)
    a = np.ascontiguousarray(pose_latest, np.float32).reshape(6)
    b = np.ascontiguousarray(pose_closest, np.float32).reshape(6)
    pf, pt, var = np.zeros(6, np.float32), np.zeros(6, np.float32), C.c_float()
    rc = lib().llsr_loop_constraint(t.ctypes.data, a.ctypes.data, b.ctypes.data, fitness, pf.ctypes.data,
                                    pt.ctypes.data, C.byref(var))
    if rc != 0:
        raise LlsrError(f"llsr_loop_constraint: {rc}")
    return pf, pt, var.value


def icp_align_host(src, tgt, cfg: _abi.LoopConfig | None = None) -> dict:
    """The loop closure's ICP (llsr_icp_align_host, host only, serial) of the (n, 4)
    clouds src onto tgt: the llsr_icp_result fields and "aligned", the source moved by T."""
    a = np.ascontiguousarray(src, np.float32).reshape(-1, 4)
    b = np.ascontiguousarray(tgt, np.float32).reshape(-1, 4)
    cfg = cfg or loop_config()
    res = _abi.IcpResult()
    out = np.zeros((max(len(a), 1), 4), np.float32)
    rc = lib().llsr_icp_align_host(a.ctypes.data, len(a), b.ctypes.data, len(b), C.byref(cfg), C.byref(res),
                                   out.ctypes.data)
    if rc != 0:
        raise LlsrError(f"llsr_icp_align_host: {rc}")
    r = res.as_dict()
    r["aligned"] = out[:len(a)]
    return r


def pg_config(**kw) -> _abi.PgConfig:
    """llsr_pg_config_default (GTSAM's NonlinearOptimizerParams defaults), fields overridden by keyword."""
    c = _abi.PgConfig()
    lib().llsr_pg_config_default(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


class PoseGraph:
    """P pose graphs optimised together (llsr_pg, include/llsr.h). device None runs the
    same loop bodies on the host (LLSR_PG_HOST). Poses are (x, y, z, roll, pitch, yaw) float32 rows."""

    def __init__(self, P: int, max_poses: int, max_loops: int, max_envelope_blocks: int | None = None,
                 device: int | None = 0):
        if max_envelope_blocks is None:
            max_envelope_blocks = (2 + max_loops) * max_poses
        self.P = P
        self._w = lib().llsr_pg_create(_abi.LLSR_PG_HOST if device is None else device, P, max_poses, max_loops,
                                       max_envelope_blocks)
        if not self._w:
            raise LlsrError("llsr_pg_create failed: bad capacities, no HIP device or no memory")

    def close(self):
        if getattr(self, "_w", None):
            lib().llsr_pg_destroy(self._w)
            self._w = None

    def __del__(self):
        self.close()

    def _check(self, rc: int, what: str):
        if rc < 0:
            e = LlsrError(f"{what} failed ({rc}): {lib().llsr_pg_last_error(self._w).decode()}")
            e.code = rc
            raise e

    def reset(self, p: int = -1):
        self._check(lib().llsr_pg_reset(self._w, p), "llsr_pg_reset")

    def append(self, p: int, poses6):
        a = np.ascontiguousarray(poses6, np.float32).reshape(-1, 6)
        self._check(lib().llsr_pg_append(self._w, p, a.ctypes.data, len(a)), "llsr_pg_append")

    def add_loop(self, p: int, from_id: int, to_id: int, pose_from6, pose_to6, variance: float):
        """pose_from6 / pose_to6 / variance as llsr_loop_constraint gives them (GTSAM's axis order)."""
        a, b = (np.ascontiguousarray(x, np.float32).reshape(6) for x in (pose_from6, pose_to6))
        self._check(lib().llsr_pg_add_loop(self._w, p, from_id, to_id, a.ctypes.data, b.ctypes.data,
                                           C.c_float(variance)), "llsr_pg_add_loop")

    def optimize(self, cfg: _abi.PgConfig | None = None, stream: int = 0) -> list:
        reps = (_abi.PgReport * self.P)()
        self._check(lib().llsr_pg_optimize(self._w, C.byref(cfg) if cfg is not None else None, reps,
                                           C.c_void_p(stream)), "llsr_pg_optimize")
        return [r.as_dict() for r in reps]

    def poses(self, p: int) -> np.ndarray:
        n = lib().llsr_pg_poses(self._w, p, None, 0)
        self._check(n, "llsr_pg_poses")
        out = np.zeros((max(n, 1), 6), np.float32)
        lib().llsr_pg_poses(self._w, p, out.ctypes.data, n)
        return out[:n].copy()


class PriorMap:
    """A saved map to localise in (llsr_prior, include/llsr.h): a static corner and a
    static surf cloud in tile order, cropped around P positions per call. device None builds the host
    twin (LLSR_PRIOR_HOST), whose crops are numpy arrays; on a device they are torch CUDA tensors."""

    KINDS = ("corner", "surf")

    def __init__(self, radius: float | None = None, tile: float | None = None, device: int | None = 0):
        c = _abi.PriorConfig()
        lib().llsr_prior_config_default(C.byref(c))
        if radius is not None:
            c.radius = radius
        if tile is not None:
            c.tile = tile
        self.device = device
        self._w = lib().llsr_prior_create(C.byref(c), _abi.LLSR_PRIOR_HOST if device is None else device)
        if not self._w:
            e = LlsrError("llsr_prior_create failed: a radius or tile that is not finite and positive, "
                          "no HIP device or no memory")
            e.code = _abi.LLSR_EINVAL
            raise e

    @classmethod
    def from_saved(cls, corner, surf, corner_leaf: float | None = 0.2, radius: float | None = None,
                   tile: float | None = None, device: int | None = 0) -> "PriorMap":
        """From saveMapService's clouds (Pipeline.mapping_save_map, LocalMap.save_map): surfaceMap is
        already a VoxelGrid of the surf leaf; cornerMap is raw, so it goes through the VoxelGrid at
        corner_leaf first (on device 0 for a host object; None or 0 loads it as it is)."""
        def host(a):
            return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, np.float32).reshape(-1, 4)
        if corner_leaf and len(corner):
            vg = LocalMap(0 if device is None else device)
            corner = vg.voxel_grid([corner], [corner_leaf])[0]
            vg.close()
        m = cls(radius, tile, device)
        m.load(host(corner), host(surf))
        return m

    def close(self):
        if getattr(self, "_w", None):
            lib().llsr_prior_destroy(self._w)
            self._w = None

    def __del__(self):
        self.close()

    def _check(self, rc: int, what: str):
        if rc < 0:
            e = LlsrError(f"{what} failed ({rc}): {lib().llsr_prior_last_error(self._w).decode()}")
            e.code = rc
            raise e
        return rc

    def load(self, corner, surf, stream: int = 0):
        c, s = (np.ascontiguousarray(a, np.float32).reshape(-1, 4) for a in (corner, surf))
        self._check(lib().llsr_prior_load(self._w, c.ctypes.data, len(c), s.ctypes.data, len(s), C.c_void_p(stream)),
                    "llsr_prior_load")

    def info(self) -> dict:
        r = _abi.PriorReport()
        self._check(lib().llsr_prior_info(self._w, C.byref(r)), "llsr_prior_info")
        d = {"radius": float(r.radius), "tile": float(r.tile), "device": int(r.device)}
        for k, name in enumerate(self.KINDS):
            d[name] = {"n_points": int(r.n_points[k]), "n_tiles": int(r.n_tiles[k]),
                       "n_tiles_used": int(r.n_tiles_used[k]), "dims": tuple(r.dims[k][:]),
                       "origin": tuple(r.origin[k][:])}
        return d

    def points(self, kind: int | str) -> np.ndarray:
        """The kind's cloud in stored order."""
        k = self.KINDS.index(kind) if isinstance(kind, str) else kind
        n = self._check(lib().llsr_prior_points(self._w, k, None, 0), "llsr_prior_points")
        out = np.zeros((max(n, 1), 4), np.float32)
        lib().llsr_prior_points(self._w, k, out.ctypes.data, n)
        return out[:n].copy()

    def tile_starts(self, kind: int | str) -> np.ndarray:
        """The kind's CSR over the tile keys, [ntiles + 1]."""
        k = self.KINDS.index(kind) if isinstance(kind, str) else kind
        n = self._check(lib().llsr_prior_tile_starts(self._w, k, None, 0), "llsr_prior_tile_starts")
        out = np.zeros(max(n, 1), np.uint32)
        lib().llsr_prior_tile_starts(self._w, k, out.ctypes.data, n)
        return out[:n].copy()

    def crop(self, positions, cap: int | None = None, count_only: bool = False, stream: int = 0) -> dict:
        """llsr_prior_crop_batch around positions (P, 3): {"out", "corner_off", "surf_off"}; position p's
        corner crop is out[corner_off[p]:corner_off[p + 1]], its surf crop out[surf_off[p]:surf_off[p + 1]].
        cap None sizes the buffer with a counting call first; a given cap that is too small raises
        LlsrError with code LLSR_ERANGE and the offsets in its `offsets` attribute."""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        P = len(pos)
        oc, os_ = np.zeros(P + 1, np.int64), np.zeros(P + 1, np.int64)

        def call(ptr, n):
            return lib().llsr_prior_crop_batch(self._w, pos.ctypes.data, P, C.c_void_p(ptr), n, oc.ctypes.data,
                                               os_.ctypes.data, C.c_void_p(stream))
        if cap is None or count_only:
            self._check(call(None, 0), "llsr_prior_crop_batch")
            if count_only:
                return {"out": None, "corner_off": oc, "surf_off": os_}
            cap = int(os_[P])
        if self.device is None:
            out = np.zeros((max(cap, 1), 4), np.float32)
            ptr = out.ctypes.data
        else:
            import torch
            out = torch.zeros((max(cap, 1), 4), dtype=torch.float32, device=torch.device("cuda", self.device))
            torch.cuda.synchronize(self.device)
            ptr = out.data_ptr()
        rc = call(ptr, cap)
        if rc == _abi.LLSR_ERANGE:
            e = LlsrError(f"llsr_prior_crop_batch failed ({rc}): {lib().llsr_prior_last_error(self._w).decode()}")
            e.code, e.offsets, e.out = rc, (oc, os_), out
            raise e
        self._check(rc, "llsr_prior_crop_batch")
        return {"out": out[:int(os_[P])], "corner_off": oc, "surf_off": os_}

    def last_crop(self) -> dict:
        """Diagnostic (llsr_prior_last_crop): ms, points tested, points written of the last crop."""
        ms, t, w = C.c_float(), C.c_int64(), C.c_int64()
        self._check(lib().llsr_prior_last_crop(self._w, C.byref(ms), C.byref(t), C.byref(w)), "llsr_prior_last_crop")
        return {"ms": ms.value, "tested": t.value, "written": w.value}


class Icp:
    """The loop closure's ICP on a HIP device (llsr_icp, include/llsr.h): a workspace that owns the
    target's cell grid and the loop's buffers. Clouds are torch CUDA float32 tensors of shape (n, 4)."""

    def __init__(self, device: int = 0):
        import torch
        self._torch = torch
        self.device = torch.device("cuda", device)
        self._w = lib().llsr_icp_create(device)
        if not self._w:
            raise LlsrError("llsr_icp_create failed: no HIP device")
        self._s = torch.cuda.Stream(device=self.device)

    def close(self):
        if getattr(self, "_w", None):
            lib().llsr_icp_destroy(self._w)
            self._w = None

    def __del__(self):
        self.close()

    def align(self, src, tgt, cfg: _abi.LoopConfig | None = None) -> dict:
        """llsr_icp_align of src onto tgt: the llsr_icp_result fields and "aligned" (a device tensor)."""
        torch = self._torch
        src, tgt = (np.array(c, np.float32) if isinstance(c, np.ndarray) else c for c in (src, tgt))
        a = torch.as_tensor(src, dtype=torch.float32, device=self.device).reshape(-1, 4).contiguous()
        b = torch.as_tensor(tgt, dtype=torch.float32, device=self.device).reshape(-1, 4).contiguous()
        out = torch.empty((max(a.shape[0], 1), 4), dtype=torch.float32, device=self.device)
        cfg = cfg or loop_config()
        res = _abi.IcpResult()
        self._s.wait_stream(torch.cuda.current_stream(self.device))
        rc = lib().llsr_icp_align(self._w, C.c_void_p(a.data_ptr() if a.shape[0] else 0), a.shape[0],
                                  C.c_void_p(b.data_ptr() if b.shape[0] else 0), b.shape[0], C.byref(cfg),
                                  C.byref(res), C.c_void_p(out.data_ptr()), C.c_void_p(self._s.cuda_stream))
        if rc != 0:
            raise LlsrError(f"llsr_icp_align failed ({rc}): {lib().llsr_icp_last_error(self._w).decode()}")
        torch.cuda.current_stream(self.device).wait_stream(self._s)
        r = res.as_dict()
        r["aligned"] = out[:a.shape[0]]
        return r

    def align_batch(self, srcs, tgts, cfgs=None) -> list:
        """llsr_icp_align_batch: srcs[p] onto tgts[p] for every p in one set of launches. cfgs is None
        (the default block), one LoopConfig for all problems, or a list with one per problem. Returns
        one dict per problem: the llsr_icp_result fields and "aligned" (a view of one device tensor)."""
        torch = self._torch
        P = len(srcs)
        if P < 1 or len(tgts) != P:
            raise ValueError("one target per source, at least one problem")

        def cat(clouds):
            host = [np.asarray(c.cpu() if hasattr(c, "cpu") else c, np.float32).reshape(-1, 4) for c in clouds]
            off = np.zeros(P + 1, np.int64)
            off[1:] = np.cumsum([len(c) for c in host])
            dev = torch.from_numpy(np.concatenate(host + [np.zeros((1, 4), np.float32)])).to(self.device)
            return dev, off

        (a, so), (b, to) = cat(srcs), cat(tgts)
        out = torch.empty_like(a)
        if cfgs is None or isinstance(cfgs, _abi.LoopConfig):
            arr = (_abi.LoopConfig * 1)(cfgs if cfgs is not None else loop_config())
        else:
            if len(cfgs) != P:
                raise ValueError("one configuration, or one per problem")
            arr = (_abi.LoopConfig * P)(*cfgs)
        res = (_abi.IcpResult * P)()
        self._s.wait_stream(torch.cuda.current_stream(self.device))
        rc = lib().llsr_icp_align_batch(self._w, P, C.c_void_p(a.data_ptr()), so.ctypes.data, C.c_void_p(b.data_ptr()),
                                        to.ctypes.data, arr, len(arr), res, C.c_void_p(out.data_ptr()),
                                        C.c_void_p(self._s.cuda_stream))
        if rc != 0:
            raise LlsrError(f"llsr_icp_align_batch failed ({rc}): {lib().llsr_icp_last_error(self._w).decode()}")
        torch.cuda.current_stream(self.device).wait_stream(self._s)
        rs = []
        for p in range(P):
            r = res[p].as_dict()
            r["aligned"] = out[so[p]:so[p + 1]]
            rs.append(r)
        return rs

    def last_passes(self) -> int:
        """Passes of the loop in the last align_batch (llsr_icp_last_passes)."""
        return lib().llsr_icp_last_passes(self._w)

    def last_times(self) -> dict:
        """HIP-event ms of the last align or align_batch: the correspondence and solve kernels summed, the
        whole call."""
        c, v, t = C.c_float(), C.c_float(), C.c_float()
        lib().llsr_icp_last_times(self._w, C.byref(c), C.byref(v), C.byref(t))
        return {"corr_ms": c.value, "solve_ms": v.value, "total_ms": t.value}


def _global_map(torch, device, call, caps, edge: bool, planar: bool) -> dict:
    """Run a llsr_map_global-shaped call with output buffers of caps[global, edge, planar] points,
    growing them once to the reported sizes on LLSR_ERANGE."""
    rep = _abi.GlobalMapReport()
    want = (True, edge, planar)
    for _ in range(2):
        bufs = [torch.empty((max(c, 1), 4), dtype=torch.float32, device=device) if w else None
                for c, w in zip(caps, want)]
        args = []
        for b in bufs:
            args += [C.c_void_p(b.data_ptr()), b.shape[0]] if b is not None else [None, 0]
        rc = call(*args, C.byref(rep))
        if rc != _abi.LLSR_ERANGE:
            break
        for k, n in enumerate((rep.n_global, rep.n_edge, rep.n_planar)):
            caps[k] = max(caps[k], int(n))
    r = {"rc": rc, "report": rep.as_dict(), "global": None, "edge": None, "planar": None}
    if rc == 0:
        for key, b, n in zip(("global", "edge", "planar"), bufs, (rep.n_global, rep.n_edge, rep.n_planar)):
            r[key] = b[:n] if b is not None else None
    return r


def _save_map(torch, device, call):
    """Run a llsr_map_save-shaped call, growing the two buffers once to the reported sizes."""
    nc, ns = C.c_int64(0), C.c_int64(0)
    caps = [1, 1]
    for _ in range(2):
        c, s = (torch.empty((cap, 4), dtype=torch.float32, device=device) for cap in caps)
        rc = call(C.c_void_p(c.data_ptr()), caps[0], C.c_void_p(s.data_ptr()), caps[1], C.byref(nc), C.byref(ns))
        if rc != _abi.LLSR_ERANGE:
            break
        caps = [max(1, nc.value), max(1, ns.value)]
    return rc, c[:nc.value], s[:ns.value]


class LocalMap:
    """MapOptimization's keyframe store + local map on a HIP device (llsr_map, include/llsr.h):
    saveKeyFramesAndFactor's clouds (MO:1686-1752), extractSurroundingKeyFrames (MO:1096-1232),
    downsampleCurrentScan (MO:1234-1267) and the VoxelGrid filters they use.

    Clouds are torch CUDA float32 tensors of shape (n, 4) (x, y, z, intensity); torch is only the
    device allocator here. Calls run on a private stream ordered after the caller's current stream
    and return once their results are ready (as the reference's calls do)."""

    def __init__(self, device: int = 0, cfg: _abi.MapConfig | None = None):
        import torch
        self._torch = torch
        self.cfg = cfg or map_config()
        self.device = torch.device("cuda", device)
        self._m = lib().llsr_map_create(C.byref(self.cfg), device)
        if not self._m:
            raise LlsrError("llsr_map_create failed: no HIP device")
        self._s = torch.cuda.Stream(device=self.device)
        self._n_corner = 0
        self._n_surf = 0
        self._gm_caps = [1, 1, 1]  # global_map's output capacities (global, edge, planar), grown on demand

    def close(self):
        if getattr(self, "_m", None):
            lib().llsr_map_destroy(self._m)
            self._m = None

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc < 0:
            raise LlsrError(f"{what} failed ({rc}): {lib().llsr_map_last_error(self._m).decode()}")
        return rc

    def _enter(self):
        self._s.wait_stream(self._torch.cuda.current_stream(self.device))
        return C.c_void_p(self._s.cuda_stream)

    def _leave(self):
        self._torch.cuda.current_stream(self.device).wait_stream(self._s)

    def _cloud(self, a):
        t = self._torch.as_tensor(a, dtype=self._torch.float32, device=self.device).reshape(-1, 4).contiguous()
        return t

    def reset(self):
        self._check(lib().llsr_map_reset(self._m), "llsr_map_reset")
        self._n_corner = self._n_surf = 0

    def voxel_grid(self, clouds, leaves):
        """pcl::VoxelGrid::filter of every cloud (list) with its leaf size; returns the filtered clouds."""
        torch = self._torch
        cl = [self._cloud(c) for c in clouds]
        off = np.zeros(len(cl) + 1, np.int64)
        off[1:] = np.cumsum([c.shape[0] for c in cl])
        packed = torch.cat(cl) if off[-1] else torch.zeros((0, 4), dtype=torch.float32, device=self.device)
        out = torch.empty((max(int(off[-1]), 1), 4), dtype=torch.float32, device=self.device)
        out_off = np.zeros(len(cl) + 1, np.int64)
        leaf = np.asarray(leaves, np.float32)
        s = self._enter()
        self._check(lib().llsr_map_voxel_grid(self._m, C.c_void_p(packed.data_ptr()), off.ctypes.data, len(cl),
                                              leaf.ctypes.data, C.c_void_p(out.data_ptr()), out_off.ctypes.data, s),
                    "llsr_map_voxel_grid")
        self._leave()
        return [out[out_off[k]:out_off[k + 1]] for k in range(len(cl))]

    def downsample_scan(self, corner_last, surf_last, outlier_last, corner_scan, surf_scan) -> dict:
        """downsampleCurrentScan (MO:1234-1267): the six ...DS clouds."""
        torch = self._torch
        cl = [self._cloud(c) for c in (corner_last, surf_last, outlier_last, corner_scan, surf_scan)]
        n = [c.shape[0] for c in cl]
        out = torch.empty((max(sum(n) + n[1] + n[2], 1), 4), dtype=torch.float32, device=self.device)
        out_off = np.zeros(7, np.int64)
        args = []
        for c, k in zip(cl, n):
            args += [C.c_void_p(c.data_ptr() if k else 0), k]
        s = self._enter()
        self._check(lib().llsr_map_downsample_scan(self._m, *args, C.c_void_p(out.data_ptr()), out_off.ctypes.data,
                                                   s), "llsr_map_downsample_scan")
        self._leave()
        names = ("corner_last_ds", "surf_last_ds", "outlier_last_ds", "corner_scan_ds", "surf_scan_ds",
                 "surf_total_last_ds")
        return {nm: out[out_off[k]:out_off[k + 1]] for k, nm in enumerate(names)}

    def add_keyframe(self, pose6, corner, surf, outlier) -> int:
        """Store a keyframe: PointTypePose x, y, z, roll, pitch, yaw + its three clouds."""
        pose = np.ascontiguousarray(pose6, np.float32)
        cl = [self._cloud(c) for c in (corner, surf, outlier)]
        args = []
        for c in cl:
            args += [C.c_void_p(c.data_ptr() if c.shape[0] else 0), c.shape[0]]
        s = self._enter()
        k = self._check(lib().llsr_map_add_keyframe(self._m, pose.ctypes.data, *args, s), "llsr_map_add_keyframe")
        self._s.synchronize()  # the copies read the caller's tensors
        self._n_corner += cl[0].shape[0]
        self._n_surf += cl[1].shape[0] + cl[2].shape[0]
        return k

    @property
    def num_keyframes(self) -> int:
        return lib().llsr_map_num_keyframes(self._m)

    def extract(self, robot_pos):
        """extractSurroundingKeyFrames: (laserCloudCornerFromMapDS, laserCloudSurfFromMapDS, report)."""
        torch = self._torch
        pos = np.ascontiguousarray(robot_pos, np.float32)
        cc, cs = max(self._n_corner, 1), max(self._n_surf, 1)
        oc = torch.empty((cc, 4), dtype=torch.float32, device=self.device)
        os_ = torch.empty((cs, 4), dtype=torch.float32, device=self.device)
        rep = _abi.MapReport()
        s = self._enter()
        self._check(lib().llsr_map_extract(self._m, pos.ctypes.data, C.c_void_p(oc.data_ptr()), cc,
                                           C.c_void_p(os_.data_ptr()), cs, C.byref(rep), s), "llsr_map_extract")
        self._leave()
        return oc[:rep.n_corner_ds], os_[:rep.n_surf_ds], rep.as_dict()

    def global_map(self, robot_pos, cfg: _abi.GlobalMapConfig | None = None, edge: bool = True,
                   planar: bool = True) -> dict:
        """publishGlobalMap (MO:775-892, llsr_map_global): {"global", "edge", "planar"} clouds (edge /
        planar None when not requested) and "report"."""
        pos = np.ascontiguousarray(robot_pos, np.float32)
        s = self._enter()
        call = lambda *out: lib().llsr_map_global(self._m, C.byref(cfg) if cfg is not None else None,  # noqa: E731
                                                  pos.ctypes.data, *out, s)
        r = _global_map(self._torch, self.device, call, self._gm_caps, edge, planar)
        self._check(r.pop("rc"), "llsr_map_global")
        self._leave()
        return r

    def save_map(self):
        """saveMapService's clouds (MO:382-395, llsr_map_save): (cornerMap, surfaceMap)."""
        s = self._enter()
        call = lambda *out: lib().llsr_map_save(self._m, *out, s)  # noqa: E731
        rc, c, su = _save_map(self._torch, self.device, call)
        self._check(rc, "llsr_map_save")
        self._leave()
        return c, su

    def _loop_call(self, call, names, sizes, caps):
        """Run a loop-closure call with one output buffer per name, growing them once to the reported
        sizes on LLSR_ERANGE; caps (points per output) may force the first attempt's capacities."""
        torch = self._torch
        rep = _abi.LoopReport()
        caps = list(caps) if caps is not None else [1] * len(names)
        for _ in range(2):
            bufs = [torch.empty((max(c, 1), 4), dtype=torch.float32, device=self.device) for c in caps]
            args = []
            for b in bufs:
                args += [C.c_void_p(b.data_ptr()), b.shape[0]]
            rc = call(rep, *args)
            if rc != _abi.LLSR_ERANGE:
                break
            caps = [max(c, int(getattr(rep, f))) for c, f in zip(caps, sizes)]
        r = rep.as_dict()
        r["rc"] = rc
        for nm, f, b in zip(names, sizes, bufs):
            r[nm] = b[:int(getattr(rep, f))] if rc == 0 and rep.found else None
        return r

    def loop_submaps(self, robot_pos, now: float, cfg: _abi.LoopConfig | None = None, caps=None) -> dict:
        """detectLoopClosure's candidate and submaps (MO:894-981, llsr_map_loop_submaps): the report
        fields and the "source", "target", "source_ds", "target_ds" clouds (None without a candidate)."""
        pos = np.ascontiguousarray(robot_pos, np.float32)
        cfg = cfg or loop_config()
        s = self._enter()
        call = lambda rep, *out: lib().llsr_map_loop_submaps(self._m, C.byref(cfg), pos.ctypes.data, now,  # noqa: E731
                                                            C.byref(rep), *out, s)
        r = self._loop_call(call, ("source", "target", "source_ds", "target_ds"),
                            ("n_source", "n_target", "n_source_ds", "n_target_ds"), caps)
        self._check(r.pop("rc"), "llsr_map_loop_submaps")
        self._leave()
        return r

    def loop_closure(self, robot_pos, now: float, cfg: _abi.LoopConfig | None = None, icp: "Icp | None" = None,
                     caps=None) -> dict:
        """performLoopClosure up to the pose constraint (MO:983-1081, llsr_map_loop_closure): the report
        fields (the alignment's among them) and the "aligned" and "target_ds" clouds."""
        pos = np.ascontiguousarray(robot_pos, np.float32)
        cfg = cfg or loop_config()
        s = self._enter()
        w = icp._w if icp is not None else None
        call = lambda rep, *out: lib().llsr_map_loop_closure(self._m, w, C.byref(cfg), pos.ctypes.data, now,  # noqa: E731
                                                            C.byref(rep), *out, s)
        r = self._loop_call(call, ("aligned", "target_ds"), ("n_source", "n_target_ds"), caps)
        self._check(r.pop("rc"), "llsr_map_loop_closure")
        self._leave()
        return r

    def set_keyframe_time(self, index: int, seconds: float):
        """cloudKeyPoses6D[index].time (llsr_map_set_keyframe_time); unset times never match a loop."""
        self._check(lib().llsr_map_set_keyframe_time(self._m, index, seconds), "llsr_map_set_keyframe_time")

    def set_key_poses(self, poses6):
        """correctPoses (MO:1757-1785, llsr_map_set_key_poses): overwrite the first len(poses6) key poses
        (x, y, z, roll, pitch, yaw) and drop the recent-keyframe queue."""
        p = np.ascontiguousarray(poses6, np.float32).reshape(-1, 6)
        self._check(lib().llsr_map_set_key_poses(self._m, p.ctypes.data, len(p)), "llsr_map_set_key_poses")

    def keyframe_times(self) -> np.ndarray:
        """cloudKeyPoses6D[*].time (llsr_map_keyframe_times): NaN where no time was set."""
        n = self._check(lib().llsr_map_keyframe_times(self._m, None, 0), "llsr_map_keyframe_times")
        out = np.zeros(max(n, 1), np.float64)
        lib().llsr_map_keyframe_times(self._m, out.ctypes.data, n)
        return out[:n]

    def keyframe_ids(self) -> np.ndarray:
        n = lib().llsr_map_keyframe_ids(self._m, None, 0)
        out = np.zeros(max(n, 1), np.int32)
        lib().llsr_map_keyframe_ids(self._m, out.ctypes.data, n)
        return out[:n]


# ---- input wire formats (llsr_input.hip) ----

def pc2_layout(fields, point_step: int) -> _abi.Pc2Layout:
    """fields: iterable of (name, offset, datatype, count) as in sensor_msgs/PointField."""
    lay = _abi.Pc2Layout()
    fields = list(fields)
    if len(fields) > _abi.PC2_MAX_FIELDS:
        raise ValueError("too many PointCloud2 fields")
    lay.point_step = point_step
    lay.num_fields = len(fields)
    for k, (name, off, dt, cnt) in enumerate(fields):
        lay.fields[k].name = name.encode()
        lay.fields[k].offset, lay.fields[k].datatype, lay.fields[k].count = off, dt, cnt
    return lay


def decode_pointcloud2(layout: _abi.Pc2Layout, messages, device: int = 0, stream: int = 0):
    """pcl::fromROSMsg<PointXYZI> of a batch of PointCloud2 messages. messages: list of
    (data bytes, width, height, row_step). The bytes are uploaded, decoded on the device, and the
    float4 points returned as a torch tensor (n, 4) with host and device point offsets [B+1]."""
    import torch
    dev = torch.device("cuda", device)
    B = len(messages)
    msgs = (_abi.Pc2Msg * B)()
    blobs, pos = [], 0
    for b, (data, width, height, row_step) in enumerate(messages):
        raw = np.frombuffer(bytes(data), np.uint8)
        pad = (-pos) % 16                     # keep every message 16-byte aligned in the pack
        if pad:
            blobs.append(np.zeros(pad, np.uint8))
            pos += pad
        msgs[b].data_offset, msgs[b].width, msgs[b].height, msgs[b].row_step = pos, width, height, row_step
        blobs.append(raw)
        pos += len(raw)
    data = torch.from_numpy(np.concatenate(blobs) if blobs else np.zeros(1, np.uint8)).to(dev)
    n = sum(w * h for _, w, h, _ in messages)
    out = torch.empty((max(n, 1), 4), dtype=torch.float32, device=dev)
    off = np.zeros(B + 1, np.int64)
    d_off = torch.empty(B + 1, dtype=torch.int64, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    rc = lib().llsr_decode_pointcloud2(C.byref(layout), C.c_void_p(data.data_ptr()), msgs, B,
                                       C.c_void_p(out.data_ptr()), off.ctypes.data, C.c_void_p(d_off.data_ptr()),
                                       C.c_void_p(stream))
    if rc != 0:
        raise LlsrError(f"llsr_decode_pointcloud2 failed ({rc})")
    return out[:n], off, d_off


def kitti_count(velodyne_dir: str) -> int:
    return lib().llsr_kitti_count(velodyne_dir.encode())


def kitti_read(path: str) -> np.ndarray:
    """One KITTI .bin frame as (n, 4) float32, read the way the reference's loader reads it."""
    out = np.zeros((_abi.KITTI_MAX_FLOATS // 4, 4), np.float32)
    n = C.c_int32()
    rc = lib().llsr_kitti_read(path.encode(), out.ctypes.data, len(out), C.byref(n))
    if rc != 0:
        raise LlsrError(f"llsr_kitti_read({path}) failed ({rc})")
    return out[:n.value].copy()


def kitti_load(velodyne_dir: str, first: int, B: int, cap_points: int, device: int = 0, stream: int = 0):
    """Frames first .. first+B-1 into HBM: (points tensor (n, 4), host offsets, device offsets)."""
    import torch
    dev = torch.device("cuda", device)
    out = torch.empty((max(cap_points, 1), 4), dtype=torch.float32, device=dev)
    off = np.zeros(B + 1, np.int64)
    d_off = torch.empty(B + 1, dtype=torch.int64, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    rc = lib().llsr_kitti_load(velodyne_dir.encode(), first, B, C.c_void_p(out.data_ptr()), cap_points,
                               off.ctypes.data, C.c_void_p(d_off.data_ptr()), C.c_void_p(stream))
    if rc != 0:
        raise LlsrError(f"llsr_kitti_load failed ({rc})")
    return out[:off[-1]], off, d_off
