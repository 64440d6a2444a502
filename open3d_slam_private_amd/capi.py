"""ctypes binding of include/o3dslam_reg.h (the drop-in C ABI).  No torch types; numpy or raw
device pointers only.  Mirrors the header 1:1 -- see the header for the reference file:line each
entry point replaces."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("O3D_REG_LIB") or os.path.join(_HERE, "lib", "libo3dslam_reg.so")   # O3D_REG_LIB: A/B builds (tools/)

STATUS_NAMES = {0: "OK", 1: "EMPTY_TARGET", 2: "EMPTY_SOURCE", 3: "NO_CORRESPONDENCES", 4: "BAD_TRANSFORM",
                5: "NOT_CONFIGURED", 6: "BAD_ARGUMENT", 7: "MISSING_FIELD", 8: "DEVICE_ERROR", 9: "UNSUPPORTED",
                10: "OUT_OF_BOUNDS"}
OUT_OF_BOUNDS = 10   # REG_OUT_OF_BOUNDS: BoundTransformationChecker's ConvergenceError
COST_P2PL, COST_GICP = 0, 1
# Open3D RegistrationICP with TransformationEstimationPointToPlane / PointToPoint (RegistrationIcpPointToPlane /
# RegistrationIcpPointToPoint, open3d_slam/src/CloudRegistration.cpp:54-101); see reg_cost in the header
COST_O3D_P2PL, COST_O3D_P2P = 2, 3
SMOOTH_LEN_MAX = 15   # reg_params.smooth_len: reg_create returns BAD_ARGUMENT above (the device checkers keep 16 poses)


class RegError(RuntimeError):
    def __init__(self, status, msg=""):
        self.status = status
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")


_DEBUG_FIELDS = ("profile_loop", "match_variant", "debug_flags", "disable_halo", "lanes_per_point", "disable_fused")


class RegParams(C.Structure):
    """include/o3dslam_reg.h reg_params.  The experiment switches of include/o3dslam_reg_debug.h (profile_loop,
    match_variant, debug_flags, disable_halo, lanes_per_point, disable_fused) are NOT part of the C struct any more; for
    the tests' and tools' convenience they can still be set as plain Python attributes on a RegParams object --
    Registration() passes them on through reg_debug_configure."""
    _fields_ = [("struct_size", C.c_int32), ("cost", C.c_int32), ("knn", C.c_int32), ("max_dist", C.c_float),
                ("epsilon", C.c_float), ("use_trimmed", C.c_int32), ("trim_ratio", C.c_float),
                ("use_surface_normal", C.c_int32), ("max_normal_angle", C.c_float),
                ("use_max_dist_filter", C.c_int32), ("outlier_max_dist", C.c_float), ("max_iter", C.c_int32),
                ("min_diff_rot", C.c_float), ("min_diff_trans", C.c_float), ("smooth_len", C.c_int32),
                ("fixed_iters", C.c_int32), ("gicp_rot_eps", C.c_float), ("gicp_trans_eps", C.c_float),
                ("cell_size", C.c_float), ("device", C.c_int32), ("sort_source", C.c_int32), ("use_xicp", C.c_int32),
                ("xicp_enough", C.c_float), ("xicp_insufficient", C.c_float), ("xicp_min_angle_deg", C.c_float),
                ("xicp_strong_angle_deg", C.c_float), ("gicp_stop_rule", C.c_int32), ("gicp_rel_fitness", C.c_float),
                ("gicp_rel_rmse", C.c_float), ("reserved", C.c_int32)]
    profile_loop = match_variant = debug_flags = disable_halo = lanes_per_point = disable_fused = 0


class RegDebugParams(C.Structure):
    _fields_ = [("struct_size", C.c_int32)] + [(k, C.c_int32) for k in _DEBUG_FIELDS] + [("reserved", C.c_int32)]


class RegResult(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("max_iter_reached", C.c_int32),
                ("rank_last", C.c_int32), ("n_inliers", C.c_int64), ("n_matched", C.c_int64), ("error", C.c_double),
                ("fitness", C.c_double), ("inlier_rmse", C.c_double), ("H_last", C.c_float * 36),
                ("b_last", C.c_float * 6), ("target_build_ms", C.c_float), ("loop_ms", C.c_float),
                ("T_iter_last", C.c_float * 16), ("n_band_stalls", C.c_int32), ("n_constraints", C.c_int32),
                ("prof_ms", C.c_float * 4), ("prof_launches", C.c_int32 * 4), ("localizable", C.c_int32 * 6),
                ("xicp_combined", C.c_double * 6), ("xicp_high", C.c_double * 6), ("source_prep_ms", C.c_float),
                ("rotation_corrected", C.c_int32), ("T_iter_prev", C.c_float * 16), ("n_tail_launches", C.c_int32),
                ("n_tail_iterations", C.c_int32)]


class NormalsOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ("normals", "eigvals", "eigvecs", "covs", "densities", "mean_dists", "ids")]


class RegCrop(C.Structure):
    _fields_ = [("type", C.c_int32), ("reserved", C.c_int32), ("center", C.c_double * 3), ("radius_min", C.c_double),
                ("radius_max", C.c_double), ("min_z", C.c_double), ("max_z", C.c_double)]


CROP_NONE, CROP_MAX_RADIUS, CROP_MIN_RADIUS, CROP_MIN_MAX_RADIUS, CROP_CYLINDER = 0, 1, 2, 3, 4


class DistStatus(C.Structure):
    _fields_ = [("sequences_done", C.c_int64), ("sequences_enqueued", C.c_int64), ("iterations", C.c_int32),
                ("done", C.c_int32), ("stall", C.c_int32), ("stream_idle", C.c_int32), ("limit_last", C.c_float),
                ("limit_prev", C.c_float)]


class DistAction(C.Structure):
    _fields_ = [("kind", C.c_int32), ("count", C.c_int32), ("seq", C.c_int64)]


class DistReply(C.Structure):
    _fields_ = [("available", C.c_int32), ("iterations", C.c_int32), ("done", C.c_int32), ("stall", C.c_int32),
                ("limit_last", C.c_float), ("limit_prev", C.c_float)]


STEER_RECORD, STEER_GENERIC, STEER_FUSED, STEER_DRAIN, STEER_DONE = 0, 1, 2, 3, 4
DT_I32, DT_I64, DT_F64 = 0, 1, 2
DIST_ID_BYTES = 128
ALL_REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p)
ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)


class Collectives(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("all_reduce_sum", ALL_REDUCE_FN), ("all_gather", ALL_GATHER_FN)]


class TargetInfo(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("n_bricks", C.c_int64), ("n_cells_occupied", C.c_int64),
                ("table_bytes", C.c_int64), ("cell_size", C.c_float), ("origin", C.c_float * 3),
                ("centroid", C.c_float * 3), ("dims", C.c_int32 * 3)]


class SsnParams(C.Structure):
    """reg_ssn_params (include/o3dslam_reg.h): SamplingSurfaceNormalDataPointsFilter's parameters."""
    _fields_ = [("struct_size", C.c_int32), ("knn", C.c_int32), ("sampling_method", C.c_int32), ("ratio", C.c_float),
                ("max_box_dim", C.c_float), ("average_existing_descriptors", C.c_int32), ("keep_normals", C.c_int32),
                ("keep_densities", C.c_int32), ("keep_eigen_values", C.c_int32), ("keep_eigen_vectors", C.c_int32)]


class SsnOut(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("normals", C.c_void_p), ("densities", C.c_void_p), ("eigvals", C.c_void_p),
                ("eigvecs", C.c_void_p), ("src_idx", C.c_void_p), ("leaf_id", C.c_void_p)]


class PointFilter(C.Structure):
    """reg_point_filter: one reading-side filter of a reg_filter_points chain."""
    _fields_ = [("type", C.c_int32), ("dim", C.c_int32), ("value", C.c_float), ("remove_inside", C.c_int32),
                ("box", C.c_float * 6), ("step", C.c_int32), ("phase", C.c_int32)]


DPF_TYPES = {"Identity": 0, "MaxDist": 1, "MinDist": 2, "BoundingBox": 3, "DistanceLimit": 4, "RemoveNaN": 5,
             "MaxQuantileOnAxis": 6, "FixStepSampling": 7}


def point_filter(spec: dict) -> PointFilter:
    """A reg_point_filter from {"type": <name without DataPointsFilter>, <reference parameter>: value, ...}; parameters
    left out take the defaults of the filter's .h."""
    t = spec["type"]
    f = PointFilter()
    f.type = DPF_TYPES[t]
    f.dim = int(spec.get("dim", 0 if t == "MaxQuantileOnAxis" else -1))
    key = {"MaxDist": "maxDist", "MinDist": "minDist", "DistanceLimit": "dist", "MaxQuantileOnAxis": "ratio"}.get(t)
    f.value = float(spec.get(key, 0.5 if t == "MaxQuantileOnAxis" else 1.0)) if key else 0.0
    f.remove_inside = int(spec.get("removeInside", 1))
    for i, (k, d) in enumerate((("xMin", -1.0), ("xMax", 1.0), ("yMin", -1.0), ("yMax", 1.0), ("zMin", -1.0),
                                ("zMax", 1.0))):
        f.box[i] = float(spec.get(k, d))
    f.step = int(spec.get("startStep", 10))
    f.phase = int(spec.get("phase", 0))
    return f


class Field(C.Structure):
    """reg_field: one descriptor field of a reg_filter_cloud call (`in_` is the C member `in`)."""
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p), ("span", C.c_int32), ("reserved", C.c_int32)]


class CloudFilter(C.Structure):
    """reg_cloud_filter: one filter of a reg_filter_cloud chain (a reg_point_filter plus the descriptor filters)."""
    _fields_ = [("struct_size", C.c_int32), ("base", PointFilter), ("field_a", C.c_int32), ("field_b", C.c_int32),
                ("field_out", C.c_int32), ("v", C.c_float * 3), ("flag", C.c_int32), ("seed", C.c_uint32),
                ("reserved", C.c_int32 * 3)]


class VoxelGridParams(C.Structure):
    """reg_voxel_grid_params (include/o3dslam_reg.h): VoxelGridDataPointsFilter's parameters."""
    _fields_ = [("struct_size", C.c_int32), ("v_size", C.c_float * 3), ("use_centroid", C.c_int32),
                ("average_existing_descriptors", C.c_int32), ("reserved", C.c_int32 * 2)]


def default_voxel_grid_params(v_size=(1.0, 1.0, 1.0), use_centroid=1, average_existing_descriptors=1) -> VoxelGridParams:
    p = VoxelGridParams()
    load_library().reg_default_voxel_grid_params(C.byref(p))
    for a in range(3):
        p.v_size[a] = float(v_size[a])
    p.use_centroid, p.average_existing_descriptors = int(use_centroid), int(average_existing_descriptors)
    return p


MAX_FIELDS = 16
MISSING_FIELD = 7    # REG_MISSING_FIELD
# descriptor filter -> (REG_DPF_*, name of field_a, name of field_b, (name, span) of field_out); "@descName": the
# filter's own parameter names the field
CLOUD_FILTERS = {
    "ObservationDirection": (8, None, None, ("observationDirections", 3)),
    "OrientNormals": (9, "normals", "observationDirections", None),
    "Shadow": (10, "normals", None, None),
    "SimpleSensorNoise": (11, None, None, ("simpleSensorNoise", 1)),
    "IncidenceAngle": (12, "normals", "observationDirections", ("incidenceAngles", 1)),
    "CutAtDescriptorThreshold": (13, "@descName", None, None),
    "MaxDensity": (14, "densities", None, None),
}


def cloud_filter_created_fields(filters) -> list:
    """(name, span) of every descriptor the chain creates, in chain order, without repeats."""
    out = []
    for spec in filters:
        made = CLOUD_FILTERS.get(spec["type"], (0, None, None, None))[3]
        if made and made not in out:
            out.append(made)
    return out


def cloud_filter(spec: dict, names: list) -> CloudFilter:
    """A reg_cloud_filter from {"type": <name without DataPointsFilter>, <reference parameter>: value, ...}; `names` lists
    the call's fields in order.  A field the filter reads that is not in `names` becomes index -1 (REG_MISSING_FIELD)."""
    c = CloudFilter()
    c.struct_size = C.sizeof(CloudFilter)
    c.field_a = c.field_b = c.field_out = -1
    t = spec["type"]
    if t not in CLOUD_FILTERS:
        c.base = point_filter(spec)
        return c
    code, a, b, made = CLOUD_FILTERS[t]
    c.base.type = code
    if a == "@descName":
        a = str(spec.get("descName", "none"))
    find = lambda name: names.index(name) if name in names else -1
    c.field_a = find(a) if a else -1
    c.field_b = find(b) if b else -1
    c.field_out = find(made[0]) if made else -1
    if t == "ObservationDirection":
        c.v[0], c.v[1], c.v[2] = float(spec.get("x", 0)), float(spec.get("y", 0)), float(spec.get("z", 0))
    elif t == "OrientNormals":
        c.flag = int(spec.get("towardCenter", 1))
    elif t == "Shadow":
        c.v[0] = np.float32(np.sin(np.float32(spec.get("eps", 0.1))))   # sin() in fp32, as the reference's T = float
    elif t == "SimpleSensorNoise":
        c.flag, c.v[0] = int(spec.get("sensorType", 0)), float(spec.get("gain", 1))
    elif t == "CutAtDescriptorThreshold":
        c.flag, c.v[0] = int(spec.get("useLargerThan", 1)), float(spec.get("threshold", 0))
    elif t == "MaxDensity":
        c.v[0], c.seed = float(spec.get("maxDensity", 10)), int(spec.get("seed", 1))
    return c


def host_glibc_rand(seed: int, count: int) -> np.ndarray:
    """reg_host_glibc_rand: the first `count` values of glibc's rand() after srand(seed)."""
    out = np.zeros(count, np.int32)
    st = load_library().reg_host_glibc_rand(int(seed), count, _ptr(out))
    if st != 0:
        raise RegError(st, "reg_host_glibc_rand")
    return out


class OctreeParams(C.Structure):
    """reg_octree_params (include/o3dslam_reg.h): OctreeGridDataPointsFilter's parameters."""
    _fields_ = [("struct_size", C.c_int32), ("build_parallel", C.c_int32), ("max_point_by_node", C.c_int64),
                ("max_size_by_node", C.c_float), ("sampling_method", C.c_int32), ("center_at_origin", C.c_int32),
                ("reserved", C.c_int32 * 5)]


class RansacParams(C.Structure):
    """reg_ransac_params (include/o3dslam_reg.h): RegistrationRANSACBasedOnCorrespondence's parameters."""
    _fields_ = [("struct_size", C.c_int32), ("ransac_n", C.c_int32), ("max_iteration", C.c_int64),
                ("confidence", C.c_double), ("max_correspondence_distance", C.c_double),
                ("distance_threshold", C.c_double), ("edge_similarity", C.c_double), ("seed", C.c_uint64),
                ("batch", C.c_int32), ("reserved", C.c_int32)]


class RansacResult(C.Structure):
    """reg_ransac_result (include/o3dslam_reg.h)."""
    _fields_ = [("struct_size", C.c_int32), ("batch", C.c_int32), ("T", C.c_double * 16), ("fitness", C.c_double),
                ("inlier_rmse", C.c_double), ("n_inliers", C.c_int64), ("n_iterations", C.c_int64),
                ("n_validated", C.c_int64), ("best_iteration", C.c_int64)]


class ScanParams(C.Structure):
    """reg_scan_params (include/o3dslam_reg.h): the scan front end's croppers, voxel size, ratio, seed and normal search."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("wide", RegCrop), ("narrow", RegCrop),
                ("voxel_size", C.c_double), ("down_sampling_ratio", C.c_double), ("seed", C.c_uint64),
                ("normal_knn", C.c_int32), ("reserved2", C.c_int32), ("normal_radius", C.c_double)]


class ScanResult(C.Structure):
    """reg_scan_result (include/o3dslam_reg.h)."""
    _fields_ = [("struct_size", C.c_int32), ("has_normals", C.c_int32), ("has_covs", C.c_int32),
                ("scan_prep_ms", C.c_float), ("n_wide", C.c_int64), ("n_voxels", C.c_int64), ("n_merge", C.c_int64),
                ("n_match", C.c_int64)]


class DenseScanParams(C.Structure):
    """reg_dense_scan_params (include/o3dslam_reg.h): the dense-map cropper and the colour range of insert_scan."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("crop", RegCrop), ("rgb_min", C.c_double * 3),
                ("rgb_max", C.c_double * 3)]


class DenseCarveParams(C.Structure):
    """reg_dense_carve_params (include/o3dslam_reg.h)."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("neighborhood_radius", C.c_double),
                ("max_ray", C.c_double), ("truncation", C.c_double)]


class DenseMapInfo(C.Structure):
    """reg_dense_map_info (include/o3dslam_reg.h)."""
    _fields_ = [("struct_size", C.c_int32), ("has_normals", C.c_int32), ("has_colors", C.c_int32), ("reserved", C.c_int32),
                ("n_voxels", C.c_int64), ("capacity", C.c_int64), ("voxel_size", C.c_double)]


class MapCloudParams(C.Structure):
    """reg_map_cloud_params (include/o3dslam_reg.h): the field set, the map builder's voxel size and cropper, the carve."""
    _fields_ = [("struct_size", C.c_int32), ("has_normals", C.c_int32), ("has_covariances", C.c_int32),
                ("carve_every_n_scans", C.c_int32), ("map_voxel_size", C.c_double), ("crop", RegCrop),
                ("carve_voxel_size", C.c_double), ("carve_max_ray", C.c_double), ("carve_truncation", C.c_double),
                ("carve_min_dot", C.c_double)]


class MapCloudInfo(C.Structure):
    """reg_map_cloud_info (include/o3dslam_reg.h)."""
    _fields_ = [("struct_size", C.c_int32), ("has_normals", C.c_int32), ("has_covariances", C.c_int32),
                ("reserved", C.c_int32), ("n_rows", C.c_int64), ("capacity", C.c_int64), ("scans_inserted", C.c_int64),
                ("crop_center", C.c_double * 3)]


class MapCloudInsertResult(C.Structure):
    """reg_map_cloud_insert_result (include/o3dslam_reg.h)."""
    _fields_ = [("struct_size", C.c_int32), ("carved", C.c_int32), ("n_carved", C.c_int64), ("n_outside", C.c_int64),
                ("n_voxels", C.c_int64), ("n_rows", C.c_int64)]


def default_map_cloud_params(crop=None, **overrides) -> MapCloudParams:
    """reg_default_map_cloud_params: the shipped map builder (voxel 0.03, MaxRadius 20, carve voxel 0.1 / ray 20 /
    truncation 0.1 / min dot 0.5 every 10 scans; normals, no covariances); crop: a crop dict of Registration.set_target_f64."""
    p = MapCloudParams()
    load_library().reg_default_map_cloud_params(C.byref(p))
    if crop is not None:
        p.crop = Registration._crop_struct(crop)
    for k, v in overrides.items():
        if k in ("has_normals", "has_covariances", "carve_every_n_scans"):
            setattr(p, k, int(v))
        elif k in ("map_voxel_size", "carve_voxel_size", "carve_max_ray", "carve_truncation", "carve_min_dot"):
            setattr(p, k, float(v))
        else:
            raise TypeError(f"unknown map cloud parameter {k}")
    return p


class SubmapsParams(C.Structure):
    """reg_submaps_params (include/o3dslam_reg.h): SubmapParameters, the place-recognition gates and every submap's map cloud."""
    _fields_ = [("struct_size", C.c_int32), ("max_submaps", C.c_int32), ("num_scans_overlap", C.c_int32),
                ("min_num_range_data", C.c_int32), ("is_use_initial_map", C.c_int32), ("is_carving_enabled", C.c_int32),
                ("min_submaps_between_loop_closures", C.c_int32), ("reserved", C.c_int32), ("max_num_points", C.c_int64),
                ("radius", C.c_double), ("revisit_min_fitness", C.c_double), ("voxel_expansion_factor", C.c_double),
                ("min_seconds_between_features", C.c_double), ("loop_closure_search_radius", C.c_double),
                ("map", MapCloudParams)]


class SubmapsInfo(C.Structure):
    """reg_submaps_info (include/o3dslam_reg.h)."""
    _fields_ = [("struct_size", C.c_int32), ("n_submaps", C.c_int32), ("active", C.c_int32), ("force_new_submap", C.c_int32),
                ("scans_in_active", C.c_int32), ("ring_size", C.c_int32), ("n_finished", C.c_int32),
                ("n_loop_closure_candidates", C.c_int32), ("last_finished", C.c_int32), ("reserved", C.c_int32),
                ("total_points", C.c_int64), ("stamp_ns", C.c_int64), ("T_map_to_sensor", C.c_double * 16)]


class SubmapInfo(C.Structure):
    """reg_submap_info (include/o3dslam_reg.h)."""
    _fields_ = [("struct_size", C.c_int32), ("id", C.c_int32), ("parent", C.c_int32), ("center_computed", C.c_int32),
                ("features_computed", C.c_int32), ("reserved", C.c_int32), ("n_rows", C.c_int64), ("scans_inserted", C.c_int64),
                ("n_keys", C.c_int64), ("origin", C.c_double * 16), ("center", C.c_double * 3), ("crop_center", C.c_double * 3),
                ("T_map_to_sensor", C.c_double * 16), ("feature_clock", C.c_double)]


class SubmapsInsertResult(C.Structure):
    """reg_submaps_insert_result (include/o3dslam_reg.h)."""
    _fields_ = [("struct_size", C.c_int32), ("decision", C.c_int32), ("previous_active", C.c_int32), ("active", C.c_int32),
                ("fitness_computed", C.c_int32), ("ring_drained", C.c_int32), ("fitness_count", C.c_int64),
                ("fitness", C.c_double), ("insert", MapCloudInsertResult)]


class SubmapFeatureParams(C.Structure):
    """reg_submap_feature_params (include/o3dslam_reg.h): what Submap::computeFeatures reads of PlaceRecognitionParameters."""
    _fields_ = [("struct_size", C.c_int32), ("normal_knn", C.c_int32), ("feature_knn", C.c_int32), ("reserved", C.c_int32),
                ("feature_voxel_size", C.c_double), ("normal_radius", C.c_double), ("feature_radius", C.c_double)]


def default_submap_feature_params(**overrides) -> SubmapFeatureParams:
    """reg_default_submap_feature_params: knn 10 within 1 m, voxel 0.5 m, FPFH 100 within 2.5 m (Parameters.hpp:121-126)."""
    p = SubmapFeatureParams()
    load_library().reg_default_submap_feature_params(C.byref(p))
    for k, v in overrides.items():
        if k not in ("normal_knn", "feature_knn", "feature_voxel_size", "normal_radius", "feature_radius"):
            raise TypeError(f"unknown feature parameter {k}")
        setattr(p, k, int(v) if k.endswith("knn") else float(v))
    return p


SUBMAPS_KEEP, SUBMAPS_SWITCH, SUBMAPS_CREATE, SUBMAPS_NEED_FITNESS = 0, 1, 2, 3
SUBMAPS_ACTION_MASK, SUBMAPS_SET_FORCE_FLAG, SUBMAPS_FORCED = 3, 4, 8
_SUBMAPS_INT = ("max_submaps", "num_scans_overlap", "min_num_range_data", "is_use_initial_map", "is_carving_enabled",
                "min_submaps_between_loop_closures", "max_num_points")
_SUBMAPS_FLOAT = ("radius", "revisit_min_fitness", "voxel_expansion_factor", "min_seconds_between_features",
                  "loop_closure_search_radius")


def default_submaps_params(map_params: "MapCloudParams | None" = None, **overrides) -> SubmapsParams:
    """reg_default_submaps_params: SubmapParameters as shipped (radius 20, 5 scans, 400000 points, fitness 0.4, overlap 3),
    factor 2.5, 64 submaps, the default map cloud; map_params replaces the map cloud's."""
    p = SubmapsParams()
    load_library().reg_default_submaps_params(C.byref(p))
    if map_params is not None:
        p.map = map_params
        p.map.struct_size = C.sizeof(MapCloudParams)
    for k, v in overrides.items():
        if k in _SUBMAPS_INT:
            setattr(p, k, int(v))
        elif k in _SUBMAPS_FLOAT:
            setattr(p, k, float(v))
        else:
            raise TypeError(f"unknown submaps parameter {k}")
    return p


def check_submaps_params(params: SubmapsParams) -> int:
    """reg_check_submaps_params: the status reg_submaps_create would return for these parameters (no device)."""
    return int(load_library().reg_check_submaps_params(C.byref(params)))


def submaps_struct_sizes() -> tuple:
    """sizeof of reg_submaps_params, reg_submaps_info, reg_submap_info, reg_submaps_insert_result,
    reg_submap_feature_params in the library."""
    out = (C.c_int32 * 5)()
    load_library().reg_submaps_struct_sizes(out)
    return tuple(out)


def host_submaps_decide(force_flag, scans_in_active, min_num_range_data, is_use_initial_map, active_points, max_num_points,
                        closest_is_active, distance_to_closest, distance_to_active, radius, adjacent, fitness_ok) -> int:
    """reg_host_submaps_decide: the SUBMAPS_* bits of updateActiveSubmap's branch for these inputs (no device)."""
    return int(load_library().reg_host_submaps_decide(int(bool(force_flag)), int(scans_in_active), int(min_num_range_data),
                                                      int(bool(is_use_initial_map)), int(active_points), int(max_num_points),
                                                      int(bool(closest_is_active)), float(distance_to_closest),
                                                      float(distance_to_active), float(radius), int(bool(adjacent)),
                                                      int(fitness_ok)))


def host_adjacency_distance(adj, marks, node) -> int:
    """reg_host_adjacency_distance: getDistanceToNearestLoopClosureSubmap on an n x n 0 / 1 matrix and marks (-1 / 0 / 1)."""
    a = np.ascontiguousarray(adj, np.uint8)
    m = np.ascontiguousarray(marks, np.int32)
    return int(load_library().reg_host_adjacency_distance(_ptr(a), _ptr(m), int(m.shape[0]), int(node)))


def host_submaps_transform_plan(parents, ids):
    """reg_host_submaps_transform_plan: (status, plan); plan[i] = position in ids of the increment submap i receives, -1 none."""
    pa = np.ascontiguousarray(parents, np.int32)
    i = np.ascontiguousarray(ids, np.int32).reshape(-1)
    plan = np.full(pa.shape[0], -1, np.int32)
    st = load_library().reg_host_submaps_transform_plan(_ptr(pa), int(pa.shape[0]), _ptr(i) if i.size else None, int(i.size),
                                                        _ptr(plan))
    return int(st), plan


def host_mapper_initial_guess(prev_map_to_sensor, odom_prev, odom_now, calib=None) -> np.ndarray:
    """reg_host_mapper_initial_guess: prev * ((odom_prev calib^-1)^-1 (odom_now calib^-1)) in fp64 with rigid inverses."""
    out = (C.c_double * 16)()
    st = load_library().reg_host_mapper_initial_guess(_T_in_f64(prev_map_to_sensor), _T_in_f64(odom_prev), _T_in_f64(odom_now),
                                                      _T_in_f64(np.eye(4) if calib is None else calib), out)
    if st != 0:
        raise RegError(st)
    return np.array(out, np.float64).reshape(4, 4).T.copy()


class UndistortParams(C.Structure):
    """reg_undistort_params (include/o3dslam_reg.h): spin direction, scan duration and the two velocities of the sensor."""
    _fields_ = [("struct_size", C.c_int32), ("spinning_clockwise", C.c_int32), ("scan_duration", C.c_double),
                ("linear_velocity", C.c_double * 3), ("angular_velocity_rpy", C.c_double * 3)]


def undistort_params(scan_duration, linear_velocity=(0.0, 0.0, 0.0), angular_velocity_rpy=(0.0, 0.0, 0.0),
                     spinning_clockwise=True) -> UndistortParams:
    """reg_undistort_params for given velocities (validated by the call that takes them)."""
    u = UndistortParams()
    u.struct_size = C.sizeof(UndistortParams)
    u.spinning_clockwise = int(bool(spinning_clockwise))
    u.scan_duration = float(scan_duration)
    u.linear_velocity = (C.c_double * 3)(*[float(v) for v in linear_velocity])
    u.angular_velocity_rpy = (C.c_double * 3)(*[float(v) for v in angular_velocity_rpy])
    return u


def host_undistort_point(p, params: UndistortParams) -> np.ndarray:
    """reg_host_undistort_point: one point of reg_undistort_scan on the host (no device)."""
    a = (C.c_double * 3)(*[float(v) for v in p])
    out = (C.c_double * 3)()
    st = load_library().reg_host_undistort_point(a, C.byref(params), out)
    if st != 0:
        raise RegError(st, "reg_host_undistort_point")
    return np.array(out, np.float64)


class PoseGraphParams(C.Structure):
    """reg_pose_graph_params (include/o3dslam_reg.h): GlobalOptimizationOption and GlobalOptimizationConvergenceCriteria."""
    _fields_ = [("struct_size", C.c_int32), ("reference_node", C.c_int32), ("max_correspondence_distance", C.c_double),
                ("preference_loop_closure", C.c_double), ("edge_prune_threshold", C.c_double), ("max_iteration", C.c_int32),
                ("max_iteration_lm", C.c_int32), ("min_relative_increment", C.c_double),
                ("min_relative_residual_increment", C.c_double), ("min_right_term", C.c_double), ("min_residual", C.c_double),
                ("upper_scale_factor", C.c_double), ("lower_scale_factor", C.c_double)]


class PoseGraphResult(C.Structure):
    """reg_pose_graph_result (include/o3dslam_reg.h): the statistics of one Levenberg-Marquardt pass."""
    _fields_ = [("struct_size", C.c_int32), ("outer_iterations", C.c_int32), ("lm_solves", C.c_int32),
                ("accepted_steps", C.c_int32), ("stop_reason", C.c_int32), ("valid_edges", C.c_int32),
                ("first_residual", C.c_double), ("last_residual", C.c_double), ("last_lambda", C.c_double),
                ("weight", C.c_double)]


class PoseGraphInfo(C.Structure):
    """reg_pose_graph_info (include/o3dslam_reg.h)."""
    _fields_ = [("struct_size", C.c_int32), ("n_nodes", C.c_int32), ("n_edges", C.c_int32), ("n_uncertain", C.c_int32),
                ("solver_rows", C.c_int64), ("device_bytes", C.c_int64)]


POSE_GRAPH_MAX_NODES = 2048   # REG_POSE_GRAPH_MAX_NODES
PG_STOP_NAMES = {0: "NONE", 1: "RIGHT_TERM", 2: "INCREMENT", 3: "RESIDUAL_INCREMENT", 4: "MAX_ITERATION_LM",
                 5: "MIN_RESIDUAL", 6: "MAX_ITERATION"}


def default_pose_graph_params(**overrides) -> PoseGraphParams:
    """reg_default_pose_graph_params (Parameters.hpp:142-147 and Open3D's criteria defaults); overrides by field name."""
    p = PoseGraphParams()
    load_library().reg_default_pose_graph_params(C.byref(p))
    for k, v in overrides.items():
        if k in ("reference_node", "max_iteration", "max_iteration_lm"):
            setattr(p, k, int(v))
        elif k != "struct_size" and k in dict(PoseGraphParams._fields_):
            setattr(p, k, float(v))
        else:
            raise TypeError(f"unknown pose graph parameter {k}")
    return p


def check_pose_graph_params(params: PoseGraphParams) -> int:
    """reg_check_pose_graph_params: the validation of PoseGraph(), without a device.  Returns the status."""
    return int(load_library().reg_check_pose_graph_params(C.byref(params)))


def pose_graph_struct_sizes() -> tuple:
    """reg_pose_graph_struct_sizes: sizeof of (reg_pose_graph_params, reg_pose_graph_result, reg_pose_graph_info)."""
    out = (C.c_int32 * 3)()
    load_library().reg_pose_graph_struct_sizes(out)
    return tuple(out)


def _rows16(T) -> np.ndarray:
    a = np.ascontiguousarray(T, np.float64)
    if a.size != 16:
        raise ValueError("a 4 x 4 matrix is expected")
    return a.reshape(16)


def host_pose_graph_edge(Ts, Tt, X):
    """reg_host_pose_graph_edge: (zeta (6), Js, Jt (6 x 6)) of one edge on the host (no device)."""
    z, Js, Jt = np.empty(6), np.empty((6, 6)), np.empty((6, 6))
    st = load_library().reg_host_pose_graph_edge(_ptr(_rows16(Ts)), _ptr(_rows16(Tt)), _ptr(_rows16(X)), _ptr(z), _ptr(Js),
                                                 _ptr(Jt))
    if st != 0:
        raise RegError(st, "reg_host_pose_graph_edge")
    return z, Js, Jt


def host_pose_vector(T) -> np.ndarray:
    """reg_host_pose_vector: (alpha, beta, gamma, x, y, z) of a pose on the host (no device)."""
    x = np.empty(6)
    st = load_library().reg_host_pose_vector(_ptr(_rows16(T)), _ptr(x))
    if st != 0:
        raise RegError(st, "reg_host_pose_vector")
    return x


def host_pose_step(delta, pose) -> np.ndarray:
    """reg_host_pose_step: V(delta) pose on the host (no device)."""
    d = np.ascontiguousarray(delta, np.float64).reshape(6)
    out = np.empty((4, 4))
    st = load_library().reg_host_pose_step(_ptr(d), _ptr(_rows16(pose)), _ptr(out))
    if st != 0:
        raise RegError(st, "reg_host_pose_step")
    return out


def host_line_process_weight(info, preference, max_correspondence_distance) -> float:
    """reg_host_line_process_weight of E x 6 x 6 information matrices on the host (no device)."""
    a = np.ascontiguousarray(info, np.float64).reshape(-1, 36)
    w = C.c_double(0.0)
    st = load_library().reg_host_line_process_weight(_ptr(a) if a.shape[0] else None, a.shape[0], float(preference),
                                                     float(max_correspondence_distance), C.byref(w))
    if st != 0:
        raise RegError(st, "reg_host_line_process_weight")
    return float(w.value)


class OdometryParams(C.Structure):
    """reg_odometry_params (include/o3dslam_reg.h): the scan cropper and processing, GICP's epsilon, the fitness gate."""
    _fields_ = [("struct_size", C.c_int32), ("use_odometry_topic", C.c_int32), ("crop", RegCrop), ("voxel_size", C.c_double),
                ("down_sampling_ratio", C.c_double), ("seed", C.c_uint64), ("normal_knn", C.c_int32), ("reserved", C.c_int32),
                ("normal_radius", C.c_double), ("gicp_epsilon", C.c_double), ("min_fitness", C.c_double)]


class OdometryResult(C.Structure):
    """reg_odometry_result (include/o3dslam_reg.h); T_matrix() / cumulative_matrix() give the 4 x 4 math layout."""
    _fields_ = [("struct_size", C.c_int32), ("accepted", C.c_int32), ("pose_updated", C.c_int32), ("registered", C.c_int32),
                ("iterations", C.c_int32), ("reserved", C.c_int32), ("n_crop", C.c_int64), ("n_voxels", C.c_int64),
                ("n_selected", C.c_int64), ("n_source", C.c_int64), ("n_target", C.c_int64), ("fitness", C.c_double),
                ("inlier_rmse", C.c_double), ("cumulative", C.c_double * 16), ("T", C.c_float * 16), ("prep_ms", C.c_float),
                ("register_ms", C.c_float)]

    def T_matrix(self) -> np.ndarray:
        return _T_out(self.T)

    def cumulative_matrix(self) -> np.ndarray:
        return np.array(self.cumulative, np.float64).reshape(4, 4).T.copy()


class OdometryInfo(C.Structure):
    """reg_odometry_info (include/o3dslam_reg.h)."""
    _fields_ = [("struct_size", C.c_int32), ("has_cloud", C.c_int32), ("has_normals", C.c_int32),
                ("has_covariances", C.c_int32), ("has_stamp", C.c_int32), ("initial_pending", C.c_int32),
                ("n_rows", C.c_int64), ("last_stamp_ns", C.c_int64), ("cumulative", C.c_double * 16)]


ODOM_ACCEPTED, ODOM_POSE_UPDATED, ODOM_REPLACE_CLOUD, ODOM_POSE_FROM_INITIAL = 1, 2, 4, 8
ODOM_ACCUMULATE, ODOM_RECORD_STAMP, ODOM_PREPROCESS, ODOM_REGISTER = 16, 32, 64, 128


def default_odometry_params(crop=None, **overrides) -> OdometryParams:
    """reg_default_odometry_params (the shipped scan cropper and processing, gicp_epsilon 1e-3, min_fitness 0.1,
    use_odometry_topic 1); crop: a crop dict of Registration.set_target_f64; overrides by field name."""
    p = OdometryParams()
    load_library().reg_default_odometry_params(C.byref(p))
    if crop is not None:
        p.crop = Registration._crop_struct(crop)
    for k, v in overrides.items():
        if k in ("use_odometry_topic", "normal_knn", "seed"):
            setattr(p, k, int(v))
        elif k in ("voxel_size", "down_sampling_ratio", "normal_radius", "gicp_epsilon", "min_fitness"):
            setattr(p, k, float(v))
        else:
            raise TypeError(f"unknown odometry parameter {k}")
    return p


def check_odometry_params(params: "RegParams", odometry: OdometryParams) -> int:
    """reg_check_odometry_params: the validation of Odometry(), without a device.  Returns the status."""
    return int(load_library().reg_check_odometry_params(C.byref(params), C.byref(odometry)))


def odometry_struct_sizes() -> tuple:
    """reg_odometry_struct_sizes: sizeof of (reg_odometry_params, reg_odometry_result, reg_odometry_info) in the library."""
    out = (C.c_int32 * 3)()
    load_library().reg_odometry_struct_sizes(out)
    return tuple(out)


def host_covariance_from_normal(normal, epsilon=1e-3) -> np.ndarray:
    """reg_host_covariance_from_normal: one row of reg_covariances_from_normals on the host (no device); 3 x 3."""
    a = (C.c_double * 3)(*[float(v) for v in normal])
    out = (C.c_double * 9)()
    st = load_library().reg_host_covariance_from_normal(a, float(epsilon), out)
    if st != 0:
        raise RegError(st, "reg_host_covariance_from_normal")
    return np.array(out, np.float64).reshape(3, 3)


def host_odometry_decide(has_previous, timestamp, last_stamp, use_odometry_topic, n_rows, fitness, min_fitness,
                         initial_pending) -> int:
    """reg_host_odometry_decide: the ODOM_* bits of addRangeScan's branch for these inputs (no device)."""
    return int(load_library().reg_host_odometry_decide(int(bool(has_previous)), int(timestamp), int(last_stamp),
                                                       int(bool(use_odometry_topic)), int(n_rows), float(fitness),
                                                       float(min_fitness), int(bool(initial_pending))))


def host_odometry_accumulate(cumulative, T) -> np.ndarray:
    """reg_host_odometry_accumulate: cumulative (4 x 4 float64) times the inverse of T (4 x 4, cast to float32 as the
    registration returns it), on the host (no device)."""
    cum = _T_in_f64(cumulative)
    Tf = _T_in(T)
    st = load_library().reg_host_odometry_accumulate(cum, _ptr(Tf))
    if st != 0:
        raise RegError(st, "reg_host_odometry_accumulate")
    return np.array(cum, np.float64).reshape(4, 4).T.copy()


def default_dense_scan_params(crop=None, rgb_min=None, rgb_max=None) -> DenseScanParams:
    """reg_default_dense_scan_params (no crop, colours within [0, 1]); crop: a crop dict of Registration.set_target_f64."""
    p = DenseScanParams()
    load_library().reg_default_dense_scan_params(C.byref(p))
    if crop is not None:
        p.crop = Registration._crop_struct(crop)
    for name, v in (("rgb_min", rgb_min), ("rgb_max", rgb_max)):
        if v is not None:
            setattr(p, name, (C.c_double * 3)(*[float(x) for x in v]))
    return p


def default_dense_carve_params(**overrides) -> DenseCarveParams:
    """reg_default_dense_carve_params: SpaceCarvingParameters as shipped (radius 0.1, max ray 20, truncation 0.1)."""
    p = DenseCarveParams()
    load_library().reg_default_dense_carve_params(C.byref(p))
    for k, v in overrides.items():
        if k not in ("neighborhood_radius", "max_ray", "truncation"):
            raise TypeError(f"unknown carve parameter {k}")
        setattr(p, k, float(v))
    return p


def host_dense_offsets(neighborhood_radius: float, voxel_size: float) -> np.ndarray:
    """reg_host_dense_offsets: the per-axis neighbourhood offsets of DenseMap.carve (no device); ValueError for arguments the
    carve refuses (more than 16 offsets, radius or voxel size not finite and > 0)."""
    out = np.zeros(16, np.float64)
    k = load_library().reg_host_dense_offsets(float(neighborhood_radius), float(voxel_size), out.ctypes.data_as(C.c_void_p))
    if k < 0:
        raise ValueError(f"no neighbourhood for radius {neighborhood_radius!r}, voxel size {voxel_size!r}")
    return out[:k].copy()


def host_scan_key(seed: int, index: int) -> int:
    """reg_host_scan_key: the 64-bit key of reg_random_down_sample for point `index` (no device)."""
    return int(load_library().reg_host_scan_key(int(seed), int(index)))


def default_scan_params(**overrides) -> ScanParams:
    """reg_default_scan_params; wide / narrow accept the crop dicts of Registration.set_target_f64."""
    p = ScanParams()
    load_library().reg_default_scan_params(C.byref(p))
    for k, v in overrides.items():
        if k in ("wide", "narrow"):
            v = Registration._crop_struct(v if v is not None else {"type": CROP_NONE})
        elif not hasattr(p, k):
            raise TypeError(f"unknown scan parameter {k}")
        setattr(p, k, v)
    p.struct_size = C.sizeof(ScanParams)
    return p


def host_ransac_est_k(est_k, confidence, count, k, ransac_n) -> float:
    """reg_host_ransac_est_k: the RANSAC stop rule after a replacement (libm on the host; no device)."""
    return float(load_library().reg_host_ransac_est_k(float(est_k), float(confidence), int(count), int(k), int(ransac_n)))


class OctreeOut(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("normals", C.c_void_p), ("covs", C.c_void_p), ("src_idx", C.c_void_p),
                ("leaf_id", C.c_void_p), ("leaf_depth", C.c_void_p)]


class PmChain(C.Structure):
    """reg_pm_chain up to `var_lambda` (REG_PM_CHAIN_SIZE_V2 bytes): the libpointmatcher chain extension (k-NN matching,
    RobustOutlierFilter, PointToPoint, and the MinDist / MedianDist / VarTrimmedDist outlier filters appended after
    `reserved`).  The C ABI accepts this size; the fields after it are then off.  PmChainV3 is the whole struct."""
    _fields_ = [("struct_size", C.c_int32), ("knn", C.c_int32), ("minimizer", C.c_int32), ("use_robust", C.c_int32),
                ("robust_fct", C.c_int32), ("tuning", C.c_float), ("scale_estimator", C.c_int32),
                ("nb_iter_for_scale", C.c_int32), ("distance_type", C.c_int32), ("approximation", C.c_float),
                ("reserved", C.c_int32 * 2),
                ("use_min_dist_filter", C.c_int32), ("outlier_min_dist", C.c_float),
                ("use_median_dist", C.c_int32), ("median_factor", C.c_float),
                ("use_var_trimmed", C.c_int32), ("var_min_ratio", C.c_float), ("var_max_ratio", C.c_float),
                ("var_lambda", C.c_float)]


class PmChainV3(PmChain):
    """The whole reg_pm_chain: PmChain plus the pose covariance, BoundTransformationChecker and SolutionRemapping fields
    appended after `var_lambda` (a ctypes subclass appends its fields to its base's)."""
    _fields_ = [("with_cov", C.c_int32), ("sensor_std_dev", C.c_float),
                ("use_bound", C.c_int32), ("max_rotation_norm", C.c_float), ("max_translation_norm", C.c_float),
                ("bound_after_counter", C.c_int32),
                ("degeneracy_method", C.c_int32), ("sr_threshold", C.c_float), ("sr_use2019", C.c_int32),
                ("reserved2", C.c_int32)]


class MinimizerStats(C.Structure):
    """reg_minimizer_stats: the ErrorMinimizer quality getters of the last registration."""
    _fields_ = [("struct_size", C.c_int32), ("returned_prior", C.c_int32), ("point_used_ratio", C.c_double),
                ("weighted_point_used_ratio", C.c_double), ("overlap", C.c_double), ("residual_error", C.c_double),
                ("n_rejected_matches", C.c_int64), ("n_rejected_points", C.c_int64)]


class TernaryXicp(C.Structure):
    """reg_ternary_xicp: degeneracyAwareness EqualityConstraints (X-ICP, ternary), a companion of the chain."""
    _fields_ = [("struct_size", C.c_int32), ("enabled", C.c_int32), ("high_information", C.c_float),
                ("enough_information", C.c_float), ("insufficient_information", C.c_float),
                ("min_alignment_angle_deg", C.c_float), ("strong_alignment_angle_deg", C.c_float), ("reserved", C.c_int32)]


class TernaryXicpResult(C.Structure):
    """reg_ternary_xicp_result: the analysis of the last iteration (taken at T_iter_prev)."""
    _fields_ = [("struct_size", C.c_int32), ("iteration", C.c_int32), ("category", C.c_int32 * 6), ("sane", C.c_int32),
                ("reserved", C.c_int32), ("combined", C.c_double * 6), ("high", C.c_double * 6),
                ("n_combined", C.c_int64 * 6), ("n_high", C.c_int64 * 6), ("n_pairs", C.c_int64),
                ("constraint", C.c_float * 6), ("partial_sums", (C.c_double * 9) * 6), ("eigenvectors", (C.c_float * 9) * 2)]


TERNARY_LOCALIZABLE, TERNARY_PARTIAL_MIXED, TERNARY_PARTIAL_HIGH, TERNARY_NONE = 0, 1, 2, 3
PM_CHAIN_SIZE_V1 = 48   # REG_PM_CHAIN_SIZE_V1: the struct up to `reserved`, still accepted (the later fields off)
PM_CHAIN_SIZE_V2 = 80   # REG_PM_CHAIN_SIZE_V2: the struct up to `var_lambda`, still accepted (covariance / Bound / SR off)
DEGENERACY_NONE, DEGENERACY_SOLUTION_REMAPPING = 0, 1
PM_POINT_TO_PLANE, PM_POINT_TO_POINT = 0, 1
ROBUST_FCTS = {"cauchy": 0, "welsch": 1, "sc": 2, "gm": 3, "tukey": 4, "huber": 5, "L1": 6, "student": 7}
SCALE_ESTIMATORS = {"none": 0, "mad": 1, "berg": 2, "std": 3}
DISTANCE_TYPES = {"point2point": 0, "point2plane": 1}


EXPORTS = ["reg_default_params", "reg_shipped_params", "reg_create", "reg_destroy", "reg_last_error",
           "reg_set_stream", "reg_set_target", "reg_set_source", "reg_register", "reg_compute", "reg_prepare",
           "reg_linearize", "reg_get_correspondences", "reg_match_local", "reg_trim_histogram", "reg_reduce_local",
           "reg_solve_update", "reg_host_solve6", "reg_host_x_to_T", "reg_host_centroid", "reg_get_target_info", "reg_profile_kernels", "reg_source_centroid_sums", "reg_prepare_centroid", "reg_compose",
           "reg_dist_begin", "reg_dist_buffers", "reg_dist_phase", "reg_dist_finish",
           "reg_dist_fused_buffers", "reg_dist_poll", "reg_estimate_normals", "reg_smooth_normals", "reg_host_solve6_xicp",
           "reg_set_target_f64", "reg_get_target_source_indices", "reg_voxelize_within_volume", "reg_carve_indices", "reg_dist_xicp_buffers", "reg_dist_gather_buffers",
           "reg_dist_record", "reg_dist_centroid_sums", "reg_dist_prepare",
           "reg_information_matrix", "reg_set_source_f64", "reg_debug_configure", "reg_debug_halo_bound", "reg_debug_halo_witness",
           "reg_debug_live_resources",
           "reg_dist_get_unique_id", "reg_dist_init", "reg_dist_init_custom", "reg_dist_register", "reg_dist_shutdown",
           "reg_dist_info", "reg_dist_steer_create", "reg_dist_steer_destroy", "reg_dist_steer_step",
           "reg_dist_steer_counts", "reg_host_tail_plan", "reg_host_o3d_update",
           "reg_default_pm_chain", "reg_check_pm_chain", "reg_set_pm_chain", "reg_get_robust_state",
           "reg_get_correspondences_k", "reg_host_robust_weights", "reg_host_pm_p2p_update",
           "reg_get_var_trim", "reg_host_var_trim",
           "reg_get_covariance", "reg_get_covariance_sums", "reg_host_censi_covariance", "reg_get_minimizer_stats",
           "reg_get_degeneracy", "reg_get_bound", "reg_host_solution_remap",
           "reg_default_ternary_xicp", "reg_check_ternary_xicp", "reg_set_ternary_xicp", "reg_get_ternary_xicp",
           "reg_host_ternary_decide", "reg_host_partial_constraint", "reg_host_solve6_xicp_rhs",
           "reg_default_ssn_params", "reg_sampling_surface_normal", "reg_filter_points",
           "reg_default_octree_params", "reg_octree_grid", "reg_host_octree_root", "reg_host_octree_random_picks",
           "reg_filter_cloud", "reg_host_glibc_rand", "reg_default_voxel_grid_params", "reg_voxel_grid",
           "reg_overlap_indices", "reg_set_pair_overlap_f64", "reg_get_source_source_indices",
           "reg_compute_fpfh", "reg_match_features", "reg_ransac_correspondences", "reg_host_ransac_est_k",
           "reg_voxel_down_sample", "reg_random_down_sample", "reg_host_scan_key", "reg_default_scan_params",
           "reg_process_scan",
           "reg_dense_map_create", "reg_dense_map_destroy", "reg_dense_map_clear", "reg_dense_map_insert",
           "reg_default_dense_scan_params", "reg_dense_map_insert_scan", "reg_default_dense_carve_params",
           "reg_dense_map_carve", "reg_dense_map_transform", "reg_dense_map_center", "reg_dense_map_get_info",
           "reg_dense_map_export", "reg_dedup_voxels", "reg_host_dense_offsets",
           "reg_default_map_cloud_params", "reg_map_cloud_create", "reg_map_cloud_destroy", "reg_map_cloud_clear",
           "reg_map_cloud_get_info", "reg_map_cloud_set", "reg_map_cloud_insert_scan", "reg_map_cloud_set_target",
           "reg_map_cloud_transform", "reg_map_cloud_center", "reg_map_cloud_export",
           "reg_undistort_scan", "reg_host_undistort_point",
           "reg_get_source_count", "reg_covariances_from_normals", "reg_host_covariance_from_normal",
           "reg_default_odometry_params", "reg_check_odometry_params", "reg_odometry_struct_sizes", "reg_odometry_create",
           "reg_odometry_destroy", "reg_odometry_clear", "reg_odometry_get_info", "reg_odometry_set_initial_transform",
           "reg_odometry_add_scan", "reg_odometry_export_cloud", "reg_odometry_get_correspondences",
           "reg_host_odometry_decide", "reg_host_odometry_accumulate",
           "reg_default_pose_graph_params", "reg_check_pose_graph_params", "reg_pose_graph_struct_sizes",
           "reg_pose_graph_create", "reg_pose_graph_destroy", "reg_pose_graph_clear", "reg_pose_graph_set",
           "reg_pose_graph_linearize", "reg_pose_graph_optimize", "reg_pose_graph_global_optimize", "reg_pose_graph_get",
           "reg_pose_graph_get_edge_ids", "reg_pose_graph_get_info", "reg_host_pose_graph_edge", "reg_host_pose_vector", "reg_host_pose_step",
           "reg_host_line_process_weight", "reg_debug_spd_solve_f64",
           "reg_default_submaps_params", "reg_default_submap_feature_params", "reg_check_submaps_params", "reg_submaps_struct_sizes", "reg_submaps_create",
           "reg_submaps_destroy", "reg_submaps_get_info", "reg_submaps_get_submap_info", "reg_submaps_set_map_to_sensor",
           "reg_submaps_insert_scan", "reg_submaps_force_new_submap", "reg_submaps_compute_features", "reg_submaps_get_keys",
           "reg_submaps_switch_fitness", "reg_submaps_set_target", "reg_submaps_export_submap", "reg_submaps_export",
           "reg_submaps_transform", "reg_submaps_add_loop_closure_edges", "reg_submaps_get_adjacency",
           "reg_submaps_pop_finished", "reg_submaps_pop_loop_closure_candidates", "reg_submaps_push_loop_closure_candidate",
           "reg_submaps_loop_closure_candidates", "reg_submaps_odometry_constraint_pairs", "reg_host_submaps_decide",
           "reg_host_adjacency_distance", "reg_host_submaps_transform_plan", "reg_host_mapper_initial_guess"]


def lib_path() -> str:
    return _SO


def build_library(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 (cross-compiles without a GPU)."""
    src_dir = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", src_dir]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return _SO


_lib = None


def load_library():
    """Load the HIP extension; fails loudly when it has not been built (no fallback exists).

    Note: PyTorch-ROCm wheels bundle their own libamdhip64.so.7.  A process that uses BOTH torch (device buffers,
    torch.distributed) and this library must `import torch` first, so that one HIP runtime serves both."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise ImportError(f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the registration path.")
    lib = C.CDLL(_SO)
    vp, i64, f32p = C.c_void_p, C.c_int64, C.c_void_p
    lib.reg_create.argtypes = [C.POINTER(RegParams), C.POINTER(vp)]
    lib.reg_destroy.argtypes = [vp]
    lib.reg_last_error.argtypes = [vp]
    lib.reg_last_error.restype = C.c_char_p
    lib.reg_set_stream.argtypes = [vp, vp]
    lib.reg_debug_configure.argtypes = [vp, C.POINTER(RegDebugParams)]
    lib.reg_debug_halo_bound.argtypes = [vp, f32p, i64, f32p]
    lib.reg_debug_halo_witness.argtypes = [vp, f32p, i64, vp]
    lib.reg_debug_live_resources.argtypes = [C.POINTER(C.c_int64)]
    lib.reg_dist_get_unique_id.argtypes = [C.c_char_p]
    lib.reg_dist_init.argtypes = [vp, C.c_char_p, C.c_int, C.c_int]
    lib.reg_dist_init_custom.argtypes = [vp, C.POINTER(Collectives), C.c_int, C.c_int]
    lib.reg_dist_register.argtypes = [vp, f32p, f32p, C.POINTER(RegResult)]
    lib.reg_dist_shutdown.argtypes = [vp]
    lib.reg_dist_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.reg_dist_steer_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_int]
    lib.reg_dist_steer_create.restype = vp
    lib.reg_dist_steer_destroy.argtypes = [vp]
    lib.reg_dist_steer_destroy.restype = None
    lib.reg_dist_steer_step.argtypes = [vp, C.POINTER(DistReply)]
    lib.reg_dist_steer_step.restype = DistAction
    lib.reg_dist_steer_counts.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.reg_dist_steer_counts.restype = None
    lib.reg_set_source_f64.argtypes = [vp, vp, vp, vp, i64, C.c_int]
    lib.reg_set_target.argtypes = [vp, f32p, i64, f32p, i64, f32p, i64, C.c_int]
    lib.reg_set_source.argtypes = [vp, f32p, i64, f32p, i64, f32p, i64, C.c_int]
    lib.reg_register.argtypes = [vp, f32p, f32p, C.POINTER(RegResult)]
    lib.reg_compute.argtypes = [vp, f32p, i64, f32p, i64, f32p, i64, C.c_int, f32p, f32p, C.POINTER(RegResult)]
    lib.reg_prepare.argtypes = [vp, f32p]
    lib.reg_linearize.argtypes = [vp, f32p, f32p, f32p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.reg_get_correspondences.argtypes = [vp, vp, vp, vp]
    lib.reg_match_local.argtypes = [vp, f32p]
    lib.reg_trim_histogram.argtypes = [vp, C.c_int, C.c_uint32, vp]
    lib.reg_reduce_local.argtypes = [vp, f32p, C.c_float, vp]
    lib.reg_solve_update.argtypes = [C.POINTER(RegParams), vp, f32p, f32p, C.POINTER(C.c_int32)]
    lib.reg_host_solve6.argtypes = [f32p, f32p, f32p]
    lib.reg_host_solve6.restype = C.c_int
    lib.reg_host_x_to_T.argtypes = [f32p, f32p]
    lib.reg_host_solve6_xicp.argtypes = [f32p, f32p, vp, f32p]
    lib.reg_host_solve6_xicp.restype = C.c_int
    lib.reg_set_target_f64.argtypes = [vp, vp, vp, vp, i64, C.c_int, C.POINTER(RegCrop), C.POINTER(C.c_int64)]
    lib.reg_get_target_source_indices.argtypes = [vp, vp]
    lib.reg_carve_indices.argtypes = [vp, vp, vp, i64, vp, i64, C.c_int, C.POINTER(C.c_double), C.POINTER(RegCrop),
                                      C.c_double, C.c_double, C.c_double, C.c_double, vp, C.POINTER(C.c_int64)]
    lib.reg_voxelize_within_volume.argtypes = [vp, vp, vp, vp, i64, C.c_int, C.POINTER(RegCrop), C.c_double, vp, vp, vp,
                                               C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.reg_overlap_indices.argtypes = [vp, vp, i64, vp, i64, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_int32, vp,
                                        C.POINTER(C.c_int64), vp, C.POINTER(C.c_int64)]
    lib.reg_set_pair_overlap_f64.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, i64, C.c_int, C.POINTER(C.c_double), C.c_double,
                                             C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.reg_get_source_source_indices.argtypes = [vp, vp]
    lib.reg_compute_fpfh.argtypes = [vp, vp, i64, vp, i64, i64, C.c_int, C.c_int, C.c_float, vp, vp, vp, C.POINTER(C.c_int64)]
    lib.reg_match_features.argtypes = [vp, vp, i64, vp, i64, C.c_int, C.c_int, vp, vp, vp, C.POINTER(C.c_int64)]
    lib.reg_ransac_correspondences.argtypes = [vp, vp, i64, vp, i64, vp, i64, C.c_int, C.POINTER(RansacParams),
                                               C.POINTER(RansacResult), vp, vp]
    lib.reg_host_ransac_est_k.argtypes = [C.c_double, C.c_double, i64, i64, C.c_int32]
    lib.reg_host_ransac_est_k.restype = C.c_double
    lib.reg_voxel_down_sample.argtypes = [vp, vp, vp, vp, i64, C.c_int, C.c_double, vp, vp, vp, C.POINTER(C.c_int64)]
    lib.reg_random_down_sample.argtypes = [vp, vp, vp, vp, i64, C.c_int, C.c_double, C.c_uint64, vp, vp, vp, vp,
                                           C.POINTER(C.c_int64)]
    lib.reg_host_scan_key.argtypes = [C.c_uint64, C.c_uint64]
    lib.reg_host_scan_key.restype = C.c_uint64
    lib.reg_default_scan_params.argtypes = [C.POINTER(ScanParams)]
    lib.reg_default_scan_params.restype = None
    lib.reg_process_scan.argtypes = [vp, vp, vp, vp, i64, C.c_int, C.POINTER(ScanParams), vp, vp, vp, C.POINTER(ScanResult)]
    pd16, pi64 = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    lib.reg_dense_map_create.argtypes = [vp, C.c_double, C.POINTER(vp)]
    lib.reg_dense_map_destroy.argtypes = [vp]
    lib.reg_dense_map_destroy.restype = None
    lib.reg_dense_map_clear.argtypes = [vp]
    lib.reg_dense_map_insert.argtypes = [vp, vp, vp, vp, i64, C.c_int, pd16, pi64, pi64]
    lib.reg_default_dense_scan_params.argtypes = [C.POINTER(DenseScanParams)]
    lib.reg_default_dense_scan_params.restype = None
    lib.reg_dense_map_insert_scan.argtypes = [vp, vp, vp, vp, i64, C.c_int, C.POINTER(DenseScanParams), pd16, pi64, pi64]
    lib.reg_default_dense_carve_params.argtypes = [C.POINTER(DenseCarveParams)]
    lib.reg_default_dense_carve_params.restype = None
    lib.reg_dense_map_carve.argtypes = [vp, vp, i64, C.c_int, pd16, C.POINTER(DenseCarveParams), vp, pi64]
    lib.reg_dense_map_transform.argtypes = [vp, pd16]
    lib.reg_dense_map_center.argtypes = [vp, pd16]
    lib.reg_dense_map_get_info.argtypes = [vp, C.POINTER(DenseMapInfo)]
    lib.reg_dense_map_export.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, i64, pi64]
    lib.reg_dedup_voxels.argtypes = [vp, vp, i64, C.c_int, C.c_double, vp, pi64]
    lib.reg_host_dense_offsets.argtypes = [C.c_double, C.c_double, vp]
    lib.reg_host_dense_offsets.restype = C.c_int32
    lib.reg_default_map_cloud_params.argtypes = [C.POINTER(MapCloudParams)]
    lib.reg_default_map_cloud_params.restype = None
    lib.reg_map_cloud_create.argtypes = [vp, C.POINTER(MapCloudParams), C.POINTER(vp)]
    lib.reg_map_cloud_destroy.argtypes = [vp]
    lib.reg_map_cloud_destroy.restype = None
    lib.reg_map_cloud_clear.argtypes = [vp]
    lib.reg_map_cloud_get_info.argtypes = [vp, C.POINTER(MapCloudInfo)]
    lib.reg_map_cloud_set.argtypes = [vp, vp, vp, vp, i64, C.c_int, C.c_double]
    lib.reg_map_cloud_insert_scan.argtypes = [vp, vp, i64, vp, vp, vp, i64, C.c_int, pd16, C.c_int,
                                              C.POINTER(MapCloudInsertResult)]
    lib.reg_map_cloud_set_target.argtypes = [vp, C.POINTER(RegCrop), pi64]
    lib.reg_map_cloud_transform.argtypes = [vp, pd16]
    lib.reg_map_cloud_center.argtypes = [vp, pd16]
    lib.reg_map_cloud_export.argtypes = [vp, C.c_int, vp, vp, vp, i64, pi64]
    lib.reg_undistort_scan.argtypes = [vp, vp, i64, C.c_int, C.POINTER(UndistortParams), vp]
    lib.reg_host_undistort_point.argtypes = [pd16, C.POINTER(UndistortParams), pd16]
    lib.reg_get_source_count.argtypes = [vp, pi64]
    lib.reg_covariances_from_normals.argtypes = [vp, vp, i64, C.c_int, C.c_double, vp]
    lib.reg_host_covariance_from_normal.argtypes = [pd16, C.c_double, pd16]
    lib.reg_default_odometry_params.argtypes = [C.POINTER(OdometryParams)]
    lib.reg_default_odometry_params.restype = None
    lib.reg_check_odometry_params.argtypes = [C.POINTER(RegParams), C.POINTER(OdometryParams)]
    lib.reg_odometry_struct_sizes.argtypes = [C.POINTER(C.c_int32)]
    lib.reg_odometry_struct_sizes.restype = None
    lib.reg_odometry_create.argtypes = [vp, C.POINTER(OdometryParams), C.POINTER(vp)]
    lib.reg_odometry_destroy.argtypes = [vp]
    lib.reg_odometry_destroy.restype = None
    lib.reg_odometry_clear.argtypes = [vp]
    lib.reg_odometry_get_info.argtypes = [vp, C.POINTER(OdometryInfo)]
    lib.reg_odometry_set_initial_transform.argtypes = [vp, pd16, C.POINTER(C.c_int32)]
    lib.reg_odometry_add_scan.argtypes = [vp, vp, vp, i64, C.c_int, i64, C.POINTER(OdometryResult)]
    lib.reg_odometry_export_cloud.argtypes = [vp, C.c_int, vp, vp, vp, i64, pi64]
    lib.reg_odometry_get_correspondences.argtypes = [vp, i64, vp, vp]
    lib.reg_host_odometry_decide.argtypes = [C.c_int32, i64, i64, C.c_int32, i64, C.c_double, C.c_double, C.c_int32]
    lib.reg_host_odometry_decide.restype = C.c_int32
    lib.reg_host_odometry_accumulate.argtypes = [pd16, vp]
    lib.reg_default_pose_graph_params.argtypes = [C.POINTER(PoseGraphParams)]
    lib.reg_default_pose_graph_params.restype = None
    lib.reg_check_pose_graph_params.argtypes = [C.POINTER(PoseGraphParams)]
    lib.reg_pose_graph_struct_sizes.argtypes = [C.POINTER(C.c_int32)]
    lib.reg_pose_graph_struct_sizes.restype = None
    lib.reg_pose_graph_create.argtypes = [vp, C.POINTER(PoseGraphParams), C.POINTER(vp)]
    lib.reg_pose_graph_destroy.argtypes = [vp]
    lib.reg_pose_graph_destroy.restype = None
    lib.reg_pose_graph_clear.argtypes = [vp]
    lib.reg_pose_graph_set.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp, i64]
    lib.reg_pose_graph_linearize.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.reg_pose_graph_optimize.argtypes = [vp, C.POINTER(PoseGraphResult)]
    lib.reg_pose_graph_global_optimize.argtypes = [vp, C.POINTER(PoseGraphResult)]
    lib.reg_pose_graph_get.argtypes = [vp, i64, vp, i64, vp, vp, vp, pi64]
    lib.reg_pose_graph_get_edge_ids.argtypes = [vp, i64, vp]
    lib.reg_pose_graph_get_info.argtypes = [vp, C.POINTER(PoseGraphInfo)]
    lib.reg_host_pose_graph_edge.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.reg_host_pose_vector.argtypes = [vp, vp]
    lib.reg_host_pose_step.argtypes = [vp, vp, vp]
    lib.reg_host_line_process_weight.argtypes = [vp, i64, C.c_double, C.c_double, C.POINTER(C.c_double)]
    lib.reg_debug_spd_solve_f64.argtypes = [vp, i64, vp, vp, vp, C.POINTER(C.c_int32)]
    i32, pi32_ = C.c_int32, C.POINTER(C.c_int32)
    lib.reg_default_submaps_params.argtypes = [C.POINTER(SubmapsParams)]
    lib.reg_default_submaps_params.restype = None
    lib.reg_check_submaps_params.argtypes = [C.POINTER(SubmapsParams)]
    lib.reg_submaps_struct_sizes.argtypes = [pi32_]
    lib.reg_submaps_struct_sizes.restype = None
    lib.reg_submaps_create.argtypes = [vp, C.POINTER(SubmapsParams), C.POINTER(vp)]
    lib.reg_submaps_destroy.argtypes = [vp]
    lib.reg_submaps_destroy.restype = None
    lib.reg_submaps_get_info.argtypes = [vp, C.POINTER(SubmapsInfo)]
    lib.reg_submaps_get_submap_info.argtypes = [vp, i32, C.POINTER(SubmapInfo)]
    lib.reg_submaps_set_map_to_sensor.argtypes = [vp, pd16]
    lib.reg_submaps_insert_scan.argtypes = [vp, vp, i64, vp, vp, vp, i64, C.c_int, pd16, i64, C.POINTER(SubmapsInsertResult)]
    lib.reg_submaps_force_new_submap.argtypes = [vp, C.POINTER(SubmapsInsertResult)]
    lib.reg_default_submap_feature_params.argtypes = [C.POINTER(SubmapFeatureParams)]
    lib.reg_default_submap_feature_params.restype = None
    lib.reg_submaps_compute_features.argtypes = [vp, i32, C.c_double, C.POINTER(SubmapFeatureParams), C.c_int, vp, vp, vp, i64, pi64,
                                                 pi32_]
    lib.reg_submaps_get_keys.argtypes = [vp, i32, vp, i64, pi64]
    lib.reg_submaps_switch_fitness.argtypes = [vp, i32, vp, i64, C.c_int, pd16, pi64, C.POINTER(C.c_double)]
    lib.reg_submaps_set_target.argtypes = [vp, C.POINTER(RegCrop), pi64]
    lib.reg_submaps_export_submap.argtypes = [vp, i32, C.c_int, vp, vp, vp, i64, pi64]
    lib.reg_submaps_export.argtypes = [vp, C.c_int, vp, vp, vp, i64, pi64]
    lib.reg_submaps_transform.argtypes = [vp, vp, vp, i32]
    lib.reg_submaps_add_loop_closure_edges.argtypes = [vp, vp, vp, i32]
    lib.reg_submaps_get_adjacency.argtypes = [vp, vp, vp, i32]
    lib.reg_submaps_pop_finished.argtypes = [vp, vp, vp, i32, pi32_]
    lib.reg_submaps_pop_loop_closure_candidates.argtypes = [vp, vp, vp, i32, pi32_]
    lib.reg_submaps_push_loop_closure_candidate.argtypes = [vp, i32, i64]
    lib.reg_submaps_loop_closure_candidates.argtypes = [vp, i32, vp, i32, pi32_]
    lib.reg_submaps_odometry_constraint_pairs.argtypes = [vp, vp, i32, vp, i32, vp, i32, pi32_]
    lib.reg_host_submaps_decide.argtypes = [i32, i32, i32, i32, i64, i64, i32, C.c_double, C.c_double, C.c_double, i32, i32]
    lib.reg_host_submaps_decide.restype = i32
    lib.reg_host_adjacency_distance.argtypes = [vp, vp, i32, i32]
    lib.reg_host_adjacency_distance.restype = i32
    lib.reg_host_submaps_transform_plan.argtypes = [vp, i32, vp, i32, vp]
    lib.reg_host_mapper_initial_guess.argtypes = [pd16, pd16, pd16, pd16, pd16]
    lib.reg_host_centroid.argtypes = [f32p, i64, i64, f32p]
    lib.reg_host_o3d_update.argtypes = [C.c_int, vp, vp, C.POINTER(C.c_int32)]
    lib.reg_get_target_info.argtypes = [vp, C.POINTER(TargetInfo)]
    lib.reg_profile_kernels.argtypes = [vp, f32p, C.c_int, f32p]
    lib.reg_source_centroid_sums.argtypes = [vp, vp]
    lib.reg_prepare_centroid.argtypes = [vp, f32p, f32p]
    lib.reg_compose.argtypes = [vp, f32p, f32p]
    lib.reg_dist_begin.argtypes = [vp, f32p]
    lib.reg_dist_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.reg_dist_phase.argtypes = [vp, C.c_int]
    lib.reg_dist_finish.argtypes = [vp, f32p, C.POINTER(RegResult)]
    lib.reg_dist_fused_buffers.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)]
    lib.reg_dist_poll.argtypes = [vp, C.POINTER(DistStatus)]
    lib.reg_dist_record.argtypes = [vp, i64, C.POINTER(DistStatus)]
    lib.reg_dist_centroid_sums.argtypes = [vp, C.POINTER(vp)]
    lib.reg_dist_prepare.argtypes = [vp, f32p, i64]
    lib.reg_information_matrix.argtypes = [vp, f32p, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.reg_dist_xicp_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.reg_dist_gather_buffers.argtypes = [vp, C.c_int, i64, C.POINTER(vp), C.POINTER(vp)]
    lib.reg_smooth_normals.argtypes = [vp, vp, vp, i64, C.c_int, C.c_int, vp]
    lib.reg_estimate_normals.argtypes = [vp, vp, i64, i64, C.c_int, C.c_int, C.c_float, vp, C.c_int,
                                         C.POINTER(NormalsOut), C.POINTER(C.c_int64)]
    lib.reg_default_pm_chain.argtypes = [C.POINTER(PmChainV3)]   # writes sizeof(reg_pm_chain) bytes
    lib.reg_default_pm_chain.restype = None
    lib.reg_check_pm_chain.argtypes = [C.POINTER(RegParams), C.POINTER(PmChain)]
    lib.reg_set_pm_chain.argtypes = [vp, C.POINTER(PmChain)]
    lib.reg_get_robust_state.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    lib.reg_get_correspondences_k.argtypes = [vp, C.c_int32, vp, vp, vp]
    lib.reg_host_robust_weights.argtypes = [C.c_int32, C.c_float, C.c_float, C.c_float, vp, i64, vp]
    lib.reg_host_pm_p2p_update.argtypes = [vp, vp, C.POINTER(C.c_int32)]
    pf, pd, pi32 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.reg_get_covariance.argtypes = [vp, vp, pi32]
    lib.reg_get_covariance_sums.argtypes = [vp, vp, vp]
    lib.reg_host_censi_covariance.argtypes = [vp, vp, C.c_float, vp, pi32]
    lib.reg_get_minimizer_stats.argtypes = [vp, C.POINTER(MinimizerStats)]
    lib.reg_get_degeneracy.argtypes = [vp, vp, vp, pf]
    lib.reg_get_bound.argtypes = [vp, pf, pf]
    lib.reg_host_solution_remap.argtypes = [vp, C.c_float, C.c_int, vp, vp, vp, vp]
    lib.reg_default_ternary_xicp.argtypes = [C.POINTER(TernaryXicp)]
    lib.reg_default_ternary_xicp.restype = None
    lib.reg_check_ternary_xicp.argtypes = [C.POINTER(RegParams), vp, C.POINTER(TernaryXicp)]
    lib.reg_set_ternary_xicp.argtypes = [vp, C.POINTER(TernaryXicp)]
    lib.reg_get_ternary_xicp.argtypes = [vp, C.POINTER(TernaryXicpResult)]
    lib.reg_host_ternary_decide.argtypes = [vp, vp, vp, vp, i64, C.POINTER(TernaryXicp), vp, pi32]
    lib.reg_host_partial_constraint.argtypes = [vp, vp, pf]
    lib.reg_host_solve6_xicp_rhs.argtypes = [f32p, f32p, vp, f32p, f32p]
    lib.reg_host_solve6_xicp_rhs.restype = C.c_int
    lib.reg_get_var_trim.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.reg_host_var_trim.argtypes = [vp, i64, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_float),
                                      C.POINTER(C.c_float)]
    lib.reg_default_ssn_params.argtypes = [C.POINTER(SsnParams)]
    lib.reg_default_ssn_params.restype = None
    lib.reg_sampling_surface_normal.argtypes = [vp, vp, i64, i64, C.c_int, C.POINTER(SsnParams), C.POINTER(SsnOut),
                                                C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.reg_filter_points.argtypes = [vp, vp, i64, vp, vp, i64, C.c_int, vp, C.c_int, vp, vp, vp, vp,
                                      C.POINTER(C.c_int64)]
    lib.reg_filter_cloud.argtypes = [vp, vp, i64, i64, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.POINTER(C.c_int64)]
    lib.reg_host_glibc_rand.argtypes = [C.c_uint32, i64, vp]
    lib.reg_default_voxel_grid_params.argtypes = [C.POINTER(VoxelGridParams)]
    lib.reg_default_voxel_grid_params.restype = None
    lib.reg_voxel_grid.argtypes = [vp, vp, i64, i64, C.c_int, vp, C.c_int, C.POINTER(VoxelGridParams), vp, vp,
                                   C.POINTER(C.c_int64)]
    lib.reg_default_octree_params.argtypes = [C.POINTER(OctreeParams)]
    lib.reg_default_octree_params.restype = None
    lib.reg_octree_grid.argtypes = [vp, vp, i64, vp, vp, i64, C.c_int, C.POINTER(OctreeParams), C.POINTER(OctreeOut),
                                    C.POINTER(C.c_int64)]
    lib.reg_host_octree_root.argtypes = [vp, vp, C.c_int, vp, C.POINTER(C.c_float)]
    lib.reg_host_octree_root.restype = None
    lib.reg_host_octree_random_picks.argtypes = [vp, i64, vp]
    for name in EXPORTS:
        getattr(lib, name)  # AttributeError if the library does not export what the header declares
    _lib = lib
    return lib


def live_resources() -> tuple:
    """reg_debug_live_resources: (device buffers, their bytes, pinned host blocks, events + owned streams) that the library
    holds in this process, all handles together."""
    out = (C.c_int64 * 4)()
    st = load_library().reg_debug_live_resources(out)
    if st != 0:
        raise RegError(st)
    return tuple(out)


def default_params() -> RegParams:
    p = RegParams()
    load_library().reg_default_params(C.byref(p))
    return p


def shipped_params() -> RegParams:
    p = RegParams()
    load_library().reg_shipped_params(C.byref(p))
    return p


class DeviceArray:
    """Device memory of the HIP runtime the library itself runs on (hipMalloc / hipFree of the libamdhip64 it loaded):
    lets the filters hand their results to reg_set_target / reg_set_source without a host round trip."""

    def __init__(self, nbytes: int):
        load_library()
        self._hip = C.CDLL("libamdhip64.so.7")   # already loaded by the library: the same runtime instance
        self._hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self._hip.hipFree.argtypes = [C.c_void_p]
        self._hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.ptr = C.c_void_p()
        self.nbytes = max(int(nbytes), 16)
        if self._hip.hipMalloc(C.byref(self.ptr), self.nbytes) != 0:
            self.ptr = C.c_void_p()
            raise RegError(8, f"hipMalloc({self.nbytes}) failed")

    @property
    def value(self) -> int:
        return int(self.ptr.value or 0)

    def upload(self, a: np.ndarray):
        a = np.ascontiguousarray(a)
        if a.nbytes > self.nbytes or self._hip.hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1) != 0:
            raise RegError(8, "hipMemcpy (host to device) failed")

    def download(self, shape, dtype=np.float32) -> np.ndarray:
        out = np.empty(shape, dtype)
        if out.nbytes > self.nbytes or self._hip.hipMemcpy(out.ctypes.data, self.ptr, out.nbytes, 2) != 0:
            raise RegError(8, "hipMemcpy (device to host) failed")
        return out

    def free(self):
        if self.ptr.value:
            self._hip.hipFree(self.ptr)
        self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def download(ptr: int, shape, dtype=np.float32) -> np.ndarray:
    """Copies a device array that starts at the raw pointer `ptr` to the host."""
    out = np.empty(shape, dtype)
    if out.nbytes:
        hip = C.CDLL("libamdhip64.so.7")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        if hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) != 0:
            raise RegError(8, "hipMemcpy (device to host) failed")
    return out


def default_ssn_params() -> SsnParams:
    p = SsnParams()
    load_library().reg_default_ssn_params(C.byref(p))
    return p


def default_octree_params(**kw) -> OctreeParams:
    """reg_octree_params at OctreeGrid.h's defaults; `kw` sets fields."""
    p = OctreeParams()
    load_library().reg_default_octree_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def host_octree_root(lo, hi, center_at_origin=True):
    """reg_host_octree_root: (centre float32[3], radius float32) of the octree's root box from per-axis min / max."""
    lo, hi = _f32(np.reshape(lo, 3)), _f32(np.reshape(hi, 3))
    c, r = np.zeros(3, np.float32), C.c_float(0)
    load_library().reg_host_octree_root(_ptr(lo), _ptr(hi), int(bool(center_at_origin)), _ptr(c), C.byref(r))
    return c, np.float32(r.value)


def host_octree_random_picks(sizes) -> np.ndarray:
    """reg_host_octree_random_picks: RandomPtsSampler's member position per leaf (glibc rand() after srand(1))."""
    sz = np.ascontiguousarray(sizes, np.int64)
    picks = np.zeros(sz.size, np.int64)
    st = load_library().reg_host_octree_random_picks(_ptr(sz), sz.size, _ptr(picks))
    if st != 0:
        raise RegError(st, "reg_host_octree_random_picks: leaf sizes must be >= 1")
    return picks


def default_pm_chain_v3() -> PmChainV3:
    """reg_default_pm_chain: knn 1, point-to-plane, every module of the chain off (the plain loop); their parameters at
    the reference's defaults."""
    c = PmChainV3()
    load_library().reg_default_pm_chain(C.byref(c))
    return c


def default_pm_chain() -> PmChain:
    """The same defaults in the struct up to `var_lambda` (struct_size = REG_PM_CHAIN_SIZE_V2): knn 1, point-to-plane,
    robust / MinDist / MedianDist / VarTrimmedDist off.  A chain of this size cannot switch the later modules on."""
    full = default_pm_chain_v3()
    c = PmChain()
    C.memmove(C.byref(c), C.byref(full), C.sizeof(PmChain))
    c.struct_size = C.sizeof(PmChain)
    return c


def check_pm_chain(params: RegParams, chain: PmChain) -> int:
    """reg_check_pm_chain status (0 = accepted) -- pure, no device."""
    return int(load_library().reg_check_pm_chain(C.byref(params), C.byref(chain)))


def default_ternary_xicp(enabled=False) -> TernaryXicp:
    """reg_default_ternary_xicp: the shipped yaml's commented EqualityConstraints values (250, 180, 35; 80, 45 degrees)."""
    t = TernaryXicp()
    load_library().reg_default_ternary_xicp(C.byref(t))
    t.enabled = 1 if enabled else 0
    return t


def check_ternary_xicp(params: RegParams, chain, ternary: TernaryXicp) -> int:
    """reg_check_ternary_xicp status (0 = accepted) -- pure, no device.  chain None: the default chain."""
    return int(load_library().reg_check_ternary_xicp(C.byref(params), C.byref(chain) if chain is not None else None,
                                                     C.byref(ternary)))


def host_ternary_decide(combined, high, n_combined, n_high, n_pairs, params: TernaryXicp):
    """reg_host_ternary_decide: (categories int32[6], sane bool) -- the device's decision on the host."""
    c, h = np.ascontiguousarray(combined, np.float64).reshape(6), np.ascontiguousarray(high, np.float64).reshape(6)
    nc, nh = np.ascontiguousarray(n_combined, np.int64).reshape(6), np.ascontiguousarray(n_high, np.int64).reshape(6)
    cat, sane = np.zeros(6, np.int32), C.c_int32()
    st = load_library().reg_host_ternary_decide(_ptr(c), _ptr(h), _ptr(nc), _ptr(nh), int(n_pairs), C.byref(params), _ptr(cat),
                                                C.byref(sane))
    if st != 0:
        raise RegError(st, "reg_host_ternary_decide")
    return cat, bool(sane.value)


def host_partial_constraint(sums9, v):
    """reg_host_partial_constraint: (value float32, finite bool) of one partial direction from its nine sums and its
    eigenvector in the optimisation frame -- the device's code on the host."""
    s = np.ascontiguousarray(sums9, np.float64).reshape(9)
    vv = np.ascontiguousarray(v, np.float32).reshape(3)
    val = C.c_float()
    st = load_library().reg_host_partial_constraint(_ptr(s), _ptr(vv), C.byref(val))
    if st not in (0, 3):
        raise RegError(st, "reg_host_partial_constraint")
    return np.float32(val.value), st == 0


def host_solve6_xicp_rhs(A, b, flags, rhs):
    """reg_host_solve6_xicp_rhs: (x float32[6], rank) with right-hand sides on the constraint rows."""
    f = np.ascontiguousarray(flags, np.int32).reshape(6)
    r = np.ascontiguousarray(rhs, np.float32).reshape(6)
    x = np.zeros(6, np.float32)
    rank = load_library().reg_host_solve6_xicp_rhs(_ptr(np.ascontiguousarray(A, np.float32).reshape(36)),
                                                   _ptr(np.ascontiguousarray(b, np.float32).reshape(6)), _ptr(f), _ptr(r), _ptr(x))
    return x, int(rank)


def host_robust_weights(fct, tuning, scale, d2, approximation=math.inf):
    """RobustOutlierFilter weights of squared distances d2 (fp32, the device's code): fct is a name or REG_ROBUST_*."""
    fid = ROBUST_FCTS[fct] if isinstance(fct, str) else int(fct)
    d = np.ascontiguousarray(d2, np.float32).reshape(-1)
    w = np.empty_like(d)
    st = load_library().reg_host_robust_weights(fid, float(tuning), float(scale), float(approximation), _ptr(d), d.size,
                                                _ptr(w))
    if st != 0:
        raise RegError(st, "reg_host_robust_weights")
    return w


def host_var_trim(d2, min_ratio=0.05, max_ratio=0.99, lam=2.35):
    """reg_host_var_trim: (k, optRatio, limit) of VarTrimmedDistOutlierFilter for the squared distances d2 (any shape;
    +inf = no match), the contract of include/o3dslam_reg.h evaluated on the host."""
    d = np.ascontiguousarray(d2, np.float32).reshape(-1)
    k, ratio, limit = C.c_int64(), C.c_float(), C.c_float()
    st = load_library().reg_host_var_trim(_ptr(d), d.size, float(min_ratio), float(max_ratio), float(lam), C.byref(k),
                                          C.byref(ratio), C.byref(limit))
    if st != 0:
        raise RegError(st, "reg_host_var_trim")
    return int(k.value), float(ratio.value), float(limit.value)


def _pack_sym6(A) -> np.ndarray:
    """Upper triangle of a 6x6 matrix, row by row (the layout of the covariance sums)."""
    A = np.asarray(A, np.float64).reshape(6, 6)
    return np.ascontiguousarray(A[np.triu_indices(6)])


def unpack_sym6(v) -> np.ndarray:
    """The symmetric 6x6 matrix of 21 packed upper-triangle values."""
    A = np.zeros((6, 6), np.float64)
    A[np.triu_indices(6)] = np.asarray(v, np.float64).reshape(21)
    return A + np.triu(A, 1).T


def host_censi_covariance(H, M, sigma=0.01):
    """reg_host_censi_covariance: (cov float32 6x6 [x y z alpha beta gamma], rank of H) from the sums H = sum v v^T and
    M = sum (a a^T + b b^T), given as 6x6 matrices or as 21 packed values -- the device's code on the host."""
    Hp = _pack_sym6(H) if np.size(H) == 36 else np.ascontiguousarray(H, np.float64).reshape(21)
    Mp = _pack_sym6(M) if np.size(M) == 36 else np.ascontiguousarray(M, np.float64).reshape(21)
    cov = np.zeros(36, np.float32)
    rank = C.c_int32()
    st = load_library().reg_host_censi_covariance(_ptr(Hp), _ptr(Mp), float(sigma), _ptr(cov), C.byref(rank))
    if st != 0:
        raise RegError(st, "reg_host_censi_covariance")
    return cov.reshape(6, 6), int(rank.value)


def host_solution_remap(A, threshold, use2019=False, P_in=None):
    """reg_host_solution_remap: one SolutionRemapping step on the fp32 normal matrix A with the projector P_in in force
    (None: the identity).  Returns (P_out float64 6x6, categories int32[6], eigenvalues float32[6] descending,
    return_prior bool)."""
    a = np.ascontiguousarray(A, np.float32).reshape(36)
    pin = np.ascontiguousarray(np.eye(6) if P_in is None else P_in, np.float64).reshape(36)
    pout = np.zeros(36, np.float64)
    cat, eig = np.zeros(6, np.int32), np.zeros(6, np.float32)
    st = load_library().reg_host_solution_remap(_ptr(a), float(threshold), int(bool(use2019)), _ptr(pin), _ptr(pout),
                                                _ptr(cat), _ptr(eig))
    if st not in (0, 3):
        raise RegError(st, "reg_host_solution_remap")
    return pout.reshape(6, 6), cat, eig, st == 3


def host_pm_p2p_update(sums):
    """Point-to-point update dT (4x4 float64, math layout; T_iter <- dT T_iter) and rank from the chain's 32 sums."""
    s = np.ascontiguousarray(sums, np.float64).reshape(32)
    U = np.zeros(16, np.float64)
    rank = C.c_int32()
    st = load_library().reg_host_pm_p2p_update(_ptr(s), _ptr(U), C.byref(rank))
    if st != 0:
        raise RegError(st, "reg_host_pm_p2p_update")
    return U.reshape(4, 4).T.copy(), rank.value


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _T_in(T):
    """numpy 4x4 (math layout) -> column-major float[16] as the ABI wants (== Eigen::Matrix4f::data())."""
    T = np.asarray(T, dtype=np.float32).reshape(4, 4)
    return np.ascontiguousarray(T.T).reshape(16)


def _T_in_f64(T):
    """numpy 4x4 (math layout) -> column-major double[16] (== Eigen::Matrix4d::data()); None stays NULL (identity)."""
    if T is None:
        return None
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    return (C.c_double * 16)(*T.T.reshape(16))


def _T_out(buf):
    return np.array(buf, dtype=np.float32).reshape(4, 4).T.copy()


class Registration:
    """One registration context (== one reg_handle)."""

    def __init__(self, params: RegParams | None = None, **overrides):
        self._lib = load_library()
        p = params if params is not None else default_params()
        for k, v in overrides.items():
            if not hasattr(p, k):
                raise TypeError(f"unknown parameter {k}")
            setattr(p, k, v)
        p.struct_size = C.sizeof(RegParams)
        self.params = p
        self._h = C.c_void_p()
        st = self._lib.reg_create(C.byref(p), C.byref(self._h))
        if st != 0:
            msg = self._lib.reg_last_error(self._h).decode() if self._h else "reg_create rejected the parameters"
            if self._h:
                self._lib.reg_destroy(self._h)
                self._h = C.c_void_p()
            raise RegError(st, msg)
        dbg = {k: int(getattr(p, k, 0)) for k in _DEBUG_FIELDS}
        if any(dbg.values()):
            self.debug_configure(**dbg)
        self._keep = []
        self.n_source = 0

    def close(self):
        if getattr(self, "_h", None):
            for m in list(getattr(self, "_dense_maps", ())):   # a reg_dense_map is destroyed before its handle
                m.close()
            for m in list(getattr(self, "_map_clouds", ())):   # and so is a reg_map_cloud
                m.close()
            for m in list(getattr(self, "_odometries", ())):   # and a reg_odometry
                m.close()
            for m in list(getattr(self, "_pose_graphs", ())):  # and a reg_pose_graph
                m.close()
            for m in list(getattr(self, "_submaps", ())):      # and a reg_submaps
                m.close()
            self._lib.reg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            raise RegError(st, self._lib.reg_last_error(self._h).decode())

    def last_error(self) -> str:
        """reg_last_error: the message of the last failing call on this handle."""
        return self._lib.reg_last_error(self._h).decode()

    def debug_configure(self, **switches):
        """reg_debug_configure: the experiment switches of include/o3dslam_reg_debug.h; those not named are zero."""
        dbg = RegDebugParams()
        dbg.struct_size = C.sizeof(RegDebugParams)
        for k, v in switches.items():
            if k not in _DEBUG_FIELDS:
                raise TypeError(f"unknown debug switch {k}")
            setattr(dbg, k, int(v))
        self._check(self._lib.reg_debug_configure(self._h, C.byref(dbg)))

    def set_stream(self, hip_stream: int):
        self._check(self._lib.reg_set_stream(self._h, C.c_void_p(hip_stream)))

    # ---- host (numpy) entry points ------------------------------------------------------------
    def set_target(self, xyz, normals=None, covs=None):
        xyz = _f32(xyz)
        nrm = _f32(normals) if normals is not None else None
        cov = _f32(covs) if covs is not None else None
        m = xyz.shape[0] if xyz.ndim == 2 else 0
        self._check(self._lib.reg_set_target(self._h, _ptr(xyz), xyz.shape[1] if xyz.ndim == 2 else 3, _ptr(nrm),
                                             nrm.shape[1] if nrm is not None else 3, _ptr(cov), m, 0))

    def set_target_f64(self, xyz, normals=None, covs=None, crop=None):
        """Target-side preparation on the device (croppers.cpp:76-170 + open3d_conversions.cpp:57-118): fp64 AoS cloud,
        optional cropping volume `crop` = dict(type=, center=, radius_min=, radius_max=, min_z=, max_z=).
        Returns the number of points kept."""
        x = np.ascontiguousarray(xyz, np.float64)
        nr = np.ascontiguousarray(normals, np.float64) if normals is not None else None
        cv = np.ascontiguousarray(covs, np.float64).reshape(-1, 9) if covs is not None else None
        c = self._crop_struct(crop)
        kept = C.c_int64(0)
        st = self._lib.reg_set_target_f64(self._h, _ptr(x), _ptr(nr), _ptr(cv), x.shape[0] if x.ndim == 2 else 0, 0,
                                          C.byref(c) if c is not None else None, C.byref(kept))
        self.n_target_kept = int(kept.value)
        self._check(st)
        return self.n_target_kept

    def set_target_f64_device(self, xyz_ptr, m, nrm_ptr=None, cov_ptr=None, crop=None):
        """As set_target_f64 with the fp64 cloud already resident in HBM (m x 3 doubles; normals m x 3; covs m x 9)."""
        c = self._crop_struct(crop)
        kept = C.c_int64(0)
        st = self._lib.reg_set_target_f64(self._h, C.c_void_p(xyz_ptr), C.c_void_p(nrm_ptr) if nrm_ptr else None,
                                          C.c_void_p(cov_ptr) if cov_ptr else None, m, 1,
                                          C.byref(c) if c is not None else None, C.byref(kept))
        self.n_target_kept = int(kept.value)
        self._check(st)
        return self.n_target_kept

    @staticmethod
    def _crop_struct(crop):
        if crop is None:
            return None
        c = RegCrop()
        c.type = int(crop.get("type", CROP_NONE))
        for k in range(3):
            c.center[k] = float(crop.get("center", (0, 0, 0))[k])
        c.radius_min = float(crop.get("radius_min", 0.0))
        c.radius_max = float(crop.get("radius_max", 0.0))
        c.min_z, c.max_z = float(crop.get("min_z", 0.0)), float(crop.get("max_z", 0.0))
        return c

    def voxelize_within_volume(self, xyz, voxel_size, volume=None, normals=None, covs=None):
        """voxelizeWithinCroppingVolume (helpers.cpp:117-192) on the device.  Returns (xyz, normals, covs, n_outside):
        the first n_outside rows are the untouched points outside `volume`, the rest one averaged point per voxel."""
        x = np.ascontiguousarray(xyz, np.float64)
        m = x.shape[0]
        nr = np.ascontiguousarray(normals, np.float64) if normals is not None else None
        cv = np.ascontiguousarray(covs, np.float64).reshape(-1, 9) if covs is not None else None
        ox = np.empty((m, 3), np.float64)
        on = np.empty((m, 3), np.float64) if nr is not None else None
        oc = np.empty((m, 9), np.float64) if cv is not None else None
        c = self._crop_struct(volume)
        n_out, n_outside = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.reg_voxelize_within_volume(self._h, _ptr(x), _ptr(nr), _ptr(cv), m, 0,
                                                         C.byref(c) if c is not None else None, float(voxel_size), _ptr(ox),
                                                         _ptr(on), _ptr(oc), C.byref(n_out), C.byref(n_outside)))
        k = int(n_out.value)
        return ox[:k], (on[:k] if on is not None else None), (oc[:k] if oc is not None else None), int(n_outside.value)

    def carve_indices(self, map_xyz, scan_xyz, sensor, voxel_size=0.1, max_ray=20.0, truncation=0.1, min_dot=0.5,
                      map_normals=None, subset=None):
        """Space carving (helpers.cpp:238-283): ascending indices of the map points to remove."""
        mp = np.ascontiguousarray(map_xyz, np.float64)
        sp = np.ascontiguousarray(scan_xyz, np.float64)
        nr = np.ascontiguousarray(map_normals, np.float64) if map_normals is not None else None
        out = np.empty(max(mp.shape[0], 1), np.int32)
        sen = (C.c_double * 3)(*[float(v) for v in sensor])
        c = self._crop_struct(subset)
        n = C.c_int64(0)
        self._check(self._lib.reg_carve_indices(self._h, _ptr(mp), _ptr(nr), mp.shape[0], _ptr(sp), sp.shape[0], 0, sen,
                                                C.byref(c) if c is not None else None, float(voxel_size), float(max_ray),
                                                float(truncation), float(min_dot), _ptr(out), C.byref(n)))
        return out[:int(n.value)].copy()

    def voxelize_within_volume_device(self, xyz_ptr, m, voxel_size, out_xyz_ptr, volume=None, nrm_ptr=None, cov_ptr=None,
                                      out_nrm_ptr=None, out_cov_ptr=None):
        """As voxelize_within_volume with the fp64 cloud and the fp64 outputs (capacity m rows each: x 3, normals x 3,
        covs x 9) resident in HBM; the kernels write the outputs in place.  Returns (n_out, n_outside)."""
        vp = lambda p: C.c_void_p(p) if p else None
        c = self._crop_struct(volume)
        n_out, n_outside = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.reg_voxelize_within_volume(self._h, vp(xyz_ptr), vp(nrm_ptr), vp(cov_ptr), m, 1,
                                                         C.byref(c) if c is not None else None, float(voxel_size),
                                                         vp(out_xyz_ptr), vp(out_nrm_ptr), vp(out_cov_ptr), C.byref(n_out),
                                                         C.byref(n_outside)))
        return int(n_out.value), int(n_outside.value)

    def carve_indices_device(self, map_ptr, m, scan_ptr, n_scan, sensor, removed_ptr, voxel_size=0.1, max_ray=20.0,
                             truncation=0.1, min_dot=0.5, map_nrm_ptr=None, subset=None):
        """As carve_indices with the fp64 map (m x 3; normals m x 3), the fp64 scan (n_scan x 3) and the int32 output
        (capacity m) resident in HBM.  Returns n_removed."""
        vp = lambda p: C.c_void_p(p) if p else None
        sen = (C.c_double * 3)(*[float(v) for v in sensor])
        c = self._crop_struct(subset)
        n = C.c_int64(0)
        self._check(self._lib.reg_carve_indices(self._h, vp(map_ptr), vp(map_nrm_ptr), m, vp(scan_ptr), n_scan, 1, sen,
                                                C.byref(c) if c is not None else None, float(voxel_size), float(max_ray),
                                                float(truncation), float(min_dot), vp(removed_ptr), C.byref(n)))
        return int(n.value)

    # ---- the scan front end ----
    def voxel_down_sample(self, xyz, voxel_size, normals=None, covs=None):
        """PointCloud::VoxelDownSample on the device.  Returns (xyz, normals, covs): one averaged row per occupied voxel,
        in ascending (z, y, x) voxel index; averaged normals are not re-normalised."""
        x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        n = x.shape[0]
        nr = np.ascontiguousarray(normals, np.float64).reshape(-1, 3) if normals is not None else None
        cv = np.ascontiguousarray(covs, np.float64).reshape(-1, 9) if covs is not None else None
        ox = np.empty((n, 3), np.float64)
        on = np.empty((n, 3), np.float64) if nr is not None else None
        oc = np.empty((n, 9), np.float64) if cv is not None else None
        n_out = C.c_int64(0)
        self._check(self._lib.reg_voxel_down_sample(self._h, _ptr(x), _ptr(nr), _ptr(cv), n, 0, float(voxel_size), _ptr(ox),
                                                    _ptr(on), _ptr(oc), C.byref(n_out)))
        k = int(n_out.value)
        return ox[:k], (on[:k] if on is not None else None), (oc[:k] if oc is not None else None)

    def voxel_down_sample_device(self, xyz_ptr, n, voxel_size, out_xyz_ptr, nrm_ptr=None, cov_ptr=None, out_nrm_ptr=None,
                                 out_cov_ptr=None):
        """As voxel_down_sample with the fp64 cloud and the fp64 outputs (n rows each) resident in HBM.  Returns n_out."""
        vp = lambda p: C.c_void_p(p) if p else None
        n_out = C.c_int64(0)
        self._check(self._lib.reg_voxel_down_sample(self._h, vp(xyz_ptr), vp(nrm_ptr), vp(cov_ptr), n, 1, float(voxel_size),
                                                    vp(out_xyz_ptr), vp(out_nrm_ptr), vp(out_cov_ptr), C.byref(n_out)))
        return int(n_out.value)

    def random_down_sample(self, n, ratio, seed=0, xyz=None, normals=None, covs=None):
        """PointCloud::RandomDownSample under the determinism contract of the header.  Returns (idx, xyz, normals, covs):
        the ascending kept indices among `n` points and the kept rows of the arrays that were given."""
        f64 = lambda a, w: np.ascontiguousarray(a, np.float64).reshape(-1, w) if a is not None else None
        x, nr, cv = f64(xyz, 3), f64(normals, 3), f64(covs, 9)
        n = int(n)
        out = [np.empty((n, w), np.float64) if a is not None else None for a, w in ((x, 3), (nr, 3), (cv, 9))]
        idx = np.empty(max(n, 1), np.int32)
        n_out = C.c_int64(0)
        self._check(self._lib.reg_random_down_sample(self._h, _ptr(x), _ptr(nr), _ptr(cv), n, 0, float(ratio), int(seed),
                                                     _ptr(idx), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), C.byref(n_out)))
        k = int(n_out.value)
        return (idx[:k].copy(),) + tuple(a[:k] if a is not None else None for a in out)

    def random_down_sample_device(self, n, ratio, seed, idx_ptr, xyz_ptr=None, nrm_ptr=None, cov_ptr=None, out_xyz_ptr=None,
                                  out_nrm_ptr=None, out_cov_ptr=None):
        """As random_down_sample with the int32 index output and the fp64 arrays resident in HBM.  Returns n_out."""
        vp = lambda p: C.c_void_p(p) if p else None
        n_out = C.c_int64(0)
        self._check(self._lib.reg_random_down_sample(self._h, vp(xyz_ptr), vp(nrm_ptr), vp(cov_ptr), n, 1, float(ratio),
                                                     int(seed), vp(idx_ptr), vp(out_xyz_ptr), vp(out_nrm_ptr),
                                                     vp(out_cov_ptr), C.byref(n_out)))
        return int(n_out.value)

    def process_scan(self, xyz, params: "ScanParams", normals=None, covs=None):
        """processForScanMatchingAndMerging (ScanToMapRegistration.cpp:57-69) on the device: returns (merge_xyz,
        merge_normals, merge_covs, result) and leaves the narrow-cropped match cloud installed as the reading;
        source_source_indices() maps its rows to merge-cloud rows.  A failing status raises; `last_scan` keeps the counts."""
        x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        n = x.shape[0]
        nr = np.ascontiguousarray(normals, np.float64).reshape(-1, 3) if normals is not None else None
        cv = np.ascontiguousarray(covs, np.float64).reshape(-1, 9) if covs is not None else None
        ox, on, oc = np.empty((n, 3), np.float64), np.empty((n, 3), np.float64), np.empty((n, 9), np.float64)
        res = self._process_scan(_ptr(x), _ptr(nr), _ptr(cv), n, 0, params, _ptr(ox), _ptr(on), _ptr(oc))
        k = int(res.n_merge)
        return ox[:k], (on[:k] if res.has_normals else None), (oc[:k] if res.has_covs else None), res

    def process_scan_device(self, xyz_ptr, n, params: "ScanParams", merge_xyz_ptr, nrm_ptr=None, cov_ptr=None,
                            merge_nrm_ptr=None, merge_cov_ptr=None):
        """As process_scan with the fp64 scan and the fp64 merge-cloud outputs (n rows each) resident in HBM.  Returns the
        ScanResult."""
        vp = lambda p: C.c_void_p(p) if p else None
        return self._process_scan(vp(xyz_ptr), vp(nrm_ptr), vp(cov_ptr), n, 1, params, vp(merge_xyz_ptr), vp(merge_nrm_ptr),
                                  vp(merge_cov_ptr))

    def _process_scan(self, x, nr, cv, n, on_device, params, ox, on, oc):
        params.struct_size = C.sizeof(ScanParams)
        res = ScanResult()
        res.struct_size = C.sizeof(ScanResult)
        st = self._lib.reg_process_scan(self._h, x, nr, cv, n, on_device, C.byref(params), ox, on, oc, C.byref(res))
        self.last_scan = res
        # n_source_kept sizes source_source_indices(), as after set_pair_overlap_f64
        self.n_source_kept = int(res.n_match) if st == 0 else 0
        self.n_source = self.n_source_kept
        self._check(st)
        return res

    # ---- motion compensation of a raw scan ----
    def undistort_scan(self, xyz, params: "UndistortParams"):
        """reg_undistort_scan: ConstantVelocityMotionCompensation::undistortInputPointCloud for given velocities; n x 3 fp64."""
        x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        out = np.empty_like(x)
        self._check(self._lib.reg_undistort_scan(self._h, _ptr(x), x.shape[0], 0, C.byref(params), _ptr(out)))
        return out

    def undistort_scan_device(self, xyz_ptr, n, params: "UndistortParams", out_xyz_ptr):
        """As undistort_scan with the fp64 arrays resident in HBM (out_xyz_ptr may be xyz_ptr)."""
        self._check(self._lib.reg_undistort_scan(self._h, C.c_void_p(xyz_ptr) if xyz_ptr else None, n, 1, C.byref(params),
                                                 C.c_void_p(out_xyz_ptr) if out_xyz_ptr else None))

    # ---- GICP covariances from normals ----
    def covariances_from_normals(self, normals, epsilon=1e-3):
        """reg_covariances_from_normals: what Open3D's GeneralizedICP derives for a cloud with normals and no covariances;
        n x 3 fp64 normals (not normalised here) -> n x 9 fp64, the covariances_ layout of set_*_f64."""
        nr = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
        out = np.empty((nr.shape[0], 9), np.float64)
        self._check(self._lib.reg_covariances_from_normals(self._h, _ptr(nr), nr.shape[0], 0, float(epsilon), _ptr(out)))
        return out

    def covariances_from_normals_device(self, nrm_ptr, n, out_cov_ptr, epsilon=1e-3):
        """As covariances_from_normals with the fp64 arrays (n x 3 in, n x 9 out) resident in HBM."""
        self._check(self._lib.reg_covariances_from_normals(self._h, C.c_void_p(nrm_ptr) if nrm_ptr else None, n, 1,
                                                           float(epsilon), C.c_void_p(out_cov_ptr) if out_cov_ptr else None))

    # ---- the dense map: maps are DenseMap objects on this handle ----
    def dedup_voxels(self, xyz, voxel_size):
        """removeDuplicatePointsWithinSameVoxels (Voxel.cpp:162-191) on the device: the ascending indices of the
        lowest-index point of every voxel, key floor(p * (1 / voxel_size))."""
        x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        idx = np.empty(max(x.shape[0], 1), np.int32)
        n = C.c_int64(0)
        self._check(self._lib.reg_dedup_voxels(self._h, _ptr(x), x.shape[0], 0, float(voxel_size), _ptr(idx), C.byref(n)))
        return idx[:int(n.value)].copy()

    def dedup_voxels_device(self, xyz_ptr, n, voxel_size, idx_ptr) -> int:
        """As dedup_voxels with the fp64 cloud and the int32 output (capacity n) resident in HBM.  Returns n_kept."""
        k = C.c_int64(0)
        self._check(self._lib.reg_dedup_voxels(self._h, C.c_void_p(xyz_ptr) if xyz_ptr else None, n, 1, float(voxel_size),
                                               C.c_void_p(idx_ptr) if idx_ptr else None, C.byref(k)))
        return int(k.value)

    def target_source_indices(self):
        idx = np.empty(self.n_target_kept, np.int32)
        self._check(self._lib.reg_get_target_source_indices(self._h, _ptr(idx)))
        return idx

    # ---- voxel overlap of two clouds / the submap-pair front of the constraint builders ----
    def overlap_indices(self, src_xyz, tgt_xyz, voxel_size, T=None, min_points=1):
        """computeIndicesOfOverlappingPoints (helpers.cpp:320-345) on the device: ascending indices (src_idx, tgt_idx) of
        the points of either fp64 cloud whose voxel holds >= min_points points of the target and of the source moved by
        `T` (4x4 sourceToTarget; None: identity)."""
        s = np.ascontiguousarray(src_xyz, np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(tgt_xyz, np.float64).reshape(-1, 3)
        si, ti = np.empty(max(s.shape[0], 1), np.int32), np.empty(max(t.shape[0], 1), np.int32)
        ns, nt = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.reg_overlap_indices(self._h, _ptr(s), s.shape[0], _ptr(t), t.shape[0], 0, _T_in_f64(T),
                                                  float(voxel_size), int(min_points), _ptr(si), C.byref(ns), _ptr(ti),
                                                  C.byref(nt)))
        return si[:int(ns.value)].copy(), ti[:int(nt.value)].copy()

    def overlap_indices_device(self, src_ptr, n, tgt_ptr, m, voxel_size, src_idx_ptr, tgt_idx_ptr, T=None, min_points=1):
        """As overlap_indices with both fp64 clouds and both int32 index outputs (capacity n / m) resident in HBM.
        Returns (n_src, n_tgt)."""
        ns, nt = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.reg_overlap_indices(self._h, C.c_void_p(src_ptr), n, C.c_void_p(tgt_ptr), m, 1, _T_in_f64(T),
                                                  float(voxel_size), int(min_points), C.c_void_p(src_idx_ptr), C.byref(ns),
                                                  C.c_void_p(tgt_idx_ptr), C.byref(nt)))
        return int(ns.value), int(nt.value)

    def set_pair_overlap_f64(self, src_xyz, tgt_xyz, voxel_size, T=None, min_points=1, src_normals=None, src_covs=None,
                             tgt_normals=None, tgt_covs=None):
        """The front of buildConstraint (constraint_builders.cpp:51-58) in one call: overlap selection of the two fp64
        clouds, SelectByIndex + fp32 cast on the device, the selected target as the reference and the selected source as
        the reading.  Returns (n_src_kept, n_tgt_kept)."""
        f64 = lambda a, w: np.ascontiguousarray(a, np.float64).reshape(-1, w) if a is not None else None
        s, sn, sc = f64(src_xyz, 3), f64(src_normals, 3), f64(src_covs, 9)
        t, tn, tc = f64(tgt_xyz, 3), f64(tgt_normals, 3), f64(tgt_covs, 9)
        return self._set_pair(_ptr(s), _ptr(sn), _ptr(sc), s.shape[0], _ptr(t), _ptr(tn), _ptr(tc), t.shape[0], 0,
                              voxel_size, T, min_points)

    def set_pair_overlap_f64_device(self, src_ptr, n, tgt_ptr, m, voxel_size, T=None, min_points=1, src_nrm_ptr=None,
                                    src_cov_ptr=None, tgt_nrm_ptr=None, tgt_cov_ptr=None):
        """As set_pair_overlap_f64 with the fp64 arrays already resident in HBM (xyz / normals x 3, covs x 9 doubles)."""
        vp = lambda p: C.c_void_p(p) if p else None
        return self._set_pair(vp(src_ptr), vp(src_nrm_ptr), vp(src_cov_ptr), n, vp(tgt_ptr), vp(tgt_nrm_ptr),
                              vp(tgt_cov_ptr), m, 1, voxel_size, T, min_points)

    def _set_pair(self, s, sn, sc, n, t, tn, tc, m, on_device, voxel_size, T, min_points):
        ks, kt = C.c_int64(0), C.c_int64(0)
        st = self._lib.reg_set_pair_overlap_f64(self._h, s, sn, sc, n, t, tn, tc, m, on_device, _T_in_f64(T),
                                                float(voxel_size), int(min_points), C.byref(ks), C.byref(kt))
        # n_target_kept sizes target_source_indices() (as after set_target_f64), n_source_kept source_source_indices()
        self.n_source_kept, self.n_target_kept = int(ks.value), int(kt.value)
        self.n_source = self.n_source_kept if st == 0 else 0
        self._check(st)
        return self.n_source_kept, self.n_target_kept

    def source_source_indices(self):
        """Position of every reading point in the source cloud given to set_pair_overlap_f64."""
        idx = np.empty(max(getattr(self, "n_source_kept", 0), 1), np.int32)
        self._check(self._lib.reg_get_source_source_indices(self._h, _ptr(idx)))
        return idx[:self.n_source_kept]

    # ---- FPFH features and mutual feature matching ----
    def compute_fpfh(self, xyz, normals, radius, max_nn=100, want_spfh=False, want_counts=False):
        """ComputeFPFHFeature with a hybrid search (Submap.cpp:255-275) on the device.  Returns a dict: `fpfh` (n, 33)
        float64 (row i = column i of Open3D's Feature::data_), on request `spfh` (n, 33) and `n_neighbours` (n,), plus
        `n_rescanned`."""
        xyz, nrm = _f32(xyz), _f32(normals)
        n = xyz.shape[0] if xyz.ndim == 2 else 0
        out = {"fpfh": np.zeros((n, 33), np.float64)}
        if want_spfh:
            out["spfh"] = np.zeros((n, 33), np.float64)
        if want_counts:
            out["n_neighbours"] = np.zeros(n, np.int32)
        resc = C.c_int64(0)
        self._check(self._lib.reg_compute_fpfh(self._h, _ptr(xyz), xyz.shape[1] if xyz.ndim == 2 else 3, _ptr(nrm),
                                               nrm.shape[1] if nrm.ndim == 2 else 3, n, 0, int(max_nn), float(radius),
                                               _ptr(out["fpfh"]), _ptr(out.get("spfh")), _ptr(out.get("n_neighbours")),
                                               C.byref(resc)))
        out["n_rescanned"] = int(resc.value)
        return out

    def compute_fpfh_device(self, xyz_ptr, xyz_stride, nrm_ptr, nrm_stride, n, radius, max_nn, fpfh_ptr, spfh_ptr=None,
                            n_neighbours_ptr=None):
        """As compute_fpfh with the fp32 cloud and normals and the outputs (fpfh / spfh n x 33 doubles, n_neighbours n
        int32) resident in HBM.  Returns n_rescanned."""
        vp = lambda p: C.c_void_p(p) if p else None
        resc = C.c_int64(0)
        self._check(self._lib.reg_compute_fpfh(self._h, vp(xyz_ptr), xyz_stride, vp(nrm_ptr), nrm_stride, n, 1, int(max_nn),
                                               float(radius), vp(fpfh_ptr), vp(spfh_ptr), vp(n_neighbours_ptr),
                                               C.byref(resc)))
        return int(resc.value)

    def match_features(self, fa, fb, backward=True, mutual=True):
        """Nearest neighbours between two sets of feature rows (na x dim, nb x dim float64).  Returns (nn_ab, nn_ba,
        mutual): nn_ba is None without `backward` and `mutual`, mutual (k, 2) int32 pairs (a, b) or None."""
        a, b = np.ascontiguousarray(fa, np.float64), np.ascontiguousarray(fb, np.float64)
        na, nb = (a.shape[0], b.shape[0]) if a.ndim == 2 and b.ndim == 2 else (0, 0)
        dim = a.shape[1] if a.ndim == 2 else 0
        if b.ndim == 2 and b.shape[1] != dim:
            dim = 0                                   # the library reports the bad argument
        nn_ab = np.full(max(na, 1), -1, np.int32)
        nn_ba = np.full(max(nb, 1), -1, np.int32) if (backward or mutual) else None
        mu = np.full((max(na, 1), 2), -1, np.int32) if mutual else None
        km = C.c_int64(0)
        self._check(self._lib.reg_match_features(self._h, _ptr(a), na, _ptr(b), nb, dim, 0, _ptr(nn_ab), _ptr(nn_ba),
                                                 _ptr(mu), C.byref(km)))
        return nn_ab[:na], (nn_ba[:nb] if nn_ba is not None else None), (mu[:int(km.value)].copy() if mutual else None)

    def match_features_device(self, fa_ptr, na, fb_ptr, nb, dim, nn_ab_ptr, nn_ba_ptr=None, mutual_ptr=None):
        """As match_features with the feature rows and the int32 outputs (nn_ab na, nn_ba nb, mutual 2 x na) resident in
        HBM.  Returns n_mutual."""
        vp = lambda p: C.c_void_p(p) if p else None
        km = C.c_int64(0)
        self._check(self._lib.reg_match_features(self._h, vp(fa_ptr), na, vp(fb_ptr), nb, int(dim), 1, vp(nn_ab_ptr),
                                                 vp(nn_ba_ptr), vp(mutual_ptr), C.byref(km)))
        return int(km.value)

    # ---- RANSAC registration on correspondences ----
    @staticmethod
    def _ransac_params(max_correspondence_distance, ransac_n, max_iteration, confidence, distance_threshold,
                       edge_similarity, seed, batch):
        p = RansacParams()
        p.struct_size = C.sizeof(RansacParams)
        p.ransac_n, p.max_iteration, p.confidence = int(ransac_n), int(max_iteration), float(confidence)
        p.max_correspondence_distance = float(max_correspondence_distance)
        p.distance_threshold, p.edge_similarity = float(distance_threshold), float(edge_similarity)
        p.seed, p.batch = int(seed) & 0xFFFFFFFFFFFFFFFF, int(batch)
        return p

    @staticmethod
    def _ransac_out(res, inliers=None, status=None):
        out = {"T": np.array(res.T, np.float64).reshape(4, 4).T.copy(), "fitness": float(res.fitness),
               "inlier_rmse": float(res.inlier_rmse), "n_inliers": int(res.n_inliers), "n_iterations": int(res.n_iterations),
               "n_validated": int(res.n_validated), "best_iteration": int(res.best_iteration), "batch": int(res.batch)}
        if inliers is not None:
            out["inliers"] = inliers[:out["n_inliers"]].copy()
        if status is not None:
            out["iter_status"] = status
        return out

    def ransac_correspondences(self, src_xyz, tgt_xyz, corres, max_correspondence_distance, ransac_n=3,
                               max_iteration=100000, confidence=0.999, distance_threshold=0.0, edge_similarity=0.0, seed=0,
                               batch=0, want_status=False):
        """RegistrationRANSACBasedOnCorrespondence on the device (reg_ransac_correspondences): fp64 clouds (n x 3, m x 3),
        `corres` (k, 2) int32 pairs (source, target).  A checker threshold <= 0 switches that checker off.  Returns a dict:
        `T` (4 x 4), `fitness`, `inlier_rmse`, `inliers` (count, 2), `n_inliers`, `n_iterations`, `n_validated`,
        `best_iteration`, `batch` (the device batch size used), and with `want_status` `iter_status` (max_iteration,) int32, filled up to n_iterations (the rest
        keeps the fill value -9)."""
        s = np.ascontiguousarray(src_xyz, np.float64).reshape(-1, 3)
        t = np.ascontiguousarray(tgt_xyz, np.float64).reshape(-1, 3)
        c = np.ascontiguousarray(corres, np.int32).reshape(-1, 2)
        p = self._ransac_params(max_correspondence_distance, ransac_n, max_iteration, confidence, distance_threshold,
                                edge_similarity, seed, batch)
        res = RansacResult()
        res.struct_size = C.sizeof(RansacResult)
        inl = np.full((max(c.shape[0], 1), 2), -1, np.int32)
        status = np.full(max(int(max_iteration), 1), -9, np.int32) if want_status else None
        self._check(self._lib.reg_ransac_correspondences(self._h, _ptr(s), s.shape[0], _ptr(t), t.shape[0], _ptr(c),
                                                         c.shape[0], 0, C.byref(p), C.byref(res), _ptr(inl), _ptr(status)))
        return self._ransac_out(res, inl, status)

    def ransac_correspondences_device(self, src_ptr, n, tgt_ptr, m, corres_ptr, k, inliers_ptr, max_correspondence_distance,
                                      ransac_n=3, max_iteration=100000, confidence=0.999, distance_threshold=0.0,
                                      edge_similarity=0.0, seed=0, batch=0, iter_status_ptr=None):
        """As ransac_correspondences with the fp64 clouds, the int32 pairs and the outputs (inliers 2 x k int32,
        iter_status max_iteration int32) resident in HBM.  Returns the dict without the arrays."""
        vp = lambda q: C.c_void_p(q) if q else None
        p = self._ransac_params(max_correspondence_distance, ransac_n, max_iteration, confidence, distance_threshold,
                                edge_similarity, seed, batch)
        res = RansacResult()
        res.struct_size = C.sizeof(RansacResult)
        self._check(self._lib.reg_ransac_correspondences(self._h, vp(src_ptr), n, vp(tgt_ptr), m, vp(corres_ptr), k, 1,
                                                         C.byref(p), C.byref(res), vp(inliers_ptr), vp(iter_status_ptr)))
        return self._ransac_out(res)

    def set_source(self, xyz, normals=None, covs=None):
        xyz = _f32(xyz)
        nrm = _f32(normals) if normals is not None else None
        cov = _f32(covs) if covs is not None else None
        n = xyz.shape[0] if xyz.ndim == 2 else 0
        self._check(self._lib.reg_set_source(self._h, _ptr(xyz), xyz.shape[1] if xyz.ndim == 2 else 3, _ptr(nrm),
                                             nrm.shape[1] if nrm is not None else 3, _ptr(cov), n, 0))
        self.n_source = n

    def set_source_f64(self, xyz, normals=None, covs=None):
        """R11, reading side: Open3D's fp64 arrays (points_ / normals_ n x 3, covariances_ n x 3 x 3) cast on the device
        as open3dToPointmatcher does (open3d_conversions.cpp:57-118)."""
        x = np.ascontiguousarray(xyz, np.float64)
        nr = np.ascontiguousarray(normals, np.float64) if normals is not None else None
        cv = np.ascontiguousarray(covs, np.float64).reshape(-1, 9) if covs is not None else None
        n = x.shape[0] if x.ndim == 2 else 0
        self._check(self._lib.reg_set_source_f64(self._h, _ptr(x), _ptr(nr), _ptr(cv), n, 0))
        self.n_source = n

    def set_source_f64_device(self, xyz_ptr, n, nrm_ptr=None, cov_ptr=None):
        self._check(self._lib.reg_set_source_f64(self._h, C.c_void_p(xyz_ptr), C.c_void_p(nrm_ptr) if nrm_ptr else None,
                                                 C.c_void_p(cov_ptr) if cov_ptr else None, n, 1))
        self.n_source = n

    def estimate_normals(self, xyz, k=10, max_dist=np.inf, viewpoint=None, regularise=False, want_eigvals=False,
                         want_covs=False, want_ids=False, want_eigvecs=False, want_densities=False,
                         want_mean_dists=False):
        """Exact k-NN + PCA normals (SurfaceNormal.cpp:152-252 / CloudRegistration.cpp:25-43).  Returns a dict with
        `normals` (n,3) and, on request, `eigvals` (n,3), `eigvecs` (n,9), `covs` (n,6), `densities` (n,),
        `mean_dists` (n,), `ids` (n,k), plus `n_rescanned`."""
        xyz = _f32(xyz)
        n = xyz.shape[0] if xyz.ndim == 2 else 0
        out = {"normals": np.zeros((n, 3), np.float32)}
        for key, want, shape, dt in (("eigvals", want_eigvals, (n, 3), np.float32), ("eigvecs", want_eigvecs, (n, 9), np.float32),
                                     ("covs", want_covs, (n, 6), np.float32), ("densities", want_densities, (n,), np.float32),
                                     ("mean_dists", want_mean_dists, (n,), np.float32), ("ids", want_ids, (n, k), np.int32)):
            if want:
                out[key] = np.zeros(shape, dt)
        o = NormalsOut()
        for key in ("normals", "eigvals", "eigvecs", "covs", "densities", "mean_dists", "ids"):
            setattr(o, key, out[key].ctypes.data if key in out else None)
        vp_ = _f32(viewpoint) if viewpoint is not None else None
        resc = C.c_int64(0)
        self._check(self._lib.reg_estimate_normals(
            self._h, _ptr(xyz), xyz.shape[1] if xyz.ndim == 2 else 3, n, 0, int(k), float(max_dist), _ptr(vp_),
            1 if regularise else 0, C.byref(o), C.byref(resc)))
        out["n_rescanned"] = int(resc.value)
        return out

    def sampling_surface_normal(self, xyz, params: "SsnParams | None" = None, want_leaf_id=False, **kw):
        """SamplingSurfaceNormalDataPointsFilter on the device (reg_sampling_surface_normal).  `kw` sets SsnParams fields.
        Returns a dict: xyz (m,3), src_idx (m,), normals / densities / eigvals / eigvecs as the keep* switches ask,
        leaf_id (n,) on request, n_out, n_unfit."""
        p = params if params is not None else default_ssn_params()
        for k, v in kw.items():
            setattr(p, k, v)
        xyz = _f32(xyz)
        n = xyz.shape[0] if xyz.ndim == 2 else 0
        out = {"xyz": np.zeros((n, 3), np.float32), "src_idx": np.zeros(n, np.int32)}
        for key, want, shape in (("normals", p.keep_normals, (n, 3)), ("densities", p.keep_densities, (n,)),
                                 ("eigvals", p.keep_eigen_values, (n, 3)), ("eigvecs", p.keep_eigen_vectors, (n, 9))):
            if want:
                out[key] = np.zeros(shape, np.float32)
        if want_leaf_id:
            out["leaf_id"] = np.zeros(n, np.int32)
        o = SsnOut()
        for key in ("xyz", "normals", "densities", "eigvals", "eigvecs", "src_idx", "leaf_id"):
            setattr(o, key, out[key].ctypes.data if key in out else None)
        m, unfit = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.reg_sampling_surface_normal(self._h, _ptr(xyz), xyz.shape[1] if xyz.ndim == 2 else 3, n, 0,
                                                          C.byref(p), C.byref(o), C.byref(m), C.byref(unfit)))
        for key in ("xyz", "src_idx", "normals", "densities", "eigvals", "eigvecs"):
            if key in out:
                out[key] = out[key][:m.value].copy()
        out["n_out"], out["n_unfit"] = int(m.value), int(unfit.value)
        return out

    def sampling_surface_normal_device(self, xyz_ptr, xyz_stride, n, params: "SsnParams", xyz_out_ptr, normals_ptr=None,
                                       densities_ptr=None, eigvals_ptr=None, eigvecs_ptr=None, src_idx_ptr=None,
                                       leaf_id_ptr=None):
        """Device-pointer form: every output holds n rows of capacity.  Returns (n_out, n_unfit)."""
        o = SsnOut(xyz_out_ptr, normals_ptr, densities_ptr, eigvals_ptr, eigvecs_ptr, src_idx_ptr, leaf_id_ptr)
        m, unfit = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.reg_sampling_surface_normal(self._h, C.c_void_p(xyz_ptr), xyz_stride, n, 1, C.byref(params),
                                                          C.byref(o), C.byref(m), C.byref(unfit)))
        return int(m.value), int(unfit.value)

    def filter_points(self, xyz, filters, normals=None, covs=None):
        """Reading-side filter chain on the device (reg_filter_points).  filters: dicts for point_filter() or
        PointFilter structs.  Returns (xyz (m,3), src_idx (m,), normals or None, covs or None)."""
        xyz = _f32(xyz)
        n = xyz.shape[0] if xyz.ndim == 2 else 0
        nr = _f32(normals) if normals is not None else None
        cv = _f32(covs) if covs is not None else None
        arr = (PointFilter * max(len(filters), 1))(*[f if isinstance(f, PointFilter) else point_filter(f) for f in filters])
        ox, oi = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        on = np.zeros((n, 3), np.float32) if nr is not None else None
        oc = np.zeros((n, 6), np.float32) if cv is not None else None
        m = C.c_int64(0)
        self._check(self._lib.reg_filter_points(self._h, _ptr(xyz), xyz.shape[1] if xyz.ndim == 2 else 3, _ptr(nr), _ptr(cv),
                                                n, 0, C.cast(arr, C.c_void_p), len(filters), _ptr(ox), _ptr(on), _ptr(oc),
                                                _ptr(oi), C.byref(m)))
        k = int(m.value)
        return ox[:k].copy(), oi[:k].copy(), (on[:k].copy() if on is not None else None), (oc[:k].copy() if oc is not None else None)

    def filter_points_device(self, xyz_ptr, xyz_stride, n, filters, out_xyz_ptr, nrm_ptr=None, cov_ptr=None,
                             out_nrm_ptr=None, out_cov_ptr=None, out_idx_ptr=None) -> int:
        arr = (PointFilter * max(len(filters), 1))(*[f if isinstance(f, PointFilter) else point_filter(f) for f in filters])
        m = C.c_int64(0)
        self._check(self._lib.reg_filter_points(self._h, C.c_void_p(xyz_ptr), xyz_stride, nrm_ptr, cov_ptr, n, 1,
                                                C.cast(arr, C.c_void_p), len(filters), out_xyz_ptr, out_nrm_ptr,
                                                out_cov_ptr, out_idx_ptr, C.byref(m)))
        return int(m.value)

    def filter_cloud(self, xyz, filters, descriptors=None):
        """Descriptor-carrying filter chain on the device (reg_filter_cloud).  filters: dicts as for point_filter() /
        cloud_filter(); descriptors: {name: (n, span) array} carried through every compaction.  Returns
        (xyz (m,3), src_idx (m,), {name: (m, span)}) with the descriptors the chain created added."""
        xyz = _f32(xyz)
        n = xyz.shape[0] if xyz.ndim == 2 else 0
        given = {k: _f32(v).reshape(n, -1) for k, v in (descriptors or {}).items()}
        spans = [(k, v.shape[1]) for k, v in given.items()]
        spans += [f for f in cloud_filter_created_fields(filters) if f[0] not in given]
        names = [k for k, _ in spans]
        outs = {k: np.zeros((n, w), np.float32) for k, w in spans}
        farr = (Field * max(len(spans), 1))()
        for i, (k, w) in enumerate(spans):
            farr[i].in_, farr[i].out, farr[i].span = (given[k].ctypes.data if k in given else None), outs[k].ctypes.data, w
        carr = (CloudFilter * max(len(filters), 1))(*[cloud_filter(f, names) for f in filters])
        ox, oi = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        m = C.c_int64(0)
        self._check(self._lib.reg_filter_cloud(self._h, _ptr(xyz), xyz.shape[1] if xyz.ndim == 2 else 3, n, 0,
                                               C.cast(farr, C.c_void_p), len(spans), C.cast(carr, C.c_void_p), len(filters),
                                               _ptr(ox), _ptr(oi), C.byref(m)))
        k = int(m.value)
        return ox[:k].copy(), oi[:k].copy(), {name: a[:k].copy() for name, a in outs.items()}

    def filter_cloud_device(self, xyz_ptr, xyz_stride, n, filters, fields, out_xyz_ptr, out_idx_ptr=None) -> int:
        """Device-pointer form.  fields: [(name, in_ptr or None, out_ptr or None, span)], every output with n rows of
        capacity.  Returns n_out."""
        names = [f[0] for f in fields]
        farr = (Field * max(len(fields), 1))()
        for i, (_, pin, pout, w) in enumerate(fields):
            farr[i].in_, farr[i].out, farr[i].span = pin or None, pout or None, w
        carr = (CloudFilter * max(len(filters), 1))(*[cloud_filter(f, names) for f in filters])
        m = C.c_int64(0)
        self._check(self._lib.reg_filter_cloud(self._h, C.c_void_p(xyz_ptr), xyz_stride, n, 1, C.cast(farr, C.c_void_p),
                                               len(fields), C.cast(carr, C.c_void_p), len(filters), out_xyz_ptr,
                                               out_idx_ptr, C.byref(m)))
        return int(m.value)

    def voxel_grid(self, xyz, params: "VoxelGridParams | None" = None, descriptors=None):
        """VoxelGridDataPointsFilter (useCentroid 1) on the device (reg_voxel_grid).  Returns (xyz (m,3), src_idx (m,),
        {name: (m, span)}): one row per occupied voxel, ascending by its first member's index."""
        p = params if params is not None else default_voxel_grid_params()
        xyz = _f32(xyz)
        n = xyz.shape[0] if xyz.ndim == 2 else 0
        given = {k: _f32(v).reshape(n, -1) for k, v in (descriptors or {}).items()}
        outs = {k: np.zeros(v.shape, np.float32) for k, v in given.items()}
        farr = (Field * max(len(given), 1))()
        for i, (k, v) in enumerate(given.items()):
            farr[i].in_, farr[i].out, farr[i].span = v.ctypes.data, outs[k].ctypes.data, v.shape[1]
        ox, oi = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        m = C.c_int64(0)
        self._check(self._lib.reg_voxel_grid(self._h, _ptr(xyz), xyz.shape[1] if xyz.ndim == 2 else 3, n, 0,
                                             C.cast(farr, C.c_void_p), len(given), C.byref(p), _ptr(ox), _ptr(oi),
                                             C.byref(m)))
        k = int(m.value)
        return ox[:k].copy(), oi[:k].copy(), {name: a[:k].copy() for name, a in outs.items()}

    def voxel_grid_device(self, xyz_ptr, xyz_stride, n, params: "VoxelGridParams", fields, out_xyz_ptr,
                          out_idx_ptr=None) -> int:
        """Device-pointer form; fields as for filter_cloud_device (every in_ptr set).  Returns n_out."""
        farr = (Field * max(len(fields), 1))()
        for i, (_, pin, pout, w) in enumerate(fields):
            farr[i].in_, farr[i].out, farr[i].span = pin or None, pout or None, w
        m = C.c_int64(0)
        self._check(self._lib.reg_voxel_grid(self._h, C.c_void_p(xyz_ptr), xyz_stride, n, 1, C.cast(farr, C.c_void_p),
                                             len(fields), C.byref(params), out_xyz_ptr, out_idx_ptr, C.byref(m)))
        return int(m.value)

    def octree_grid(self, xyz, params: "OctreeParams | None" = None, normals=None, covs=None, **kw):
        """OctreeGridDataPointsFilter on the device (reg_octree_grid).  `kw` sets OctreeParams fields.  Returns a dict:
        xyz (m,3), src_idx (m,), normals / covs when given, leaf_id (n,), leaf_depth (n,), n_out."""
        p = params if params is not None else default_octree_params()
        for k, v in kw.items():
            setattr(p, k, v)
        xyz = _f32(xyz)
        n = xyz.shape[0] if xyz.ndim == 2 else 0
        nr = _f32(normals) if normals is not None else None
        cv = _f32(covs) if covs is not None else None
        out = {"xyz": np.zeros((n, 3), np.float32), "src_idx": np.zeros(n, np.int32),
               "leaf_id": np.zeros(n, np.int32), "leaf_depth": np.zeros(n, np.int32)}
        if nr is not None:
            out["normals"] = np.zeros((n, 3), np.float32)
        if cv is not None:
            out["covs"] = np.zeros((n, 6), np.float32)
        o = OctreeOut()
        for key in ("xyz", "normals", "covs", "src_idx", "leaf_id", "leaf_depth"):
            setattr(o, key, out[key].ctypes.data if key in out else None)
        m = C.c_int64(0)
        self._check(self._lib.reg_octree_grid(self._h, _ptr(xyz), xyz.shape[1] if xyz.ndim == 2 else 3, _ptr(nr), _ptr(cv),
                                              n, 0, C.byref(p), C.byref(o), C.byref(m)))
        for key in ("xyz", "src_idx", "normals", "covs"):
            if key in out:
                out[key] = out[key][:m.value].copy()
        out["n_out"] = int(m.value)
        return out

    def octree_grid_device(self, xyz_ptr, xyz_stride, n, params: "OctreeParams", xyz_out_ptr, nrm_ptr=None, cov_ptr=None,
                           normals_out_ptr=None, covs_out_ptr=None, src_idx_ptr=None, leaf_id_ptr=None,
                           leaf_depth_ptr=None) -> int:
        """Device-pointer form: outputs hold n rows of capacity.  Returns n_out."""
        o = OctreeOut(xyz_out_ptr, normals_out_ptr, covs_out_ptr, src_idx_ptr, leaf_id_ptr, leaf_depth_ptr)
        m = C.c_int64(0)
        self._check(self._lib.reg_octree_grid(self._h, C.c_void_p(xyz_ptr), xyz_stride, nrm_ptr, cov_ptr, n, 1,
                                              C.byref(params), C.byref(o), C.byref(m)))
        return int(m.value)

    def smooth_normals(self, normals, ids):
        """SurfaceNormalDataPointsFilter's smoothNormals (SurfaceNormal.cpp:259-283) on the device, sequential semantics.
        Returns (smoothed normals (n,3), sweeps launched)."""
        nr = np.ascontiguousarray(normals, dtype=np.float32).copy()
        ii = np.ascontiguousarray(ids, dtype=np.int32)
        passes = C.c_int32(0)
        self._check(self._lib.reg_smooth_normals(self._h, _ptr(nr), _ptr(ii), nr.shape[0], ii.shape[1], 0, C.byref(passes)))
        return nr, int(passes.value)

    def estimate_normals_device(self, xyz_ptr, xyz_stride, n, normals_ptr, k=10, max_dist=np.inf, viewpoint=None,
                                regularise=False, eigvals_ptr=None, covs_ptr=None, ids_ptr=None, eigvecs_ptr=None,
                                densities_ptr=None, mean_dists_ptr=None):
        vp_ = _f32(viewpoint) if viewpoint is not None else None
        o = NormalsOut()
        o.normals, o.eigvals, o.eigvecs, o.covs = normals_ptr, eigvals_ptr, eigvecs_ptr, covs_ptr
        o.densities, o.mean_dists, o.ids = densities_ptr, mean_dists_ptr, ids_ptr
        resc = C.c_int64(0)
        self._check(self._lib.reg_estimate_normals(
            self._h, C.c_void_p(xyz_ptr), xyz_stride, n, 1, int(k), float(max_dist), _ptr(vp_), 1 if regularise else 0,
            C.byref(o), C.byref(resc)))
        return int(resc.value)

    # ---- device-pointer entry points (inputs already resident in HBM) ---------------------------
    def set_target_device(self, xyz_ptr, xyz_stride, m, nrm_ptr=None, nrm_stride=3, cov_ptr=None):
        self._check(self._lib.reg_set_target(self._h, C.c_void_p(xyz_ptr), xyz_stride,
                                             C.c_void_p(nrm_ptr) if nrm_ptr else None, nrm_stride,
                                             C.c_void_p(cov_ptr) if cov_ptr else None, m, 1))

    def set_source_device(self, xyz_ptr, xyz_stride, n, nrm_ptr=None, nrm_stride=3, cov_ptr=None):
        self._check(self._lib.reg_set_source(self._h, C.c_void_p(xyz_ptr), xyz_stride,
                                             C.c_void_p(nrm_ptr) if nrm_ptr else None, nrm_stride,
                                             C.c_void_p(cov_ptr) if cov_ptr else None, n, 1))
        self.n_source = n

    def register(self, T_init=None):
        Ti = _T_in(np.eye(4) if T_init is None else T_init)
        To = np.zeros(16, np.float32)
        res = RegResult()
        st = self._lib.reg_register(self._h, _ptr(Ti), _ptr(To), C.byref(res))
        self.last_result = res
        self._check(st)
        return _T_out(To), res

    def information_matrix(self, T, max_dist):
        """GetInformationMatrixFromPointClouds analogue (constraint_builders.cpp:69-73): (6x6 float64, n_pairs)."""
        Ti = _T_in(T)
        info = (C.c_double * 36)()
        n = C.c_int64(0)
        self._check(self._lib.reg_information_matrix(self._h, _ptr(Ti), float(max_dist), info, C.byref(n)))
        return np.array(info[:], np.float64).reshape(6, 6), int(n.value)

    def halo_bound(self, xyz):
        """reg_debug_halo_bound: per position (frame of set_target's input) the empty-space bound the search reads for its
        halo bin [m]; 0 for a bin that lists points, -1 where the search does not consult the directory."""
        x = _f32(xyz)
        out = np.empty(x.shape[0], np.float32)
        self._check(self._lib.reg_debug_halo_bound(self._h, _ptr(x), x.shape[0], _ptr(out)))
        return out

    def halo_witness(self, xyz):
        """reg_debug_halo_witness: per position (frame of set_target's input) the witness point that the halo directory names
        for its bin, as an original index; -1 for none, -2 for a bin that lists points.  A position outside the halo grid
        lies in no bin: it gets what the search takes from the border bin it clamps to (its witness, or the first record
        of its run)."""
        x = _f32(xyz)
        out = np.empty(x.shape[0], np.int32)
        self._check(self._lib.reg_debug_halo_witness(self._h, _ptr(x), x.shape[0], _ptr(out)))
        return out

    def prepare(self, T_init=None):
        Ti = _T_in(np.eye(4) if T_init is None else T_init)
        self._check(self._lib.reg_prepare(self._h, _ptr(Ti)))

    def linearize(self, T_iter=None):
        Ti = _T_in(np.eye(4) if T_iter is None else T_iter)
        H = np.zeros(36, np.float32)
        b = np.zeros(6, np.float32)
        err = C.c_double()
        cnt = C.c_int64()
        self._check(self._lib.reg_linearize(self._h, _ptr(Ti), _ptr(H), _ptr(b), C.byref(err), C.byref(cnt)))
        return H.reshape(6, 6), b, err.value, cnt.value

    def source_count(self) -> int:
        """reg_get_source_count: the rows of the reading the handle holds, whoever installed it.  n_source is a cached copy."""
        n = C.c_int64(0)
        self._check(self._lib.reg_get_source_count(self._h, C.byref(n)))
        self.n_source = int(n.value)
        return self.n_source

    def correspondences(self, want_w=True):
        n = self.source_count()
        ids = np.empty(n, np.int32)
        d2 = np.empty(n, np.float32)
        w = np.empty(n, np.float32) if want_w else None
        self._check(self._lib.reg_get_correspondences(self._h, _ptr(ids), _ptr(d2), _ptr(w)))
        return ids, d2, w

    def set_pm_chain(self, chain: "PmChain | None"):
        """reg_set_pm_chain: None (or the default chain) returns to the plain loop; resets the robust state."""
        if chain is not None:
            chain.struct_size = C.sizeof(type(chain))   # PmChain (REG_PM_CHAIN_SIZE_V2) or PmChainV3
        self.pm_chain = chain
        self._check(self._lib.reg_set_pm_chain(self._h, C.byref(chain) if chain is not None else None))

    def set_ternary_xicp(self, ternary: "TernaryXicp | None"):
        """reg_set_ternary_xicp: None (or enabled = 0) turns EqualityConstraints off."""
        if ternary is not None:
            ternary.struct_size = C.sizeof(TernaryXicp)
        self._check(self._lib.reg_set_ternary_xicp(self._h, C.byref(ternary) if ternary is not None else None))
        self.ternary_xicp = ternary

    def get_ternary_xicp(self) -> TernaryXicpResult:
        """reg_get_ternary_xicp: the EqualityConstraints analysis of the last iteration."""
        out = TernaryXicpResult()
        out.struct_size = C.sizeof(TernaryXicpResult)
        self._check(self._lib.reg_get_ternary_xicp(self._h, C.byref(out)))
        return out

    def get_correspondences_k(self, knn=None, want_w=True):
        """(ids, d2, w) of the last iteration, each n x knn, reading input order, ascending (d2, id)."""
        if knn is None:
            knn = self.pm_chain.knn if getattr(self, "pm_chain", None) is not None else 1
        n = self.source_count()
        ids = np.empty((n, knn), np.int32)
        d2 = np.empty((n, knn), np.float32)
        w = np.empty((n, knn), np.float32) if want_w else None
        self._check(self._lib.reg_get_correspondences_k(self._h, int(knn), _ptr(ids), _ptr(d2), _ptr(w)))
        return ids, d2, w

    def robust_state(self):
        """(scale, iteration) of the chain's RobustOutlierFilter as the next registration starts with them."""
        sc = C.c_float()
        it = C.c_int32()
        self._check(self._lib.reg_get_robust_state(self._h, C.byref(sc), C.byref(it)))
        return float(sc.value), int(it.value)

    def get_var_trim(self):
        """(optRatio, k, n) of the chain's VarTrimmedDistOutlierFilter in the last iteration (at T_iter_prev)."""
        ratio, k, n = C.c_float(), C.c_int64(), C.c_int64()
        self._check(self._lib.reg_get_var_trim(self._h, C.byref(ratio), C.byref(k), C.byref(n)))
        return float(ratio.value), int(k.value), int(n.value)

    def get_covariance(self):
        """(cov float32 6x6 in the order [x y z alpha beta gamma], rank of H) of the last with_cov registration."""
        cov = np.zeros(36, np.float32)
        rank = C.c_int32()
        self._check(self._lib.reg_get_covariance(self._h, _ptr(cov), C.byref(rank)))
        return cov.reshape(6, 6), int(rank.value)

    def get_covariance_sums(self):
        """(H, M) float64 6x6: the sums the covariance of the last with_cov registration came from."""
        Hp, Mp = np.zeros(21, np.float64), np.zeros(21, np.float64)
        self._check(self._lib.reg_get_covariance_sums(self._h, _ptr(Hp), _ptr(Mp)))
        return unpack_sym6(Hp), unpack_sym6(Mp)

    def get_minimizer_stats(self) -> MinimizerStats:
        st = MinimizerStats()
        st.struct_size = C.sizeof(MinimizerStats)
        self._check(self._lib.reg_get_minimizer_stats(self._h, C.byref(st)))
        return st

    def get_degeneracy(self):
        """(categories int32[6], eigenvalues float32[6] descending, condition number) of SolutionRemapping's last step."""
        cat, eig, cond = np.zeros(6, np.int32), np.zeros(6, np.float32), C.c_float()
        self._check(self._lib.reg_get_degeneracy(self._h, _ptr(cat), _ptr(eig), C.byref(cond)))
        return cat, eig, float(cond.value)

    def get_bound(self):
        """(rotation [rad], translation) BoundTransformationChecker compared against its limits after the last update."""
        r, t = C.c_float(), C.c_float()
        self._check(self._lib.reg_get_bound(self._h, C.byref(r), C.byref(t)))
        return float(r.value), float(t.value)

    def target_info(self) -> TargetInfo:
        info = TargetInfo()
        self._check(self._lib.reg_get_target_info(self._h, C.byref(info)))
        return info

    def profile_kernels(self, T_iter=None, reps=20):
        ms = np.zeros(3, np.float32)
        Ti = _T_in(np.eye(4) if T_iter is None else T_iter)
        self._check(self._lib.reg_profile_kernels(self._h, _ptr(Ti), reps, _ptr(ms)))
        return {"match_ms": float(ms[0]), "select_ms": float(ms[1]), "linearize_ms": float(ms[2])}

    # ---- distributed halves ---------------------------------------------------------------------
    def source_centroid_sums(self):
        s = np.zeros(3, np.int64)
        self._check(self._lib.reg_source_centroid_sums(self._h, _ptr(s)))
        return s

    def prepare_centroid(self, T_init, c_read):
        c = np.ascontiguousarray(c_read, np.float32)
        self._check(self._lib.reg_prepare_centroid(self._h, _ptr(_T_in(T_init)), _ptr(c)))

    def compose(self, T_iter):
        To = np.zeros(16, np.float32)
        self._check(self._lib.reg_compose(self._h, _ptr(_T_in(T_iter)), _ptr(To)))
        return _T_out(To)

    # ---- stream-ordered distributed path ----------------------------------------------------------
    def dist_begin(self, T_start=None):
        self._check(self._lib.reg_dist_begin(self._h, _ptr(_T_in(T_start)) if T_start is not None else None))

    def dist_gather_buffers(self, n_ranks, n_max):
        """(d2_local_ptr, d2_all_ptr) of the select-by-gather iteration: n_max and n_ranks * n_max float32."""
        lp, ap = C.c_void_p(), C.c_void_p()
        self._check(self._lib.reg_dist_gather_buffers(self._h, int(n_ranks), int(n_max), C.byref(lp), C.byref(ap)))
        return lp.value, ap.value

    def dist_xicp_buffers(self):
        """(center_ptr, sums_ptr): 4 and 12 float64 to all-reduce after phases 7 and 8 of the first iteration."""
        cp, sp = C.c_void_p(), C.c_void_p()
        self._check(self._lib.reg_dist_xicp_buffers(self._h, C.byref(cp), C.byref(sp)))
        return cp.value, sp.value

    def dist_buffers(self):
        """(hist_ptr, sums_ptr): device addresses of the 3x2048 int32 histograms and the 32 float64 sums."""
        hp, sp = C.c_void_p(), C.c_void_p()
        self._check(self._lib.reg_dist_buffers(self._h, C.byref(hp), C.byref(sp)))
        return hp.value, sp.value

    def dist_fused_buffers(self, n_ranks, rank):
        """(contrib_ptr, gathered_ptr, contrib_bytes) of the fused multi-GPU iteration."""
        cp, gp, nb = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._check(self._lib.reg_dist_fused_buffers(self._h, n_ranks, rank, C.byref(cp), C.byref(gp), C.byref(nb)))
        return cp.value, gp.value, nb.value

    def dist_poll(self):
        st = DistStatus()
        self._check(self._lib.reg_dist_poll(self._h, C.byref(st)))
        return st

    def dist_centroid_sums(self):
        """Enqueues this slice's integer centroid sums; returns the device address of the 3 int64 to all-reduce."""
        p = C.c_void_p()
        self._check(self._lib.reg_dist_centroid_sums(self._h, C.byref(p)))
        return p.value

    def dist_prepare(self, T_init, n_global):
        Ti = _T_in(np.eye(4) if T_init is None else T_init)
        self._check(self._lib.reg_dist_prepare(self._h, _ptr(Ti), int(n_global)))

    def dist_record(self, seq_rel):
        """Report of ONE specific sequence (1-based since dist_begin); .sequences_done == seq_rel when available."""
        st = DistStatus()
        self._check(self._lib.reg_dist_record(self._h, int(seq_rel), C.byref(st)))
        return st

    def dist_phase(self, phase):
        self._check(self._lib.reg_dist_phase(self._h, phase))

    def dist_finish(self):
        To = np.zeros(16, np.float32)
        res = RegResult()
        st = self._lib.reg_dist_finish(self._h, _ptr(To), C.byref(res))
        self.last_result = res
        self._check(st)
        return _T_out(To), res

    # ---- multi-GPU registration behind the C ABI (RCCL, or a custom transport) --------------------------
    def dist_init(self, unique_id: bytes, rank: int, n_ranks: int):
        """ncclCommInitRank on the handle's device; `unique_id` = the 128 bytes of dist_unique_id() of rank 0."""
        buf = C.create_string_buffer(bytes(unique_id), DIST_ID_BYTES)
        self._check(self._lib.reg_dist_init(self._h, buf, int(rank), int(n_ranks)))

    def dist_init_custom(self, all_reduce_sum, all_gather, rank: int, n_ranks: int):
        """Transport given as Python callables (buf_ptr, count, dtype, stream) / (send_ptr, recv_ptr, bytes_per_rank,
        stream) -> 0 on success; both operate on DEVICE memory."""
        self._cb = (ALL_REDUCE_FN(lambda ctx, buf, n, dt, st: int(all_reduce_sum(buf, n, dt, st))),
                    ALL_GATHER_FN(lambda ctx, snd, rcv, nb, st: int(all_gather(snd, rcv, nb, st))))
        c = Collectives(None, self._cb[0], self._cb[1])
        self._check(self._lib.reg_dist_init_custom(self._h, C.byref(c), int(rank), int(n_ranks)))

    def dist_register(self, T_init=None):
        """Collective: == ICP::compute for the reading that is partitioned over the ranks of the group."""
        Ti = _T_in(np.eye(4) if T_init is None else T_init)
        To = np.zeros(16, np.float32)
        res = RegResult()
        st = self._lib.reg_dist_register(self._h, _ptr(Ti), _ptr(To), C.byref(res))
        self.last_result = res
        self._check(st)
        return _T_out(To), res

    def dist_info(self):
        n, g, f, s = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.reg_dist_info(self._h, C.byref(n), C.byref(g), C.byref(f), C.byref(s)))
        return {"n_global": n.value, "n_generic": g.value, "n_fused": f.value, "n_stalls": s.value}

    def dist_shutdown(self):
        self._check(self._lib.reg_dist_shutdown(self._h))

    def match_local(self, T_iter):
        self._check(self._lib.reg_match_local(self._h, _ptr(_T_in(T_iter))))

    def trim_histogram(self, level, prefix=0):
        hist = np.zeros(2048, np.uint32)
        self._check(self._lib.reg_trim_histogram(self._h, level, prefix, _ptr(hist)))
        return hist

    def reduce_local(self, T_iter, trim_limit=math.inf):
        sums = np.zeros(32, np.float64)
        self._check(self._lib.reg_reduce_local(self._h, _ptr(_T_in(T_iter)), trim_limit, _ptr(sums)))
        return sums


class DenseMap:
    """One dense map (== one reg_dense_map; o3d_slam::VoxelizedPointCloud) on the handle of `reg`: per-voxel running sums
    resident on the device, sorted by key.  It uses the stream and the working storage of `reg` and must be closed before
    it (close() of either order is safe here: the map keeps `reg` alive and closes itself first)."""

    def __init__(self, reg: Registration, voxel_size: float):
        self._lib = load_library()
        self.reg = reg
        self._m = C.c_void_p()
        reg._check(self._lib.reg_dense_map_create(reg._h, float(voxel_size), C.byref(self._m)))
        self.voxel_size = float(voxel_size)
        if not hasattr(reg, "_dense_maps"):
            reg._dense_maps = weakref.WeakSet()
        reg._dense_maps.add(self)

    def close(self):
        if getattr(self, "_m", None) and getattr(self.reg, "_h", None):
            self._lib.reg_dense_map_destroy(self._m)
        self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        self.reg._check(st)

    @staticmethod
    def _f64(a):
        return np.ascontiguousarray(a, np.float64).reshape(-1, 3) if a is not None else None

    def insert(self, xyz, normals=None, colors=None, T=None):
        """VoxelizedPointCloud::insert of T * cloud (T None: no transform).  Returns (n_voxels, n_new)."""
        x, nr, cl = self._f64(xyz), self._f64(normals), self._f64(colors)
        return self._insert(_ptr(x), _ptr(nr), _ptr(cl), x.shape[0], 0, T)

    def insert_device(self, xyz_ptr, n, nrm_ptr=None, col_ptr=None, T=None):
        """As insert with the fp64 arrays (n x 3 each) resident in HBM."""
        vp = lambda p: C.c_void_p(p) if p else None
        return self._insert(vp(xyz_ptr), vp(nrm_ptr), vp(col_ptr), n, 1, T)

    def _insert(self, x, nr, cl, n, on_device, T):
        nv, nn = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.reg_dense_map_insert(self._m, x, nr, cl, n, on_device, _T_in_f64(T), C.byref(nv), C.byref(nn)))
        return int(nv.value), int(nn.value)

    def insert_scan(self, xyz, params: DenseScanParams, normals=None, colors=None, T=None):
        """Submap.cpp:99-106: dense-map cropper, ColorRangeCropper, transform by T (map to sensor), insert.  Returns
        (n_inserted, n_voxels)."""
        x, nr, cl = self._f64(xyz), self._f64(normals), self._f64(colors)
        return self._insert_scan(_ptr(x), _ptr(nr), _ptr(cl), x.shape[0], 0, params, T)

    def insert_scan_device(self, xyz_ptr, n, params: DenseScanParams, nrm_ptr=None, col_ptr=None, T=None):
        """As insert_scan with the fp64 arrays (n x 3 each) resident in HBM."""
        vp = lambda p: C.c_void_p(p) if p else None
        return self._insert_scan(vp(xyz_ptr), vp(nrm_ptr), vp(col_ptr), n, 1, params, T)

    def _insert_scan(self, x, nr, cl, n, on_device, params, T):
        params.struct_size = C.sizeof(DenseScanParams)
        ni, nv = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.reg_dense_map_insert_scan(self._m, x, nr, cl, n, on_device, C.byref(params), _T_in_f64(T),
                                                        C.byref(ni), C.byref(nv)))
        return int(ni.value), int(nv.value)

    def carve(self, scan_xyz, sensor, params: "DenseCarveParams | None" = None, want_keys=True):
        """getKeysOfCarvedPoints + removeKey (helpers.cpp:360-390, Submap.cpp:153-156).  Returns the erased keys (k x 3
        int32, (x, y, z) per row, ascending key order), or their number with want_keys=False."""
        x = self._f64(scan_xyz)
        keys = np.empty((max(self.info().n_voxels, 1), 3), np.int32) if want_keys else None
        k = self._carve(_ptr(x), x.shape[0], 0, sensor, params, _ptr(keys))
        return keys[:k].copy() if want_keys else k

    def carve_device(self, scan_ptr, n_scan, sensor, params: "DenseCarveParams | None" = None, keys_ptr=None) -> int:
        """As carve with the fp64 scan and the int32 key output (n_voxels x 3, may be None) resident in HBM.  Returns
        n_removed."""
        vp = lambda p: C.c_void_p(p) if p else None
        return self._carve(vp(scan_ptr), n_scan, 1, sensor, params, vp(keys_ptr))

    def _carve(self, x, n, on_device, sensor, params, keys):
        p = params if params is not None else default_dense_carve_params()
        p.struct_size = C.sizeof(DenseCarveParams)
        sen = (C.c_double * 3)(*[float(v) for v in sensor])
        k = C.c_int64(0)
        self._check(self._lib.reg_dense_map_carve(self._m, x, n, on_device, sen, C.byref(p), keys, C.byref(k)))
        return int(k.value)

    def transform(self, T):
        """VoxelizedPointCloud::transform, literally: every position and normal SUM becomes R S + t; keys stay."""
        self._check(self._lib.reg_dense_map_transform(self._m, _T_in_f64(T)))

    def center(self) -> np.ndarray:
        """computeCenter (helpers.cpp:392-402)."""
        c = (C.c_double * 3)()
        self._check(self._lib.reg_dense_map_center(self._m, c))
        return np.array(c, np.float64)

    def clear(self):
        self._check(self._lib.reg_dense_map_clear(self._m))

    def info(self) -> DenseMapInfo:
        i = DenseMapInfo()
        i.struct_size = C.sizeof(DenseMapInfo)
        self._check(self._lib.reg_dense_map_get_info(self._m, C.byref(i)))
        return i

    def export(self, want_keys=True, want_counts=True):
        """toPointCloud (+ raw keys and counts): dict(xyz, normals, colors, keys, counts) in ascending key order; normals /
        colors are None while the map has not met the field."""
        i = self.info()
        n = int(i.n_voxels)
        f = lambda on, w, t: np.empty((max(n, 1), w), t) if on else None
        x, nr, cl = f(True, 3, np.float64), f(i.has_normals, 3, np.float64), f(i.has_colors, 3, np.float64)
        ky, ct = f(want_keys, 3, np.int32), f(want_counts, 1, np.int32)
        k = C.c_int64(0)
        self._check(self._lib.reg_dense_map_export(self._m, 0, _ptr(x), _ptr(nr), _ptr(cl), _ptr(ky), _ptr(ct), max(n, 1),
                                                   C.byref(k)))
        cut = lambda a: a[:int(k.value)] if a is not None else None
        return dict(xyz=cut(x), normals=cut(nr), colors=cut(cl), keys=cut(ky),
                    counts=cut(ct).reshape(-1) if ct is not None else None)

    def export_device(self, capacity_rows, xyz_ptr=None, nrm_ptr=None, col_ptr=None, keys_ptr=None, counts_ptr=None) -> int:
        """As export into arrays resident in HBM (capacity_rows rows each; any may be None).  Returns n_voxels."""
        vp = lambda p: C.c_void_p(p) if p else None
        k = C.c_int64(0)
        self._check(self._lib.reg_dense_map_export(self._m, 1, vp(xyz_ptr), vp(nrm_ptr), vp(col_ptr), vp(keys_ptr),
                                                   vp(counts_ptr), int(capacity_rows), C.byref(k)))
        return int(k.value)


class MapCloud:
    """One map cloud (== one reg_map_cloud; Submap::mapCloud_, the scan-matching map of a submap) on the handle of `reg`:
    fp64 points, optional normals and covariances resident on the device in the reference's point order.  It uses the
    stream and the working storage of `reg` and must be closed before it (close() of either order is safe here: the map
    keeps `reg` alive and closes itself first)."""

    def __init__(self, reg: Registration, params: "MapCloudParams | None" = None):
        self._lib = load_library()
        self.reg = reg
        self._m = C.c_void_p()
        p = params if params is not None else default_map_cloud_params()
        p.struct_size = C.sizeof(MapCloudParams)
        reg._check(self._lib.reg_map_cloud_create(reg._h, C.byref(p), C.byref(self._m)))
        self.params = p
        if not hasattr(reg, "_map_clouds"):
            reg._map_clouds = weakref.WeakSet()
        reg._map_clouds.add(self)

    def close(self):
        if getattr(self, "_m", None) and getattr(self.reg, "_h", None):
            self._lib.reg_map_cloud_destroy(self._m)
        self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        self.reg._check(st)

    @staticmethod
    def _f64(a, width=3):
        return np.ascontiguousarray(a, np.float64).reshape(-1, width) if a is not None else None

    def set(self, xyz, normals=None, covs=None, voxel_size=0.0):
        """The isUseInitialMap_ branch (Submap.cpp:47-52): the map becomes the cloud, voxel-down-sampled when voxel_size > 0;
        not transformed, the scan counter untouched.  Returns the rows of the map."""
        x, nr, cv = self._f64(xyz), self._f64(normals), self._f64(covs, 9)
        self._check(self._lib.reg_map_cloud_set(self._m, _ptr(x), _ptr(nr), _ptr(cv), x.shape[0], 0, float(voxel_size)))
        return int(self.info().n_rows)

    def set_device(self, xyz_ptr, n, nrm_ptr=None, cov_ptr=None, voxel_size=0.0):
        """As set with the fp64 arrays resident in HBM."""
        vp = lambda p: C.c_void_p(p) if p else None
        self._check(self._lib.reg_map_cloud_set(self._m, vp(xyz_ptr), vp(nrm_ptr), vp(cov_ptr), n, 1, float(voxel_size)))
        return int(self.info().n_rows)

    def insert_scan(self, raw_xyz, scan_xyz, T, scan_normals=None, scan_covs=None, perform_carving=True) -> MapCloudInsertResult:
        """Submap::insertScan (Submap.cpp:54-95): carve with the transformed raw scan, append the transformed pre-processed
        scan, move the cropper to the translation of T (map to sensor), voxelise within it."""
        r = self._f64(raw_xyz)
        x, nr, cv = self._f64(scan_xyz), self._f64(scan_normals), self._f64(scan_covs, 9)
        return self._insert_scan(_ptr(r), r.shape[0] if r is not None else 0, _ptr(x), _ptr(nr), _ptr(cv), x.shape[0], 0, T,
                                 perform_carving)

    def insert_scan_device(self, raw_ptr, n_raw, scan_ptr, n_scan, T, scan_nrm_ptr=None, scan_cov_ptr=None,
                           perform_carving=True) -> MapCloudInsertResult:
        """As insert_scan with the fp64 arrays resident in HBM (the merge cloud of process_scan_device, for instance)."""
        vp = lambda p: C.c_void_p(p) if p else None
        return self._insert_scan(vp(raw_ptr), n_raw, vp(scan_ptr), vp(scan_nrm_ptr), vp(scan_cov_ptr), n_scan, 1, T,
                                 perform_carving)

    def _insert_scan(self, r, n_raw, x, nr, cv, n, on_device, T, carve):
        res = MapCloudInsertResult()
        res.struct_size = C.sizeof(MapCloudInsertResult)
        self._check(self._lib.reg_map_cloud_insert_scan(self._m, r, n_raw, x, nr, cv, n, on_device, _T_in_f64(T),
                                                        int(bool(carve)), C.byref(res)))
        return res

    def set_target(self, crop=None) -> int:
        """cropSubmap + open3dToPointmatcher + initReference from the resident arrays onto the handle of `reg`: exactly
        Registration.set_target_f64_device of the map.  Returns the rows kept; target_source_indices() indexes map rows."""
        c = Registration._crop_struct(crop)
        kept = C.c_int64(0)
        st = self._lib.reg_map_cloud_set_target(self._m, C.byref(c) if c is not None else None, C.byref(kept))
        self.reg.n_target_kept = int(kept.value)
        self._check(st)
        return self.reg.n_target_kept

    def transform(self, T):
        """PointCloud::Transform as Submap::transform applies it to mapCloud_."""
        self._check(self._lib.reg_map_cloud_transform(self._m, _T_in_f64(T)))

    def center(self) -> np.ndarray:
        """GetCenter: the sequential sum of the rows divided by their number."""
        c = (C.c_double * 3)()
        self._check(self._lib.reg_map_cloud_center(self._m, c))
        return np.array(c, np.float64)

    def clear(self):
        self._check(self._lib.reg_map_cloud_clear(self._m))

    def info(self) -> MapCloudInfo:
        i = MapCloudInfo()
        i.struct_size = C.sizeof(MapCloudInfo)
        self._check(self._lib.reg_map_cloud_get_info(self._m, C.byref(i)))
        return i

    def export(self):
        """dict(xyz, normals, covs) in the map's row order; normals / covs are None when the map lacks the field."""
        i = self.info()
        n = int(i.n_rows)
        f = lambda on, w: np.empty((max(n, 1), w), np.float64) if on else None
        x, nr, cv = f(True, 3), f(i.has_normals, 3), f(i.has_covariances, 9)
        k = C.c_int64(0)
        self._check(self._lib.reg_map_cloud_export(self._m, 0, _ptr(x), _ptr(nr), _ptr(cv), max(n, 1), C.byref(k)))
        cut = lambda a: a[:int(k.value)] if a is not None else None
        return dict(xyz=cut(x), normals=cut(nr), covs=cut(cv))

    def export_device(self, capacity_rows, xyz_ptr=None, nrm_ptr=None, cov_ptr=None) -> int:
        """As export into arrays resident in HBM (capacity_rows rows each; any may be None).  Returns n_rows."""
        vp = lambda p: C.c_void_p(p) if p else None
        k = C.c_int64(0)
        self._check(self._lib.reg_map_cloud_export(self._m, 1, vp(xyz_ptr), vp(nrm_ptr), vp(cov_ptr), int(capacity_rows),
                                                   C.byref(k)))
        return int(k.value)


class Submaps:
    """One submap collection (== one reg_submaps; o3d_slam::SubmapCollection) on the handle of `reg`: every submap's map
    cloud, its occupancy keys and the overlap ring stay on the device; the active index, the queues and the adjacency matrix
    live on the host inside the library.  It uses the stream and the working storage of `reg` and must be closed before it
    (close() of either order is safe here: the object keeps `reg` alive and closes itself first)."""

    def __init__(self, reg: Registration, params: "SubmapsParams | None" = None):
        self._lib = load_library()
        self.reg = reg
        self._s = C.c_void_p()
        p = params if params is not None else default_submaps_params()
        p.struct_size = C.sizeof(SubmapsParams)
        reg._check(self._lib.reg_submaps_create(reg._h, C.byref(p), C.byref(self._s)))
        self.params = p
        if not hasattr(reg, "_submaps"):
            reg._submaps = weakref.WeakSet()
        reg._submaps.add(self)

    def close(self):
        if getattr(self, "_s", None) and getattr(self.reg, "_h", None):
            self._lib.reg_submaps_destroy(self._s)
        self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        self.reg._check(st)

    def info(self) -> SubmapsInfo:
        i = SubmapsInfo()
        i.struct_size = C.sizeof(SubmapsInfo)
        self._check(self._lib.reg_submaps_get_info(self._s, C.byref(i)))
        return i

    def submap_info(self, idx) -> SubmapInfo:
        i = SubmapInfo()
        i.struct_size = C.sizeof(SubmapInfo)
        self._check(self._lib.reg_submaps_get_submap_info(self._s, int(idx), C.byref(i)))
        return i

    def set_map_to_sensor(self, T):
        self._check(self._lib.reg_submaps_set_map_to_sensor(self._s, _T_in_f64(T)))

    def insert_scan(self, raw_xyz, scan_xyz, T, stamp_ns, scan_normals=None, scan_covs=None) -> SubmapsInsertResult:
        """SubmapCollection::insertScan: the scan enters the ring, updateActiveSubmap decides, the scan is merged (and on a
        change of the active submap the ring is drained into the new one)."""
        f = MapCloud._f64
        r, x, nr, cv = f(raw_xyz), f(scan_xyz), f(scan_normals), f(scan_covs, 9)
        return self._insert(_ptr(r), r.shape[0] if r is not None else 0, _ptr(x), _ptr(nr), _ptr(cv), x.shape[0], 0, T, stamp_ns)

    def insert_scan_device(self, raw_ptr, n_raw, scan_ptr, n_scan, T, stamp_ns, scan_nrm_ptr=None,
                           scan_cov_ptr=None) -> SubmapsInsertResult:
        """As insert_scan with the fp64 arrays resident in HBM."""
        vp = lambda p: C.c_void_p(p) if p else None
        return self._insert(vp(raw_ptr), n_raw, vp(scan_ptr), vp(scan_nrm_ptr), vp(scan_cov_ptr), n_scan, 1, T, stamp_ns)

    def _insert(self, r, n_raw, x, nr, cv, n, on_device, T, stamp_ns):
        res = SubmapsInsertResult()
        res.struct_size = C.sizeof(SubmapsInsertResult)
        self._check(self._lib.reg_submaps_insert_scan(self._s, r, n_raw, x, nr, cv, n, on_device, _T_in_f64(T), int(stamp_ns),
                                                      C.byref(res)))
        return res

    def force_new_submap(self) -> SubmapsInsertResult:
        res = SubmapsInsertResult()
        res.struct_size = C.sizeof(SubmapsInsertResult)
        self._check(self._lib.reg_submaps_force_new_submap(self._s, C.byref(res)))
        return res

    def compute_features(self, idx, now_seconds, params: "SubmapFeatureParams | None" = None):
        """Submap::computeFeatures on the caller's clock.  Without params: the gate and the occupancy keys; returns whether it
        ran.  With params also the sparse cloud, its normals and FPFH features, computed on the device from the resident map:
        returns None when the gate held, else dict(xyz n x 3 float32, normals n x 3 float32, fpfh n x 33 float64)."""
        done = C.c_int32(0)
        if params is None:
            self._check(self._lib.reg_submaps_compute_features(self._s, int(idx), float(now_seconds), None, 0, None, None, None, 0,
                                                               None, C.byref(done)))
            return bool(done.value)
        cap = max(int(self.submap_info(idx).n_rows), 1)
        x, nr, f = np.empty((cap, 3), np.float32), np.empty((cap, 3), np.float32), np.empty((cap, 33), np.float64)
        n = C.c_int64(0)
        params.struct_size = C.sizeof(SubmapFeatureParams)
        self._check(self._lib.reg_submaps_compute_features(self._s, int(idx), float(now_seconds), C.byref(params), 0, _ptr(x), _ptr(nr),
                                                           _ptr(f), cap, C.byref(n), C.byref(done)))
        if not done.value:
            return None
        k = int(n.value)
        return dict(xyz=x[:k].copy(), normals=nr[:k].copy(), fpfh=f[:k].copy())

    def compute_features_device(self, idx, now_seconds, params: "SubmapFeatureParams", capacity_rows, xyz_ptr=None, nrm_ptr=None,
                                fpfh_ptr=None):
        """As compute_features with the outputs resident in HBM.  Returns (ran, sparse rows)."""
        vp = lambda p: C.c_void_p(p) if p else None
        done, n = C.c_int32(0), C.c_int64(0)
        params.struct_size = C.sizeof(SubmapFeatureParams)
        self._check(self._lib.reg_submaps_compute_features(self._s, int(idx), float(now_seconds), C.byref(params), 1, vp(xyz_ptr),
                                                           vp(nrm_ptr), vp(fpfh_ptr), int(capacity_rows), C.byref(n), C.byref(done)))
        return bool(done.value), int(n.value)

    def keys(self, idx) -> np.ndarray:
        """The occupancy keys of a submap, ascending uint64."""
        n = C.c_int64(0)
        self._check(self._lib.reg_submaps_get_keys(self._s, int(idx), None, 0, C.byref(n)))
        out = np.empty(max(int(n.value), 1), np.uint64)
        self._check(self._lib.reg_submaps_get_keys(self._s, int(idx), _ptr(out), out.shape[0], C.byref(n)))
        return out[:int(n.value)]

    def switch_fitness(self, idx, scan_xyz, T):
        """(count, fitness) of the revisiting check of a host scan at pose T against submap idx."""
        x = MapCloud._f64(scan_xyz)
        return self._fitness(idx, _ptr(x) if x.shape[0] else None, x.shape[0], 0, T)

    def switch_fitness_device(self, idx, scan_ptr, n, T):
        return self._fitness(idx, C.c_void_p(scan_ptr) if scan_ptr else None, n, 1, T)

    def _fitness(self, idx, x, n, on_device, T):
        c, f = C.c_int64(0), C.c_double(0.0)
        self._check(self._lib.reg_submaps_switch_fitness(self._s, int(idx), x, n, on_device, _T_in_f64(T), C.byref(c), C.byref(f)))
        return int(c.value), float(f.value)

    def set_target(self, crop=None) -> int:
        """cropSubmap + initReference of the ACTIVE submap onto the handle of `reg`."""
        c = Registration._crop_struct(crop)
        kept = C.c_int64(0)
        st = self._lib.reg_submaps_set_target(self._s, C.byref(c) if c is not None else None, C.byref(kept))
        self.reg.n_target_kept = int(kept.value)
        self._check(st)
        return self.reg.n_target_kept

    def _export(self, n, call):
        p = self.params.map
        f = lambda on, w: np.empty((max(n, 1), w), np.float64) if on else None
        x, nr, cv = f(True, 3), f(p.has_normals, 3), f(p.has_covariances, 9)
        k = C.c_int64(0)
        self._check(call(_ptr(x), _ptr(nr), _ptr(cv), max(n, 1), C.byref(k)))
        cut = lambda a: a[:int(k.value)] if a is not None else None
        return dict(xyz=cut(x), normals=cut(nr), covs=cut(cv))

    def export_submap(self, idx):
        """dict(xyz, normals, covs) of one submap's map cloud in its row order."""
        return self._export(int(self.submap_info(idx).n_rows),
                            lambda x, nr, cv, cap, k: self._lib.reg_submaps_export_submap(self._s, int(idx), 0, x, nr, cv, cap, k))

    def export(self):
        """Mapper::getAssembledMapPointCloud: every submap's rows in submap order."""
        return self._export(int(self.info().total_points),
                            lambda x, nr, cv, cap, k: self._lib.reg_submaps_export(self._s, 0, x, nr, cv, cap, k))

    def export_device(self, capacity_rows, xyz_ptr=None, nrm_ptr=None, cov_ptr=None) -> int:
        vp = lambda p: C.c_void_p(p) if p else None
        k = C.c_int64(0)
        self._check(self._lib.reg_submaps_export(self._s, 1, vp(xyz_ptr), vp(nrm_ptr), vp(cov_ptr), int(capacity_rows), C.byref(k)))
        return int(k.value)

    def transform(self, ids, dTs):
        """SubmapCollection::transform: ids[k] receives dTs[k]; the others follow their parents (reg_host_submaps_transform_plan)."""
        i = np.ascontiguousarray(ids, np.int32).reshape(-1)
        t = np.ascontiguousarray([np.asarray(T, np.float64).reshape(4, 4).T for T in dTs], np.float64).reshape(-1)
        self._check(self._lib.reg_submaps_transform(self._s, _ptr(i) if i.size else None, _ptr(t) if i.size else None, int(i.size)))

    def add_loop_closure_edges(self, pairs):
        p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        a, b = np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])
        self._check(self._lib.reg_submaps_add_loop_closure_edges(self._s, _ptr(a), _ptr(b), int(p.shape[0])))

    def adjacency(self):
        """(adj n x n uint8, marks n int32: -1 no entry, 0, 1)."""
        n = int(self.info().n_submaps)
        adj, marks = np.zeros((n, n), np.uint8), np.zeros(n, np.int32)
        self._check(self._lib.reg_submaps_get_adjacency(self._s, _ptr(adj), _ptr(marks), n))
        return adj, marks

    def _pop(self, fn, n):
        ids, stamps, k = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64), C.c_int32(0)
        self._check(fn(self._s, _ptr(ids), _ptr(stamps), ids.shape[0], C.byref(k)))
        return [(int(a), int(b)) for a, b in zip(ids[:k.value], stamps[:k.value])]

    def pop_finished(self):
        return self._pop(self._lib.reg_submaps_pop_finished, int(self.info().n_finished))

    def pop_loop_closure_candidates(self):
        return self._pop(self._lib.reg_submaps_pop_loop_closure_candidates, int(self.info().n_loop_closure_candidates))

    def push_loop_closure_candidate(self, idx, stamp_ns):
        self._check(self._lib.reg_submaps_push_loop_closure_candidate(self._s, int(idx), int(stamp_ns)))

    def loop_closure_candidates(self, last_finished) -> list:
        n = int(self.info().n_submaps)
        out, k = np.zeros(n, np.int32), C.c_int32(0)
        self._check(self._lib.reg_submaps_loop_closure_candidates(self._s, int(last_finished), _ptr(out), n, C.byref(k)))
        return out[:k.value].tolist()

    def odometry_constraint_pairs(self, candidates=None, existing=()) -> list:
        n = int(self.info().n_submaps)
        c = None if candidates is None else np.ascontiguousarray(candidates, np.int32).reshape(-1)
        e = np.ascontiguousarray(existing, np.int32).reshape(-1, 2)
        cap = max(n, 0 if c is None else c.size, 1)
        out, k = np.zeros((cap, 2), np.int32), C.c_int32(0)
        self._check(self._lib.reg_submaps_odometry_constraint_pairs(
            self._s, _ptr(c) if c is not None else None, 0 if c is None else int(c.size), _ptr(e) if e.size else None,
            int(e.shape[0]), _ptr(out), cap, C.byref(k)))
        return [tuple(r) for r in out[:k.value].tolist()]


class Odometry:
    """One LidarOdometry (== one reg_odometry; Odometry.cpp) on the handle of `reg`: the previous pre-processed cloud stays
    on the device between scans, the cumulative pose on the host inside the library.  It uses the stream and the working
    storage of `reg`, installs its own reference and reading there, and must be closed before it (close() of either order is
    safe here: the object keeps `reg` alive and closes itself first).  Every row count comes from the library."""

    def __init__(self, reg: Registration, params: "OdometryParams | None" = None):
        self._lib = load_library()
        self.reg = reg
        self._o = C.c_void_p()
        p = params if params is not None else default_odometry_params()
        p.struct_size = C.sizeof(OdometryParams)
        reg._check(self._lib.reg_odometry_create(reg._h, C.byref(p), C.byref(self._o)))
        self.params = p
        if not hasattr(reg, "_odometries"):
            reg._odometries = weakref.WeakSet()
        reg._odometries.add(self)

    def close(self):
        if getattr(self, "_o", None) and getattr(self.reg, "_h", None):
            self._lib.reg_odometry_destroy(self._o)
        self._o = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        self.reg._check(st)

    def add_scan(self, xyz, timestamp, normals=None) -> OdometryResult:
        """addRangeScan: n x 3 fp64 points (and normals) of a scan in the sensor frame, the stamp in nanoseconds."""
        x = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        nr = np.ascontiguousarray(normals, np.float64).reshape(-1, 3) if normals is not None else None
        return self._add_scan(_ptr(x), _ptr(nr), x.shape[0], 0, timestamp)

    def add_scan_device(self, xyz_ptr, n, timestamp, nrm_ptr=None) -> OdometryResult:
        """As add_scan with the fp64 arrays resident in HBM."""
        vp = lambda p: C.c_void_p(p) if p else None
        return self._add_scan(vp(xyz_ptr), vp(nrm_ptr), n, 1, timestamp)

    def _add_scan(self, x, nr, n, on_device, timestamp):
        res = OdometryResult()
        res.struct_size = C.sizeof(OdometryResult)
        st = self._lib.reg_odometry_add_scan(self._o, x, nr, n, on_device, int(timestamp), C.byref(res))
        self.last_result = res
        self._check(st)
        return res

    def set_initial_transform(self, T) -> bool:
        """setInitialTransform: False (nothing changes) while an earlier one is still pending."""
        applied = C.c_int32(0)
        self._check(self._lib.reg_odometry_set_initial_transform(self._o, _T_in_f64(T), C.byref(applied)))
        return bool(applied.value)

    def clear(self):
        self._check(self._lib.reg_odometry_clear(self._o))

    def info(self) -> OdometryInfo:
        i = OdometryInfo()
        i.struct_size = C.sizeof(OdometryInfo)
        self._check(self._lib.reg_odometry_get_info(self._o, C.byref(i)))
        return i

    def cumulative(self) -> np.ndarray:
        """odomToRangeSensorCumulative_ as a 4 x 4 float64 matrix."""
        return np.array(self.info().cumulative, np.float64).reshape(4, 4).T.copy()

    def export_cloud(self):
        """getPreProcessedCloud: dict(xyz, normals, covs); normals / covs are None when the cloud lacks the field."""
        i = self.info()
        n = int(i.n_rows)
        f = lambda on, w: np.empty((max(n, 1), w), np.float64) if on else None
        x, nr, cv = f(True, 3), f(i.has_normals, 3), f(i.has_covariances, 9)
        k = C.c_int64(0)
        self._check(self._lib.reg_odometry_export_cloud(self._o, 0, _ptr(x), _ptr(nr), _ptr(cv), max(n, 1), C.byref(k)))
        cut = lambda a: a[:int(k.value)] if a is not None else None
        return dict(xyz=cut(x), normals=cut(nr), covs=cut(cv))

    def export_cloud_device(self, capacity_rows, xyz_ptr=None, nrm_ptr=None, cov_ptr=None) -> int:
        """As export_cloud into arrays resident in HBM (capacity_rows rows each; any may be None).  Returns n_rows."""
        vp = lambda p: C.c_void_p(p) if p else None
        k = C.c_int64(0)
        self._check(self._lib.reg_odometry_export_cloud(self._o, 1, vp(xyz_ptr), vp(nrm_ptr), vp(cov_ptr), int(capacity_rows),
                                                        C.byref(k)))
        return int(k.value)

    def correspondences(self):
        """(ids, d2) of the last registration of this object: one row per point of the then previous cloud, ids into the
        then new cloud (-1: none)."""
        n = int(self.last_result.n_source) if getattr(self, "last_result", None) is not None else 0
        ids, d2 = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.float32)
        self._check(self._lib.reg_odometry_get_correspondences(self._o, ids.shape[0], _ptr(ids), _ptr(d2)))
        return ids[:n], d2[:n]


class PoseGraph:
    """One pose graph (== one reg_pose_graph) on the handle of `reg`: Open3D's GlobalOptimization as
    OptimizationProblem::solve runs it.  The graph lives on the host inside the library; a pass uploads it and works on the
    stream of `reg`; the dense factor buffer is sized on first use and kept.  All matrices are row-major fp64."""

    def __init__(self, reg: "Registration", params: "PoseGraphParams | None" = None):
        self._lib = load_library()
        self.reg = reg
        self._g = C.c_void_p()
        p = params if params is not None else default_pose_graph_params()
        p.struct_size = C.sizeof(PoseGraphParams)
        reg._check(self._lib.reg_pose_graph_create(reg._h, C.byref(p), C.byref(self._g)))
        self.params = p
        if not hasattr(reg, "_pose_graphs"):
            reg._pose_graphs = weakref.WeakSet()
        reg._pose_graphs.add(self)

    def close(self):
        if getattr(self, "_g", None) and getattr(self.reg, "_h", None):
            self._lib.reg_pose_graph_destroy(self._g)
        self._g = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        self.reg._check(st)

    def set(self, poses, src, tgt, X, info, uncertain, confidence=None):
        """poses n x 4 x 4; per edge source and target ids, X (4 x 4), info (6 x 6), uncertain, confidence (None: 1)."""
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 16)
        s = np.ascontiguousarray(src, np.int32).reshape(-1)
        t = np.ascontiguousarray(tgt, np.int32).reshape(-1)
        E = s.shape[0]
        Xa = np.ascontiguousarray(X, np.float64).reshape(E, 16)
        Ia = np.ascontiguousarray(info, np.float64).reshape(E, 36)
        u = np.ascontiguousarray(np.asarray(uncertain).astype(bool), np.int32).reshape(E)
        c = np.ascontiguousarray(confidence, np.float64).reshape(E) if confidence is not None else None
        if t.shape[0] != E:
            raise ValueError("src and tgt differ in length")
        e = lambda a: _ptr(a) if E else None
        self._check(self._lib.reg_pose_graph_set(self._g, _ptr(P), P.shape[0], e(s), e(t), e(Xa), e(Ia), e(u),
                                                 e(c) if c is not None else None, E))

    def clear(self):
        self._check(self._lib.reg_pose_graph_clear(self._g))

    def info(self) -> PoseGraphInfo:
        i = PoseGraphInfo()
        i.struct_size = C.sizeof(PoseGraphInfo)
        self._check(self._lib.reg_pose_graph_get_info(self._g, C.byref(i)))
        return i

    def linearize(self, want_H=True):
        """reg_pose_graph_linearize at the current poses and confidences: dict(H, b, zeta, residual, weight)."""
        i = self.info()
        M, E = 6 * int(i.n_nodes), int(i.n_edges)
        H = np.empty((M, M)) if want_H else None
        b, zeta = np.empty(M), np.empty((max(E, 1), 6))
        r, w = C.c_double(0.0), C.c_double(0.0)
        self._check(self._lib.reg_pose_graph_linearize(self._g, _ptr(H), _ptr(b), _ptr(zeta), C.byref(r), C.byref(w)))
        return dict(H=H, b=b, zeta=zeta[:E], residual=float(r.value), weight=float(w.value))

    def optimize(self) -> PoseGraphResult:
        """One Levenberg-Marquardt pass on the graph as it stands."""
        res = PoseGraphResult()
        res.struct_size = C.sizeof(PoseGraphResult)
        self._check(self._lib.reg_pose_graph_optimize(self._g, C.byref(res)))
        return res

    def global_optimize(self):
        """GlobalOptimization: pass, prune, pass, prune, reference compensation.  Returns the two passes' results."""
        res = (PoseGraphResult * 2)()
        for r in res:
            r.struct_size = C.sizeof(PoseGraphResult)
        self._check(self._lib.reg_pose_graph_global_optimize(self._g, res))
        return [res[0], res[1]]

    def get(self):
        """dict(poses n x 4 x 4, src, tgt, confidence, ids) of the graph as it stands; ids: every edge's index in the list
        set() received."""
        i = self.info()
        n, E = int(i.n_nodes), int(i.n_edges)
        P = np.empty((max(n, 1), 4, 4))
        s, t, c = np.empty(max(E, 1), np.int32), np.empty(max(E, 1), np.int32), np.empty(max(E, 1))
        k = C.c_int64(0)
        self._check(self._lib.reg_pose_graph_get(self._g, P.shape[0], _ptr(P), s.shape[0], _ptr(s), _ptr(t), _ptr(c),
                                                 C.byref(k)))
        ids = np.empty(max(E, 1), np.int32)
        self._check(self._lib.reg_pose_graph_get_edge_ids(self._g, ids.shape[0], _ptr(ids)))
        E = int(k.value)
        return dict(poses=P[:n], src=s[:E], tgt=t[:E], confidence=c[:E], ids=ids[:E])


def debug_spd_solve(reg: "Registration", A, b):
    """reg_debug_spd_solve_f64: (x, status) of the pose graph's dense solver on A x = b; x is None when a pivot fails
    (status = 1 + its row)."""
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64).reshape(-1)
    x = np.empty_like(b)
    status = C.c_int32(0)
    st = load_library().reg_debug_spd_solve_f64(reg._h, b.shape[0], _ptr(A), _ptr(b), _ptr(x), C.byref(status))
    if st == 4:   # REG_BAD_TRANSFORM: a pivot
        return None, int(status.value)
    reg._check(st)
    return x, int(status.value)


def dist_unique_id() -> bytes:
    """ncclGetUniqueId (rank 0); hand the 128 bytes to the other ranks by any means."""
    buf = C.create_string_buffer(DIST_ID_BYTES)
    st = load_library().reg_dist_get_unique_id(buf)
    if st != 0:
        raise RegError(st, "reg_dist_get_unique_id (is librccl loadable?)")
    return buf.raw


class Steer:
    """The steering state machine of reg_dist_register (pure host code in the library: no device needed)."""

    def __init__(self, trimming, fixed_iters, max_iter, settle_tol=0.05, can_fuse=True):
        self._lib = load_library()
        self._s = C.c_void_p(self._lib.reg_dist_steer_create(int(bool(trimming)), int(fixed_iters), int(max_iter),
                                                             float(settle_tol), int(bool(can_fuse))))

    def step(self, reply: "DistReply | None" = None) -> DistAction:
        return self._lib.reg_dist_steer_step(self._s, C.byref(reply) if reply is not None else None)

    def counts(self):
        g, f, s = C.c_int32(), C.c_int32(), C.c_int32()
        self._lib.reg_dist_steer_counts(self._s, C.byref(g), C.byref(f), C.byref(s))
        return g.value, f.value, s.value

    def __del__(self):
        try:
            if self._s:
                self._lib.reg_dist_steer_destroy(self._s)
                self._s = None
        except Exception:
            pass


def solve_update(params: RegParams, sums, T_iter):
    """R8 + T_iter update on the host (identical on every rank)."""
    lib = load_library()
    s = np.ascontiguousarray(sums, np.float64)
    To = np.zeros(16, np.float32)
    rank = C.c_int32()
    st = lib.reg_solve_update(C.byref(params), _ptr(s), _ptr(_T_in(T_iter)), _ptr(To), C.byref(rank))
    if st != 0:
        raise RegError(st, "reg_solve_update")
    return _T_out(To), rank.value


def host_solve6(A, b):
    x = np.zeros(6, np.float32)
    rank = load_library().reg_host_solve6(_ptr(_f32(A).reshape(36)), _ptr(_f32(b)), _ptr(x))
    return x, rank


def host_solve6_xicp(A, b, flags):
    x = np.zeros(6, np.float32)
    f = np.ascontiguousarray(flags, np.int32)
    rank = load_library().reg_host_solve6_xicp(_ptr(_f32(A).reshape(36)), _ptr(_f32(b)), _ptr(f), _ptr(x))
    return x, rank


def host_x_to_T(x):
    T = np.zeros(16, np.float32)
    load_library().reg_host_x_to_T(_ptr(_f32(x)), _ptr(T))
    return _T_out(T)


def host_centroid(xyz):
    xyz = _f32(xyz)
    out = np.zeros(3, np.float32)
    load_library().reg_host_centroid(_ptr(xyz), xyz.shape[1], xyz.shape[0], _ptr(out))
    return out


def host_o3d_update(cost, sums):
    """Update matrix U (4x4 float64, math layout; T <- U T) and rank of one iteration of an Open3D cost from its reduced
    32-double record -- the arithmetic of the update kernel, on the host (reg_host_o3d_update)."""
    s = np.ascontiguousarray(sums, np.float64).reshape(32)
    U = np.zeros(16, np.float64)
    rank = C.c_int32()
    st = load_library().reg_host_o3d_update(int(cost), _ptr(s), _ptr(U), C.byref(rank))
    if st != 0:
        raise RegError(st, "reg_host_o3d_update")
    return U.reshape(4, 4).T.copy(), rank.value


def host_tail_plan(n, cus=256, tile=0):
    """Launch plan of the persistent tail kernel for an n-point reading: (usable, workgroups, workgroups per XCD class, reading
    points per XCD class) -- host-only (reg_host_tail_plan).  tile: octets per XCD tile (0: contiguous eighths)."""
    lib = load_library()
    lib.reg_host_tail_plan.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    lib.reg_host_tail_plan.restype = None
    out = (C.c_int32 * 4)()
    lib.reg_host_tail_plan(int(n), int(cus), int(tile), out)
    return bool(out[0]), int(out[1]), int(out[2]), int(out[3])


def host_predict_band(limit, prev=math.inf, prev2=math.inf, last_count=0, last_lo=math.inf, last_hi=math.inf, debug_narrow=0):
    """The band [lo, hi) every loop path predicts for the next trimmed limit from the last three limits (newest first; inf:
    none) and the population / edges of the last band (0 / inf: unknown) -- host-only (reg_host_predict_band).  float32."""
    lib = load_library()
    lib.reg_host_predict_band.argtypes = [C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_float, C.c_float, C.c_int32,
                                          C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.reg_host_predict_band.restype = None
    out = (C.c_float * 2)()
    lib.reg_host_predict_band(float(limit), float(prev), float(prev2), int(last_count), float(last_lo), float(last_hi),
                              int(debug_narrow), out, None)
    return np.float32(out[0]), np.float32(out[1])


def host_band_constants():
    """Constants of the band predictor as compiled: dict of kTailBandCap, kTailWideRel, floor, ratio_max, centre_gain,
    geom_rel, guard_frac, forced_wide."""
    lib = load_library()
    lib.reg_host_predict_band.argtypes = [C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_float, C.c_float, C.c_int32,
                                          C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.reg_host_predict_band.restype = None
    c = (C.c_float * 8)()
    lib.reg_host_predict_band(math.inf, math.inf, math.inf, 0, math.inf, math.inf, 0, None, c)
    names = ("band_cap", "wide_rel", "floor", "ratio_max", "centre_gain", "geom_rel", "guard_frac", "forced_wide")
    return {k: float(np.float32(v)) for k, v in zip(names, c)}


# ---- pose-graph constraints from the resident submap collection (include/o3dslam_reg.h) -------------------------
class ConstraintParams(C.Structure):
    """reg_constraint_params (include/o3dslam_reg.h): the arguments of buildConstraint / the loop-closure refinement."""
    _fields_ = [("struct_size", C.c_int32), ("cost", C.c_int32), ("max_iteration", C.c_int32), ("is_compute_overlap", C.c_int32),
                ("skip_refinement", C.c_int32), ("estimate_information", C.c_int32), ("overlap_voxel_size", C.c_double),
                ("icp_max_correspondence_distance", C.c_double), ("information_max_distance", C.c_double)]


class ConstraintResult(C.Structure):
    """reg_constraint_result (include/o3dslam_reg.h); T_matrix() / information_matrix() give the 4 x 4 and 6 x 6 math layout."""
    _fields_ = [("struct_size", C.c_int32), ("source", C.c_int32), ("target", C.c_int32), ("iterations", C.c_int32),
                ("converged", C.c_int32), ("refined", C.c_int32), ("information_estimated", C.c_int32), ("reserved", C.c_int32),
                ("n_source_selected", C.c_int64), ("n_target_selected", C.c_int64), ("n_info_pairs", C.c_int64),
                ("fitness", C.c_double), ("inlier_rmse", C.c_double), ("T", C.c_double * 16), ("information", C.c_double * 36)]

    def T_matrix(self) -> np.ndarray:
        return np.array(self.T, np.float64).reshape(4, 4).T.copy()

    def information_matrix(self) -> np.ndarray:
        return np.array(self.information, np.float64).reshape(6, 6)


EXPORTS += ["reg_default_odometry_constraint_params", "reg_check_constraint_params", "reg_constraints_struct_sizes",
            "reg_submaps_build_constraint", "reg_submaps_compute_odometry_constraints", "reg_submaps_get_odometry_constraints",
            "reg_submaps_clear_odometry_constraints", "reg_submaps_get_features", "reg_host_registration_consistent"]
CONSISTENCY_COMPONENTS = ("roll", "pitch", "yaw", "x", "y", "z")   # bit k of reg_host_registration_consistent's mask
_constraints_bound = False


def _constraints_lib():
    """The library with the prototypes of this section set."""
    global _constraints_bound
    lib = load_library()
    if not _constraints_bound:
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        pd = C.POINTER(C.c_double)
        lib.reg_default_odometry_constraint_params.argtypes = [vp, C.c_int, C.POINTER(ConstraintParams)]
        lib.reg_check_constraint_params.argtypes = [C.POINTER(ConstraintParams)]
        lib.reg_constraints_struct_sizes.argtypes = [C.POINTER(i32)]
        lib.reg_constraints_struct_sizes.restype = None
        lib.reg_submaps_build_constraint.argtypes = [vp, i32, i32, C.POINTER(ConstraintParams), pd, C.POINTER(ConstraintResult)]
        lib.reg_submaps_compute_odometry_constraints.argtypes = [vp, vp, i32, C.POINTER(ConstraintParams), C.POINTER(i32)]
        lib.reg_submaps_get_odometry_constraints.argtypes = [vp, i32, vp, vp, vp, vp, vp, C.POINTER(i32)]
        lib.reg_submaps_clear_odometry_constraints.argtypes = [vp]
        lib.reg_submaps_get_features.argtypes = [vp, i32, C.c_int, vp, vp, vp, vp, i64, C.POINTER(i64)]
        lib.reg_host_registration_consistent.argtypes = [pd, pd, C.POINTER(i32)]
        _constraints_bound = True
    return lib


def constraint_params(cost=COST_O3D_P2PL, max_iteration=100, is_compute_overlap=True, skip_refinement=False,
                      estimate_information=True, overlap_voxel_size=0.0, icp_max_correspondence_distance=0.0,
                      information_max_distance=None) -> ConstraintParams:
    """A reg_constraint_params; information_max_distance defaults to icp_max_correspondence_distance (buildConstraint)."""
    p = ConstraintParams()
    p.struct_size = C.sizeof(ConstraintParams)
    p.cost, p.max_iteration = int(cost), int(max_iteration)
    p.is_compute_overlap, p.skip_refinement = int(bool(is_compute_overlap)), int(bool(skip_refinement))
    p.estimate_information = int(bool(estimate_information))
    p.overlap_voxel_size = float(overlap_voxel_size)
    p.icp_max_correspondence_distance = float(icp_max_correspondence_distance)
    p.information_max_distance = float(icp_max_correspondence_distance if information_max_distance is None
                                       else information_max_distance)
    return p


def check_constraint_params(params: ConstraintParams) -> int:
    """reg_check_constraint_params: the status reg_submaps_build_constraint would return for these parameters (no device)."""
    return int(_constraints_lib().reg_check_constraint_params(C.byref(params) if params is not None else None))


def constraints_struct_sizes() -> tuple:
    """sizeof of reg_constraint_params, reg_constraint_result in the library."""
    out = (C.c_int32 * 2)()
    _constraints_lib().reg_constraints_struct_sizes(out)
    return tuple(out)


def host_registration_consistent(T, bounds):
    """reg_host_registration_consistent: (consistent, failed mask) of isRegistrationConsistent for the 4 x 4 T and the bounds
    (roll, pitch, yaw [rad], x, y, z [m]); bit k of the mask names CONSISTENCY_COMPONENTS[k]."""
    b = (C.c_double * 6)(*[float(v) for v in bounds])
    mask = C.c_int32(0)
    st = _constraints_lib().reg_host_registration_consistent(_T_in_f64(T), b, C.byref(mask))
    if st != 0:
        raise RegError(st, "reg_host_registration_consistent")
    return mask.value == 0, int(mask.value)


def _submaps_default_odometry_constraint_params(self, refine=False) -> ConstraintParams:
    """reg_default_odometry_constraint_params: buildOdometryConstraint's arguments for this collection's map voxel size."""
    p = ConstraintParams()
    self._check(_constraints_lib().reg_default_odometry_constraint_params(self._s, int(bool(refine)), C.byref(p)))
    return p


def _submaps_build_constraint(self, source, target, params: ConstraintParams, T_init=None) -> ConstraintResult:
    """reg_submaps_build_constraint: overlap selection, registration and information matrix between two resident submaps, on
    a handle of the collection's own (the handle of `reg` keeps its reference and reading)."""
    res = ConstraintResult()
    res.struct_size = C.sizeof(ConstraintResult)
    if params is not None:
        params.struct_size = C.sizeof(ConstraintParams)
    self._check(_constraints_lib().reg_submaps_build_constraint(self._s, int(source), int(target),
                                                                C.byref(params) if params is not None else None,
                                                                _T_in_f64(T_init), C.byref(res)))
    return res


def _submaps_compute_odometry_constraints(self, candidates=None, params: "ConstraintParams | None" = None) -> int:
    """reg_submaps_compute_odometry_constraints: builds the missing odometry constraints (of the candidates, or of every
    finished pair) into the collection's list; returns how many were added.  All or nothing."""
    c = None if candidates is None else np.ascontiguousarray(candidates, np.int32).reshape(-1)
    if c is not None and c.size == 0:
        return 0
    if params is not None:
        params.struct_size = C.sizeof(ConstraintParams)
    added = C.c_int32(0)
    self._check(_constraints_lib().reg_submaps_compute_odometry_constraints(
        self._s, _ptr(c) if c is not None else None, 0 if c is None else int(c.size),
        C.byref(params) if params is not None else None, C.byref(added)))
    return int(added.value)


def _submaps_odometry_constraints(self) -> list:
    """reg_submaps_get_odometry_constraints: [dict(source, target, T 4 x 4, information 6 x 6, information_valid, is_odometry)]."""
    lib, n = _constraints_lib(), C.c_int32(0)
    self._check(lib.reg_submaps_get_odometry_constraints(self._s, 0, None, None, None, None, None, C.byref(n)))
    k = max(int(n.value), 1)
    src, tgt, flags = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32)
    T, info = np.zeros((k, 16), np.float64), np.zeros((k, 36), np.float64)
    self._check(lib.reg_submaps_get_odometry_constraints(self._s, k, _ptr(src), _ptr(tgt), _ptr(T), _ptr(info), _ptr(flags), C.byref(n)))
    return [dict(source=int(src[i]), target=int(tgt[i]), T=T[i].reshape(4, 4).T.copy(), information=info[i].reshape(6, 6).copy(),
                 information_valid=bool(flags[i] & 1), is_odometry=bool(flags[i] & 2)) for i in range(int(n.value))]


def _submaps_clear_odometry_constraints(self):
    self._check(_constraints_lib().reg_submaps_clear_odometry_constraints(self._s))


def _submaps_get_features(self, idx):
    """reg_submaps_get_features: the stored sparse cloud and features of a submap, dict(xyz64 n x 3 float64, xyz n x 3 float32,
    normals n x 3 float32, fpfh n x 33 float64); n = 0 before its features were computed."""
    lib, n = _constraints_lib(), C.c_int64(0)
    self._check(lib.reg_submaps_get_features(self._s, int(idx), 0, None, None, None, None, 0, C.byref(n)))
    k = int(n.value)
    cap = max(k, 1)
    x64, x, nr, f = (np.empty((cap, 3), np.float64), np.empty((cap, 3), np.float32), np.empty((cap, 3), np.float32),
                     np.empty((cap, 33), np.float64))
    self._check(lib.reg_submaps_get_features(self._s, int(idx), 0, _ptr(x64), _ptr(x), _ptr(nr), _ptr(f), cap, C.byref(n)))
    return dict(xyz64=x64[:k].copy(), xyz=x[:k].copy(), normals=nr[:k].copy(), fpfh=f[:k].copy())


def _submaps_get_features_device(self, idx, capacity_rows, xyz64_ptr=None, xyz_ptr=None, nrm_ptr=None, fpfh_ptr=None) -> int:
    """As get_features with the outputs resident in HBM.  Returns the stored rows."""
    vp = lambda p: C.c_void_p(p) if p else None
    n = C.c_int64(0)
    self._check(_constraints_lib().reg_submaps_get_features(self._s, int(idx), 1, vp(xyz64_ptr), vp(xyz_ptr), vp(nrm_ptr),
                                                            vp(fpfh_ptr), int(capacity_rows), C.byref(n)))
    return int(n.value)


Submaps.default_odometry_constraint_params = _submaps_default_odometry_constraint_params
Submaps.build_constraint = _submaps_build_constraint
Submaps.compute_odometry_constraints = _submaps_compute_odometry_constraints
Submaps.odometry_constraints = _submaps_odometry_constraints
Submaps.clear_odometry_constraints = _submaps_clear_odometry_constraints
Submaps.get_features = _submaps_get_features
Submaps.get_features_device = _submaps_get_features_device


class LoopClosureParams(C.Structure):
    """reg_loop_closure_params (include/o3dslam_reg.h): the gates of buildLoopClosureConstraints, RANSAC's and the refinement's
    parameters."""
    _fields_ = [("struct_size", C.c_int32), ("ransac_min_correspondence_set_size", C.c_int32), ("min_refinement_fitness", C.c_double),
                ("consistency_bounds", C.c_double * 6), ("ransac", RansacParams), ("refine", ConstraintParams)]


class LoopClosureVerdict(C.Structure):
    """reg_loop_closure_verdict (include/o3dslam_reg.h); T_ransac_matrix() gives the 4 x 4 math layout."""
    _fields_ = [("struct_size", C.c_int32), ("source", C.c_int32), ("candidate", C.c_int32), ("verdict", C.c_int32),
                ("ransac_failed_mask", C.c_int32), ("icp_failed_mask", C.c_int32), ("refined", C.c_int32), ("reserved", C.c_int32),
                ("n_correspondences", C.c_int64), ("ransac_iterations", C.c_int64), ("stamp_ns", C.c_int64),
                ("ransac_fitness", C.c_double), ("ransac_inlier_rmse", C.c_double), ("T_ransac", C.c_double * 16),
                ("constraint", ConstraintResult)]

    def T_ransac_matrix(self) -> np.ndarray:
        return np.array(self.T_ransac, np.float64).reshape(4, 4).T.copy()


EXPORTS += ["reg_loop_closure_struct_sizes", "reg_submaps_build_loop_closure_constraints"]
LC_ACCEPTED, LC_RANSAC_SET_TOO_SMALL, LC_RANSAC_INCONSISTENT, LC_FITNESS_TOO_LOW, LC_ICP_INCONSISTENT = range(5)


def loop_closure_struct_sizes() -> tuple:
    """sizeof of reg_loop_closure_params, reg_loop_closure_verdict in the library."""
    lib = load_library()
    lib.reg_loop_closure_struct_sizes.argtypes = [C.POINTER(C.c_int32)]
    lib.reg_loop_closure_struct_sizes.restype = None
    out = (C.c_int32 * 2)()
    lib.reg_loop_closure_struct_sizes(out)
    return tuple(out)


def loop_closure_params(refine: ConstraintParams, max_correspondence_distance=0.75, ransac_n=3, max_iteration=1000000,
                        confidence=0.99, distance_threshold=0.75, edge_similarity=0.5, seed=0, min_correspondence_set_size=25,
                        min_refinement_fitness=0.7, bounds=(math.pi / 2, math.pi / 2, math.pi / 2, 10.0, 10.0, 15.0)) -> LoopClosureParams:
    """A reg_loop_closure_params with PlaceRecognitionParameters' defaults (Parameters.hpp:113-135); bounds = maxDrift roll,
    pitch, yaw [rad], x, y, z [m]."""
    p = LoopClosureParams()
    p.struct_size = C.sizeof(LoopClosureParams)
    p.ransac_min_correspondence_set_size = int(min_correspondence_set_size)
    p.min_refinement_fitness = float(min_refinement_fitness)
    p.consistency_bounds = (C.c_double * 6)(*[float(b) for b in bounds])
    r = p.ransac
    r.struct_size, r.ransac_n, r.max_iteration, r.confidence = C.sizeof(RansacParams), int(ransac_n), int(max_iteration), float(confidence)
    r.max_correspondence_distance, r.distance_threshold = float(max_correspondence_distance), float(distance_threshold)
    r.edge_similarity, r.seed, r.batch = float(edge_similarity), int(seed), 0
    p.refine = refine
    p.refine.struct_size = C.sizeof(ConstraintParams)
    return p


def _submaps_build_loop_closure_constraints(self, last_finished, stamp_ns, params: LoopClosureParams) -> list:
    """reg_submaps_build_loop_closure_constraints: one LoopClosureVerdict per candidate of `last_finished`, in candidate order
    (feature matching, RANSAC, the gates and the refinement on the stored features and the resident maps)."""
    lib = _constraints_lib()
    lib.reg_submaps_build_loop_closure_constraints.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.POINTER(LoopClosureParams),
                                                               C.POINTER(LoopClosureVerdict), C.c_int32, C.POINTER(C.c_int32)]
    cap = max(int(self.info().n_submaps), 1)
    out = (LoopClosureVerdict * cap)()
    out[0].struct_size = C.sizeof(LoopClosureVerdict)
    n = C.c_int32(0)
    params.struct_size = C.sizeof(LoopClosureParams)
    self._check(lib.reg_submaps_build_loop_closure_constraints(self._s, int(last_finished), int(stamp_ns), C.byref(params), out, cap,
                                                               C.byref(n)))
    res = []
    for k in range(int(n.value)):
        v = LoopClosureVerdict()
        C.memmove(C.byref(v), C.byref(out[k]), C.sizeof(LoopClosureVerdict))
        res.append(v)
    return res


Submaps.build_loop_closure_constraints = _submaps_build_loop_closure_constraints


# ---- the dense maps of the collection and the fused carve ---------------------------------------------------------
class SubmapsDenseParams(C.Structure):
    """reg_submaps_dense_params (include/o3dslam_reg.h): the dense-map builder of every submap of a collection."""
    _fields_ = [("struct_size", C.c_int32), ("carve_every_n_scans", C.c_int32), ("carve_in_map_frame", C.c_int32),
                ("reserved", C.c_int32), ("voxel_size", C.c_double), ("scan", DenseScanParams), ("carve", DenseCarveParams)]


class SubmapsDenseInsertResult(C.Structure):
    """reg_submaps_dense_insert_result (include/o3dslam_reg.h)."""
    _fields_ = [("struct_size", C.c_int32), ("carved", C.c_int32), ("n_inserted", C.c_int64), ("n_voxels", C.c_int64),
                ("n_removed", C.c_int64), ("scans_inserted", C.c_int64)]


EXPORTS += ["reg_dense_map_carve_scan", "reg_default_submaps_dense_params", "reg_check_submaps_dense_params",
            "reg_submaps_dense_struct_sizes", "reg_submaps_enable_dense_maps", "reg_submaps_insert_scan_dense_map",
            "reg_submaps_get_dense_info", "reg_submaps_export_dense_submap", "reg_debug_dense_carve"]
_dense_bound = False


def _dense_lib():
    """The library with the prototypes of this section set."""
    global _dense_bound
    lib = load_library()
    if not _dense_bound:
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        pd, pi64 = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        lib.reg_dense_map_carve_scan.argtypes = [vp, vp, i64, C.c_int, pd, C.POINTER(DenseCarveParams), pd, vp, pi64]
        lib.reg_default_submaps_dense_params.argtypes = [C.POINTER(SubmapsDenseParams)]
        lib.reg_default_submaps_dense_params.restype = None
        lib.reg_check_submaps_dense_params.argtypes = [C.POINTER(SubmapsDenseParams)]
        lib.reg_submaps_dense_struct_sizes.argtypes = [C.POINTER(i32)]
        lib.reg_submaps_dense_struct_sizes.restype = None
        lib.reg_submaps_enable_dense_maps.argtypes = [vp, C.POINTER(SubmapsDenseParams)]
        lib.reg_submaps_insert_scan_dense_map.argtypes = [vp, i32, vp, vp, vp, i64, C.c_int, pd, i32,
                                                          C.POINTER(SubmapsDenseInsertResult)]
        lib.reg_submaps_get_dense_info.argtypes = [vp, i32, C.POINTER(DenseMapInfo), pi64]
        lib.reg_submaps_export_dense_submap.argtypes = [vp, i32, C.c_int, vp, vp, vp, vp, vp, i64, pi64]
        lib.reg_debug_dense_carve.argtypes = [vp, i32, i32, pi64]
        _dense_bound = True
    return lib


def default_submaps_dense_params(crop=None, rgb_min=None, rgb_max=None, carve: "DenseCarveParams | None" = None,
                                 **overrides) -> SubmapsDenseParams:
    """reg_default_submaps_dense_params (every 10 scans, the reference's carve frame, voxel 0.03, no crop, colours within
    [0, 1], the shipped carve); crop / rgb_min / rgb_max as default_dense_scan_params, carve replaces the carve parameters."""
    p = SubmapsDenseParams()
    _dense_lib().reg_default_submaps_dense_params(C.byref(p))
    p.scan = default_dense_scan_params(crop, rgb_min, rgb_max)
    if carve is not None:
        p.carve = carve
        p.carve.struct_size = C.sizeof(DenseCarveParams)
    for k, v in overrides.items():
        if k in ("carve_every_n_scans", "carve_in_map_frame"):
            setattr(p, k, int(v))
        elif k == "voxel_size":
            p.voxel_size = float(v)
        else:
            raise TypeError(f"unknown dense-map parameter {k}")
    return p


def check_submaps_dense_params(params: "SubmapsDenseParams | None") -> int:
    """reg_check_submaps_dense_params: the status reg_submaps_enable_dense_maps would return for these parameters (no device)."""
    return int(_dense_lib().reg_check_submaps_dense_params(C.byref(params) if params is not None else None))


def submaps_dense_struct_sizes() -> tuple:
    """sizeof of reg_submaps_dense_params, reg_submaps_dense_insert_result in the library."""
    out = (C.c_int32 * 2)()
    _dense_lib().reg_submaps_dense_struct_sizes(out)
    return tuple(out)


def debug_dense_carve(reg: "Registration", lanes_per_ray=0, collect_stats=False) -> dict:
    """reg_debug_dense_carve: sets the measurement switches of carve_scan on the handle of `reg` and returns what its last
    carve_scan left: dict(bricks, samples, coarse_done, rays)."""
    out = (C.c_int64 * 4)()
    reg._check(_dense_lib().reg_debug_dense_carve(reg._h, int(lanes_per_ray), int(bool(collect_stats)), out))
    return dict(bricks=int(out[0]), samples=int(out[1]), coarse_done=int(out[2]), rays=int(out[3]))


def _dense_map_carve_scan(self, scan_xyz, sensor, params: "DenseCarveParams | None" = None, T=None, want_keys=True):
    """reg_dense_map_carve_scan: Submap::carve for the dense map in one call -- transform by T (None: the scan as given),
    first-wins de-duplication at the map's voxel size, getKeysOfCarvedPoints, erase.  Returns the erased keys (k x 3 int32,
    ascending key order), or their number with want_keys=False."""
    x = self._f64(scan_xyz)
    keys = np.empty((max(self.info().n_voxels, 1), 3), np.int32) if want_keys else None
    k = self._carve_scan(_ptr(x), x.shape[0], 0, sensor, params, T, _ptr(keys))
    return keys[:k].copy() if want_keys else k


def _dense_map_carve_scan_device(self, scan_ptr, n_scan, sensor, params: "DenseCarveParams | None" = None, T=None,
                                 keys_ptr=None) -> int:
    """As carve_scan with the fp64 scan and the int32 key output (n_voxels x 3, may be None) resident in HBM."""
    vp = lambda p: C.c_void_p(p) if p else None
    return self._carve_scan(vp(scan_ptr), n_scan, 1, sensor, params, T, vp(keys_ptr))


def _dense_map_carve_scan_call(self, x, n, on_device, sensor, params, T, keys):
    p = params if params is not None else default_dense_carve_params()
    p.struct_size = C.sizeof(DenseCarveParams)
    sen = (C.c_double * 3)(*[float(v) for v in sensor])
    k = C.c_int64(0)
    self._check(_dense_lib().reg_dense_map_carve_scan(self._m, x, n, on_device, sen, C.byref(p), _T_in_f64(T), keys, C.byref(k)))
    return int(k.value)


DenseMap.carve_scan = _dense_map_carve_scan
DenseMap.carve_scan_device = _dense_map_carve_scan_device
DenseMap._carve_scan = _dense_map_carve_scan_call


def _submaps_enable_dense_maps(self, params: "SubmapsDenseParams | None" = None):
    """reg_submaps_enable_dense_maps: every submap, existing and future, gets a dense map."""
    p = params if params is not None else default_submaps_dense_params()
    p.struct_size = C.sizeof(SubmapsDenseParams)
    self._check(_dense_lib().reg_submaps_enable_dense_maps(self._s, C.byref(p)))
    self.dense_params = p


def _submaps_insert_scan_dense_map(self, idx, xyz, T, normals=None, colors=None, perform_carving=True) -> SubmapsDenseInsertResult:
    """Submap::insertScanDenseMap of submap idx: croppers, transform, insert, and the carve when it is due."""
    x, nr, cl = DenseMap._f64(xyz), DenseMap._f64(normals), DenseMap._f64(colors)
    return self._insert_dense(idx, _ptr(x), _ptr(nr), _ptr(cl), x.shape[0], 0, T, perform_carving)


def _submaps_insert_scan_dense_map_device(self, idx, xyz_ptr, n, T, nrm_ptr=None, col_ptr=None,
                                          perform_carving=True) -> SubmapsDenseInsertResult:
    """As insert_scan_dense_map with the fp64 arrays (n x 3 each) resident in HBM."""
    vp = lambda p: C.c_void_p(p) if p else None
    return self._insert_dense(idx, vp(xyz_ptr), vp(nrm_ptr), vp(col_ptr), n, 1, T, perform_carving)


def _submaps_insert_dense(self, idx, x, nr, cl, n, on_device, T, perform_carving):
    res = SubmapsDenseInsertResult()
    res.struct_size = C.sizeof(SubmapsDenseInsertResult)
    self._check(_dense_lib().reg_submaps_insert_scan_dense_map(self._s, int(idx), x, nr, cl, int(n), on_device, _T_in_f64(T),
                                                               int(bool(perform_carving)), C.byref(res)))
    return res


def _submaps_dense_info(self, idx):
    """(DenseMapInfo, scans_inserted) of the dense map of submap idx."""
    i, k = DenseMapInfo(), C.c_int64(0)
    i.struct_size = C.sizeof(DenseMapInfo)
    self._check(_dense_lib().reg_submaps_get_dense_info(self._s, int(idx), C.byref(i), C.byref(k)))
    return i, int(k.value)


def _submaps_export_dense_submap(self, idx, want_keys=True, want_counts=True):
    """getDenseMapCopy().toPointCloud() (+ raw keys and counts) of submap idx: the dict of DenseMap.export."""
    i = self.dense_info(idx)[0]
    n = int(i.n_voxels)
    f = lambda on, w, t: np.empty((max(n, 1), w), t) if on else None
    x, nr, cl = f(True, 3, np.float64), f(i.has_normals, 3, np.float64), f(i.has_colors, 3, np.float64)
    ky, ct = f(want_keys, 3, np.int32), f(want_counts, 1, np.int32)
    k = C.c_int64(0)
    self._check(_dense_lib().reg_submaps_export_dense_submap(self._s, int(idx), 0, _ptr(x), _ptr(nr), _ptr(cl), _ptr(ky), _ptr(ct),
                                                             max(n, 1), C.byref(k)))
    cut = lambda a: a[:int(k.value)] if a is not None else None
    return dict(xyz=cut(x), normals=cut(nr), colors=cut(cl), keys=cut(ky), counts=cut(ct).reshape(-1) if ct is not None else None)


def _submaps_export_dense_submap_device(self, idx, capacity_rows, xyz_ptr=None, nrm_ptr=None, col_ptr=None, keys_ptr=None,
                                        counts_ptr=None) -> int:
    """As export_dense_submap into arrays resident in HBM (capacity_rows rows each; any may be None).  Returns n_voxels."""
    vp = lambda p: C.c_void_p(p) if p else None
    k = C.c_int64(0)
    self._check(_dense_lib().reg_submaps_export_dense_submap(self._s, int(idx), 1, vp(xyz_ptr), vp(nrm_ptr), vp(col_ptr),
                                                             vp(keys_ptr), vp(counts_ptr), int(capacity_rows), C.byref(k)))
    return int(k.value)


Submaps.enable_dense_maps = _submaps_enable_dense_maps
Submaps.insert_scan_dense_map = _submaps_insert_scan_dense_map
Submaps.insert_scan_dense_map_device = _submaps_insert_scan_dense_map_device
Submaps._insert_dense = _submaps_insert_dense
Submaps.dense_info = _submaps_dense_info
Submaps.export_dense_submap = _submaps_export_dense_submap
Submaps.export_dense_submap_device = _submaps_export_dense_submap_device
