"""ctypes plumbing over the C-ABI of libscvod.so (include/scvod.h) for tests/ and bench.py.

This is NOT the product's host side (that is the C++ facade in ../host/, mirroring the
reference's SSC / PatchWork classes); it only lets Python drive the same extern "C" entry
points with numpy arrays and torch device tensors.  There is no CPU fallback: loading fails
loudly when libscvod.so is missing and scvod_create fails when no HIP device is present.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "..", "csrc", "libscvod.so")

MAX_PATCHES = 1024


class Params(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "sensor_height", "min_dis", "max_dis", "min_angle", "max_angle", "min_azimuth", "max_azimuth",
        "range_res", "sector_res", "azimuth_res", "occupancy", "max_z", "min_z", "car_square")] + \
               [("toBeClass", C.c_int32), ("reserved", C.c_int32)]


class PwParams(C.Structure):
    _fields_ = [("num_iter", C.c_int32), ("num_lpr", C.c_int32), ("num_min_pts", C.c_int32),
                ("num_rings_of_interest", C.c_int32), ("num_sectors_each_zone", C.c_int32 * 4),
                ("num_rings_each_zone", C.c_int32 * 4), ("th_seeds", C.c_double), ("th_dist", C.c_double),
                ("max_range", C.c_double), ("min_range", C.c_double), ("uprightness_thr", C.c_double),
                ("adaptive_seed_selection_margin", C.c_double), ("elevation_thr", C.c_double * 4),
                ("flatness_thr", C.c_double * 4)]


APRI_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("range", "f4"), ("angle", "f4"), ("azimuth", "f4"),
                       ("intensity", "f4"), ("range_idx", "i4"), ("sector_idx", "i4"), ("azimuth_idx", "i4"),
                       ("voxel_idx", "i4")])
PLANE_DTYPE = np.dtype([("normal", "f4", 3), ("mean", "f4", 3), ("sv", "f4", 3), ("n_pts", "i4"), ("n_ground", "i4"),
                        ("status", "i4")])
assert APRI_DTYPE.itemsize == 44 and PLANE_DTYPE.itemsize == 48


# struct scvod_object (include/scvod.h): one cluster of the object table, 64 bytes
OBJECT_DTYPE = np.dtype([("scan", "i4"), ("name", "i4"), ("n_points", "i4"), ("n_voxels", "i4"), ("box_min", "f4", 3),
                         ("box_max", "f4", 3), ("center", "f4", 3), ("angle_diff", "f4"), ("cls", "i1"), ("state", "i1"),
                         ("dynamic", "u1"), ("reserved", "u1"), ("point_begin", "i4")])
OBJ_NO_TRACK = 1


class Object(C.Structure):
    _fields_ = [("scan", C.c_int32), ("name", C.c_int32), ("n_points", C.c_int32), ("n_voxels", C.c_int32),
                ("box_min", C.c_float * 3), ("box_max", C.c_float * 3), ("center", C.c_float * 3), ("angle_diff", C.c_float),
                ("cls", C.c_int8), ("state", C.c_int8), ("dynamic", C.c_uint8), ("reserved", C.c_uint8), ("point_begin", C.c_int32)]


# struct scvod_object_shape (include/scvod.h): the eigenvalue descriptor of one object, 96 bytes
OBJECT_SHAPE_DTYPE = np.dtype([("cov", "f4", 6), ("eig", "f4", 3), ("flags", "i4"), ("feat", "f8", 7)])
FEATURE_NAMES = ("linearity", "planarity", "scattering", "omnivariance", "anisotropy", "eigen_entropy", "change_of_curvature")


class ObjectShape(C.Structure):
    _fields_ = [("cov", C.c_float * 6), ("eig", C.c_float * 3), ("flags", C.c_int32), ("feat", C.c_double * 7)]


class FeatureParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("kOneThird", "kLinearityMax", "kPlanarityMax", "kScatteringMax", "kOmnivarianceMax",
                                          "kAnisotropyMax", "kEigenEntropyMax", "kChangeOfCurvatureMax")]


# struct scvod_object_esf (include/scvod.h): the ESF descriptor of one object, 64 bytes
OBJECT_ESF_DTYPE = np.dtype([("fold10", "f4", 10), ("n_valid", "i4"), ("n_points", "i4"), ("flags", "i4"), ("lines", "u4", 3)])
ESF_SIG = 640
ESF_CACHE_POINTS = 3584  # SCVOD_ESF_CACHE_POINTS


class ObjectEsf(C.Structure):
    _fields_ = [("fold10", C.c_float * 10), ("n_valid", C.c_int32), ("n_points", C.c_int32), ("flags", C.c_int32), ("lines", C.c_uint32 * 3)]


class EsfParams(C.Structure):
    """struct scvod_esf_params (include/scvod.h)"""
    _fields_ = [("samples", C.c_int32), ("seed", C.c_uint32), ("min_points", C.c_int32), ("cls_mask", C.c_uint32), ("reserved", C.c_int32 * 4)]


class EvalParams(C.Structure):
    """struct scvod_eval_params (include/scvod.h)"""
    _fields_ = [("voxelsize", C.c_double), ("n_dynamic_classes", C.c_int32), ("dynamic_classes", C.c_uint16 * 16)]


EVAL_COUNTS = ("num_gt_static", "num_gt_dynamic", "num_est_static", "num_est_dynamic", "num_preserved", "num_static_preserved",
               "num_dynamic_preserved")


class EvalResult(C.Structure):
    """struct scvod_eval_result (include/scvod.h): the seven counts of metric.preservation_rejection, then PR, RR, F1"""
    _fields_ = [(n, C.c_int64) for n in EVAL_COUNTS] + [(n, C.c_double) for n in ("PR", "RR", "F1")]


EVAL_RESULT = EvalResult
# scvod_evaluate_device's per-point byte; scvod_classify_map_device's classes are metric.py's TP_STATIC .. UNMATCHED
EVAL_INLIER, EVAL_GT_DYNAMIC, EVAL_EST_DYNAMIC = 1, 2, 4


class ClassParams(C.Structure):
    """struct scvod_class_params (include/scvod.h)"""
    _fields_ = [("max_dist", C.c_float), ("cell", C.c_float), ("n_ground", C.c_int32), ("n_building", C.c_int32), ("n_tree", C.c_int32),
                ("ground", C.c_uint16 * 8), ("building", C.c_uint16 * 8), ("tree", C.c_uint16 * 8)]


class ClassResult(C.Structure):
    """struct scvod_class_result (include/scvod.h): conf[truth class][estimate class], pd_far, then what scvod_class_finish fills"""
    _fields_ = [("conf", (C.c_int64 * 5) * 4), ("pd_far", C.c_int64), ("num", C.c_int64 * 4), ("P", C.c_int64 * 4),
                ("rate_P", C.c_float * 4), ("rate_N", C.c_float * 4)]


CLASS_RESULT = ClassResult
# truth classes (rows of conf) and estimate classes (its columns); scvod_score_classes_device's per-point byte
CLASS_TRUTH = ("ground", "building", "tree", "pd")
CLASS_ESTIMATE = ("other", "ground", "building", "tree", "none")
CLASS_P = 32


class InstanceParams(C.Structure):
    """struct scvod_instance_params (include/scvod.h)"""
    _fields_ = [("n_dynamic_classes", C.c_int32), ("dynamic_classes", C.c_uint16 * 16), ("n_static_classes", C.c_int32),
                ("static_classes", C.c_uint16 * 16), ("removed_below", C.c_double), ("retained_from", C.c_double), ("min_points", C.c_int64)]


INSTANCE_COUNTS = ("hd_gt", "hd_removed", "ld_gt", "ld_retained", "hd_points", "hd_points_preserved", "ld_points", "ld_points_preserved",
                   "skipped")


class InstanceResult(C.Structure):
    """struct scvod_instance_result (include/scvod.h)"""
    _fields_ = [(n, C.c_int64) for n in INSTANCE_COUNTS] + [(n, C.c_double) for n in ("hd_removed_rate", "ld_retained_rate")]


# struct scvod_instance: one record of scvod_score_instances_device's table
INSTANCE_DTYPE = np.dtype([("label", "<u4"), ("first_point", "<i4"), ("n_points", "<i8"), ("n_inlier", "<i8"), ("n_preserved", "<i8")])
INSTANCE_STATS = ("written", "distinct", "overflow", "spilled_tiles")

# struct scvod_object_truth: the truth label one object of the table covers (scvod_batch_object_truth), 32 bytes
OBJECT_TRUTH_DTYPE = np.dtype([("label", "<u4"), ("n_label", "<i4"), ("n_class", "<i4"), ("n_moving", "<i4"), ("n_distinct", "<i4"),
                               ("n_points", "<i4"), ("reserved", "<i4", 2)])
OBJ_TRUTH_ONCHIP_LABELS = 128  # SCVOD_OBJ_TRUTH_ONCHIP_LABELS
OBJECT_TRUTH_STATS = ("written", "objects", "overflow", "fallback_objects", "moving_points", "moving_members")


class ObjectTruthParams(C.Structure):
    """struct scvod_object_truth_params (include/scvod.h)"""
    _fields_ = [("moving_from", C.c_double), ("pure_from", C.c_double), ("min_points", C.c_int64)]


OBJECT_TRUTH_COUNTS = ("moving_objects", "moving_dynamic", "moving_car_static", "moving_car_untracked", "moving_not_car", "static_objects",
                       "static_dynamic", "mixed_objects", "skipped")


class ObjectTruthResult(C.Structure):
    """struct scvod_object_truth_result (include/scvod.h)"""
    _fields_ = [(n, C.c_int64) for n in OBJECT_TRUTH_COUNTS] + [(n, C.c_double) for n in ("precision", "recall")]


class MapFilterParams(C.Structure):
    """struct scvod_map_filter_params (include/scvod.h), 24 bytes"""
    _fields_ = [("radius", C.c_float), ("flags", C.c_int32), ("vote_num", C.c_int32), ("vote_den", C.c_int32), ("min_points", C.c_int32),
                ("reserved", C.c_int32)]


# struct scvod_map_filter_object: what the members of one object of the table said (scvod_batch_map_filter's d_votes), 32 bytes
MAP_FILTER_OBJECT_DTYPE = np.dtype([("n_cell", "<i4"), ("n_near", "<i4"), ("n_miss", "<i4"), ("n_out", "<i4"), ("n_points", "<i4"),
                                    ("verdict", "<i4"), ("reserved", "<i4", 2)])
MAPF_KNOWN, MAPF_NOVEL, MAPF_OUT = 0, 1, 2  # SCVOD_MAPF_*: the side byte of StaticMap.filter
MAPF_OBJECT_VOTE = 1                         # SCVOD_MAPF_OBJECT_VOTE
MAP_FILTER_TILE = 2048                       # SCVOD_MAP_FILTER_TILE
MAPF_OUTPUTS = ("result", "side", "order", "bounds", "xyzi", "payload", "votes")
MAP_FILTER_STATS = ("points", "known", "novel", "out", "moved_to_known", "moved_to_novel", "objects_voted", "objects_known")


class VisibilityParams(C.Structure):
    """scvod_visibility_params (include/scvod.h), 32 bytes"""
    _fields_ = [("before", C.c_int32), ("after", C.c_int32), ("halo", C.c_int32), ("gap_abs", C.c_float), ("gap_rel", C.c_float),
                ("min_through", C.c_int32), ("vote_num", C.c_int32), ("vote_den", C.c_int32)]


VIS_UNTESTED, VIS_KEEP, VIS_SEEN_THROUGH = 0, 1, 2   # SCVOD_VIS_*: the verdict byte
VIS_WITH_GROUND = 1                                   # SCVOD_VIS_WITH_GROUND
VIS_IMAGES_ONLY = 2                                   # SCVOD_VIS_IMAGES_ONLY
VIS_MAX_WINDOW = 32                                   # SCVOD_VIS_MAX_WINDOW
VIS_OUTPUTS = ("votes", "verdict", "images", "scan_counts")
VIS_STATS = ("queries", "seen_through", "through", "agree", "occluded", "outside_or_empty", "pairs")


class CloudVisibilityParams(C.Structure):
    """scvod_cloud_visibility_params (include/scvod.h), 32 bytes"""
    _fields_ = [("halo", C.c_int32), ("gap_abs", C.c_float), ("gap_rel", C.c_float), ("max_range", C.c_float), ("min_through", C.c_int32),
                ("vote_num", C.c_int32), ("vote_den", C.c_int32), ("reserved", C.c_int32)]


CVIS_NO_SORT = 1                                      # SCVOD_CVIS_NO_SORT
CVIS_OUTPUTS = ("votes", "verdict")
CVIS_STATS = ("points", "finite", "seen_through", "keep", "untested", "through", "agree", "occluded", "empty", "steps")


class ObjectVisibilityParams(C.Structure):
    """scvod_object_visibility_params (include/scvod.h), 32 bytes"""
    _fields_ = [("flags", C.c_int32), ("min_points", C.c_int32), ("min_tested", C.c_int32), ("min_through", C.c_int32),
                ("vote_num", C.c_int32), ("vote_den", C.c_int32), ("reserved", C.c_int32 * 2)]


OBJVIS_POOL_PAIRS = 1                                 # SCVOD_OBJVIS_POOL_PAIRS
OBJVIS_WITH_TRACK = 2                                 # SCVOD_OBJVIS_WITH_TRACK
OBJVIS_TILE = 2048                                    # SCVOD_OBJVIS_TILE
OBJVIS_OUTPUTS = ("records", "verdict")
OBJVIS_STATS = ("objects", "voted", "forced", "seen_through", "moved_to_seen_through", "moved_to_keep", "written", "overflow")
# struct scvod_object_visibility: one object's share of the vote (scvod_batch_object_visibility), 48 bytes
OBJECT_VISIBILITY_DTYPE = np.dtype([("n_points", "<i4"), ("n_untested", "<i4"), ("n_keep", "<i4"), ("n_seen", "<i4"),
                                    ("sum_through", "<i4"), ("sum_agree", "<i4"), ("sum_occluded", "<i4"), ("sum_other", "<i4"),
                                    ("verdict", "<i4"), ("how", "<i4"), ("reserved", "<i4", 2)])
assert OBJECT_VISIBILITY_DTYPE.itemsize == 48


class TrackParams(C.Structure):
    """scvod_track_params (include/scvod.h), 32 bytes"""
    _fields_ = [("flags", C.c_int32), ("occupancy", C.c_float), ("gate", C.c_float), ("size_ratio", C.c_float),
                ("min_points", C.c_int32), ("min_length", C.c_int32), ("reserved", C.c_int32 * 2)]


class TracksResult(C.Structure):
    """scvod_tracks_result (include/scvod.h), 72 bytes"""
    _fields_ = [("tracks", C.c_int64), ("moving_tracks", C.c_int64), ("moving_members", C.c_int64),
                ("moving_members_dynamic", C.c_int64), ("still_tracks", C.c_int64), ("still_members", C.c_int64),
                ("still_members_dynamic", C.c_int64), ("recall_along", C.c_double), ("false_alarm", C.c_double)]


TRK_NO_GATE = 1                                       # SCVOD_TRK_NO_GATE
TRK_ANY_CLASS = 2                                     # SCVOD_TRK_ANY_CLASS
TRK_OUTPUTS = ("links", "tracks", "track_objects", "n_tracks")
TRK_STATS = ("objects", "tracks", "written", "overlap_links", "gate_links", "refused", "longest", "overflow")
# struct scvod_object_link: how one object of the table continues across scans (scvod_object_tracks_device), 32 bytes
OBJECT_LINK_DTYPE = np.dtype([("track", "<i4"), ("rank", "<i4"), ("pred", "<i4"), ("succ", "<i4"), ("kind", "<i4"), ("weight", "<i4"),
                              ("step", "<f4"), ("reserved", "<i4")])
assert OBJECT_LINK_DTYPE.itemsize == 32
# struct scvod_track: one listed track, 64 bytes
TRACK_DTYPE = np.dtype([("first_object", "<i4"), ("last_object", "<i4"), ("length", "<i4"), ("first_scan", "<i4"), ("last_scan", "<i4"),
                        ("n_dynamic", "<i4"), ("n_gate_links", "<i4"), ("object_begin", "<i4"), ("net", "<f4", 3), ("path", "<f4"),
                        ("max_step", "<f4"), ("reserved", "<i4", 3)])
assert TRACK_DTYPE.itemsize == 64


class TrackVisibilityParams(C.Structure):
    """scvod_track_visibility_params (include/scvod.h), 40 bytes"""
    _fields_ = [("flags", C.c_int32), ("window", C.c_int32), ("min_travel", C.c_float), ("min_length", C.c_int32),
                ("min_moved", C.c_int32), ("min_flagged", C.c_int32), ("vote_num", C.c_int32), ("vote_den", C.c_int32),
                ("reserved", C.c_int32 * 2)]


TRKVIS_NO_DYNAMIC = 1                                 # SCVOD_TRKVIS_NO_DYNAMIC
TRKVIS_CLEAR = 2                                      # SCVOD_TRKVIS_CLEAR
TRKVIS_OUTPUTS = ("track_votes", "object_votes", "verdict")
TRKVIS_STATS = ("objects", "tracks", "tracks_voted", "members_motion", "members_cleared", "to_seen_through", "to_keep", "latch")
# struct scvod_track_vote: one per listed track (scvod_track_visibility_device), 32 bytes
TRACK_VOTE_DTYPE = np.dtype([("length", "<i4"), ("n_flagged", "<i4"), ("n_moved", "<i4"), ("verdict", "<i4"), ("how", "<i4"),
                             ("max_travel2", "<f4"), ("reserved", "<i4", 2)])
assert TRACK_VOTE_DTYPE.itemsize == 32
# struct scvod_object_track_vote: one per object of the table, 16 bytes
OBJECT_TRACK_VOTE_DTYPE = np.dtype([("track", "<i4"), ("verdict", "<i4"), ("how", "<i4"), ("travel2", "<f4")])
assert OBJECT_TRACK_VOTE_DTYPE.itemsize == 16


class ComponentVisibilityParams(C.Structure):
    """scvod_component_visibility_params (include/scvod.h), 32 bytes"""
    _fields_ = [("flags", C.c_int32), ("min_cells", C.c_int32), ("max_cells", C.c_int32), ("min_tested", C.c_int32),
                ("min_through", C.c_int32), ("vote_num", C.c_int32), ("vote_den", C.c_int32), ("reserved", C.c_int32)]


CMPVIS_POOL_PAIRS = 1                                 # SCVOD_CMPVIS_POOL_PAIRS
MAP_COMPONENTS_OUTPUTS = ("component", "table", "n")
MAP_COMPONENTS_STATS = ("records", "nodes", "padding", "absent", "duplicates", "components", "written", "overflow")
CMPVIS_OUTPUTS = ("records", "verdict")
CMPVIS_STATS = ("components", "voted", "seen_through", "moved_to_seen_through", "moved_to_keep", "written", "beyond_cap", "overflow")
# struct scvod_map_component: one connected component of the map's cells (scvod_map_components), 48 bytes
MAP_COMPONENT_DTYPE = np.dtype([("key", "<u8"), ("n_records", "<i4"), ("first_record", "<i4"), ("cell_min", "<i4", 3),
                                ("cell_max", "<i4", 3), ("reserved", "<i4", 2)])
assert MAP_COMPONENT_DTYPE.itemsize == 48
# struct scvod_component_visibility: one component's share of the vote (scvod_map_component_visibility), 64 bytes
COMPONENT_VISIBILITY_DTYPE = np.dtype([("n_records", "<i4"), ("n_untested", "<i4"), ("n_keep", "<i4"), ("n_seen", "<i4"),
                                       ("sum_through", "<i8"), ("sum_agree", "<i8"), ("sum_occluded", "<i8"), ("sum_empty", "<i8"),
                                       ("verdict", "<i4"), ("how", "<i4"), ("reserved", "<i4", 2)])
assert COMPONENT_VISIBILITY_DTYPE.itemsize == 64


class SplitParams(C.Structure):
    """struct scvod_split_params (include/scvod.h)"""
    _fields_ = [("cell", C.c_float), ("max_rings", C.c_int32), ("base_stride", C.c_int32), ("query_stride", C.c_int32),
                ("n_reject_classes", C.c_int32), ("reject_classes", C.c_uint16 * 16)]


# scvod_map_split_device's byte per base point; the partition's segments come in the order HIT, MISS, GATED
SPLIT_MISS, SPLIT_HIT, SPLIT_GATED = 0, 1, 2
SPLIT_STATS = ("n_hit", "n_miss", "n_gated", "pass1_queries", "ring_queries", "exhaustive_queries")


class RegisterParams(C.Structure):
    """scvod_register_params (64 bytes); use256 points at host bytes the caller keeps alive for the call (register_params_default does)"""
    _fields_ = [("max_iterations", C.c_int32), ("min_corr", C.c_int32), ("mode", C.c_int32), ("reserved", C.c_int32),
                ("max_dist", C.c_float), ("max_range", C.c_float), ("eps_rot", C.c_double), ("eps_trans", C.c_double),
                ("lam", C.c_double), ("pivot_eps", C.c_double), ("use256", C.c_void_p)]


REG_POINT, REG_PLANE = 0, 1
REG_MAX_ITERATIONS, REG_CONVERGED, REG_DEGENERATE = 0, 1, 2
REGISTER_RECORD_DTYPE = np.dtype([("status", "i4"), ("iterations", "i4"), ("n_corr", "i8"), ("sum_r2", "f8"), ("last_omega", "f8"),
                                  ("last_v", "f8"), ("skip_nan", "i4"), ("skip_range", "i4"), ("skip_label", "i4"), ("skip_no_corr", "i4"),
                                  ("skip_normal", "i4"), ("reserved", "i4")])
REGISTER_STATS = ("scans", "converged", "max_iterations", "degenerate", "correspondences", "iterations", "skipped", "points")


class NormalParams(C.Structure):
    """scvod_normal_params (16 bytes)"""
    _fields_ = [("radius", C.c_float), ("min_neighbours", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


NORMALS_STATS = ("queries", "finite", "below_min", "nonfinite_queries", "cloud_left_out", "largest_k", "sum_k", "zero")
NORMALS_QUERY_ORDER, NORMALS_ENTRY_ORDER, NORMALS_WAVE_BLOCKS = 1, 2, 4  # scvod_set_normals_variant


class ScanResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_points", "n_ground", "n_nonground", "n_dropped", "n_apri", "n_rejected",
                                          "n_voxels", "n_patches")] + \
               [(n, C.c_void_p) for n in ("cls", "ground_idx", "nonground_idx", "planes", "apri", "apri_src",
                                          "rejected_src", "vox_key", "vox_pt_begin", "vox_pts", "vox_av", "vox_cov")]


class TrackResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_apri", "n_clusters", "n_car_points", "n_dynamic_clusters", "n_dynamic_points",
                                          "reserved")] + \
               [(n, C.c_void_p) for n in ("cluster_root", "cluster_size", "cluster_state", "n_unique", "pair_begin",
                                          "pair_label", "pair_count", "pt_dyn")]


# ssc/ keys of config/*.yaml -> Params fields (include/utility.h:283-310)
YAML_KEYS = {"sensor_height_": "sensor_height", "min_dis_": "min_dis", "max_dis_": "max_dis", "min_angle_": "min_angle",
             "max_angle_": "max_angle", "min_azimuth_": "min_azimuth", "max_azimuth_": "max_azimuth",
             "range_res_": "range_res", "sector_res_": "sector_res", "azimuth_res_": "azimuth_res",
             "occupancy_": "occupancy", "max_z_": "max_z", "min_z_": "min_z", "car_square_": "car_square",
             "toBeClass_": "toBeClass"}

# values of the two YAML files shipped by the reference (config/semantickitti.yaml:24-55, config/parkinglot.yaml:23-48)
PRESETS = {
    "semantickitti": dict(sensor_height=1.73, min_dis=1.5, max_dis=30.0, min_angle=0.0, max_angle=360.0,
                          min_azimuth=-40.0, max_azimuth=80.0, range_res=0.4, sector_res=1.2, azimuth_res=2.0,
                          occupancy=0.4, max_z=0.8, min_z=-1.2, car_square=30.0, toBeClass=10),
    "parkinglot": dict(sensor_height=1.83, min_dis=0.8, max_dis=40.0, min_angle=0.0, max_angle=360.0,
                       min_azimuth=-30.0, max_azimuth=60.0, range_res=0.4, sector_res=1.2, azimuth_res=2.0,
                       occupancy=0.8, max_z=1.0, min_z=-1.0, car_square=2.0, toBeClass=6),
    # the parameters behind the reference's published seq-05 row (doc/note.txt:36: skip 5, max_z 4.0, min_z 1.0, car_square 50; its
    # refine_height / car_height / car_angle feed code that is commented out or out of scope): the committed YAML with those three
    "semantickitti_seq05": dict(sensor_height=1.73, min_dis=1.5, max_dis=30.0, min_angle=0.0, max_angle=360.0,
                                min_azimuth=-40.0, max_azimuth=80.0, range_res=0.4, sector_res=1.2, azimuth_res=2.0,
                                occupancy=0.4, max_z=4.0, min_z=1.0, car_square=50.0, toBeClass=10),
    # BASELINE.json configs[4]: OS1-128 stream with a 2x finer voxel grid
    "os128_fine": dict(sensor_height=1.73, min_dis=1.5, max_dis=30.0, min_angle=0.0, max_angle=360.0,
                       min_azimuth=-40.0, max_azimuth=80.0, range_res=0.2, sector_res=0.6, azimuth_res=1.0,
                       occupancy=0.4, max_z=0.8, min_z=-1.2, car_square=30.0, toBeClass=10),
}

_lib = None


def load_lib():
    """Load libscvod.so (after torch, so both share torch's HIP runtime).  Raises if missing."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        import torch  # noqa: F401  (must come first: one libamdhip64 per process)
    except Exception:
        pass
    path = os.path.abspath(os.environ.get("SCVOD_LIB", LIB_PATH))  # (SCVOD_LIB: a development build, e.g. libscvod_prof.so)
    if not os.path.exists(path):
        # the library is a build product (git-ignored): compile it in-tree when a hipcc is around
        import shutil
        import subprocess
        if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
            subprocess.check_call(["make", "-C", os.path.dirname(path)])
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the SCV-OD hot path has no CPU fallback)")
    lib = C.CDLL(path)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    sig = {
        "scvod_params_default": (None, [C.POINTER(Params)]),
        "scvod_pw_params_default": (None, [C.POINTER(PwParams)]),
        "scvod_grid_dims": (None, [C.POINTER(Params)] + [C.POINTER(i32)] * 4),
        "scvod_create": (C.c_int, [C.POINTER(Params), C.POINTER(PwParams), C.c_int, i64, i32, C.POINTER(vp)]),
        "scvod_destroy": (None, [vp]),
        "scvod_last_error": (C.c_char_p, [vp]),
        "scvod_arena_bytes": (i64, [vp]),
        "scvod_process_scan": (C.c_int, [vp, vp, i32, C.POINTER(ScanResult)]),
        "scvod_patchwork": (C.c_int, [vp, vp, i32, C.POINTER(ScanResult)]),
        "scvod_bin_scan": (C.c_int, [vp, vp, i32, i32, i32, C.POINTER(ScanResult)]),
        "scvod_voxelize": (C.c_int, [vp, vp, i32, C.POINTER(ScanResult)]),
        "scvod_pose_delta": (None, [vp, vp, vp]),
        "scvod_track_probe": (C.c_int, [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp]),
        "scvod_batch_process": (C.c_int, [vp, vp, vp, i32, vp, i32]),
        "scvod_batch_counts": (C.c_int, [vp, vp]),
        "scvod_batch_fetch": (C.c_int, [vp, i32, C.POINTER(ScanResult)]),
        "scvod_batch_cluster": (C.c_int, [vp, vp, i32]),
        "scvod_batch_fetch_clusters": (C.c_int, [vp, i32, vp, i32]),
        "scvod_cluster": (C.c_int, [vp, vp, i32, vp]),
        "scvod_batch_cluster_types": (C.c_int, [vp, vp, i32]),
        "scvod_batch_fetch_cluster_types": (C.c_int, [vp, i32, i32, i32, vp, i32]),
        "scvod_batch_track": (C.c_int, [vp, vp, vp, vp, i32, vp, i32]),
        "scvod_batch_fetch_track": (C.c_int, [vp, i32, C.POINTER(TrackResult)]),
        "scvod_batch_export_table": (C.c_int, [vp, i32, vp, i64, vp]),
        "scvod_set_track_mode": (C.c_int, [vp, i32, i32, i32]),
        "scvod_set_cluster_exact": (C.c_int, [vp, i32]),
        "scvod_batch_cluster_stats": (C.c_int, [vp, vp]),
        "scvod_batch_cluster_rule_stats": (C.c_int, [vp, vp]),
        "scvod_batch_cluster_help_stats": (C.c_int, [vp, vp]),
        "scvod_set_max_name_literal": (C.c_int, [vp, i32]),
        "scvod_set_intensity_merge": (C.c_int, [vp, i32, i32, f32, f32]),
        "scvod_batch_cluster_merge_stats": (C.c_int, [vp, vp]),
        "scvod_set_voxel_descriptors": (C.c_int, [vp, i32]),
        "scvod_set_region_growing": (C.c_int, [vp, i32, i32, i32, C.c_double, f32, C.c_double]),
        "scvod_batch_fetch_cluster_classes": (C.c_int, [vp, i32, i32, i32, i32, vp, i32]),
        "scvod_batch_fetch_region_growing": (C.c_int, [vp, i32, vp, vp, i32]),
        "scvod_batch_region_growing_stats": (C.c_int, [vp, vp]),
        "scvod_set_intensity_calibration": (C.c_int, [vp, i32, i32, f32]),
        "scvod_batch_fetch_intensity_calibration": (C.c_int, [vp, i32, vp, vp, i32]),
        "scvod_batch_intensity_calibration_stats": (C.c_int, [vp, vp]),
        "scvod_batch_intensity_calibration_candidates": (C.c_int, [vp, vp]),
        "scvod_batch_cluster_last_name": (C.c_int, [vp, vp, i32, vp]),
        "scvod_set_chain_capacity": (C.c_int, [vp, i64]),
        "scvod_chain_workspace_bytes": (i64, [vp]),
        "scvod_get_params": (C.c_int, [vp, vp]),
        "scvod_set_track_owned": (C.c_int, [vp, i32]),
        "scvod_set_track_halo": (C.c_int, [vp, vp, i32]),
        "scvod_batch_track_chains": (C.c_int, [vp, vp, i32]),
        "scvod_chain_state_bytes": (i64, [vp]),
        "scvod_chain_export_state": (C.c_int, [vp, i32, i32, vp, i64, vp]),
        "scvod_batch_track_resume": (C.c_int, [vp, vp, i32, vp, i32]),
        "scvod_batch_track_compare": (C.c_int, [vp, vp, i32, vp, vp]),
        "scvod_batch_track_compare_device": (C.c_int, [vp, vp, i32, vp, vp]),
        "scvod_batch_map_accumulate_range": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
        "scvod_batch_track_stats": (C.c_int, [vp, vp]),
        "scvod_batch_track_tables": (C.c_int, [vp, vp]),
        "scvod_map_create": (C.c_int, [C.c_int, i64, f32, C.POINTER(vp)]),
        "scvod_map_destroy": (None, [vp]),
        "scvod_map_last_error": (C.c_char_p, [vp]),
        "scvod_map_capacity": (i64, [vp]),
        "scvod_map_clear": (C.c_int, [vp, vp]),
        "scvod_pose_matrix": (None, [vp, vp]),
        "scvod_batch_map_accumulate": (C.c_int, [vp, vp, vp, i32, vp]),
        "scvod_map_export": (C.c_int, [vp, vp, i64, C.POINTER(i64), vp]),
        "scvod_map_merge": (C.c_int, [vp, vp, i64, vp]),
        "scvod_map_export_parts": (C.c_int, [vp, i32, vp, i64, vp, vp]),
        "scvod_map_export_parts_padded": (C.c_int, [vp, i32, vp, i64, vp, vp]),
        "scvod_map_points": (C.c_int, [vp, vp, vp, i64, C.POINTER(i64), vp]),
        "scvod_map_create_kind": (C.c_int, [C.c_int, i64, f32, i32, C.POINTER(vp)]),
        "scvod_map_kind": (i32, [vp]),
        "scvod_map_scratch_bytes": (i64, [vp]),
        "scvod_map_accumulate_labelled": (C.c_int, [vp, vp, vp, vp, i32, vp, vp, vp]),
        "scvod_batch_map_accumulate_classes": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
        "scvod_map_points_labelled": (C.c_int, [vp, vp, vp, vp, i64, vp, C.POINTER(i64), vp]),
        "scvod_map_query": (C.c_int, [vp, vp, vp, i32, vp, f32, vp, vp, vp, vp, vp, vp, vp]),
        "scvod_batch_map_query": (C.c_int, [vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, vp]),
        "scvod_map_query_stats": (C.c_int, [vp, vp]),
        "scvod_map_query_scratch_bytes": (i64, [vp]),
        "scvod_map_filter_params_default": (None, [C.POINTER(MapFilterParams)]),
        "scvod_map_filter": (C.c_int, [vp, vp, vp, i32, vp, C.POINTER(MapFilterParams), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "scvod_batch_map_filter": (C.c_int, [vp, vp, vp, C.POINTER(MapFilterParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
        "scvod_map_filter_stats": (C.c_int, [vp, vp]),
        "scvod_map_filter_scratch_bytes": (i64, [vp]),
        "scvod_batch_point_labels": (C.c_int, [vp, vp, i64, i32, vp]),
        "scvod_batch_export_points": (C.c_int, [vp, i32, vp, vp, vp, vp, vp, i64, vp, vp]),
        "scvod_batch_export_stats": (C.c_int, [vp, vp]),
        "scvod_batch_objects": (C.c_int, [vp, i32, vp, i64, vp, vp, i64, vp, vp]),
        "scvod_batch_objects_stats": (C.c_int, [vp, vp]),
        "scvod_batch_objects_scratch_bytes": (i64, [vp]),
        "scvod_feature_params_default": (None, [C.POINTER(FeatureParams)]),
        "scvod_set_object_features": (C.c_int, [vp, C.POINTER(FeatureParams)]),
        "scvod_batch_object_shapes": (C.c_int, [vp, vp, i64, vp]),
        "scvod_batch_object_shapes_stats": (C.c_int, [vp, vp]),
        "scvod_feature_row": (None, [vp, vp, vp]),
        "scvod_compare_feature": (f32, [vp, vp]),
        "scvod_esf_params_default": (None, [C.POINTER(EsfParams)]),
        "scvod_esf_device": (C.c_int, [vp, vp, vp, i64, C.POINTER(EsfParams), vp, vp, i64, vp]),
        "scvod_batch_object_esf": (C.c_int, [vp, C.POINTER(EsfParams), vp, vp, i64, vp]),
        "scvod_esf_stats": (C.c_int, [vp, vp]),
        "scvod_esf_scratch_bytes": (i64, [vp]),
        "scvod_esf_fold10": (None, [vp, vp]),
        "scvod_feature_row21": (None, [vp, vp, vp, vp]),
        "scvod_batch_timings": (C.c_int, [vp, vp, vp, i32]),
        "scvod_set_timing": (C.c_int, [vp, i32]),
        "scvod_nn_search": (C.c_int, [vp, vp, i32, vp, i32, f32, vp, vp, vp]),
        "scvod_nn_radius_search": (C.c_int, [vp, vp, i32, vp, i32, f32, vp, vp]),
        "scvod_nn_search_device": (C.c_int, [vp, vp, i32, vp, i32, f32, vp, vp, vp, vp]),
        "scvod_eval_params_default": (None, [C.POINTER(EvalParams)]),
        "scvod_eval_finish": (None, [vp, C.POINTER(EvalResult)]),
        "scvod_evaluate_device": (C.c_int, [vp, vp, vp, i32, vp, vp, i32, C.POINTER(EvalParams), vp, vp]),
        "scvod_batch_evaluate": (C.c_int, [vp, vp, vp, i32, C.POINTER(EvalParams), vp, vp]),
        "scvod_evaluate_stats": (C.c_int, [vp, C.POINTER(EvalResult)]),
        "scvod_evaluate_scratch_bytes": (i64, [vp]),
        "scvod_classify_map_device": (C.c_int, [vp, vp, vp, i32, vp, i32, vp, i32, f32, f32, vp, vp]),
        "scvod_classify_map_stats": (C.c_int, [vp, vp]),
        "scvod_batch_point_classes": (C.c_int, [vp, vp, i64, i32, vp]),
        "scvod_class_params_default": (None, [C.POINTER(ClassParams)]),
        "scvod_class_finish": (None, [vp, C.POINTER(ClassResult)]),
        "scvod_score_classes_device": (C.c_int, [vp, vp, vp, i32, vp, vp, i32, C.POINTER(ClassParams), vp, vp]),
        "scvod_batch_score_classes": (C.c_int, [vp, vp, vp, i32, C.POINTER(ClassParams), vp, vp]),
        "scvod_score_classes_stats": (C.c_int, [vp, C.POINTER(ClassResult)]),
        "scvod_score_classes_pass2_queries": (i64, [vp]),
        "scvod_score_classes_scratch_bytes": (i64, [vp]),
        "scvod_score_instances_device": (C.c_int, [vp, vp, vp, i64, vp, i32, vp, vp]),
        "scvod_score_instances_stats": (C.c_int, [vp, vp]),
        "scvod_score_instances_scratch_bytes": (i64, [vp]),
        "scvod_set_score_instances_variant": (C.c_int, [vp, i32]),
        "scvod_instance_params_default": (None, [C.POINTER(InstanceParams)]),
        "scvod_instance_finish": (C.c_int, [vp, i64, C.POINTER(InstanceParams), C.POINTER(InstanceResult)]),
        "scvod_instance_merge": (C.c_int, [vp, i64, vp, i64, vp, i64, C.POINTER(i64)]),
        "scvod_batch_object_truth": (C.c_int, [vp, vp, C.POINTER(EvalParams), vp, i64, vp]),
        "scvod_batch_object_truth_stats": (C.c_int, [vp, vp]),
        "scvod_batch_object_truth_scratch_bytes": (i64, [vp]),
        "scvod_object_truth_params_default": (None, [C.POINTER(ObjectTruthParams)]),
        "scvod_object_truth_finish": (C.c_int, [vp, vp, i64, C.POINTER(ObjectTruthParams), C.POINTER(ObjectTruthResult)]),
        "scvod_split_params_default": (None, [C.POINTER(SplitParams)]),
        "scvod_map_split_device": (C.c_int, [vp, vp, vp, i32, vp, i32, C.POINTER(SplitParams), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "scvod_map_split_stats": (C.c_int, [vp, vp]),
        "scvod_map_split_scratch_bytes": (i64, [vp]),
        "scvod_map_split": (C.c_int, [vp, vp, vp, i32, vp, i32, C.POINTER(SplitParams), vp, vp, vp, vp]),
        "scvod_batch_voxelgrid": (C.c_int, [vp, vp, vp, vp, i32, vp, f32, vp, i64, vp, vp]),
        "scvod_voxelgrid": (C.c_int, [vp, vp, vp, i32, vp, f32, vp, i32, vp]),
        "scvod_stack_offsets": (C.c_int, [vp, i32, i32, i32, i32, vp, vp, i32, vp]),
        "scvod_pose_from_matrix": (None, [vp, vp]),
        "scvod_batch_stack_scans": (C.c_int, [vp, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, i64, vp]),
        "scvod_stack_scans": (C.c_int, [vp, vp, vp, i32, vp, i32, i32, i32, vp, i64]),
        "scvod_stack_scratch_bytes": (i64, [vp]),
        "scvod_visibility_params_default": (None, [C.POINTER(VisibilityParams)]),
        "scvod_visibility_viewers": (C.c_int, [vp, i32, i32, i32, vp, vp, i32]),
        "scvod_visibility_device": (C.c_int, [vp, vp, vp, i32, vp, vp, vp, C.POINTER(VisibilityParams), vp, vp, vp, vp, vp]),
        "scvod_batch_visibility": (C.c_int, [vp, vp, vp, C.POINTER(VisibilityParams), i32, vp, vp, vp, vp, vp]),
        "scvod_visibility_stats": (C.c_int, [vp, vp]),
        "scvod_visibility_scratch_bytes": (i64, [vp]),
        "scvod_cloud_visibility_params_default": (None, [C.POINTER(CloudVisibilityParams)]),
        "scvod_cloud_visibility_device": (C.c_int, [vp, vp, i64, vp, vp, i32, C.POINTER(CloudVisibilityParams), i32, vp, vp, vp]),
        "scvod_cloud_visibility_stats": (C.c_int, [vp, vp]),
        "scvod_cloud_visibility_scratch_bytes": (i64, [vp]),
        "scvod_object_visibility_params_default": (None, [C.POINTER(ObjectVisibilityParams)]),
        "scvod_batch_object_visibility": (C.c_int, [vp, vp, vp, vp, C.POINTER(ObjectVisibilityParams), vp, i64, vp, vp]),
        "scvod_batch_object_visibility_stats": (C.c_int, [vp, vp]),
        "scvod_batch_object_visibility_scratch_bytes": (i64, [vp]),
        "scvod_track_params_default": (None, [C.POINTER(TrackParams)]),
        "scvod_object_tracks_device": (C.c_int, [vp, vp, vp, i32, vp, vp, vp, vp, C.POINTER(TrackParams), vp, i64, vp, i64, vp, vp, vp]),
        "scvod_batch_object_tracks": (C.c_int, [vp, vp, vp, C.POINTER(TrackParams), vp, i64, vp, i64, vp, vp, vp]),
        "scvod_object_tracks_stats": (C.c_int, [vp, vp]),
        "scvod_object_tracks_scratch_bytes": (i64, [vp]),
        "scvod_tracks_finish": (C.c_int, [vp, i64, C.c_double, C.POINTER(TracksResult)]),
        "scvod_track_visibility_params_default": (None, [C.POINTER(TrackVisibilityParams)]),
        "scvod_track_visibility_device": (C.c_int, [vp, vp, vp, i32, vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, i64,
                                                    C.POINTER(TrackVisibilityParams), vp, i64, vp, i64, vp]),
        "scvod_track_visibility_stats": (C.c_int, [vp, vp]),
        "scvod_track_visibility_scratch_bytes": (i64, [vp]),
        "scvod_map_components": (C.c_int, [vp, vp, i64, i32, vp, vp, i64, vp, vp]),
        "scvod_map_components_stats": (C.c_int, [vp, vp]),
        "scvod_map_components_scratch_bytes": (i64, [vp]),
        "scvod_component_visibility_params_default": (None, [C.POINTER(ComponentVisibilityParams)]),
        "scvod_map_component_visibility": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, C.POINTER(ComponentVisibilityParams), vp, i64, vp, vp]),
        "scvod_map_component_visibility_stats": (C.c_int, [vp, vp]),
        "scvod_register_params_default": (None, [C.POINTER(RegisterParams)]),
        "scvod_register_check": (C.c_int, [C.POINTER(RegisterParams), f32, i32, vp]),
        "scvod_map_register": (C.c_int, [vp, vp, vp, i32, vp, vp, C.POINTER(RegisterParams), vp, vp, vp, vp]),
        "scvod_batch_map_register": (C.c_int, [vp, vp, vp, vp, C.POINTER(RegisterParams), vp, vp, vp, vp]),
        "scvod_map_register_stats": (C.c_int, [vp, vp]),
        "scvod_map_register_scratch_bytes": (i64, [vp]),
        "scvod_register_device": (C.c_int, [vp, vp, vp, i32, vp, vp, vp, vp, i32, C.POINTER(RegisterParams), vp, vp, vp]),
        "scvod_register_stats": (C.c_int, [vp, vp]),
        "scvod_register_scratch_bytes": (i64, [vp]),
        "scvod_normal_params_default": (None, [C.POINTER(NormalParams)]),
        "scvod_normals_check": (C.c_int, [C.POINTER(NormalParams), i32, i64, i32, i64, vp, vp, i32]),
        "scvod_normals_device": (C.c_int, [vp, vp, i32, i32, vp, i32, i32, vp, vp, i32, C.POINTER(NormalParams), vp, vp, vp, vp, vp]),
        "scvod_normals_stats": (C.c_int, [vp, vp]),
        "scvod_normals_scratch_bytes": (i64, [vp]),
        "scvod_map_points_normals": (C.c_int, [vp, vp, C.POINTER(NormalParams), vp, vp, vp, vp, vp, i64, vp, vp]),
        "scvod_set_normals_variant": (C.c_int, [vp, i32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # raises AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


EXPORTED_SYMBOLS = ["scvod_params_default", "scvod_pw_params_default", "scvod_grid_dims", "scvod_create",
                    "scvod_destroy", "scvod_last_error", "scvod_arena_bytes", "scvod_process_scan", "scvod_patchwork",
                    "scvod_bin_scan", "scvod_voxelize", "scvod_pose_delta", "scvod_track_probe", "scvod_batch_process",
                    "scvod_batch_counts", "scvod_batch_fetch", "scvod_batch_cluster", "scvod_batch_fetch_clusters", "scvod_cluster",
                    "scvod_batch_cluster_types", "scvod_batch_fetch_cluster_types",
                    "scvod_batch_track", "scvod_batch_fetch_track", "scvod_set_track_mode", "scvod_set_cluster_exact", "scvod_batch_cluster_stats", "scvod_batch_cluster_rule_stats", "scvod_batch_cluster_help_stats", "scvod_set_max_name_literal", "scvod_set_intensity_merge", "scvod_batch_cluster_merge_stats", "scvod_set_voxel_descriptors", "scvod_set_region_growing", "scvod_batch_fetch_cluster_classes", "scvod_batch_fetch_region_growing", "scvod_batch_region_growing_stats", "scvod_set_intensity_calibration", "scvod_batch_fetch_intensity_calibration", "scvod_batch_intensity_calibration_stats", "scvod_batch_intensity_calibration_candidates", "scvod_batch_cluster_last_name", "scvod_set_chain_capacity", "scvod_chain_workspace_bytes", "scvod_get_params", "scvod_set_track_owned", "scvod_set_track_halo", "scvod_batch_track_chains", "scvod_chain_state_bytes", "scvod_chain_export_state", "scvod_batch_track_resume", "scvod_batch_track_compare", "scvod_batch_track_compare_device", "scvod_batch_map_accumulate_range", "scvod_batch_track_stats", "scvod_batch_export_table", "scvod_batch_track_tables", "scvod_sequence_ingest",
                    "scvod_map_create", "scvod_map_destroy", "scvod_map_last_error", "scvod_map_capacity", "scvod_map_clear",
                    "scvod_pose_matrix", "scvod_batch_map_accumulate", "scvod_map_export", "scvod_map_export_parts", "scvod_map_export_parts_padded", "scvod_map_merge", "scvod_map_points",
                    "scvod_map_create_kind", "scvod_map_kind", "scvod_map_scratch_bytes", "scvod_map_accumulate_labelled",
                    "scvod_batch_map_accumulate_classes", "scvod_map_points_labelled",
                    "scvod_map_query", "scvod_batch_map_query", "scvod_map_query_stats", "scvod_map_query_scratch_bytes",
                    "scvod_map_filter_params_default", "scvod_map_filter", "scvod_batch_map_filter", "scvod_map_filter_stats",
                    "scvod_map_filter_scratch_bytes",
                    "scvod_batch_point_labels", "scvod_batch_export_points", "scvod_batch_export_stats",
                    "scvod_batch_objects", "scvod_batch_objects_stats", "scvod_batch_objects_scratch_bytes",
                    "scvod_feature_params_default", "scvod_set_object_features", "scvod_batch_object_shapes", "scvod_batch_object_shapes_stats",
                    "scvod_feature_row", "scvod_compare_feature",
                    "scvod_batch_timings", "scvod_set_timing", "scvod_nn_search", "scvod_nn_radius_search", "scvod_nn_search_device", "scvod_batch_voxelgrid", "scvod_voxelgrid",
                    "scvod_eval_params_default", "scvod_eval_finish", "scvod_evaluate_device", "scvod_batch_evaluate", "scvod_evaluate_stats",
                    "scvod_evaluate_scratch_bytes", "scvod_classify_map_device", "scvod_classify_map_stats",
                    "scvod_batch_point_classes", "scvod_class_params_default", "scvod_class_finish", "scvod_score_classes_device",
                    "scvod_batch_score_classes", "scvod_score_classes_stats", "scvod_score_classes_pass2_queries",
                    "scvod_score_classes_scratch_bytes",
                    "scvod_score_instances_device", "scvod_score_instances_stats", "scvod_score_instances_scratch_bytes",
                    "scvod_set_score_instances_variant", "scvod_instance_params_default", "scvod_instance_finish", "scvod_instance_merge",
                    "scvod_batch_object_truth", "scvod_batch_object_truth_stats", "scvod_batch_object_truth_scratch_bytes",
                    "scvod_object_truth_params_default", "scvod_object_truth_finish",
                    "scvod_stack_offsets", "scvod_pose_from_matrix", "scvod_batch_stack_scans", "scvod_stack_scans",
                    "scvod_stack_scratch_bytes",
                    "scvod_visibility_params_default", "scvod_visibility_viewers", "scvod_visibility_device", "scvod_batch_visibility",
                    "scvod_visibility_stats", "scvod_visibility_scratch_bytes",
                    "scvod_cloud_visibility_params_default", "scvod_cloud_visibility_device", "scvod_cloud_visibility_stats",
                    "scvod_cloud_visibility_scratch_bytes",
                    "scvod_object_visibility_params_default", "scvod_batch_object_visibility", "scvod_batch_object_visibility_stats",
                    "scvod_batch_object_visibility_scratch_bytes",
                    "scvod_track_params_default", "scvod_object_tracks_device", "scvod_batch_object_tracks", "scvod_object_tracks_stats",
                    "scvod_object_tracks_scratch_bytes", "scvod_tracks_finish",
                    "scvod_track_visibility_params_default", "scvod_track_visibility_device", "scvod_track_visibility_stats",
                    "scvod_track_visibility_scratch_bytes",
                    "scvod_map_components","scvod_map_components_stats", "scvod_map_components_scratch_bytes",
                    "scvod_component_visibility_params_default", "scvod_map_component_visibility",
                    "scvod_map_component_visibility_stats",
                    "scvod_split_params_default", "scvod_map_split_device", "scvod_map_split_stats", "scvod_map_split_scratch_bytes",
                    "scvod_map_split",
                    "scvod_register_params_default", "scvod_register_check", "scvod_map_register", "scvod_batch_map_register",
                    "scvod_map_register_stats", "scvod_map_register_scratch_bytes", "scvod_register_device", "scvod_register_stats",
                    "scvod_register_scratch_bytes",
                    "scvod_normal_params_default", "scvod_normals_check", "scvod_normals_device", "scvod_normals_stats",
                    "scvod_normals_scratch_bytes", "scvod_map_points_normals", "scvod_set_normals_variant",
                    "scvod_esf_params_default", "scvod_esf_device", "scvod_batch_object_esf", "scvod_esf_stats", "scvod_esf_scratch_bytes",
                    "scvod_esf_fold10", "scvod_feature_row21"]


def register_params_default(use256=None, **kw):
    """scvod_register_params with this project's (untuned) defaults, overridden by keyword (lam: the struct's lambda).  use256: None
    (every label), a [256] array, or the labels that take part; the bytes stay alive with the returned struct"""
    p = RegisterParams()
    load_lib().scvod_register_params_default(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    if use256 is not None:
        a = np.asarray(use256)
        if a.shape != (256,):
            a = np.zeros(256, np.uint8)
            a[np.asarray(use256, np.int64).reshape(-1)] = 1
        p._use_bytes = np.ascontiguousarray(a != 0, np.uint8)
        p.use256 = p._use_bytes.ctypes.data
    return p


def register_check(params=None, leaf=0.0, has_normals=False, d_src_xyzi=0):
    """scvod_register_check: the status (0 or SCVOD_ERR_INVALID) the register calls would return before touching a device"""
    return int(load_lib().scvod_register_check(C.byref(params) if params is not None else None, float(leaf), int(bool(has_normals)),
                                               C.c_void_p(int(d_src_xyzi))))


def register_result(d_pose_out, d_records):
    """the outputs of a register call on the host (synchronises): dict(matrices float64 [n_scans, 3, 4], poses float32 [n_scans, 6] =
    {x, y, z, roll, pitch, yaw} of the matrices narrowed to float (scvod_pose_from_matrix: NOT a bit-exact round trip), records
    REGISTER_RECORD_DTYPE [n_scans])"""
    M = d_pose_out.cpu().numpy().reshape(-1, 3, 4)
    rec = d_records.cpu().numpy().view(np.uint8).reshape(-1)[:64 * len(M)].view(REGISTER_RECORD_DTYPE)
    poses = np.stack([pose_from_matrix(m.astype(np.float32)) for m in M]) if len(M) else np.zeros((0, 6), np.float32)
    return dict(matrices=M, poses=poses, records=rec)


def _register_outputs(n_scans, device):
    import torch
    dev = torch.device("cuda", device)
    return (torch.empty((max(n_scans, 1), 12), dtype=torch.float64, device=dev)[:n_scans],
            torch.empty((max(n_scans, 1) * 64,), dtype=torch.uint8, device=dev)[:64 * n_scans])


def normal_params_default(**kw):
    """scvod_normal_params with this project's (untuned) defaults -- radius 0.5, min_neighbours 5 -- overridden by keyword"""
    p = NormalParams()
    load_lib().scvod_normal_params_default(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def normals_check(params=None, cloud_stride=3, n_cloud=0, query_stride=0, n_query=0, seg_offsets=None, viewpoints=None, n_segments=None):
    """scvod_normals_check: the status (0 or SCVOD_ERR_INVALID) the normals calls would return before touching a device"""
    seg = None if seg_offsets is None else np.ascontiguousarray(seg_offsets, np.int32)
    view = None if viewpoints is None else np.ascontiguousarray(viewpoints, np.float32)
    if n_segments is None:
        n_segments = 0 if seg is None else len(seg) - 1
    return int(load_lib().scvod_normals_check(C.byref(params) if params is not None else None, int(cloud_stride), int(n_cloud), int(query_stride),
                                              int(n_query), None if seg is None else seg.ctypes.data_as(C.c_void_p),
                                              None if view is None else view.ctypes.data_as(C.c_void_p), int(n_segments)))


def eval_params_default(voxelsize=None, dynamic_classes=None):
    """scvod_eval_params with the reference's defaults (voxelsize 0.2, the classes 252..259), overridden by keyword"""
    p = EvalParams()
    load_lib().scvod_eval_params_default(C.byref(p))
    if voxelsize is not None:
        p.voxelsize = float(voxelsize)
    if dynamic_classes is not None:
        cl = [int(v) for v in dynamic_classes]
        p.n_dynamic_classes = len(cl)  # (more than 16: the library refuses the call)
        for k, v in enumerate(cl[:16]):
            p.dynamic_classes[k] = v
    return p


def _eval_dict(r):
    return {k: getattr(r, k) for k, _ in EvalResult._fields_}


def eval_finish(counts):
    """the seven counts of metric.preservation_rejection (in EVAL_RESULT's order) -> the dict with PR / RR / F1.  Host only"""
    cnt = np.ascontiguousarray(counts, np.int64)
    assert cnt.size == 7
    r = EvalResult()
    load_lib().scvod_eval_finish(cnt.ctypes.data_as(C.c_void_p), C.byref(r))
    return _eval_dict(r)


def class_params_default(max_dist=None, cell=None, ground=None, building=None, tree=None):
    """scvod_class_params with the reference's lists (plotObject.cpp:3-5), max_dist 0.75 and cell 0.25, overridden by keyword"""
    p = ClassParams()
    load_lib().scvod_class_params_default(C.byref(p))
    if max_dist is not None:
        p.max_dist = float(max_dist)
    if cell is not None:
        p.cell = float(cell)
    for name, lst in (("ground", ground), ("building", building), ("tree", tree)):
        if lst is not None:
            cl = [int(v) for v in lst]
            setattr(p, "n_" + name, len(cl))  # (more than 8: the library refuses the call)
            arr = getattr(p, name)
            for k in range(8):
                arr[k] = cl[k] if k < len(cl) else 0
    return p


def _class_dict(r):
    return dict(conf=[[int(v) for v in row] for row in r.conf], pd_far=int(r.pd_far), num=[int(v) for v in r.num], P=[int(v) for v in r.P],
                rate_P=np.asarray(list(r.rate_P), np.float32), rate_N=np.asarray(list(r.rate_N), np.float32))


def class_finish(conf_and_far):
    """conf (4 x 5, row-major) and pd_far, 21 counts -> the dict with num, P, rate_P, rate_N (fp32).  Host only"""
    cnt = np.ascontiguousarray(conf_and_far, np.int64).reshape(-1)
    assert cnt.size == 21
    r = ClassResult()
    load_lib().scvod_class_finish(cnt.ctypes.data_as(C.c_void_p), C.byref(r))
    return _class_dict(r)


def instance_params_default(dynamic_classes=None, static_classes=None, removed_below=None, retained_from=None, min_points=None):
    """scvod_instance_params with the defaults (dynamic 252..259, their static counterparts, both thresholds 0.5, min_points 1),
    overridden by keyword"""
    p = InstanceParams()
    load_lib().scvod_instance_params_default(C.byref(p))
    for name, lst in (("dynamic_classes", dynamic_classes), ("static_classes", static_classes)):
        if lst is not None:
            cl = [int(v) for v in lst]
            setattr(p, "n_" + name, len(cl))  # (more than 16: scvod_instance_finish refuses them)
            arr = getattr(p, name)
            for k in range(16):
                arr[k] = cl[k] if k < len(cl) else 0
    if removed_below is not None:
        p.removed_below = float(removed_below)
    if retained_from is not None:
        p.retained_from = float(retained_from)
    if min_points is not None:
        p.min_points = int(min_points)
    return p


def _status(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with status {rc}")


def instance_finish(table, params=None):
    """a table of INSTANCE_DTYPE records -> the dict of scvod_instance_result (object counts, point sums, the two rates).  Host only"""
    t = np.ascontiguousarray(table, INSTANCE_DTYPE).reshape(-1)
    r = InstanceResult()
    _status(load_lib().scvod_instance_finish(t.ctypes.data_as(C.c_void_p) if t.size else None, t.size,
                                             C.byref(params) if params is not None else None, C.byref(r)), "scvod_instance_finish")
    return {k: getattr(r, k) for k, _ in InstanceResult._fields_}


def map_filter_params_default(**kw):
    """scvod_map_filter_params with the defaults (radius 0, flags 0, vote 1 / 2, min_points 1), overridden by keyword"""
    p = MapFilterParams()
    load_lib().scvod_map_filter_params_default(C.byref(p))
    for name, value in kw.items():
        assert name in dict(MapFilterParams._fields_), name
        setattr(p, name, value)
    return p


def object_truth_params_default(moving_from=None, pure_from=None, min_points=None):
    """scvod_object_truth_params with the defaults (both thresholds 0.5, min_points 1), overridden by keyword"""
    p = ObjectTruthParams()
    load_lib().scvod_object_truth_params_default(C.byref(p))
    if moving_from is not None:
        p.moving_from = float(moving_from)
    if pure_from is not None:
        p.pure_from = float(pure_from)
    if min_points is not None:
        p.min_points = int(min_points)
    return p


def object_truth_finish(objects, truth, params=None):
    """the OBJECT_DTYPE records of a table and the OBJECT_TRUTH_DTYPE records of batch_object_truth on it -> the dict of
    scvod_object_truth_result (object counts, precision and recall of the dynamic flag).  Host only"""
    o = np.ascontiguousarray(objects, OBJECT_DTYPE).reshape(-1)
    t = np.ascontiguousarray(truth, OBJECT_TRUTH_DTYPE).reshape(-1)
    assert o.size == t.size
    r = ObjectTruthResult()
    _status(load_lib().scvod_object_truth_finish(o.ctypes.data_as(C.c_void_p) if o.size else None, t.ctypes.data_as(C.c_void_p) if t.size else None,
                                                 o.size, C.byref(params) if params is not None else None, C.byref(r)), "scvod_object_truth_finish")
    return {k: getattr(r, k) for k, _ in ObjectTruthResult._fields_}


def instance_merge(a, b):
    """two tables ascending by key -> one: counts added, first_point the smaller of the two.  Host only"""
    a = np.ascontiguousarray(a, INSTANCE_DTYPE).reshape(-1)
    b = np.ascontiguousarray(b, INSTANCE_DTYPE).reshape(-1)
    out = np.zeros(a.size + b.size, INSTANCE_DTYPE)
    n = C.c_int64(0)
    _status(load_lib().scvod_instance_merge(a.ctypes.data_as(C.c_void_p) if a.size else None, a.size,
                                            b.ctypes.data_as(C.c_void_p) if b.size else None, b.size,
                                            out.ctypes.data_as(C.c_void_p) if out.size else None, out.size, C.byref(n)), "scvod_instance_merge")
    return out[:n.value].copy()


def visibility_params_default(**kw):
    """scvod_visibility_params with the defaults (2 viewers on each side, halo 0, gap 0.4 m + 2 %, min_through 2, vote 1 / 2),
    overridden by keyword"""
    p = VisibilityParams()
    load_lib().scvod_visibility_params_default(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def cloud_visibility_params_default(**kw):
    """scvod_cloud_visibility_params with the defaults (halo 0, gap 0.4 m + 2 %, max_range 0, min_through 2, vote 1 / 2: the scan
    stage's values, not tuned for maps), overridden by keyword"""
    p = CloudVisibilityParams()
    load_lib().scvod_cloud_visibility_params_default(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def object_visibility_params_default(**kw):
    """scvod_object_visibility_params with the defaults (flags 0, min_points 1, min_tested 1, min_through 2, vote 1 / 2: this project's
    values, not from real data), overridden by keyword"""
    p = ObjectVisibilityParams()
    load_lib().scvod_object_visibility_params_default(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def track_params_default(**kw):
    """scvod_track_params with the defaults (flags 0, occupancy -1 = the ctx's, gate 2.0, size_ratio 1.5, min_points 10, min_length 2:
    this project's values, not from real data and untuned), overridden by keyword"""
    p = TrackParams()
    load_lib().scvod_track_params_default(C.byref(p))
    for k, v in kw.items():
        assert k in {f[0] for f in TrackParams._fields_} - {"reserved"}, k
        setattr(p, k, v)
    return p


def track_visibility_params_default(**kw):
    """scvod_track_visibility_params with the defaults (flags 0, window 0, min_travel 2.0, min_length 2, min_moved 1, min_flagged 2,
    vote 1 / 2: this project's values, not from real data and untuned), overridden by keyword"""
    p = TrackVisibilityParams()
    load_lib().scvod_track_visibility_params_default(C.byref(p))
    for k, v in kw.items():
        assert k in {f[0] for f in TrackVisibilityParams._fields_} - {"reserved"}, k
        setattr(p, k, v)
    return p


def tracks_finish(tracks, min_travel):
    """TRACK_DTYPE records -> the dict of scvod_tracks_result: tracks, moving / still tracks, members and dynamic members, and the two
    rates in percent (NaN for a zero denominator); a track moves iff |net| >= min_travel.  Host only"""
    t = np.ascontiguousarray(tracks, TRACK_DTYPE).reshape(-1)
    r = TracksResult()
    rc = load_lib().scvod_tracks_finish(t.ctypes.data_as(C.c_void_p) if t.size else None, int(t.size), float(min_travel), C.byref(r))
    if rc != 0:
        raise RuntimeError(f"scvod_tracks_finish failed with status {rc}")
    return {k: getattr(r, k) for k, _ in TracksResult._fields_}


def component_visibility_params_default(**kw):
    """scvod_component_visibility_params with the library's defaults (flags 0, min_cells 1, max_cells 0 = no limit, min_tested 1,
    min_through 2, vote 1 / 2: this project's values, not from real data), overridden by keyword"""
    p = ComponentVisibilityParams()
    load_lib().scvod_component_visibility_params_default(C.byref(p))
    for k, v in kw.items():
        assert k in {f[0] for f in ComponentVisibilityParams._fields_} - {"reserved"}, k
        setattr(p, k, int(v))
    return p


def visibility_viewers(n_scans, next_scan=None, before=2, after=2):
    """the viewer lists of the vote (host only): (begin [n_scans + 1], viewers): per scan the successors along next_scan, nearest first,
    then the predecessors"""
    nx = None if next_scan is None else np.ascontiguousarray(next_scan, np.int32)
    assert nx is None or nx.shape[0] == n_scans
    begin = np.zeros(int(n_scans) + 1, np.int32)
    cap = max(int(n_scans) * (int(before) + int(after)), 1) if 0 <= before <= 64 and 0 <= after <= 64 else 1
    viewers = np.zeros(cap, np.int32)
    n = load_lib().scvod_visibility_viewers(None if nx is None else nx.ctypes.data_as(C.c_void_p), int(n_scans), int(before), int(after),
                                            begin.ctypes.data_as(C.c_void_p), viewers.ctypes.data_as(C.c_void_p), cap)
    _status(min(n, 0), "scvod_visibility_viewers")
    return begin, viewers[:n]


def split_params_default(cell=None, max_rings=None, base_stride=None, query_stride=None, reject_classes=None):
    """scvod_split_params with the defaults (cell 0.2, max_rings 3, packed xyz on both sides, no reject class), overridden by keyword;
    reject_classes=(252,) is the gate of SSC::segDF's evaluation block"""
    p = SplitParams()
    load_lib().scvod_split_params_default(C.byref(p))
    if cell is not None:
        p.cell = float(cell)
    for name, v in (("max_rings", max_rings), ("base_stride", base_stride), ("query_stride", query_stride)):
        if v is not None:
            setattr(p, name, int(v))
    if reject_classes is not None:
        cl = [int(v) for v in reject_classes]
        p.n_reject_classes = len(cl)  # (more than 16: the library refuses the call)
        for k in range(16):
            p.reject_classes[k] = cl[k] if k < len(cl) else 0
    return p


def feature_params(**kw):
    """scvod_feature_params with the reference's defaults (utility.h:318-325), fields overridden by keyword"""
    p = FeatureParams()
    load_lib().scvod_feature_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, float(v))
    return p


def feature_row(obj, shape=None):
    """the 11-value row of getDescriptorByEigenValue from one OBJECT_DTYPE record and, optionally, its OBJECT_SHAPE_DTYPE record
    (None: the six constants 1.0).  Host only"""
    o = np.ascontiguousarray(obj, OBJECT_DTYPE).reshape(1)
    sh = np.ascontiguousarray(shape, OBJECT_SHAPE_DTYPE).reshape(1) if shape is not None else None
    out = np.zeros(11, np.float64)
    load_lib().scvod_feature_row(o.ctypes.data_as(C.c_void_p), sh.ctypes.data_as(C.c_void_p) if sh is not None else None,
                                 out.ctypes.data_as(C.c_void_p))
    return out


def esf_params_default(**kw):
    """scvod_esf_params with the defaults (20000 samples, seed 0, min_points 3, every class), fields overridden by keyword"""
    p = EsfParams()
    load_lib().scvod_esf_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, int(v))
    return p


def esf_fold10(sig640):
    """fold10 of one normalised 640-value signature (float32 [10]).  Host only"""
    sig = np.ascontiguousarray(sig640, np.float32)
    assert sig.size == ESF_SIG
    out = np.zeros(10, np.float32)
    load_lib().scvod_esf_fold10(sig.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def feature_row21(obj, shape, esf):
    """SSC::getFeature21: feature_row(obj, shape) and the fold10 of one OBJECT_ESF_DTYPE record.  Host only"""
    o = np.ascontiguousarray(obj, OBJECT_DTYPE).reshape(1)
    sh = np.ascontiguousarray(shape, OBJECT_SHAPE_DTYPE).reshape(1) if shape is not None else None
    e = np.ascontiguousarray(esf, OBJECT_ESF_DTYPE).reshape(1)
    out = np.zeros(21, np.float64)
    load_lib().scvod_feature_row21(o.ctypes.data_as(C.c_void_p), sh.ctypes.data_as(C.c_void_p) if sh is not None else None,
                                   e.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def compare_feature(a, b):
    """SSC::compareFeature of two 11-value rows (a float).  Host only"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.size >= 10 and b.size >= 10
    return float(load_lib().scvod_compare_feature(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))


def make_params(preset=None, **kw):
    p = Params()
    load_lib().scvod_params_default(C.byref(p))
    vals = dict(PRESETS[preset]) if preset else {}
    vals.update(kw)
    for k, v in vals.items():
        setattr(p, k, v)
    return p


def params_from_yaml(path):
    """Reads the `ssc:` block of a reference YAML file (config/*.yaml) into Params; keys that the
    hot path does not use are ignored, missing keys keep the nh.param<> defaults."""
    import yaml
    with open(path) as f:
        doc = yaml.safe_load(f)
    p = make_params()
    for k, v in (doc.get("ssc") or {}).items():
        if k in YAML_KEYS:
            setattr(p, YAML_KEYS[k], int(v) if YAML_KEYS[k] == "toBeClass" else float(v))
    return p


def grid_dims(p):
    out = [C.c_int32() for _ in range(4)]
    load_lib().scvod_grid_dims(C.byref(p), *[C.byref(o) for o in out])
    return tuple(o.value for o in out)


def _arr(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n).copy()


def _unpack(r):
    d = {k: getattr(r, k) for k in ("n_points", "n_ground", "n_nonground", "n_dropped", "n_apri", "n_rejected",
                                    "n_voxels", "n_patches")}
    d["cls"] = _arr(r.cls, r.n_points, np.uint8)
    d["ground_idx"] = _arr(r.ground_idx, r.n_ground, np.int32)
    d["nonground_idx"] = _arr(r.nonground_idx, r.n_nonground, np.int32)
    d["planes"] = _arr(r.planes, r.n_patches, PLANE_DTYPE)
    d["apri"] = _arr(r.apri, r.n_apri, APRI_DTYPE)
    d["apri_src"] = _arr(r.apri_src, r.n_apri, np.int32)
    d["rejected_src"] = _arr(r.rejected_src, r.n_rejected, np.int32)
    d["vox_key"] = _arr(r.vox_key, r.n_voxels, np.int32)
    d["vox_pt_begin"] = _arr(r.vox_pt_begin, r.n_voxels + 1, np.int32)
    d["vox_pts"] = _arr(r.vox_pts, r.n_apri if r.n_voxels else 0, np.int32)
    d["vox_av"] = _arr(r.vox_av, r.n_voxels, np.float32)
    d["vox_cov"] = _arr(r.vox_cov, r.n_voxels, np.float32)
    return d


class ScvodError(RuntimeError):
    pass


class Ctx:
    def __init__(self, params, max_points_total, max_scans=1, device=0, pw=None):
        self.lib = load_lib()
        self.params = params
        self.device = int(device)
        self.h = C.c_void_p()
        rc = self.lib.scvod_create(C.byref(params), C.byref(pw) if pw is not None else None, device,
                                   int(max_points_total), int(max_scans), C.byref(self.h))
        if rc != 0:
            self.h = C.c_void_p()
            raise ScvodError(f"scvod_create failed with status {rc} "
                             "(-2 = no HIP device: the SCV-OD path is GPU-only, there is no CPU fallback)")

    def close(self):
        if self.h:
            self.lib.scvod_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise ScvodError(f"status {rc}: {self.lib.scvod_last_error(self.h).decode()}")

    @staticmethod
    def _f32(a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        return a, a.ctypes.data_as(C.c_void_p)

    @staticmethod
    def _i32(a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        return a, a.ctypes.data_as(C.c_void_p)

    def process_scan(self, xyzi):
        a, p = self._f32(xyzi)
        r = ScanResult()
        self._chk(self.lib.scvod_process_scan(self.h, p, a.shape[0], C.byref(r)))
        return _unpack(r)

    def patchwork(self, xyzi):
        a, p = self._f32(xyzi)
        r = ScanResult()
        self._chk(self.lib.scvod_patchwork(self.h, p, a.shape[0], C.byref(r)))
        return _unpack(r)

    def bin_scan(self, xyzi, apply_filter=True, with_voxels=True):
        a, p = self._f32(xyzi)
        r = ScanResult()
        self._chk(self.lib.scvod_bin_scan(self.h, p, a.shape[0], int(apply_filter), int(with_voxels), C.byref(r)))
        return _unpack(r)

    def voxelize(self, apri):
        a = np.ascontiguousarray(apri)
        r = ScanResult()
        self._chk(self.lib.scvod_voxelize(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], C.byref(r)))
        self._n_scans, self._n_pts = 1, int(a.shape[0])  # (a batch of one scan: the batch_* calls may follow)
        return _unpack(r)

    def pose_delta(self, pose_pre, pose_next):
        a, pa = self._f32(pose_pre)
        b, pb = self._f32(pose_next)
        T = np.zeros(12, np.float32)
        self.lib.scvod_pose_delta(pa, pb, T.ctypes.data_as(C.c_void_p))
        return T

    def track_probe(self, xyzi, offsets, T, next_keys, next_labels):
        a, pa = self._f32(xyzi)
        o, po = self._i32(offsets)
        t, pt = self._f32(T)
        k, pk = self._i32(next_keys)
        n_c = o.shape[0] - 1
        n_pts = int(o[-1])
        if next_labels is not None:
            l, pl = self._i32(next_labels)
        else:
            l, pl = None, None
        hit = np.zeros(max(n_pts, 1), np.int32)
        uq = np.zeros(max(n_pts, 1), np.int32)
        ub = np.zeros(n_c + 1, np.int32)
        self._chk(self.lib.scvod_track_probe(self.h, pa, po, n_c, pt, pk, pl, k.shape[0], hit.ctypes.data_as(C.c_void_p),
                                             uq.ctypes.data_as(C.c_void_p), ub.ctypes.data_as(C.c_void_p)))
        return hit[:n_pts], uq[:ub[-1]], ub

    # ---- device-resident batch API (torch tensors) ----
    def batch_process(self, d_xyzi, scan_offsets, stream=None, sync=True):
        off, po = self._i32(scan_offsets)
        self._n_scans = off.shape[0] - 1
        self._n_pts = int(off[-1])
        ptr = C.c_void_p(d_xyzi.data_ptr())
        self._chk(self.lib.scvod_batch_process(self.h, ptr, po, self._n_scans, C.c_void_p(stream or 0), int(sync)))

    def batch_counts(self):
        out = np.zeros((self._n_scans, 8), np.int32)
        self._chk(self.lib.scvod_batch_counts(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def batch_fetch(self, s):
        r = ScanResult()
        self._chk(self.lib.scvod_batch_fetch(self.h, int(s), C.byref(r)))
        return _unpack(r)

    def batch_cluster(self, stream=None, sync=True):
        self._chk(self.lib.scvod_batch_cluster(self.h, C.c_void_p(stream or 0), int(sync)))

    def batch_fetch_clusters(self, s, cap):
        out = np.zeros(max(cap, 1), np.int32)
        n = self.lib.scvod_batch_fetch_clusters(self.h, int(s), out.ctypes.data_as(C.c_void_p), int(cap))
        if n < 0:
            self._chk(n)
        return out[:n]

    def batch_cluster_types(self, stream=None, sync=True):
        self._chk(self.lib.scvod_batch_cluster_types(self.h, C.c_void_p(stream or 0), int(sync)))

    def batch_fetch_cluster_types(self, s, cap, car_label=2, other_label=1):
        out = np.zeros(max(cap, 1), np.int32)
        n = self.lib.scvod_batch_fetch_cluster_types(self.h, int(s), car_label, other_label, out.ctypes.data_as(C.c_void_p), int(cap))
        if n < 0:
            self._chk(n)
        return out[:n]

    def cluster(self, apri):
        a = np.ascontiguousarray(apri)
        out = np.zeros(max(a.shape[0], 1), np.int32)
        self._chk(self.lib.scvod_cluster(self.h, a.ctypes.data_as(C.c_void_p), a.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out[:a.shape[0]]

    def batch_track(self, T, next_scan=None, ext_tables=None, stream=None, sync=True):
        """T [n_scans, 12] (row s: delta of scan s to its successor); next_scan [n_scans] or None (s + 1);
        ext_tables: list of torch device tensors written by batch_export_table on another shard."""
        t, pt = self._f32(T)
        assert t.size == 12 * self._n_scans, "one 3x4 transform per scan"
        pn = None
        if next_scan is not None:
            nx, pn = self._i32(next_scan)
            assert nx.shape[0] == self._n_scans
        n_ext = len(ext_tables) if ext_tables else 0
        ptrs = (C.c_void_p * max(n_ext, 1))(*[C.c_void_p(e.data_ptr()) for e in (ext_tables or [])])
        self._ext_keep = ext_tables  # the device buffers must outlive the asynchronous launch
        self._chk(self.lib.scvod_batch_track(self.h, pt, pn, ptrs if n_ext else None, n_ext, C.c_void_p(stream or 0), int(sync)))

    # ---- one sequence over several shards (include/scvod.h: scvod_set_track_owned ...) ----
    def set_track_owned(self, first_owned_scan):
        self._chk(self.lib.scvod_set_track_owned(self.h, int(first_owned_scan)))

    def set_track_halo(self, is_halo):
        m = np.ascontiguousarray(is_halo, np.uint8)
        self._chk(self.lib.scvod_set_track_halo(self.h, m.ctypes.data_as(C.c_void_p), len(m)))

    def batch_track_chains(self):
        """first scan of every chain of the last batch_track"""
        out = np.zeros(max(self._n_scans, 1), np.int32)
        n = self.lib.scvod_batch_track_chains(self.h, out.ctypes.data_as(C.c_void_p), len(out))
        if n < 0:
            self._chk(n)
        return out[:n].copy()

    def chain_export_state(self, chain, which, stream=None):
        """the state chain `chain` ended in (which=1) / assumed at its first own step (which=0): a torch uint8 device tensor"""
        import torch
        nb = int(self.lib.scvod_chain_state_bytes(self.h))
        buf = torch.zeros(nb, dtype=torch.uint8, device=f"cuda:{self.device}")
        self._chk(self.lib.scvod_chain_export_state(self.h, int(chain), int(which), C.c_void_p(buf.data_ptr()), nb, C.c_void_p(stream or 0)))
        torch.cuda.synchronize(self.device)
        hdr = buf[:16].view(torch.int32).cpu().numpy()
        used = 16 + 32 * int(hdr[0]) + ((4 * int(hdr[2]) + 15) // 16) * 16 + 16 * int(hdr[1])
        return buf[:max(used, 16)].clone()

    def chain_export_states(self, chains, which, stream=None):
        """chain_export_state for several chains: the export kernels back to back, ONE synchronisation, one copy of the headers"""
        import torch
        chains = [int(c) for c in chains]
        if not chains:
            return []
        nb = int(self.lib.scvod_chain_state_bytes(self.h))
        big = torch.empty((len(chains), nb), dtype=torch.uint8, device=f"cuda:{self.device}")
        for k, c in enumerate(chains):
            self._chk(self.lib.scvod_chain_export_state(self.h, c, int(which), C.c_void_p(big[k].data_ptr()), nb, C.c_void_p(stream or 0)))
        hdr = big[:, :16].contiguous().view(torch.int32).cpu().numpy().reshape(len(chains), 4)  # (synchronises)
        out = []
        for k in range(len(chains)):
            used = 16 + 32 * int(hdr[k, 0]) + ((4 * int(hdr[k, 2]) + 15) // 16) * 16 + 16 * int(hdr[k, 1])
            out.append(big[k, :max(used, 16)])
        return out

    def batch_track_resume(self, states, stream=None):
        """states[k]: the record the shard before this one exported (which=1) for chain k, or None"""
        self._resume_keep = states
        ptrs = (C.c_void_p * max(len(states), 1))(*[C.c_void_p(t.data_ptr() if t is not None else 0) for t in states])
        self._chk(self.lib.scvod_batch_track_resume(self.h, ptrs, len(states), C.c_void_p(stream or 0), 1))

    def batch_track_compare(self, states, stream=None):
        """how many chains would be walked again if `states` (as for batch_track_resume) were resumed from; changes nothing"""
        self._resume_keep = states
        ptrs = (C.c_void_p * max(len(states), 1))(*[C.c_void_p(t.data_ptr() if t is not None else 0) for t in states])
        out = C.c_int32(0)
        self._chk(self.lib.scvod_batch_track_compare(self.h, ptrs, len(states), C.byref(out), C.c_void_p(stream or 0)))
        return int(out.value)

    def chain_export_state_into(self, chain, which, buf, stream=None):
        """the record of chain_export_state written into `buf` (a torch uint8 device tensor of fixed size) without a word read on the
        host: a state that needs more room leaves header word 3 = 2 (compare_device then counts the chain as differing)"""
        self._chk(self.lib.scvod_chain_export_state(self.h, int(chain), int(which), C.c_void_p(buf.data_ptr()), int(buf.numel()), C.c_void_p(stream or 0)))

    def batch_track_compare_device(self, states, d_differ, stream=None):
        """batch_track_compare with the verdict ADDED to d_differ (a torch int32 device tensor the caller cleared): asynchronous"""
        self._resume_keep = states
        ptrs = (C.c_void_p * max(len(states), 1))(*[C.c_void_p(t.data_ptr() if t is not None else 0) for t in states])
        self._chk(self.lib.scvod_batch_track_compare_device(self.h, ptrs, len(states), C.c_void_p(d_differ.data_ptr()), C.c_void_p(stream or 0)))

    def batch_fetch_track(self, s):
        r = TrackResult()
        self._chk(self.lib.scvod_batch_fetch_track(self.h, int(s), C.byref(r)))

        def arr(ptr, n, dt):
            if n == 0 or not ptr:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32 if dt == np.int32 else C.c_uint8)), shape=(n,)).copy()
        ncl = r.n_clusters
        pb = arr(r.pair_begin, ncl + 1, np.int32)
        npair = int(pb[-1]) if ncl else 0
        return dict(n_apri=r.n_apri, n_clusters=ncl, n_car_points=r.n_car_points, n_dynamic_clusters=r.n_dynamic_clusters,
                    n_dynamic_points=r.n_dynamic_points, cluster_root=arr(r.cluster_root, ncl, np.int32),
                    cluster_size=arr(r.cluster_size, ncl, np.int32), cluster_state=arr(r.cluster_state, ncl, np.int32),
                    n_unique=arr(r.n_unique, ncl, np.int32), pair_begin=pb, pair_label=arr(r.pair_label, npair, np.int32),
                    pair_count=arr(r.pair_count, npair, np.int32), pt_dyn=arr(r.pt_dyn, r.n_apri, np.uint8))

    def set_track_mode(self, chain=True, segment_steps=0, warmup_steps=-1, generic_step=False):
        """chain=True: the reference's sequential tracking chain (default); False: first-order decisions.
        segment_steps 0: chosen per job; warmup_steps -1: keep the current value."""
        self._chk(self.lib.scvod_set_track_mode(self.h, (3 if generic_step else 1) if chain else 0, int(segment_steps), int(warmup_steps)))

    def set_cluster_exact(self, on=True):
        """True / 1 (default of a context since round 6): the components the local rule does not settle are clustered again in visiting
        order whatever their size (k_cc_exact, passes shared with helper blocks); 0: only while they have <= 4096 nodes together (larger
        ones keep "everything found is joined" and are counted: the default of rounds 3-5); 2: exact without the rule; 3: like 1, every
        scan's workgroup on its own"""
        self._chk(self.lib.scvod_set_cluster_exact(self.h, int(on)))

    def batch_cluster_stats(self):
        out = np.zeros(4, np.int32)
        self._chk(self.lib.scvod_batch_cluster_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        r2 = np.zeros(2, np.int32)
        self._chk(self.lib.scvod_batch_cluster_rule_stats(self.h, r2.ctypes.data_as(C.c_void_p)))
        h2 = np.zeros(2, np.int32)
        self._chk(self.lib.scvod_batch_cluster_help_stats(self.h, h2.ctypes.data_as(C.c_void_p)))
        return dict(scans_approximated=int(out[0]), nodes_concerned=int(out[1]), exact=bool(out[2]), scans_on_hbm_forest=int(out[3]),
                    runs_settled_by_rule=int(r2[0]), runs_clustered_again=int(r2[1]), scans_that_shared_their_rounds=int(h2[0]), chunks_taken_by_helpers=int(h2[1]))

    def set_intensity_merge(self, iterations=3, search_c=2, diff=2.0, cov=1.0):
        """SSC::refineClusterByIntensity (ssc.cpp:571-635) after the clustering; iterations = 0 turns it off (the default).  The
        defaults are the values of both shipped YAML files"""
        self._chk(self.lib.scvod_set_intensity_merge(self.h, int(iterations), int(search_c), float(diff), float(cov)))

    def set_voxel_descriptors(self, mode=0):
        """When a batch's vox_av / vox_cov are computed: 0 (the default) at their first request -- a batch_fetch, or the clustering of
        a ctx with the intensity merge on -- by a kernel of their own, 1 inside the voxel stage of every batch.  Same bits either way;
        takes effect with the next batch.  The per-scan calls (process_scan, bin_scan, voxelize) always compute them at once"""
        self._chk(self.lib.scvod_set_voxel_descriptors(self.h, int(mode)))

    def batch_cluster_merge_stats(self):
        out = np.zeros(4, np.int32)
        self._chk(self.lib.scvod_batch_cluster_merge_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return dict(clusters_before=int(out[0]), fusions=int(out[1]), clusters_after=int(out[2]), scans_fused=int(out[3]))

    def set_region_growing(self, on=True, k=10, min_segment=20, smoothness_deg=10.0, curvature_threshold=1.2, plane_fraction=0.2):
        """SSC::recognize's region growing (ssc.cpp:797-860) in scvod_batch_cluster_types: building / tree of the clusters above
        car_square.  The defaults are the reference's values; off until called"""
        self._chk(self.lib.scvod_set_region_growing(self.h, 1 if on else 0, int(k), int(min_segment), float(smoothness_deg),
                                                    float(curvature_threshold), float(plane_fraction)))

    def batch_fetch_cluster_classes(self, s, cap, car_label=2, building_label=0, tree_label=1):
        """per apri point: -1 erased, car / building / tree label (utility.h's building 0, tree 1, car 2 by default)"""
        out = np.zeros(max(cap, 1), np.int32)
        n = self.lib.scvod_batch_fetch_cluster_classes(self.h, int(s), int(car_label), int(building_label), int(tree_label),
                                                       out.ctypes.data_as(C.c_void_p), int(cap))
        if n < 0:
            self._chk(n)
        return out[:n]

    def batch_fetch_region_growing(self, s, cap):
        """(normal_curv [n, 4] float32, NaN off the candidates; segment [n] int32: apri index of the segment's seed or -1)"""
        nc = np.zeros((max(cap, 1), 4), np.float32)
        seg = np.zeros(max(cap, 1), np.int32)
        n = self.lib.scvod_batch_fetch_region_growing(self.h, int(s), nc.ctypes.data_as(C.c_void_p), seg.ctypes.data_as(C.c_void_p), int(cap))
        if n < 0:
            self._chk(n)
        return nc[:n], seg[:n]

    def batch_region_growing_stats(self):
        out = np.zeros(8, np.int32)
        self._chk(self.lib.scvod_batch_region_growing_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return dict(candidate_clusters=int(out[0]), building_clusters=int(out[1]), candidate_points=int(out[2]), kept_edges=int(out[3]),
                    max_rounds=int(out[4]), hbm_clusters=int(out[5]), tail_points=int(out[6]))

    def set_intensity_calibration(self, on=True, search_num=10, max_intensity=200.0):
        """SSC::intensityCalibrationByCurvature (ssc.cpp:98-153) between Patchwork and the voxel stage of every later batch: the
        intensity of every non-ground point divided by the cosine of its incidence angle (normal from its search_num nearest points,
        3..16).  The defaults are the reference's; off until called"""
        self._chk(self.lib.scvod_set_intensity_calibration(self.h, 1 if on else 0, int(search_num), float(max_intensity)))

    def batch_fetch_intensity_calibration(self, s, cap):
        """(normal_curv [n, 4] float32, calibrated intensity [n] float32) per non-ground point of scan s, in nonground_idx order"""
        nc = np.zeros((max(cap, 1), 4), np.float32)
        inten = np.zeros(max(cap, 1), np.float32)
        n = self.lib.scvod_batch_fetch_intensity_calibration(self.h, int(s), nc.ctypes.data_as(C.c_void_p), inten.ctypes.data_as(C.c_void_p), int(cap))
        if n < 0:
            self._chk(n)
        return nc[:n], inten[:n]

    def batch_intensity_calibration_stats(self):
        out = np.zeros(8, np.int32)
        self._chk(self.lib.scvod_batch_intensity_calibration_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return dict(points=int(out[0]), clamped_before=int(out[1]), cos_floored=int(out[2]), capped_after=int(out[3]), nan_normals=int(out[4]),
                    fallback_queries=int(out[5]), max_ring=int(out[6]))

    def batch_intensity_calibration_candidates(self):
        out = np.zeros(1, np.int64)
        self._chk(self.lib.scvod_batch_intensity_calibration_candidates(self.h, out.ctypes.data_as(C.c_void_p)))
        return int(out[0])

    def set_max_name_literal(self, literal=True):
        """ssc.cpp:354 keeps the LAST USED running number in Frame::max_name; False = fresh numbers (rounds 1-3)"""
        self._chk(self.lib.scvod_set_max_name_literal(self.h, 1 if literal else 0))

    def batch_cluster_last_name(self, n_scans):
        """per scan {name of the cluster that still carries Frame::max_name or -1, voxel slot, status, events}, and the batch's counters"""
        out = np.zeros((max(n_scans, 1), 4), np.int32)
        st = np.zeros(4, np.int32)
        rc = self.lib.scvod_batch_cluster_last_name(self.h, out.ctypes.data_as(C.c_void_p), n_scans, st.ctypes.data_as(C.c_void_p))
        if rc < 0:
            self._chk(rc)
        return out[:n_scans], dict(unknown_too_large=int(st[0]), unknown_irregular=int(st[1]))

    def set_chain_capacity(self, pool_points):
        self._chk(self.lib.scvod_set_chain_capacity(self.h, int(pool_points)))

    def batch_track_stats(self):
        out = np.zeros(8, np.int32)
        self._chk(self.lib.scvod_batch_track_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return dict(chain=bool(out[0]), segments=int(out[1]), verified=int(out[2]), rewalked=int(out[3]), error_bits=int(out[4]),
                    segment_steps=int(out[5]), warmup_steps=int(out[6]), max_name_undetermined=int(out[7]))

    def batch_track_tables(self, stream=None):
        self._chk(self.lib.scvod_batch_track_tables(self.h, C.c_void_p(stream or 0)))

    def batch_export_table(self, s, d_out, stream=None):
        """d_out: torch int32 device tensor [cap_records, 4]"""
        self._chk(self.lib.scvod_batch_export_table(self.h, int(s), C.c_void_p(d_out.data_ptr()), int(d_out.shape[0]),
                                                    C.c_void_p(stream or 0)))

    # ---- the result handed on (include/scvod.h: scvod_batch_point_labels ...) ----
    def batch_point_labels(self, d_labels=None, flags=0, stream=None):
        """one PT_* byte per INPUT point of the last batch into d_labels (a torch uint8 device tensor of at least the batch's point
        count; allocated when None).  Asynchronous on `stream`; flags 0 or MAP_IGNORE_DYNAMIC"""
        if d_labels is None:
            import torch
            d_labels = torch.empty(max(self._n_pts, 1), dtype=torch.uint8, device=f"cuda:{self.device}")
        self._chk(self.lib.scvod_batch_point_labels(self.h, C.c_void_p(d_labels.data_ptr()), int(d_labels.numel()), int(flags),
                                                    C.c_void_p(stream or 0)))
        return d_labels

    def batch_point_classes(self, d_classes=None, flags=0, stream=None):
        """batch_point_labels with the region growing's split in the byte: PT_STATIC_BUILDING where a PT_STATIC_OTHER point's cluster
        is a building.  Same arguments, same state rules"""
        if d_classes is None:
            import torch
            d_classes = torch.empty(max(self._n_pts, 1), dtype=torch.uint8, device=f"cuda:{self.device}")
        self._chk(self.lib.scvod_batch_point_classes(self.h, C.c_void_p(d_classes.data_ptr()), int(d_classes.numel()), int(flags),
                                                     C.c_void_p(stream or 0)))
        return d_classes

    def batch_export_points(self, d_out_offsets, d_xyzi_out=None, flags=0, poses=None, d_payload_in=None, d_payload_out=None,
                            d_src_out=None, stream=None):
        """the kept points of the last batch, compacted in input order, into d_xyzi_out (torch float32 device tensor [cap, 4]; None:
        count only); d_out_offsets: torch int32 device tensor [n_scans + 1]; d_src_out int32 [cap], d_payload_in uint32-sized words
        per input point, d_payload_out the same per exported point (int32 tensors do).  poses None: sensor frame, else [n_scans, 6]
        (copied before the call returns).  Asynchronous on `stream`: batch_export_stats() tells how many points there were"""
        assert d_out_offsets.numel() >= self._n_scans + 1
        cap = 0
        if d_xyzi_out is not None:
            assert d_xyzi_out.is_contiguous() and d_xyzi_out.numel() % 4 == 0
            cap = d_xyzi_out.numel() // 4
            for t in (d_src_out, d_payload_out):
                assert t is None or t.numel() >= cap
        pp = None
        if poses is not None:
            p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
            assert p.shape[0] == self._n_scans
            pp = p.ctypes.data_as(C.c_void_p)

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        self._chk(self.lib.scvod_batch_export_points(self.h, int(flags), pp, ptr(d_payload_in), ptr(d_xyzi_out), ptr(d_payload_out),
                                                     ptr(d_src_out), int(cap), ptr(d_out_offsets), C.c_void_p(stream or 0)))

    def batch_export_stats(self):
        """{written, kept, overflow} of the last batch_export_points; synchronises its stream; raises when that export overflowed"""
        out = np.zeros(4, np.int64)
        self._chk(self.lib.scvod_batch_export_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return dict(written=int(out[0]), kept=int(out[1]), overflow=bool(out[2]))

    # ---- the clusters as an object table (include/scvod.h: scvod_batch_objects) ----
    def batch_objects(self, d_obj_offsets, d_objects=None, flags=0, d_member_src=None, d_point_object=None, stream=None):
        """the clusters of the last batch that survived the box refine as OBJECT_DTYPE records into d_objects (a contiguous torch
        device tensor of 64-byte rows, e.g. uint8 [cap, 64]; None: no records); d_obj_offsets: torch int32 device tensor
        [n_scans + 1]; d_member_src int32 [cap_members]: the input index of every member point, grouped by object; d_point_object
        int32 [batch points]: the object of every input point, -1 for none.  flags 0 or OBJ_NO_TRACK.  Asynchronous on `stream`:
        batch_objects_stats() tells how many objects and member points there were"""
        assert d_obj_offsets.numel() >= self._n_scans + 1
        cap = 0
        if d_objects is not None:
            nbytes = d_objects.numel() * d_objects.element_size()
            assert d_objects.is_contiguous() and nbytes % OBJECT_DTYPE.itemsize == 0
            cap = nbytes // OBJECT_DTYPE.itemsize
        assert d_point_object is None or d_point_object.numel() >= self._n_pts

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        self._chk(self.lib.scvod_batch_objects(self.h, int(flags), ptr(d_objects), int(cap), ptr(d_obj_offsets), ptr(d_member_src),
                                               int(d_member_src.numel()) if d_member_src is not None else 0, ptr(d_point_object),
                                               C.c_void_p(stream or 0)))

    def batch_objects_stats(self):
        """{written, objects, members, overflow} of the last batch_objects; synchronises its stream; raises when that call overflowed"""
        out = np.zeros(4, np.int64)
        self._chk(self.lib.scvod_batch_objects_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return dict(written=int(out[0]), objects=int(out[1]), members=int(out[2]), overflow=bool(out[3]))

    def batch_objects_scratch_bytes(self):
        """device scratch of the object table on this ctx (not part of arena_bytes)"""
        return int(self.lib.scvod_batch_objects_scratch_bytes(self.h))

    # ---- the eigenvalue descriptor of the table's objects (include/scvod.h: scvod_batch_object_shapes) ----
    def set_object_features(self, params=None, **kw):
        """the constants of the features: a FeatureParams, or the defaults with fields overridden by keyword"""
        p = params if params is not None else feature_params(**kw)
        self._chk(self.lib.scvod_set_object_features(self.h, C.byref(p)))

    def batch_object_shapes(self, d_shapes, stream=None):
        """one OBJECT_SHAPE_DTYPE record per object of the last batch_objects that asked for more than the counts, in table order,
        into d_shapes (a contiguous torch device tensor of 96-byte rows, e.g. uint8 [cap, 96]).  Asynchronous on `stream`"""
        nbytes = d_shapes.numel() * d_shapes.element_size()
        assert d_shapes.is_contiguous() and nbytes % OBJECT_SHAPE_DTYPE.itemsize == 0
        self._chk(self.lib.scvod_batch_object_shapes(self.h, C.c_void_p(d_shapes.data_ptr()), nbytes // OBJECT_SHAPE_DTYPE.itemsize,
                                                     C.c_void_p(stream or 0)))

    def batch_object_shapes_stats(self):
        """{written, objects, not_finite, overflow} of the last batch_object_shapes; synchronises its stream; raises after an overflow"""
        out = np.zeros(4, np.int64)
        self._chk(self.lib.scvod_batch_object_shapes_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return dict(written=int(out[0]), objects=int(out[1]), not_finite=int(out[2]), overflow=bool(out[3]))

    # ---- the ESF descriptor (include/scvod.h: scvod_esf_device, scvod_batch_object_esf) ----
    @staticmethod
    def _esf_buffers(d_records, d_sig640):
        nbytes = d_records.numel() * d_records.element_size()
        assert d_records.is_contiguous() and nbytes % OBJECT_ESF_DTYPE.itemsize == 0
        cap = nbytes // OBJECT_ESF_DTYPE.itemsize
        if d_sig640 is not None:
            assert d_sig640.is_contiguous() and d_sig640.element_size() == 4 and d_sig640.numel() >= cap * ESF_SIG
        return cap, C.c_void_p(d_sig640.data_ptr()) if d_sig640 is not None else None

    def esf_device(self, d_xyzi, d_begin, d_records, d_sig640=None, params=None, stream=None):
        """one OBJECT_ESF_DTYPE record per run [d_begin[o], d_begin[o + 1]) of d_xyzi (float32 [n, 4] and int32 [objects + 1] torch
        device tensors) into d_records (a contiguous device tensor of 64-byte rows) and, optionally, the normalised signatures
        into d_sig640 (float32 [cap, 640]).  params: an EsfParams (None: the defaults).  Asynchronous on `stream`"""
        assert d_xyzi.is_contiguous() and d_xyzi.element_size() == 4 and d_begin.is_contiguous() and d_begin.element_size() == 4
        cap, sig = self._esf_buffers(d_records, d_sig640)
        self._chk(self.lib.scvod_esf_device(self.h, C.c_void_p(d_xyzi.data_ptr()), C.c_void_p(d_begin.data_ptr()), d_begin.numel() - 1,
                                            C.byref(params) if params is not None else None, C.c_void_p(d_records.data_ptr()), sig, cap,
                                            C.c_void_p(stream or 0)))

    def batch_object_esf(self, d_records, d_sig640=None, params=None, stream=None):
        """the same for every object of the last batch_objects that asked for more than the counts, in table order; params.cls_mask
        selects by class.  Asynchronous on `stream`"""
        cap, sig = self._esf_buffers(d_records, d_sig640)
        self._chk(self.lib.scvod_batch_object_esf(self.h, C.byref(params) if params is not None else None, C.c_void_p(d_records.data_ptr()),
                                                  sig, cap, C.c_void_p(stream or 0)))

    def esf_stats(self):
        """{written, objects, flagged, overflow, valid_samples, masked, uncached} of the last ESF call; synchronises its stream;
        raises after an overflow"""
        out = np.zeros(8, np.int64)
        self._chk(self.lib.scvod_esf_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return dict(written=int(out[0]), objects=int(out[1]), flagged=int(out[2]), overflow=bool(out[3]), valid_samples=int(out[4]),
                    masked=int(out[5]), uncached=int(out[6]))

    def esf_scratch_bytes(self):
        """device scratch of the ESF stage on this ctx (not part of arena_bytes or any other stage's scratch)"""
        return int(self.lib.scvod_esf_scratch_bytes(self.h))

    # ---- the truth label of the table's objects (include/scvod.h: scvod_batch_object_truth) ----
    def batch_object_truth(self, d_gt_label, params=None, cap=None, stream=None):
        """one OBJECT_TRUTH_DTYPE record per object of the last batch_objects that asked for more than the counts, in table order:
        d_gt_label holds one 4-byte label per input point of the batch (torch device tensor), params an EvalParams (only its class
        list is read; None: the defaults).  Returns a torch uint8 device tensor [cap, 32] (cap None: the batch's points, which holds
        every table); the rows behind the records written are not initialised.  Asynchronous on `stream`:
        batch_object_truth_stats() tells how many records were written"""
        import torch
        assert d_gt_label.is_contiguous() and d_gt_label.element_size() == 4 and d_gt_label.numel() >= self._n_pts
        cap = int(self._n_pts if cap is None else cap)
        out = torch.empty((max(cap, 1), OBJECT_TRUTH_DTYPE.itemsize), dtype=torch.uint8, device=d_gt_label.device)
        self._chk(self.lib.scvod_batch_object_truth(self.h, C.c_void_p(d_gt_label.data_ptr()), C.byref(params) if params is not None else None,
                                                    C.c_void_p(out.data_ptr()), cap, C.c_void_p(stream or 0)))
        return out[:cap]

    def batch_object_truth_stats(self):
        """{written, objects, overflow, fallback_objects, moving_points, moving_members} of the last batch_object_truth; synchronises
        its stream; raises after an overflow"""
        out = np.zeros(8, np.int64)
        self._chk(self.lib.scvod_batch_object_truth_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return dict(written=int(out[0]), objects=int(out[1]), overflow=bool(out[2]), fallback_objects=int(out[3]), moving_points=int(out[4]),
                    moving_members=int(out[5]))

    def batch_object_truth_scratch_bytes(self):
        """device scratch of the stage on this ctx (not part of arena_bytes or batch_objects_scratch_bytes)"""
        return int(self.lib.scvod_batch_object_truth_scratch_bytes(self.h))

    def set_timing(self, on):
        self._chk(self.lib.scvod_set_timing(self.h, int(bool(on))))

    def timings(self, cap=64):
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = self.lib.scvod_batch_timings(self.h, names, ms, cap)
        return [(names[i].decode(), float(ms[i])) for i in range(max(n, 0))]

    def arena_bytes(self):
        return int(self.lib.scvod_arena_bytes(self.h))

    def chain_workspace_bytes(self):
        """the tracking chain's walker workspace of the last job (not part of arena_bytes)"""
        return int(self.lib.scvod_chain_workspace_bytes(self.h))

    def nn_search_device(self, d_map_xyz, d_query_xyz, radius, stream=None):
        """torch CUDA tensors [n, 3] float32 in, (idx int32, sqdist float32, within uint8) CUDA tensors out."""
        import torch
        nq = int(d_query_xyz.shape[0])
        idx = torch.empty(max(nq, 1), dtype=torch.int32, device=d_query_xyz.device)
        sq = torch.empty(max(nq, 1), dtype=torch.float32, device=d_query_xyz.device)
        w = torch.empty(max(nq, 1), dtype=torch.uint8, device=d_query_xyz.device)
        self._chk(self.lib.scvod_nn_search_device(self.h, C.c_void_p(d_map_xyz.data_ptr()), int(d_map_xyz.shape[0]),
                                                  C.c_void_p(d_query_xyz.data_ptr()), nq, float(radius), C.c_void_p(idx.data_ptr()),
                                                  C.c_void_p(sq.data_ptr()), C.c_void_p(w.data_ptr()),
                                                  C.c_void_p(stream) if stream else None))
        return idx[:nq], sq[:nq], w[:nq]

    # ---- refining scan poses against a cloud (include/scvod.h: scvod_register_device) ----
    def register_device(self, d_src_xyzi, scan_offsets, d_tgt_xyz, poses=None, labels=None, d_tgt_normals=None, params=None, stream=None):
        """torch CUDA tensors in: the source [n, 4] float32, the target [m, 3] float32 and (plane mode) its normals [m, 3]; labels uint8
        [n] or None.  (d_pose_out float64 [n_scans, 12], d_records uint8 [n_scans * 64]) on the device, stream-ordered;
        register_result brings them to the host"""
        off = np.ascontiguousarray(scan_offsets, np.int32)
        p = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p is None or p.shape[0] == len(off) - 1
        pose, rec = _register_outputs(len(off) - 1, self.device)
        n_tgt = int(d_tgt_xyz.shape[0])
        self._chk(self.lib.scvod_register_device(self.h, C.c_void_p(d_src_xyzi.data_ptr()), off.ctypes.data_as(C.c_void_p), len(off) - 1,
                                                 None if p is None else p.ctypes.data_as(C.c_void_p),
                                                 None if labels is None else C.c_void_p(labels.data_ptr()),
                                                 C.c_void_p(d_tgt_xyz.data_ptr()) if n_tgt else None,
                                                 None if d_tgt_normals is None else C.c_void_p(d_tgt_normals.data_ptr()), n_tgt,
                                                 C.byref(params) if params is not None else None, C.c_void_p(pose.data_ptr()),
                                                 C.c_void_p(rec.data_ptr()), C.c_void_p(stream) if stream else None))
        return pose, rec

    def register_stats(self):
        """REGISTER_STATS of the last register_device call on this ctx (synchronises its stream)"""
        o = (C.c_int64 * 8)()
        self._chk(self.lib.scvod_register_stats(self.h, o))
        return dict(zip(REGISTER_STATS, (int(v) for v in o)))

    def register_scratch_bytes(self):
        return int(self.lib.scvod_register_scratch_bytes(self.h))

    # ---- surface normals of a cloud (include/scvod.h: scvod_normals_device) ----
    def normals_device(self, d_cloud, d_query=None, params=None, seg_offsets=None, viewpoints=None, want=("curvature",), stream=None):
        """torch CUDA float32 tensors in: the cloud [m, 3 or 4] and the queries [n, 3 or 4] (None: the cloud itself).  seg_offsets
        [n_segments + 1] with viewpoints [n_segments, 3] orient the normals.  dict(normals float32 [n, 3] -- what register_device takes as
        d_tgt_normals -- and, as `want` names them, curvature float32 [n], count int32 [n], sums int64 [n, 10]) on the device,
        stream-ordered"""
        import torch
        assert d_cloud.is_contiguous() and d_cloud.dim() == 2 and d_cloud.dtype == torch.float32
        assert d_query is None or (d_query.is_contiguous() and d_query.dim() == 2 and d_query.dtype == torch.float32)
        m = int(d_cloud.shape[0])
        n = m if d_query is None else int(d_query.shape[0])
        dev = d_cloud.device
        out = dict(normals=torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev))
        if "curvature" in want:
            out["curvature"] = torch.empty((max(n, 1),), dtype=torch.float32, device=dev)
        if "count" in want:
            out["count"] = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
        if "sums" in want:
            out["sums"] = torch.empty((max(n, 1), 10), dtype=torch.int64, device=dev)
        seg = None if seg_offsets is None else np.ascontiguousarray(seg_offsets, np.int32)
        view = None if viewpoints is None else np.ascontiguousarray(viewpoints, np.float32).reshape(-1, 3)
        assert (seg is None) == (view is None) and (seg is None or len(view) == len(seg) - 1)

        def ptr(t):
            return None if t is None else C.c_void_p(t.data_ptr())

        # a query cloud of no rows has no storage, and a NULL d_query would mean the self form: one row that is never read stands in
        q_arg = d_query if d_query is None or n else torch.zeros((1, int(d_query.shape[1])), dtype=torch.float32, device=dev)
        self._chk(self.lib.scvod_normals_device(self.h, ptr(d_cloud) if m else None, int(d_cloud.shape[1]), m, ptr(q_arg),
                                                0 if d_query is None else int(d_query.shape[1]), n,
                                                None if seg is None else seg.ctypes.data_as(C.c_void_p),
                                                None if view is None else view.ctypes.data_as(C.c_void_p), 0 if seg is None else len(seg) - 1,
                                                C.byref(params) if params is not None else None, ptr(out["normals"]), ptr(out.get("curvature")),
                                                ptr(out.get("count")), ptr(out.get("sums")), C.c_void_p(stream) if stream else None))
        return {k: v[:n] for k, v in out.items()}

    def normals_stats(self):
        """NORMALS_STATS of the last normals call on this ctx, the map form included (synchronises its stream)"""
        o = (C.c_int64 * 8)()
        self._chk(self.lib.scvod_normals_stats(self.h, o))
        return dict(zip(NORMALS_STATS, (int(v) for v in o)))

    def normals_scratch_bytes(self):
        return int(self.lib.scvod_normals_scratch_bytes(self.h))

    def set_normals_variant(self, variant=0):
        """development switch: NORMALS_QUERY_ORDER or NORMALS_ENTRY_ORDER (0: the default arm), plus NORMALS_WAVE_BLOCKS"""
        self._chk(self.lib.scvod_set_normals_variant(self.h, int(variant)))

    # ---- evaluation against labelled truth on the device (include/scvod.h: scvod_evaluate_device ...) ----
    @staticmethod
    def _xyz(t):
        assert t.is_contiguous() and t.numel() % 3 == 0 and t.element_size() == 4
        return (C.c_void_p(t.data_ptr()) if t.numel() else None), t.numel() // 3

    def evaluate_device(self, d_gt_xyz, d_gt_label, d_est_xyz, d_est_label, params=None, d_point_result=None, stream=None):
        """ground truth against an estimate, both on the device: contiguous torch float32 [n, 3] clouds, labels as 4-byte words (int32
        tensors holding the uint32 bits do).  d_point_result: torch uint8 [n_gt] or None.  Asynchronous on `stream`: evaluate_stats()"""
        pg, n_gt = self._xyz(d_gt_xyz)
        pe, n_est = self._xyz(d_est_xyz)
        assert d_gt_label.numel() >= n_gt and d_est_label.numel() >= n_est and d_gt_label.element_size() == 4 == d_est_label.element_size()
        assert d_point_result is None or d_point_result.numel() >= n_gt
        self._chk(self.lib.scvod_evaluate_device(self.h, pg, C.c_void_p(d_gt_label.data_ptr()) if n_gt else None, n_gt, pe,
                                                 C.c_void_p(d_est_label.data_ptr()) if n_est else None, n_est,
                                                 C.byref(params) if params is not None else None,
                                                 C.c_void_p(d_point_result.data_ptr()) if d_point_result is not None else None,
                                                 C.c_void_p(stream or 0)))

    def batch_evaluate(self, d_gt_label, poses, flags=0, params=None, d_point_result=None, stream=None):
        """the ERASOR protocol of quality.compare for the last batch: every input point in the world frame (poses [n_scans, 6], copied
        before the call returns) with its label (4-byte words per input point) against the points batch_export_points would keep with
        the same flags.  Asynchronous on `stream`: evaluate_stats()"""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p.shape[0] == self._n_scans and d_gt_label.numel() >= self._n_pts and d_gt_label.element_size() == 4
        assert d_point_result is None or d_point_result.numel() >= self._n_pts
        self._chk(self.lib.scvod_batch_evaluate(self.h, C.c_void_p(d_gt_label.data_ptr()), p.ctypes.data_as(C.c_void_p), int(flags),
                                                C.byref(params) if params is not None else None,
                                                C.c_void_p(d_point_result.data_ptr()) if d_point_result is not None else None,
                                                C.c_void_p(stream or 0)))

    def evaluate_stats(self):
        """the dict of metric.preservation_rejection for the last evaluate_device / batch_evaluate; synchronises its stream"""
        r = EvalResult()
        self._chk(self.lib.scvod_evaluate_stats(self.h, C.byref(r)))
        return _eval_dict(r)

    def evaluate_scratch_bytes(self):
        """device scratch of the evaluation on this ctx (not part of arena_bytes)"""
        return int(self.lib.scvod_evaluate_scratch_bytes(self.h))

    # ---- class scores against labelled truth on the device (include/scvod.h: scvod_score_classes_device ...) ----
    def score_classes_device(self, d_gt_xyz, d_gt_label, d_est_xyz, d_est_class, params=None, d_point_result=None, stream=None):
        """labelled truth against an estimate with one PT_* byte per point (batch_point_classes' bytes), both on the device: contiguous
        torch float32 [n, 3] clouds, labels as 4-byte words, classes as uint8.  d_point_result: torch uint8 [n_gt] or None.
        Asynchronous on `stream`: score_classes_stats()"""
        pg, n_gt = self._xyz(d_gt_xyz)
        pe, n_est = self._xyz(d_est_xyz)
        assert d_gt_label.numel() >= n_gt and d_gt_label.element_size() == 4
        assert d_est_class.numel() >= n_est and d_est_class.element_size() == 1
        assert d_point_result is None or d_point_result.numel() >= n_gt
        self._chk(self.lib.scvod_score_classes_device(self.h, pg, C.c_void_p(d_gt_label.data_ptr()) if n_gt else None, n_gt, pe,
                                                      C.c_void_p(d_est_class.data_ptr()) if n_est else None, n_est,
                                                      C.byref(params) if params is not None else None,
                                                      C.c_void_p(d_point_result.data_ptr()) if d_point_result is not None else None,
                                                      C.c_void_p(stream or 0)))

    def batch_score_classes(self, d_gt_label, poses, flags=0, params=None, d_point_result=None, stream=None):
        """batch_evaluate's protocol for the class scores: every input point of the last batch in the world frame with its label against
        the points batch_export_points would keep with the same flags, each carrying its byte of batch_point_classes.  Asynchronous on
        `stream`: score_classes_stats()"""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p.shape[0] == self._n_scans and d_gt_label.numel() >= self._n_pts and d_gt_label.element_size() == 4
        assert d_point_result is None or d_point_result.numel() >= self._n_pts
        self._chk(self.lib.scvod_batch_score_classes(self.h, C.c_void_p(d_gt_label.data_ptr()), p.ctypes.data_as(C.c_void_p), int(flags),
                                                     C.byref(params) if params is not None else None,
                                                     C.c_void_p(d_point_result.data_ptr()) if d_point_result is not None else None,
                                                     C.c_void_p(stream or 0)))

    def score_classes_stats(self):
        """conf, pd_far, num, P, rate_P, rate_N of the last score_classes_device / batch_score_classes; synchronises its stream"""
        r = ClassResult()
        self._chk(self.lib.scvod_score_classes_stats(self.h, C.byref(r)))
        return _class_dict(r)

    def score_classes_pass2_queries(self):
        """truth points of the last scoring call that needed the ring search (a cost measure); synchronises its stream"""
        n = int(self.lib.scvod_score_classes_pass2_queries(self.h))
        if n < 0:
            self._chk(n)
        return n

    def score_classes_scratch_bytes(self):
        """device scratch of the class scores on this ctx (not part of arena_bytes or evaluate_scratch_bytes)"""
        return int(self.lib.scvod_score_classes_scratch_bytes(self.h))

    # ---- object scores from a device instance table (include/scvod.h: scvod_score_instances_device ...) ----
    def score_instances_device(self, d_key, d_point_result, cap_instances=65536, d_instances=None, stream=None, count_only=False):
        """the points grouped by their 4-byte key and counted per group: d_key 4-byte words and d_point_result uint8 (the bytes of
        evaluate_device / batch_evaluate), contiguous CUDA tensors of one length.  d_instances: a CUDA tensor of at least
        cap_instances * 32 bytes, allocated when None; count_only=True passes none at all.  Returns (d_instances, d_n): the records as
        bytes (view them with INSTANCE_DTYPE after the download) and the int64 [1] record count, both on the device.  Asynchronous on
        `stream`: score_instances_stats()"""
        import torch
        n = int(d_key.numel())
        assert d_key.is_contiguous() and d_key.element_size() == 4
        assert d_point_result.is_contiguous() and d_point_result.element_size() == 1 and d_point_result.numel() >= n
        cap = int(cap_instances)
        if count_only:
            d_instances = None
        elif d_instances is None:
            d_instances = torch.empty(max(cap, 1) * INSTANCE_DTYPE.itemsize, dtype=torch.uint8, device=d_key.device)
        else:
            assert d_instances.is_contiguous() and d_instances.numel() * d_instances.element_size() >= cap * INSTANCE_DTYPE.itemsize
        d_n = torch.empty(1, dtype=torch.int64, device=d_key.device)
        self._chk(self.lib.scvod_score_instances_device(self.h, C.c_void_p(d_key.data_ptr()) if n else None,
                                                        C.c_void_p(d_point_result.data_ptr()) if n else None, n,
                                                        C.c_void_p(d_instances.data_ptr()) if d_instances is not None else None, cap,
                                                        C.c_void_p(d_n.data_ptr()), C.c_void_p(stream or 0)))
        return d_instances, d_n

    def score_instances_stats(self):
        """{written, distinct, overflow, spilled_tiles} of the last score_instances_device; synchronises its stream; raises after an
        overflow"""
        out = np.zeros(4, np.int64)
        self._chk(self.lib.scvod_score_instances_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return dict(zip(INSTANCE_STATS, (int(v) for v in out)))

    def score_instances_scratch_bytes(self):
        """device scratch of the object scores on this ctx (not part of arena_bytes or the other stages' scratch)"""
        return int(self.lib.scvod_score_instances_scratch_bytes(self.h))

    def batch_score_instances(self, d_gt_label, poses, flags=0, eval_params=None, cap_instances=65536, stream=None):
        """batch_evaluate with a result byte per input point, then score_instances_device keyed by d_gt_label on the same stream, no
        host synchronisation in between.  One read at the end returns the table as a numpy array of INSTANCE_DTYPE; evaluate_stats()
        holds the batch's counters"""
        import torch
        n = self._n_pts
        res = torch.empty(max(n, 1), dtype=torch.uint8, device=d_gt_label.device)
        self.batch_evaluate(d_gt_label, poses, flags=flags, params=eval_params, d_point_result=res, stream=stream)
        # (stream None: the library runs the scoring on the evaluation's stream)
        d_inst, _ = self.score_instances_device(d_gt_label.reshape(-1)[:n], res[:n], cap_instances=cap_instances, stream=stream)
        written = self.score_instances_stats()["written"]
        return d_inst[:written * INSTANCE_DTYPE.itemsize].cpu().numpy().view(INSTANCE_DTYPE).copy()

    # ---- a map split by nearest-neighbour hits on the device (include/scvod.h: scvod_map_split_device ...) ----
    def map_split_device(self, d_base, d_query, params=None, d_base_label=None, d_mark=None, d_order=None, d_seg4=None, d_base_out=None,
                         d_payload_in=None, d_payload_out=None, d_nn_idx=None, d_nn_sqdist=None, stream=None):
        """every query point marks its nearest base point; the base cloud is handed out as HIT | MISS | GATED segments in base order.
        d_base / d_query: contiguous torch float32 [n, 3] or [n, 4] CUDA tensors (the strides of `params` are set from their shapes);
        d_base_label and the payloads 4-byte words per base point; d_mark uint8 [n_base], d_order int32 [n_base], d_seg4 int64 [4],
        d_base_out like d_base, d_nn_idx int32 / d_nn_sqdist float32 [n_query]; every output may be None.  Asynchronous on `stream`:
        map_split_stats()"""
        p = SplitParams()
        if params is not None:
            C.memmove(C.byref(p), C.byref(params), C.sizeof(p))
        else:
            self.lib.scvod_split_params_default(C.byref(p))
        for t, name in ((d_base, "base_stride"), (d_query, "query_stride")):
            assert t.is_contiguous() and t.element_size() == 4 and t.dim() == 2 and t.shape[1] in (3, 4)
            setattr(p, name, int(t.shape[1]))
        n_base, n_query = int(d_base.shape[0]), int(d_query.shape[0])
        for t, size in ((d_base_label, 4), (d_payload_in, 4), (d_payload_out, 4), (d_mark, 1), (d_order, 4)):
            assert t is None or (t.numel() >= n_base and t.element_size() == size and t.is_contiguous())
        for t in (d_nn_idx, d_nn_sqdist):
            assert t is None or (t.numel() >= n_query and t.element_size() == 4 and t.is_contiguous())
        assert d_seg4 is None or (d_seg4.numel() >= 4 and d_seg4.element_size() == 8)
        assert d_base_out is None or (d_base_out.numel() >= d_base.numel() and d_base_out.element_size() == 4 and d_base_out.is_contiguous())

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
        self._chk(self.lib.scvod_map_split_device(self.h, ptr(d_base), ptr(d_base_label), n_base, ptr(d_query), n_query, C.byref(p),
                                                  ptr(d_mark), ptr(d_order), ptr(d_seg4), ptr(d_base_out), ptr(d_payload_in),
                                                  ptr(d_payload_out), ptr(d_nn_idx), ptr(d_nn_sqdist), C.c_void_p(stream or 0)))

    def map_split_stats(self):
        """n_hit, n_miss, n_gated and the queries finished by the 27-cell, the ring and the exhaustive pass of the last
        map_split_device; synchronises its stream"""
        out = np.zeros(8, np.int64)
        self._chk(self.lib.scvod_map_split_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return dict(zip(SPLIT_STATS, (int(v) for v in out)))

    def map_split_scratch_bytes(self):
        """device scratch of the split on this ctx (not part of arena_bytes, evaluate_scratch_bytes or score_classes_scratch_bytes)"""
        return int(self.lib.scvod_map_split_scratch_bytes(self.h))

    def classify_map_device(self, d_orig_xyz, d_pred_static, d_static_xyz, d_dynamic_xyz, r15=0.15, r10=0.1, d_class=None, stream=None):
        """metric.classify_map_points on the device: contiguous torch float32 [n, 3] clouds, d_pred_static one byte per point of the
        original map (uint8 or bool), d_class torch uint8 [n] or None (counts only).  Asynchronous on `stream`: classify_map_stats()"""
        po, n = self._xyz(d_orig_xyz)
        ps, n_s = self._xyz(d_static_xyz)
        pd, n_d = self._xyz(d_dynamic_xyz)
        assert d_pred_static.numel() >= n and d_pred_static.element_size() == 1 and (d_class is None or d_class.numel() >= n)
        self._chk(self.lib.scvod_classify_map_device(self.h, po, C.c_void_p(d_pred_static.data_ptr()) if n else None, n, ps, n_s, pd, n_d,
                                                     float(r15), float(r10), C.c_void_p(d_class.data_ptr()) if d_class is not None else None,
                                                     C.c_void_p(stream or 0)))

    def classify_map_stats(self):
        """points per class {unmatched, tp_static, fn_static, tn_dynamic, fn_dynamic} of the last classify_map_device; synchronises"""
        out = np.zeros(5, np.int64)
        self._chk(self.lib.scvod_classify_map_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return dict(zip(("unmatched", "tp_static", "fn_static", "tn_dynamic", "fn_dynamic"), (int(v) for v in out)))

    # ---- scan stacking (include/scvod.h: scvod_batch_stack_scans) ----
    def batch_stack_scans(self, d_xyzi_in, offsets, poses, d_xyzi_out, window=3, interval=3, reference_bound=False, d_payload_in=None,
                          d_payload_out=None, d_src_out=None, stream=None):
        """every `window` consecutive scans (a group every `interval` scans) stacked into the frame of the group's middle scan: the
        middle scan first, bit for bit, then the others in ascending scan index, moved by pose_delta(pose_k, pose_mid).  d_xyzi_in /
        d_xyzi_out: torch float32 device tensors [*, 4]; offsets [n_in + 1] and poses [n_in, 6] host arrays (copied before the call
        returns); d_payload_* uint32-sized words per point (int32 tensors do), d_src_out int32 per output point.  Asynchronous on
        `stream`, no host synchronisation, the last batch stays valid.  Returns (out_offsets, mid) as stack_offsets does"""
        off = np.ascontiguousarray(offsets, np.int32)
        n_in = off.shape[0] - 1
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p.shape[0] == n_in
        out_offsets, mid = stack_offsets(off, window, interval, reference_bound)
        assert d_xyzi_out.numel() % 4 == 0
        cap = d_xyzi_out.numel() // 4
        for t in (d_src_out, d_payload_out):
            assert t is None or t.numel() >= min(cap, int(out_offsets[-1]))

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        self._chk(self.lib.scvod_batch_stack_scans(self.h, ptr(d_xyzi_in), off.ctypes.data_as(C.c_void_p), n_in,
                                                   p.ctypes.data_as(C.c_void_p), int(window), int(interval),
                                                   STACK_REFERENCE_BOUND if reference_bound else 0, ptr(d_payload_in), ptr(d_xyzi_out),
                                                   ptr(d_payload_out), ptr(d_src_out), int(cap), C.c_void_p(stream or 0)))
        return out_offsets, mid

    def stack_scans(self, xyzi, offsets, poses, window=3, interval=3, reference_bound=False):
        """the same for scans in host memory (upload, stack, download; synchronous).  Returns (stacked xyzi, out_offsets, mid)"""
        x, px = self._f32(xyzi)
        off = np.ascontiguousarray(offsets, np.int32)
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        out_offsets, mid = stack_offsets(off, window, interval, reference_bound)
        out = np.zeros((max(int(out_offsets[-1]), 1), 4), np.float32)
        self._chk(self.lib.scvod_stack_scans(self.h, px, off.ctypes.data_as(C.c_void_p), off.shape[0] - 1, p.ctypes.data_as(C.c_void_p),
                                             int(window), int(interval), STACK_REFERENCE_BOUND if reference_bound else 0,
                                             out.ctypes.data_as(C.c_void_p), int(out_offsets[-1])))
        return out[:int(out_offsets[-1])], out_offsets, mid

    def stack_scratch_bytes(self):
        """device scratch the stacking holds on this ctx (0 before the first batch_stack_scans)"""
        return int(self.lib.scvod_stack_scratch_bytes(self.h))

    # ---- seen-through points (include/scvod.h: scvod_visibility_device) ----
    def _visibility_outputs(self, n, n_scans, want):
        """the device tensors a vote writes, by name (VIS_OUTPUTS), and the four pointers in the C order"""
        import torch
        want = VIS_OUTPUTS if want is None else tuple(want)
        assert all(w in VIS_OUTPUTS for w in want), want
        _, S, A, _ = grid_dims(self.params)
        dev = torch.device("cuda", self.device)
        shape = {"votes": ((n,), torch.int32), "verdict": ((n,), torch.uint8), "images": ((n_scans, A, S), torch.float32),
                 "scan_counts": ((n_scans, 6), torch.int64)}
        out = {w: torch.empty(shape[w][0], dtype=shape[w][1], device=dev) for w in want}
        return out, [C.c_void_p(out[w].data_ptr()) if w in out else None for w in VIS_OUTPUTS]

    def visibility_device(self, d_xyzi, scan_offsets, poses=None, next_scan=None, params=None, d_query_mask=None,
                          want=("votes", "verdict"), stream=None):
        """scvod_visibility_device of the caller's cloud (torch float32 [n, 4] on the ctx's device): a dict of device tensors, one per
        name in `want` (VIS_OUTPUTS; None: all) -- votes int32 [n] (the bits of the uint32: bytes n_through, n_agree, n_occluded,
        n_outside + n_empty), verdict uint8 [n] (VIS_*), images float32 [n_scans, A, S], scan_counts int64 [n_scans, 6].  Rows are at
        the input index, so the offsets should start at 0.  d_query_mask: torch uint8 [n] or None (every point).  Stream-ordered."""
        off = np.ascontiguousarray(scan_offsets, np.int32)
        n_scans = len(off) - 1
        p = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p is None or p.shape[0] == n_scans
        nx = None if next_scan is None else np.ascontiguousarray(next_scan, np.int32)
        assert nx is None or nx.shape[0] == n_scans
        prm = params if params is not None else visibility_params_default()
        out, ptr = self._visibility_outputs(int(off[-1]) if len(off) else 0, n_scans, want)
        self._chk(self.lib.scvod_visibility_device(self.h, C.c_void_p(d_xyzi.data_ptr()), off.ctypes.data_as(C.c_void_p), n_scans,
                                                   None if p is None else p.ctypes.data_as(C.c_void_p),
                                                   None if nx is None else nx.ctypes.data_as(C.c_void_p),
                                                   None if d_query_mask is None else C.c_void_p(d_query_mask.data_ptr()), C.byref(prm),
                                                   *ptr, C.c_void_p(stream or 0)))
        return out

    def batch_visibility(self, poses, next_scan=None, params=None, flags=0, want=("votes", "verdict"), stream=None):
        """scvod_batch_visibility: the same for the input cloud of the last batch; queries are Patchwork's non-ground points, or every
        input point with flags=VIS_WITH_GROUND"""
        p = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p is None or p.shape[0] == self._n_scans
        nx = None if next_scan is None else np.ascontiguousarray(next_scan, np.int32)
        assert nx is None or nx.shape[0] == self._n_scans
        prm = params if params is not None else visibility_params_default()
        out, ptr = self._visibility_outputs(int(self._n_pts), self._n_scans, want)
        self._chk(self.lib.scvod_batch_visibility(self.h, None if p is None else p.ctypes.data_as(C.c_void_p),
                                                  None if nx is None else nx.ctypes.data_as(C.c_void_p), C.byref(prm), int(flags), *ptr,
                                                  C.c_void_p(stream or 0)))
        return out

    def visibility_stats(self):
        """{queries, seen_through, through, agree, occluded, outside_or_empty, pairs} of the last vote (synchronises its stream)"""
        o = (C.c_int64 * 8)()
        self._chk(self.lib.scvod_visibility_stats(self.h, o))
        return dict(zip(VIS_STATS, (int(v) for v in o[:7])))

    def visibility_scratch_bytes(self):
        """device scratch the vote holds on this ctx (0 before the first call)"""
        return int(self.lib.scvod_visibility_scratch_bytes(self.h))

    # ---- the objects of the table vote on the verdict (include/scvod.h: scvod_batch_object_visibility) ----
    def batch_object_visibility(self, d_verdict, d_votes=None, d_objects=None, params=None, cap=None, want=("records", "verdict"), in_place=False,
                                stream=None):
        """scvod_batch_object_visibility on the table the last batch_objects (with lists) left: d_verdict uint8 [points] and d_votes
        int32 [points] as batch_visibility wrote them, d_objects the table's OBJECT_DTYPE records as a contiguous device tensor (read
        with OBJVIS_WITH_TRACK only).  A dict of device tensors, one per name in `want` (OBJVIS_OUTPUTS): records uint8 [cap, 48] (view
        as OBJECT_VISIBILITY_DTYPE on the host; cap None: the batch's points, which holds every table; the rows behind the records
        written are not initialised), verdict uint8 [points] -- with in_place=True d_verdict itself, rewritten.  Stream-ordered;
        batch_object_visibility_stats() tells what happened"""
        import torch
        want = tuple(want)
        assert all(w in OBJVIS_OUTPUTS for w in want), want
        n = int(self._n_pts)
        assert d_verdict.dtype == torch.uint8 and d_verdict.is_contiguous() and d_verdict.numel() >= n
        assert d_votes is None or (d_votes.is_contiguous() and d_votes.element_size() == 4 and d_votes.numel() >= n)
        assert d_objects is None or d_objects.is_contiguous()
        out = {}
        cap = int(n if cap is None else cap)
        if "records" in want:
            out["records"] = torch.empty((max(cap, 1), OBJECT_VISIBILITY_DTYPE.itemsize), dtype=torch.uint8, device=d_verdict.device)[:cap]
        if "verdict" in want:
            out["verdict"] = d_verdict if in_place else torch.empty((max(n, 1),), dtype=torch.uint8, device=d_verdict.device)[:n]
        self._chk(self.lib.scvod_batch_object_visibility(
            self.h, C.c_void_p(d_verdict.data_ptr()), None if d_votes is None else C.c_void_p(d_votes.data_ptr()),
            None if d_objects is None else C.c_void_p(d_objects.data_ptr()), C.byref(params) if params is not None else None,
            C.c_void_p(out["records"].data_ptr()) if "records" in out else None, cap if "records" in out else 0,
            C.c_void_p(out["verdict"].data_ptr()) if "verdict" in out else None, C.c_void_p(stream or 0)))
        return out

    def batch_object_visibility_stats(self):
        """{objects, voted, forced, seen_through, moved_to_seen_through, moved_to_keep, written, overflow} of the last
        batch_object_visibility; synchronises its stream; raises after an overflow"""
        o = (C.c_int64 * 8)()
        self._chk(self.lib.scvod_batch_object_visibility_stats(self.h, o))
        return dict(zip(OBJVIS_STATS, (int(v) for v in o)))

    def batch_object_visibility_scratch_bytes(self):
        """device scratch of the stage on this ctx (not part of arena_bytes or batch_objects_scratch_bytes)"""
        return int(self.lib.scvod_batch_object_visibility_scratch_bytes(self.h))

    # ---- the objects of a table linked into tracks (include/scvod.h: scvod_object_tracks_device) ----
    @staticmethod
    def _tracks_outputs(dev, cap_links, cap_tracks, want, guard):
        """the output tensors of a tracks call: name -> uint8 / int32 device tensor with `guard` extra rows behind the capacity (filled
        with 0xA5 bytes, for tests), and the capacity-sized views"""
        import torch
        want = TRK_OUTPUTS if want is None else tuple(want)
        assert all(w in TRK_OUTPUTS for w in want), want
        rows = {"links": (cap_links, OBJECT_LINK_DTYPE.itemsize), "tracks": (cap_tracks, TRACK_DTYPE.itemsize),
                "track_objects": (cap_links, 4), "n_tracks": (1, 4)}
        full = {w: torch.full((rows[w][0] + guard + 1, rows[w][1]), 0xA5, dtype=torch.uint8, device=dev) for w in want}
        return full, {w: full[w][:rows[w][0]] for w in want}

    def object_tracks_device(self, d_objects, d_obj_offsets, n_scans, next_scan=None, poses=None, d_cand_begin=None, d_cand=None,
                             params=None, cap_links=None, cap_tracks=None, want=None, guard=0, stream=None, full=False):
        """scvod_object_tracks_device on the caller's table: d_objects a contiguous device tensor of 64-byte OBJECT_DTYPE rows,
        d_obj_offsets int32 [n_scans + 1] (device), next_scan / poses host arrays or None, d_cand_begin int32 [objects + 1] and d_cand
        int32 [pairs, 2] device tensors or None.  cap_links None: the rows of d_objects; cap_tracks None: cap_links.  Returns a dict of
        uint8 device tensors, one per name in `want` (TRK_OUTPUTS; None: all): links [cap_links, 32] (OBJECT_LINK_DTYPE), tracks
        [cap_tracks, 64] (TRACK_DTYPE), track_objects [cap_links, 4] (int32), n_tracks [1, 4] (int32); the rows behind what was written
        hold 0xA5 bytes.  full=True: (views, the tensors with their `guard` rows behind).  Stream-ordered"""
        nbytes = d_objects.numel() * d_objects.element_size()
        assert d_objects.is_contiguous() and nbytes % OBJECT_DTYPE.itemsize == 0
        cap_links = nbytes // OBJECT_DTYPE.itemsize if cap_links is None else int(cap_links)
        cap_tracks = cap_links if cap_tracks is None else int(cap_tracks)
        nx = None if next_scan is None else np.ascontiguousarray(next_scan, np.int32)
        p = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert (nx is None or nx.shape[0] == n_scans) and (p is None or p.shape[0] == n_scans)
        whole, out = self._tracks_outputs(d_objects.device, cap_links, cap_tracks, want, guard)

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        self._chk(self.lib.scvod_object_tracks_device(
            self.h, ptr(d_objects), ptr(d_obj_offsets), int(n_scans), None if nx is None else nx.ctypes.data_as(C.c_void_p),
            None if p is None else p.ctypes.data_as(C.c_void_p), ptr(d_cand_begin), ptr(d_cand),
            C.byref(params) if params is not None else None, ptr(whole.get("links")), cap_links, ptr(whole.get("tracks")), cap_tracks,
            ptr(whole.get("track_objects")), ptr(whole.get("n_tracks")), C.c_void_p(stream or 0)))
        return (out, whole) if full else out

    def batch_object_tracks(self, d_objects, poses=None, params=None, cap_links=None, cap_tracks=None, want=None, guard=0, stream=None,
                            full=False):
        """scvod_batch_object_tracks: the same on the table the last batch_objects (with lists, with tracking) left; d_objects are the
        records that call wrote; the successor table is the one the last batch_track was given.  Outputs as object_tracks_device"""
        nbytes = d_objects.numel() * d_objects.element_size()
        assert d_objects.is_contiguous() and nbytes % OBJECT_DTYPE.itemsize == 0
        cap_links = nbytes // OBJECT_DTYPE.itemsize if cap_links is None else int(cap_links)
        cap_tracks = cap_links if cap_tracks is None else int(cap_tracks)
        p = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p is None or p.shape[0] == self._n_scans
        whole, out = self._tracks_outputs(d_objects.device, cap_links, cap_tracks, want, guard)

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        self._chk(self.lib.scvod_batch_object_tracks(
            self.h, ptr(d_objects), None if p is None else p.ctypes.data_as(C.c_void_p), C.byref(params) if params is not None else None,
            ptr(whole.get("links")), cap_links, ptr(whole.get("tracks")), cap_tracks, ptr(whole.get("track_objects")), ptr(whole.get("n_tracks")),
            C.c_void_p(stream or 0)))
        return (out, whole) if full else out

    def object_tracks_stats(self):
        """{objects, tracks, written, overlap_links, gate_links, refused, longest, overflow} of the last tracks call of either form;
        synchronises its stream; raises after an overflow"""
        o = (C.c_int64 * 8)()
        self._chk(self.lib.scvod_object_tracks_stats(self.h, o))
        return dict(zip(TRK_STATS, (int(v) for v in o)))

    def object_tracks_scratch_bytes(self):
        """device scratch of the stage on this ctx (not part of arena_bytes or batch_objects_scratch_bytes)"""
        return int(self.lib.scvod_object_tracks_scratch_bytes(self.h))

    # ---- the tracks of a table vote on the seen-through verdict (include/scvod.h: scvod_track_visibility_device) ----
    def track_visibility(self, d_objects, d_obj_offsets, n_scans, poses, trk, d_point_object, d_verdict, d_object_vis=None, params=None,
                         cap_objects=None, cap_tracks=None, cap_track_votes=None, cap_object_votes=None, want=None, in_place=False,
                         guard=0, stream=None, full=False):
        """scvod_track_visibility_device.  d_objects: a contiguous device tensor of 64-byte OBJECT_DTYPE rows; d_obj_offsets int32
        [n_scans + 1] (device); poses a host array [n_scans, 6] or None; trk: the dict object_tracks_device / batch_object_tracks
        returned (links, tracks, track_objects, n_tracks); d_point_object int32 [n_points] and d_verdict uint8 [n_points] device
        tensors, either may be None (no d_point_object: records only; no d_verdict: every byte UNTESTED; n_points is the length of the
        one that is given); d_object_vis the records of batch_object_visibility or None.  cap_objects None: the rows of d_objects;
        cap_tracks None: the rows of trk["tracks"]; cap_track_votes / cap_object_votes None: cap_tracks / cap_objects.  Returns a dict
        of uint8 device tensors, one per name in `want` (TRKVIS_OUTPUTS; None: all that the inputs allow): track_votes
        [cap_track_votes, 32] (TRACK_VOTE_DTYPE), object_votes [cap_object_votes, 16] (OBJECT_TRACK_VOTE_DTYPE), verdict [n_points]
        (in_place=True: d_verdict itself).  Record rows behind what was written hold 0xA5 bytes, and with guard > 0 every output has
        `guard` rows (verdict: 16 * guard bytes) of 0xA5 in front of it and behind it.  full=True: (views, the tensors with their guard
        rows).  Stream-ordered"""
        import torch
        nbytes = d_objects.numel() * d_objects.element_size()
        assert d_objects.is_contiguous() and nbytes % OBJECT_DTYPE.itemsize == 0
        cap_objects = nbytes // OBJECT_DTYPE.itemsize if cap_objects is None else int(cap_objects)
        cap_tracks = int(trk["tracks"].shape[0]) if cap_tracks is None else int(cap_tracks)
        cap_tv = cap_tracks if cap_track_votes is None else int(cap_track_votes)
        cap_ov = cap_objects if cap_object_votes is None else int(cap_object_votes)
        p = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p is None or p.shape[0] == n_scans
        n_points = int(d_point_object.numel()) if d_point_object is not None else (int(d_verdict.numel()) if d_verdict is not None else 0)
        assert d_verdict is None or (d_verdict.dtype == torch.uint8 and d_verdict.numel() == n_points)
        paint = d_point_object is not None
        want = tuple(w for w in TRKVIS_OUTPUTS if paint or w != "verdict") if want is None else tuple(want)
        assert all(w in TRKVIS_OUTPUTS for w in want) and (paint or "verdict" not in want) and not (in_place and d_verdict is None)
        dev = d_objects.device
        rows = {"track_votes": (cap_tv, TRACK_VOTE_DTYPE.itemsize), "object_votes": (cap_ov, OBJECT_TRACK_VOTE_DTYPE.itemsize)}
        whole, out = {}, {}
        for w in want:
            if w == "verdict":
                if in_place:
                    whole[w] = out[w] = d_verdict
                else:
                    whole[w] = torch.full((n_points + 32 * guard,), 0xA5, dtype=torch.uint8, device=dev)
                    out[w] = whole[w][16 * guard:16 * guard + n_points]
            else:
                whole[w] = torch.full((rows[w][0] + 2 * guard + 1, rows[w][1]), 0xA5, dtype=torch.uint8, device=dev)
                out[w] = whole[w][guard:guard + rows[w][0]]

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        self._chk(self.lib.scvod_track_visibility_device(
            self.h, ptr(d_objects), ptr(d_obj_offsets), int(n_scans), None if p is None else p.ctypes.data_as(C.c_void_p),
            ptr(trk["links"]), cap_objects, ptr(trk["tracks"]), cap_tracks, ptr(trk["track_objects"]), ptr(trk["n_tracks"]),
            ptr(d_object_vis), ptr(d_point_object), ptr(d_verdict), ptr(out.get("verdict")), n_points,
            C.byref(params) if params is not None else None, ptr(out.get("track_votes")), cap_tv, ptr(out.get("object_votes")), cap_ov,
            C.c_void_p(stream or 0)))
        return (out, whole) if full else out

    def track_visibility_stats(self):
        """{objects, tracks, tracks_voted, members_motion, members_cleared, to_seen_through, to_keep, latch} of the last
        track_visibility call; synchronises its stream; raises after a capacity overflow (latch bit 1 or 2)"""
        o = (C.c_int64 * 8)()
        self._chk(self.lib.scvod_track_visibility_stats(self.h, o))
        return dict(zip(TRKVIS_STATS, (int(v) for v in o)))

    def track_visibility_scratch_bytes(self):
        """device scratch of the stage on this ctx (not part of arena_bytes and no other stage's scratch)"""
        return int(self.lib.scvod_track_visibility_scratch_bytes(self.h))

    # ---- a cloud against every scan's range image (include/scvod.h: scvod_cloud_visibility_device) ----
    def cloud_visibility(self, d_xyzi, d_images, poses, params=None, flags=0, want=("votes", "verdict"), stream=None):
        """scvod_cloud_visibility_device: the world-frame cloud `d_xyzi` (torch float32 [n, 4] on the ctx's device) against the range
        images `d_images` (torch float32 [n_scans, A, S], as batch_visibility / visibility_device write them) of the scans at `poses`
        ([n_scans, 6] or None: the zero pose).  A dict of device tensors, one per name in `want` (CVIS_OUTPUTS; None: both): votes
        int16 [n, 4] holding the uint16 bits {n_through, n_agree, n_occluded, n_empty}, verdict uint8 [n] (VIS_*).  Stream-ordered."""
        import torch
        want = CVIS_OUTPUTS if want is None else tuple(want)
        assert all(w in CVIS_OUTPUTS for w in want), want
        _, S, A, _ = grid_dims(self.params)
        n = int(d_xyzi.shape[0])
        n_scans = int(d_images.shape[0])
        assert d_images.dtype == torch.float32 and d_images.is_contiguous() and d_images.numel() == n_scans * A * S
        assert d_xyzi.dtype == torch.float32 and d_xyzi.is_contiguous() and (n == 0 or d_xyzi.shape[1] == 4)
        p = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p is None or p.shape[0] == n_scans
        prm = params if params is not None else cloud_visibility_params_default()
        dev = torch.device("cuda", self.device)
        out = {}
        if "votes" in want:
            out["votes"] = torch.empty((n, 4), dtype=torch.int16, device=dev)
        if "verdict" in want:
            out["verdict"] = torch.empty((n,), dtype=torch.uint8, device=dev)
        ptr = [C.c_void_p(out[w].data_ptr()) if w in out and n > 0 else None for w in CVIS_OUTPUTS]
        self._chk(self.lib.scvod_cloud_visibility_device(self.h, C.c_void_p(d_xyzi.data_ptr()) if n > 0 else None, n,
                                                         C.c_void_p(d_images.data_ptr()) if n_scans > 0 else None,
                                                         None if p is None else p.ctypes.data_as(C.c_void_p), n_scans, C.byref(prm),
                                                         int(flags), *ptr, C.c_void_p(stream or 0)))
        return out

    def cloud_visibility_stats(self):
        """{points, finite, seen_through, keep, untested (among the finite), through, agree, occluded, empty, steps} of the last
        cloud_visibility (synchronises its stream); steps: the (chunk, scan) steps that were not skipped"""
        o = (C.c_int64 * 10)()
        self._chk(self.lib.scvod_cloud_visibility_stats(self.h, o))
        return dict(zip(CVIS_STATS, (int(v) for v in o)))

    def cloud_visibility_scratch_bytes(self):
        """device scratch the stage holds on this ctx (0 before the first call)"""
        return int(self.lib.scvod_cloud_visibility_scratch_bytes(self.h))

    def voxelgrid(self, xyzi, leaf=(0.08, 0.08, 0.08), labels=None, max_intensity=1.0):
        """SSC::getCloud label filter + pcl::VoxelGrid of one host scan (ssc.cpp:1063-1076, 1103-1106)."""
        x, px = self._f32(xyzi)
        n = x.shape[0]
        lf = np.asarray(leaf, np.float32)
        lab = None if labels is None else np.ascontiguousarray(labels, np.uint32)
        out = np.zeros((max(n, 1), 4), np.float32)
        n_out = C.c_int32(0)
        self._chk(self.lib.scvod_voxelgrid(self.h, px, None if lab is None else lab.ctypes.data_as(C.c_void_p), n,
                                           lf.ctypes.data_as(C.c_void_p), float(max_intensity), out.ctypes.data_as(C.c_void_p),
                                           out.shape[0], C.byref(n_out)))
        return out[:n_out.value]

    def batch_voxelgrid(self, d_xyzi, offsets, d_out, leaf=(0.08, 0.08, 0.08), d_labels=None, max_intensity=1.0, stream=None):
        """Device-resident form: d_xyzi / d_out / d_labels are torch CUDA tensors; returns the output offsets."""
        offs = np.ascontiguousarray(offsets, np.int32)
        lf = np.asarray(leaf, np.float32)
        out_off = np.zeros(len(offs), np.int32)
        self._chk(self.lib.scvod_batch_voxelgrid(self.h, C.c_void_p(d_xyzi.data_ptr()),
                                                 None if d_labels is None else C.c_void_p(d_labels.data_ptr()),
                                                 offs.ctypes.data_as(C.c_void_p), len(offs) - 1, lf.ctypes.data_as(C.c_void_p),
                                                 float(max_intensity), C.c_void_p(d_out.data_ptr()), int(d_out.shape[0]),
                                                 out_off.ctypes.data_as(C.c_void_p), C.c_void_p(stream) if stream else None))
        return out_off

    def nn_search(self, map_xyz, query_xyz, radius):
        m, pm = self._f32(map_xyz)
        q, pq = self._f32(query_xyz)
        nq = q.shape[0]
        idx = np.zeros(max(nq, 1), np.int32)
        sq = np.zeros(max(nq, 1), np.float32)
        w = np.zeros(max(nq, 1), np.uint8)
        self._chk(self.lib.scvod_nn_search(self.h, pm, m.shape[0], pq, nq, float(radius), idx.ctypes.data_as(C.c_void_p),
                                           sq.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)))
        return idx[:nq], sq[:nq], w[:nq]


    def nn_radius_search(self, map_xyz, query_xyz, radius):
        """nearest map point strictly inside `radius` per query: (idx or -1, squared distance or +inf, found)"""
        m, pm = self._f32(map_xyz)
        q, pq = self._f32(query_xyz)
        nq = q.shape[0]
        idx = np.zeros(max(nq, 1), np.int32)
        sq = np.zeros(max(nq, 1), np.float32)
        self._chk(self.lib.scvod_nn_radius_search(self.h, pm, m.shape[0], pq, nq, float(radius), idx.ctypes.data_as(C.c_void_p),
                                                  sq.ctypes.data_as(C.c_void_p)))
        return idx[:nq], sq[:nq], (idx[:nq] >= 0).astype(np.uint8)


MAP_NO_GROUND, MAP_NO_REJECTED, MAP_IGNORE_DYNAMIC = 1, 2, 4
MAP_PART_UNTRACKED, MAP_PART_TRACKED = 8, 16
MAP_KIND_PLAIN, MAP_KIND_LABELLED = 0, 1  # SCVOD_MAP_KIND_*
# scvod_batch_point_labels: one byte per input point (include/scvod.h, SCVOD_PT_*)
PT_DROPPED, PT_GROUND, PT_REJECTED, PT_UNCLUSTERED, PT_STATIC_OTHER, PT_STATIC_CAR, PT_DYNAMIC = range(7)
PT_STATIC_BUILDING = 7  # scvod_batch_point_classes only
MAPQ_MISS, MAPQ_CELL, MAPQ_NEAR, MAPQ_OUT = 0, 1, 2, 3  # SCVOD_MAPQ_*: the result byte of StaticMap.query
MAPQ_OUTPUTS = ("result", "cell_val", "nn_key", "nn_sqdist", "scan_counts")


class StaticMap:
    """World-frame static map (include/scvod.h, scvod_map_*): device-resident set of occupied cells, mergeable across shards."""

    def __init__(self, capacity_cells, leaf=0.2, device=0, kind=MAP_KIND_PLAIN):
        """kind: MAP_KIND_PLAIN, or MAP_KIND_LABELLED for the recognised map (a label byte per cell)"""
        self.lib = load_lib()
        h = C.c_void_p()
        rc = self.lib.scvod_map_create_kind(int(device), int(capacity_cells), float(leaf), int(kind), C.byref(h))
        if rc != 0:
            raise ScvodError(f"status {rc}: scvod_map_create_kind failed")
        self.h = h
        self.leaf = float(leaf)
        self.device = int(device)
        self.kind = int(kind)

    def _chk(self, rc):
        if rc != 0:
            raise ScvodError(f"status {rc}: {self.lib.scvod_map_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            self.lib.scvod_map_destroy(self.h)
            self.h = None

    def clear(self, stream=None):
        self._chk(self.lib.scvod_map_clear(self.h, C.c_void_p(stream or 0)))

    def accumulate(self, ctx, poses, flags=0, stream=None):
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p.shape[0] == ctx._n_scans
        self._chk(self.lib.scvod_batch_map_accumulate(ctx.h, self.h, p.ctypes.data_as(C.c_void_p), int(flags), C.c_void_p(stream or 0)))

    def accumulate_range(self, ctx, poses, first, count, flags=0, stream=None):
        """scans [first, first + count) of the batch only: a shard's own block without its halo"""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p.shape[0] == ctx._n_scans
        self._chk(self.lib.scvod_batch_map_accumulate_range(ctx.h, self.h, p.ctypes.data_as(C.c_void_p), int(flags), int(first), int(count), C.c_void_p(stream or 0)))

    @staticmethod
    def _table256(t):
        """a keep / select table as 256 bytes: None (all), a [256] array, or the labels that are set"""
        if t is None:
            return None, None
        a = np.asarray(t)
        if a.shape != (256,):
            a = np.zeros(256, np.uint8)
            a[np.asarray(t, np.int64).reshape(-1)] = 1
        a = np.ascontiguousarray(a != 0, np.uint8)
        return a, a.ctypes.data_as(C.c_void_p)

    def accumulate_labelled(self, d_xyzi, d_labels, scan_offsets, poses=None, keep=None, stream=None):
        """labelled maps: the caller's own cloud (torch float32 [n, 4]) and label bytes (torch uint8 [n]); keep: see _table256"""
        off = np.ascontiguousarray(scan_offsets, np.int32)
        p = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p is None or p.shape[0] == len(off) - 1
        k, pk = self._table256(keep)
        self._chk(self.lib.scvod_map_accumulate_labelled(self.h, C.c_void_p(d_xyzi.data_ptr()), C.c_void_p(d_labels.data_ptr()),
                                                         off.ctypes.data_as(C.c_void_p), len(off) - 1,
                                                         None if p is None else p.ctypes.data_as(C.c_void_p), pk, C.c_void_p(stream or 0)))

    def accumulate_classes(self, ctx, poses, flags=0, first=0, count=-1, stream=None):
        """labelled maps: the recognised map of the ctx's last batch (scvod_batch_map_accumulate_classes)"""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p.shape[0] == ctx._n_scans
        self._chk(self.lib.scvod_batch_map_accumulate_classes(ctx.h, self.h, p.ctypes.data_as(C.c_void_p), int(flags), int(first), int(count),
                                                              C.c_void_p(stream or 0)))

    def scratch_bytes(self):
        return int(self.lib.scvod_map_scratch_bytes(self.h))

    def _query_outputs(self, n, n_scans, radius, want):
        """the device tensors a query writes, by name (MAPQ_OUTPUTS), and the five pointers in the C order"""
        import torch
        want = tuple(w for w in MAPQ_OUTPUTS if float(radius) > 0.0 or not w.startswith("nn_")) if want is None else tuple(want)
        assert all(w in MAPQ_OUTPUTS for w in want), want
        dev = torch.device("cuda", self.device)
        shape = {"result": ((n,), torch.uint8), "cell_val": ((n,), torch.int64), "nn_key": ((n,), torch.int64),
                 "nn_sqdist": ((n,), torch.float32), "scan_counts": ((n_scans, 4), torch.int64)}
        out = {w: torch.empty(shape[w][0], dtype=shape[w][1], device=dev) for w in want}
        return out, [C.c_void_p(out[w].data_ptr()) if w in out else None for w in MAPQ_OUTPUTS]

    def query(self, d_xyzi, scan_offsets, poses=None, radius=0.0, select=None, want=("result",), stream=None):
        """scvod_map_query of the caller's cloud (torch float32 [n, 4] on the map's device): a dict of device tensors, one per name in
        `want` (MAPQ_OUTPUTS; None: every output the radius allows) -- result uint8 [n], cell_val and nn_key int64 [n] (the bits of the
        uint64), nn_sqdist float32 [n], scan_counts int64 [n_scans, 4] = {CELL, NEAR, MISS, OUT}.  Rows are at the input index, so the
        offsets should start at 0.  select: see _table256 (labelled maps only).  Stream-ordered, no synchronisation."""
        off = np.ascontiguousarray(scan_offsets, np.int32)
        p = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p is None or p.shape[0] == len(off) - 1
        out, ptr = self._query_outputs(int(off[-1]) if len(off) else 0, len(off) - 1, radius, want)
        k, pk = self._table256(select)
        self._chk(self.lib.scvod_map_query(self.h, C.c_void_p(d_xyzi.data_ptr()), off.ctypes.data_as(C.c_void_p), len(off) - 1,
                                           None if p is None else p.ctypes.data_as(C.c_void_p), float(radius), pk, *ptr, C.c_void_p(stream or 0)))
        return out

    def query_batch(self, ctx, poses, radius=0.0, select=None, want=("result",), stream=None):
        """scvod_batch_map_query: the same for every input point of the ctx's last batch"""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p.shape[0] == ctx._n_scans
        out, ptr = self._query_outputs(int(ctx._n_pts), ctx._n_scans, radius, want)
        k, pk = self._table256(select)
        self._chk(self.lib.scvod_batch_map_query(ctx.h, self.h, p.ctypes.data_as(C.c_void_p), float(radius), pk, *ptr, C.c_void_p(stream or 0)))
        return out

    def query_stats(self):
        """{points, cell, near, miss, out} of the last query (synchronises its stream)"""
        o = (C.c_int64 * 8)()
        self._chk(self.lib.scvod_map_query_stats(self.h, o))
        return dict(zip(("points", "cell", "near", "miss", "out"), (int(v) for v in o[:5])))

    def query_scratch_bytes(self):
        return int(self.lib.scvod_map_query_scratch_bytes(self.h))

    # ---- refining scan poses against the map (include/scvod.h: scvod_map_register) ----
    def register(self, d_xyzi, scan_offsets, poses=None, labels=None, params=None, select=None, stream=None):
        """scvod_map_register of the caller's cloud (torch float32 [n, 4]; labels: torch uint8 [n] or None): (d_pose_out float64
        [n_scans, 12], d_records uint8 [n_scans * 64]) on the device, stream-ordered; register_result brings them to the host"""
        off = np.ascontiguousarray(scan_offsets, np.int32)
        p = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p is None or p.shape[0] == len(off) - 1
        pose, rec = _register_outputs(len(off) - 1, self.device)
        k, pk = self._table256(select)
        self._chk(self.lib.scvod_map_register(self.h, C.c_void_p(d_xyzi.data_ptr()), off.ctypes.data_as(C.c_void_p), len(off) - 1,
                                              None if p is None else p.ctypes.data_as(C.c_void_p),
                                              None if labels is None else C.c_void_p(labels.data_ptr()),
                                              C.byref(params) if params is not None else None, pk, C.c_void_p(pose.data_ptr()),
                                              C.c_void_p(rec.data_ptr()), C.c_void_p(stream or 0)))
        return pose, rec

    def register_batch(self, ctx, poses, labels=None, params=None, select=None, stream=None):
        """scvod_batch_map_register: the same for the input cloud of the ctx's last batch (labels: typically ctx's point labels)"""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p.shape[0] == ctx._n_scans
        pose, rec = _register_outputs(ctx._n_scans, self.device)
        k, pk = self._table256(select)
        self._chk(self.lib.scvod_batch_map_register(ctx.h, self.h, p.ctypes.data_as(C.c_void_p),
                                                    None if labels is None else C.c_void_p(labels.data_ptr()),
                                                    C.byref(params) if params is not None else None, pk, C.c_void_p(pose.data_ptr()),
                                                    C.c_void_p(rec.data_ptr()), C.c_void_p(stream or 0)))
        return pose, rec

    def register_stats(self):
        """REGISTER_STATS of the last register call on this map (synchronises its stream)"""
        o = (C.c_int64 * 8)()
        self._chk(self.lib.scvod_map_register_stats(self.h, o))
        return dict(zip(REGISTER_STATS, (int(v) for v in o)))

    def register_scratch_bytes(self):
        return int(self.lib.scvod_map_register_scratch_bytes(self.h))

    # ---- cleaning scans against the map (include/scvod.h: scvod_map_filter) ----
    def _filter_outputs(self, n, n_scans, want, payload, votes_cap):
        """the device tensors a filter writes, by name (MAPF_OUTPUTS), and the pointers result .. xyzi, payload out, votes"""
        import torch
        want = tuple(want)
        assert all(w in MAPF_OUTPUTS for w in want), want
        assert "payload" not in want or payload is not None, "a payload output needs a payload input"
        dev = torch.device("cuda", self.device)
        shape = {"result": ((n,), torch.uint8), "side": ((n,), torch.uint8), "order": ((n,), torch.int32), "bounds": ((n_scans, 2), torch.int32),
                 "xyzi": ((n, 4), torch.float32), "payload": ((n,), torch.int32), "votes": ((int(votes_cap or 0), 8), torch.int32)}
        out = {w: torch.empty(shape[w][0], dtype=shape[w][1], device=dev) for w in want}
        return out, {w: (C.c_void_p(out[w].data_ptr()) if w in out else None) for w in MAPF_OUTPUTS}

    def filter(self, d_xyzi, scan_offsets, poses=None, params=None, select=None, want=("side",), payload=None, stream=None):
        """scvod_map_filter of the caller's cloud (torch float32 [n, 4] on the map's device): a dict of device tensors, one per name in
        `want` -- result and side uint8 [n], order int32 [n] (in-scan indices: KNOWN, NOVEL, OUT per scan), bounds int32 [n_scans, 2],
        xyzi float32 [n, 4], payload int32 [n] (the gather of `payload`, a torch tensor of one 32-bit word per point).  Rows are at the
        input index, so the offsets should start at 0.  Stream-ordered, no synchronisation."""
        off = np.ascontiguousarray(scan_offsets, np.int32)
        p = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p is None or p.shape[0] == len(off) - 1
        out, ptr = self._filter_outputs(int(off[-1]) if len(off) else 0, len(off) - 1, want, payload, None)
        k, pk = self._table256(select)
        self._chk(self.lib.scvod_map_filter(self.h, C.c_void_p(d_xyzi.data_ptr()), off.ctypes.data_as(C.c_void_p), len(off) - 1,
                                            None if p is None else p.ctypes.data_as(C.c_void_p), C.byref(params) if params is not None else None, pk,
                                            ptr["result"], ptr["side"], ptr["order"], ptr["bounds"], ptr["xyzi"],
                                            None if payload is None else C.c_void_p(payload.data_ptr()), ptr["payload"], C.c_void_p(stream or 0)))
        return out

    def filter_batch(self, ctx, poses, params=None, select=None, want=("side",), payload=None, votes_cap=None, stream=None):
        """scvod_batch_map_filter: the same for every input point of the ctx's last batch.  With MAPF_OBJECT_VOTE in params.flags the
        objects of the ctx's last object table vote; "votes" in want: int32 [votes_cap, 8] records (view as MAP_FILTER_OBJECT_DTYPE on
        the host; votes_cap None: one per input point, which no table outgrows)"""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        assert p.shape[0] == ctx._n_scans
        cap = int(ctx._n_pts) if votes_cap is None else int(votes_cap)
        out, ptr = self._filter_outputs(int(ctx._n_pts), ctx._n_scans, want, payload, cap)
        k, pk = self._table256(select)
        self._chk(self.lib.scvod_batch_map_filter(ctx.h, self.h, p.ctypes.data_as(C.c_void_p), C.byref(params) if params is not None else None, pk,
                                                  ptr["result"], ptr["side"], ptr["order"], ptr["bounds"], ptr["xyzi"],
                                                  None if payload is None else C.c_void_p(payload.data_ptr()), ptr["payload"],
                                                  ptr["votes"], cap if "votes" in out else 0, C.c_void_p(stream or 0)))
        return out

    def filter_stats(self):
        """the MAP_FILTER_STATS of the last filter as a dict (synchronises its stream); ScvodError with status -4 after a votes overflow"""
        o = (C.c_int64 * 8)()
        self._chk(self.lib.scvod_map_filter_stats(self.h, o))
        return dict(zip(MAP_FILTER_STATS, (int(v) for v in o)))

    def filter_scratch_bytes(self):
        return int(self.lib.scvod_map_filter_scratch_bytes(self.h))

    def points_labelled(self, select=None, stream=None):
        """labelled maps: (xyzi float32 [n, 4], labels uint8 [n], records int64 [n, 2]) of the cells whose label is selected (see
        _table256; None: all), device tensors in the same (unspecified) order"""
        import torch
        n0 = max(self.count(stream), 1)
        dev = torch.device("cuda", self.device)
        xyzi = torch.empty((n0, 4), dtype=torch.float32, device=dev)
        lab = torch.empty((n0,), dtype=torch.uint8, device=dev)
        rec = torch.empty((n0, 2), dtype=torch.int64, device=dev)
        n = C.c_int64()
        k, pk = self._table256(select)
        self._chk(self.lib.scvod_map_points_labelled(self.h, C.c_void_p(xyzi.data_ptr()), C.c_void_p(lab.data_ptr()), C.c_void_p(rec.data_ptr()), n0,
                                                     pk, C.byref(n), C.c_void_p(stream or 0)))
        return xyzi[:int(n.value)], lab[:int(n.value)], rec[:int(n.value)]

    def count(self, stream=None):
        n = C.c_int64()
        self._chk(self.lib.scvod_map_export(self.h, None, 0, C.byref(n), C.c_void_p(stream or 0)))
        return int(n.value)

    def export(self, d_records=None, stream=None):
        """records as a torch int64 device tensor [n, 2] (cell key, packed point); unspecified order"""
        import torch
        if d_records is None:
            d_records = torch.empty((max(self.count(stream), 1), 2), dtype=torch.int64, device=torch.device("cuda", self.device))
        n = C.c_int64()
        self._chk(self.lib.scvod_map_export(self.h, C.c_void_p(d_records.data_ptr()), int(d_records.shape[0]), C.byref(n), C.c_void_p(stream or 0)))
        return d_records[:int(n.value)]

    def export_parts(self, n_parts, stream=None):
        """(records [n, 2] int64 grouped by owner shard, counts per shard): the send side of the map's reduce-scatter"""
        import torch
        rec = torch.empty((max(self.count(stream), 1), 2), dtype=torch.int64, device=torch.device("cuda", self.device))
        cnt = (C.c_int64 * int(n_parts))()
        self._chk(self.lib.scvod_map_export_parts(self.h, int(n_parts), C.c_void_p(rec.data_ptr()), int(rec.shape[0]), cnt, C.c_void_p(stream or 0)))
        counts = [int(v) for v in cnt]
        return rec[:sum(counts)], counts

    def export_parts_padded(self, n_parts, d_records, d_counts=None, stream=None):
        """d_records: torch int64 device tensor [n_parts, cap, 2], filled group by group, padded with key -1; d_counts: int64
        device tensor [n_parts] or None.  No host synchronisation (the timed multi-GPU step)."""
        assert d_records.dim() == 3 and d_records.shape[0] == n_parts and d_records.shape[2] == 2 and d_records.is_contiguous()
        self._chk(self.lib.scvod_map_export_parts_padded(self.h, int(n_parts), C.c_void_p(d_records.data_ptr()), int(d_records.shape[1]),
                                                         C.c_void_p(d_counts.data_ptr()) if d_counts is not None else None, C.c_void_p(stream or 0)))

    def merge(self, d_records, stream=None):
        self._chk(self.lib.scvod_map_merge(self.h, C.c_void_p(d_records.data_ptr()), int(d_records.numel() // 2), C.c_void_p(stream or 0)))

    # ---- connected components of the map's cells and their vote (include/scvod.h: scvod_map_components) ----
    def components(self, records, connectivity=26, cap=None, want=MAP_COMPONENTS_OUTPUTS, stream=None):
        """scvod_map_components of the list `records` (torch int64 [n, 2] on the map's device, as points / points_labelled / export hand
        it out; only the keys are read): a dict of device tensors, one per name in `want` (MAP_COMPONENTS_OUTPUTS; "table" brings "n") --
        component int32 [n] (-1: no node), table uint8 [cap, 48] (view as MAP_COMPONENT_DTYPE on the host; cap None: n, which holds
        every table; the rows behind n are not initialised), n int64 [1].  Components are numbered ascending by their smallest cell
        key.  Stream-ordered, no synchronisation; components_stats() tells what happened"""
        import torch
        want = tuple(want)
        assert all(w in MAP_COMPONENTS_OUTPUTS for w in want), want
        assert records.dtype == torch.int64 and records.is_contiguous() and (records.numel() == 0 or records.shape[-1] == 2)
        n = int(records.numel() // 2)
        cap = int(n if cap is None else cap)
        dev = torch.device("cuda", self.device)
        out = {}
        if "component" in want:
            out["component"] = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)[:n]
        if "table" in want:
            out["table"] = torch.empty((max(cap, 1), MAP_COMPONENT_DTYPE.itemsize), dtype=torch.uint8, device=dev)[:cap]
        if "n" in want or "table" in want:
            out["n"] = torch.empty((1,), dtype=torch.int64, device=dev)
        self._chk(self.lib.scvod_map_components(
            self.h, C.c_void_p(records.data_ptr()) if n > 0 else None, n, int(connectivity),
            C.c_void_p(out["component"].data_ptr()) if "component" in out and n > 0 else None,
            C.c_void_p(out["table"].data_ptr()) if "table" in out else None, cap if "table" in out else 0,
            C.c_void_p(out["n"].data_ptr()) if "n" in out else None, C.c_void_p(stream or 0)))
        return out

    def components_stats(self):
        """the MAP_COMPONENTS_STATS of the last components() as a dict (synchronises its stream); ScvodError with status -4 after a
        table overflow"""
        o = (C.c_int64 * 8)()
        self._chk(self.lib.scvod_map_components_stats(self.h, o))
        return dict(zip(MAP_COMPONENTS_STATS, (int(v) for v in o)))

    def components_scratch_bytes(self):
        return int(self.lib.scvod_map_components_scratch_bytes(self.h))

    def component_visibility(self, comp, verdict, votes=None, params=None, cap_components=None, cap=None, want=CMPVIS_OUTPUTS, in_place=False,
                             stream=None):
        """scvod_map_component_visibility: `comp` the dict components() returned for the same list (its "component" and "n"), verdict
        uint8 [n] and votes int16 [n, 4] as Ctx.cloud_visibility wrote them for the same points (votes None: no pooled sums).  A dict
        of device tensors, one per name in `want` (CMPVIS_OUTPUTS): records uint8 [cap, 64] (view as COMPONENT_VISIBILITY_DTYPE on the
        host; cap None: n), verdict uint8 [n] -- with in_place=True `verdict` itself, rewritten.  cap_components None: n (every
        component votes).  Stream-ordered, no host read; component_visibility_stats() tells what happened"""
        import torch
        want = tuple(want)
        assert all(w in CMPVIS_OUTPUTS for w in want), want
        d_comp, d_n = comp["component"], comp["n"]
        n = int(d_comp.numel())
        assert d_comp.dtype == torch.int32 and d_comp.is_contiguous() and d_n.dtype == torch.int64
        assert verdict.dtype == torch.uint8 and verdict.is_contiguous() and verdict.numel() == n
        assert votes is None or (votes.is_contiguous() and votes.element_size() == 2 and votes.numel() == 4 * n)
        cap = int(n if cap is None else cap)
        cap_components = int(n if cap_components is None else cap_components)
        out = {}
        if "records" in want:
            out["records"] = torch.empty((max(cap, 1), COMPONENT_VISIBILITY_DTYPE.itemsize), dtype=torch.uint8, device=verdict.device)[:cap]
        if "verdict" in want:
            out["verdict"] = verdict if in_place else torch.empty((max(n, 1),), dtype=torch.uint8, device=verdict.device)[:n]
        self._chk(self.lib.scvod_map_component_visibility(
            self.h, C.c_void_p(d_comp.data_ptr()) if n > 0 else None, n, C.c_void_p(d_n.data_ptr()), cap_components,
            C.c_void_p(verdict.data_ptr()) if n > 0 else None, None if votes is None or n == 0 else C.c_void_p(votes.data_ptr()),
            C.byref(params) if params is not None else None, C.c_void_p(out["records"].data_ptr()) if "records" in out else None,
            cap if "records" in out else 0, C.c_void_p(out["verdict"].data_ptr()) if "verdict" in out and n > 0 else None,
            C.c_void_p(stream or 0)))
        return out

    def component_visibility_stats(self):
        """the CMPVIS_STATS of the last component_visibility() as a dict (synchronises its stream); ScvodError with status -4 after a
        records overflow"""
        o = (C.c_int64 * 8)()
        self._chk(self.lib.scvod_map_component_visibility_stats(self.h, o))
        return dict(zip(CMPVIS_STATS, (int(v) for v in o)))

    def points_normals(self, ctx, params=None, select=None, with_labels=False, cap=None, stream=None):
        """scvod_map_points_normals: dict(xyzi float32 [n, 4], xyz float32 [n, 3] packed -- ready for Ctx.register_device --, normals
        float32 [n, 3], curvature float32 [n] and, labelled maps with with_labels, labels uint8 [n]) device tensors, row i the same cell,
        the order unspecified.  select: see _table256 (labelled maps only).  cap None: the map's count.  Errors are the ctx's"""
        import torch
        n0 = max(self.count(stream), 1) if cap is None else int(cap)
        dev = torch.device("cuda", self.device)
        xyzi = torch.empty((max(n0, 1), 4), dtype=torch.float32, device=dev)
        nrm = torch.empty((max(n0, 1), 3), dtype=torch.float32, device=dev)
        cur = torch.empty((max(n0, 1),), dtype=torch.float32, device=dev)
        lab = torch.empty((max(n0, 1),), dtype=torch.uint8, device=dev) if with_labels else None
        n = C.c_int64()
        k, pk = self._table256(select)
        ctx._chk(self.lib.scvod_map_points_normals(ctx.h, self.h, C.byref(params) if params is not None else None, pk, C.c_void_p(xyzi.data_ptr()),
                                                   None if lab is None else C.c_void_p(lab.data_ptr()), C.c_void_p(nrm.data_ptr()),
                                                   C.c_void_p(cur.data_ptr()), n0, C.byref(n), C.c_void_p(stream or 0)))
        n = int(n.value)
        out = dict(xyzi=xyzi[:n], normals=nrm[:n], curvature=cur[:n])
        if lab is not None:
            out["labels"] = lab[:n]
        # the points are complete (the call synchronised behind them); the packed copy is finished before this returns, so a register
        # call on any stream may read it.  The normals are stream-ordered on the call's stream
        out["xyz"] = xyzi[:n, :3].contiguous()
        torch.cuda.current_stream(dev).synchronize()
        return out

    def points(self, stream=None):
        """(xyzi float32 [n, 4], records int64 [n, 2]) device tensors, same (unspecified) order"""
        import torch
        n0 = max(self.count(stream), 1)
        dev = torch.device("cuda", self.device)
        xyzi = torch.empty((n0, 4), dtype=torch.float32, device=dev)
        rec = torch.empty((n0, 2), dtype=torch.int64, device=dev)
        n = C.c_int64()
        self._chk(self.lib.scvod_map_points(self.h, C.c_void_p(xyzi.data_ptr()), C.c_void_p(rec.data_ptr()), n0, C.byref(n), C.c_void_p(stream or 0)))
        return xyzi[:int(n.value)], rec[:int(n.value)]


def pose_matrix(pose):
    p = np.ascontiguousarray(pose, np.float32)
    t = np.zeros(12, np.float32)
    load_lib().scvod_pose_matrix(p.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p))
    return t


STACK_REFERENCE_BOUND = 1  # SCVOD_STACK_REFERENCE_BOUND


def stack_offsets(offsets, window=3, interval=3, reference_bound=False):
    """(out_offsets [n_out + 1], mid [n_out]) of the scan stacking (scvod_stack_offsets; host only): group g holds the scans
    g * interval .. g * interval + window - 1 and hands on the pose of scan mid[g].  reference_bound: the loop bound of the
    reference's stacker, which drops the last complete group when the scan count is a multiple of interval"""
    lib = load_lib()
    off = np.ascontiguousarray(offsets, np.int32)
    n_in = off.shape[0] - 1
    flags = STACK_REFERENCE_BOUND if reference_bound else 0
    n_out = lib.scvod_stack_offsets(off.ctypes.data_as(C.c_void_p), n_in, int(window), int(interval), flags, None, None, 0, None)
    if n_out < 0:
        raise ScvodError(f"scvod_stack_offsets: status {n_out} (window {window}, interval {interval})")
    out = np.zeros(n_out + 1, np.int32)
    mid = np.zeros(n_out, np.int32)
    rc = lib.scvod_stack_offsets(off.ctypes.data_as(C.c_void_p), n_in, int(window), int(interval), flags, out.ctypes.data_as(C.c_void_p),
                                 mid.ctypes.data_as(C.c_void_p), n_out, None)
    if rc != n_out:
        raise ScvodError(f"scvod_stack_offsets: status {rc}")
    return out, mid


def pose_from_matrix(M):
    """{x, y, z, roll, pitch, yaw} of a row-major 3x4 (or 12-vector) pose matrix (scvod_pose_from_matrix; host only)"""
    m = np.ascontiguousarray(M, np.float32).reshape(12)
    out = np.zeros(6, np.float32)
    load_lib().scvod_pose_from_matrix(m.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out
