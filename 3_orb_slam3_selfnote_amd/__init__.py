"""orb-frontend-mi355x: ORB-SLAM3's per-frame feature front end on MI355X.

Host-side mirror (Python, ctypes) of the C ABI in include/orbhip.h, keeping the reference's names:
`ORBextractor` (include/ORBextractor.h:43-109), `ORBmatcher` (include/ORBmatcher.h:35-108).  The C++ drop-in
classes with the reference's exact signatures live in csrc/adapter/.  This module is what tests/ and bench.py
drive; it contains no compute of its own and no CPU fallback: if liborbhip.so is missing or no HIP device is
usable, construction raises.

The package name starts with a digit (it is fixed by the project layout), so import it with
    importlib.import_module("3_orb_slam3_selfnote_amd")
"""
import ctypes as C
import os
import time

import numpy as np

from . import build as _build

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORBHIP_LIB", os.path.join(HERE, "liborbhip.so"))  # ORBHIP_LIB: diagnostic builds only

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28

E_EMPTY, E_ARG, E_HIP, E_CAP = -1, -2, -3, -4
CLOSE_MAX_KEYPOINTS = 4096  # ORBX_CLOSE_MAX_KEYPOINTS
FISHEYE_MAX_KEYPOINTS = 12960  # ORBM_FISHEYE_MAX_KEYPOINTS
CLAHE_BAND_ROWS = 32  # ORBX_CLAHE_BAND_ROWS
REMAP_FRAME_CHUNK = 16  # ORBX_REMAP_FRAME_CHUNK

# every symbol include/orbhip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "orbx_create", "orbx_destroy", "orbx_last_error", "orbx_get_levels", "orbx_get_scale_factor",
    "orbx_get_scale_tables", "orbx_get_features_per_level", "orbx_configure", "orbx_max_keypoints", "orbx_extract",
    "orbx_extract_batch_device", "orbx_get_host_us", "orbx_level_info", "orbx_download_level", "orbx_download_pyramid", "orbx_download_blurred_level",
    "orbx_download_candidates", "orbx_download_level_keypoints", "orbx_set_profiling", "orbx_get_stage_ms",
    "orbx_ref_cosf", "orbx_ref_sinf", "orbx_ref_atanf", "orbx_ref_atan2f", "orbx_ref_logf", "orbx_logf_device", "orbx_ref_tanf", "orbx_tanf_device", "orbx_cosf_device", "orbx_sinf_device", "orbx_atanf_device", "orbx_atan2f_device", "orbx_fast_atan2_device", "orbx_compute_stereo_matches", "orbx_compute_stereo_matches_batch_device", "orbx_stereo_from_rgbd_batch_device", "orbx_close_points_batch_device", "orbx_cvt_color_gray", "orbx_cvt_color_gray_device",
    "orbx_clahe", "orbx_clahe_device", "orbx_remap_linear", "orbx_remap_linear_device",
    "orbx_clahe_batch_device", "orbx_remap_linear_batch_device", "orbx_clahe_band_lut_rows",
    "orbm_create", "orbm_destroy", "orbm_last_error", "orbm_descriptor_distance", "orbm_search_by_projection",
    "orbm_search_by_projection_batch_device", "orbm_search_by_projection_fisheye", "orbm_search_by_projection_last_frame_fisheye", "orbm_search_by_projection_last_frame_fisheye_batch_device", "orbm_rig_concat_batch_device", "orbm_unproject", "orbm_fisheye_ratio_test", "orbm_fisheye_triangulate", "orbm_fisheye_triangulate_device", "orbm_stereo_fisheye_matches_batch_device", "orbm_stereo_fisheye_matches", "orbm_search_by_projection_last_frame", "orbm_search_by_projection_last_frame_batch_device", "orbm_search_local_points", "orbm_search_local_points_batch_device", "orbm_search_local_points_fisheye", "orbm_search_local_points_fisheye_batch_device", "orbm_rig_right_camera", "orbm_search_by_projection_keyframe", "orbm_search_by_projection_sim3", "orbm_search_by_projection_sim3_cam", "orbm_fuse_sim3_cam", "orbm_search_for_triangulation", "orbm_triangulation_candidates", "orbm_search_for_triangulation_pred", "orbm_search_for_triangulation_kb8", "orbm_search_for_triangulation_neighbours", "orbm_search_for_triangulation_kb8_neighbours", "orbm_new_point_geometry", "orbm_new_point_geometry_device", "orbm_create_new_map_points", "orbm_create_new_map_points_kb8", "orbm_search_for_initialization", "orbm_search_by_bow", "orbm_search_by_bow_fisheye", "orbm_search_by_bow_keyframes", "orbm_search_by_bow_candidates", "orbm_search_by_bow_keyframes_candidates", "orbm_fuse", "orbm_fuse_sim3", "orbm_fuse_keyframes", "orbm_fuse_sim3_keyframes", "orbm_search_by_sim3", "orbm_distinctive_descriptors", "orbm_update_map_points", "orbm_map_point_normal_depth", "orbm_keyframe_culling", "orbm_keyframe_culling_open", "orbm_keyframe_culling_step", "orbm_keyframe_culling_host", "orbm_keyframe_culling_host_error", "orbm_update_local_map", "orbm_update_local_map_device", "orbm_update_local_map_host", "orbm_update_local_map_host_error", "orbm_update_connections", "orbm_update_connections_host", "orbm_gather_local_map_device", "orbm_two_view_reconstruct", "orbm_two_view_reconstruct_host", "orbm_two_view_host_error", "orbm_two_view_models", "orbm_two_view_models_host", "orbm_two_view_check_rt", "orbm_two_view_check_rt_host", "orbm_sim3_solve", "orbm_sim3_solve_host", "orbm_sim3_host_error", "orbm_sim3_hypotheses", "orbm_sim3_hypotheses_host", "orbm_sim3_check", "orbm_sim3_check_host", "orbm_sim3_ransac_iterations", "orbm_knn_match2", "orbm_hamming_matrix", "orbm_three_maxima",
    "orbm_radius_by_viewing_cos", "orbm_project", "orbm_undistort_keypoints", "orbm_image_bounds", "orbm_undistort_keypoints_batch_device", "orbm_set_profiling", "orbm_set_scan_mode", "orbm_set_hamming_engine", "orbm_get_last_ms", "orbm_get_stage_ms",
]
# the vocabulary's symbols (orbv_*), a list of their own: tests/test_abi.py holds ABI_SYMBOLS equal to the header's orbx_ / orbm_ names;
# tests/test_voc_abi.py holds this one equal to its orbv_ names, and build() asks the library for both
VOC_ABI_SYMBOLS = [
    "orbv_create", "orbv_destroy", "orbv_last_error", "orbv_n_nodes", "orbv_n_words", "orbv_max_children", "orbv_min_leaf_level",
    "orbv_transform_host", "orbv_transform", "orbv_batch_scratch_bytes", "orbv_transform_batch_device", "orbv_transform_batch_device_form",
]


# the keyframe database's symbols (orbd_*), held equal to the header's orbd_ names by tests/test_kfdb_abi.py
KFDB_ABI_SYMBOLS = [
    "orbd_create", "orbd_create_for_vocabulary", "orbd_destroy", "orbd_last_error", "orbd_n_words", "orbd_capacity", "orbd_size",
    "orbd_add", "orbd_add_device", "orbd_erase", "orbd_clear", "orbd_clear_map", "orbd_set_map", "orbd_get_members",
    "orbd_query_reloc", "orbd_query_reloc_host", "orbd_query_place", "orbd_query_place_host", "orbd_batch_scratch_bytes",
    "orbd_score_batch_device", "orbd_accumulate_reloc", "orbd_accumulate_place",
]
MAX_KEYFRAMES = 16384  # ORBD_MAX_KEYFRAMES
COVISIBLES = 10  # ORBD_COVISIBLES
NO_TAG = 0xFFFFFFFFFFFFFFFF  # ORBD_NO_TAG


class FrameStruct(C.Structure):  # orbm_frame_t
    _fields_ = [("n", C.c_int32), ("keys_un", C.c_void_p), ("descriptors", C.c_void_p), ("u_right", C.c_void_p),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


class MapPointUpdateStruct(C.Structure):  # orbm_map_point_update_t
    _fields_ = [("nmp", C.c_int32), ("start", C.c_void_p), ("desc", C.c_void_p), ("centre", C.c_void_p), ("in_desc", C.c_void_p),
                ("pos", C.c_void_p), ("ref_centre", C.c_void_p), ("ref_scale", C.c_void_p), ("ref_max_scale", C.c_void_p)]


class VocNodesStruct(C.Structure):  # orbv_nodes_t
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("weighting", C.c_int32), ("scoring", C.c_int32), ("n_nodes", C.c_int32),
                ("parent", C.c_void_p), ("is_leaf", C.c_void_p), ("descriptor", C.c_void_p), ("weight", C.c_void_p)]


class KfdbMembersStruct(C.Structure):  # orbd_members_t
    _fields_ = [("reloc_query", C.c_uint64), ("place_query", C.c_uint64), ("reloc_score", C.c_float), ("place_score", C.c_float)]


class CullingStruct(C.Structure):  # orbm_culling_t
    _fields_ = [("K", C.c_int32), ("skip", C.c_void_p), ("th_depth", C.c_void_p), ("row_start", C.c_void_p), ("row_point", C.c_void_p),
                ("row_level", C.c_void_p), ("row_depth", C.c_void_p), ("P", C.c_int32), ("bad", C.c_void_p), ("n_obs", C.c_void_p),
                ("obs_start", C.c_void_p), ("obs_kf", C.c_void_p), ("obs_level", C.c_void_p), ("obs_w", C.c_void_p), ("mono", C.c_int32),
                ("redundant_th", C.c_float)]


CULL_MAX_KEYFRAMES = 1024  # ORBM_CULL_MAX_KEYFRAMES
_CULL_TYPES = dict(skip=np.uint8, th_depth=np.float32, row_start=np.int32, row_point=np.int32, row_level=np.int32, row_depth=np.float32,
                   bad=np.uint8, n_obs=np.int32, obs_start=np.int32, obs_kf=np.int32, obs_level=np.int32, obs_w=np.uint8)


def culling_struct(scene):
    """(CullingStruct, the arrays it points to) from a scene dict: the arrays of orbm_culling_t by name (K and P come from row_start and
    obs_start; row_depth may be None when mono), `mono` and `redundant_th`."""
    A = {k: (None if scene.get(k) is None else np.ascontiguousarray(scene[k], dtype=t)) for k, t in _CULL_TYPES.items()}
    c = CullingStruct()
    c.K, c.P = len(A["row_start"]) - 1, len(A["obs_start"]) - 1
    for k in _CULL_TYPES:
        setattr(c, k, _p(A[k]))
    c.mono, c.redundant_th = int(scene["mono"]), float(scene["redundant_th"])
    return c, A


def _culling_outputs(c):
    K, P = max(c.K, 1), max(c.P, 1)
    return np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.uint8), np.zeros(P, np.int32), np.zeros(P, np.uint8)


def keyframe_culling_host(scene, erasable=None):
    """LocalMapping::KeyFrameCulling (LocalMapping.cc:1158-1310) on the CPU with the kernels' own statement (orbm_keyframe_culling_host,
    csrc/orb_ref_culling.h).  Same arguments and results as ORBmatcher.KeyFrameCulling; not a fallback of it."""
    L = load()
    c, keep = culling_struct(scene)
    era = None if erasable is None else np.ascontiguousarray(erasable, dtype=np.uint8)
    out = _culling_outputs(c)
    rc = L.orbm_keyframe_culling_host(C.byref(c), _p(era), *[_p(o) for o in out])
    if rc == E_ARG:
        raise ValueError("orbm_keyframe_culling_host: bad argument (%s)" % L.orbm_keyframe_culling_host_error().decode())
    _check_free(rc, "orbm_keyframe_culling_host")
    return out[0][:c.K], out[1][:c.K], out[2][:c.K], out[3][:c.P], out[4][:c.P]


class MapGraph(C.Structure):  # orbm_map_graph_t
    _fields_ = [("G", C.c_int32), ("kf_rank", C.c_void_p), ("kf_bad", C.c_void_p), ("kf_map", C.c_void_p), ("kf_row_start", C.c_void_p),
                ("row_point", C.c_void_p), ("kf_best", C.c_void_p), ("kf_child_start", C.c_void_p), ("kf_child", C.c_void_p),
                ("kf_parent", C.c_void_p), ("kf_prev", C.c_void_p), ("P", C.c_int32), ("pt_bad", C.c_void_p), ("obs_start", C.c_void_p),
                ("obs_kf", C.c_void_p)]


MAP_MAX_KEYFRAMES = 16384  # ORBM_MAP_MAX_KEYFRAMES
MAP_BEST = 10  # ORBM_MAP_BEST
_GRAPH_TYPES = dict(kf_rank=np.int32, kf_bad=np.uint8, kf_map=np.int32, kf_row_start=np.int32, row_point=np.int32, kf_best=np.int32,
                    kf_child_start=np.int32, kf_child=np.int32, kf_parent=np.int32, kf_prev=np.int32, pt_bad=np.uint8, obs_start=np.int32,
                    obs_kf=np.int32)


def map_graph(scene):
    """(MapGraph, the arrays it points to) from a dict of the arrays of orbm_map_graph_t by name (G and P come from kf_row_start and
    obs_start; kf_prev may be None)."""
    A = {k: (None if scene.get(k) is None else np.ascontiguousarray(scene[k], dtype=t)) for k, t in _GRAPH_TYPES.items()}
    g = MapGraph()
    g.G, g.P = len(A["kf_row_start"]) - 1, len(A["obs_start"]) - 1
    for k in _GRAPH_TYPES:
        setattr(g, k, _p(A[k]))
    return g, A


def map_graph_device(scene, device=0):
    """The same tables resident on the device: (MapGraph holding device addresses, the torch tensors that own them)."""
    import torch
    g, A = map_graph(scene)
    keep = {}
    for k, a in A.items():
        if a is None:
            setattr(g, k, None)
            continue
        keep[k] = torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to("cuda:%d" % device)
        setattr(g, k, C.c_void_p(keep[k].data_ptr()))
    return g, keep


def _local_map_outputs(N, cap_kf, cap_pts):
    return (np.zeros(max(cap_kf, 1), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(max(N, 1), np.uint8),
            np.zeros(max(cap_pts, 1), np.int32), np.zeros(1, np.int32))


def _local_map_result(rc, out, N, what):
    if rc == E_CAP:
        raise OrbError("%s: a list does not fit (needs %d keyframes, %d points)" % (what, out[1][0], out[6][0]))
    if rc < 0:
        raise OrbError("%s rc=%d" % (what, rc))
    return dict(local_kf=out[0][:out[1][0]].copy(), kf_max=int(out[2][0]), max_votes=int(out[3][0]), slot_bad=out[4][:N].copy(),
                local_point=out[5][:out[6][0]].copy())


def _local_map_caps(g, A, cap_kf, cap_pts):
    return (g.G + 24 if cap_kf is None else int(cap_kf)), (min(g.P, len(A["row_point"])) if cap_pts is None else int(cap_pts))


def update_local_map_host(scene, frame_point, inertial=False, last_kf=-1, cap_kf=None, cap_pts=None):
    """Tracking::UpdateLocalMap (Tracking.cc:3542-3762) on the CPU with the kernels' own statement (orbm_update_local_map_host,
    csrc/orb_ref_localmap.h).  Same arguments and results as ORBmatcher.UpdateLocalMap; not a fallback of it."""
    L = load()
    g, A = map_graph(scene)
    fp = np.ascontiguousarray(frame_point, dtype=np.int32)
    cap_kf, cap_pts = _local_map_caps(g, A, cap_kf, cap_pts)
    out = _local_map_outputs(len(fp), cap_kf, cap_pts)
    rc = L.orbm_update_local_map_host(C.byref(g), len(fp), _p(fp), int(bool(inertial)), int(last_kf), cap_kf, cap_pts, *[_p(o) for o in out])
    if rc == E_ARG:
        raise ValueError("orbm_update_local_map_host: bad argument (%s)" % L.orbm_update_local_map_host_error().decode())
    return _local_map_result(rc, out, len(fp), "orbm_update_local_map_host")


def _connections_outputs(T, cap):
    return (np.zeros(T + 1, np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(T + 1, np.int32),
            np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(T, 1), np.int32), np.zeros(max(T, 1), np.int32))


def _connections_result(rc, out, T, what):
    if rc == E_CAP:
        raise OrbError("%s: the lists do not fit (needs %d)" % (what, out[0][T]))
    if rc < 0:
        raise OrbError("%s rc=%d" % (what, rc))
    cs, os_ = out[0], out[3]
    return [dict(conn_kf=out[1][cs[t]:cs[t + 1]].copy(), conn_w=out[2][cs[t]:cs[t + 1]].copy(), ord_kf=out[4][os_[t]:os_[t + 1]].copy(),
                 ord_w=out[5][os_[t]:os_[t + 1]].copy(), kf_max=int(out[6][t]), nmax=int(out[7][t])) for t in range(T)]


def update_connections_host(scene, targets, th=15, cap=None):
    """KFcounter and the ordered lists of KeyFrame::UpdateConnections (KeyFrame.cc:407-492) for every keyframe of `targets`, on the CPU with
    the kernels' own statement (orbm_update_connections_host).  Same arguments and results as ORBmatcher.UpdateConnections."""
    L = load()
    g, A = map_graph(scene)
    tg = np.ascontiguousarray(targets, dtype=np.int32)
    cap = len(tg) * g.G if cap is None else int(cap)
    out = _connections_outputs(len(tg), cap)
    rc = L.orbm_update_connections_host(C.byref(g), len(tg), _p(tg), int(th), cap, *[_p(o) for o in out])
    if rc == E_ARG:
        raise ValueError("orbm_update_connections_host: bad argument (%s)" % L.orbm_update_local_map_host_error().decode())
    return _connections_result(rc, out, len(tg), "orbm_update_connections_host")


class TwoViewDetailsStruct(C.Structure):  # orbm_two_view_details_t
    _fields_ = [(k, C.c_void_p) for k in ("SH", "SF", "best_it", "H21", "F21", "inliersH", "inliersF", "score", "used_H", "nhyp", "R", "t",
                                          "nGood", "parallax", "chosen", "status")]


TV_STATUS = dict(NOT_INLIER=0, GOOD=1, LOW_PARALLAX=2, NONFINITE=3, BEHIND1=4, BEHIND2=5, REPROJ1=6, REPROJ2=7)  # ORBM_TV_*


class TwoViewResult:
    """What TwoViewReconstruction::Reconstruct returns and leaves behind: ok (the bool), R21 [3,3], t21 [3], vP3D [n1,3], vbTriangulated
    [n1] (the four are None unless ok), and `details`: every array of orbm_two_view_details_t by name (SH, SF, best_it, H21, F21,
    inliersH, inliersF, score, used_H, nhyp, R, t, nGood, parallax, chosen, status)."""

    def __init__(self, ok, R21, t21, vP3D, vbTriangulated, details):
        self.ok, self.R21, self.t21, self.vP3D, self.vbTriangulated, self.details = ok, R21, t21, vP3D, vbTriangulated, details

    def __bool__(self):
        return self.ok


def _two_view_inputs(keys1, keys2, matches12):
    keys1, keys2 = np.ascontiguousarray(keys1, dtype=KP_DTYPE), np.ascontiguousarray(keys2, dtype=KP_DTYPE)
    matches12 = np.ascontiguousarray(matches12, dtype=np.int32)
    if len(matches12) != len(keys1):
        raise ValueError("matches12 has one entry per keypoint of the first frame")
    return keys1, keys2, matches12, int((matches12 >= 0).sum())


def _two_view_reconstruct(call, what, error, keys1, keys2, matches12, K, sigma, iterations, sets):
    keys1, keys2, matches12, N = _two_view_inputs(keys1, keys2, matches12)
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    iterations = int(iterations)
    sets = np.ascontiguousarray(sets, dtype=np.int32)
    if sets.size != 8 * max(iterations, 0):
        raise ValueError("sets is [iterations][8]")
    n1, I = len(keys1), max(iterations, 1)
    R21, t21, p3d, tri = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros((max(n1, 1), 3), np.float32), np.zeros(max(n1, 1), np.uint8)
    d = dict(SH=np.zeros(1, np.float32), SF=np.zeros(1, np.float32), best_it=np.full(2, -1, np.int32), H21=np.zeros((3, 3), np.float32),
             F21=np.zeros((3, 3), np.float32), inliersH=np.zeros(max(N, 1), np.uint8), inliersF=np.zeros(max(N, 1), np.uint8),
             score=np.zeros((2, I), np.float32), used_H=np.full(1, -1, np.int32), nhyp=np.zeros(1, np.int32), R=np.zeros((8, 3, 3), np.float32),
             t=np.zeros((8, 3), np.float32), nGood=np.zeros(8, np.int32), parallax=np.zeros(8, np.float32), chosen=np.full(1, -1, np.int32),
             status=np.zeros((8, max(N, 1)), np.uint8))
    ds = TwoViewDetailsStruct()
    for k, a in d.items():
        setattr(ds, k, _p(a))
    rc = call(_p(keys1), n1, _p(keys2), len(keys2), _p(matches12), _p(K), C.c_float(sigma), iterations, _p(sets), _p(R21), _p(t21), _p(p3d),
              _p(tri), C.byref(ds))
    if rc == E_ARG:
        raise ValueError("%s: bad argument (%s)" % (what, error()))
    if rc < 0:
        raise OrbError("%s rc=%d (%s)" % (what, rc, error()))
    d["inliersH"], d["inliersF"], d["status"] = d["inliersH"][:N], d["inliersF"][:N], d["status"][:, :N]
    ok = rc == 1
    return TwoViewResult(ok, R21 if ok else None, t21 if ok else None, p3d[:n1] if ok else None, tri[:n1].astype(bool) if ok else None, d)


def _two_view_models(call, what, error, keys1, keys2, matches12, sigma, iterations, sets):
    keys1, keys2, matches12, N = _two_view_inputs(keys1, keys2, matches12)
    iterations = int(iterations)
    sets = np.ascontiguousarray(sets, dtype=np.int32)
    if sets.size != 8 * max(iterations, 0):
        raise ValueError("sets is [iterations][8]")
    I = max(iterations, 1)
    H21, H12, F21 = (np.zeros((I, 3, 3), np.float32) for _ in range(3))
    score, best, masks = np.zeros((2, I), np.float32), np.full(2, -1, np.int32), np.zeros((2, max(N, 1)), np.uint8)
    rc = call(_p(keys1), len(keys1), _p(keys2), len(keys2), _p(matches12), C.c_float(sigma), iterations, _p(sets), _p(H21), _p(H12), _p(F21),
              _p(score), _p(best), _p(masks))
    if rc == E_ARG:
        raise ValueError("%s: bad argument (%s)" % (what, error()))
    if rc < 0:
        raise OrbError("%s rc=%d (%s)" % (what, rc, error()))
    return dict(H21=H21, H12=H12, F21=F21, score=score, best_it=best, masks=masks.reshape(-1)[:2 * N].reshape(2, N))


def _two_view_check_rt(call, what, error, keys1, keys2, matches12, inliers, K, sigma, R, t):
    keys1, keys2, matches12, N = _two_view_inputs(keys1, keys2, matches12)
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(9)
    R, t = np.ascontiguousarray(R, dtype=np.float32).reshape(-1, 9), np.ascontiguousarray(t, dtype=np.float32).reshape(-1, 3)
    inliers = np.ascontiguousarray(inliers, dtype=np.uint8)
    if len(R) != len(t) or len(inliers) != N:
        raise ValueError("R [nhyp][9], t [nhyp][3], inliers [N]")
    nhyp, n1 = len(R), len(keys1)
    H = max(nhyp, 1)
    p3d, good, status = np.zeros((H, max(n1, 1), 3), np.float32), np.zeros((H, max(n1, 1)), np.uint8), np.zeros((H, max(N, 1)), np.uint8)
    nGood, cos_rank, parallax = np.zeros(H, np.int32), np.zeros(H, np.float32), np.zeros(H, np.float32)
    rc = call(_p(keys1), n1, _p(keys2), len(keys2), _p(matches12), _p(inliers), _p(K), C.c_float(sigma), nhyp, _p(R), _p(t), _p(p3d), _p(good),
              _p(status), _p(nGood), _p(cos_rank), _p(parallax))
    if rc == E_ARG:
        raise ValueError("%s: bad argument (%s)" % (what, error()))
    if rc < 0:
        raise OrbError("%s rc=%d (%s)" % (what, rc, error()))
    return dict(vP3D=p3d[:nhyp, :n1], vbGood=good[:nhyp, :n1], status=status[:nhyp, :N], nGood=nGood[:nhyp], cos_rank=cos_rank[:nhyp],
                parallax=parallax[:nhyp])


def _two_view_host_error():
    return load().orbm_two_view_host_error().decode()


def two_view_reconstruct_host(keys1, keys2, matches12, K, sigma, iterations, sets):
    """TwoViewReconstruction::Reconstruct (TwoViewReconstruction.cc:39-127) on the CPU with the kernels' own statement
    (orbm_two_view_reconstruct_host, csrc/orb_ref_twoview.h).  Same arguments and result as ORBmatcher.TwoViewReconstruct; for tests
    without a GPU, not a fallback of it."""
    return _two_view_reconstruct(load().orbm_two_view_reconstruct_host, "orbm_two_view_reconstruct_host", _two_view_host_error, keys1, keys2,
                                 matches12, K, sigma, iterations, sets)


def two_view_models_host(keys1, keys2, matches12, sigma, iterations, sets):
    """orbm_two_view_models_host: every iteration's H21, H12, F21 and scores, the winners and their inlier vectors, on the CPU."""
    return _two_view_models(load().orbm_two_view_models_host, "orbm_two_view_models_host", _two_view_host_error, keys1, keys2, matches12, sigma,
                            iterations, sets)


def two_view_check_rt_host(keys1, keys2, matches12, inliers, K, sigma, R, t):
    """orbm_two_view_check_rt_host: CheckRT (TwoViewReconstruction.cc:802-911) for the caller's hypotheses, on the CPU."""
    return _two_view_check_rt(load().orbm_two_view_check_rt_host, "orbm_two_view_check_rt_host", _two_view_host_error, keys1, keys2, matches12,
                              inliers, K, sigma, R, t)


class Sim3ProblemStruct(C.Structure):  # orbm_sim3_problem_t
    _fields_ = [("n1", C.c_int32), ("N", C.c_int32), ("idx1", C.c_void_p), ("Xw1", C.c_void_p), ("Xw2", C.c_void_p), ("sigma2_1", C.c_void_p),
                ("sigma2_2", C.c_void_p), ("Tcw1", C.c_void_p), ("Tcw2", C.c_void_p), ("cam_type1", C.c_int32), ("cam_type2", C.c_int32),
                ("cam_params1", C.c_void_p), ("cam_params2", C.c_void_p), ("fix_scale", C.c_int32), ("min_inliers", C.c_int32),
                ("iterations_done", C.c_int32), ("max_iterations", C.c_int32)]


class Sim3ResultStruct(C.Structure):  # orbm_sim3_result_t
    _fields_ = [(k, C.c_int32) for k in ("converged", "it_stop", "best_it", "best_inliers", "improved", "no_more")] + [
        ("T12", C.c_float * 16), ("R12", C.c_float * 9), ("t12", C.c_float * 3), ("s12", C.c_float), ("best_mask", C.c_void_p),
        ("vbInliers", C.c_void_p)]


class Sim3DetailsStruct(C.Structure):  # orbm_sim3_details_t
    _fields_ = [(k, C.c_void_p) for k in ("counts", "T12", "T21", "quat", "masks", "wall_ms")]


class Sim3Result:
    """What one call of Sim3Solver::iterate returns and leaves behind: converged, it_stop, best_it, best_inliers, improved, no_more (ints);
    T12 [4,4], R12 [3,3], t12 [3], s12 of the best of this call (zeros when best_it < 0); best_mask [N]; vbInliers [n1]; and `details`:
    counts [iterations], T12 / T21 [iterations,4,4], quat [iterations,4], masks [iterations,N]; wall_ms [4]: the device form's host clock
    per phase (orbm_sim3_details_t::wall_ms), zeros from the CPU form."""

    def __init__(self, r, best_mask, vbInliers, details, wall_ms):
        self.wall_ms = wall_ms
        for k in ("converged", "it_stop", "best_it", "best_inliers", "improved", "no_more"):
            setattr(self, k, int(getattr(r, k)))
        self.T12 = np.array(r.T12, np.float32).reshape(4, 4)
        self.R12 = np.array(r.R12, np.float32).reshape(3, 3)
        self.t12 = np.array(r.t12, np.float32)
        self.s12 = np.float32(r.s12)
        self.best_mask, self.vbInliers, self.details = best_mask, vbInliers, details

    def __bool__(self):
        return bool(self.converged)


def _sim3_problem(prob):
    """orbm_sim3_problem_t from a dict (n1, idx1, Xw1, Xw2, sigma2_1, sigma2_2, Tcw1, Tcw2, cam_type1, cam_type2, cam_params1, cam_params2,
    fix_scale, min_inliers and optionally iterations_done = 0, max_iterations = 300).  Returns (struct, N, n1, the arrays it points into)."""
    keep = dict(idx1=np.ascontiguousarray(prob["idx1"], dtype=np.int32).reshape(-1))
    N = len(keep["idx1"])
    for k, w in (("Xw1", 3), ("Xw2", 3), ("sigma2_1", 1), ("sigma2_2", 1)):
        keep[k] = np.ascontiguousarray(prob[k], dtype=np.float32).reshape(-1)
        if keep[k].size != w * N:
            raise ValueError("%s has %d entries per pair" % (k, w))
    for k in ("Tcw1", "Tcw2"):
        keep[k] = np.ascontiguousarray(prob[k], dtype=np.float32).reshape(-1)
        if keep[k].size != 16:
            raise ValueError("%s is a 4 x 4 pose" % k)
    for k, t in (("cam_params1", "cam_type1"), ("cam_params2", "cam_type2")):
        keep[k] = np.zeros(8, np.float32)
        v = np.asarray(prob[k], dtype=np.float32).reshape(-1)
        keep[k][:min(len(v), 8)] = v[:8]
    P = Sim3ProblemStruct()
    P.n1, P.N = int(prob["n1"]), N
    for k, a in keep.items():
        setattr(P, k, a.ctypes.data if a.size else None)
    P.cam_type1, P.cam_type2 = int(prob["cam_type1"]), int(prob["cam_type2"])
    P.fix_scale, P.min_inliers = int(bool(prob["fix_scale"])), int(prob["min_inliers"])
    P.iterations_done, P.max_iterations = int(prob.get("iterations_done", 0)), int(prob.get("max_iterations", 300))
    return P, N, max(int(prob["n1"]), 0), keep


def _sim3_sets(sets, iterations):
    sets = np.ascontiguousarray(sets, dtype=np.int32)
    if sets.size != 3 * max(int(iterations), 0):
        raise ValueError("sets is [iterations][3]")
    return sets


def _sim3_rc(rc, what, error):
    if rc == E_ARG:
        raise ValueError("%s: bad argument (%s)" % (what, error()))
    if rc < 0:
        raise OrbError("%s rc=%d (%s)" % (what, rc, error()))


def _sim3_solve(call, what, error, prob, sets, best_inliers_in):
    P, N, n1, keep = _sim3_problem(prob)
    sets = np.asarray(sets, dtype=np.int32)
    iterations = sets.size // 3
    sets = _sim3_sets(sets, iterations)
    I = max(iterations, 1)
    best_mask, vb = np.zeros(max(N, 1), np.uint8), np.zeros(max(n1, 1), np.uint8)
    d = dict(counts=np.zeros(I, np.int32), T12=np.zeros((I, 4, 4), np.float32), T21=np.zeros((I, 4, 4), np.float32),
             quat=np.zeros((I, 4), np.float32), masks=np.zeros((I, max(N, 1)), np.uint8))
    wall_ms = np.zeros(4, np.float64)
    ds = Sim3DetailsStruct()
    for k, a in d.items():
        setattr(ds, k, a.ctypes.data)
    ds.wall_ms = wall_ms.ctypes.data
    r = Sim3ResultStruct()
    r.best_mask, r.vbInliers = best_mask.ctypes.data, vb.ctypes.data
    _sim3_rc(call(C.byref(P), iterations, _p(sets), int(best_inliers_in), C.byref(r), C.byref(ds)), what, error)
    d["masks"] = d["masks"].reshape(-1)[:I * N].reshape(I, N)
    return Sim3Result(r, best_mask[:N], vb[:n1], d, wall_ms)


def _sim3_hypotheses(call, what, error, prob, sets):
    P, N, n1, keep = _sim3_problem(prob)
    sets = np.asarray(sets, dtype=np.int32)
    iterations = sets.size // 3
    sets = _sim3_sets(sets, iterations)
    I = max(iterations, 1)
    T12, T21, quat = np.zeros((I, 4, 4), np.float32), np.zeros((I, 4, 4), np.float32), np.zeros((I, 4), np.float32)
    _sim3_rc(call(C.byref(P), iterations, _p(sets), _p(T12), _p(T21), _p(quat)), what, error)
    return dict(T12=T12, T21=T21, quat=quat)


def _sim3_check(call, what, error, prob, T12, T21):
    P, N, n1, keep = _sim3_problem(prob)
    T12, T21 = np.ascontiguousarray(T12, dtype=np.float32).reshape(-1, 16), np.ascontiguousarray(T21, dtype=np.float32).reshape(-1, 16)
    if len(T12) != len(T21):
        raise ValueError("T12, T21 [nhyp][16]")
    nhyp = len(T12)
    H = max(nhyp, 1)
    counts, masks = np.zeros(H, np.int32), np.zeros((H, max(N, 1)), np.uint8)
    _sim3_rc(call(C.byref(P), nhyp, _p(T12), _p(T21), _p(counts), _p(masks)), what, error)
    return dict(counts=counts[:nhyp], masks=masks.reshape(-1)[:nhyp * N].reshape(nhyp, N))


def _sim3_host_error():
    return load().orbm_sim3_host_error().decode()


def sim3_solve_host(prob, sets, best_inliers_in=0):
    """One call of Sim3Solver::iterate (Sim3Solver.cc:176-321) behind the constructor, on the CPU with the kernels' own statement
    (orbm_sim3_solve_host, csrc/orb_ref_sim3.h).  Same arguments and result as ORBmatcher.Sim3Solve; for tests without a GPU, not a
    fallback of it."""
    return _sim3_solve(load().orbm_sim3_solve_host, "orbm_sim3_solve_host", _sim3_host_error, prob, sets, best_inliers_in)


def sim3_hypotheses_host(prob, sets):
    """orbm_sim3_hypotheses_host: ComputeSim3 for every set, on the CPU: T12, T21 [iterations,4,4], quat [iterations,4]."""
    return _sim3_hypotheses(load().orbm_sim3_hypotheses_host, "orbm_sim3_hypotheses_host", _sim3_host_error, prob, sets)


def sim3_check_host(prob, T12, T21):
    """orbm_sim3_check_host: CheckInliers for the caller's transforms, on the CPU: counts [nhyp], masks [nhyp,N]."""
    return _sim3_check(load().orbm_sim3_check_host, "orbm_sim3_check_host", _sim3_host_error, prob, T12, T21)


def sim3_ransac_iterations(probability, min_inliers, max_its, N):
    """Sim3Solver::SetRansacParameters (Sim3Solver.cc:150-174): the value left in mRansacMaxIts (orbm_sim3_ransac_iterations)."""
    return int(load().orbm_sim3_ransac_iterations(float(probability), int(min_inliers), int(max_its), int(N)))


def sim3_draw_sets(N, iterations, rand):
    """The minimal sets of `iterations` iterations of Sim3Solver::iterate (Sim3Solver.cc:199-213) as [iterations][3] int32: per iteration
    three times DUtils::Random::RandomInt(0, size - 1) of the shrinking index vector, the drawn entry replaced by the last.  rand: a
    callable returning the next value of libc rand(); RandomInt(min, max) is int(((double)rand() / ((double)RAND_MAX + 1.0)) * (max - min + 1)) + min
    (Random.cpp:47-50)."""
    if N < 3:
        raise ValueError("the draw needs three pairs")
    sets = np.zeros((iterations, 3), np.int32)
    for it in range(iterations):
        avail = list(range(N))
        for j in range(3):
            randi = int((float(rand()) / 2147483648.0) * len(avail))
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


class FuseTargetStruct(C.Structure):  # orbm_fuse_target_t
    _fields_ = [("kf", FrameStruct), ("scale_factors", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("nlevels", C.c_int32),
                ("log_scale_factor", C.c_float), ("Tcw", C.c_void_p), ("Ow", C.c_void_p), ("cam_type", C.c_int32), ("cam_params", C.c_void_p),
                ("bf", C.c_float)]


class FuseSim3TargetStruct(C.Structure):  # orbm_fuse_sim3_target_t
    _fields_ = [("kf", FrameStruct), ("scale_factors", C.c_void_p), ("nlevels", C.c_int32), ("log_scale_factor", C.c_float),
                ("Scw", C.c_void_p), ("cam_type", C.c_int32), ("cam_params", C.c_void_p)]


class KeyFrameStruct(C.Structure):  # orbm_keyframe_t
    _fields_ = [("n", C.c_int32), ("keys_un", C.c_void_p), ("descriptors", C.c_void_p), ("u_right", C.c_void_p),
                ("has_mappoint", C.c_void_p), ("n_nodes", C.c_int32), ("node_id", C.c_void_p), ("node_start", C.c_void_p),
                ("node_idx", C.c_void_p), ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p), ("nlevels", C.c_int32)]


class KeyFrameGeometryStruct(C.Structure):  # orbm_keyframe_geometry_t
    _fields_ = [("Tcw", C.c_void_p), ("Ow", C.c_void_p), ("Tcw_right", C.c_void_p), ("Ow_right", C.c_void_p), ("Twc", C.c_void_p)] + \
               [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")] + [("depth", C.c_void_p), ("keys", C.c_void_p)]


# ORBM_NP_* of include/orbhip.h: the outcome of the body of LocalMapping::CreateNewMapPoints' loop for one pair
(NP_NO_MATCH, NP_ACCEPTED, NP_LOW_PARALLAX, NP_ZERO_W, NP_EMPTY_STEREO, NP_BEHIND1, NP_BEHIND2, NP_REPROJ1, NP_REPROJ1_STEREO, NP_REPROJ2,
 NP_REPROJ2_STEREO, NP_ZERO_DIST, NP_FAR, NP_SCALE, NP_NSTATUS) = range(15)
NEW_POINT_DTYPE = np.dtype([("neighbour", "<i4"), ("idx1", "<i4"), ("idx2", "<i4"), ("x3D", "<f4", (3,))])          # orbm_new_point_t
NP_CAMERA_DTYPE = np.dtype([("Tcw", "<f4", (2, 12)), ("Ow", "<f4", (2, 3)), ("Twc", "<f4", (12,)), ("cam", "<f4", (2, 8))] +
                           [(k, "<f4") for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")] +
                           [("sf", "<f4", (16,)), ("sigma2", "<f4", (16,)), ("cam_type", "<i4"), ("n_left", "<i4")])     # orbm_new_point_camera_t
NP_OBS_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4"), ("u_right", "<f4"), ("depth", "<f4"), ("key_x", "<f4"), ("key_y", "<f4"),
                         ("right", "<i4")])                                                                           # orbm_new_point_obs_t


class LastFrameStruct(C.Structure):  # orbm_last_frame_t
    _fields_ = [("n", C.c_int32), ("has_mp", C.c_void_p), ("Xw", C.c_void_p), ("mpdesc", C.c_void_p), ("last_keys", C.c_void_p),
                ("obs", C.c_void_p), ("Tcw", C.c_void_p), ("Tlw", C.c_void_p)]


class LocalMapStruct(C.Structure):  # orbm_local_map_t
    _fields_ = [("n", C.c_int32), ("eligible", C.c_void_p), ("Xw", C.c_void_p), ("normal", C.c_void_p), ("max_dist", C.c_void_p),
                ("min_dist", C.c_void_p), ("mpdesc", C.c_void_p), ("obs", C.c_void_p), ("Tcw", C.c_void_p)]


class TrackStruct(C.Structure):  # orbm_track_t
    _fields_ = [("in_view", C.c_void_p), ("proj_x", C.c_void_p), ("proj_y", C.c_void_p), ("proj_xr", C.c_void_p), ("depth", C.c_void_p),
                ("view_cos", C.c_void_p), ("level", C.c_void_p)]


class TrackRigStruct(C.Structure):  # orbm_track_rig_t
    _fields_ = [(k, C.c_void_p) for k in ("in_view", "in_view_r", "proj_x", "proj_y", "depth", "view_cos", "proj_xr", "proj_yr", "depth_r",
                                          "view_cos_r", "level", "level_r")]


TRACK_RIG_FIELDS = (("in_view", np.uint8), ("in_view_r", np.uint8), ("proj_x", np.float32), ("proj_y", np.float32), ("depth", np.float32),
                    ("view_cos", np.float32), ("proj_xr", np.float32), ("proj_yr", np.float32), ("depth_r", np.float32),
                    ("view_cos_r", np.float32), ("level", np.int32), ("level_r", np.int32))


class QueryStruct(C.Structure):  # orbm_queries_t
    _fields_ = [("nq", C.c_int32), ("descriptors", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p),
                ("radius", C.c_void_p), ("min_level", C.c_void_p), ("max_level", C.c_void_p), ("u_r", C.c_void_p),
                ("flags", C.c_void_p)]


PAIR_PRED = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int)   # orbm_pair_predicate_t

_lib = None


def load(build_if_needed=True):
    """dlopen liborbhip.so (building it first when the sources are newer).  Raises if that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  Two HIP
    # runtimes in one process cannot both own the device, so when torch is installed it is imported FIRST: the
    # loader then resolves liborbhip.so's NEEDED libamdhip64.so.7 to the copy torch already mapped, and torch
    # tensors, streams and liborbhip kernels share one runtime.  Without torch the system ROCm runtime is used.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if build_if_needed and os.path.exists("/opt/rocm/bin/hipcc") and "ORBHIP_LIB" not in os.environ:
        _build.build()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("liborbhip.so is not built (run __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    L.orbx_create.restype = vp
    L.orbx_create.argtypes = [i32, f32, i32, i32, i32, i32]
    L.orbx_destroy.argtypes = [vp]
    L.orbx_last_error.restype = C.c_char_p
    L.orbx_last_error.argtypes = [vp]
    L.orbx_get_levels.argtypes = [vp]
    L.orbx_get_scale_factor.restype = f32
    L.orbx_get_scale_factor.argtypes = [vp]
    L.orbx_get_scale_tables.argtypes = [vp, vp, vp, vp, vp]
    L.orbx_get_features_per_level.argtypes = [vp, vp]
    L.orbx_configure.argtypes = [vp, i32, i32, i32]
    L.orbx_max_keypoints.argtypes = [vp]
    L.orbx_extract.argtypes = [vp, vp, i32, i32, sz, i32, i32, vp, vp, i32, vp]
    L.orbx_extract_batch_device.argtypes = [vp, vp, i32, i32, sz, sz, i32, i32, i32, vp, vp, vp, i32, vp]
    L.orbx_get_host_us.argtypes = [vp, vp, i32]
    L.orbx_level_info.argtypes = [vp, i32, vp, vp]
    L.orbx_download_level.argtypes = [vp, i32, i32, i32, vp, sz]
    L.orbx_download_pyramid.argtypes = [vp, i32, i32, vp, sz, vp, vp]
    L.orbx_download_blurred_level.argtypes = [vp, i32, i32, vp, sz]
    L.orbx_download_candidates.argtypes = [vp, i32, i32, vp, i32]
    L.orbx_download_level_keypoints.argtypes = [vp, i32, i32, vp, i32]
    L.orbx_set_profiling.argtypes = [vp, i32]
    L.orbx_get_stage_ms.argtypes = [vp, vp, i32]
    L.orbx_compute_stereo_matches.argtypes = [vp, i32, vp, i32, i32, vp, vp, i32, vp, vp, f32, f32, vp, vp]
    L.orbx_compute_stereo_matches_batch_device.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, f32, f32, vp, vp, vp, vp]
    L.orbx_stereo_from_rgbd_batch_device.argtypes = [i32, vp, vp, vp, i32, i32, vp, i32, i32, i32, sz, sz, f32, f32, vp, vp, vp, vp]
    L.orbx_close_points_batch_device.argtypes = [i32, vp, vp, i32, i32, f32, i32, vp, vp, vp, vp, vp, f32, f32, f32, f32, vp, vp, vp, vp]
    L.orbx_cvt_color_gray.argtypes = [vp, vp, i32, i32, sz, i32, i32, vp, sz]
    L.orbx_cvt_color_gray_device.argtypes = [vp, i32, i32, sz, i32, i32, vp, sz, vp]
    L.orbx_clahe.argtypes = [vp, vp, i32, i32, sz, C.c_double, i32, i32, vp, sz]
    L.orbx_clahe_device.argtypes = [vp, i32, i32, sz, C.c_double, i32, i32, vp, vp, sz, vp]
    L.orbx_remap_linear.argtypes = [vp, vp, i32, i32, sz, vp, vp, i32, i32, vp, sz]
    L.orbx_remap_linear_device.argtypes = [vp, i32, i32, sz, vp, vp, sz, i32, i32, vp, sz, vp]
    L.orbx_clahe_batch_device.argtypes = [i32, vp, i32, i32, sz, sz, C.c_double, i32, i32, vp, vp, sz, sz, vp]
    L.orbx_remap_linear_batch_device.argtypes = [i32, vp, i32, i32, sz, sz, vp, vp, sz, i32, i32, vp, sz, sz, vp]
    L.orbx_clahe_band_lut_rows.argtypes = [i32, i32, i32, i32, vp, vp]
    L.orbx_ref_cosf.restype = f32
    L.orbx_ref_cosf.argtypes = [f32]
    L.orbx_ref_sinf.restype = f32
    L.orbx_ref_sinf.argtypes = [f32]
    L.orbx_ref_atanf.restype = f32
    L.orbx_ref_atanf.argtypes = [f32]
    L.orbx_ref_atan2f.restype = f32
    L.orbx_ref_atan2f.argtypes = [f32, f32]
    L.orbx_ref_logf.restype = f32
    L.orbx_ref_logf.argtypes = [f32]
    L.orbx_logf_device.argtypes = [vp, i32, vp, vp]
    L.orbx_ref_tanf.restype = f32
    L.orbx_ref_tanf.argtypes = [f32]
    L.orbx_tanf_device.argtypes = [vp, i32, vp, vp]
    L.orbx_cosf_device.argtypes = L.orbx_sinf_device.argtypes = L.orbx_atanf_device.argtypes = [vp, i32, vp, vp]
    L.orbx_atan2f_device.argtypes = L.orbx_fast_atan2_device.argtypes = [vp, vp, i32, vp, vp]
    L.orbm_create.restype = vp
    L.orbm_create.argtypes = [i32]
    L.orbm_destroy.argtypes = [vp]
    L.orbm_last_error.restype = C.c_char_p
    L.orbm_last_error.argtypes = [vp]
    L.orbm_descriptor_distance.argtypes = [vp, vp]
    L.orbm_search_by_projection.argtypes = [vp, vp, vp, f32, i32, i32, vp, vp, vp, vp]
    L.orbm_search_by_projection_batch_device.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, i32, i32, f32, i32, i32,
                                                         vp, vp, vp, vp, vp, vp]
    L.orbm_search_by_projection_fisheye.argtypes = [vp, vp, i32, vp, vp, vp, f32, i32, vp, vp, vp, vp]
    L.orbm_search_by_projection_last_frame_fisheye.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, f32, f32,
                                                               i32, i32, vp, vp]
    L.orbm_search_by_projection_last_frame_fisheye_batch_device.argtypes = [vp, vp, i32, vp, i32, vp, i32, i32, vp, i32, vp, i32, i32, vp, i32, vp, i32,
                                                                            vp, f32, f32, i32, i32, vp, vp, vp, vp, vp]
    L.orbm_rig_concat_batch_device.argtypes = [i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.orbm_unproject.argtypes = [vp, i32, vp, vp]
    L.orbm_fisheye_ratio_test.argtypes = [i32, i32]
    L.orbm_fisheye_triangulate.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_fisheye_triangulate_device.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_stereo_fisheye_matches_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.orbm_stereo_fisheye_matches.argtypes = [vp, vp, vp, i32, i32, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_search_for_initialization.argtypes = [vp, vp, vp, vp, i32, f32, i32, vp]
    L.orbm_fuse.argtypes = [vp, vp, vp, vp, i32, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, f32, f32, vp, vp]
    L.orbm_fuse_keyframes.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp]
    L.orbm_fuse_sim3_keyframes.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp]
    L.orbm_fuse_sim3.argtypes = [vp, vp, vp, i32, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp]
    L.orbm_fuse_sim3_cam.argtypes = [vp, vp, vp, i32, f32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, f32, vp, vp]
    L.orbm_search_by_projection_sim3_cam.argtypes = [vp, vp, vp, i32, f32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, f32, vp, vp]
    L.orbm_search_by_sim3.argtypes = [vp] + [vp, vp, i32, f32, vp, vp, vp, vp, vp, vp, vp] * 2 + [f32, vp, vp, vp, f32, vp]
    L.orbm_distinctive_descriptors.argtypes = [vp, i32, vp, vp, vp]
    L.orbm_update_map_points.argtypes = [vp, vp, vp, vp, vp, vp]
    L.orbm_map_point_normal_depth.argtypes = [i32, vp, vp, vp, f32, f32, vp, vp, vp]
    L.orbm_keyframe_culling.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_keyframe_culling_open.argtypes = [vp, vp]
    L.orbm_keyframe_culling_step.argtypes = [vp, i32, vp, vp, vp]
    L.orbm_keyframe_culling_host.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.orbm_keyframe_culling_host_error.argtypes = []
    L.orbm_keyframe_culling_host_error.restype = C.c_char_p
    L.orbm_update_local_map.argtypes = [vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_update_local_map_device.argtypes = [vp, vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_update_local_map_host.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_update_local_map_host_error.argtypes = []
    L.orbm_update_local_map_host_error.restype = C.c_char_p
    L.orbm_update_connections.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_update_connections_host.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_gather_local_map_device.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    tv = [vp, i32, vp, i32, vp]   # keys1, n1, keys2, n2, matches12
    L.orbm_two_view_reconstruct.argtypes = [vp] + tv + [vp, f32, i32, vp, vp, vp, vp, vp, vp]
    L.orbm_two_view_reconstruct_host.argtypes = tv + [vp, f32, i32, vp, vp, vp, vp, vp, vp]
    L.orbm_two_view_host_error.argtypes = []
    L.orbm_two_view_host_error.restype = C.c_char_p
    L.orbm_two_view_models.argtypes = [vp] + tv + [f32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_two_view_models_host.argtypes = tv + [f32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_two_view_check_rt.argtypes = [vp] + tv + [vp, vp, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_two_view_check_rt_host.argtypes = tv + [vp, vp, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbm_sim3_solve.argtypes = [vp, vp, i32, vp, i32, vp, vp]
    L.orbm_sim3_solve_host.argtypes = [vp, i32, vp, i32, vp, vp]
    L.orbm_sim3_host_error.argtypes = []
    L.orbm_sim3_host_error.restype = C.c_char_p
    L.orbm_sim3_hypotheses.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.orbm_sim3_hypotheses_host.argtypes = [vp, i32, vp, vp, vp, vp]
    L.orbm_sim3_check.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.orbm_sim3_check_host.argtypes = [vp, i32, vp, vp, vp, vp]
    L.orbm_sim3_ransac_iterations.argtypes = [C.c_double, i32, i32, i32]
    L.orbm_knn_match2.argtypes = [vp, vp, i32, vp, i32, vp, vp]
    L.orbm_search_by_bow.argtypes = [vp, vp, vp, f32, i32, vp]
    L.orbm_search_by_bow_fisheye.argtypes = [vp, vp, vp, i32, f32, i32, vp]
    L.orbm_search_by_bow_keyframes.argtypes = [vp, vp, vp, f32, i32, vp]
    L.orbm_search_by_bow_candidates.argtypes = [vp, i32, vp, vp, i32, vp, f32, i32, vp, vp]
    L.orbm_search_by_bow_keyframes_candidates.argtypes = [vp, vp, i32, vp, vp, f32, i32, vp, vp]
    L.orbm_hamming_matrix.argtypes = [vp, vp, i32, vp, i32, vp]
    L.orbm_search_for_triangulation.argtypes = [vp] * 10 + [i32, i32, i32, vp]
    L.orbm_triangulation_candidates.argtypes = [vp, vp, vp, f32, f32, i32, i32, vp, vp, vp, i32]
    L.orbm_search_for_triangulation_pred.argtypes = [vp, vp, vp, f32, f32, i32, i32, i32, i32, PAIR_PRED, vp, vp]
    L.orbm_search_for_triangulation_kb8.argtypes = [vp, vp, i32, vp, i32, f32, f32, vp, vp, vp, i32, i32, i32, vp]
    L.orbm_search_for_triangulation_neighbours.argtypes = [vp, vp, i32] + [vp] * 9 + [i32, i32, vp, vp]
    L.orbm_search_for_triangulation_kb8_neighbours.argtypes = [vp, vp, i32, i32] + [vp] * 7 + [i32, i32, vp, vp]
    L.orbm_new_point_geometry.argtypes = [i32, vp, vp, vp, vp, f32, i32, f32, vp, vp]
    L.orbm_new_point_geometry_device.argtypes = [i32, vp, vp, vp, vp, f32, i32, f32, vp, vp, vp]
    L.orbm_create_new_map_points.argtypes = [vp, vp, vp, f32, i32, vp, vp] + [vp] * 8 + [i32, i32, f32, vp, i32, vp, vp, vp]
    L.orbm_create_new_map_points_kb8.argtypes = [vp, vp, vp, f32, i32, i32, vp, vp] + [vp] * 6 + [i32, i32, f32, vp, i32, vp, vp, vp]
    L.orbm_search_by_projection_sim3.argtypes = [vp, vp, vp, i32, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, vp, vp]
    L.orbm_search_by_projection_keyframe.argtypes = [vp, vp, vp, i32, f32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, f32, i32, i32, vp, vp]
    L.orbm_search_by_projection_last_frame.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, f32, f32, f32,
                                                       i32, i32, vp, vp]
    L.orbm_search_by_projection_last_frame_batch_device.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, i32, i32, vp, i32, i32, vp, f32, f32, f32,
                                                                    i32, i32, vp, vp, vp, vp, vp]
    L.orbm_search_local_points.argtypes = [vp, vp, vp, i32, f32, vp, i32, vp, f32, f32, f32, i32, f32, f32, vp, vp, vp, vp]
    L.orbm_search_local_points_batch_device.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, i32, i32, vp, i32, f32, i32, vp, f32, f32, f32,
                                                        i32, f32, f32, vp, vp, vp, vp, vp, vp]
    L.orbm_search_local_points_fisheye.argtypes = [vp, vp, i32, vp, vp, vp, i32, f32, vp, vp, vp, i32, vp, i32, vp, f32, f32, i32, f32, f32,
                                                   vp, vp, vp, vp]
    L.orbm_search_local_points_fisheye_batch_device.argtypes = [vp, vp, i32, vp, i32, vp, i32, i32, vp, vp, vp, i32, vp, i32, i32, vp, i32, f32,
                                                                vp, vp, i32, vp, i32, vp, f32, f32, i32, f32, f32, vp, vp, vp, vp, vp, vp]
    L.orbm_rig_right_camera.restype = None
    L.orbm_rig_right_camera.argtypes = [vp, vp, vp, vp, vp]
    L.orbm_three_maxima.argtypes = [vp, i32, vp, vp, vp]
    L.orbm_radius_by_viewing_cos.restype = f32
    L.orbm_radius_by_viewing_cos.argtypes = [f32]
    L.orbm_project.argtypes = [i32, vp, f32, f32, f32, vp, vp]
    L.orbm_undistort_keypoints.argtypes = [i32, vp, vp, vp, i32, vp]
    L.orbm_image_bounds.argtypes = [i32, i32, vp, vp, i32, vp, vp, vp, vp]
    L.orbm_undistort_keypoints_batch_device.argtypes = [vp, vp, i32, vp, i32, i32, i32, vp, vp, i32, vp, vp]
    L.orbm_set_profiling.argtypes = [vp, i32]
    L.orbm_set_scan_mode.argtypes = [vp, i32]
    L.orbm_set_scan_mode.restype = i32
    L.orbm_set_hamming_engine.argtypes = [vp, i32]
    L.orbm_set_hamming_engine.restype = i32
    L.orbm_get_last_ms.restype = f32
    L.orbm_get_last_ms.argtypes = [vp]
    L.orbm_get_stage_ms.argtypes = [vp, vp, i32]
    L.orbv_create.restype = vp
    L.orbv_create.argtypes = [vp, i32]
    L.orbv_destroy.restype = None
    L.orbv_destroy.argtypes = [vp]
    L.orbv_last_error.restype = C.c_char_p
    L.orbv_last_error.argtypes = [vp]
    for name in ("orbv_n_nodes", "orbv_n_words", "orbv_max_children", "orbv_min_leaf_level"):
        getattr(L, name).argtypes = [vp]
    L.orbv_transform_host.argtypes = [vp, vp, i32, i32] + [vp] * 9
    L.orbv_transform.argtypes = [vp, vp, i32, i32] + [vp] * 9
    L.orbv_batch_scratch_bytes.restype = sz
    L.orbv_batch_scratch_bytes.argtypes = [i32, i32]
    L.orbv_transform_batch_device.argtypes = [vp, vp, i32, i32, vp, i32, i32] + [vp] * 11
    L.orbv_transform_batch_device_form.argtypes = [vp, i32, vp, i32, i32, vp, i32, i32] + [vp] * 11
    u64 = C.c_uint64
    L.orbd_create.restype = vp
    L.orbd_create.argtypes = [i32, i32, i32, i32]
    L.orbd_create_for_vocabulary.restype = vp
    L.orbd_create_for_vocabulary.argtypes = [vp, i32, i32]
    L.orbd_destroy.restype = None
    L.orbd_destroy.argtypes = [vp]
    L.orbd_last_error.restype = C.c_char_p
    L.orbd_last_error.argtypes = [vp]
    for name in ("orbd_n_words", "orbd_capacity", "orbd_size", "orbd_clear"):
        getattr(L, name).argtypes = [vp]
    L.orbd_add.argtypes = [vp, u64, u64, vp, vp, i32, vp]
    L.orbd_add_device.argtypes = [vp, u64, u64, vp, vp, vp, i32, i32, vp, vp]
    L.orbd_erase.argtypes = [vp, u64]
    L.orbd_clear_map.argtypes = [vp, u64]
    L.orbd_set_map.argtypes = [vp, u64, u64]
    L.orbd_get_members.argtypes = [vp, u64, vp]
    for name in ("orbd_query_reloc", "orbd_query_reloc_host"):
        getattr(L, name).argtypes = [vp, u64, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]
    for name in ("orbd_query_place", "orbd_query_place_host"):
        getattr(L, name).argtypes = [vp, u64, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]
    L.orbd_batch_scratch_bytes.restype = sz
    L.orbd_batch_scratch_bytes.argtypes = [vp, i32]
    L.orbd_score_batch_device.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp]
    L.orbd_accumulate_reloc.argtypes = [vp, u64, u64, vp, vp, i32, vp, vp, vp]
    L.orbd_accumulate_place.argtypes = [vp, u64, vp, vp, i32, vp, vp, vp]
    _lib = L
    return L


def _p(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    return a.ctypes.data_as(C.c_void_p)


class OrbError(RuntimeError):
    pass


class ORBextractor:
    """ORB_SLAM3::ORBextractor (ORBextractor.h:43-109) on one MI355X.

    __call__(image, mask, vLappingArea) mirrors operator() (ORBextractor.cc:1071-1184) and returns
    (monoIndex, keypoints[KP_DTYPE], descriptors[n,32])."""

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device=0):
        self.L = load()
        self.h = self.L.orbx_create(int(nfeatures), C.c_float(scaleFactor), int(nlevels), int(iniThFAST), int(minThFAST), int(device))
        if not self.h:
            raise OrbError("orbx_create failed: no usable HIP device %d or bad parameters (no CPU fallback)" % device)
        self.nlevels = int(nlevels)
        self.nfeatures = int(nfeatures)
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.L.orbx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc == E_HIP:
            raise OrbError("%s: %s" % (what, self.L.orbx_last_error(self.h).decode()))
        if rc == E_ARG:
            raise ValueError("%s: bad argument (%s)" % (what, self.L.orbx_last_error(self.h).decode()))
        return rc

    # --- getters, ORBextractor.h:61-81 ---
    def GetLevels(self):
        return self.L.orbx_get_levels(self.h)

    def GetScaleFactor(self):
        return float(self.L.orbx_get_scale_factor(self.h))

    def _tables(self):
        t = [np.zeros(self.nlevels, dtype=np.float32) for _ in range(4)]
        self.L.orbx_get_scale_tables(self.h, *[_p(a) for a in t])
        return t

    def GetScaleFactors(self):
        return self._tables()[0]

    def GetInverseScaleFactors(self):
        return self._tables()[1]

    def GetScaleSigmaSquares(self):
        return self._tables()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._tables()[3]

    def features_per_level(self):
        a = np.zeros(self.nlevels, dtype=np.int32)
        self.L.orbx_get_features_per_level(self.h, _p(a))
        return a.tolist()

    def configure(self, rows, cols, max_batch=1):
        return self._check(self.L.orbx_configure(self.h, int(rows), int(cols), int(max_batch)), "orbx_configure")

    def max_keypoints(self):
        return self.L.orbx_max_keypoints(self.h)

    def __call__(self, image, mask=None, vLappingArea=(0, 1000)):
        if image is None or image.size == 0:
            return -1, np.zeros(0, dtype=KP_DTYPE), np.zeros((0, 32), dtype=np.uint8)  # ORBextractor.cc:1075-1076
        if image.dtype != np.uint8 or image.ndim != 2:
            raise ValueError("image must be CV_8UC1 (ORBextractor.cc:1080)")
        if image.strides[1] != 1:
            image = np.ascontiguousarray(image)
        rows, cols = image.shape
        cap = self.configure(rows, cols, 1)
        kps = np.zeros(cap, dtype=KP_DTYPE)
        desc = np.zeros((cap, 32), dtype=np.uint8)
        n = C.c_int(0)
        # the C call alone (what a C++ caller of the adapter pays), for tools/run_sequence.py.  The argument objects are made BEFORE the
        # clock starts: an allocation inside the timed region can start CPython's full garbage collection, which takes ~40 ms once a
        # large package such as PyTorch is imported - that was the "36 ms stall" of round 2's sequence runs (tools/stall_probe.py)
        args = (self.h, _p(image), rows, cols, C.c_size_t(image.strides[0]), int(vLappingArea[0]), int(vLappingArea[1]), _p(kps), _p(desc), cap, C.byref(n))
        t0 = time.perf_counter()
        rc = self.L.orbx_extract(*args)
        self.last_call_s = time.perf_counter() - t0
        if rc == E_EMPTY:
            return -1, kps[:0], desc[:0]
        if rc == E_CAP:
            raise OrbError("keypoint capacity bound violated: %d > %d" % (n.value, cap))
        self._check(rc, "orbx_extract")
        return rc, kps[:n.value].copy(), desc[:n.value].copy()

    def cvtColorGray(self, im, rgb=True):
        """cvtColor(im, gray, CV_RGB2GRAY / CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY) of Tracking::GrabImage* (Tracking.cc:1122-1135)."""
        im = np.ascontiguousarray(im, dtype=np.uint8)
        if im.ndim != 3 or im.shape[2] not in (3, 4):
            raise ValueError("expected an H x W x 3|4 uint8 image")
        H, W, ch = im.shape
        out = np.empty((H, W), np.uint8)
        rc = self.L.orbx_cvt_color_gray(self.h, _p(im), H, W, C.c_size_t(W * ch), ch, int(bool(rgb)), _p(out), C.c_size_t(W))
        if rc < 0:
            raise OrbError("orbx_cvt_color_gray rc=%d: %s" % (rc, self.L.orbx_last_error(self.h).decode()))
        return out

    def CLAHE(self, im, clip_limit=3.0, tiles=(8, 8)):
        """cv::createCLAHE(clip_limit, Size(tiles))->apply(im, im) of the TUM-VI examples (mono_tum_vi.cc:101-109)."""
        im = np.ascontiguousarray(im, dtype=np.uint8)
        if im.ndim != 2:
            raise ValueError("expected an H x W uint8 image")
        H, W = im.shape
        out = np.empty((H, W), np.uint8)
        rc = self.L.orbx_clahe(self.h, _p(im), H, W, C.c_size_t(W), C.c_double(clip_limit), int(tiles[0]), int(tiles[1]), _p(out), C.c_size_t(W))
        if rc < 0:
            raise OrbError("orbx_clahe rc=%d: %s" % (rc, self.L.orbx_last_error(self.h).decode()))
        return out

    def remap(self, im, mapx=None, mapy=None, size=None):
        """cv::remap(im, out, M1, M2, INTER_LINEAR) of the stereo examples (stereo_euroc.cc:166-167).  Maps are kept on the device:
        leave them out (and give size=(rows, cols)) to reuse the ones of the previous call."""
        im = np.ascontiguousarray(im, dtype=np.uint8)
        if mapx is not None:
            mapx = np.ascontiguousarray(mapx, dtype=np.float32); mapy = np.ascontiguousarray(mapy, dtype=np.float32)
            if mapx.shape != mapy.shape or mapx.ndim != 2:
                raise ValueError("mapx / mapy must be equal-shaped 2-D float32 arrays")
            size = mapx.shape
        H, W = size
        out = np.empty((H, W), np.uint8)
        rc = self.L.orbx_remap_linear(self.h, _p(im), im.shape[0], im.shape[1], C.c_size_t(im.shape[1]), _p(mapx) if mapx is not None else None,
                                      _p(mapy) if mapy is not None else None, H, W, _p(out), C.c_size_t(W))
        if rc < 0:
            raise OrbError("orbx_remap_linear rc=%d: %s" % (rc, self.L.orbx_last_error(self.h).decode()))
        return out

    def ComputeStereoMatches(self, right, keysL, descL, keysR, descR, mb, mbf, frame_l=0, frame_r=0):
        """Frame::ComputeStereoMatches (Frame.cc:901-1079).  self / right = mpORBextractorLeft / Right after extracting the two
        images (their pyramids are still on the device).  Returns (mvuRight, mvDepth)."""
        keysL, keysR = np.ascontiguousarray(keysL, dtype=KP_DTYPE), np.ascontiguousarray(keysR, dtype=KP_DTYPE)
        descL, descR = np.ascontiguousarray(descL, dtype=np.uint8), np.ascontiguousarray(descR, dtype=np.uint8)
        uR = np.full(len(keysL), -1, dtype=np.float32)
        depth = np.full(len(keysL), -1, dtype=np.float32)
        rc = self.L.orbx_compute_stereo_matches(self.h, int(frame_l), right.h, int(frame_r), len(keysL), _p(keysL), _p(descL), len(keysR),
                                                _p(keysR), _p(descR), C.c_float(mb), C.c_float(mbf), _p(uR), _p(depth))
        if rc < 0:
            raise OrbError("orbx_compute_stereo_matches rc=%d: %s" % (rc, self.L.orbx_last_error(self.h).decode()))
        return uR, depth

    def compute_stereo_matches_batch_device(self, right, nframes, d_keysL, d_descL, d_countsL, d_keysR, d_descR, d_countsR, cap, mb, mbf,
                                            d_uRight, d_depth, d_nstereo=None, stream=None):
        """Frame::ComputeStereoMatches (Frame.cc:901-1079) for the `nframes` pairs of the last two extract_batch_device calls of self
        (left) and right, everything resident: all pointers are device addresses (ints), asynchronous on `stream`.  d_uRight /
        d_depth [nframes][cap] float32 receive mvuRight / mvDepth (entries beyond a frame's left count are left alone), d_nstereo
        [nframes] int32 (optional) the number of stereo matches after the median filter."""
        vp = lambda a: C.c_void_p(a) if a else None
        rc = self.L.orbx_compute_stereo_matches_batch_device(self.h, right.h if right is not None else None, int(nframes), vp(d_keysL), vp(d_descL),
                                                             vp(d_countsL), vp(d_keysR), vp(d_descR), vp(d_countsR), int(cap), C.c_float(mb),
                                                             C.c_float(mbf), vp(d_uRight), vp(d_depth), vp(d_nstereo), vp(stream))
        self._check(rc, "orbx_compute_stereo_matches_batch_device")
        if rc < 0:
            raise OrbError("orbx_compute_stereo_matches_batch_device rc=%d" % rc)
        return rc

    def extract_batch_device(self, d_images, rows, cols, stride, frame_stride, nframes, d_kps, d_desc, d_counts, cap,
                             vLappingArea=(0, 1000), stream=None):
        """All pointers are device addresses (ints).  Asynchronous on `stream` (hipStream_t as int; None/0 = the
        device's default stream, which is also torch's default current stream)."""
        rc = self.L.orbx_extract_batch_device(self.h, C.c_void_p(d_images), int(rows), int(cols), C.c_size_t(stride),
                                              C.c_size_t(frame_stride), int(nframes), int(vLappingArea[0]),
                                              int(vLappingArea[1]), C.c_void_p(d_kps), C.c_void_p(d_desc),
                                              C.c_void_p(d_counts), int(cap), C.c_void_p(stream) if stream else None)
        self._check(rc, "orbx_extract_batch_device")
        if rc < 0:
            raise OrbError("orbx_extract_batch_device rc=%d" % rc)
        return rc

    # --- mvImagePyramid (ORBextractor.h:83) and stage taps ---
    def level_shape(self, level):
        r, c = C.c_int(), C.c_int()
        self._check(self.L.orbx_level_info(self.h, level, C.byref(r), C.byref(c)), "orbx_level_info")
        return r.value, c.value

    def image_pyramid_level(self, level, frame=0, border=0):
        r, c = self.level_shape(level)
        out = np.zeros((r + 2 * border, c + 2 * border), dtype=np.uint8)
        self._check(self.L.orbx_download_level(self.h, frame, level, border, _p(out), C.c_size_t(out.strides[0])), "orbx_download_level")
        return out

    def image_pyramid(self, frame=0, border=0):
        """mvImagePyramid of one frame in one transfer (orbx_download_pyramid): list of per-level arrays incl. the border frame."""
        off = np.zeros(self.nlevels, np.uint64); st = np.zeros(self.nlevels, np.uint64)
        nbytes = self._check(self.L.orbx_download_pyramid(self.h, int(frame), int(border), None, 0, _p(off), _p(st)), "orbx_download_pyramid")
        buf = np.zeros(max(nbytes, 1), np.uint8)
        self._check(self.L.orbx_download_pyramid(self.h, int(frame), int(border), _p(buf), C.c_size_t(buf.size), _p(off), _p(st)), "orbx_download_pyramid")
        out = []
        for l in range(self.nlevels):
            r, c = self.level_shape(l)
            rows, stride = r + 2 * border, int(st[l])
            out.append(buf[int(off[l]):int(off[l]) + rows * stride].reshape(rows, stride)[:, :c + 2 * border])
        return out

    def blurred_level(self, level, frame=0):
        r, c = self.level_shape(level)
        out = np.zeros((r, c), dtype=np.uint8)
        self._check(self.L.orbx_download_blurred_level(self.h, frame, level, _p(out), C.c_size_t(out.strides[0])), "orbx_download_blurred_level")
        return out

    def level_candidates(self, level, frame=0):
        r, c = self.level_shape(level)
        cap = (r * c) // 4 + 64
        out = np.zeros((cap, 3), dtype=np.float32)
        n = self._check(self.L.orbx_download_candidates(self.h, frame, level, _p(out), cap), "orbx_download_candidates")
        return out[:n].copy()

    def level_keypoints(self, level, frame=0):
        cap = self.max_keypoints() + 8
        out = np.zeros((cap, 3), dtype=np.float32)
        n = self._check(self.L.orbx_download_level_keypoints(self.h, frame, level, _p(out), cap), "orbx_download_level_keypoints")
        return out[:n].copy()

    def set_profiling(self, on=True):
        self.L.orbx_set_profiling(self.h, 1 if on else 0)

    def stage_ms(self):
        ms = np.zeros(5, dtype=np.float32)
        n = self.L.orbx_get_stage_ms(self.h, _p(ms), 5)
        return dict(zip(["pyramid", "fast", "octree", "blur", "describe"], ms[:n].tolist()))


class FrameView:
    """The slice of ORB_SLAM3::Frame the projection searches read (Frame.h mvKeysUn, mDescriptors, mvuRight,
    mnMinX..mnMaxY; Frame.cc:872-899), plus mvpMapPoints as (slot, slot_obs) arrays."""

    def __init__(self, keys_un, descriptors, bounds, u_right=None):
        self.keys_un = np.ascontiguousarray(keys_un, dtype=KP_DTYPE)
        self.descriptors = np.ascontiguousarray(descriptors, dtype=np.uint8)
        self.u_right = None if u_right is None else np.ascontiguousarray(u_right, dtype=np.float32)
        self.bounds = tuple(float(b) for b in bounds)  # mnMinX, mnMaxX, mnMinY, mnMaxY
        self.N = len(self.keys_un)
        self.slot = np.full(self.N, -1, dtype=np.int32)     # mvpMapPoints[i] as query id, -1 = NULL
        self.slot_obs = np.zeros(self.N, dtype=np.uint8)    # Observations()>0 of the holder

    def struct(self):
        return FrameStruct(self.N, _p(self.keys_un), _p(self.descriptors), _p(self.u_right), C.c_float(self.bounds[0]),
                           C.c_float(self.bounds[1]), C.c_float(self.bounds[2]), C.c_float(self.bounds[3]))


class KeyFrameView:
    """The slice of ORB_SLAM3::KeyFrame that SearchForTriangulation reads: mvKeysUn, mDescriptors, mvuRight, the map-point
    occupancy, mFeatVec (as {node id: [indices]}), mvScaleFactors, mvLevelSigma2."""

    def __init__(self, keys_un, descriptors, feat_vec, scale_factors, level_sigma2, u_right=None, has_mappoint=None):
        self.keys_un = np.ascontiguousarray(keys_un, dtype=KP_DTYPE)
        self.descriptors = np.ascontiguousarray(descriptors, dtype=np.uint8)
        self.N = len(self.keys_un)
        self.u_right = np.full(self.N, -1, np.float32) if u_right is None else np.ascontiguousarray(u_right, dtype=np.float32)
        self.has_mappoint = np.zeros(self.N, np.uint8) if has_mappoint is None else np.ascontiguousarray(has_mappoint, dtype=np.uint8)
        ids = sorted(feat_vec.keys())                      # std::map iteration order
        self.node_id = np.array(ids, dtype=np.uint32)
        self.node_start = np.zeros(len(ids) + 1, dtype=np.int32)
        idx = []
        for k, nid in enumerate(ids):
            idx.extend(int(i) for i in feat_vec[nid])
            self.node_start[k + 1] = len(idx)
        self.node_idx = np.array(idx, dtype=np.int32) if idx else np.zeros(1, np.int32)
        self.sf = np.ascontiguousarray(scale_factors, dtype=np.float32)
        self.sigma2 = np.ascontiguousarray(level_sigma2, dtype=np.float32)

    def struct(self):
        return KeyFrameStruct(self.N, _p(self.keys_un), _p(self.descriptors), _p(self.u_right), _p(self.has_mappoint), len(self.node_id),
                              _p(self.node_id), _p(self.node_start), _p(self.node_idx), _p(self.sf), _p(self.sigma2), len(self.sf))


class FuseTarget:
    """One target keyframe of ORBmatcher.FuseKeyFrames (orbm_fuse_target_t): what ORBmatcher.Fuse takes of a keyframe.  KF: FrameView of
    the keyframe (for a rig the raw keypoints and descriptor rows of one image); Tcw row-major 4x4, the right camera's for bRight."""

    def __init__(self, KF, scale_factors, inv_level_sigma2, log_scale_factor, Tcw, Ow, cam_type, cam_params, bf):
        a = lambda x: np.ascontiguousarray(x, dtype=np.float32)
        self.KF = KF
        self.sf, self.inv_sigma2 = a(scale_factors), a(inv_level_sigma2)
        self.log_sf = float(log_scale_factor)
        self.Tcw, self.Ow, self.cam = a(Tcw), a(Ow), a(cam_params)
        self.cam_type, self.bf = int(cam_type), float(bf)

    def struct(self):
        return FuseTargetStruct(self.KF.struct(), _p(self.sf), _p(self.inv_sigma2), len(self.sf), C.c_float(self.log_sf), _p(self.Tcw), _p(self.Ow),
                                self.cam_type, _p(self.cam), C.c_float(self.bf))


class FuseSim3Target:
    """One corrected keyframe of ORBmatcher.FuseSim3KeyFrames (orbm_fuse_sim3_target_t): what ORBmatcher.FuseSim3 takes of a keyframe.
    Scw row-major 4x4 Sim3, or the pose for the SearchAndFuse overload that passes GetPose()."""

    def __init__(self, KF, scale_factors, log_scale_factor, Scw, cam_type, cam_params):
        a = lambda x: np.ascontiguousarray(x, dtype=np.float32)
        self.KF = KF
        self.sf = a(scale_factors)
        self.log_sf = float(log_scale_factor)
        self.Scw, self.cam = a(Scw), a(cam_params)
        self.cam_type = int(cam_type)

    def struct(self):
        return FuseSim3TargetStruct(self.KF.struct(), _p(self.sf), len(self.sf), C.c_float(self.log_sf), _p(self.Scw), self.cam_type, _p(self.cam))


class KeyFrameGeometry:
    """What the body of LocalMapping::CreateNewMapPoints' loop reads of a keyframe beyond KeyFrameView (orbm_keyframe_geometry_t):
    Tcw = [Rcw | tcw] (3x4), Ow, for rigs the right camera's Tcw_right / Ow_right, Twc (3x4), the intrinsics fx .. invfy, mb, mbf,
    mvDepth and mvKeys (both only where a keypoint has u_right >= 0)."""

    def __init__(self, Tcw, Ow, fx=0.0, fy=0.0, cx=0.0, cy=0.0, invfx=None, invfy=None, mb=0.0, mbf=0.0, Twc=None, depth=None, keys=None,
                 Tcw_right=None, Ow_right=None):
        f = lambda x, n: None if x is None else np.ascontiguousarray(x, dtype=np.float32).reshape(-1)[:n].copy()
        self.Tcw, self.Ow, self.Tcw_right, self.Ow_right, self.Twc = f(Tcw, 12), f(Ow, 3), f(Tcw_right, 12), f(Ow_right, 3), f(Twc, 12)
        inv = lambda given, f_: given if given is not None else (np.float32(1.0) / np.float32(f_) if f_ else 0.0)   # invfx = 1.0f / fx (Frame.cc:169)
        self.scalars = [np.float32(v) for v in (fx, fy, cx, cy, inv(invfx, fx), inv(invfy, fy), mb, mbf)]
        self.depth = None if depth is None else np.ascontiguousarray(depth, dtype=np.float32)
        self.keys = None if keys is None else np.ascontiguousarray(keys, dtype=KP_DTYPE)

    def struct(self):
        return KeyFrameGeometryStruct(_p(self.Tcw), _p(self.Ow), _p(self.Tcw_right), _p(self.Ow_right), _p(self.Twc), *[float(v) for v in self.scalars],
                                      _p(self.depth), _p(self.keys))


def new_point_camera(KF, G, cam_type, cams, n_left=-1):
    """orbm_new_point_camera_t of keyframe (KF, G): cams = mvParameters of mpCamera [, mpCamera2]."""
    c = np.zeros((), NP_CAMERA_DTYPE)
    cams = np.ascontiguousarray(cams, dtype=np.float32).reshape(-1)
    npar = 4 if cam_type == 0 else 8
    c["Tcw"][0], c["Ow"][0], c["cam"][0][:npar] = G.Tcw, G.Ow, cams[:npar]
    if n_left != -1:
        c["Tcw"][1], c["Ow"][1], c["cam"][1][:npar] = G.Tcw_right, G.Ow_right, cams[8:8 + npar]
    if G.Twc is not None:
        c["Twc"] = G.Twc
    for k, v in zip(("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf"), G.scalars):
        c[k] = v
    c["sf"][:len(KF.sf)], c["sigma2"][:len(KF.sigma2)] = KF.sf, KF.sigma2
    c["cam_type"], c["n_left"] = cam_type, n_left
    return c


def new_point_obs(KF, G, idx, n_left=-1):
    """orbm_new_point_obs_t [len(idx)] of the keypoints idx of keyframe (KF, G) as LocalMapping.cc:613-632 reads them."""
    idx = np.asarray(idx, dtype=np.int64)
    o = np.zeros(len(idx), NP_OBS_DTYPE)
    o["x"], o["y"], o["octave"] = KF.keys_un["x"][idx], KF.keys_un["y"][idx], KF.keys_un["octave"][idx]
    o["u_right"] = -1.0 if n_left != -1 else KF.u_right[idx]
    st = o["u_right"] >= 0
    if st.any():
        o["depth"][st], o["key_x"][st], o["key_y"][st] = G.depth[idx[st]], G.keys["x"][idx[st]], G.keys["y"][idx[st]]
    o["right"] = (idx >= n_left) if n_left != -1 else 0
    return o


def map_point_normal_depth(centre, pos, ref_centre, ref_scale, ref_max_scale):
    """MapPoint::UpdateNormalAndDepth (MapPoint.cc:486-545) for one map point on the host (orbm_map_point_normal_depth): centre [n, 3] the
    camera centres of its entries in the reference's walk order.  Returns (normal [3], min_dist, max_dist); n == 0 writes nothing (NaN)."""
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    centre, pos, ref_centre = f(centre), f(pos), f(ref_centre)
    normal, mn, mx = np.full(3, np.nan, np.float32), np.full(1, np.nan, np.float32), np.full(1, np.nan, np.float32)
    _check_free(load().orbm_map_point_normal_depth(len(centre) // 3, _p(centre), _p(pos), _p(ref_centre), float(ref_scale), float(ref_max_scale),
                                                   _p(normal), _p(mn), _p(mx)), "orbm_map_point_normal_depth")
    return normal, mn[0], mx[0]


def pack_map_points(points):
    """The flat arrays of orbm_map_point_update_t from a list of points, each a mapping with `desc` [n, 32], `centre` [n, 3], `in_desc` [n]
    (one row per entry, in the reference's walk order), `pos` [3], `ref_centre` [3], `ref_scale`, `ref_max_scale`."""
    n = len(points)
    start = np.zeros(n + 1, np.int32)
    for i, pt in enumerate(points):
        start[i + 1] = start[i] + len(pt["desc"])
    cat = lambda k, t, w: np.ascontiguousarray(np.concatenate([np.asarray(pt[k], t).reshape((-1,) + w) for pt in points]) if n else np.zeros((0,) + w, t))
    col = lambda k, w: np.ascontiguousarray(np.array([np.asarray(pt[k], np.float32).reshape(w) for pt in points], np.float32).reshape((n,) + w))
    return dict(start=start, desc=cat("desc", np.uint8, (32,)), centre=cat("centre", np.float32, (3,)), in_desc=cat("in_desc", np.uint8, ()),
                pos=col("pos", (3,)), ref_centre=col("ref_centre", (3,)), ref_scale=col("ref_scale", ()), ref_max_scale=col("ref_max_scale", ()))


def new_point_geometry(c1, c2, obs1, obs2, scale_factor1, far_points=False, th_far_points=0.0):
    """The body of LocalMapping::CreateNewMapPoints' loop (LocalMapping.cc:605-880) for the pairs (obs1[i], obs2[i]) on the host
    (orbm_new_point_geometry): (status [n] of NP_*, x3D [n, 3], zero where the pair is not accepted)."""
    obs1, obs2 = np.ascontiguousarray(obs1, dtype=NP_OBS_DTYPE), np.ascontiguousarray(obs2, dtype=NP_OBS_DTYPE)
    n = len(obs1)
    c1, c2 = np.ascontiguousarray(c1, dtype=NP_CAMERA_DTYPE), np.ascontiguousarray(c2, dtype=NP_CAMERA_DTYPE)
    status, x3 = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 3), np.float32)
    _check_free(load().orbm_new_point_geometry(n, _p(c1), _p(c2), _p(obs1), _p(obs2), float(scale_factor1), int(bool(far_points)), float(th_far_points),
                                               _p(status), _p(x3)), "orbm_new_point_geometry")
    return status[:n], x3[:n]


def new_point_geometry_device(n, c1, c2, d_obs1, d_obs2, scale_factor1, far_points, th_far_points, d_status, d_x3d, stream=None):
    """The same over device arrays (addresses as ints), asynchronous on `stream` (orbm_new_point_geometry_device)."""
    c1, c2 = np.ascontiguousarray(c1, dtype=NP_CAMERA_DTYPE), np.ascontiguousarray(c2, dtype=NP_CAMERA_DTYPE)
    rc = load().orbm_new_point_geometry_device(int(n), _p(c1), _p(c2), _dp(d_obs1), _dp(d_obs2), float(scale_factor1), int(bool(far_points)),
                                               float(th_far_points), _dp(d_status), _dp(d_x3d), _dp(stream))
    return _check_free(rc, "orbm_new_point_geometry_device")


class ORBmatcher:
    """ORB_SLAM3::ORBmatcher (ORBmatcher.h:35-108) -- the projection-search members, on one MI355X."""
    TH_LOW = 50
    TH_HIGH = 100
    HISTO_LENGTH = 30

    def __init__(self, nnratio=0.6, checkOri=True, device=0):
        self.L = load()
        self.m = self.L.orbm_create(int(device))
        if not self.m:
            raise OrbError("orbm_create failed: no usable HIP device %d (no CPU fallback)" % device)
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)

    def close(self):
        if getattr(self, "m", None):
            self.L.orbm_destroy(self.m)
            self.m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc == E_HIP:
            raise OrbError("%s: %s" % (what, self.L.orbm_last_error(self.m).decode()))
        if rc == E_ARG:
            raise ValueError("%s: bad argument (%s)" % (what, self.L.orbm_last_error(self.m).decode()))
        return rc

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        b = np.ascontiguousarray(b, dtype=np.uint8)
        return load().orbm_descriptor_distance(_p(a), _p(b))

    @staticmethod
    def RadiusByViewingCos(viewCos):
        return float(load().orbm_radius_by_viewing_cos(C.c_float(viewCos)))

    @staticmethod
    def ComputeThreeMaxima(histo_sizes):
        h = np.ascontiguousarray(histo_sizes, dtype=np.int32)
        i1, i2, i3 = C.c_int(), C.c_int(), C.c_int()
        load().orbm_three_maxima(_p(h), len(h), C.byref(i1), C.byref(i2), C.byref(i3))
        return i1.value, i2.value, i3.value

    def search_window(self, frame, qdesc, u, v, radius, min_level, max_level, flags=None, u_r=None, nnratio=None,
                      th_dist=None, use_second=True):
        """orbm_search_by_projection: the core shared by the SearchByProjection overloads."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        qdesc, u, v, radius = a(qdesc, np.uint8), a(u, np.float32), a(v, np.float32), a(radius, np.float32)
        min_level, max_level = a(min_level, np.int32), a(max_level, np.int32)
        nq = len(u)
        flags = None if flags is None else a(flags, np.uint8)
        u_r = None if u_r is None else a(u_r, np.float32)
        qs = QueryStruct(nq, _p(qdesc), _p(u), _p(v), _p(radius), _p(min_level), _p(max_level), _p(u_r), _p(flags))
        fs = frame.struct()
        moq = np.full(nq, -1, dtype=np.int32)
        bd = np.full(nq, 256, dtype=np.int32)
        args = (self.m, C.byref(fs), C.byref(qs), C.c_float(self.mfNNratio if nnratio is None else nnratio),
                int(self.TH_HIGH if th_dist is None else th_dist), int(bool(use_second)), _p(frame.slot), _p(frame.slot_obs), _p(moq), _p(bd))
        t0 = time.perf_counter()
        rc = self.L.orbm_search_by_projection(*args)
        self.last_call_s = time.perf_counter() - t0   # the C call alone (arguments made before the clock starts, see ORBextractor.__call__)
        self._check(rc, "orbm_search_by_projection")
        if rc < 0:
            raise OrbError("orbm_search_by_projection rc=%d" % rc)
        return rc, moq, bd

    def SearchByProjection(self, F, mp_in_view, mp_desc, mp_projX, mp_projY, mp_viewCos, mp_level, scale_factors, th=1.0,
                           mp_obs=None, mp_projXR=None):
        """SearchByProjection(Frame &F, const vector<MapPoint*>&, th, ...) -- ORBmatcher.cc:44-143 (mono /
        rectified-stereo half).  MapPoint fields arrive as arrays: mbTrackInView (&& !isBad && far-point test),
        GetDescriptor(), mTrackProjX/Y, mTrackViewCos, mnTrackScaleLevel, Observations()>0."""
        sf = np.asarray(scale_factors, dtype=np.float32)
        lvl = np.asarray(mp_level, dtype=np.int32)
        vc = np.asarray(mp_viewCos, dtype=np.float32)
        r = np.where(vc.astype(np.float64) > 0.998, np.float32(2.5), np.float32(4.0)).astype(np.float32)  # :216-222
        if float(np.float32(th)) != 1.0:
            r = (r * np.float32(th)).astype(np.float32)                                                    # :69-70
        radius = (r * sf[np.clip(lvl, 0, len(sf) - 1)]).astype(np.float32)                               # :73
        nq = len(lvl)
        obs = np.ones(nq, np.uint8) if mp_obs is None else np.asarray(mp_obs, dtype=np.uint8)
        flags = (np.asarray(mp_in_view, dtype=np.uint8) & 1) | ((obs & 1) << 1)
        return self.search_window(F, mp_desc, mp_projX, mp_projY, radius, lvl - 1, lvl, flags=flags, u_r=mp_projXR,
                                  nnratio=self.mfNNratio, th_dist=self.TH_HIGH, use_second=True)

    def SearchByProjectionLastFrame(self, CurrentFrame, scale_factors, has_mp, Xw, mp_desc, last_keys, Tcw, Tlw, cam_type,
                                    cam_params, th, bMono=True, mb=0.0, mbf=0.0, mp_obs=None):
        """SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) -- ORBmatcher.cc:2027-2289."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        sf = a(scale_factors, np.float32)
        has_mp, Xw, mp_desc = a(has_mp, np.uint8), a(Xw, np.float32), a(mp_desc, np.uint8)
        last_keys = a(last_keys, KP_DTYPE)
        Tcw, Tlw, cam_params = a(Tcw, np.float32), a(Tlw, np.float32), a(cam_params, np.float32)
        obs = None if mp_obs is None else a(mp_obs, np.uint8)
        fs = CurrentFrame.struct()
        rc = self.L.orbm_search_by_projection_last_frame(self.m, C.byref(fs), _p(sf), len(sf), len(has_mp), _p(has_mp), _p(Xw),
                                                         _p(mp_desc), _p(last_keys), _p(obs), _p(Tcw), _p(Tlw), int(cam_type),
                                                         _p(cam_params), C.c_float(mb), C.c_float(mbf), C.c_float(th), int(bool(bMono)),
                                                         int(self.mbCheckOrientation), _p(CurrentFrame.slot), _p(CurrentFrame.slot_obs))
        self._check(rc, "orbm_search_by_projection_last_frame")
        if rc < 0:
            raise OrbError("orbm_search_by_projection_last_frame rc=%d" % rc)
        return rc

    def SearchLocalPoints(self, CurrentFrame, scale_factors, log_scale_factor, eligible, Xw, normal, max_dist, min_dist, mp_desc, Tcw,
                          cam_type, cam_params, th, bFarPoints=False, thFarPoints=0.0, mbf=0.0, viewing_cos_limit=0.5, mp_obs=None):
        """Tracking::SearchLocalPoints (Tracking.cc:3449-3539) after the frame's own points are marked: Frame::isInFrustum
        (Frame.cc:572-661) of every local map point, then SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints,
        thFarPoints) (ORBmatcher.cc:44-143), both on the device.  MapPoint fields arrive as arrays: eligible = !isBad() &&
        mnLastFrameSeen != CurrentFrame.mnId, GetWorldPos(), GetNormal(), raw mfMaxDistance / mfMinDistance, GetDescriptor(),
        Observations()>0.  CurrentFrame.slot / slot_obs are updated in place.  Returns (nmatches, match_of_point, track): track
        holds what isInFrustum writes (in_view, proj_x, proj_y, proj_xr, depth, view_cos, level); entries it does not write are 0."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        sf = a(scale_factors, np.float32)
        elig, Xw, normal = a(eligible, np.uint8), a(Xw, np.float32), a(normal, np.float32)
        max_dist, min_dist, mp_desc = a(max_dist, np.float32), a(min_dist, np.float32), a(mp_desc, np.uint8)
        Tcw, cam_params = a(Tcw, np.float32), a(cam_params, np.float32)
        obs = None if mp_obs is None else a(mp_obs, np.uint8)
        nmp = len(elig)
        track = dict(in_view=np.zeros(nmp, np.uint8), proj_x=np.zeros(nmp, np.float32), proj_y=np.zeros(nmp, np.float32),
                     proj_xr=np.zeros(nmp, np.float32), depth=np.zeros(nmp, np.float32), view_cos=np.zeros(nmp, np.float32),
                     level=np.zeros(nmp, np.int32))
        ts = TrackStruct(*[_p(track[k]) for k in ("in_view", "proj_x", "proj_y", "proj_xr", "depth", "view_cos", "level")])
        ms = LocalMapStruct(nmp, _p(elig), _p(Xw), _p(normal), _p(max_dist), _p(min_dist), _p(mp_desc), _p(obs), _p(Tcw))
        moq = np.full(nmp, -1, dtype=np.int32)
        fs = CurrentFrame.struct()
        rc = self.L.orbm_search_local_points(self.m, C.byref(fs), _p(sf), len(sf), C.c_float(log_scale_factor), C.byref(ms), int(cam_type),
                                             _p(cam_params), C.c_float(mbf), C.c_float(viewing_cos_limit), C.c_float(th), int(bool(bFarPoints)),
                                             C.c_float(thFarPoints), C.c_float(self.mfNNratio), _p(CurrentFrame.slot), _p(CurrentFrame.slot_obs),
                                             _p(moq), C.byref(ts))
        self._check(rc, "orbm_search_local_points")
        if rc < 0:
            raise OrbError("orbm_search_local_points rc=%d" % rc)
        return rc, moq, track

    def SearchLocalPointsFisheye(self, CurrentFrame, n_left, left_to_right, right_to_left, scale_factors, log_scale_factor, eligible, Xw,
                                 normal, max_dist, min_dist, mp_desc, Tcw, Trl, tlr, cam_type, cam_params, cam_type2, cam_params2, th,
                                 bFarPoints=False, thFarPoints=0.0, viewing_cos_limit=0.5, mp_obs=None, track=None):
        """Tracking::SearchLocalPoints for a fisheye-stereo frame (Nleft != -1): Frame::isInFrustumChecks per camera
        (Frame.cc:650-660, :1270-1343), then both halves of SearchByProjection(Frame&, const vector<MapPoint*>&, ...)
        (ORBmatcher.cc:44-214), on the device (orbm_search_local_points_fisheye).  CurrentFrame: FrameView over the raw keypoints
        mvKeys ++ mvKeysRight / mDescriptors; left_to_right / right_to_left = mvLeftToRightMatch / mvRightToLeftMatch or None; Trl =
        mTrl (3x4 or 4x4), tlr = mTlr.col(3); cam_type2 / cam_params2 = mpCamera2.  track: dict of the twelve arrays of
        orbm_track_rig_t holding the MapPoints' current values (updated in place; depth is read by the far-point test where the left
        check fails), default all 0.  Returns (nmatches, match_of_point[2 * nmp], track); slots written hold local-map indices."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        sf = a(scale_factors, np.float32)
        elig, Xw, normal = a(eligible, np.uint8), a(Xw, np.float32), a(normal, np.float32)
        max_dist, min_dist, mp_desc = a(max_dist, np.float32), a(min_dist, np.float32), a(mp_desc, np.uint8)
        Tcw, cam_params, cam_params2 = a(Tcw, np.float32), a(cam_params, np.float32), a(cam_params2, np.float32)
        Trl, tlr = a(Trl, np.float32).reshape(-1), a(tlr, np.float32).reshape(-1)
        if Trl.size not in (12, 16) or tlr.size < 3:
            raise ValueError("orbm_search_local_points_fisheye: Trl must hold 12 or 16 floats and tlr 3")
        obs = None if mp_obs is None else a(mp_obs, np.uint8)
        l2r = None if left_to_right is None else a(left_to_right, np.int32)
        r2l = None if right_to_left is None else a(right_to_left, np.int32)
        nmp = len(elig)
        if track is None:
            track = {k: np.zeros(nmp, t) for k, t in TRACK_RIG_FIELDS}
        ts = TrackRigStruct(*[_p(track[k]) for k, _ in TRACK_RIG_FIELDS])
        ms = LocalMapStruct(nmp, _p(elig), _p(Xw), _p(normal), _p(max_dist), _p(min_dist), _p(mp_desc), _p(obs), _p(Tcw))
        mop = np.full(2 * nmp, -1, dtype=np.int32)
        fs = CurrentFrame.struct()
        rc = self.L.orbm_search_local_points_fisheye(self.m, C.byref(fs), int(n_left), _p(l2r), _p(r2l), _p(sf), len(sf), C.c_float(log_scale_factor),
                                                     C.byref(ms), _p(Trl), _p(tlr), int(cam_type), _p(cam_params), int(cam_type2), _p(cam_params2),
                                                     C.c_float(viewing_cos_limit), C.c_float(th), int(bool(bFarPoints)), C.c_float(thFarPoints),
                                                     C.c_float(self.mfNNratio), _p(CurrentFrame.slot), _p(CurrentFrame.slot_obs), _p(mop), C.byref(ts))
        self._check(rc, "orbm_search_local_points_fisheye")
        if rc < 0:
            raise OrbError("orbm_search_local_points_fisheye rc=%d" % rc)
        return rc, mop, track

    def SearchByProjectionFisheye(self, F, n_left, left_to_right, right_to_left, mp_desc, scale_factors, th,
                                  in_view, projX, projY, viewCos, level, in_view_r, projXR, projYR, viewCosR, levelR, mp_obs=None):
        """SearchByProjection(Frame &F, const vector<MapPoint*>&, th, ...) for a fisheye-stereo frame (Nleft != -1) --
        ORBmatcher.cc:44-214 complete.  F: FrameView over mvKeys ++ mvKeysRight / mDescriptors (N = Nleft + Nright).
        Returns (nmatches, match_left[nmp], match_right[nmp]) with right matches as indices into the right image."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        sf = a(scale_factors, np.float32)
        nmp = len(level)
        lvl, lvlR = a(level, np.int32), a(levelR, np.int32)

        def radius_of(vc, lv, with_th):
            r = np.where(a(vc, np.float32).astype(np.float64) > 0.998, np.float32(2.5), np.float32(4.0)).astype(np.float32)  # :216-222
            if with_th and float(np.float32(th)) != 1.0:
                r = (r * np.float32(th)).astype(np.float32)                                                                  # :69-70
            return (r * sf[np.clip(lv, 0, len(sf) - 1)]).astype(np.float32)

        obs = np.ones(nmp, np.uint8) if mp_obs is None else a(mp_obs, np.uint8)
        nq = 2 * nmp
        u, v, rad = np.zeros(nq, np.float32), np.zeros(nq, np.float32), np.zeros(nq, np.float32)
        minl, maxl, flags = np.zeros(nq, np.int32), np.zeros(nq, np.int32), np.zeros(nq, np.uint8)
        u[0::2], v[0::2], rad[0::2] = a(projX, np.float32), a(projY, np.float32), radius_of(viewCos, lvl, True)
        u[1::2], v[1::2], rad[1::2] = a(projXR, np.float32), a(projYR, np.float32), radius_of(viewCosR, lvlR, False)  # :148: no th
        minl[0::2], maxl[0::2] = lvl - 1, lvl
        minl[1::2], maxl[1::2] = lvlR - 1, lvlR
        flags[0::2] = (a(in_view, np.uint8) & 1) | ((obs & 1) << 1)
        flags[1::2] = ((a(in_view_r, np.uint8) & 1) & (lvlR != -1)) | ((obs & 1) << 1)                                 # :147
        qdesc = np.repeat(a(mp_desc, np.uint8).reshape(nmp, 32), 2, axis=0).copy()
        l2r = None if left_to_right is None else a(left_to_right, np.int32)
        r2l = None if right_to_left is None else a(right_to_left, np.int32)
        qs = QueryStruct(nq, _p(qdesc), _p(u), _p(v), _p(rad), _p(minl), _p(maxl), None, _p(flags))
        fs = F.struct()
        moq = np.full(nq, -1, dtype=np.int32)
        rc = self.L.orbm_search_by_projection_fisheye(self.m, C.byref(fs), int(n_left), _p(l2r), _p(r2l), C.byref(qs),
                                                      C.c_float(self.mfNNratio), int(self.TH_HIGH), _p(F.slot), _p(F.slot_obs), _p(moq), None)
        self._check(rc, "orbm_search_by_projection_fisheye")
        if rc < 0:
            raise OrbError("orbm_search_by_projection_fisheye rc=%d" % rc)
        mr = moq[1::2].copy()
        mr[mr >= 0] -= int(n_left)
        return rc, moq[0::2].copy(), mr

    def SearchByProjectionLastFrameFisheye(self, CurrentFrame, n_left, scale_factors, has_mp, Xw, mp_desc, last_keys, Tcw, Tlw, Trl,
                                           cam_type, cam_params, th, bMono=False, mb=0.0, mp_obs=None):
        """SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) for a fisheye-stereo current frame --
        ORBmatcher.cc:2027-2289 complete (incl. the right-camera pass :2189-2256)."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        sf = a(scale_factors, np.float32)
        has_mp, Xw, mp_desc = a(has_mp, np.uint8), a(Xw, np.float32), a(mp_desc, np.uint8)
        last_keys = a(last_keys, KP_DTYPE)
        Tcw, Tlw, Trl, cam_params = a(Tcw, np.float32), a(Tlw, np.float32), a(Trl, np.float32), a(cam_params, np.float32)
        obs = None if mp_obs is None else a(mp_obs, np.uint8)
        fs = CurrentFrame.struct()
        rc = self.L.orbm_search_by_projection_last_frame_fisheye(self.m, C.byref(fs), int(n_left), _p(sf), len(sf), len(has_mp), _p(has_mp),
                                                                 _p(Xw), _p(mp_desc), _p(last_keys), _p(obs), _p(Tcw), _p(Tlw), _p(Trl),
                                                                 int(cam_type), _p(cam_params), C.c_float(mb), C.c_float(th), int(bool(bMono)),
                                                                 int(self.mbCheckOrientation), _p(CurrentFrame.slot), _p(CurrentFrame.slot_obs))
        self._check(rc, "orbm_search_by_projection_last_frame_fisheye")
        if rc < 0:
            raise OrbError("orbm_search_by_projection_last_frame_fisheye rc=%d" % rc)
        return rc

    def SearchForInitialization(self, F1, F2, vbPrevMatched, windowSize=10):
        """SearchForInitialization(Frame &F1, Frame &F2, vbPrevMatched, vnMatches12, windowSize) -- ORBmatcher.cc:722-837.
        F1, F2: FrameView; vbPrevMatched: (N1, 2) float32, updated in place.  Returns (nmatches, vnMatches12)."""
        assert vbPrevMatched.dtype == np.float32 and vbPrevMatched.flags["C_CONTIGUOUS"] and vbPrevMatched.shape == (F1.N, 2)
        m12 = np.full(F1.N, -1, dtype=np.int32)
        f1, f2 = F1.struct(), F2.struct()
        rc = self.L.orbm_search_for_initialization(self.m, C.byref(f1), C.byref(f2), _p(vbPrevMatched), int(windowSize),
                                                   C.c_float(self.mfNNratio), int(self.mbCheckOrientation), _p(m12))
        self._check(rc, "orbm_search_for_initialization")
        if rc < 0:
            raise OrbError("orbm_search_for_initialization rc=%d" % rc)
        return rc, m12

    def SearchByBoW(self, KF, F, n_left=None):
        """SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches) -- ORBmatcher.cc:273-469 (Nleft == -1).
        KF, F: KeyFrameView (KF.has_mappoint = pMP && !isBad).  Returns (nmatches, matchF[F.N] = keyframe keypoint index or -1)."""
        m = np.full(max(F.N, 1), -1, dtype=np.int32)
        ks, fs = KF.struct(), F.struct()
        if n_left is not None:   # fisheye-stereo frame: F = mvKeys ++ mvKeysRight, Frame::Nleft = n_left
            rc = self.L.orbm_search_by_bow_fisheye(self.m, C.byref(ks), C.byref(fs), int(n_left), C.c_float(self.mfNNratio), int(self.mbCheckOrientation), _p(m))
        else:
            rc = self.L.orbm_search_by_bow(self.m, C.byref(ks), C.byref(fs), C.c_float(self.mfNNratio), int(self.mbCheckOrientation), _p(m))
        self._check(rc, "orbm_search_by_bow")
        if rc < 0:
            raise OrbError("orbm_search_by_bow rc=%d" % rc)
        return rc, m[:F.N]

    def SearchByBoWKeyFrames(self, KF1, KF2):
        """SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12) -- ORBmatcher.cc:839-979.
        Returns (nmatches, matches12[KF1.N] = keypoint index in KF2 or -1)."""
        m = np.full(max(KF1.N, 1), -1, dtype=np.int32)
        a, b = KF1.struct(), KF2.struct()
        rc = self.L.orbm_search_by_bow_keyframes(self.m, C.byref(a), C.byref(b), C.c_float(self.mfNNratio), int(self.mbCheckOrientation), _p(m))
        self._check(rc, "orbm_search_by_bow_keyframes")
        if rc < 0:
            raise OrbError("orbm_search_by_bow_keyframes rc=%d" % rc)
        return rc, m[:KF1.N]

    def _bow_candidates(self, what, call, K, n, skip):
        """The outputs of a one-call SearchByBoW: call(skip, rows, nmatches) -> rc.  Returns (nmatches [K], rows [K, n])."""
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
        if sk is not None and len(sk) != K:
            raise ValueError("%s: skip needs one entry per candidate" % what)
        rows, nm = np.full(max(K * n, 1), -1, dtype=np.int32), np.zeros(max(K, 1), np.int32)
        rc = call(_p(sk) if sk is not None and len(sk) else None, _p(rows), _p(nm))
        self._check(rc, what)
        if rc < 0:
            raise OrbError("%s rc=%d" % (what, rc))
        assert rc == int(nm[:K].sum())
        return nm[:K].copy(), rows[:K * n].reshape(K, n)

    def SearchByBoWCandidates(self, KFs, F, n_left=None, skip=None):
        """SearchByBoW(pKF, F, vpMapPointMatches) of all K candidate keyframes KFs against ONE frame F in one call
        (orbm_search_by_bow_candidates; the loop of Tracking::Relocalization, Tracking.cc:3796-3816).  n_left: Frame::Nleft of a
        fisheye-stereo frame (F = mvKeys ++ mvKeysRight); skip [K] marks the candidates that are isBad().
        Returns (nmatches [K], matchF [K, F.N]): row j = what SearchByBoW(KFs[j], F, n_left) returns."""
        K = len(KFs)
        fs = F.struct()
        tab, ptab = self._keyframe_table(KFs)
        call = lambda sk, rows, nm: self.L.orbm_search_by_bow_candidates(self.m, K, ptab, C.byref(fs), -1 if n_left is None else int(n_left), sk,
                                                                         C.c_float(self.mfNNratio), int(self.mbCheckOrientation), rows, nm)
        return self._bow_candidates("orbm_search_by_bow_candidates", call, K, F.N, skip)

    def SearchByBoWKeyFramesCandidates(self, KF1, KF2s, skip=None):
        """SearchByBoW(pKF1, pKF2, vpMatches12) of ONE keyframe KF1 against all K keyframes KF2s in one call
        (orbm_search_by_bow_keyframes_candidates; the loop of LoopClosing::DetectCommonRegionsFromBoW, LoopClosing.cc:724-739).
        Returns (nmatches [K], matches12 [K, KF1.N]): row j = what SearchByBoWKeyFrames(KF1, KF2s[j]) returns."""
        K = len(KF2s)
        s1 = KF1.struct()
        tab, ptab = self._keyframe_table(KF2s)
        call = lambda sk, rows, nm: self.L.orbm_search_by_bow_keyframes_candidates(self.m, C.byref(s1), K, ptab, sk, C.c_float(self.mfNNratio),
                                                                                   int(self.mbCheckOrientation), rows, nm)
        return self._bow_candidates("orbm_search_by_bow_keyframes_candidates", call, K, KF1.N, skip)

    def Fuse(self, KF, scale_factors, inv_level_sigma2, log_scale_factor, valid, Xw, normal, mp_desc, max_dist, min_dist, Tcw, Ow,
             cam_type, cam_params, bf, th=3.0):
        """Search part of Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, th) -- ORBmatcher.cc:1425-1658.
        KF: FrameView of the keyframe (u_right = mvuRight).  Returns (nFused, bestIdx[nP], bestDist[nP])."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        sf, is2 = a(scale_factors, np.float32), a(inv_level_sigma2, np.float32)
        valid, Xw, normal, mp_desc = a(valid, np.uint8), a(Xw, np.float32), a(normal, np.float32), a(mp_desc, np.uint8)
        max_dist, min_dist, Tcw, Ow, cam = a(max_dist, np.float32), a(min_dist, np.float32), a(Tcw, np.float32), a(Ow, np.float32), a(cam_params, np.float32)
        n = len(valid)
        bi, bd = np.full(max(n, 1), -1, np.int32), np.full(max(n, 1), 256, np.int32)
        fs = KF.struct()
        rc = self.L.orbm_fuse(self.m, C.byref(fs), _p(sf), _p(is2), len(sf), C.c_float(log_scale_factor), n, _p(valid), _p(Xw), _p(normal), _p(mp_desc),
                              _p(max_dist), _p(min_dist), _p(Tcw), _p(Ow), int(cam_type), _p(cam), C.c_float(bf), C.c_float(th), _p(bi), _p(bd))
        self._check(rc, "orbm_fuse")
        if rc < 0:
            raise OrbError("orbm_fuse rc=%d" % rc)
        return rc, bi[:n], bd[:n]

    def FuseKeyFrames(self, targets, valid, Xw, normal, mpdesc, max_dist, min_dist, th=3.0):
        """The search part of every Fuse call of LocalMapping::SearchInNeighbors' loop (LocalMapping.cc:989-1000) in one call: one list of
        map points against all targets (FuseTarget).  valid: [T, nP], row t as Fuse's valid for target t.
        Returns (total, best_idx [T, nP], best_dist [T, nP], nfused [T]); row t is what Fuse returns for target t (FUSE RULE, orbhip.h)."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        T = len(targets)
        Xw, normal, mpdesc = a(Xw, np.float32), a(normal, np.float32), a(mpdesc, np.uint8)
        max_dist, min_dist = a(max_dist, np.float32), a(min_dist, np.float32)
        n = len(max_dist)
        valid = a(valid, np.uint8).reshape(T, n)
        bi, bd, nf = np.full((T, n), -1, np.int32), np.full((T, n), 256, np.int32), np.zeros(T, np.int32)
        tab = (FuseTargetStruct * max(T, 1))(*[t.struct() for t in targets])
        rc = self.L.orbm_fuse_keyframes(self.m, T, C.cast(tab, C.c_void_p), n, _p(valid), _p(Xw), _p(normal), _p(mpdesc), _p(max_dist), _p(min_dist),
                                        C.c_float(th), _p(bi), _p(bd), _p(nf))
        self._check(rc, "orbm_fuse_keyframes")
        if rc < 0:
            raise OrbError("orbm_fuse_keyframes rc=%d" % rc)
        return rc, bi, bd, nf

    def FuseSim3(self, KF, scale_factors, log_scale_factor, valid, Xw, normal, mp_desc, max_dist, min_dist, Scw, cam, th=4.0, cam_type=0):
        """Search part of Fuse(KeyFrame *pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint) -- ORBmatcher.cc:1660-1786."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        sf = a(scale_factors, np.float32)
        valid, Xw, normal, mp_desc = a(valid, np.uint8), a(Xw, np.float32), a(normal, np.float32), a(mp_desc, np.uint8)
        max_dist, min_dist, Scw, cam = a(max_dist, np.float32), a(min_dist, np.float32), a(Scw, np.float32), a(cam, np.float32)
        n = len(valid)
        bi, bd = np.full(max(n, 1), -1, np.int32), np.full(max(n, 1), 256, np.int32)
        fs = KF.struct()
        rc = self.L.orbm_fuse_sim3_cam(self.m, C.byref(fs), _p(sf), len(sf), C.c_float(log_scale_factor), n, _p(valid), _p(Xw), _p(normal), _p(mp_desc),
                                       _p(max_dist), _p(min_dist), _p(Scw), int(cam_type), _p(cam), C.c_float(th), _p(bi), _p(bd))
        self._check(rc, "orbm_fuse_sim3")
        if rc < 0:
            raise OrbError("orbm_fuse_sim3 rc=%d" % rc)
        return rc, bi[:n], bd[:n]

    def FuseSim3KeyFrames(self, targets, valid, Xw, normal, mpdesc, max_dist, min_dist, th=4.0):
        """The search part of every Fuse call of LoopClosing::SearchAndFuse's loop (LoopClosing.cc:2631-2707) in one call: one list of map
        points against all corrected keyframes (FuseSim3Target).  valid: [T, nP], row t as FuseSim3's valid for target t.  Returns
        (total, best_idx [T, nP], best_dist [T, nP], nfused [T]); row t is what FuseSim3 returns for target t (SEARCH-AND-FUSE RULE, orbhip.h)."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        T = len(targets)
        Xw, normal, mpdesc = a(Xw, np.float32), a(normal, np.float32), a(mpdesc, np.uint8)
        max_dist, min_dist = a(max_dist, np.float32), a(min_dist, np.float32)
        n = len(max_dist)
        valid = a(valid, np.uint8).reshape(T, n)
        bi, bd, nf = np.full((T, n), -1, np.int32), np.full((T, n), 256, np.int32), np.zeros(T, np.int32)
        tab = (FuseSim3TargetStruct * max(T, 1))(*[t.struct() for t in targets])
        rc = self.L.orbm_fuse_sim3_keyframes(self.m, T, C.cast(tab, C.c_void_p), n, _p(valid), _p(Xw), _p(normal), _p(mpdesc), _p(max_dist),
                                             _p(min_dist), C.c_float(th), _p(bi), _p(bd), _p(nf))
        self._check(rc, "orbm_fuse_sim3_keyframes")
        if rc < 0:
            raise OrbError("orbm_fuse_sim3_keyframes rc=%d" % rc)
        return rc, bi, bd, nf

    def SearchBySim3(self, KF1, side1, KF2, side2, s12, R12, t12, cam1, th):
        """SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vpMatches12, s12, R12, t12, th) -- ORBmatcher.cc:1788-2012.
        KF1, KF2: FrameView of the keyframes; side_k = dict(sf, log_sf, valid, Xw, desc, max_dist, min_dist, Rw, tw).
        Returns (nFound, matches12[KF1.N])."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        keep = []

        def pack(KF, S):
            sf = a(S["sf"], np.float32)
            arrs = [a(S["valid"], np.uint8), a(S["Xw"], np.float32), a(S["desc"], np.uint8), a(S["max_dist"], np.float32), a(S["min_dist"], np.float32),
                    a(S["Rw"], np.float32), a(S["tw"], np.float32)]
            fs = KF.struct()
            keep.extend([sf, fs] + arrs)
            return [C.byref(fs), _p(sf), len(sf), C.c_float(S["log_sf"])] + [_p(x) for x in arrs]

        R12, t12, cam1 = a(R12, np.float32), a(t12, np.float32), a(cam1, np.float32)
        m12 = np.full(max(KF1.N, 1), -1, np.int32)
        rc = self.L.orbm_search_by_sim3(self.m, *pack(KF1, side1), *pack(KF2, side2), C.c_float(s12), _p(R12), _p(t12), _p(cam1), C.c_float(th), _p(m12))
        self._check(rc, "orbm_search_by_sim3")
        if rc < 0:
            raise OrbError("orbm_search_by_sim3 rc=%d" % rc)
        return rc, m12[:KF1.N]

    def ComputeDistinctiveDescriptors(self, groups):
        """MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:350-436) for many map points at once.
        groups: list of (N_p, 32) uint8 arrays (the descriptors observing map point p).  Returns BestIdx per map point."""
        start = np.zeros(len(groups) + 1, np.int32)
        for i, g in enumerate(groups):
            start[i + 1] = start[i] + len(g)
        desc = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint8).reshape(-1, 32) for g in groups]) if len(groups) else np.zeros((0, 32), np.uint8))
        best = np.full(max(len(groups), 1), -1, np.int32)
        rc = self.L.orbm_distinctive_descriptors(self.m, len(groups), _p(start), _p(desc), _p(best))
        self._check(rc, "orbm_distinctive_descriptors")
        if rc < 0:
            raise OrbError("orbm_distinctive_descriptors rc=%d" % rc)
        return best[:len(groups)]

    def UpdateMapPoints(self, points, fill=np.nan):
        """MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:350-436) and MapPoint::UpdateNormalAndDepth (MapPoint.cc:467-547) for all
        map points of one call (orbm_update_map_points; LocalMapping.cc:1040-1053).  points: see pack_map_points, or its result.
        Returns (best [n], normal [n, 3], min_dist [n], max_dist [n]): best relative to the point's first entry, -1 where no entry has
        in_desc set; a point without entries has best -1 and keeps `fill` in its floats."""
        A = points if isinstance(points, dict) else pack_map_points(points)
        n = len(A["start"]) - 1
        u = MapPointUpdateStruct(n, *[_p(A[k]) for k in ("start", "desc", "centre", "in_desc", "pos", "ref_centre", "ref_scale", "ref_max_scale")])
        best = np.full(max(n, 1), -1, np.int32)
        normal, mn, mx = np.full((max(n, 1), 3), fill, np.float32), np.full(max(n, 1), fill, np.float32), np.full(max(n, 1), fill, np.float32)
        rc = self.L.orbm_update_map_points(self.m, C.byref(u), _p(best), _p(normal), _p(mn), _p(mx))
        self._check(rc, "orbm_update_map_points")
        if rc < 0:
            raise OrbError("orbm_update_map_points rc=%d" % rc)
        return best[:n], normal[:n], mn[:n], mx[:n]

    def KeyFrameCulling(self, scene, erasable=None):
        """LocalMapping::KeyFrameCulling (LocalMapping.cc:1158-1310) under the non-inertial rule, the whole loop on the device
        (orbm_keyframe_culling).  scene: see culling_struct; erasable [K] = !mbNotErase per keyframe, None = all.  Returns (n_mps [K],
        n_red [K], culled [K], n_obs_out [P], bad_out [P]): nMPs and nRedundantObservations at each keyframe's turn, which keyframes were
        erased, and Observations() / isBad() of every map point after the loop."""
        c, keep = culling_struct(scene)
        era = None if erasable is None else np.ascontiguousarray(erasable, dtype=np.uint8)
        out = _culling_outputs(c)
        rc = self.L.orbm_keyframe_culling(self.m, C.byref(c), _p(era), *[_p(o) for o in out])
        self._check(rc, "orbm_keyframe_culling")
        if rc < 0:
            raise OrbError("orbm_keyframe_culling rc=%d" % rc)
        return out[0][:c.K], out[1][:c.K], out[2][:c.K], out[3][:c.P], out[4][:c.P]

    def _tv_call(self, fn):
        return lambda *a: fn(self.m, *a)

    def _tv_error(self):
        return self.L.orbm_last_error(self.m).decode()

    def TwoViewReconstruct(self, keys1, keys2, matches12, K, sigma=1.0, iterations=200, sets=None):
        """bool TwoViewReconstruction::Reconstruct(vKeys1, vKeys2, vMatches12, R21, t21, vP3D, vbTriangulated)
        (TwoViewReconstruction.cc:39-127) on the device (orbm_two_view_reconstruct).  keys1 / keys2: KP_DTYPE arrays (mvKeysUn of the two
        frames), matches12 [n1] as SearchForInitialization returns it, K the 3x3 calibration, sets [iterations][8] = mvSets, drawn by the
        caller as the reference draws them (DUtils::Random over rand()).  Returns a TwoViewResult."""
        if sets is None:
            raise ValueError("sets [iterations][8] come from the caller (the reference draws them from libc rand())")
        return _two_view_reconstruct(self._tv_call(self.L.orbm_two_view_reconstruct), "orbm_two_view_reconstruct", self._tv_error, keys1, keys2,
                                     matches12, K, sigma, iterations, sets)

    def TwoViewModels(self, keys1, keys2, matches12, sigma, iterations, sets):
        """The first device stage alone (orbm_two_view_models): H21, H12, F21 and scores of every iteration, best_it, masks."""
        return _two_view_models(self._tv_call(self.L.orbm_two_view_models), "orbm_two_view_models", self._tv_error, keys1, keys2, matches12,
                                sigma, iterations, sets)

    def TwoViewCheckRT(self, keys1, keys2, matches12, inliers, K, sigma, R, t):
        """The second device stage alone (orbm_two_view_check_rt): CheckRT for the caller's hypotheses R [nhyp,3,3], t [nhyp,3]."""
        return _two_view_check_rt(self._tv_call(self.L.orbm_two_view_check_rt), "orbm_two_view_check_rt", self._tv_error, keys1, keys2,
                                  matches12, inliers, K, sigma, R, t)

    def Sim3Solve(self, prob, sets, best_inliers_in=0):
        """Sim3Solver's constructor and one call of iterate(nIterations, bNoMore, vbInliers, nInliers[, bConverge]) (Sim3Solver.cc:35-321) on
        the device (orbm_sim3_solve).  prob: the dict of _sim3_problem (the kept pairs and both keyframes); sets [iterations][3] drawn by the
        caller as the reference draws them (sim3_draw_sets over rand()); best_inliers_in = mnBestInliers.  Returns a Sim3Result."""
        return _sim3_solve(self._tv_call(self.L.orbm_sim3_solve), "orbm_sim3_solve", self._tv_error, prob, sets, best_inliers_in)

    def Sim3Hypotheses(self, prob, sets):
        """The first device stage and the host tail alone (orbm_sim3_hypotheses): T12, T21 and the quaternion row of every set."""
        return _sim3_hypotheses(self._tv_call(self.L.orbm_sim3_hypotheses), "orbm_sim3_hypotheses", self._tv_error, prob, sets)

    def Sim3Check(self, prob, T12, T21):
        """The second device stage alone (orbm_sim3_check): CheckInliers for the caller's transforms T12, T21 [nhyp,4,4]."""
        return _sim3_check(self._tv_call(self.L.orbm_sim3_check), "orbm_sim3_check", self._tv_error, prob, T12, T21)

    def UpdateLocalMap(self, scene, frame_point, inertial=False, last_kf=-1, cap_kf=None, cap_pts=None):
        """Tracking::UpdateLocalMap (Tracking.cc:3542-3762) on the device from host tables (orbm_update_local_map).  scene: see map_graph;
        frame_point [N] = the frame's mvpMapPoints as point indices, -1 = NULL.  Returns a dict: local_kf (mvpLocalKeyFrames), kf_max
        (pKFmax or -1), max_votes, slot_bad [N] (the slots the reference sets to NULL), local_point (mvpLocalMapPoints).  The capacities
        default to what always fits."""
        g, A = map_graph(scene)
        fp = np.ascontiguousarray(frame_point, dtype=np.int32)
        cap_kf, cap_pts = _local_map_caps(g, A, cap_kf, cap_pts)
        out = _local_map_outputs(len(fp), cap_kf, cap_pts)
        rc = self.L.orbm_update_local_map(self.m, C.byref(g), len(fp), _p(fp), int(bool(inertial)), int(last_kf), cap_kf, cap_pts, *[_p(o) for o in out])
        self._check(rc, "orbm_update_local_map")
        return _local_map_result(rc, out, len(fp), "orbm_update_local_map")

    def UpdateLocalMapDevice(self, d_graph, N, d_frame_point, inertial, last_kf, cap_kf, cap_pts, d_local_kf, d_n_local_kf, d_kf_max, d_max_votes,
                             d_slot_bad, d_local_point, d_n_local_point, stream=None):
        """The resident form (orbm_update_local_map_device): d_graph is a MapGraph holding device addresses (map_graph_device), every other
        d_ argument a device address (int).  Asynchronous on `stream`; writes are clamped at the capacities, the counts say what was needed."""
        rc = self.L.orbm_update_local_map_device(self.m, C.byref(d_graph), int(N), _dp(d_frame_point), int(bool(inertial)), int(last_kf), int(cap_kf),
                                                 int(cap_pts), _dp(d_local_kf), _dp(d_n_local_kf), _dp(d_kf_max), _dp(d_max_votes), _dp(d_slot_bad),
                                                 _dp(d_local_point), _dp(d_n_local_point), _dp(stream))
        self._check(rc, "orbm_update_local_map_device")
        if rc < 0:
            raise OrbError("orbm_update_local_map_device rc=%d" % rc)

    def UpdateConnections(self, scene, targets, th=15, cap=None):
        """KFcounter and the ordered lists of KeyFrame::UpdateConnections (KeyFrame.cc:407-492) for every keyframe of `targets`, all counted
        from the state at entry (CONNECTIONS RULE, include/orbhip.h), on the device (orbm_update_connections).  Returns one dict per target:
        conn_kf / conn_w (mConnectedKeyFrameWeights in rank order), ord_kf / ord_w (mvpOrderedConnectedKeyFrames / mvOrderedWeights),
        kf_max, nmax.  What the member writes on other keyframes stays the caller's.  cap defaults to T * G elements per list, which always
        fits; the device block of a call grows as 20 * T * G bytes, so pass a long loop over a large map in chunks of targets."""
        g, A = map_graph(scene)
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        cap = len(tg) * g.G if cap is None else int(cap)
        out = _connections_outputs(len(tg), cap)
        rc = self.L.orbm_update_connections(self.m, C.byref(g), len(tg), _p(tg), int(th), cap, *[_p(o) for o in out])
        self._check(rc, "orbm_update_connections")
        return _connections_result(rc, out, len(tg), "orbm_update_connections")

    def GatherLocalMapDevice(self, P, N, d_frame_point, d_local_point, d_n_local_point, cap, d_pt_bad, d_Xw, d_normal, d_max_dist, d_min_dist,
                             d_mpdesc, d_obs, out, d_map_n, stream=None):
        """orbm_gather_local_map_device: fills the device arrays of `out` (a LocalMapStruct of device addresses) from the local-point list
        that UpdateLocalMapDevice left on the device and per-point tables; d_map_n receives the live count."""
        rc = self.L.orbm_gather_local_map_device(self.m, int(P), int(N), _dp(d_frame_point), _dp(d_local_point), _dp(d_n_local_point), int(cap),
                                                 _dp(d_pt_bad), _dp(d_Xw), _dp(d_normal), _dp(d_max_dist), _dp(d_min_dist), _dp(d_mpdesc), _dp(d_obs),
                                                 C.byref(out), _dp(d_map_n), _dp(stream))
        self._check(rc, "orbm_gather_local_map_device")
        if rc < 0:
            raise OrbError("orbm_gather_local_map_device rc=%d" % rc)

    def KeyFrameCullingOpen(self, scene):
        """Opens the stepwise walk (orbm_keyframe_culling_open): uploads the scene and computes the loop-entry status of every row.  An
        unfinished walk is discarded."""
        c, keep = culling_struct(scene)
        rc = self.L.orbm_keyframe_culling_open(self.m, C.byref(c))
        self._check(rc, "orbm_keyframe_culling_open")
        if rc < 0:
            raise OrbError("orbm_keyframe_culling_open rc=%d" % rc)
        self._cull_counts = (np.full(max(c.K, 1), -1, np.int32), np.full(max(c.K, 1), -1, np.int32), c.K)

    def KeyFrameCullingStep(self, applied):
        """One step of the walk (orbm_keyframe_culling_step): erases the keyframe the previous step returned if `applied`, then walks on to
        the next unskipped keyframe that passes the test.  Returns (k, n_mps [K], n_red [K]): k = that keyframe or K at the end; the
        counts of every keyframe walked so far, -1 where the walk has not been yet."""
        n_mps, n_red, K = getattr(self, "_cull_counts", (np.zeros(1, np.int32), np.zeros(1, np.int32), 0))
        k = np.full(1, -1, np.int32)
        rc = self.L.orbm_keyframe_culling_step(self.m, int(bool(applied)), _p(k), _p(n_mps), _p(n_red))
        self._check(rc, "orbm_keyframe_culling_step")
        if rc < 0:
            raise OrbError("orbm_keyframe_culling_step rc=%d" % rc)
        return int(k[0]), n_mps[:K].copy(), n_red[:K].copy()

    def ComputeStereoFishEyeMatches(self, keysL, descL, monoL, keysR, descR, monoR, level_sigma2, Tlr, cam_params, cam_params2, p3d=None):
        """Frame::ComputeStereoFishEyeMatches (Frame.cc:1228-1268) of one rig frame from host arrays (orbm_stereo_fisheye_matches).
        keysL / keysR: KP_DTYPE arrays (mvKeys / mvKeysRight), lapping rows from monoL / monoR; Tlr: 3x4 [mRlr | mtlr].  Returns
        (mvLeftToRightMatch, mvRightToLeftMatch, mvDepth, mvStereo3Dpoints [Nleft, 3], (nMatches, descMatches)); p3d: initial contents of
        the 3-D points, kept where unmatched (zeros by default)."""
        f = lambda x: np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        keysL, keysR = np.ascontiguousarray(keysL, dtype=KP_DTYPE), np.ascontiguousarray(keysR, dtype=KP_DTYPE)
        descL, descR = np.ascontiguousarray(descL, dtype=np.uint8), np.ascontiguousarray(descR, dtype=np.uint8)
        nL, nR = len(keysL), len(keysR)
        sig = f(level_sigma2)
        l2r, r2l = np.full(max(nL, 1), -1, np.int32), np.full(max(nR, 1), -1, np.int32)
        depth = np.full(max(nL, 1), -1.0, np.float32)
        p3 = np.zeros((max(nL, 1), 3), np.float32) if p3d is None else np.array(p3d, dtype=np.float32, order="C").reshape(-1, 3)
        nm = np.zeros(2, np.int32)
        rc = self.L.orbm_stereo_fisheye_matches(self.m, _p(keysL), _p(descL), nL, int(monoL), _p(keysR), _p(descR), nR, int(monoR), _p(sig), len(sig),
                                                _p(f(Tlr)), _p(f(cam_params)), _p(f(cam_params2)), _p(l2r), _p(r2l), _p(depth), _p(p3), _p(nm))
        self._check(rc, "orbm_stereo_fisheye_matches")
        if rc < 0:
            raise OrbError("orbm_stereo_fisheye_matches rc=%d" % rc)
        return l2r[:nL], r2l[:nR], depth[:nL], p3[:nL], (int(nm[0]), int(nm[1]))

    def stereo_fisheye_matches_batch_device(self, nframes, d_keysL, d_descL, d_countsL, d_keysR, d_descR, d_countsR, cap, level_sigma2, Tlr,
                                            cam_params, cam_params2, out_stride, d_left_to_right, d_right_to_left, d_depth, d_p3d, d_nmatches=None,
                                            stream=None):
        """Frame::ComputeStereoFishEyeMatches for `nframes` resident rig frames (orbm_stereo_fisheye_matches_batch_device): the d_*
        arguments are device addresses (ints): what two extract_batch_device calls of the same cap wrote, and the output tables of
        out_stride entries per frame; level_sigma2, Tlr and the parameter sets are host arrays.  Asynchronous on `stream`."""
        what = "orbm_stereo_fisheye_matches_batch_device: "
        f = lambda x: np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        if level_sigma2 is None or Tlr is None or cam_params is None or cam_params2 is None:
            raise ValueError(what + "missing level_sigma2, Tlr or camera parameters")
        sig = f(level_sigma2)
        if f(Tlr).size != 12 or f(cam_params).size != 8 or f(cam_params2).size != 8:
            raise ValueError(what + "Tlr needs 12 floats, each KannalaBrandt8 parameter set 8")
        if not (d_keysL and d_descL and d_countsL and d_keysR and d_descR and d_countsR):
            raise ValueError(what + "missing input")
        if not (d_left_to_right and d_right_to_left and d_depth and d_p3d):
            raise ValueError(what + "missing output")
        if not 0 <= nframes <= 65535:
            raise ValueError(what + "nframes outside [0, 65535]")
        if cap <= 0 or 2 * cap > FISHEYE_MAX_KEYPOINTS:
            raise ValueError(what + "cap outside (0, %d]" % (FISHEYE_MAX_KEYPOINTS // 2))
        if out_stride < cap:
            raise ValueError(what + "out_stride below cap")
        if not 1 <= len(sig) <= 16:
            raise ValueError(what + "nlevels outside [1, 16]")
        rc = self.L.orbm_stereo_fisheye_matches_batch_device(self.m, int(nframes), _dp(d_keysL), _dp(d_descL), _dp(d_countsL), _dp(d_keysR), _dp(d_descR),
                                                             _dp(d_countsR), int(cap), _p(sig), len(sig), _p(f(Tlr)), _p(f(cam_params)), _p(f(cam_params2)),
                                                             int(out_stride), _dp(d_left_to_right), _dp(d_right_to_left), _dp(d_depth), _dp(d_p3d),
                                                             _dp(d_nmatches), _dp(stream))
        self._check(rc, "orbm_stereo_fisheye_matches_batch_device")
        if rc < 0:
            raise OrbError("orbm_stereo_fisheye_matches_batch_device rc=%d" % rc)

    def knnMatch2(self, query, train):
        """cv::BFMatcher(NORM_HAMMING).knnMatch(query, train, matches, 2) (Frame.cc:1246).  Returns (idx[nq, 2], dist[nq, 2])."""
        query, train = np.ascontiguousarray(query, dtype=np.uint8), np.ascontiguousarray(train, dtype=np.uint8)
        nq = len(query)
        idx, dist = np.full((max(nq, 1), 2), -1, np.int32), np.full((max(nq, 1), 2), -1, np.int32)
        rc = self.L.orbm_knn_match2(self.m, _p(query), nq, _p(train), len(train), _p(idx), _p(dist))
        self._check(rc, "orbm_knn_match2")
        if rc < 0:
            raise OrbError("orbm_knn_match2 rc=%d" % rc)
        return idx[:nq], dist[:nq]

    def SearchByProjectionKeyFrame(self, CurrentFrame, scale_factors, log_scale_factor, valid, Xw, mp_desc, kf_angle, max_dist,
                                   min_dist, Tcw, cam_type, cam_params, th, ORBdist):
        """SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*>&, th, ORBdist) -- ORBmatcher.cc:2291-2413."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        sf = a(scale_factors, np.float32)
        valid, Xw, mp_desc = a(valid, np.uint8), a(Xw, np.float32), a(mp_desc, np.uint8)
        kf_angle, max_dist, min_dist = a(kf_angle, np.float32), a(max_dist, np.float32), a(min_dist, np.float32)
        Tcw, cam_params = a(Tcw, np.float32), a(cam_params, np.float32)
        fs = CurrentFrame.struct()
        rc = self.L.orbm_search_by_projection_keyframe(self.m, C.byref(fs), _p(sf), len(sf), C.c_float(log_scale_factor), len(valid), _p(valid),
                                                       _p(Xw), _p(mp_desc), _p(kf_angle), _p(max_dist), _p(min_dist), _p(Tcw), int(cam_type),
                                                       _p(cam_params), C.c_float(th), int(ORBdist), int(self.mbCheckOrientation),
                                                       _p(CurrentFrame.slot), _p(CurrentFrame.slot_obs))
        self._check(rc, "orbm_search_by_projection_keyframe")
        if rc < 0:
            raise OrbError("orbm_search_by_projection_keyframe rc=%d" % rc)
        return rc

    def SearchByProjectionSim3(self, KF, scale_factors, log_scale_factor, valid, Xw, normal, mp_desc, max_dist, min_dist, Scw, cam, th,
                               ratioHamming=1.0, cam_type=0):
        """SearchByProjection(KeyFrame *pKF, cv::Mat Scw, vpPoints, vpMatched, th, ratioHamming) -- ORBmatcher.cc:489-720.
        KF is a FrameView of the keyframe's keypoints; KF.slot plays vpMatched."""
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        sf = a(scale_factors, np.float32)
        valid, Xw, normal, mp_desc = a(valid, np.uint8), a(Xw, np.float32), a(normal, np.float32), a(mp_desc, np.uint8)
        max_dist, min_dist, Scw, cam = a(max_dist, np.float32), a(min_dist, np.float32), a(Scw, np.float32), a(cam, np.float32)
        fs = KF.struct()
        rc = self.L.orbm_search_by_projection_sim3_cam(self.m, C.byref(fs), _p(sf), len(sf), C.c_float(log_scale_factor), len(valid), _p(valid),
                                                       _p(Xw), _p(normal), _p(mp_desc), _p(max_dist), _p(min_dist), _p(Scw), int(cam_type), _p(cam), int(th),
                                                       C.c_float(ratioHamming), _p(KF.slot), _p(KF.slot_obs))
        self._check(rc, "orbm_search_by_projection_sim3")
        if rc < 0:
            raise OrbError("orbm_search_by_projection_sim3 rc=%d" % rc)
        return rc

    def SearchForTriangulation(self, KF1, KF2, R1w, t1w, R2w, t2w, Cw1, cam1, cam2, bOnlyStereo=False, bCoarse=False):
        """SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) -- ORBmatcher.cc:981-1222.
        Returns (nmatches, vMatchedPairs as an int array [k, 2])."""
        a = lambda x: np.ascontiguousarray(x, dtype=np.float32)
        R1w, t1w, R2w, t2w, Cw1, cam1, cam2 = a(R1w), a(t1w), a(R2w), a(t2w), a(Cw1), a(cam1), a(cam2)
        m12 = np.full(max(KF1.N, 1), -1, dtype=np.int32)
        s1, s2 = KF1.struct(), KF2.struct()
        rc = self.L.orbm_search_for_triangulation(self.m, C.byref(s1), C.byref(s2), _p(R1w), _p(t1w), _p(R2w), _p(t2w), _p(Cw1), _p(cam1),
                                                  _p(cam2), int(bool(bOnlyStereo)), int(bool(bCoarse)), int(self.mbCheckOrientation), _p(m12))
        self._check(rc, "orbm_search_for_triangulation")
        if rc < 0:
            raise OrbError("orbm_search_for_triangulation rc=%d" % rc)
        m12 = m12[:KF1.N]
        i1 = np.nonzero(m12 >= 0)[0]
        return rc, np.stack([i1, m12[i1]], axis=1).astype(np.int64)

    def TriangulationCandidates(self, KF1, KF2, ep, epipole_gate, bOnlyStereo=False):
        """orbm_triangulation_candidates: (start[KF1.N + 1], idx2[], dist[]) - per keypoint of KF1 the same-node keypoints of KF2 that
        pass every gate in front of the epipolar predicate (ORBmatcher.cc:1080-1113), ordered (dist ascending, node position descending)."""
        s1, s2 = KF1.struct(), KF2.struct()
        start = np.zeros(KF1.N + 1, np.int32)
        cap = 4096
        while True:
            idx2, dist = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
            tot = self.L.orbm_triangulation_candidates(self.m, C.byref(s1), C.byref(s2), C.c_float(ep[0]), C.c_float(ep[1]), int(bool(epipole_gate)),
                                                       int(bool(bOnlyStereo)), _p(start), _p(idx2), _p(dist), cap)
            self._check(tot, "orbm_triangulation_candidates")
            if tot < 0:
                raise OrbError("orbm_triangulation_candidates rc=%d" % tot)
            if tot <= cap:
                return start, idx2[:tot].copy(), dist[:tot].copy()
            cap = tot

    def SearchForTriangulationPred(self, KF1, KF2, ep, epipole_gate, pred, bOnlyStereo=False, bCoarse=False):
        """SearchForTriangulation for camera models whose epipolarConstrain is not Pinhole's (KannalaBrandt8, rigs): pred(idx1, idx2) is
        the caller's predicate (ORBmatcher.cc:1148).  Returns (nmatches, vMatchedPairs [k, 2])."""
        s1, s2 = KF1.struct(), KF2.struct()
        m12 = np.full(max(KF1.N, 1), -1, dtype=np.int32)
        cb = PAIR_PRED(lambda user, i1, i2: 1 if pred(i1, i2) else 0)
        rc = self.L.orbm_search_for_triangulation_pred(self.m, C.byref(s1), C.byref(s2), C.c_float(ep[0]), C.c_float(ep[1]), int(bool(epipole_gate)),
                                                       int(bool(bOnlyStereo)), int(bool(bCoarse)), int(self.mbCheckOrientation), cb, None, _p(m12))
        self._check(rc, "orbm_search_for_triangulation_pred")
        if rc < 0:
            raise OrbError("orbm_search_for_triangulation_pred rc=%d" % rc)
        m12 = m12[:KF1.N]
        i1 = np.nonzero(m12 >= 0)[0]
        return rc, np.stack([i1, m12[i1]], axis=1).astype(np.int64)

    def SearchForTriangulationKB8(self, KF1, KF2, ep, cams1, cams2, T12, n_left1=-1, n_left2=-1, bOnlyStereo=False, bCoarse=False):
        """SearchForTriangulation between KannalaBrandt8 keyframes (n_left == -1) or two-camera KannalaBrandt8 rigs (n_left = NLeft, the
        views hold [mvKeys; mvKeysRight]) with KannalaBrandt8::epipolarConstrain on the device (orbm_search_for_triangulation_kb8).
        cams? [8] or [2, 8], T12 [12] or [4, 12] = [R12 | t12] per camera pair ll, lr, rl, rr.  Returns (nmatches, vMatchedPairs [k, 2])."""
        rig = n_left1 != -1 or n_left2 != -1
        a = lambda x: np.ascontiguousarray(x, dtype=np.float32).reshape(-1) if x is not None else None   # None: the ABI's refusal
        cams1, cams2, T12 = a(cams1), a(cams2), a(T12)
        for v, per in ((cams1, 8), (cams2, 8), (T12, 12)):
            if v is not None and len(v) != per * ((2 if per == 8 else 4) if rig else 1):
                raise ValueError("SearchForTriangulationKB8: %d floats where %s are expected" % (len(v), "2 x 8 / 4 x 12" if rig else "8 / 12"))
        s1, s2 = KF1.struct(), KF2.struct()
        m12 = np.full(max(KF1.N, 1), -1, dtype=np.int32)
        rc = self.L.orbm_search_for_triangulation_kb8(self.m, C.byref(s1), int(n_left1), C.byref(s2), int(n_left2), C.c_float(ep[0]), C.c_float(ep[1]),
                                                      _p(cams1) if cams1 is not None else None, _p(cams2) if cams2 is not None else None,
                                                      _p(T12) if T12 is not None else None, int(bool(bOnlyStereo)), int(bool(bCoarse)),
                                                      int(self.mbCheckOrientation), _p(m12))
        self._check(rc, "orbm_search_for_triangulation_kb8")
        if rc < 0:
            raise OrbError("orbm_search_for_triangulation_kb8 rc=%d" % rc)
        m12 = m12[:KF1.N]
        i1 = np.nonzero(m12 >= 0)[0]
        return rc, np.stack([i1, m12[i1]], axis=1).astype(np.int64)

    @staticmethod
    def _keyframe_table(KFs):
        """orbm_keyframe_t[K] of the views (kept alive by the caller) - (ctypes array or None, its address or None)."""
        if not KFs:
            return None, None
        tab = (KeyFrameStruct * len(KFs))(*[k.struct() for k in KFs])
        return tab, C.cast(tab, C.c_void_p)

    def _neighbour_rows(self, rc, what, m12, nm, K, n1):
        self._check(rc, what)
        if rc < 0:
            raise OrbError("%s rc=%d" % (what, rc))
        assert rc == int(nm[:K].sum())
        return m12[:K * n1].reshape(K, n1), nm[:K].copy()

    def SearchForTriangulationNeighbours(self, KF1, KF2s, R1w, t1w, Cw1, cam1, R2w, t2w, cam2, skip=None, bOnlyStereo=False, bCoarse=False):
        """SearchForTriangulation of KF1 against all K neighbours KF2s in one call (orbm_search_for_triangulation_neighbours; the loop of
        LocalMapping::CreateNewMapPoints, LocalMapping.cc:475-583), Pinhole keyframes.  R2w [K, 3, 3], t2w [K, 3], cam2 [K, 4]; skip [K]
        marks the neighbours the baseline tests drop.  Returns (matches12 [K, KF1.N], nmatches [K]): row j = vMatches12 of the per-pair
        member from the state at loop entry, without the rotation check; the caller masks idx1 that received a map point since."""
        K = len(KF2s)
        a = lambda x, n: np.ascontiguousarray(x, dtype=np.float32).reshape(-1) if x is not None else None
        R1w, t1w, Cw1, cam1, R2w, t2w, cam2 = a(R1w, 9), a(t1w, 3), a(Cw1, 3), a(cam1, 4), a(R2w, 9 * K), a(t2w, 3 * K), a(cam2, 4 * K)
        for v, n in ((R1w, 9), (t1w, 3), (Cw1, 3), (cam1, 4), (R2w, 9 * K), (t2w, 3 * K), (cam2, 4 * K)):
            if v is not None and len(v) != n:
                raise ValueError("SearchForTriangulationNeighbours: %d floats where %d are expected" % (len(v), n))
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
        if sk is not None and len(sk) != K:
            raise ValueError("SearchForTriangulationNeighbours: skip needs one entry per neighbour")
        s1 = KF1.struct()
        tab, ptab = self._keyframe_table(KF2s)
        m12, nm = np.full(max(K * KF1.N, 1), -1, dtype=np.int32), np.zeros(max(K, 1), np.int32)
        q = lambda v: _p(v) if v is not None and len(v) else None
        rc = self.L.orbm_search_for_triangulation_neighbours(self.m, C.byref(s1), K, ptab, q(R1w), q(t1w), q(Cw1), q(cam1), q(R2w), q(t2w), q(cam2),
                                                             q(sk), int(bool(bOnlyStereo)), int(bool(bCoarse)), _p(m12), _p(nm))
        return self._neighbour_rows(rc, "orbm_search_for_triangulation_neighbours", m12, nm, K, KF1.N)

    def SearchForTriangulationKB8Neighbours(self, KF1, KF2s, ep, cams1, cams2, T12, n_left1=-1, n_left2=None, skip=None, bOnlyStereo=False,
                                            bCoarse=False):
        """The same for KannalaBrandt8 keyframes (n_left1 == -1) or two-camera KannalaBrandt8 rigs (orbm_search_for_triangulation_kb8_neighbours).
        Per neighbour: ep [K, 2], cams2 [K, 8] or [K, 2, 8], T12 [K, 12] or [K, 4, 12], n_left2 [K] (default: all -1); cams1 [8] or [2, 8].
        Returns (matches12 [K, KF1.N], nmatches [K])."""
        K = len(KF2s)
        rig = n_left1 != -1
        f = lambda x: np.ascontiguousarray(x, dtype=np.float32) if x is not None else None
        ep, cams1, cams2, T12 = f(ep), f(cams1), f(cams2), f(T12)
        c1 = None
        if cams1 is not None:
            c1 = np.zeros(16, np.float32)
            c1[:cams1.size] = cams1.reshape(-1)[:16]
        c2 = t12 = None
        if cams2 is not None and K:      # the ABI's strides are a rig's
            c2 = np.zeros((K, 16), np.float32)
            c2[:, :(16 if rig else 8)] = cams2.reshape(K, -1)
        if T12 is not None and K:
            t12 = np.zeros((K, 48), np.float32)
            t12[:, :(48 if rig else 12)] = T12.reshape(K, -1)
        if ep is not None:
            ep = np.ascontiguousarray(ep.reshape(K, 2))
        nl2 = np.full(K, -1, np.int32) if n_left2 is None else np.ascontiguousarray(n_left2, dtype=np.int32)
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
        if len(nl2) != K or (sk is not None and len(sk) != K):
            raise ValueError("SearchForTriangulationKB8Neighbours: n_left2 and skip need one entry per neighbour")
        s1 = KF1.struct()
        tab, ptab = self._keyframe_table(KF2s)
        m12, nm = np.full(max(K * KF1.N, 1), -1, dtype=np.int32), np.zeros(max(K, 1), np.int32)
        q = lambda v: _p(v) if v is not None and v.size else None
        rc = self.L.orbm_search_for_triangulation_kb8_neighbours(self.m, C.byref(s1), int(n_left1), K, ptab, q(nl2), q(ep), q(c1), q(c2), q(t12), q(sk),
                                                                 int(bool(bOnlyStereo)), int(bool(bCoarse)), _p(m12), _p(nm))
        return self._neighbour_rows(rc, "orbm_search_for_triangulation_kb8_neighbours", m12, nm, K, KF1.N)

    @staticmethod
    def _geometry_table(Gs):
        if not Gs:
            return None, None
        tab = (KeyFrameGeometryStruct * len(Gs))(*[g.struct() for g in Gs])
        return tab, C.cast(tab, C.c_void_p)

    def _new_points(self, call, what, K, n1, cap, status, matches):
        """Runs call(points, cap, status, matches12, nmatches) and shapes (points, status, matches12, nmatches)."""
        cap = n1 if cap is None else int(cap)
        pts = np.zeros(max(cap, 1), NEW_POINT_DTYPE)
        st = np.zeros(max(K * n1, 1), np.uint8) if status else None
        m12 = np.full(max(K * n1, 1), -1, np.int32) if matches else None
        nm = np.zeros(max(K, 1), np.int32) if matches else None
        rc = call(_p(pts) if cap > 0 else None, cap, _p(st), _p(m12), _p(nm))
        self._check(rc, what)
        if rc < 0:
            raise OrbError("%s rc=%d" % (what, rc))
        shape = lambda a: None if a is None else a[:K * n1].reshape(K, n1)
        return (pts[:rc] if rc <= cap else rc), shape(st), shape(m12), (None if nm is None else nm[:K].copy())

    def CreateNewMapPoints(self, KF1, G1, scale_factor1, KF2s, G2s, R1w, t1w, Cw1, cam1, R2w, t2w, cam2, skip=None, bCoarse=False, far_points=False,
                           th_far_points=0.0, cap=None, status=True, matches=True):
        """LocalMapping::CreateNewMapPoints (LocalMapping.cc:470-905) for Pinhole keyframes, mono and rectified stereo mixed per keypoint
        (orbm_create_new_map_points): SearchForTriangulationNeighbours, then the body of the loop on every matched pair on the device.
        G1 / G2s: KeyFrameGeometry; scale_factor1 = mfScaleFactor of KF1.  Returns (points, status [K, N1] or None, matches12 [K, N1] or None,
        nmatches [K] or None): points is a NEW_POINT_DTYPE array in the reference's creation order - or, when it holds more than cap entries
        (default KF1.N, which always suffices), the needed count as an int.  The caller keeps the entries with neighbour < i when
        CheckNewKeyFrames() ends the loop in front of neighbour i."""
        K = len(KF2s)
        a = lambda x: np.ascontiguousarray(x, dtype=np.float32).reshape(-1) if x is not None else None
        R1w, t1w, Cw1, cam1, R2w, t2w, cam2 = a(R1w), a(t1w), a(Cw1), a(cam1), a(R2w), a(t2w), a(cam2)
        for v, n in ((R1w, 9), (t1w, 3), (Cw1, 3), (cam1, 4), (R2w, 9 * K), (t2w, 3 * K), (cam2, 4 * K)):
            if v is not None and len(v) != n:
                raise ValueError("CreateNewMapPoints: %d floats where %d are expected" % (len(v), n))
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
        if (sk is not None and len(sk) != K) or (G2s is not None and len(G2s) != K):
            raise ValueError("CreateNewMapPoints: skip and G2s need one entry per neighbour")
        s1, g1 = KF1.struct(), (G1.struct() if G1 is not None else None)
        tab, ptab = self._keyframe_table(KF2s)
        gtab, pgtab = self._geometry_table(G2s)
        q = lambda v: _p(v) if v is not None and len(v) else None
        call = lambda pts, cap_, st, m12, nm: self.L.orbm_create_new_map_points(
            self.m, C.byref(s1), C.byref(g1) if g1 is not None else None, float(scale_factor1), K, ptab, pgtab, q(R1w), q(t1w), q(Cw1), q(cam1), q(R2w),
            q(t2w), q(cam2), q(sk), int(bool(bCoarse)), int(bool(far_points)), float(th_far_points), pts, cap_, st, m12, nm)
        return self._new_points(call, "orbm_create_new_map_points", K, KF1.N, cap, status, matches)

    def CreateNewMapPointsKB8(self, KF1, G1, scale_factor1, KF2s, G2s, ep, cams1, cams2, T12, n_left1=-1, n_left2=None, skip=None, bCoarse=False,
                              far_points=False, th_far_points=0.0, cap=None, status=True, matches=True):
        """The same for KannalaBrandt8 keyframes (n_left1 == -1) or two-camera KannalaBrandt8 rigs (orbm_create_new_map_points_kb8); the
        search's arguments are SearchForTriangulationKB8Neighbours', for rigs G?.Tcw_right / Ow_right are read."""
        K = len(KF2s)
        rig = n_left1 != -1
        f = lambda x: np.ascontiguousarray(x, dtype=np.float32) if x is not None else None
        ep, cams1, cams2, T12 = f(ep), f(cams1), f(cams2), f(T12)
        c1 = None
        if cams1 is not None:
            c1 = np.zeros(16, np.float32)
            c1[:cams1.size] = cams1.reshape(-1)[:16]
        c2 = t12 = None
        if cams2 is not None and K:      # the ABI's strides are a rig's
            c2 = np.zeros((K, 16), np.float32)
            c2[:, :(16 if rig else 8)] = cams2.reshape(K, -1)
        if T12 is not None and K:
            t12 = np.zeros((K, 48), np.float32)
            t12[:, :(48 if rig else 12)] = T12.reshape(K, -1)
        if ep is not None:
            ep = np.ascontiguousarray(ep.reshape(K, 2))
        nl2 = np.full(K, -1, np.int32) if n_left2 is None else np.ascontiguousarray(n_left2, dtype=np.int32)
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8)
        if len(nl2) != K or (sk is not None and len(sk) != K) or (G2s is not None and len(G2s) != K):
            raise ValueError("CreateNewMapPointsKB8: n_left2, skip and G2s need one entry per neighbour")
        s1, g1 = KF1.struct(), (G1.struct() if G1 is not None else None)
        tab, ptab = self._keyframe_table(KF2s)
        gtab, pgtab = self._geometry_table(G2s)
        q = lambda v: _p(v) if v is not None and v.size else None
        call = lambda pts, cap_, st, m12, nm: self.L.orbm_create_new_map_points_kb8(
            self.m, C.byref(s1), C.byref(g1) if g1 is not None else None, float(scale_factor1), int(n_left1), K, ptab, pgtab, q(nl2), q(ep), q(c1), q(c2),
            q(t12), q(sk), int(bool(bCoarse)), int(bool(far_points)), float(th_far_points), pts, cap_, st, m12, nm)
        return self._new_points(call, "orbm_create_new_map_points_kb8", K, KF1.N, cap, status, matches)

    def hamming_matrix(self, q, c):
        q = np.ascontiguousarray(q, dtype=np.uint8)
        c = np.ascontiguousarray(c, dtype=np.uint8)
        d = np.zeros((len(q), len(c)), dtype=np.uint16)
        self._check(self.L.orbm_hamming_matrix(self.m, _p(q), len(q), _p(c), len(c), _p(d)), "orbm_hamming_matrix")
        return d

    def undistort_batch_device(self, d_keys, key_stride, d_counts, count_stride, nframes, K, D, d_keys_un, stream=None, n_const=0):
        """Frame::UndistortKeyPoints (Frame.cc:837-870) on keypoints resident in HBM; pointers are device addresses (ints)."""
        K, D = np.ascontiguousarray(K, dtype=np.float32), np.ascontiguousarray(D, dtype=np.float32)
        rc = self.L.orbm_undistort_keypoints_batch_device(self.m, C.c_void_p(d_keys), int(key_stride), C.c_void_p(d_counts) if d_counts else None,
                                                          int(count_stride), int(n_const), int(nframes), _p(K), _p(D), len(D), C.c_void_p(d_keys_un),
                                                          C.c_void_p(stream) if stream else None)
        self._check(rc, "orbm_undistort_keypoints_batch_device")
        if rc < 0:
            raise OrbError("orbm_undistort_keypoints_batch_device rc=%d" % rc)

    def search_local_points_batch_device(self, cur0, frame_stride, d_frame_n, frame_n_stride, map0, map_stride, d_map_n, map_n_stride,
                                         npairs, scale_factors, log_scale_factor, cam_type, cam_params, th, d_slot, d_slot_obs,
                                         d_match_of_point, track0, d_nmatches, bFarPoints=False, thFarPoints=0.0, mbf=0.0,
                                         viewing_cos_limit=0.5, stream=None):
        """Tracking::SearchLocalPoints for `npairs` (frame, local map) problems resident in HBM (orbm_search_local_points_batch_device).
        cur0 / map0 / track0: FrameStruct / LocalMapStruct / TrackStruct of problem 0 holding device addresses; the other pointers are
        device addresses (ints, d_frame_n / d_map_n / d_match_of_point may be None); asynchronous on `stream`."""
        sf, cam_params = np.ascontiguousarray(scale_factors, dtype=np.float32), np.ascontiguousarray(cam_params, dtype=np.float32)
        v = lambda x: C.c_void_p(x) if x else None
        rc = self.L.orbm_search_local_points_batch_device(self.m, C.byref(cur0), int(frame_stride), v(d_frame_n), int(frame_n_stride), C.byref(map0),
                                                          int(map_stride), v(d_map_n), int(map_n_stride), int(npairs), _p(sf), len(sf),
                                                          C.c_float(log_scale_factor), int(cam_type), _p(cam_params), C.c_float(mbf),
                                                          C.c_float(viewing_cos_limit), C.c_float(th), int(bool(bFarPoints)), C.c_float(thFarPoints),
                                                          C.c_float(self.mfNNratio), v(d_slot), v(d_slot_obs), v(d_match_of_point), C.byref(track0),
                                                          v(d_nmatches), v(stream))
        self._check(rc, "orbm_search_local_points_batch_device")
        if rc < 0:
            raise OrbError("orbm_search_local_points_batch_device rc=%d" % rc)

    def search_local_points_fisheye_batch_device(self, cur0, frame_stride, d_frame_n, frame_n_stride, d_n_left, n_left_stride, d_left_to_right,
                                                 d_right_to_left, map0, map_stride, d_map_n, map_n_stride, npairs, scale_factors,
                                                 log_scale_factor, Trl, tlr, cam_type, cam_params, cam_type2, cam_params2, th, d_slot, d_slot_obs,
                                                 d_match_of_point, track0, d_nmatches, n_left=0, bFarPoints=False, thFarPoints=0.0,
                                                 viewing_cos_limit=0.5, stream=None):
        """Tracking::SearchLocalPoints for `npairs` (fisheye-stereo frame, local map) problems resident in HBM
        (orbm_search_local_points_fisheye_batch_device).  cur0 / map0 / track0: FrameStruct / LocalMapStruct / TrackRigStruct of
        problem 0 holding device addresses; the other pointers are device addresses (ints; d_frame_n / d_n_left / d_left_to_right /
        d_right_to_left / d_map_n / d_match_of_point may be None, n_left is the constant Nleft when d_n_left is None); Trl, tlr,
        scale_factors and both cam_params are host arrays; asynchronous on `stream`."""
        a = lambda x: np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        sf, cam_params, cam_params2 = a(scale_factors), a(cam_params), a(cam_params2)
        Trl, tlr = None if Trl is None else a(Trl), None if tlr is None else a(tlr)
        what = "orbm_search_local_points_fisheye_batch_device: "
        if Trl is None or tlr is None:
            raise ValueError(what + "Trl or tlr is missing")
        if Trl.size not in (12, 16) or tlr.size < 3:
            raise ValueError(what + "Trl must hold 12 or 16 floats and tlr 3")
        if npairs < 0 or not d_slot or not d_slot_obs or not d_nmatches:
            raise ValueError(what + "npairs < 0 or a missing output")
        if not 1 <= len(sf) <= 16 or any(int(t) not in (0, 1) or len(q) < (4 if int(t) == 0 else 8) for t, q in ((cam_type, cam_params), (cam_type2, cam_params2))):
            raise ValueError(what + "nlevels outside [1, 16] or an unknown camera")
        if not d_n_left and not 0 <= int(n_left) <= cur0.n:
            raise ValueError(what + "n_left outside [0, N]")
        if frame_stride > FISHEYE_MAX_KEYPOINTS:
            raise ValueError(what + "frame_stride above %d" % FISHEYE_MAX_KEYPOINTS)
        v = lambda x: C.c_void_p(x) if x else None
        rc = self.L.orbm_search_local_points_fisheye_batch_device(
            self.m, C.byref(cur0), int(frame_stride), v(d_frame_n), int(frame_n_stride), v(d_n_left), int(n_left_stride), int(n_left),
            v(d_left_to_right), v(d_right_to_left), C.byref(map0), int(map_stride), v(d_map_n), int(map_n_stride), int(npairs), _p(sf), len(sf),
            C.c_float(log_scale_factor), _p(Trl), _p(tlr), int(cam_type), _p(cam_params), int(cam_type2), _p(cam_params2),
            C.c_float(viewing_cos_limit), C.c_float(th), int(bool(bFarPoints)), C.c_float(thFarPoints), C.c_float(self.mfNNratio), v(d_slot),
            v(d_slot_obs), v(d_match_of_point), C.byref(track0), v(d_nmatches), v(stream))
        self._check(rc, "orbm_search_local_points_fisheye_batch_device")
        if rc < 0:
            raise OrbError("orbm_search_local_points_fisheye_batch_device rc=%d" % rc)
        return rc

    def search_by_projection_last_frame_fisheye_batch_device(self, cur0, frame_stride, d_frame_n, frame_n_stride, d_n_left, n_left_stride,
                                                             last0, last_stride, d_last_n, last_n_stride, npairs, scale_factors, Trl,
                                                             cam_type, cam_params, th, d_slot, d_slot_obs, d_match_of_query, d_nmatches,
                                                             n_left=0, bMono=False, mb=0.0, stream=None):
        """SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) for `npairs` fisheye-stereo current frames
        resident in HBM (orbm_search_by_projection_last_frame_fisheye_batch_device).  cur0 / last0: FrameStruct / LastFrameStruct of
        problem 0 holding device addresses; the other pointers are device addresses (ints; d_frame_n / d_n_left / d_last_n /
        d_match_of_query may be None, n_left is the constant Nleft when d_n_left is None); Trl, scale_factors and cam_params are host
        arrays; asynchronous on `stream`.  The refusals that need no device raise ValueError before the library is called."""
        sf, cam_params = np.ascontiguousarray(scale_factors, dtype=np.float32), np.ascontiguousarray(cam_params, dtype=np.float32)
        if Trl is None:
            raise ValueError("orbm_search_by_projection_last_frame_fisheye_batch_device: Trl is missing")
        Trl = np.ascontiguousarray(Trl, dtype=np.float32).reshape(-1)
        if Trl.size not in (12, 16):
            raise ValueError("orbm_search_by_projection_last_frame_fisheye_batch_device: Trl must hold 12 or 16 floats")
        if npairs < 0 or not d_slot or not d_slot_obs or not d_nmatches:
            raise ValueError("orbm_search_by_projection_last_frame_fisheye_batch_device: npairs < 0 or a missing output")
        if not 1 <= len(sf) <= 16 or int(cam_type) not in (0, 1) or len(cam_params) < (4 if int(cam_type) == 0 else 8):
            raise ValueError("orbm_search_by_projection_last_frame_fisheye_batch_device: nlevels outside [1, 16] or an unknown camera")
        if not d_n_left and not 0 <= int(n_left) <= cur0.n:
            raise ValueError("orbm_search_by_projection_last_frame_fisheye_batch_device: n_left outside [0, N]")
        if frame_stride > FISHEYE_MAX_KEYPOINTS:
            raise ValueError("orbm_search_by_projection_last_frame_fisheye_batch_device: frame_stride above %d" % FISHEYE_MAX_KEYPOINTS)
        v = lambda x: C.c_void_p(x) if x else None
        rc = self.L.orbm_search_by_projection_last_frame_fisheye_batch_device(
            self.m, C.byref(cur0), int(frame_stride), v(d_frame_n), int(frame_n_stride), v(d_n_left), int(n_left_stride), int(n_left), C.byref(last0),
            int(last_stride), v(d_last_n), int(last_n_stride), int(npairs), _p(sf), len(sf), _p(Trl), int(cam_type), _p(cam_params), C.c_float(mb),
            C.c_float(th), int(bool(bMono)), int(self.mbCheckOrientation), v(d_slot), v(d_slot_obs), v(d_match_of_query), v(d_nmatches), v(stream))
        self._check(rc, "orbm_search_by_projection_last_frame_fisheye_batch_device")
        if rc < 0:
            raise OrbError("orbm_search_by_projection_last_frame_fisheye_batch_device rc=%d" % rc)
        return rc

    def set_profiling(self, on=True):
        self.L.orbm_set_profiling(self.m, 1 if on else 0)

    def set_scan_mode(self, mode):
        """0 = per frame pair on the device (default), 1 = k_match_scan, 2 = k_match_walk; results do not depend on it."""
        self._check(self.L.orbm_set_scan_mode(self.m, int(mode)), "orbm_set_scan_mode")

    def set_hamming_engine(self, engine):
        """0 = vector ALU, 1 = open-window blocks on the matrix pipe (k_match_scan_mfma), 2 (default) = as 1 + the lists of all-open frame
        pairs built inside k_match_resolve (fused form); results do not depend on it."""
        self._check(self.L.orbm_set_hamming_engine(self.m, int(engine)), "orbm_set_hamming_engine")

    def last_ms(self):
        return float(self.L.orbm_get_last_ms(self.m))

    def stage_ms(self):
        ms = np.zeros(2, dtype=np.float32)
        n = self.L.orbm_get_stage_ms(self.m, _p(ms), 2)
        return dict(zip(["match_scan", "match_resolve"], ms[:n].tolist()))


def undistort_keypoints(keys, K, D):
    """Frame::UndistortKeyPoints (Frame.cc:837-870): mvKeys -> mvKeysUn."""
    keys = np.ascontiguousarray(keys, dtype=KP_DTYPE)
    K, D = np.ascontiguousarray(K, dtype=np.float32), np.ascontiguousarray(D, dtype=np.float32)
    out = np.zeros_like(keys)
    load().orbm_undistort_keypoints(len(keys), _p(keys), _p(K), _p(D), len(D), _p(out))
    return out


def image_bounds(cols, rows, K, D):
    """Frame::ComputeImageBounds (Frame.cc:872-899): (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    K, D = np.ascontiguousarray(K, dtype=np.float32), np.ascontiguousarray(D, dtype=np.float32)
    v = [C.c_float() for _ in range(4)]
    load().orbm_image_bounds(int(cols), int(rows), _p(K), _p(D), len(D), *[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def project(cam_type, params, X, Y, Z):
    """GeometricCamera::project: 0 = Pinhole (Pinhole.cpp:46-49), 1 = KannalaBrandt8 (KannalaBrandt8.cpp:29-45)."""
    params = np.ascontiguousarray(params, dtype=np.float32)
    u, v = C.c_float(), C.c_float()
    load().orbm_project(int(cam_type), _p(params), C.c_float(X), C.c_float(Y), C.c_float(Z), C.byref(u), C.byref(v))
    return u.value, v.value


def rig_right_camera(Tcw, Trl, tlr):
    """The right camera of Frame::isInFrustumChecks (Frame.cc:1276-1280) as the kernels form it: ([mR | mt] as 3x4, twc)."""
    a = lambda x: np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    Tr, twc = np.zeros(12, np.float32), np.zeros(3, np.float32)
    load().orbm_rig_right_camera(_p(a(Tcw)), _p(a(Trl)), _p(a(tlr)), _p(Tr), _p(twc))
    return Tr.reshape(3, 4), twc


def _dp(a):
    return C.c_void_p(a) if a else None


def _check_free(rc, what):
    if rc == E_ARG:
        raise ValueError("%s: bad argument" % what)
    if rc < 0:
        raise OrbError("%s rc=%d" % (what, rc))
    return rc


def stereo_from_rgbd_batch_device(nframes, d_keys, d_keys_un, d_counts, count_stride, cap, d_depth_image, depth_type, rows, cols, row_stride,
                                  frame_stride, depth_factor, mbf, d_uRight, d_depth, d_nstereo=None, stream=None):
    """Frame::ComputeStereoFromRGBD (Frame.cc:1082-1103) for `nframes` resident RGB-D frames (orbx_stereo_from_rgbd_batch_device):
    all pointers are device addresses (ints), asynchronous on `stream`.  depth_type 0 = uint16, 1 = float32; strides in bytes;
    depth_factor = mDepthMapFactor (already the reciprocal).  d_uRight / d_depth [nframes][cap] float32 receive mvuRight / mvDepth
    for i < N, d_nstereo [nframes] int32 (optional) the number of keypoints with depth."""
    rc = load().orbx_stereo_from_rgbd_batch_device(int(nframes), _dp(d_keys), _dp(d_keys_un), _dp(d_counts), int(count_stride), int(cap),
                                                   _dp(d_depth_image), int(depth_type), int(rows), int(cols), C.c_size_t(row_stride),
                                                   C.c_size_t(frame_stride), C.c_float(depth_factor), C.c_float(mbf), _dp(d_uRight), _dp(d_depth),
                                                   _dp(d_nstereo), _dp(stream))
    return _check_free(rc, "orbx_stereo_from_rgbd_batch_device")


def clahe_batch_device(nframes, d_src, rows, cols, src_stride, src_frame_stride, clip_limit, tiles_x, tiles_y, d_lut, d_dst, dst_stride,
                       dst_frame_stride, stream=None):
    """createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply of the TUM-VI examples (mono_tum_vi.cc:101-109) for `nframes` resident
    frames (orbx_clahe_batch_device): all pointers are device addresses (ints), asynchronous on `stream`, strides in bytes.  Frame f at
    d_src + f * src_frame_stride, result at d_dst + f * dst_frame_stride; d_dst == d_src with equal strides is the in-place form.
    d_lut: nframes * tiles_x * tiles_y * 256 bytes of scratch."""
    rc = load().orbx_clahe_batch_device(int(nframes), _dp(d_src), int(rows), int(cols), C.c_size_t(src_stride), C.c_size_t(src_frame_stride),
                                        C.c_double(clip_limit), int(tiles_x), int(tiles_y), _dp(d_lut), _dp(d_dst), C.c_size_t(dst_stride),
                                        C.c_size_t(dst_frame_stride), _dp(stream))
    return _check_free(rc, "orbx_clahe_batch_device")


def remap_linear_batch_device(nframes, d_src, src_rows, src_cols, src_stride, src_frame_stride, d_mapx, d_mapy, map_stride_elems, rows, cols,
                              d_dst, dst_stride, dst_frame_stride, stream=None):
    """cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) of the stereo examples (stereo_euroc.cc:166-167) for `nframes` resident frames
    with one float map pair (orbx_remap_linear_batch_device): all pointers are device addresses (ints), asynchronous on `stream`,
    image strides in bytes, map_stride_elems in floats.  The destination must not overlap the source.  A thread serves
    REMAP_FRAME_CHUNK frames with one decoded map entry."""
    rc = load().orbx_remap_linear_batch_device(int(nframes), _dp(d_src), int(src_rows), int(src_cols), C.c_size_t(src_stride),
                                               C.c_size_t(src_frame_stride), _dp(d_mapx), _dp(d_mapy), C.c_size_t(map_stride_elems), int(rows), int(cols),
                                               _dp(d_dst), C.c_size_t(dst_stride), C.c_size_t(dst_frame_stride), _dp(stream))
    return _check_free(rc, "orbx_remap_linear_batch_device")


def clahe_band_lut_rows(rows, tiles_y, y0, y1):
    """(first, count) of the table rows orbx_clahe_batch_device stages for the image rows y0 .. y1 (orbx_clahe_band_lut_rows)."""
    first, count = C.c_int(), C.c_int()
    _check_free(load().orbx_clahe_band_lut_rows(int(rows), int(tiles_y), int(y0), int(y1), C.byref(first), C.byref(count)), "orbx_clahe_band_lut_rows")
    return first.value, count.value


def close_points_batch_device(nframes, d_depth, d_counts, count_stride, cap, th_depth, max_point, d_order, d_nvisit, d_tracked=None, d_close=None,
                              d_keys_un=None, fx=0.0, fy=0.0, cx=0.0, cy=0.0, d_x3Dc=None, d_pose=None, d_x3Dw=None, stream=None):
    """The depth-ordered close-point rule of Tracking::UpdateLastFrame / CreateNewKeyFrame (Tracking.cc:2808-2860, :3345-3416) for
    `nframes` resident frames (orbx_close_points_batch_device): d_order [nframes][cap] int32 receives the keypoint indices in
    visiting order, d_nvisit [nframes] their number.  Optional: d_close [nframes][2] (nTrackedClose, nNonTrackedClose, from the bytes
    d_tracked), d_x3Dc / d_x3Dw [nframes][cap][3] (Frame::UnprojectStereo; need d_keys_un, fx, fy, cx, cy and, for d_x3Dw, d_pose
    [nframes][12] = [Rwc | Ow])."""
    rc = load().orbx_close_points_batch_device(int(nframes), _dp(d_depth), _dp(d_counts), int(count_stride), int(cap), C.c_float(th_depth), int(max_point),
                                               _dp(d_order), _dp(d_nvisit), _dp(d_tracked), _dp(d_close), _dp(d_keys_un), C.c_float(fx), C.c_float(fy),
                                               C.c_float(cx), C.c_float(cy), _dp(d_x3Dc), _dp(d_pose), _dp(d_x3Dw), _dp(stream))
    return _check_free(rc, "orbx_close_points_batch_device")


def rig_concat_batch_device(nframes, d_keysL, d_descL, d_countsL, d_keysR, d_descR, d_countsR, cap, d_keys, d_desc, d_n, stream=None):
    """The Frame of a two-camera fisheye rig from two resident extractions (Frame.cc:1162-1164, :1201; orbm_rig_concat_batch_device):
    per frame the nL left keypoints / descriptors and the nR right ones directly behind them in d_keys [nframes][2 * cap] /
    d_desc [nframes][2 * cap][32], d_n [nframes][2] = {nL + nR, nL}.  All pointers are device addresses (ints), asynchronous on
    `stream`."""
    rc = load().orbm_rig_concat_batch_device(int(nframes), _dp(d_keysL), _dp(d_descL), _dp(d_countsL), _dp(d_keysR), _dp(d_descR), _dp(d_countsR),
                                             int(cap), _dp(d_keys), _dp(d_desc), _dp(d_n), _dp(stream))
    return _check_free(rc, "orbm_rig_concat_batch_device")


def unproject(cam_params, xy):
    """KannalaBrandt8::unproject (KannalaBrandt8.cpp:112-139) of the pixels xy [n, 2]: rays [n, 3] (orbm_unproject, host)."""
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    rays = np.zeros((max(len(xy), 1), 3), np.float32)
    _check_free(load().orbm_unproject(_p(np.ascontiguousarray(cam_params, dtype=np.float32)), len(xy), _p(xy), _p(rays)), "orbm_unproject")
    return rays[:len(xy)]


def fisheye_triangulate(kp1, kp2, sigma1, sigma2, Tlr, cam_params, cam_params2, p3d_fill=0.0):
    """KannalaBrandt8::TriangulateMatches (KannalaBrandt8.cpp:343-412) of the keypoint pairs kp1 / kp2 [n, 2] on the host
    (orbm_fisheye_triangulate): (depth [n] = z1 or -1, p3D [n, 3], p3d_fill where the function returns early)."""
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    n = len(f(kp1)) // 2
    depth, p3 = np.zeros(max(n, 1), np.float32), np.full((max(n, 1), 3), p3d_fill, np.float32)
    _check_free(load().orbm_fisheye_triangulate(n, _p(f(kp1)), _p(f(kp2)), _p(f(sigma1)), _p(f(sigma2)), _p(f(Tlr)), _p(f(cam_params)),
                                                _p(f(cam_params2)), _p(depth), _p(p3)), "orbm_fisheye_triangulate")
    return depth[:n], p3[:n]


def fisheye_triangulate_device(n, d_kp1, d_kp2, d_sigma1, d_sigma2, Tlr, cam_params, cam_params2, d_depth, d_p3d, stream=None):
    """The same over device arrays (addresses as ints), asynchronous on `stream` (orbm_fisheye_triangulate_device)."""
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    rc = load().orbm_fisheye_triangulate_device(int(n), _dp(d_kp1), _dp(d_kp2), _dp(d_sigma1), _dp(d_sigma2), _p(f(Tlr)), _p(f(cam_params)),
                                                _p(f(cam_params2)), _dp(d_depth), _dp(d_p3d), _dp(stream))
    return _check_free(rc, "orbm_fisheye_triangulate_device")


def _voc_error(what, rc):
    msg = (load().orbv_last_error(None) or b"").decode()
    if rc == E_ARG:
        raise ValueError("%s: %s" % (what, msg or "bad argument"))
    raise OrbError("%s rc=%d: %s" % (what, rc, msg))


class ORBVocabulary:
    """ORB_SLAM3::ORBVocabulary (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>, ORBVocabulary.h:29-30): the transform of
    Frame::ComputeBoW (Frame.cc:828-835) and KeyFrame::ComputeBoW (KeyFrame.cc:100-110) over orbv_* of include/orbhip.h.

    device >= 0 uploads the tables; device = -1 gives a handle on which only transform_host works (so that the statement of
    csrc/orb_ref_voc.h can be tested without a GPU; it is not a fallback: transform raises on it)."""

    WEIGHTING = ("TF_IDF", "TF", "IDF", "BINARY")                                              # BowVector.h:39-45
    SCORING = ("L1_NORM", "L2_NORM", "CHI_SQUARE", "KL", "BHATTACHARYYA", "DOT_PRODUCT")       # BowVector.h:48-56

    def __init__(self, k, L, weighting, scoring, parent, is_leaf, descriptor, weight, device=0):
        self.L_lib = load()
        self.k, self.L, self.weighting, self.scoring, self.device = int(k), int(L), int(weighting), int(scoring), int(device)
        self.parent = np.ascontiguousarray(parent, dtype=np.uint32)
        self.is_leaf = np.ascontiguousarray(is_leaf, dtype=np.uint8)
        self.descriptor = np.ascontiguousarray(descriptor, dtype=np.uint8).reshape(-1, 32)
        self.weight = np.ascontiguousarray(weight, dtype=np.float64)
        n = len(self.parent)
        if not (len(self.is_leaf) == len(self.descriptor) == len(self.weight) == n):
            raise ValueError("ORBVocabulary: the node tables differ in length")
        s = VocNodesStruct(self.k, self.L, self.weighting, self.scoring, n, _p(self.parent), _p(self.is_leaf), _p(self.descriptor),
                           _p(self.weight))
        self.v = self.L_lib.orbv_create(C.byref(s), self.device)
        if not self.v:
            msg = (self.L_lib.orbv_last_error(None) or b"").decode()
            if "HIP: " in msg:
                raise OrbError("orbv_create: " + msg)
            raise ValueError("orbv_create: " + msg)
        self.n_nodes = self.L_lib.orbv_n_nodes(self.v)
        self.n_words = self.L_lib.orbv_n_words(self.v)
        self.max_children = self.L_lib.orbv_max_children(self.v)
        self.min_leaf_level = self.L_lib.orbv_min_leaf_level(self.v)

    def __del__(self):
        try:
            if getattr(self, "v", None):
                self.L_lib.orbv_destroy(self.v)
                self.v = None
        except Exception:
            pass

    @classmethod
    def from_nodes(cls, k, L, weighting, scoring, parent, is_leaf, descriptor, weight, device=0):
        """m_nodes flattened in id order (orbv_nodes_t): node 0 is the root, parent[i] < i, descriptor [n, 32] uint8, weight float64."""
        return cls(k, L, weighting, scoring, parent, is_leaf, descriptor, weight, device=device)

    @staticmethod
    def parse_text(path):
        """The tables of an ORBvoc-format text file: (k, L, scoring, weighting, parent, is_leaf, descriptor, weight).  First line
        `k L scoring weighting`, then one line per node `parent is_leaf d0 .. d31 weight` (TemplatedVocabulary.h:1338-1424)."""
        with open(path) as f:
            head = f.readline().split()
            k, L, scoring, weighting = (int(x) for x in head[:4])
            parent, leaf, desc, weight = [0], [0], [np.zeros(32, np.uint8)], [0.0]
            for line in f:
                t = line.split()
                if not t:
                    continue
                parent.append(int(t[0]))
                leaf.append(1 if int(t[1]) > 0 else 0)
                desc.append(np.array([int(x) for x in t[2:34]], dtype=np.uint8))
                weight.append(float(t[34]))
        return k, L, scoring, weighting, np.array(parent, np.uint32), np.array(leaf, np.uint8), np.stack(desc), np.array(weight, np.float64)

    @classmethod
    def load_text(cls, path, device=0):
        """loadFromTextFile (TemplatedVocabulary.h:1338-1424).  ONE DIFFERENCE from the loader: blank lines are skipped.  The loader
        makes a node of every line it reads (:1378-1386), and its `while(!f.eof())` reads one empty line for every newline after
        the last node line - the one that ends the file as saveToTextFile writes it included.  On an empty line `>> pid` and
        `>> nIsLeaf` fail at the stream's sentry and store nothing, so the parent and the leaf flag of that node are indeterminate
        reads; its weight is 0 (Node()) and its descriptor whatever cv::Mat::create(1, 32, CV_8U) returns.  Compiled with g++
        -std=c++11 -O2 against libstdc++ (tests/test_ref_voc.py prints it) the node hangs under the PREVIOUS line's parent, is
        flagged as a leaf and takes a new word id, so size() grows by one per empty line.  Skipping the line costs exactly that:
        this vocabulary has one word fewer than size() reports there - a word of weight 0 that no BowVector can hold, with a
        descriptor that cannot be reproduced.  Every word id, node id and weight of the real nodes is the loader's (the extra nodes
        come last).  A drop-in build passes m_nodes as the loader left them through from_nodes / orbv_create instead
        (csrc/adapter/snippets/ComputeBoW_hip.cc), extra nodes included; tests/test_ref_voc.py and tests/test_gpu_ref_voc.py run
        that path on the compiled loader's own tables."""
        k, L, scoring, weighting, parent, leaf, desc, weight = cls.parse_text(path)
        return cls(k, L, weighting, scoring, parent, leaf, desc, weight, device=device)

    def _transform(self, fn, what, desc, levelsup):
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        n = len(desc)
        m = max(n, 1)
        word, node = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        bow_id, bow_val = np.zeros(m, np.uint32), np.zeros(m, np.float64)
        fv_node, fv_start, fv_idx = np.zeros(m, np.uint32), np.zeros(m + 1, np.int32), np.zeros(m, np.int32)
        n_bow, n_fv = C.c_int32(-1), C.c_int32(-1)
        rc = fn(self.v, _p(desc), n, int(levelsup), _p(word), _p(node), _p(bow_id), _p(bow_val), C.byref(n_bow), _p(fv_node), _p(fv_start),
                _p(fv_idx), C.byref(n_fv))
        if rc < 0:
            _voc_error(what, rc)
        nb, nf = n_bow.value, n_fv.value
        return dict(word=word[:n], node=node[:n], bow_id=bow_id[:nb].copy(), bow_val=bow_val[:nb].copy(), fv_node_id=fv_node[:nf].copy(),
                    fv_start=fv_start[:nf + 1].copy(), fv_idx=fv_idx[:int(fv_start[nf])].copy())

    def transform(self, desc, levelsup=4):
        """transform(features, mBowVec, mFeatVec, levelsup) on the device (orbv_transform).  Returns a dict of the flat layouts: word,
        node [n]; bow_id (ascending), bow_val = the BowVector; fv_node_id (ascending), fv_start, fv_idx = the FeatureVector as
        orbm_keyframe_t reads it.  Raises on a device = -1 handle: there is no host fallback."""
        return self._transform(self.L_lib.orbv_transform, "orbv_transform", desc, levelsup)

    def transform_host(self, desc, levelsup=4):
        """The same through orbv_transform_host: csrc/orb_ref_voc.h in plain C++ (what tests compare the kernels and the model with)."""
        return self._transform(self.L_lib.orbv_transform_host, "orbv_transform_host", desc, levelsup)

    @staticmethod
    def feat_vec(t):
        """{node id: [feature indices]} of a transform result: what KeyFrameView takes as mFeatVec."""
        return {int(nid): [int(i) for i in t["fv_idx"][t["fv_start"][g]:t["fv_start"][g + 1]]] for g, nid in enumerate(t["fv_node_id"])}

    @staticmethod
    def batch_scratch_bytes(nframes, cap):
        return int(load().orbv_batch_scratch_bytes(int(nframes), int(cap)))

    def transform_batch_device(self, d_descriptors, nframes, cap, d_n, n_stride, levelsup, d_bow_id, d_bow_val, d_n_bow, d_fv_node_id,
                               d_fv_start, d_fv_idx, d_n_fv, d_scratch, d_word=None, d_node=None, stream=None, descend_form=None):
        """The transform for `nframes` resident frames (orbv_transform_batch_device): all pointers are device addresses (ints),
        asynchronous on `stream`.  d_descriptors [nframes][cap][32]; live count of frame p = d_n[p * n_stride]; outputs of frame p at
        p * cap (d_fv_start at p * (cap + 1)); d_scratch: batch_scratch_bytes(nframes, cap) bytes.  descend_form (0 / 1) selects the
        descent kernel through orbv_transform_batch_device_form, for tests and measurements."""
        tail = (_dp(d_descriptors), int(nframes), int(cap), _dp(d_n), int(n_stride), int(levelsup), _dp(d_word), _dp(d_node), _dp(d_bow_id),
                _dp(d_bow_val), _dp(d_n_bow), _dp(d_fv_node_id), _dp(d_fv_start), _dp(d_fv_idx), _dp(d_n_fv), _dp(d_scratch), _dp(stream))
        if descend_form is None:
            rc = self.L_lib.orbv_transform_batch_device(self.v, *tail)
        else:
            rc = self.L_lib.orbv_transform_batch_device_form(self.v, int(descend_form), *tail)
        if rc < 0:
            _voc_error("orbv_transform_batch_device", rc)
        return rc


def _kfdb_error(what, rc):
    msg = (load().orbd_last_error(None) or b"").decode()
    if rc == E_ARG:
        raise ValueError("%s: %s" % (what, msg or "bad argument"))
    raise OrbError("%s rc=%d: %s" % (what, rc, msg))


class KeyFrameDatabase:
    """ORB_SLAM3::KeyFrameDatabase (KeyFrameDatabase.cc:39-98) with its two live queries, DetectRelocalizationCandidates
    (KeyFrameDatabase.cc:814-926) and DetectNBestCandidates (KeyFrameDatabase.cc:620-811), over orbd_* of include/orbhip.h.

    Keyframes are named by tags (any unsigned 64-bit integer but NO_TAG).  A BowVector is a pair (ids, values) or a transform result
    (a dict with bow_id / bow_val).  device >= 0 allocates the device tables; device = -1 gives a handle on which only the _host forms
    work (so that csrc/orb_ref_kfdb.h can be tested without a GPU; it is not a fallback: the device forms raise on it)."""

    def __init__(self, n_words, capacity=MAX_KEYFRAMES, scoring=0, device=0, vocabulary=None):
        self.L_lib = load()
        self.device = int(device)
        if vocabulary is not None:
            self.d = self.L_lib.orbd_create_for_vocabulary(vocabulary.v, int(capacity), self.device)
        else:
            self.d = self.L_lib.orbd_create(int(n_words), int(scoring), int(capacity), self.device)
        if not self.d:
            msg = (self.L_lib.orbd_last_error(None) or b"").decode()
            if "HIP: " in msg:
                raise OrbError("orbd_create: " + msg)
            raise ValueError("orbd_create: " + msg)
        self.n_words = self.L_lib.orbd_n_words(self.d)
        self.capacity = self.L_lib.orbd_capacity(self.d)

    @classmethod
    def for_vocabulary(cls, voc, capacity=MAX_KEYFRAMES, device=0):
        return cls(0, capacity, device=device, vocabulary=voc)

    def __del__(self):
        try:
            if getattr(self, "d", None):
                self.L_lib.orbd_destroy(self.d)
                self.d = None
        except Exception:
            pass

    def __len__(self):
        return self.L_lib.orbd_size(self.d)

    @staticmethod
    def _bow(bow):
        if isinstance(bow, dict):
            bow = (bow["bow_id"], bow["bow_val"])
        ids = np.ascontiguousarray(bow[0], dtype=np.uint32).reshape(-1)
        val = np.ascontiguousarray(bow[1], dtype=np.float64).reshape(-1)
        if len(ids) != len(val):
            raise ValueError("KeyFrameDatabase: ids and values differ in length")
        return ids, val

    @staticmethod
    def _members(init):
        if init is None:
            return None
        return C.byref(KfdbMembersStruct(int(init.get("reloc_query", 0)), int(init.get("place_query", 0)), float(init.get("reloc_score", 0.0)),
                                         float(init.get("place_score", 0.0))))

    def _rc(self, rc, what):
        if rc < 0:
            _kfdb_error(what, rc)
        return rc

    def add(self, tag, map_id, bow, init=None):
        """KeyFrameDatabase::add (KeyFrameDatabase.cc:39-45).  init: a dict of reloc_query, reloc_score, place_query, place_score."""
        ids, val = self._bow(bow)
        self._rc(self.L_lib.orbd_add(self.d, int(tag), int(map_id), _p(ids), _p(val), len(ids), self._members(init)), "orbd_add")

    def add_device(self, tag, map_id, d_bow_id, d_bow_val, d_n_bow, cap, p, init=None, stream=None):
        """add for frame p of a transform_batch_device output, device to device (orbd_add_device)."""
        self._rc(self.L_lib.orbd_add_device(self.d, int(tag), int(map_id), _dp(d_bow_id), _dp(d_bow_val), _dp(d_n_bow), int(cap), int(p),
                                            self._members(init), _dp(stream)), "orbd_add_device")

    def erase(self, tag):
        """KeyFrameDatabase::erase (KeyFrameDatabase.cc:47-66)."""
        self._rc(self.L_lib.orbd_erase(self.d, int(tag)), "orbd_erase")

    def clear(self):
        """KeyFrameDatabase::clear (KeyFrameDatabase.cc:68-72)."""
        self._rc(self.L_lib.orbd_clear(self.d), "orbd_clear")

    def clear_map(self, map_id):
        """KeyFrameDatabase::clearMap (KeyFrameDatabase.cc:74-98)."""
        self._rc(self.L_lib.orbd_clear_map(self.d, int(map_id)), "orbd_clear_map")

    def set_map(self, tag, map_id):
        self._rc(self.L_lib.orbd_set_map(self.d, int(tag), int(map_id)), "orbd_set_map")

    def members(self, tag):
        """mnRelocQuery, mRelocScore, mnPlaceRecognitionQuery, mPlaceRecognitionScore as the handle holds them."""
        m = KfdbMembersStruct()
        self._rc(self.L_lib.orbd_get_members(self.d, int(tag), C.byref(m)), "orbd_get_members")
        return dict(reloc_query=m.reloc_query, place_query=m.place_query, reloc_score=np.float32(m.reloc_score),
                    place_score=np.float32(m.place_score))

    def _query(self, name, query_id, connected, bow):
        ids, val = self._bow(bow)
        cap = self.capacity          # not len(self): another thread may add between the two calls
        tags, scores = np.zeros(cap, np.uint64), np.zeros(cap, np.float32)
        ns, mx, mn, nl = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        tail = (_p(ids), _p(val), len(ids), _p(tags), _p(scores), cap, C.byref(ns), C.byref(mx), C.byref(mn), C.byref(nl))
        if connected is None:
            rc = getattr(self.L_lib, name)(self.d, int(query_id), *tail)
        else:
            con = np.ascontiguousarray(connected, dtype=np.uint64).reshape(-1)
            rc = getattr(self.L_lib, name)(self.d, int(query_id), _p(con), len(con), *tail)
        self._rc(rc, name)
        return dict(tags=tags[:ns.value].copy(), scores=scores[:ns.value].copy(), max_common=mx.value, min_common=mn.value,
                    n_listed=nl.value)

    def query_reloc(self, query_id, bow):
        """The device part of DetectRelocalizationCandidates (KeyFrameDatabase.cc:816-871): lScoreAndMatch as tags / scores in the
        reference's order, max_common, min_common, n_listed.  Raises on a device = -1 handle: there is no host fallback."""
        return self._query("orbd_query_reloc", query_id, None, bow)

    def query_reloc_host(self, query_id, bow):
        return self._query("orbd_query_reloc_host", query_id, None, bow)

    def query_place(self, query_id, connected, bow):
        """The device part of DetectNBestCandidates (KeyFrameDatabase.cc:627-711); connected: pKF->GetConnectedKeyFrames() as tags."""
        return self._query("orbd_query_place", query_id, list(connected), bow)

    def query_place_host(self, query_id, connected, bow):
        return self._query("orbd_query_place_host", query_id, list(connected), bow)

    @staticmethod
    def _covisibles(tags, covisibles_of):
        table = np.full((max(len(tags), 1), COVISIBLES), NO_TAG, np.uint64)
        for i, t in enumerate(tags):
            row = list(covisibles_of(int(t)))[:COVISIBLES]
            table[i, :len(row)] = row
        return table

    def accumulate_reloc(self, query_id, map_id, scored, covisibles_of):
        """KeyFrameDatabase.cc:873-923 on a query_reloc result; covisibles_of(tag) = GetBestCovisibilityKeyFrames(10) as tags.
        Returns vpRelocCandidates as tags."""
        tags = np.ascontiguousarray(scored["tags"], dtype=np.uint64)
        scores = np.ascontiguousarray(scored["scores"], dtype=np.float32)
        table = self._covisibles(tags, covisibles_of)
        out, n = np.zeros(max(len(tags), 1), np.uint64), C.c_int32(-1)
        self._rc(self.L_lib.orbd_accumulate_reloc(self.d, int(query_id), int(map_id), _p(tags), _p(scores), len(tags), _p(table), _p(out),
                                                  C.byref(n)), "orbd_accumulate_reloc")
        return [int(t) for t in out[:n.value]]

    def accumulate_place(self, query_id, scored, covisibles_of):
        """KeyFrameDatabase.cc:713-748 on a query_place result: lAccScoreAndMatch after the sort, as (accScore [n] float32, tags [n])."""
        tags = np.ascontiguousarray(scored["tags"], dtype=np.uint64)
        scores = np.ascontiguousarray(scored["scores"], dtype=np.float32)
        table = self._covisibles(tags, covisibles_of)
        acc, best = np.zeros(max(len(tags), 1), np.float32), np.zeros(max(len(tags), 1), np.uint64)
        self._rc(self.L_lib.orbd_accumulate_place(self.d, int(query_id), _p(tags), _p(scores), len(tags), _p(table), _p(acc), _p(best)),
                 "orbd_accumulate_place")
        return acc[:len(tags)].copy(), [int(t) for t in best[:len(tags)]]

    @staticmethod
    def take_n_best(sorted_acc, n_candidates, query_map, map_of, is_bad=lambda tag: False, map_is_bad=lambda m: False):
        """The take loop of KeyFrameDatabase.cc:760-783 over accumulate_place's list: (vpLoopCand, vpMergeCand).  As written, the
        reference's loop never advances past a bad keyframe (:764-765); this one skips it."""
        loop, merge, seen = [], [], set()
        for t in sorted_acc[1]:
            if not (len(loop) < n_candidates or len(merge) < n_candidates):
                break
            if is_bad(t):
                continue
            if t not in seen:
                if map_of(t) == query_map and len(loop) < n_candidates:
                    loop.append(t)
                elif map_of(t) != query_map and len(merge) < n_candidates and not map_is_bad(map_of(t)):
                    merge.append(t)
                seen.add(t)
        return loop, merge

    def DetectRelocalizationCandidates(self, query_id, bow, covisibles_of, map_id, host=False):
        """KeyFrameDatabase::DetectRelocalizationCandidates (KeyFrameDatabase.cc:814-926): vpRelocCandidates as tags."""
        scored = (self.query_reloc_host if host else self.query_reloc)(query_id, bow)
        if len(scored["tags"]) == 0:
            return []
        return self.accumulate_reloc(query_id, map_id, scored, covisibles_of)

    def DetectNBestCandidates(self, query_id, connected, bow, covisibles_of, n_candidates, query_map, map_of, is_bad=lambda tag: False,
                              map_is_bad=lambda m: False, host=False):
        """KeyFrameDatabase::DetectNBestCandidates (KeyFrameDatabase.cc:620-811): (vpLoopCand, vpMergeCand) as tags."""
        scored = (self.query_place_host if host else self.query_place)(query_id, connected, bow)
        if len(scored["tags"]) == 0:
            return [], []
        return self.take_n_best(self.accumulate_place(query_id, scored, covisibles_of), n_candidates, query_map, map_of, is_bad, map_is_bad)

    def batch_scratch_bytes(self, nq):
        return int(self.L_lib.orbd_batch_scratch_bytes(self.d, int(nq)))

    def score_batch_device(self, query_ids, d_bow_id, d_bow_val, d_n_bow, cap, d_out_tag, d_out_score, out_cap, d_counts, d_scratch,
                           stream=None):
        """The relocalisation query for len(query_ids) resident BowVectors (orbd_score_batch_device): device addresses (ints),
        asynchronous on `stream`; reads the handle's query ids and does not update them.  d_out_tag / d_out_score [nq][out_cap],
        d_counts [nq][4] = max_common, min_common, scored, listed; d_scratch: batch_scratch_bytes(nq) bytes."""
        q = np.ascontiguousarray(query_ids, dtype=np.uint64).reshape(-1)
        rc = self.L_lib.orbd_score_batch_device(self.d, len(q), _p(q), _dp(d_bow_id), _dp(d_bow_val), _dp(d_n_bow), int(cap), _dp(d_out_tag),
                                                _dp(d_out_score), int(out_cap), _dp(d_counts), _dp(d_scratch), _dp(stream))
        return self._rc(rc, "orbd_score_batch_device")
