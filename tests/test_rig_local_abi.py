"""CPU: orbm_search_local_points_fisheye and orbm_search_local_points_fisheye_batch_device exist on both sides of the ABI, their
refusals that need no device, the model of tests/rig_local_model.py against closed forms, and the conditions its scenes must meet
for the comparisons of tests/test_gpu_rig_local.py to mean something - judged by model + oracle alone."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import local_map_model as M
import rig_local_model as RL
import rig_model as RM
import test_abi_null
from conftest import ROOT
from oracle import oracle_py

f32 = np.float32
HOST = "orbm_search_local_points_fisheye"
BATCH = "orbm_search_local_points_fisheye_batch_device"


def test_symbols_structs_and_mirrors(pkg):
    L = pkg.load()
    for name, nargs in ((HOST, 24), (BATCH, 35), ("orbm_rig_right_camera", 5)):
        assert name in pkg.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    assert [f[0] for f in pkg.TrackRigStruct._fields_] == [k for k, _ in RL.FIELDS] == [k for k, _ in pkg.TRACK_RIG_FIELDS]
    assert C.sizeof(pkg.TrackRigStruct) == 12 * C.sizeof(C.c_void_p)
    assert [t for _, t in pkg.TRACK_RIG_FIELDS] == [t for _, t in RL.FIELDS]
    sig = inspect.signature(pkg.ORBmatcher.search_local_points_fisheye_batch_device)
    assert list(sig.parameters)[:14] == ["self", "cur0", "frame_stride", "d_frame_n", "frame_n_stride", "d_n_left", "n_left_stride", "d_left_to_right",
                                         "d_right_to_left", "map0", "map_stride", "d_map_n", "map_n_stride", "npairs"]
    assert sig.parameters["n_left"].default == 0 and sig.parameters["stream"].default is None and sig.parameters["bFarPoints"].default is False
    assert "track" in inspect.signature(pkg.ORBmatcher.SearchLocalPointsFisheye).parameters
    with open(os.path.join(ROOT, "include", "orbhip.h")) as f:
        header = f.read()
    assert ("int %s(" % HOST) in header and ("int %s(" % BATCH) in header and "} orbm_track_rig_t;" in header
    decl = header[header.index("} orbm_track_rig_t;") - 600:header.index("} orbm_track_rig_t;")]
    order = [decl.index(k) for k in ("*in_view,", "*in_view_r;", "*proj_x,", "*proj_y,", "*depth,", "*view_cos;", "*proj_xr,", "*proj_yr,", "*depth_r,",
                                     "*view_cos_r;", "*level,", "*level_r;")]
    assert order == sorted(order)


def test_null_sweep_survives_the_new_symbols():
    test_abi_null.test_null_arguments_do_not_crash()


def _batch_args(pkg):
    n, nmp = 6, 4
    A = dict(keys=np.zeros(n, pkg.KP_DTYPE), desc=np.zeros((n, 32), np.uint8), elig=np.ones(nmp, np.uint8), v3=np.zeros((nmp, 3), f32), f=np.ones(nmp, f32),
             md=np.zeros((nmp, 32), np.uint8), T=np.eye(4, dtype=f32), slot=np.full(n, -1, np.int32), sobs=np.zeros(n, np.uint8), nm=np.zeros(1, np.int32))
    A["track"] = {k: np.zeros(nmp, t) for k, t in pkg.TRACK_RIG_FIELDS}
    p = lambda a: a.ctypes.data
    fs = pkg.FrameStruct(n, p(A["keys"]), p(A["desc"]), None, 0.0, 600.0, 0.0, 400.0)
    ms = pkg.LocalMapStruct(nmp, p(A["elig"]), p(A["v3"]), p(A["v3"]), p(A["f"]), p(A["f"]), p(A["md"]), None, p(A["T"]))
    ts = pkg.TrackRigStruct(*[p(A["track"][k]) for k, _ in pkg.TRACK_RIG_FIELDS])
    pin = np.array([400, 400, 300, 200], f32)
    good = dict(cur0=fs, frame_stride=n, d_frame_n=None, frame_n_stride=0, d_n_left=None, n_left_stride=0, d_left_to_right=None, d_right_to_left=None, map0=ms,
                map_stride=nmp, d_map_n=None, map_n_stride=0, npairs=1, scale_factors=np.ones(8, f32), log_scale_factor=0.18, Trl=np.eye(4, dtype=f32),
                tlr=np.zeros(3, f32), cam_type=0, cam_params=pin, cam_type2=0, cam_params2=pin, th=1.0, d_slot=p(A["slot"]), d_slot_obs=p(A["sobs"]),
                d_match_of_point=None, track0=ts, d_nmatches=p(A["nm"]), n_left=3)
    return A, good


def test_refusals_without_device(pkg):
    """The mirror refuses what needs no device before it calls the library; a matcher without a handle stands in for one, so a call
    that passes the mirror's checks reaches the library's own first refusal, the NULL handle."""
    L = pkg.load()
    m = pkg.ORBmatcher.__new__(pkg.ORBmatcher)
    m.L, m.m, m.mfNNratio, m.mbCheckOrientation = L, None, 0.8, True
    A, good = _batch_args(pkg)
    bad = [(dict(Trl=None), "missing"), (dict(tlr=None), "missing"), (dict(Trl=np.eye(3, dtype=f32)), "12 or 16"), (dict(tlr=np.zeros(2, f32)), "12 or 16"),
           (dict(npairs=-1), "npairs"), (dict(d_slot=None), "missing output"), (dict(d_slot_obs=None), "missing output"), (dict(d_nmatches=None), "missing output"),
           (dict(scale_factors=np.ones(17, f32)), "nlevels"), (dict(cam_type=2), "camera"), (dict(cam_type2=2), "camera"), (dict(cam_type2=1), "camera"),
           (dict(n_left=-1), "n_left"), (dict(n_left=7), "n_left"), (dict(frame_stride=pkg.FISHEYE_MAX_KEYPOINTS + 1), "frame_stride")]
    for c, what in bad:
        with pytest.raises(ValueError, match=what):
            m.search_local_points_fisheye_batch_device(**dict(good, **c))
    with pytest.raises(ValueError, match="null handle"):
        m.search_local_points_fisheye_batch_device(**good)
    F = pkg.FrameView(A["keys"], A["desc"], (0.0, 600.0, 0.0, 400.0))
    with pytest.raises(ValueError, match="12 or 16"):
        m.SearchLocalPointsFisheye(F, 3, None, None, np.ones(8, f32), 0.18, A["elig"], A["v3"], A["v3"], A["f"], A["f"], A["md"], A["T"], np.eye(3, dtype=f32),
                                   np.zeros(3, f32), 0, good["cam_params"], 0, good["cam_params"], 1.0)
    with pytest.raises(ValueError, match="null handle"):
        m.SearchLocalPointsFisheye(F, 3, None, None, np.ones(8, f32), 0.18, A["elig"], A["v3"], A["v3"], A["f"], A["f"], A["md"], A["T"], np.eye(4, dtype=f32),
                                   np.zeros(3, f32), 0, good["cam_params"], 0, good["cam_params"], 1.0)
    assert (A["slot"] == -1).all() and (A["nm"] == 0).all() and all((v == 0).all() for v in A["track"].values())


def test_right_camera_host_equals_model(pkg):
    """orbm_rig_right_camera (the expressions the kernel uses, host build) against the model's Frame.cc:1276-1280, bit for bit."""
    rng = np.random.default_rng(4)
    for _ in range(200):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        Tcw = np.eye(4, dtype=f32)
        Tcw[:3, :3], Tcw[:3, 3] = R, rng.normal(size=3)
        Trl = np.eye(4, dtype=f32)
        Trl[:3, :3], Trl[:3, 3] = RL.rot(2, rng.normal() * 0.01) @ RL.rot(1, rng.normal() * 0.05), rng.normal(size=3) * 0.2
        tlr = rng.normal(size=3).astype(f32)
        Tr, twc = pkg.rig_right_camera(Tcw, Trl, tlr)
        Rm, tm, cm = RL.right_camera(Tcw, Trl, tlr)
        assert np.array_equal(Tr[:, :3].view(np.uint32), Rm.view(np.uint32)) and np.array_equal(Tr[:, 3].view(np.uint32), tm.view(np.uint32))
        assert np.array_equal(twc.view(np.uint32), cm.view(np.uint32))


@pytest.mark.parametrize("cam", [0, 1])
def test_model_closed_form(oracle, synth, cam):
    """Trl = I, tlr = 0, cam2 = cam: the right fields equal the left ones, and both equal local_map_model.is_in_frustum where that one
    reports in_view (it resets the projection to -1 and has no level -1; this branch has neither)."""
    S = dict(RL.cached_scene(oracle, synth, cam))
    S.update(Trl=np.eye(4, dtype=f32), tlr=np.zeros(3, f32), cam_params2=S["cam_params"])
    tr = RL.is_in_frustum_rig(S)
    assert np.array_equal(tr["in_view"], tr["in_view_r"]) and np.array_equal(tr["level"], tr["level_r"])
    iv = tr["in_view"] != 0
    for a, b in zip(RL.LEFT[:4], RL.RIGHT[:4]):
        assert np.array_equal(tr[a][iv].view(np.uint32), tr[b][iv].view(np.uint32)), a
    ref = M.is_in_frustum(S["Xw"], S["normal"], S["max_dist"], S["min_dist"], S["eligible"], S["Tcw"], S["cam"], S["cam_params"], S["bounds"], len(S["sf"]),
                          S["log_sf"], 0.0, 0.5, oracle_py.project)
    assert np.array_equal(ref["in_view"], tr["in_view"]) and iv.sum() > 300
    for k in ("proj_x", "proj_y", "depth", "view_cos"):
        assert np.array_equal(ref[k][iv].view(np.uint32), tr[k][iv].view(np.uint32)), k
    assert np.array_equal(ref["level"][iv], tr["level"][iv])
    e = S["eligible"] != 0
    assert (tr["level"][e & ~iv] == -1).all() and (tr["level"][~e] == -777).all() and (tr["proj_x"][~iv] == RL.POISON).all()


@pytest.mark.parametrize("cam", [0, 1])
def test_scene_conditions(oracle, synth, cam):
    """Per problem: at least 20 points seen by the left camera only, the right only, both, neither; 20 accepted right-half matches;
    10 partner writes in each direction; 5 right halves dropped by the `continue` of ORBmatcher.cc:127 (at th = 4)."""
    for p in range(4):
        S = RL.cached_scene(oracle, synth, cam, p)
        for th in (1.0, 4.0):
            E = RL.expected(oracle, S, th)
            cls = RL.classes(E["track"], S["eligible"])
            l2r_writes = int(((E["mL"] >= 0) & (S["l2r"][np.maximum(E["mL"], 0)] >= 0)).sum())
            r2l_writes = int(((E["mR"] >= 0) & (S["r2l"][np.maximum(E["mR"], 0)] >= 0)).sum())
            nright = int((E["mR"] >= 0).sum())
            assert E["n"] == int((E["mL"] >= 0).sum()) + nright + l2r_writes + r2l_writes
            dropped = len(RL.dropped_by_continue(oracle, S, E, th)) if th == 4.0 else None
            print("cam %d problem %d th %g: N %d Nleft %d map %d classes L/R/both/neither %s nmatches %d right %d partner writes %d / %d dropped %s" %
                  (cam, p, th, len(S["kl"]) + len(S["kr"]), len(S["kl"]), len(S["Xw"]), cls, E["n"], nright, l2r_writes, r2l_writes, dropped))
            assert min(cls) >= 20 and nright >= 20 and l2r_writes >= 10 and r2l_writes >= 10
            if th == 4.0:
                assert dropped >= 5


def test_constructed_scene_conditions(oracle, synth):
    """At least one hand-placed point per branch: each of the five rejections on each side, a NaN projection, the far-point skip decided
    by a stale incoming depth, a partner write that releases a claim held with observations, the level clamped at both ends."""
    sf = RM.stream(oracle, synth)[3]
    S, track0, ix = RL.constructed(sf)
    E = RL.expected(oracle, S, 1.0, bFar=True, thFar=10.0, track0=track0)
    tr = E["track"]
    assert set(tr["reason"].tolist()) >= {0, 1, 2, 3, 4, 5} and set(tr["reason_r"].tolist()) >= {0, 1, 2, 3, 4, 5}
    assert tr["reason"][ix["behind_r"]] == 2 and tr["reason_r"][ix["behind_r"]] == 1
    c = ix["centre"]
    assert tr["in_view"][c] == 1 and np.isnan(tr["proj_x"][c]) and tr["raw"][c] == M.INT_MIN and tr["level"][c] == 0 and E["L"][c] == 0
    t = ix["top_level"]
    assert tr["in_view"][t] == 1 and tr["raw"][t] >= len(sf) and tr["level"][t] == len(sf) - 1
    for k in ("left_only", "B"):
        assert tr["in_view"][ix[k]] == 1 and tr["in_view_r"][ix[k]] == 0 and tr["level_r"][ix[k]] == -1 and tr["proj_xr"][ix[k]] == RL.POISON
    for k in ("right_only", "right_only_stale", "A", "C"):
        assert tr["in_view"][ix[k]] == 0 and tr["in_view_r"][ix[k]] == 1 and tr["level"][ix[k]] == -1 and tr["proj_x"][ix[k]] == RL.POISON
    # the stale depth decides: the left check failed, so depth is what the caller passed
    s, r = ix["right_only_stale"], ix["right_only"]
    assert tr["depth"][s] == f32(50.0) and E["R"][s] == 0 and E["mR"][s] == -1 and tr["depth"][r] == f32(1.0) and E["R"][r] == 1 and E["mR"][r] >= 0
    assert RL.expected(oracle, S, 1.0, bFar=False, track0=track0)["mR"][s] >= 0
    assert E["mL"][ix["both"]] >= 0 and E["mR"][ix["both"]] >= 0
    # the release: after A, keypoint b is held with observations; B's partner write leaves it without; C takes it
    nl = len(S["kl"])
    afterA = RL.expected(oracle, S, 1.0, bFar=True, thFar=10.0, track0=track0, upto=ix["A"] + 1)
    assert afterA["slot"][ix["kp_b"]] == ix["A"] and afterA["slot_obs"][ix["kp_b"]] == 1
    afterB = RL.expected(oracle, S, 1.0, bFar=True, thFar=10.0, track0=track0, upto=ix["B"] + 1)
    assert afterB["mL"][ix["B"]] == ix["kp_a"] and afterB["slot"][ix["kp_b"]] == ix["B"] and afterB["slot_obs"][ix["kp_b"]] == 0
    assert E["mR"][ix["C"]] == ix["kp_b"] - nl and E["slot"][ix["kp_b"]] == ix["C"] and E["slot_obs"][ix["kp_b"]] == 1
    nop = RL.expected(oracle, S, 1.0, bFar=True, thFar=10.0, track0=track0, partners=False)
    assert nop["mR"][ix["C"]] == -1 and nop["slot"][ix["kp_b"]] == ix["A"]
