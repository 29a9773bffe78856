"""One list of loop / merge map points and the corrected keyframes of LoopClosing::SearchAndFuse (LoopClosing.cc:2631-2707) for the
one-call Sim3 Fuse (orbm_fuse_sim3_keyframes), built without images.  A helper, not a conftest.

The points, keypoints and groups are those of tests/fuse_keyframes_scene.py (nP = 601, T = 7; that file is imported, not edited).  What
changes is how a target is given: instead of a pose and a camera centre it has Scw = s_t * [R_t | t_t] in float (row 3 = 0 0 0 1), which
ORBmatcher::Fuse(pKF, Scw, ...) decomposes again (ORBmatcher.cc:1672-1677); mvuRight, bf and mvInvLevelSigma2 are not part of a target.

Targets:
  0  Pinhole, 752 x 480, 8 levels of 1.2, s = 1 EXACTLY: Scw is the pose, as the overload that passes GetPose() gives it (:2686)
  1  Pinhole from another pose, s = 0.93
  2  KannalaBrandt8, 512 x 512 bounds, 6 levels of 1.3 (its own level table), s = 1.07
  3  DUP: Pinhole with more keypoints than two LDS chunks of the kernel (2 x 256), s = 1.21; the `dup` points have keypoint A behind a
     cell border at a low index and keypoint B in front of it at an index above 512, with one descriptor and octave: the reference
     answers B, the first of GetFeaturesInArea's walk
  4  kf.n == 0, s = 0.88
  5  a Pinhole target with a valid row of zeros, s = 1.13
  6  a second KannalaBrandt8 target with other parameters, pose and 8 levels of 1.2, s = 0.97

Groups with one gate of the Sim3 overload each (make_scene(undo=group) builds the scene without that one change):
  behind :1702   bounds :1713   range :1722   angle :1728   level :1753   th_low :1768   and dup (target DUP).
The two chi-square groups of the imported scene are ordinary points here: this overload has no such gate."""
import numpy as np

import fuse_keyframes_scene as FS

f32 = np.float32
NP = FS.NP
DUP = FS.DUP
CHUNK = FS.CHUNK
REAL = FS.REAL                                                  # targets that have keypoints and valid points
SCALES = (1.0, 0.93, 1.07, 1.21, 0.88, 1.13, 0.97)
POSE = 0                                                        # the target whose Scw is a pose
GATES = ("behind", "bounds", "range", "angle", "level", "th_low")
GROUPS = FS.GROUPS


def make_scene(undo=None, seed=23):
    """The dict of fuse_keyframes_scene.make_scene with, per target, Scw (4x4 float32) and scale; ur is None everywhere."""
    S = FS.make_scene(undo, seed)
    for t, tg in enumerate(S["targets"]):
        Scw = np.eye(4, dtype=f32)
        Scw[:3] = (f32(SCALES[t]) * tg["Tcw"][:3]).astype(f32)     # s = 1: the pose, bit for bit
        tg["Scw"], tg["scale"], tg["ur"] = Scw, SCALES[t], None
    return S


_cache = {}


def scene(undo=None):
    """make_scene, built once per process; the tests leave it unchanged."""
    if undo not in _cache:
        _cache[undo] = make_scene(undo)
    return _cache[undo]


subset = FS.subset
many_small_targets = FS.many_small_targets


def truncated(S, t, n):
    """Scene with the single target t cut to its first n keypoints."""
    tg = S["targets"][t]
    assert n <= len(tg["k"])
    out = subset(S, [t], np.arange(S["nP"]))
    out["targets"] = [dict(tg, k=np.ascontiguousarray(tg["k"][:n]), d=np.ascontiguousarray(tg["d"][:n]))]
    return out


def product_target(pkg, tg):
    return pkg.FuseSim3Target(pkg.FrameView(tg["k"], tg["d"], tg["bounds"]), tg["sf"], tg["log_sf"], tg["Scw"], tg["cam_type"], tg["cam"])


def oracle_frame(oracle, tg, desc=None):
    k = tg["k"]
    return oracle.OracleFrame(k["x"], k["y"], k["octave"], k["angle"], tg["d"] if desc is None else desc, tg["bounds"], tg["sf"])


def oracle_row(oracle, S, t, th, valid=None, mpdesc=None, frame=None):
    """(nFused, bestIdx, bestDist) of the reference's Sim3 Fuse search for target t of S."""
    tg = S["targets"][t]
    v = S["valid"][t] if valid is None else valid
    if len(tg["k"]) == 0:                                         # vIndices is empty for every point (ORBmatcher.cc:1739)
        return 0, np.full(len(v), -1, np.int32), np.full(len(v), 256, np.int32)
    F = oracle_frame(oracle, tg) if frame is None else frame
    return oracle.fuse_sim3(F, v, S["Xw"], S["normal"], S["mpdesc"] if mpdesc is None else mpdesc, S["max_dist"], S["min_dist"], tg["Scw"], tg["cam"],
                            tg["log_sf"], th, cam_type=tg["cam_type"])


def product_row(pkg, matcher, S, t, th, valid=None, mpdesc=None):
    """The same through the per-target entry orbm_fuse_sim3_cam."""
    tg = S["targets"][t]
    KF = pkg.FrameView(tg["k"], tg["d"], tg["bounds"])
    return matcher.FuseSim3(KF, tg["sf"], tg["log_sf"], S["valid"][t] if valid is None else valid, S["Xw"], S["normal"],
                            S["mpdesc"] if mpdesc is None else mpdesc, S["max_dist"], S["min_dist"], tg["Scw"], tg["cam"], th, cam_type=tg["cam_type"])
