"""A synthetic keyframe pair for SearchForTriangulation between KannalaBrandt8 keyframes and two-camera KannalaBrandt8 rigs
(ORBmatcher.cc:981-1222 with KannalaBrandt8::epipolarConstrain at :1148), built without images.  A helper, not a conftest.

n points on rays unproject(CAM1, u, v), u, v in [60, 452], at log-uniform depths of 1-8 m in front of KF1's left camera, which is the
world frame.  KF2's camera is rotated by 0.03 rad about y and -0.02 rad about x and its centre moved to `centre`.  The calibration
(CAM1, CAM2, TLR) is rig_stereo_model's; every projection is the model's `project` plus up to 0.5 px of noise.  On a rig the camera
that sees a point is drawn per keyframe and point, the right one through Trl * T; the left camera's keypoints come first.
Descriptors are random 256-bit strings, KF2's copy has 0-13 bits flipped in bytes 8..31 only, so that the `_bow` hash of
tests/test_gpu_match.py (bytes 0 and 7) keeps a pair in one node.  Every third point gets 1 to 4 decoys: further KF2 keypoints with
the descriptor of KF2's copy at wrong pixels, listed after it - equal distance and later in the node, so the reference prefers them
and the geometry has to reject them before the right keypoint is reached.  When the epipole lies inside the image every fourth decoy
is put within 25 px of it, for the epipole gate.  Octaves and angles are random, has_mappoint is set for 15 % on both sides."""
import math

import numpy as np

import rig_stereo_model as M

f32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
SIDEWAYS = (-0.30, 0.04, 0.05)     # the epipole lies outside the image
FORWARD = (-0.10, 0.02, -0.30)     # KF2 behind KF1: the epipole lies inside the image


def scale_factors(nlevels=8, scale_factor=1.2):
    """mvScaleFactors of ORBextractor.cc:413-421."""
    out = [f32(1.0)]
    for _ in range(nlevels - 1):
        out.append(f32(float(out[-1]) * float(f32(scale_factor))))
    return np.array(out, f32)


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def make_scene(n, rig, centre=SIDEWAYS, seed=5, max_decoys=4):
    rng = np.random.default_rng(seed)
    Tlr = _pose(M.TLR[:, :3].astype(np.float64), M.TLR[:, 3].astype(np.float64))
    Trl = np.linalg.inv(Tlr)
    ay, ax = 0.03, -0.02
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    T2w = np.linalg.inv(_pose(Ry @ Rx, np.array(centre, np.float64)))
    T1w = np.eye(4)
    cam_T = lambda Tkw, right: (Trl @ Tkw) if right else Tkw          # world -> camera of the keyframe
    cams = (M.CAM1, M.CAM2)
    ep = M.project(M.CAM1, *[M.r(v) for v in (T2w @ np.array([0.0, 0.0, 0.0, 1.0]))[:3]])   # pKF2->mpCamera->project(R2w * Cw1 + t2w), Cw1 = 0
    ep_inside = 0 <= ep[0] < 512 and 0 <= ep[1] < 512

    def see(Tkw, right, X):
        Xc = cam_T(Tkw, right) @ np.append(X, 1.0)
        u, v = M.project(cams[right], *[M.r(t) for t in Xc[:3]])
        a, rad = rng.uniform(0, 2 * math.pi), rng.uniform(0, 0.5)
        return u + rad * math.cos(a), v + rad * math.sin(a)

    rows1, rows2 = [], []           # (right, x, y, descriptor)
    ndecoys = 0
    for i in range(n):
        u, v = rng.uniform(60, 452, 2)
        X = np.array(M.unproject(M.CAM1, u, v)) * math.exp(rng.uniform(math.log(1.0), math.log(8.0)))
        s1, s2 = (int(rng.integers(0, 2)), int(rng.integers(0, 2))) if rig else (0, 0)
        d1 = rng.integers(0, 256, 32, dtype=np.uint8)
        d2 = d1.copy()
        for b in rng.choice(np.arange(64, 256), int(rng.integers(0, 14)), replace=False):
            d2[b // 8] ^= np.uint8(1 << (b % 8))
        rows1.append((s1, *see(T1w, s1, X), d1))
        rows2.append((s2, *see(T2w, s2, X), d2))
        if i % 3 == 0:
            for _ in range(int(rng.integers(1, max_decoys + 1))):
                sd = int(rng.integers(0, 2)) if rig else 0
                if ep_inside and ndecoys % 4 == 3:
                    px, py = ep[0] + rng.uniform(-25, 25), ep[1] + rng.uniform(-25, 25)
                else:
                    px, py = rng.uniform(20, 492, 2)
                rows2.append((sd, px, py, d2))
                ndecoys += 1

    def pack(rows):
        order = sorted(range(len(rows)), key=lambda k: rows[k][0])          # stable: the left camera's keypoints first, each side in order
        keys = np.zeros(len(rows), KP_DTYPE)
        desc = np.zeros((len(rows), 32), np.uint8)
        for o, k in enumerate(order):
            keys["x"][o], keys["y"][o] = rows[k][1], rows[k][2]
            desc[o] = rows[k][3]
        keys["size"] = 31.0
        keys["octave"] = rng.integers(0, 8, len(rows))
        keys["angle"] = rng.uniform(0, 360, len(rows)).astype(f32)
        n_left = sum(1 for r_ in rows if r_[0] == 0)
        return keys, desc, (n_left if rig else -1), (rng.random(len(rows)) < 0.15).astype(np.uint8)

    k1, d1, nl1, mp1 = pack(rows1)
    k2, d2, nl2, mp2 = pack(rows2)
    pairs = [(a, b) for a in (0, 1) for b in (0, 1)] if rig else [(0, 0)]         # ll, lr, rl, rr (:1011-1019)
    T12 = np.stack([(cam_T(T1w, a) @ np.linalg.inv(cam_T(T2w, b)))[:3, :].astype(f32).reshape(12) for a, b in pairs])
    camsA = np.stack([M.CAM1, M.CAM2]) if rig else M.CAM1[None, :]
    return dict(rig=rig, k1=k1, d1=d1, k2=k2, d2=d2, n_left1=nl1, n_left2=nl2, mp1=mp1, mp2=mp2, T12=T12, cams1=camsA, cams2=camsA.copy(),
                ep=(f32(ep[0]), f32(ep[1])), sf=scale_factors(), sigma2=M.LEVEL_SIGMA2)


def bow(desc, nodes):
    """The `_bow` hash of tests/test_gpu_match.py: node id from bytes 0 and 7 of the descriptor."""
    ids = (desc[:, 0].astype(np.int64) >> 2) * 2 + (desc[:, 7].astype(np.int64) >> 7)
    fv = {}
    for i, k in enumerate(ids % nodes):
        fv.setdefault(int(k) * 7 + 3, []).append(i)
    return fv


def predicate(S, log=None):
    """KannalaBrandt8::epipolarConstrain (KannalaBrandt8.cpp:244-247) through the numpy model, with the camera pair of :1115-1145.
    log, a list, receives (idx1, idx2, camera pair, outcome) per evaluation."""
    k1, k2 = S["k1"], S["k2"]

    def pred(i1, i2):
        a = int(S["rig"] and i1 >= S["n_left1"])
        b = int(S["rig"] and i2 >= S["n_left2"])
        z, _, why = M.triangulate_matches(S["cams1"][a], S["cams2"][b], (k1["x"][i1], k1["y"][i1]), (k2["x"][i2], k2["y"][i2]), S["T12"][2 * a + b],
                                          S["sigma2"][k1["octave"][i1]], S["sigma2"][k2["octave"][i2]])
        ok = bool(f32(z) > f32(0.0001))
        if log is not None:
            log.append((i1, i2, 2 * a + b, why))
        return ok
    return pred


def oracle_views(oracle, S, nodes, u_right1=None, u_right2=None, fv1=None, fv2=None, mp=True):
    fv1 = bow(S["d1"], nodes) if fv1 is None else fv1
    fv2 = bow(S["d2"], nodes) if fv2 is None else fv2
    O1 = oracle.OracleKeyFrame(S["k1"], S["d1"], fv1, S["sf"], S["sigma2"], u_right=u_right1, has_mp=S["mp1"] if mp else None)
    O2 = oracle.OracleKeyFrame(S["k2"], S["d2"], fv2, S["sf"], S["sigma2"], u_right=u_right2, has_mp=S["mp2"] if mp else None)
    return O1, O2


def product_views(pkg, S, nodes, u_right1=None, u_right2=None, fv1=None, fv2=None, mp=True):
    fv1 = bow(S["d1"], nodes) if fv1 is None else fv1
    fv2 = bow(S["d2"], nodes) if fv2 is None else fv2
    K1 = pkg.KeyFrameView(S["k1"], S["d1"], fv1, S["sf"], S["sigma2"], u_right=u_right1, has_mappoint=S["mp1"] if mp else None)
    K2 = pkg.KeyFrameView(S["k2"], S["d2"], fv2, S["sf"], S["sigma2"], u_right=u_right2, has_mappoint=S["mp2"] if mp else None)
    return K1, K2


_cache = {}


def scene(n, rig, centre=SIDEWAYS):
    """make_scene, built once per process; the tests leave it unchanged."""
    key = (n, rig, centre)
    if key not in _cache:
        _cache[key] = make_scene(n, rig, centre)
    return _cache[key]
