"""Scenes for the device form of LocalMapping::CreateNewMapPoints (orbm_create_new_map_points*, orbm_new_point_geometry*), built without
images.  A helper, not a conftest.

  * pinhole(kinds, ...): triangulation_neighbours_scene (n1 = 200, K = 4, 120-200 keypoints per neighbour) with what the body reads on
    top: poses and centres, mb, mbf, mvDepth = mbf / (x - uRight), mvKeys (mvKeysUn moved by a quarter pixel, so that reading the wrong
    array shows).  A share of the stereo keypoints gets the disparity of its true depth - the base scene's constant 9 px makes most
    stereo pairs fail the stereo reprojection test - and some of the others a far or non-positive depth.
  * kb8(rig): the K = 3 scenes of test_triangulation_neighbours_abi.kb8_scenes with the poses of triangulation_kb8_scene.make_scene, for
    rigs the right cameras' through Trl.
  * planted(): groups of hand-made pairs (keyframe constants, keypoint records) that reach every ORBM_NP_* status; the neighbours are a
    wide-baseline one, a close one (stereo parallax beats the rays'), one straight ahead (a point in front of one camera and behind the
    other), one whose centre is a stereo point of the new keyframe (dist2 == 0) and one with a sheared pose: the homogeneous coordinate
    of a triangulation is exactly 0 only when a column of A is, which orthonormal poses reach only up to rounding.
The records carry the layouts of orbm_new_point_camera_t / orbm_new_point_obs_t (tests/test_new_points_model.py compares them with the
package's)."""
import math

import numpy as np

import new_points_model as NM
import rig_stereo_model as M
import triangulation_kb8_scene as SC
import triangulation_neighbours_scene as NS

f32 = np.float32
CAMERA = np.dtype([("Tcw", "<f4", (2, 12)), ("Ow", "<f4", (2, 3)), ("Twc", "<f4", (12,)), ("cam", "<f4", (2, 8))] +
                  [(k, "<f4") for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")] +
                  [("sf", "<f4", (16,)), ("sigma2", "<f4", (16,)), ("cam_type", "<i4"), ("n_left", "<i4")])
OBS = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4"), ("u_right", "<f4"), ("depth", "<f4"), ("key_x", "<f4"), ("key_y", "<f4"), ("right", "<i4")])
SCALE_FACTOR = f32(1.2)
MB = f32(0.11)
KEY_SHIFT = f32(0.25)


def camera(R, t, cam_type, cams, sf, sigma2, intr=None, mb=0.0, right=None, n_left=-1):
    """A keyframe's constants from its world-to-camera pose (R, t in double); right = (R, t) of a rig's second camera."""
    c = np.zeros((), CAMERA)

    def pose(R_, t_, k):
        c["Tcw"][k] = np.concatenate([np.asarray(R_, np.float64), np.asarray(t_, np.float64).reshape(3, 1)], 1).astype(f32).reshape(12)
        c["Ow"][k] = (-np.asarray(R_, np.float64).T @ np.asarray(t_, np.float64)).astype(f32)
    pose(R, t, 0)
    if right is not None:
        pose(right[0], right[1], 1)
    c["Twc"] = np.concatenate([np.asarray(R, np.float64).T, (-np.asarray(R, np.float64).T @ np.asarray(t, np.float64)).reshape(3, 1)], 1).astype(f32).reshape(12)
    cams = np.asarray(cams, f32).reshape(-1, 4 if cam_type == 0 else 8)
    for k in range(len(cams)):
        c["cam"][k][:cams.shape[1]] = cams[k]
    if intr is not None:
        c["fx"], c["fy"], c["cx"], c["cy"] = intr
        c["invfx"], c["invfy"] = f32(1) / f32(intr[0]), f32(1) / f32(intr[1])
        c["mb"], c["mbf"] = mb, f32(mb) * f32(intr[0])
    c["sf"][:len(sf)], c["sigma2"][:len(sigma2)] = sf, sigma2
    c["cam_type"], c["n_left"] = cam_type, n_left
    return c


def observations(keys_un, u_right, depth, keys, idx, n_left=-1):
    """orbm_new_point_obs_t records of the keypoints idx (LocalMapping.cc:613-632)."""
    idx = np.asarray(idx, np.int64)
    o = np.zeros(len(idx), OBS)
    o["x"], o["y"], o["octave"] = keys_un["x"][idx], keys_un["y"][idx], keys_un["octave"][idx]
    o["u_right"] = -1.0 if n_left != -1 else u_right[idx]
    st = o["u_right"] >= 0
    if st.any():
        o["depth"][st], o["key_x"][st], o["key_y"][st] = depth[idx[st]], keys["x"][idx[st]], keys["y"][idx[st]]
    o["right"] = (idx >= n_left) if n_left != -1 else 0
    return o


def geometry_view(pkg, c, depth=None, keys=None):
    """pkg.KeyFrameGeometry of the constants c."""
    rig = int(c["n_left"]) != -1
    return pkg.KeyFrameGeometry(c["Tcw"][0], c["Ow"][0], c["fx"], c["fy"], c["cx"], c["cy"], c["invfx"], c["invfy"], c["mb"], c["mbf"], Twc=c["Twc"],
                                depth=depth, keys=keys, Tcw_right=c["Tcw"][1] if rig else None, Ow_right=c["Ow"][1] if rig else None)


def model_status(c1, c2, o1, o2, far=False, th_far=0.0, sf1=SCALE_FACTOR):
    """(status [n] uint8, x3D [n, 3] float32, zero where not accepted) of the numpy model."""
    st, X = np.zeros(len(o1), np.uint8), np.zeros((len(o1), 3), f32)
    for i in range(len(o1)):
        st[i], x = NM.geometry(c1, c2, o1[i], o2[i], sf1, far, th_far)
        if x is not None:
            X[i] = x
    return st, X


# ---- Pinhole, mono and stereo mixed: the neighbours scene plus what the body reads -----------------------------------------------------
def _stereo_extras(keys_un, ur, true_z, rng, mbf):
    """mvuRight / mvDepth / mvKeys of one keyframe: true_z[i] > 0 where the keypoint's depth is known (a share gets the true disparity)."""
    ur = ur.copy()
    n = len(keys_un)
    pick = rng.random(n)
    for i in np.nonzero(ur >= 0)[0]:
        if true_z[i] > 0 and pick[i] < 0.6:
            ur[i] = keys_un["x"][i] - f32(mbf) / f32(true_z[i])
    depth = np.where(ur >= 0, f32(mbf) / (keys_un["x"] - ur), f32(-1)).astype(f32)
    odd = np.nonzero((ur >= 0) & (pick > 0.9))[0]
    depth[odd[0::2]] = 0.0          # UnprojectStereo's empty matrix, where that arm is taken
    depth[odd[1::2]] = 4000.0       # a stereo parallax of zero
    keys = keys_un.copy()
    keys["x"] += KEY_SHIFT
    keys["y"] -= KEY_SHIFT
    return ur.astype(f32), depth, keys


def make_pinhole(kinds=NS.REPLAY, n1=200, seed=11, poses=NS.POSES, stereo_share=None):
    S = dict(NS.scene(kinds)) if (n1, seed, poses) == (200, 11, NS.POSES) else NS.make_scene(kinds, n1, seed, poses=poses)
    S["nbs"] = [dict(nb) for nb in S["nbs"]]
    rng = np.random.default_rng(seed + 1000)
    cam = S["cam"]
    mbf = float(MB * cam[0])
    if stereo_share is not None:
        S["ur1"] = np.where(rng.random(len(S["k1"])) < stereo_share, S["k1"]["x"] - f32(9), f32(-1)).astype(f32)
        for nb in S["nbs"]:
            nb["ur"] = np.where(rng.random(len(nb["k"])) < stereo_share, nb["k"]["x"] - f32(9), f32(-1)).astype(f32)
    # KF1 is the world frame and keypoint i the projection of point i, whose depth is make_scene's second draw; the neighbours' stereo
    # keypoints keep the base scene's constant disparity
    redraw = np.random.default_rng(seed)
    redraw.uniform(40, NS.W - 40, n1), redraw.uniform(40, NS.H - 40, n1)
    z1 = np.exp(redraw.uniform(math.log(2.0), math.log(10.0), n1))
    S["c1"] = camera(S["R1w"], S["t1w"], 0, cam, S["sf1"], S["sigma2_1"], intr=cam, mb=MB)
    S["ur1"], S["depth1"], S["keys1"] = _stereo_extras(S["k1"], S["ur1"], z1, rng, mbf)
    S["c2"] = []
    for nb in S["nbs"]:
        nb["ur"], nb["depth"], nb["keys"] = _stereo_extras(nb["k"], nb["ur"], np.full(len(nb["k"]), -1.0), rng, mbf)
        S["c2"].append(camera(nb["R2w"], nb["t2w"], 0, cam, nb["sf"], nb["sigma2"], intr=cam, mb=MB))
    return S


_cache = {}


def pinhole(kinds=NS.REPLAY):
    if kinds not in _cache:
        _cache[kinds] = make_pinhole(kinds)
    return _cache[kinds]


def with_duplicates(base, count):
    """The scene with the first `count` keypoints of KF1 that hold no map point appended once more; built once per base scene."""
    key = ("duplicates", count)
    if key not in base:
        S = {k: v for k, v in base.items() if not isinstance(k, tuple)}
        free = np.nonzero(base["mp1"] == 0)[0][:count]
        for k in ("k1", "d1", "ur1", "mp1", "depth1", "keys1"):
            S[k] = np.concatenate([base[k], base[k][free]])
        S["fv1"] = SC.bow(S["d1"], NS.NODES)
        base[key] = S
    return base[key]


def shared_idx2(points):
    """The entries of a list whose (neighbour, idx2) occurs twice."""
    return [p for p in points if sum(1 for q in points if q[0] == p[0] and q[2] == p[2]) == 2]


def product_pinhole(pkg, S, mp=None):
    """(KF1, G1, [KF2], [G2]) views of a pinhole() scene."""
    K1 = pkg.KeyFrameView(S["k1"], S["d1"], S["fv1"], S["sf1"], S["sigma2_1"], u_right=S["ur1"], has_mappoint=S["mp1"] if mp is None else mp)
    views = [pkg.KeyFrameView(nb["k"], nb["d"], nb["fv"], nb["sf"], nb["sigma2"], u_right=nb["ur"], has_mappoint=nb["mp"]) for nb in S["nbs"]]
    G1 = geometry_view(pkg, S["c1"], S["depth1"], S["keys1"])
    return K1, G1, views, [geometry_view(pkg, c, nb["depth"], nb["keys"]) for c, nb in zip(S["c2"], S["nbs"])]


def pinhole_pairs(S, j, row):
    """Keypoint records of the matched pairs of row j (ascending idx1)."""
    nb = S["nbs"][j]
    i1 = np.nonzero(row >= 0)[0]
    return i1, observations(S["k1"], S["ur1"], S["depth1"], S["keys1"], i1), observations(nb["k"], nb["ur"], nb["depth"], nb["keys"], row[i1])


# ---- KannalaBrandt8: single cameras and rigs ----------------------------------------------------------------------------------------
def make_kb8(Ss, centres):
    """The constants of KF1 and of every neighbour of the scenes Ss (triangulation_kb8_scene.make_scene with these centres)."""
    rig = Ss[0]["rig"]
    Tlr = SC._pose(M.TLR[:, :3].astype(np.float64), M.TLR[:, 3].astype(np.float64))
    Trl = np.linalg.inv(Tlr)
    ay, ax = 0.03, -0.02
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])

    def cam_of(Tkw, S, n_left, cams):
        right = None
        if rig:
            Tr = Trl @ Tkw
            right = (Tr[:3, :3], Tr[:3, 3])
        return camera(Tkw[:3, :3], Tkw[:3, 3], 1, cams, S["sf"], S["sigma2"], right=right, n_left=n_left)

    c1 = cam_of(np.eye(4), Ss[0], Ss[0]["n_left1"], Ss[0]["cams1"])
    c2 = [cam_of(np.linalg.inv(SC._pose(Ry @ Rx, np.array(c, np.float64))), S, S["n_left2"], S["cams2"]) for S, c in zip(Ss, centres)]
    return c1, c2


def kb8_pairs(Ss, j, row):
    S = Ss[j]
    i1 = np.nonzero(row >= 0)[0]
    none = np.zeros(0, f32)
    return (i1, observations(S["k1"], np.full(len(S["k1"]), -1, f32), none, S["k1"], i1, S["n_left1"]),
            observations(S["k2"], np.full(len(S["k2"]), -1, f32), none, S["k2"], row[i1], S["n_left2"]))


# ---- planted pairs: every status ----------------------------------------------------------------------------------------------------
def planted():
    """[(name, c1, c2, obs1, obs2, far_points, th_far_points)]: Pinhole groups that together reach every ORBM_NP_* status but NO_MATCH."""
    cam = NS.CAM
    fx, fy, cx, cy = (float(v) for v in cam)
    mbf = float(MB * cam[0])
    sf = SC.scale_factors(8)
    sig = (sf * sf).astype(f32)
    I = np.eye(3)
    mk = lambda R, t: camera(R, t, 0, cam, sf, sig, intr=cam, mb=MB)
    c1 = mk(I, np.zeros(3))
    wide = mk(NS._rot(0.02, -0.01).T, -NS._rot(0.02, -0.01).T @ np.array([0.25, 0.03, 0.04]))
    close = mk(I, -np.array([0.02, 0.0, 0.0]))
    ahead = mk(I, -np.array([0.5, 0.0, 10.0]))

    def proj(c, X):
        T = c["Tcw"][0].astype(np.float64).reshape(3, 4)
        Xc = T[:, :3] @ X + T[:, 3]
        return fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy, Xc[2]

    def ob(c, X, octave=0, stereo=None, dx=0.0, dy=0.0):
        """The keypoint of X in c, moved by (dx, dy); stereo: None mono, "true" a consistent right coordinate, or a depth to claim."""
        u, v, z = proj(c, np.asarray(X, np.float64))
        o = np.zeros((), OBS)
        o["x"], o["y"], o["octave"], o["u_right"] = u + dx, v + dy, octave, -1.0
        if stereo is not None:
            zs = z if stereo == "true" else float(stereo)
            o["depth"] = zs
            o["u_right"] = o["x"] - f32(mbf / zs) if zs > 0 else o["x"] - f32(9)
            o["key_x"], o["key_y"] = o["x"] + KEY_SHIFT, o["y"] - KEY_SHIFT
        return o

    pack = lambda rows: (np.array([a for a, _ in rows], OBS), np.array([b for _, b in rows], OBS))
    out = []
    P = [np.array([0.4, -0.3, 4.0]), np.array([-1.0, 0.5, 6.0]), np.array([0.8, 0.6, 3.0]), np.array([-0.3, -0.2, 8.5])]
    rows = []
    for X in P:
        rows += [(ob(c1, X), ob(wide, X)),                                  # accepted, mono - mono
                 (ob(c1, X, stereo="true"), ob(wide, X)),                   # accepted, stereo - mono, triangulated
                 (ob(c1, X), ob(wide, X, stereo="true")),                   # accepted, mono - stereo
                 (ob(c1, X, dy=12.0), ob(wide, X)),                         # REPROJ1
                 (ob(c1, X, octave=7, dy=8.0), ob(wide, X)),                # REPROJ2: level 7 forgives 4 px in KF1, level 0 does not
                 (ob(c1, X, stereo=X[2] * 3), ob(wide, X)),                 # REPROJ1_STEREO: the right coordinate claims 3 x the depth
                 (ob(c1, X), ob(wide, X, stereo=X[2] * 3)),                 # REPROJ2_STEREO
                 (ob(c1, X, octave=7), ob(wide, X)),                        # SCALE: ratioDist * ratioFactor < ratioOctave
                 (ob(c1, X), ob(wide, X, octave=7)),                        # SCALE: ratioDist > ratioOctave * ratioFactor
                 (ob(c1, X * 5000), ob(wide, X * 5000))]                    # LOW_PARALLAX: both rays equal, no stereo
    out.append(("wide", c1, wide, *pack(rows), False, 0.0))
    out.append(("wide, far points", c1, wide, *pack(rows), True, 6.0))      # FAR for the points beyond 6 m
    rows = []
    for X in P:
        rows += [(ob(c1, X, stereo="true"), ob(close, X)),                  # UnprojectStereo(idx1): the stereo parallax beats the rays'
                 (ob(c1, X), ob(close, X, stereo="true")),                  # UnprojectStereo(idx2)
                 (ob(c1, X, stereo=0.0), ob(close, X)),                     # EMPTY_STEREO on the first arm
                 (ob(c1, X), ob(close, X, stereo=-1.0)),                    # ... and on the second
                 (ob(c1, X), ob(close, X))]                                 # LOW_PARALLAX
    out.append(("close", c1, close, *pack(rows), False, 0.0))
    rows = [(ob(c1, X), ob(ahead, X)) for X in (np.array([0.0, 0.0, 5.0]), np.array([0.2, 0.1, 6.0]))]          # BEHIND2: in front of KF1 only
    rows += [(ob(c1, X), ob(ahead, X)) for X in (np.array([0.3, 0.0, -3.0]), np.array([-0.2, 0.2, -5.0]))]      # BEHIND1: behind both
    out.append(("ahead", c1, ahead, *pack(rows), False, 0.0))
    # ZERO_DIST: the neighbour's centre IS the point UnprojectStereo(idx1) returns
    o1, o2 = ob(c1, P[0], stereo="true"), ob(close, P[0])
    centre = np.array(NM.unproject_stereo(c1, o1), f32)
    at_point = close.copy()
    at_point["Ow"][0] = centre
    out.append(("centre at the point", c1, at_point, *pack([(o1, o2)]), False, 0.0))
    # ZERO_W: both keypoints at the principal point, a stereo parallax of exactly 1, and a neighbour whose third row is sheared: column 2
    # of A is exactly zero while the rays differ by 1e-3 rad
    sheared = mk(I, -np.array([0.3, 0.1, 0.0]))
    sheared["Tcw"][0][8] = 0.001
    z = np.zeros((), OBS)
    z["x"], z["y"], z["u_right"] = cam[2], cam[3], -1.0
    zs = z.copy()
    zs["depth"], zs["u_right"], zs["key_x"], zs["key_y"] = 5000.0, cam[2] - f32(mbf / 5000.0), cam[2], cam[3]
    out.append(("sheared", c1, sheared, *pack([(zs, z)]), False, 0.0))
    return out


# ---- expected values of the one-call entries: loop-entry tables, the sequential rule, the replay of the reference's loop ---------------
class Expected:
    """For one scene and one setting (coarse, far_points, th_far_points): row_of(j, has_mappoint) -> vMatches12 of neighbour j (the
    oracle's search), pairs_of(j, row) -> (idx1, obs1, obs2), c1 / c2 the constants.  Model results are kept per (j, idx1, idx2)."""

    def __init__(self, K, n1, row_of, pairs_of, c1, c2, mp1, far=False, th_far=0.0):
        self.K, self.n1, self.row_of, self.pairs_of, self.c1, self.c2, self.mp1, self.far, self.th_far = K, n1, row_of, pairs_of, c1, c2, mp1, far, th_far
        self.memo = {}

    def body(self, j, row):
        """status [n1], x3D [n1, 3] of the pairs of `row` of neighbour j."""
        st, X = np.zeros(self.n1, np.uint8), np.zeros((self.n1, 3), f32)
        i1, o1, o2 = self.pairs_of(j, row)
        for k, i in enumerate(i1):
            key = (j, int(i), int(row[i]))
            if key not in self.memo:
                s, x = NM.geometry(self.c1, self.c2[j], o1[k], o2[k], SCALE_FACTOR, self.far, self.th_far)
                self.memo[key] = (s, np.zeros(3, f32) if x is None else np.array(x, f32))
            st[i], X[i] = self.memo[key]
        return st, X

    def tables(self, skip=None):
        """rows [K, n1], nmatches [K], status [K, n1], x3D [K, n1, 3] from the state at loop entry; a skipped neighbour is empty."""
        rows, st, X = np.full((self.K, self.n1), -1, np.int32), np.zeros((self.K, self.n1), np.uint8), np.zeros((self.K, self.n1, 3), f32)
        for j in range(self.K):
            if skip is not None and skip[j]:
                continue
            rows[j] = self.row_of(j, self.mp1)
            st[j], X[j] = self.body(j, rows[j])
        return rows, (rows >= 0).sum(1).astype(np.int32), st, X

    def rule(self, skip=None):
        """The list of the SEQUENTIAL RULE from the loop-entry tables: [(j, idx1, idx2, x3D)]."""
        rows, _, st, X = self.tables(skip)
        return [(j, i1, i2, X[j, i1]) for j, i1, i2 in NM.first_accepted(st, rows)]

    def replay(self, skip=None, stop=None):
        """The reference's loop itself (LocalMapping.cc:525-904) stopped in front of neighbour `stop`: search with the CURRENT map-point
        flags, the body per pair in ascending idx1, AddMapPoint on acceptance."""
        has, out = self.mp1.copy(), []
        for j in range(self.K if stop is None else stop):
            if skip is not None and skip[j]:
                continue
            row = self.row_of(j, has)
            st, X = self.body(j, row)
            for i1 in np.nonzero(st == NM.ACCEPTED)[0]:
                out.append((j, int(i1), int(row[i1]), X[i1]))
                has[i1] = 1
        return out


def same_list(a, b):
    return len(a) == len(b) and all(x[:3] == y[:3] and np.array_equal(x[3].view(np.uint32), y[3].view(np.uint32)) for x, y in zip(a, b))


def as_list(points):
    """A NEW_POINT_DTYPE array as the tuples above."""
    return [(int(p["neighbour"]), int(p["idx1"]), int(p["idx2"]), np.array(p["x3D"], f32)) for p in points]


def expected_pinhole(oracle, S, coarse=False, far=False, th_far=0.0):
    key = ("expected", coarse, far, th_far)
    if key not in S:
        S[key] = Expected(len(S["nbs"]), len(S["k1"]), lambda j, has: NS.oracle_row(oracle, S, j, mp=has, coarse=coarse),
                          lambda j, row: pinhole_pairs(S, j, row), S["c1"], S["c2"], S["mp1"], far, th_far)
    return S[key]


_kb8 = {}


def expected_kb8(oracle, Ss, centres, pred_of, coarse=False, far=False, th_far=0.0):
    """Ss: K scenes that share KF1.  pred_of(S): the numpy model's epipolarConstrain."""
    key = (Ss[0]["rig"], coarse, far, th_far)
    if key not in _kb8:
        c1, c2 = make_kb8(Ss, centres)
        n1 = len(Ss[0]["k1"])

        def row_of(j, has):
            S = dict(Ss[j], mp1=has)
            O1, O2 = SC.oracle_views(oracle, S, 4)
            _, pairs = oracle.search_for_triangulation_pred(O1, O2, S["ep"], not S["rig"], pred_of(S), coarse=coarse, check_ori=False)
            row = np.full(n1, -1, np.int32)
            row[pairs[:, 0]] = pairs[:, 1]
            return row
        _kb8[key] = Expected(len(Ss), n1, row_of, lambda j, row: kb8_pairs(Ss, j, row), c1, c2, Ss[0]["mp1"], far, th_far)
    return _kb8[key]


def product_kb8(pkg, Ss, c1, c2):
    """(KF1, G1, [KF2], [G2]) views of the KannalaBrandt8 scenes."""
    K1, _ = SC.product_views(pkg, Ss[0], 4)
    views = [SC.product_views(pkg, S, 4)[1] for S in Ss]
    return K1, geometry_view(pkg, c1), views, [geometry_view(pkg, c) for c in c2]
