"""One list of map points and the target keyframes of LocalMapping::SearchInNeighbors (LocalMapping.cc:909-1058) for the one-call Fuse
(orbm_fuse_keyframes), built without images.  A helper, not a conftest.

nP = 601 points at depths of 2-10 m in front of the world origin; every target looks at them from its own pose, with its own camera,
bounds and scale tables.  A target's keypoints are the projections of the points it sees (80 % of them), within 0.4 px, at an octave
inside the predicted level window, with the point's descriptor and 0-13 flipped bits; random keypoints with random descriptors lie
between them.  Every point belongs to one GROUP, which says what was done to it so that one gate of ORBmatcher::Fuse
(ORBmatcher.cc:1455-1622) rejects it; make_scene(undo=group) builds the same scene without that one change, so a test can show that
the gate - and nothing else - is what rejects the group:
  behind      the point is mirrored through the origin: negative depth in every target (:1475)
  bounds      the point is moved sideways by 1.6 z: it projects outside every target's image (:1490)
  range       mfMaxDistance is halved: dist3D > 1.2 * max (:1505)
  angle       the normal is flipped (10 % of the points, as in test_fuse_n3): PO . Pn < 0.5 dist (:1514)
  th_low      80 bits of the point's descriptor are flipped: bestDist > TH_LOW (:1622)
  level       the keypoints of the point lie one octave above the window [lvl - 1, lvl] (or two below) (:1555)
  chi2_mono   the keypoints (mvuRight < 0) lie 2.6 sigma beside the projection: e2 / sigma2 = 6.76 > 5.99 (:1600-1606)
  chi2_stereo in targets with mvuRight: keypoint and right coordinate lie 2 sigma beside: e2 / sigma2 = 8 > 7.8, where the
              two-term error, 4, would pass 5.99 (:1585-1597); elsewhere the point is an ordinary one
  dup         defined through target DUP (below); elsewhere ordinary

Targets (T = 7):
  0  Pinhole, monocular, 752 x 480, 8 levels of 1.2
  1  Pinhole with mvuRight on 60 % of the keypoints (bf = 47.9): both chi-square limits are reached
  2  KannalaBrandt8, 512 x 512 bounds, 6 levels of 1.3: its own tables and bounds
  3  DUP: Pinhole, more keypoints than two chunks of k_fuse_keyframes (2 x 256).  Every `dup` point projects onto the border of two grid
     cells; it has keypoint A one pixel behind the border, at an index below 16, and keypoint B one pixel in front of it, at an index
     above 512, with ONE descriptor and octave: equal distance, both pass every gate.  GetFeaturesInArea walks B's cell first (ix outer,
     iy inner), so the reference answers B - against the lower index and the earlier chunk.  undo = "dup" gives B a random descriptor.
  4  kf.n == 0
  5  a target like 0 from another pose, with a valid row of zeros
  6  the right image of a KannalaBrandt8 rig whose left image is target 2: raw keypoints, the descriptor rows behind NLeft, the right
     camera's pose and parameters (the caller adds n_left to the indices; nothing in the search does)"""
import math

import numpy as np

f32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
NP = 601
DUP = 3
CHUNK = 256                                                     # FUSE_CH of csrc/orb_fuse_kernels.h
PIN = np.array([458.654, 457.296, 367.215, 248.375], f32)       # Examples/Monocular/EuRoC.yaml
KB8 = np.array([190.978477 * 2, 190.973307 * 2, 256.0, 256.0, 0.003482389402, 0.000715034845, -0.002053236141, 0.000202936736], f32)
KB8_R = np.array([190.442369 * 2, 190.434438 * 2, 252.59, 254.94, 0.003400412, 0.001766799, -0.002663367, 0.000329907], f32)
GROUPS = ("none", "behind", "bounds", "range", "angle", "th_low", "level", "chi2_mono", "chi2_stereo", "dup")
GROUP_P = (0.53, 0.03, 0.03, 0.04, 0.10, 0.04, 0.06, 0.06, 0.09, 0.02)
REAL = (0, 1, 2, 3, 6)                                          # targets that have keypoints and valid points
# per target: kind, bounds, levels, factor, with mvuRight, rotation about y / x, camera centre
TARGETS = (("pin", (0.0, 752.0, 0.0, 480.0), 8, 1.2, False, 0.010, -0.005, (0.12, 0.02, 0.03)),
           ("pin", (0.0, 752.0, 0.0, 480.0), 8, 1.2, True, -0.012, 0.008, (-0.15, 0.01, -0.04)),
           ("kb8", (0.0, 512.0, 0.0, 512.0), 6, 1.3, False, 0.020, 0.010, (0.05, -0.06, 0.10)),
           ("pin", (0.0, 752.0, 0.0, 480.0), 8, 1.2, False, 0.004, 0.012, (0.08, 0.07, -0.02)),
           ("empty", (0.0, 752.0, 0.0, 480.0), 8, 1.2, False, 0.0, 0.0, (0.0, 0.0, 0.0)),
           ("pin", (0.0, 752.0, 0.0, 480.0), 8, 1.2, False, -0.006, -0.010, (-0.05, -0.08, 0.06)),
           ("kb8r", (0.0, 512.0, 0.0, 512.0), 8, 1.2, False, 0.020, 0.010, (0.05, -0.06, 0.10)))
TRL = (0.004, -0.003, (-0.101, 0.002, 0.001))                   # right camera of the rig from its left one: rotation y / x, translation


def scale_factors(nlevels, factor):
    sf = np.ones(nlevels, f32)
    for i in range(1, nlevels):
        sf[i] = f32(sf[i - 1] * f32(factor))
    return sf


def _rot(ay, ax):
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    return Ry @ Rx


def _project(kind, cam, Xc):
    """Pinhole / KannalaBrandt8 projection in double (where keypoints are put; the searches do their own in float)."""
    cam = cam.astype(np.float64)
    x, y, z = Xc[..., 0], Xc[..., 1], Xc[..., 2]
    if kind == "pin":
        return np.stack([cam[0] * x / z + cam[2], cam[1] * y / z + cam[3]], -1)
    th, psi = np.arctan2(np.sqrt(x * x + y * y), z), np.arctan2(y, x)
    r = th + cam[4] * th ** 3 + cam[5] * th ** 5 + cam[6] * th ** 7 + cam[7] * th ** 9
    return np.stack([cam[0] * r * np.cos(psi) + cam[2], cam[1] * r * np.sin(psi) + cam[3]], -1)


def _flip(d, bits, rng):
    d = d.copy()
    for b in rng.choice(256, bits, replace=False):
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def make_scene(undo=None, seed=23):
    """dict: nP, Xw, normal, mpdesc, max_dist, min_dist, group [nP] (index into GROUPS), valid [T][nP], targets: list of dicts k, d, ur
    (or None), bounds, sf, inv_sigma2, log_sf, nlevels, Tcw, Ow, cam_type, cam, bf, n_left (rig right image: what the caller adds), and
    for target DUP dupA / dupB {point: keypoint index}."""
    rng = np.random.default_rng(seed)
    group = rng.choice(len(GROUPS), NP, p=GROUP_P)
    G = lambda name: GROUPS.index(name)
    on = lambda name: undo != name
    sf8 = scale_factors(8, 1.2)
    # the pose of target DUP first: its `dup` points are defined through its image
    poses = []
    for kind, bounds, nlevels, factor, stereo, ay, ax, centre in TARGETS:
        R = _rot(ay, ax).T
        t = -R @ np.array(centre, np.float64)
        if kind == "kb8r":                                         # Trw = Trl * Tlw
            Rrl, trl = _rot(TRL[0], TRL[1]), np.array(TRL[2], np.float64)
            R, t = Rrl @ R, Rrl @ t + trl
        poses.append((R, t))
    uv = np.stack([rng.uniform(60, 752 - 60, NP), rng.uniform(50, 480 - 50, NP)], 1)
    z = np.exp(rng.uniform(math.log(2.0), math.log(10.0), NP))
    X = np.stack([(uv[:, 0] - PIN[2]) / PIN[0] * z, (uv[:, 1] - PIN[3]) / PIN[1] * z, z], 1)
    cw, ch = 752.0 / 64, 480.0 / 48
    dup_axis = {}
    Rd, td = poses[DUP]
    for n_, i in enumerate(np.nonzero(group == G("dup"))[0]):
        axis = n_ % 2                                              # border between two columns (ix) / two rows (iy) of the grid
        p = uv[i].copy()
        p[axis] = (math.floor(p[axis] / (cw, ch)[axis]) + 0.5) * (cw, ch)[axis]   # PosInGrid rounds: cell borders lie at (k + 0.5) cells
        Xc = np.array([(p[0] - PIN[2]) / PIN[0] * z[i], (p[1] - PIN[3]) / PIN[1] * z[i], z[i]])
        X[i] = Rd.T @ (Xc - td)
        dup_axis[int(i)] = axis
    oct_ref = rng.integers(0, 8, NP)
    oct_ref[group == G("dup")] = rng.integers(3, 7, int((group == G("dup")).sum()))   # sigma large enough for the pixel beside the border
    dist_ref = np.linalg.norm(X, axis=1)
    max_dist0 = dist_ref * sf8[oct_ref]
    mpdesc0 = rng.integers(0, 256, (NP, 32), dtype=np.uint8)
    normal = X / dist_ref[:, None]
    Xt, max_dist, mpdesc = X.copy(), max_dist0.copy(), mpdesc0.copy()
    if on("behind"):
        Xt[group == G("behind")] *= -1.0
    if on("bounds"):
        Xt[group == G("bounds"), 0] += 1.6 * z[group == G("bounds")]
    if on("range"):
        max_dist[group == G("range")] *= 0.5
    if on("angle"):
        normal[group == G("angle")] *= -1.0
    far = np.array([_flip(d, 80, rng) for d in mpdesc0])           # drawn for every point: the stream does not depend on `undo`
    if on("th_low"):
        mpdesc[group == G("th_low")] = far[group == G("th_low")]
    S = dict(nP=NP, Xw=Xt.astype(f32), normal=normal.astype(f32), mpdesc=mpdesc, max_dist=max_dist.astype(f32),
             min_dist=(max_dist0 / sf8[7]).astype(f32), group=group, targets=[])
    valid = (rng.random((len(TARGETS), NP)) < 0.9).astype(np.uint8)
    valid[5] = 0
    S["valid"] = valid
    for t, (kind, bounds, nlevels, factor, stereo, ay, ax, centre) in enumerate(TARGETS):
        R, tv = poses[t]
        sf = scale_factors(nlevels, factor)
        cam = {"pin": PIN, "kb8": KB8, "kb8r": KB8_R, "empty": PIN}[kind]
        Tcw = np.eye(4)
        Tcw[:3, :3], Tcw[:3, 3] = R, tv
        Tcw = Tcw.astype(f32)
        Ow = (-Tcw[:3, :3].T.astype(np.float64) @ Tcw[:3, 3].astype(np.float64)).astype(f32)
        tg = dict(kind=kind, bounds=bounds, sf=sf, inv_sigma2=(f32(1) / (sf * sf)).astype(f32), log_sf=float(np.log(f32(factor))), nlevels=nlevels,
                  Tcw=Tcw, Ow=Ow, cam_type=0 if kind in ("pin", "empty") else 1, cam=cam, bf=47.9 if stereo else 0.0, n_left=0, dupA={}, dupB={})
        xy, octs, desc, ur = [], [], [], []
        late = []                                                  # keypoints B of target DUP: appended behind everything else

        def put(p, o, d, r=-1.0):
            xy.append(p), octs.append(o), desc.append(d), ur.append(r)

        if kind != "empty":
            Xc = X @ R.T + tv                                      # the UNtampered points: where their keypoints lie
            pk = "pin" if kind == "pin" else "kb8"
            proj = _project(pk, cam, Xc)
            dist = np.linalg.norm(X - (-R.T @ tv), axis=1)
            lvl = np.clip(np.ceil(np.log(max_dist0 / dist) / math.log(factor)), 0, nlevels - 1).astype(int)
            see = rng.random(NP) < 0.8
            ang = rng.uniform(0, 2 * math.pi, NP)
            noise = rng.uniform(0, 0.4, (NP, 1)) * np.stack([np.cos(ang), np.sin(ang)], 1)
            low = rng.random(NP) < 0.4                             # octave lvl - 1 instead of lvl
            has_ur = rng.random(NP) < 0.6
            nflip = rng.integers(0, 14, NP)
            if t == DUP:
                for i, axis in dup_axis.items():
                    o = int(lvl[i])
                    d = _flip(mpdesc0[i], int(nflip[i]), rng)
                    e = np.zeros(2)
                    e[axis] = 1.0
                    tg["dupA"][i] = len(xy)
                    put(proj[i] + e, o, d)                         # behind the border: the later cell, the lower index
                    other = rng.integers(0, 256, 32, dtype=np.uint8)
                    late.append((i, proj[i] - e, o, d if on("dup") else other))
            for i in range(NP):
                inside = Xc[i, 2] > 0.5 and bounds[0] + 20 <= proj[i, 0] < bounds[1] - 20 and bounds[2] + 20 <= proj[i, 1] < bounds[3] - 20
                if rng.random() < 0.35:                            # a stray keypoint
                    put(np.array([rng.uniform(bounds[0] + 5, bounds[1] - 5), rng.uniform(bounds[2] + 5, bounds[3] - 5)]), int(rng.integers(0, nlevels)),
                        rng.integers(0, 256, 32, dtype=np.uint8), -1.0)
                if not (see[i] and inside) or (t == DUP and i in dup_axis):
                    continue
                g = GROUPS[group[i]]
                d = _flip(mpdesc0[i], int(nflip[i]), rng)
                o = int(lvl[i] - 1) if low[i] and lvl[i] > 0 else int(lvl[i])
                p = proj[i] + noise[i]
                r = float(p[0] - 47.9 / Xc[i, 2]) if stereo and has_ur[i] else -1.0
                if g == "level" and on("level"):
                    o = int(lvl[i] + 1) if lvl[i] + 1 < nlevels else int(lvl[i] - 2)
                    if o < 0:
                        continue
                if g == "chi2_mono":
                    r = -1.0
                    p = proj[i] + (np.array([2.6 * float(sf[o]), 0.0]) if on("chi2_mono") else 0.0)
                if g == "chi2_stereo" and stereo:
                    s2 = 2.0 * float(sf[o]) if on("chi2_stereo") else 0.0
                    p = proj[i] + np.array([s2, 0.0])
                    r = float(proj[i, 0] - 47.9 / Xc[i, 2] - s2)   # ur - kp_ur = +2 sigma as well
                put(p, o, d, r)
            for i, p, o, d in late:
                tg["dupB"][i] = len(xy)
                put(p, o, d)
        n = len(xy)
        k = np.zeros(n, KP_DTYPE)
        if n:
            a = np.asarray(xy, np.float64)
            k["x"], k["y"] = a[:, 0], a[:, 1]
        k["size"], k["octave"], k["class_id"] = 31.0, np.asarray(octs, np.int32) if n else 0, -1
        k["angle"] = rng.uniform(0, 360, n).astype(f32)
        tg["k"], tg["d"] = k, np.asarray(desc, np.uint8).reshape(n, 32)
        tg["ur"] = np.asarray(ur, f32) if stereo else None
        S["targets"].append(tg)
    S["targets"][6]["n_left"] = len(S["targets"][2]["k"])
    return S


_cache = {}


def scene(undo=None):
    """make_scene, built once per process; the tests leave it unchanged."""
    if undo not in _cache:
        _cache[undo] = make_scene(undo)
    return _cache[undo]


def subset(S, targets, points):
    """The scene restricted to some targets and points (a view with its own arrays)."""
    points = np.asarray(points)
    out = dict(S, nP=len(points), targets=[S["targets"][t] for t in targets], valid=np.ascontiguousarray(S["valid"][np.asarray(targets)][:, points]))
    for key in ("Xw", "normal", "mpdesc", "max_dist", "min_dist", "group"):
        out[key] = np.ascontiguousarray(S[key][points])
    return out


def many_small_targets(S, rows, T=12, nP=5, order=(0, 1, 2, 3, 6), all_ur=False):
    """T targets of 3 to 8 keypoints and nP points out of S: a call whose staged block has more parts than the 32 it holds inline.
    The targets are copies of the targets `order` in turn, copy c cut to the keypoints that the reference gives to the chosen points
    (rows[t] = oracle_row of the full target t) and the first of its other keypoints up to 3 + c % 6; the points are the first nP that
    the first two targets of `order` both take, so each of their copies still fuses all of them.  all_ur: a target without mvuRight
    gets one of all -1 (every keypoint monocular), so that every target brings three arrays."""
    both = np.nonzero((rows[order[0]][1] >= 0) & (rows[order[1]][1] >= 0))[0][:nP]
    assert len(both) == nP
    out = subset(S, [order[c % len(order)] for c in range(T)], both)
    small = []
    for c, tg in enumerate(out["targets"]):
        hits = sorted({int(v) for v in rows[order[c % len(order)]][1][both] if v >= 0})
        rest = [i for i in range(len(tg["k"])) if i not in hits]
        sel = np.array(sorted(hits + rest[:max(0, 3 + c % 6 - len(hits))]))
        ur = tg["ur"][sel] if tg["ur"] is not None else (np.full(len(sel), -1, f32) if all_ur else None)
        small.append(dict(tg, k=np.ascontiguousarray(tg["k"][sel]), d=np.ascontiguousarray(tg["d"][sel]), ur=ur, dupA={}, dupB={}))
    out["targets"] = small
    return out


def product_target(pkg, tg):
    return pkg.FuseTarget(pkg.FrameView(tg["k"], tg["d"], tg["bounds"], u_right=tg["ur"]), tg["sf"], tg["inv_sigma2"], tg["log_sf"], tg["Tcw"], tg["Ow"],
                          tg["cam_type"], tg["cam"], tg["bf"])


def oracle_frame(oracle, tg, desc=None):
    k = tg["k"]
    return oracle.OracleFrame(k["x"], k["y"], k["octave"], k["angle"], tg["d"] if desc is None else desc, tg["bounds"], tg["sf"], u_right=tg["ur"])


def oracle_row(oracle, S, t, th, valid=None, mpdesc=None, frame=None):
    """(nFused, bestIdx, bestDist) of the reference's Fuse search for target t of S."""
    tg = S["targets"][t]
    v = S["valid"][t] if valid is None else valid
    if len(tg["k"]) == 0:                                         # vIndices is empty for every point (ORBmatcher.cc:1530)
        return 0, np.full(len(v), -1, np.int32), np.full(len(v), 256, np.int32)
    F = oracle_frame(oracle, tg) if frame is None else frame
    return oracle.fuse(F, v, S["Xw"], S["normal"], S["mpdesc"] if mpdesc is None else mpdesc, S["max_dist"], S["min_dist"], tg["Tcw"], tg["Ow"],
                       tg["cam_type"], tg["cam"], tg["bf"], tg["inv_sigma2"], tg["log_sf"], th)


def product_row(pkg, matcher, S, t, th, valid=None, mpdesc=None):
    """The same through the per-target entry orbm_fuse."""
    tg = S["targets"][t]
    KF = pkg.FrameView(tg["k"], tg["d"], tg["bounds"], u_right=tg["ur"])
    return matcher.Fuse(KF, tg["sf"], tg["inv_sigma2"], tg["log_sf"], S["valid"][t] if valid is None else valid, S["Xw"], S["normal"],
                        S["mpdesc"] if mpdesc is None else mpdesc, S["max_dist"], S["min_dist"], tg["Tcw"], tg["Ow"], tg["cam_type"], tg["cam"], tg["bf"], th)
