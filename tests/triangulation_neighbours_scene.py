"""One synthetic Pinhole keyframe and its K neighbours for the one-call SearchForTriangulation (orbm_search_for_triangulation_neighbours;
the loop of LocalMapping::CreateNewMapPoints, LocalMapping.cc:475-583), built without images.  A helper, not a conftest.

n points at depths of 2-10 m in front of KF1, which is the world frame; a neighbour sees a random subset of them from its own pose,
every projection with up to 0.5 px of noise.  Descriptors are random 256-bit strings, a neighbour's copy has 0-13 bits flipped in
bytes 8..31 only, so that the node hash of triangulation_kb8_scene.bow (bytes 0 and 7) keeps a pair in one node.  Per neighbour:
  * every third point gets a decoy: a later keypoint with the copy's descriptor at a random pixel - equal distance, later in the node,
    so the reference prefers it and the epipolar gate has to reject it; where the epipole lies inside the image every second decoy is
    put within 8 px of it, for the epipole gate (which only monocular pairs feel);
  * every fifth point gets a twin: a later keypoint with the copy's descriptor at the copy's own pixel - both pass every gate, the
    later one has to win (the tie rule of ORBmatcher.cc:1096-1153: `dist > bestDist -> skip`, update on <=);
  * 60 % of the keypoints are stereo (mvuRight >= 0), 15 % hold a map point, octaves are random below the neighbour's nlevels;
  * `wide` puts 80 keypoints of one node, with descriptors far from everything, IN FRONT of the others: the node's real candidates lie
    beyond position 64, in a wavefront's second trip;
  * kind "nonode": the feature vector uses node ids KF1 does not have; kind "empty": n = 0."""
import math

import numpy as np

import triangulation_kb8_scene as SC

f32 = np.float32
CAM = np.array([458.654, 457.296, 367.215, 248.375], f32)      # Examples/Monocular/EuRoC.yaml
W, H = 752, 480
NODES = 6
WIDE_KEY = 3                                                    # bow() key of descriptors with bytes 0 and 7 zero (node id 0)
MAIN = (("real", 200, 8, True), ("nonode", 120, 5, False), ("empty", 0, 8, False), ("real", 150, 6, False))
REPLAY = (("real", 200, 8, True), ("real", 150, 6, False), ("real", 170, 7, False), ("real", 130, 8, False))
POSES = ((0.02, -0.01, (0.25, 0.03, 0.04)), (-0.03, 0.02, (-0.30, 0.02, -0.05)), (0.01, 0.01, (0.03, -0.02, 0.35)), (0.015, -0.02, (0.20, -0.10, 0.02)))


def _rot(ay, ax):
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    return Ry @ Rx


def _keys(xy, octaves, rng):
    k = np.zeros(len(xy), SC.KP_DTYPE)
    if len(xy):
        k["x"], k["y"] = np.asarray(xy, np.float64)[:, 0], np.asarray(xy, np.float64)[:, 1]
    k["size"] = 31.0
    k["octave"] = octaves
    k["angle"] = rng.uniform(0, 360, len(xy)).astype(f32)
    return k


def make_scene(kinds=MAIN, n1=200, seed=11, nodes=NODES, poses=POSES):
    """dict: k1, d1, ur1, mp1, fv1, sf1, sigma2_1, R1w, t1w, Cw1, cam, and `nbs`, a list of dicts k, d, ur, mp, fv, sf, sigma2, R2w, t2w,
    nlevels, kind, twins (pairs (first, later) of keypoint indices at one pixel with one descriptor).  poses: per neighbour (rotation
    about y, about x, camera centre)."""
    rng = np.random.default_rng(seed)
    uv = np.stack([rng.uniform(40, W - 40, n1), rng.uniform(40, H - 40, n1)], 1)
    z = np.exp(rng.uniform(math.log(2.0), math.log(10.0), n1))
    X = np.stack([(uv[:, 0] - CAM[2]) / CAM[0] * z, (uv[:, 1] - CAM[3]) / CAM[1] * z, z], 1)
    noise = lambda m: rng.uniform(0, 0.5, (m, 1)) * np.stack([np.cos(a := rng.uniform(0, 2 * math.pi, m)), np.sin(a)], 1)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    sf8 = SC.scale_factors(8)
    S = dict(k1=_keys(uv + noise(n1), rng.integers(0, 8, n1), rng), d1=d1, sf1=sf8, sigma2_1=(sf8 * sf8).astype(f32),
             R1w=np.eye(3, dtype=f32), t1w=np.zeros(3, f32), Cw1=np.zeros(3, f32), cam=CAM, nbs=[])
    S["ur1"] = np.where(rng.random(n1) < 0.6, S["k1"]["x"] - f32(9), f32(-1)).astype(f32)
    S["mp1"] = (rng.random(n1) < 0.15).astype(np.uint8)
    S["fv1"] = SC.bow(d1, nodes)
    for j, (kind, n2, nlevels, wide) in enumerate(kinds):
        ay, ax, centre = poses[j]
        R2w = _rot(ay, ax).T
        t2w = -R2w @ np.array(centre, np.float64)
        sf = SC.scale_factors(nlevels)
        nb = dict(kind=kind, nlevels=nlevels, sf=sf, sigma2=(sf * sf).astype(f32), R2w=R2w.astype(f32), t2w=t2w.astype(f32), twins=[])
        xy, desc = [], []
        if kind != "empty":
            if wide:
                for _ in range(80):
                    d = rng.integers(0, 256, 32, dtype=np.uint8)
                    d[0], d[7] = 0, 0
                    xy.append(rng.uniform(20, [W - 20, H - 20]))
                    desc.append(d)
            C2 = nb["R2w"].astype(np.float64) @ S["Cw1"] + nb["t2w"]
            ep = (CAM[0] * C2[0] / C2[2] + CAM[2], CAM[1] * C2[1] / C2[2] + CAM[3])
            ep_inside = C2[2] > 0 and 0 <= ep[0] < W and 0 <= ep[1] < H
            ndecoys = 0
            for i in rng.permutation(n1)[:n2]:
                Xc = R2w @ X[i] + t2w
                p = np.array([CAM[0] * Xc[0] / Xc[2] + CAM[2], CAM[1] * Xc[1] / Xc[2] + CAM[3]]) + noise(1)[0]
                d2 = d1[i].copy()
                for b in rng.choice(np.arange(64, 256), int(rng.integers(0, 14)), replace=False):
                    d2[b // 8] ^= np.uint8(1 << (b % 8))
                first = len(xy)
                xy.append(p)
                desc.append(d2)
                if i % 3 == 0:
                    near = ep_inside and ndecoys % 2 == 1
                    xy.append(np.array(ep) + rng.uniform(-8, 8, 2) if near else rng.uniform(20, [W - 20, H - 20]))
                    desc.append(d2)
                    ndecoys += 1
                if i % 5 == 0:
                    nb["twins"].append((first, len(xy)))
                    xy.append(p)
                    desc.append(d2)
        n = len(xy)
        nb["k"] = _keys(xy, rng.integers(0, nlevels, n), rng)
        nb["d"] = np.array(desc, np.uint8).reshape(n, 32)
        nb["ur"] = np.where(rng.random(n) < 0.6, nb["k"]["x"] - f32(9), f32(-1)).astype(f32)
        for a, b in nb["twins"]:                      # a twin is the same keypoint twice: the same mvuRight too
            nb["ur"][b] = nb["ur"][a]
        nb["mp"] = (rng.random(n) < 0.15).astype(np.uint8)
        for a, b in nb["twins"]:
            nb["mp"][b] = nb["mp"][a]
        fv = SC.bow(nb["d"], nodes) if n else {}
        nb["fv"] = {k + 1000: v for k, v in fv.items()} if kind == "nonode" else fv
        S["nbs"].append(nb)
    return S


def product_kf1(pkg, S, mp=None):
    return pkg.KeyFrameView(S["k1"], S["d1"], S["fv1"], S["sf1"], S["sigma2_1"], u_right=S["ur1"], has_mappoint=S["mp1"] if mp is None else mp)


def product_nb(pkg, nb):
    return pkg.KeyFrameView(nb["k"], nb["d"], nb["fv"], nb["sf"], nb["sigma2"], u_right=nb["ur"], has_mappoint=nb["mp"])


def oracle_kf1(oracle, S, mp=None):
    return oracle.OracleKeyFrame(S["k1"], S["d1"], S["fv1"], S["sf1"], S["sigma2_1"], u_right=S["ur1"], has_mp=S["mp1"] if mp is None else mp)


def oracle_nb(oracle, nb):
    return oracle.OracleKeyFrame(nb["k"], nb["d"], nb["fv"], nb["sf"], nb["sigma2"], u_right=nb["ur"], has_mp=nb["mp"])


def oracle_row(oracle, S, j, mp=None, only_stereo=False, coarse=False):
    """vMatches12 of the reference's per-pair member for neighbour j, as a row [n1] of keypoint indices or -1."""
    nb = S["nbs"][j]
    n, pairs = oracle.search_for_triangulation(oracle_kf1(oracle, S, mp), oracle_nb(oracle, nb), S["R1w"], S["t1w"], nb["R2w"], nb["t2w"], S["Cw1"], S["cam"],
                                               S["cam"], only_stereo=only_stereo, coarse=coarse, check_ori=False)
    row = np.full(len(S["k1"]), -1, np.int32)
    row[pairs[:, 0]] = pairs[:, 1]
    assert n == len(pairs)
    return row


def replay(S, row_of, seed=7):
    """The reference's loop (LocalMapping.cc:475-583, :892): after neighbour j a seeded half of its matched idx1 receive a map point.
    row_of(j, has_mappoint) -> row j as the loop sees it.  Returns the rows and the flags in front of every iteration."""
    rng = np.random.default_rng(seed)
    has = S["mp1"].copy()
    rows, flags = [], []
    for j in range(len(S["nbs"])):
        flags.append(has.copy())
        row = row_of(j, has)
        rows.append(row)
        matched = np.nonzero(row >= 0)[0]
        has = has.copy()
        has[matched[rng.random(len(matched)) < 0.5]] = 1
    return rows, flags


def masked(rows0, S, flags):
    """The masking rule: rows from the state at loop entry, -1 wherever idx1 received a map point in the iterations before."""
    out = []
    for j, row in enumerate(rows0):
        r = np.array(row, np.int32)
        r[(flags[j] != 0) & (S["mp1"] == 0)] = -1
        out.append(r)
    return out


_cache = {}


def scene(kinds=MAIN):
    """make_scene, built once per process; the tests leave it unchanged."""
    if kinds not in _cache:
        _cache[kinds] = make_scene(kinds)
    return _cache[kinds]
