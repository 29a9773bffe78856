"""numpy / float32 restatement of Tracking::SearchLocalPoints for a fisheye-stereo frame (Frame::Nleft != -1), and the scenes
shared by tests/test_rig_local_abi.py (CPU: what the scenes must contain, judged by this model and the oracle alone) and
tests/test_gpu_rig_local.py.

Frustum test: Frame::isInFrustum's else branch (Frame.cc:650-660) = Frame::isInFrustumChecks (Frame.cc:1270-1343) once per camera
with MapPoint::PredictScale (MapPoint.cc:587-602); every step is the IEEE single or double operation of the reference's expression
in source order, with the project's conventions for small cv::Mat products (local_map_model, csrc/orb_ref_geometry.h).  The camera
is the oracle's (oracle.project), log is the host's glibc logf.  Search: the model's track values fed to
OracleFisheyeFrame.search_by_projection_mp (ORBmatcher.cc:44-214).

Scenes follow tests/rig_model.py: the synthetic stream of three 752 x 480 frames (frame 1 the left image, frame 2 the right one),
the keypoints of frame 0 as map points on the rays of the left camera under test."""
import numpy as np

import local_map_model as M
import rig_model as RM

f32 = np.float32
FIELDS = (("in_view", np.uint8), ("in_view_r", np.uint8), ("proj_x", f32), ("proj_y", f32), ("depth", f32), ("view_cos", f32),
          ("proj_xr", f32), ("proj_yr", f32), ("depth_r", f32), ("view_cos_r", f32), ("level", np.int32), ("level_r", np.int32))
LEFT = ("proj_x", "proj_y", "depth", "view_cos", "level")
RIGHT = ("proj_xr", "proj_yr", "depth_r", "view_cos_r", "level_r")
POISON = f32(-777.25)          # a caller's value in a float track field; -777 in a level
PRE_VALUE = 100000             # a caller's local-map index no search of these scenes can write
NNRATIO = 0.8


def mat3_mul_add(R, x, t):
    """cv::Mat A*B + C for 3x3 * 3x1: a0*b0 + a1*b1 + a2*b2 in float, then + C in double (orb_ref_geometry.h mat3_mul_add)."""
    R, x, t = np.asarray(R, f32), np.asarray(x, f32), np.asarray(t, f32)
    out = np.zeros(3, f32)
    for i in range(3):
        t0 = f32(f32(f32(R[i, 0] * x[0]) + f32(R[i, 1] * x[1])) + f32(R[i, 2] * x[2]))
        out[i] = f32(np.float64(t0) + np.float64(t[i]))
    return out


def right_camera(Tcw, Trl, tlr):
    """Frame.cc:1276-1280: (mR = Rrl*mRcw, mt = Rrl*mtcw + trl, twc = mRwc*tlr + mOw)."""
    T, G = np.asarray(Tcw, f32).reshape(4, 4), np.asarray(Trl, f32).reshape(-1, 4)
    tlr = np.asarray(tlr, f32).reshape(-1)
    R = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            R[i, j] = f32(f32(f32(G[i, 0] * T[0, j]) + f32(G[i, 1] * T[1, j])) + f32(G[i, 2] * T[2, j]))
    t = mat3_mul_add(G[:3, :3], T[:3, 3], G[:3, 3])
    twc = mat3_mul_add(T[:3, :3].T, tlr[:3], M.camera_centre(T))
    return R, t, twc


def frustum_checks(P, normal, max_dist, min_dist, R, t, twc, cam_type, cam, bounds, nlevels, log_sf, limit, project):
    """isInFrustumChecks for one point and one camera -> (reason, u, v, level, view_cos, depth, raw level).  reason 0: all checks pass;
    1 PcZ < 0 (:1294), 2 / 3 outside the bounds in x / y (:1302-1305), 4 outside the scale range (:1313), 5 viewCos below the limit (:1321)."""
    min_x, max_x, min_y, max_y = (f32(b) for b in bounds)
    with np.errstate(all="ignore"):
        pc = mat3_mul_add(R, P, t)
        depth = M.norm3(pc)
        if pc[2] < f32(0.0):
            return 1, None, None, -1, None, depth, None
        u, v = (f32(c) for c in project(cam_type, cam, float(pc[0]), float(pc[1]), float(pc[2])))
        if u < min_x or u > max_x:
            return 2, u, v, -1, None, depth, None
        if v < min_y or v > max_y:
            return 3, u, v, -1, None, depth, None
        po = np.asarray(P, f32) - twc
        dist = M.norm3(po)
        if dist < f32(0.8) * min_dist or dist > f32(1.2) * max_dist:
            return 4, u, v, -1, None, depth, None
        d = 0.0
        for k in range(3):
            d += float(po[k]) * float(normal[k])
        vcos = f32(np.float64(d) / np.float64(dist))
        if vcos < f32(limit):
            return 5, u, v, -1, vcos, depth, None
        raw = M.cvtt_f32_i32(np.ceil(M.glibc_logf(max_dist / dist) / f32(log_sf)))
        lvl = 0 if raw < 0 else (nlevels - 1 if raw >= nlevels else raw)
        return 0, u, v, lvl, vcos, depth, raw


def is_in_frustum_rig(S, track0=None, limit=0.5, project=None):
    """The twelve track arrays after Frame::isInFrustum for every local map point of scene S, starting from track0 (the MapPoints'
    current values; default poison), plus the diagnostics reason / reason_r / raw / raw_r (not part of the ABI)."""
    if project is None:
        from oracle import oracle_py
        project = oracle_py.project
    n = len(S["Xw"])
    tr = {k: (np.full(n, -777 if t == np.int32 else (9 if t == np.uint8 else POISON), t) if track0 is None else track0[k].copy()) for k, t in FIELDS}
    T = np.asarray(S["Tcw"], f32).reshape(4, 4)
    Rr, tr_, twc_r = right_camera(T, S["Trl"], S["tlr"])
    sides = ((T[:3, :3], T[:3, 3], M.camera_centre(T), S["cam"], S["cam_params"], "in_view", LEFT, "reason", "raw"),
             (Rr, tr_, twc_r, S["cam2"], S["cam_params2"], "in_view_r", RIGHT, "reason_r", "raw_r"))
    for _, _, _, _, _, _, _, rk, wk in sides:
        tr[rk], tr[wk] = np.full(n, -1, np.int32), np.zeros(n, np.int64)
    nlevels = len(S["sf"])
    for j in range(n):
        tr["in_view"][j] = tr["in_view_r"][j] = 0
        if not S["eligible"][j]:
            continue
        tr["level"][j] = tr["level_r"][j] = -1                                   # :653-654
        for R, t, twc, ct, cp, flag, names, rk, wk in sides:
            reason, u, v, lvl, vcos, depth, raw = frustum_checks(S["Xw"][j], S["normal"][j], S["max_dist"][j], S["min_dist"][j], R, t, twc, ct, cp,
                                                                 S["bounds"], nlevels, S["log_sf"], limit, project)
            tr[rk][j] = reason
            if reason == 0:
                tr[flag][j] = 1
                tr[wk][j] = raw
                for name, val in zip(names, (u, v, depth, vcos, lvl)):
                    tr[name][j] = val
    return tr


def search_masks(S, tr, bFar, thFar):
    """Who takes part (ORBmatcher.cc:53-59) and which halves make a query (:62, :145-147; a NaN projection makes none)."""
    take = (S["eligible"] != 0) & ((tr["in_view"] != 0) | (tr["in_view_r"] != 0))
    if bFar:
        with np.errstate(invalid="ignore"):
            take &= ~(tr["depth"] > f32(thFar))                                  # mTrackDepth as it stands: in/out
    L = take & (tr["in_view"] != 0) & ~np.isnan(tr["proj_x"]) & ~np.isnan(tr["proj_y"])
    R = take & (tr["in_view_r"] != 0) & (tr["level_r"] != -1) & ~np.isnan(tr["proj_xr"]) & ~np.isnan(tr["proj_yr"])
    return L.astype(np.uint8), R.astype(np.uint8)


def oracle_frame(oracle, S):
    kl, kr = S["kl"], S["kr"]
    OFl = oracle.OracleFrame(kl["x"], kl["y"], kl["octave"], kl["angle"], S["dl"], S["bounds"], S["sf"])
    OFr = oracle.OracleFrame(kr["x"], kr["y"], kr["octave"], kr["angle"], S["dr"], S["bounds"], S["sf"])
    return oracle.OracleFisheyeFrame(OFl, OFr)


def expected(oracle, S, th, bFar=False, thFar=0.0, obs="scene", partners=True, track0=None, limit=0.5, slots=None, upto=None, maskL=None, tr=None):
    """Model + oracle -> dict(track, n, slot, slot_obs, mop[2 nmp], mL, mR).  obs: "scene" / None (all 1) / an array.  upto: only the
    first `upto` local map points search; maskL: a left mask ANDed in (both for the scene conditions of the CPU tests)."""
    tr = is_in_frustum_rig(S, track0, limit) if tr is None else tr               # tr: the model's result of an earlier call
    L, R = search_masks(S, tr, bFar, thFar)
    if upto is not None:
        L[upto:] = 0; R[upto:] = 0
    if maskL is not None:
        L &= maskL
    nl, nr = len(S["kl"]), len(S["kr"])
    l2r = S["l2r"] if partners else np.full(nl, -1, np.int32)
    r2l = S["r2l"] if partners else np.full(nr, -1, np.int32)
    qobs = S["obs"] if isinstance(obs, str) else (np.ones(len(L), np.uint8) if obs is None else obs)
    OF = oracle_frame(oracle, S)
    s0 = S["slot0"], S["sobs0"]
    OF.slot[:], OF.slot_obs[:] = s0 if slots is None else slots
    lv = lambda a, m: np.where(m != 0, a, 0).astype(np.int32)
    n, mL, mR = OF.search_by_projection_mp(l2r, r2l, L, R, S["desc"], tr["proj_x"], tr["proj_y"], tr["view_cos"], lv(tr["level"], L), tr["proj_xr"],
                                           tr["proj_yr"], tr["view_cos_r"], lv(tr["level_r"], R), th, NNRATIO, qobs=qobs)
    mop = np.full(2 * len(L), -1, np.int32)
    mop[0::2] = mL
    mop[1::2] = np.where(mR >= 0, mR + nl, -1)
    return dict(track=tr, n=n, slot=OF.slot.copy(), slot_obs=OF.slot_obs.copy(), mop=mop, mL=mL, mR=mR, L=L, R=R)


def dropped_by_continue(oracle, S, E, th, **kw):
    """Local map points whose right half the `continue` of ORBmatcher.cc:127 dropped: both halves make a query, neither matched, and
    with the left half taken out - the slots before the point are the same, and a failed left half writes nothing - the right half
    matches."""
    out = []
    for i in np.nonzero((E["L"] != 0) & (E["R"] != 0) & (E["mL"] < 0) & (E["mR"] < 0))[0]:
        m = np.ones(len(E["L"]), np.uint8)
        m[i] = 0
        if expected(oracle, S, th, upto=i + 1, maskL=m, tr=E["track"], **kw)["mR"][i] >= 0:
            out.append(int(i))
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    R = np.eye(3)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def rig(cam, offs, angle=0.002, scale2=1.002):
    """(Trl, tlr, cam_params2): RM.rig_pose's baseline with a small relative rotation about the optical axis; Tlr = Trl^-1; the right
    camera's own parameters (focal lengths off by 0.2 %)."""
    Trl = RM.rig_pose(cam, offs).astype(np.float64)
    Trl[:3, :3] = rot(2, angle)
    tlr = -(Trl[:3, :3].T @ Trl[:3, 3])
    p2 = RM.CAMS[cam].copy()
    p2[:2] = (p2[:2].astype(np.float64) * scale2).astype(f32)
    return Trl.astype(f32), tlr.astype(f32), p2


def scene(oracle, synth, cam, p=0, seed=RM.SEED, nextra=300, nedge=300, ndup=60, ext=None):
    """Problem p of a camera model: random subsets of the left / right keypoints and of the map points of frame 0 (so N, Nleft and the
    map count differ between problems), a pose with a small rotation, `nextra` random points in and around both views at depths
    0.8 .. 12 and `nedge` near ones around the vertical image borders (random descriptors), distances / normals / eligibility / observations drawn as synth.make_local_map_scene draws them,
    45 % of the keypoints with a stereo partner, 8 % of the slots occupied (half of them with observations), `ndup` left keypoints
    doubled (same place, level and descriptor: the ratio test of a point that lands there fails, ORBmatcher.cc:126)."""
    frames, offs, ext0, sf = RM.stream(oracle, synth, seed)
    (k0, d0), (kl, dl), (kr, dr) = ext if ext is not None else ext0
    rng = np.random.default_rng(seed + 1000 * cam + 31 * p)
    W, H = RM.BOUNDS[1], RM.BOUNDS[3]
    keepL = np.sort(rng.permutation(len(kl))[: len(kl) - rng.integers(20, 120)])
    keepR = np.sort(rng.permutation(len(kr))[: len(kr) - rng.integers(20, 120)])
    keep0 = np.sort(rng.permutation(len(k0))[: len(k0) - rng.integers(300, 500)])
    kl, dl, kr, dr, k0, d0 = kl[keepL], dl[keepL], kr[keepR], dr[keepR], k0[keep0], d0[keep0]
    dup = rng.permutation(len(kl))[:ndup]
    kl, dl = np.concatenate([kl, kl[dup]]), np.concatenate([dl, dl[dup]])
    Rcw = rot(1, 0.01 * (p + 1)) @ rot(0, -0.004 * p)
    tcw = np.array([0.05 * p, -0.02, RM.TZ[p % len(RM.TZ)]])
    Tcw = np.eye(4)
    Tcw[:3, :3], Tcw[:3, 3] = Rcw, tcw
    u = k0["x"].astype(np.float64) + float(offs[0][0] - offs[1][0])
    v = k0["y"].astype(np.float64) + float(offs[0][1] - offs[1][1])
    unproject = synth.kb8_unproject if cam == 1 else synth.pinhole_unproject
    rays = unproject(RM.CAMS[cam], u, v)
    Xc0 = rays * (RM.Z / rays[:, 2:3])
    ue, ve = rng.uniform(-150, W + 150, nextra), rng.uniform(-60, H + 60, nextra)
    Xce = unproject(RM.CAMS[cam], ue, ve) * rng.uniform(0.8, 12.0, nextra)[:, None]
    Xce[rng.random(nextra) < 0.08, 2] *= -1
    # near points around the left and right image borders: the disparity of the rig grows with 1 / depth, so one camera sees them
    ub = np.where(rng.random(nedge) < 0.5, rng.uniform(-80, 80, nedge), rng.uniform(W - 80, W + 80, nedge))
    Xcb = unproject(RM.CAMS[cam], ub, rng.uniform(20, H - 20, nedge)) * rng.uniform(0.5, 1.0, nedge)[:, None]
    Xce, nextra = np.concatenate([Xce, Xcb]), nextra + nedge
    Xc = np.concatenate([Xc0, Xce])
    nmap = len(Xc)
    Xw = ((Xc - tcw[None, :]) @ Rcw).astype(f32)
    desc = np.concatenate([d0, rng.integers(0, 256, (nextra, 32), dtype=np.uint8)])
    octv = np.concatenate([k0["octave"], rng.integers(0, 8, nextra)]).astype(np.int64)
    Tcw = Tcw.astype(f32)
    PO = Xw.astype(np.float64) - M.camera_centre(Tcw).astype(np.float64)[None, :]
    dist = np.linalg.norm(PO, axis=1)
    maxd = dist * sf[octv] * rng.uniform(0.93, 1.02, nmap)
    gate = rng.random(nmap)
    maxd[gate < 0.03] *= 0.6
    near = (gate >= 0.03) & (gate < 0.06)
    mind = maxd / sf[len(sf) - 1]
    mind[near] = dist[near] * 1.5
    dirn = PO / dist[:, None]
    tilt = np.where(rng.random(nmap) < 0.25, rng.uniform(0, 1.4, nmap), rng.uniform(0, 0.08, nmap))
    perp = np.cross(dirn, rng.normal(size=(nmap, 3)))
    perp /= np.linalg.norm(perp, axis=1)[:, None]
    normal = (dirn * np.cos(tilt)[:, None] + perp * np.sin(tilt)[:, None]).astype(f32)
    perm = rng.permutation(nmap)
    c = lambda a: np.ascontiguousarray(a[perm])
    nl, nr = len(kl), len(kr)
    l2r, r2l = np.full(nl, -1, np.int32), np.full(nr, -1, np.int32)
    picks_l = rng.permutation(nl)[: int(0.45 * min(nl, nr))]
    picks_r = rng.permutation(nr)[: len(picks_l)]
    l2r[picks_l], r2l[picks_r] = picks_r, picks_l
    N = nl + nr
    slot0 = np.full(N, -1, np.int32)
    pre = rng.random(N) < 0.08
    slot0[pre] = PRE_VALUE
    sobs0 = (pre & (rng.random(N) < 0.5)).astype(np.uint8)
    Trl, tlr, p2 = rig(cam, offs)
    return dict(kl=kl, dl=dl, kr=kr, dr=dr, sf=sf, log_sf=float(M.glibc_logf(f32(1.2))), bounds=RM.BOUNDS, cam=cam, cam_params=RM.CAMS[cam], cam2=cam,
                cam_params2=p2, Trl=Trl, tlr=tlr, Tcw=Tcw, Xw=c(Xw), desc=c(desc), normal=c(normal), max_dist=c(maxd.astype(f32)),
                min_dist=c(mind.astype(f32)), eligible=c((rng.random(nmap) < 0.9).astype(np.uint8)), obs=c((rng.random(nmap) < 0.9).astype(np.uint8)),
                l2r=l2r, r2l=r2l, slot0=slot0, sobs0=sobs0)


_scenes = {}


def cached_scene(oracle, synth, cam, p=0):
    if (cam, p) not in _scenes:
        _scenes[(cam, p)] = scene(oracle, synth, cam, p)
    return _scenes[(cam, p)]


def classes(tr, eligible):
    """Counts of the eligible points seen by the left camera only, the right only, both, neither."""
    e, l, r = eligible != 0, tr["in_view"] != 0, tr["in_view_r"] != 0
    return int((e & l & ~r).sum()), int((e & ~l & r).sum()), int((e & l & r).sum()), int((e & ~l & ~r).sum())


def constructed(sf):
    """Hand-placed points, one or more per branch of the frustum test and the search (Pinhole, Tcw = I so that world = left camera;
    the right camera 0.3 to the left of the left one, turned by 0.05 rad about y, with its own focal lengths).  Returns the scene, the
    track the MapPoints hold before the call and a dict of the indices the tests name."""
    cam = RM.CAMS[0]
    fx, fy, cx, cy = (float(x) for x in cam)
    p2 = cam.copy()
    p2[:2] = (p2[:2].astype(np.float64) * 1.01).astype(f32)
    Trl = np.eye(4)
    Trl[:3, :3] = rot(1, 0.05)
    Trl[:3, 3] = [0.3, 0.0, 0.05]
    tlr = -(Trl[:3, :3].T @ Trl[:3, 3])
    Trl, tlr = Trl.astype(f32), tlr.astype(f32)
    z = 5.0
    at = lambda u, v, d=z: [(u - cx) / fx * d, (v - cy) / fy * d, d]
    pts, idx = [], {}

    def add(name, P, mx=None, mn=None, nrm=None, obs=1, did=0, depth0=POISON):
        d = float(np.linalg.norm(P))
        idx[name] = len(pts)
        pts.append(dict(P=P, mx=d * 0.97 if mx is None else mx, mn=d / 4 if mn is None else mn, nrm=list(np.array(P) / max(d, 1e-9)) if nrm is None else nrm,
                        obs=obs, did=did, depth0=depth0))

    add("behind", [0.1, 0.1, -1.0])                                  # reason 1 on both sides
    add("behind_r", [3.0, 0.0, 0.05])                                # PcZ >= 0 left (far outside in x), < 0 right
    add("out_x", at(-300, 200))                                      # reason 2 on both sides
    add("out_y", at(300, -200))                                      # reason 3 on both sides
    add("far_scale", at(300, 200), mx=1.0)                           # reason 4: beyond 1.2 mfMaxDistance
    add("near_scale", at(320, 220), mn=20.0, mx=40.0)                # reason 4: below 0.8 mfMinDistance
    add("oblique", at(340, 240), nrm=[1.0, 0.0, 0.0])                # reason 5
    add("centre", [0.0, 0.0, 0.0], mx=1.0, mn=0.0, nrm=[0, 0, 1])    # left: NaN projection, dist 0, ratio inf: raw level INT_MIN -> 0
    add("top_level", at(200, 300), mx=float(np.linalg.norm(at(200, 300))) * float(sf[-1]) * 3.0, mn=0.1)   # raw level >= nlevels
    # seen by one camera only (the right image is 27 px to the right at z = 5): left u = 745 -> right outside; left u = -12 -> right inside
    add("left_only", at(745, 100), did=1)
    add("right_only", at(-12, 120), did=2, depth0=f32(1.0))          # incoming depth below thFarPoints: searched
    add("right_only_stale", at(-12, 300), did=3, depth0=f32(50.0))   # incoming depth above thFarPoints: skipped, with the left check failing
    add("both", at(400, 240), did=4)
    # a partner write releases a claim held with observations: A (obs, right only) takes right keypoint b; B (no obs, left only) takes
    # left keypoint a whose partner is b: slot[b] = B without observations; C (obs, right only, A's place and descriptor) takes b again
    add("A", at(-14, 200), did=5)
    add("B", at(735, 420), did=6, obs=0)
    add("C", at(-14, 200), did=5)
    n = len(pts)
    S = dict(sf=sf, log_sf=float(M.glibc_logf(f32(1.2))), bounds=RM.BOUNDS, cam=0, cam_params=cam, cam2=0, cam_params2=p2, Trl=Trl, tlr=tlr,
             Tcw=np.eye(4, dtype=f32), Xw=np.array([q["P"] for q in pts], f32), normal=np.array([q["nrm"] for q in pts], f32),
             max_dist=np.array([q["mx"] for q in pts], f32), min_dist=np.array([q["mn"] for q in pts], f32), eligible=np.ones(n, np.uint8),
             obs=np.array([q["obs"] for q in pts], np.uint8))
    bank = np.random.default_rng(99).integers(0, 256, (16, 32), dtype=np.uint8)
    S["desc"] = bank[[q["did"] for q in pts]]
    track0 = {k: np.full(n, -777 if t == np.int32 else (9 if t == np.uint8 else POISON), t) for k, t in FIELDS}
    track0["depth"] = np.array([q["depth0"] for q in pts], f32)
    # keypoints on the model's own projections
    S.update(kl=np.zeros(0, RM_KP()), dl=np.zeros((0, 32), np.uint8), kr=np.zeros(0, RM_KP()), dr=np.zeros((0, 32), np.uint8))
    tr = is_in_frustum_rig(S, track0)
    left = [("left_only", 1), ("both", 4), ("B", 6), ("top_level", 0)]
    right = [("right_only", 2), ("right_only_stale", 3), ("both", 4), ("A", 5)]
    oct_of = lambda name, side: int(tr["level" if side == 0 else "level_r"][idx[name]])

    def keys(rows, side):
        k = np.zeros(len(rows) + 1, RM_KP())
        for i, (name, _) in enumerate(rows):
            j = idx[name]
            k[i]["x"], k[i]["y"] = (tr["proj_x"][j], tr["proj_y"][j]) if side == 0 else (tr["proj_xr"][j], tr["proj_yr"][j])
            k[i]["octave"], k[i]["size"] = oct_of(name, side), 31.0
        k[-1]["x"], k[-1]["y"], k[-1]["size"] = 600.0, 40.0, 31.0   # a keypoint no window reaches
        return k, np.concatenate([bank[[d for _, d in rows]], bank[15:16]])

    S["kl"], S["dl"] = keys(left, 0)
    S["kr"], S["dr"] = keys(right, 1)
    nl, nr = len(S["kl"]), len(S["kr"])
    S["l2r"], S["r2l"] = np.full(nl, -1, np.int32), np.full(nr, -1, np.int32)
    S["l2r"][2] = 3                                                  # keypoint of B -> keypoint of A (one direction only)
    S["r2l"][2] = 1                                                  # right keypoint of `both` -> its left keypoint
    S["slot0"], S["sobs0"] = np.full(nl + nr, -1, np.int32), np.zeros(nl + nr, np.uint8)
    idx.update(kp_a=2, kp_b=nl + 3)
    return S, track0, idx


def RM_KP():
    return np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
