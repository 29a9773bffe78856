"""Scenes for the last-frame search of a two-camera fisheye rig (ORBmatcher.cc:2027-2289, CurrentFrame.Nleft != -1), shared by
tests/test_rig_abi.py (CPU: what the scenes must contain, judged by the oracle alone) and tests/test_gpu_rig_batch.py.

As tests/test_gpu_match.py::_fisheye_scene: one shifted synthetic stream of three 752 x 480 frames; the map points are the
keypoints of frame 0, frame 1 is the left image and frame 2 the right image of the current frame.  Unlike there, a map point lies
on the ray that the camera model UNDER TEST un-projects from the pixel where its keypoint appears in the left image (Pinhole in
closed form, KannalaBrandt8 by inverting r(theta) numerically), at z = 5 in the left camera, so that its projection lands on the
keypoint for both models.  The right camera is a translation of the left one (Trl = [I | b]) chosen for the shift between the
two images at that depth: exact under Pinhole, within the search radius under KannalaBrandt8."""
import numpy as np

from conftest import EUROC

SEED = 3600
BOUNDS = (0.0, 752.0, 0.0, 480.0)
Z = 5.0
MB = 0.11
CAMS = {0: np.array([458.654, 457.296, 367.215, 248.375], np.float32),
        1: np.array([190.978477 * 2, 190.973307 * 2, 376.0, 240.0, 0.003482389402, 0.000715034845, -0.002053236141, 0.000202936736], np.float32)}
TZ = (0.3, -0.3, 0.0, 0.3)          # forward, backward, neutral level windows with mb = 0.11; problem 3 repeats the first pose
THS = (7.0, 14.0)
NPRE = 60
PRE_VALUE = 100000                  # a caller's last-frame index no search of these scenes can write

_stream = {}


def stream(oracle, synth, seed=SEED):
    """(frames, offsets, [(keys, desc)] of the three frames by the oracle's extractor, scale factors); extracted once per process."""
    if seed not in _stream:
        frames, offs = synth.make_stream(seed, 3)
        o = oracle.OracleExtractor(**EUROC)
        ext = []
        for f in frames:
            _, k, d = o.extract(f)
            ext.append((k, d))
        _stream[seed] = (frames, offs, ext, np.asarray(o.scale_factors, np.float32))
    return _stream[seed]


def place_points(synth, cam, u, v, tcw):
    """World points (Tlw = I, Rcw = I, tcw given) whose camera coordinates lie on the model's ray through (u, v) at z = Z."""
    rays = synth.kb8_unproject(CAMS[cam], u, v) if cam == 1 else synth.pinhole_unproject(CAMS[cam], u, v)
    Xc = rays * (Z / rays[:, 2:3])
    return np.ascontiguousarray((Xc - np.asarray(tcw, np.float64)[None, :]).astype(np.float32))


def rig_pose(cam, offs):
    """Trl = [I | b]: the translation that moves a point at depth Z by the pixel shift between the left and the right image."""
    p = CAMS[cam]
    Trl = np.eye(4, dtype=np.float32)
    Trl[:3, 3] = [(offs[1][0] - offs[2][0]) * Z / p[0], (offs[1][1] - offs[2][1]) * Z / p[1], 0.0]
    return Trl


def problems(oracle, synth, cam, seed=SEED, ext=None):
    """The four problems of one batch call: per problem its own random subset of the left and right keypoints and of the last
    frame's points (so N, Nleft and nLast differ), 20 % of the points without a map point, 10 % without observations, 3 % behind
    the camera, 60 occupied slots with mixed slot_obs.  ext = ((k0, d0), (kl, dl), (kr, dr)) replaces the oracle's extraction."""
    frames, offs, ext0, sf = stream(oracle, synth, seed)
    (k0, d0), (kl, dl), (kr, dr) = ext if ext is not None else ext0
    rng = np.random.default_rng(seed + 17 * cam)
    out = []
    for p, tz in enumerate(TZ):
        keepL = np.sort(rng.permutation(len(kl))[: len(kl) - rng.integers(20, 120)])
        keepR = np.sort(rng.permutation(len(kr))[: len(kr) - rng.integers(20, 120)])
        keep0 = np.sort(rng.permutation(len(k0))[: len(k0) - rng.integers(5, 60)])
        q = dict(kl=kl[keepL], dl=dl[keepL], kr=kr[keepR], dr=dr[keepR], k0=k0[keep0], d0=d0[keep0], tz=tz, cam=cam, sf=sf)
        n0 = len(keep0)
        Tcw = np.eye(4, dtype=np.float32)
        Tcw[2, 3] = tz
        u = q["k0"]["x"].astype(np.float64) + float(offs[0][0] - offs[1][0])
        v = q["k0"]["y"].astype(np.float64) + float(offs[0][1] - offs[1][1])
        Xw = place_points(synth, cam, u, v, Tcw[:3, 3])
        behind = rng.random(n0) < 0.03
        Xw[behind, 2] = np.float32(-1.0) - np.float32(tz)
        q.update(Xw=Xw, Tcw=Tcw, Tlw=np.eye(4, dtype=np.float32), Trl=rig_pose(cam, offs), u=u, v=v, behind=behind,
                 has_mp=(rng.random(n0) < 0.8).astype(np.uint8), obs=(rng.random(n0) < 0.9).astype(np.uint8))
        N = len(keepL) + len(keepR)
        q["pre"] = rng.permutation(N)[:NPRE]
        q["pre_obs"] = (rng.random(NPRE) < 0.5).astype(np.uint8)
        out.append(q)
    return out


def initial_slots(q):
    N = len(q["kl"]) + len(q["kr"])
    slot, sobs = np.full(N, -1, np.int32), np.zeros(N, np.uint8)
    slot[q["pre"]] = PRE_VALUE
    sobs[q["pre"]] = q["pre_obs"]
    return slot, sobs


def oracle_search(oracle, q, th, mono=False, check_ori=True, slots=None):
    """The oracle's SearchByProjection for one problem -> (nmatches, slot, slot_obs)."""
    kl, kr, sf = q["kl"], q["kr"], q["sf"]
    OFl = oracle.OracleFrame(kl["x"], kl["y"], kl["octave"], kl["angle"], q["dl"], BOUNDS, sf)
    OFr = oracle.OracleFrame(kr["x"], kr["y"], kr["octave"], kr["angle"], q["dr"], BOUNDS, sf)
    OF = oracle.OracleFisheyeFrame(OFl, OFr)
    slot, sobs = initial_slots(q) if slots is None else slots
    OF.slot[:] = slot
    OF.slot_obs[:] = sobs
    n = OF.search_by_projection_ff(q["has_mp"], q["Xw"], q["d0"], q["k0"]["octave"], q["k0"]["angle"], q["Tcw"], q["Tlw"], q["Trl"], q["cam"],
                                   CAMS[q["cam"]], th, mono=mono, check_ori=check_ori, mb=MB, qobs=q["obs"])
    return n, OF.slot.copy(), OF.slot_obs.copy()


CHAIN_TH = 7.0
CHAIN_LAP = ((0, 400), (352, 752))      # lapping areas of the left and the right extraction
CHAIN_FRAMES = ((1, 2, 0.3), (2, 1, -0.3))   # (left image, right image, tz) of the two rig frames of the chain test


def chain_problems(oracle, synth, cam, ext=None, seed=SEED):
    """The two rig frames of tests/test_gpu_rig_batch.py::test_chain_from_extraction as problems: every keypoint of frame 0 is a
    map point with observations, no slot is occupied.  ext[f] = (kl, dl, kr, dr) replaces the oracle's own extraction of the
    images with the lapping areas CHAIN_LAP (the GPU test passes what it downloaded)."""
    frames, offs, ext0, sf = stream(oracle, synth, seed)
    k0, d0 = ext0[0]
    n0 = len(k0)
    out = []
    for f, (li, ri, tz) in enumerate(CHAIN_FRAMES):
        if ext is None:
            o = oracle.OracleExtractor(**EUROC)
            (_, kl, dl), (_, kr, dr) = o.extract(frames[li], CHAIN_LAP[0]), o.extract(frames[ri], CHAIN_LAP[1])
        else:
            kl, dl, kr, dr = ext[f]
        Tcw = np.eye(4, dtype=np.float32)
        Tcw[2, 3] = tz
        u = k0["x"].astype(np.float64) + float(offs[0][0] - offs[li][0])
        v = k0["y"].astype(np.float64) + float(offs[0][1] - offs[li][1])
        out.append(dict(kl=kl, dl=dl, kr=kr, dr=dr, k0=k0, d0=d0, Xw=place_points(synth, cam, u, v, Tcw[:3, 3]), Tcw=Tcw,
                        Tlw=np.eye(4, dtype=np.float32), Trl=rig_pose(cam, offs), has_mp=np.ones(n0, np.uint8), obs=np.ones(n0, np.uint8), cam=cam, sf=sf,
                        tz=tz, u=u, v=v, behind=np.zeros(n0, bool), pre=np.zeros(0, np.int64), pre_obs=np.zeros(0, np.uint8)))
    return out


def scene_counts(oracle, q, th, mono=False):
    """(matches, new matches in the left image, in the right image, matches undone by the rotation histogram) of the oracle's result."""
    s0, _ = initial_slots(q)
    n, slot, _ = oracle_search(oracle, q, th, mono=mono)
    n_unpruned, _, _ = oracle_search(oracle, q, th, mono=mono, check_ori=False)
    new = (slot != s0) & (slot >= 0)
    nl = len(q["kl"])
    return n, int(new[:nl].sum()), int(new[nl:].sum()), n_unpruned - n
