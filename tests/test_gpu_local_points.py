"""GPU: Tracking::SearchLocalPoints on the device (orbm_search_local_points, orbm_search_local_points_batch_device): Frame::isInFrustum
with PredictScale through the logf replica (k_local_map_project), then SearchByProjection(Frame&, const vector<MapPoint*>&, th,
bFarPoints, thFarPoints).  Expected values: tests/local_map_model.py followed by the oracle's M2 search.  The track fields are compared
bit for bit (in_view, proj_x, proj_y of every eligible point, the rest where in_view is set; NaN equals NaN whatever its payload),
the search by slot, slot_obs, match_of_point and nmatches."""
import ctypes as C

import numpy as np
import pytest

import local_map_model as M
from conftest import EUROC, TUMVI
from oracle import oracle_py

pytestmark = pytest.mark.gpu

f32 = np.float32
PIN = np.array([458.654, 457.296, 367.215, 248.375], f32)      # Examples/Monocular/EuRoC.yaml:9-12
FIELDS = ("in_view", "proj_x", "proj_y", "proj_xr", "depth", "view_cos", "level")


class Scene:
    pass


def make_scene(pkg, oracle, synth, seed, kind, nmap=3000):
    """A current frame extracted from a shifted synthetic stream and its local map (synth.make_local_map_scene)."""
    S = Scene()
    if kind == "tumvi":
        H, W, cfg, S.cam_type, S.cam = 512, 512, TUMVI, 1, synth.TUMVI_KB8
    else:
        H, W, cfg, S.cam_type, S.cam = 480, 752, EUROC, 0, PIN
    S.bounds = (0.0, float(W), 0.0, float(H))
    frames, offs = synth.make_stream(seed, 2, H=H, W=W)
    o = oracle.OracleExtractor(**cfg)
    _, k0, d0 = o.extract(frames[0])
    _, S.k1, S.d1 = o.extract(frames[1])
    S.sf = np.asarray(o.scale_factors, f32)
    S.log_sf = float(M.glibc_logf(f32(1.2)))
    S.mbf = 47.9 if kind == "stereo" else 0.0
    shift = (offs[0][0] - offs[1][0], offs[0][1] - offs[1][1])
    L = synth.make_local_map_scene(S.cam_type, S.cam, k0, d0, S.k1, shift, seed, S.sf, W, H, nmap=nmap, mbf=S.mbf)
    S.Xw, S.desc, S.normal, S.maxd, S.mind = L["Xw"], L["desc"], L["normal"], L["max_dist"], L["min_dist"]
    S.elig, S.obs, S.Tcw, S.slot0, S.sobs0, S.u_right = L["eligible"], L["obs"], L["Tcw"], L["slot"], L["slot_obs"], L["u_right"]
    return S


def fequal(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def check_track(tr, ref, elig):
    e = np.asarray(elig) != 0
    assert np.array_equal(tr["in_view"], ref["in_view"])
    for k in ("proj_x", "proj_y"):
        assert fequal(tr[k], ref[k])[e].all(), k
    iv = ref["in_view"] != 0
    for k in ("proj_xr", "depth", "view_cos"):
        assert fequal(tr[k], ref[k])[iv].all(), k
    assert np.array_equal(tr["level"][iv], ref["level"][iv])


def model(S, viewing_cos_limit=0.5, Tcw=None):
    return M.is_in_frustum(S.Xw, S.normal, S.maxd, S.mind, S.elig, S.Tcw if Tcw is None else Tcw, S.cam_type, S.cam, S.bounds, len(S.sf),
                           S.log_sf, S.mbf, viewing_cos_limit, oracle_py.project)


def expected(oracle, S, ref, th, bFar, thFar, elig=None):
    elig = S.elig if elig is None else elig
    OF = oracle.OracleFrame(S.k1["x"], S.k1["y"], S.k1["octave"], S.k1["angle"], S.d1, S.bounds, S.sf, u_right=S.u_right)
    OF.slot[:] = S.slot0
    OF.slot_obs[:] = S.sobs0
    n, moq = OF.search_by_projection_mp(M.query_mask(ref, elig, bFar, thFar), S.desc, ref["proj_x"], ref["proj_y"], ref["view_cos"], ref["level"],
                                        th, 0.8, qobs=S.obs, projXR=ref["proj_xr"])
    return n, moq, OF.slot, OF.slot_obs


def run_host(pkg, m, S, th, bFar, thFar, viewing_cos_limit=0.5):
    F = pkg.FrameView(S.k1, S.d1, S.bounds, u_right=S.u_right)
    F.slot[:] = S.slot0
    F.slot_obs[:] = S.sobs0
    n, moq, tr = m.SearchLocalPoints(F, S.sf, S.log_sf, S.elig, S.Xw, S.normal, S.maxd, S.mind, S.desc, S.Tcw, S.cam_type, S.cam, th,
                                     bFarPoints=bFar, thFarPoints=thFar, mbf=S.mbf, viewing_cos_limit=viewing_cos_limit, mp_obs=S.obs)
    return n, moq, tr, F


def check_scene(pkg, oracle, m, S, th, bFar, thFar, ref=None, viewing_cos_limit=0.5):
    ref = model(S, viewing_cos_limit) if ref is None else ref
    n, moq, tr, F = run_host(pkg, m, S, th, bFar, thFar, viewing_cos_limit)
    check_track(tr, ref, S.elig)
    n_ref, moq_ref, slot_ref, sobs_ref = expected(oracle, S, ref, th, bFar, thFar)
    assert n == n_ref
    assert np.array_equal(moq, moq_ref)
    assert np.array_equal(F.slot, slot_ref) and np.array_equal(F.slot_obs, sobs_ref)
    return n_ref, ref


_scenes = {}


def scene(pkg, oracle, synth, kind):
    if kind not in _scenes:
        _scenes[kind] = make_scene(pkg, oracle, synth, {"euroc": 5100, "tumvi": 5200, "stereo": 5300}[kind], kind)
    return _scenes[kind]


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.ORBmatcher(0.8, True)
    yield m
    m.close()


@pytest.mark.parametrize("kind", ["euroc", "tumvi", "stereo"])
def test_scenes(pkg, oracle, synth, matcher, kind):
    S = scene(pkg, oracle, synth, kind)
    ref = model(S)
    iv = ref["in_view"] != 0
    assert 0.3 * len(S.Xw) < iv.sum() < 0.95 * len(S.Xw)
    thFar = float(np.median(ref["depth"][iv]))
    counts = []
    for th in (1.0, 3.0, 5.0, 10.0, 15.0):
        for bFar in (False, True):
            n, _ = check_scene(pkg, oracle, matcher, S, th, bFar, thFar, ref=ref)
            counts.append(n)
    assert min(counts[0::2]) >= 100, counts      # hundreds of matches without the far-point gate


def test_constructed_branches(pkg, oracle, synth, matcher):
    """Every branch of isInFrustum and PredictScale on hand-placed points (Pinhole, pose with a -0 translation)."""
    S = scene(pkg, oracle, synth, "euroc")
    T = np.eye(4, dtype=f32)
    T[2, 3] = -0.0
    rng = np.random.default_rng(7)
    pts, maxd, mind, nrm = [], [], [], []

    def add(P, mx, mn, n=None):
        pts.append(P); maxd.append(mx); mind.append(mn); nrm.append([0, 0, 1] if n is None else n)

    add([0, 0, -5], 10, 1)                        # behind the camera
    add([1, 1, 0.0], 10, 1)                       # PcZ = +0: infinite projection
    add([-1, -1, -0.0], 10, 1)                    # PcZ = -0
    add([0, 0, 0], 1, 0)                          # at the camera centre: NaN projection, dist 0, NaN viewCos, ratio inf
    ua, va = oracle.project(0, PIN, -1.0, -0.5, 5.0)
    ub, vb = oracle.project(0, PIN, 1.0, 0.7, 5.0)
    for P in ([-1.0, -0.5, 5.0], [1.0, 0.7, 5.0], [-1.01, 0, 5.0], [1.01, 0, 5.0], [0, -0.51, 5.0], [0, 0.71, 5.0]):   # on / beyond each bound
        add(P, 10, 1)
    d = f32(4.0)
    for k in range(-3, 4):                        # each distance gate, stepping over it by ulps
        g = np.nextafter(f32(d / f32(0.8)), f32(np.inf) if k > 0 else f32(0))
        for _ in range(abs(k)):
            g = np.nextafter(g, f32(np.inf) if k > 0 else f32(0))
        add([0, 0, d], 10, g)
        g = f32(d / f32(1.2))
        for _ in range(abs(k)):
            g = np.nextafter(g, f32(np.inf) if k > 0 else f32(0))
        add([0, 0, d], g, 1)
    # the level boundaries of PredictScale: points at (0, 0, d) with d a power of two, so that ratio = max_dist / dist is max_dist / 4
    # exactly; max_dist = d * sf[k] and up to 3 ulps either side.  The clamp at nlevels after them.
    bnd = []
    for k in range(8):
        for s in range(-3, 4):
            mx = f32(d * S.sf[k])
            for _ in range(abs(s)):
                mx = np.nextafter(mx, f32(np.inf) if s > 0 else f32(0))
            bnd.append(len(pts))
            add([0, 0, d], mx, 0.5)
    add([0, 0, d], f32(d * S.sf[7] * f32(3.0)), 0.5)
    P = np.array([0.2, -0.1, 3.0])                # viewCos around the limit 0.5 and around 0.998 (PO = P: the camera centre is -0)
    dirn = P / np.linalg.norm(P)
    perp = np.cross(dirn, [0.0, 1.0, 0.0])
    perp /= np.linalg.norm(perp)
    for c, eps in ((0.5, 0.0), (0.5, 1e-7), (0.5, -1e-7), (0.5, 3e-7), (0.998, 0.0), (0.998, 3e-6), (0.998, -3e-6), (0.998, 1e-5),
                   (0.998, -1e-5), (1.0, 0.0), (0.3, 0.0)):
        ang = np.arccos(c) + eps
        add(list(P), 10, 1, list(dirn * np.cos(ang) + perp * np.sin(ang)))
    for _ in range(40):
        add(list(rng.uniform([-2, -1.5, 1], [2, 1.5, 8])), 12, 0.5, list(rng.normal(size=3)))
    n = len(pts)
    C2 = Scene()
    C2.__dict__.update(S.__dict__)
    C2.Xw, C2.maxd, C2.mind = np.array(pts, f32), np.array(maxd, f32), np.array(mind, f32)
    nn = np.array(nrm, np.float64)
    C2.normal = (nn / np.maximum(np.linalg.norm(nn, axis=1), 1e-12)[:, None]).astype(f32)
    C2.Tcw, C2.cam_type, C2.cam = T, 0, PIN
    C2.bounds = (ua, ub, va, vb)
    C2.desc = S.desc[:n].copy()
    C2.elig = np.ones(n, np.uint8)
    C2.elig[rng.random(n) < 0.1] = 0
    C2.obs = (rng.random(n) < 0.7).astype(np.uint8)
    ref = model(C2)
    assert ref["in_view"][3] == 1 and np.isnan(ref["proj_x"][3]) and ref["level"][3] == 0
    assert len(set(ref["level"][ref["in_view"] != 0].tolist())) == 8
    # boundary-sensitive points: a logf one ulp off would move their level
    lg = lambda x: M.cvtt_f32_i32(np.ceil(x / f32(S.log_sf)))
    sens = 0
    for j in bnd:
        if not C2.elig[j]:
            continue
        v = M.glibc_logf(C2.maxd[j] / f32(4.0))
        sens += lg(v) != lg(np.nextafter(v, f32(np.inf))) or lg(v) != lg(np.nextafter(v, f32(-np.inf)))
    assert sens >= 4, sens
    vc = ref["view_cos"][ref["in_view"] != 0]
    assert ((vc > 0.4999) & (vc < 0.5001)).sum() >= 2 and ((vc > 0.9979) & (vc < 0.9981)).sum() >= 3
    # the search runs on the scene's keypoints (bounds of the constructed frame)
    check_scene(pkg, oracle, matcher, C2, 3.0, False, 0.0, ref=ref)
    limit = float(ref["view_cos"][ref["in_view"] != 0][-1])      # a viewCos exactly at the limit
    check_scene(pkg, oracle, matcher, C2, 1.0, True, float(ref["depth"][ref["in_view"] != 0][0]), viewing_cos_limit=limit)
    # KannalaBrandt8 projects a point at PcZ = -0 inside the image: only PcZ < 0 is rejected (Frame.cc:592)
    K = scene(pkg, oracle, synth, "tumvi")
    K2 = Scene()
    K2.__dict__.update(K.__dict__)
    K2.Xw = np.array([[-1, -1, -0.0], [-1, -1, -1e-3], [1, 1, 0.0], [0.3, -0.2, -0.0], [0.5, 0.5, 2.0]], f32)
    n = len(K2.Xw)
    K2.maxd, K2.mind = np.full(n, 10, f32), np.full(n, 0.1, f32)
    K2.normal = np.tile(f32([0, 0, 1]), (n, 1))
    K2.Tcw = T
    K2.desc, K2.elig, K2.obs = K.desc[:n].copy(), np.ones(n, np.uint8), np.ones(n, np.uint8)
    ref = model(K2, viewing_cos_limit=-2.0)
    assert ref["proj_x"][0] != -1 and ref["in_view"][0] == 1 and ref["proj_x"][1] == -1 and ref["in_view"][1] == 0
    check_scene(pkg, oracle, matcher, K2, 3.0, False, 0.0, ref=ref, viewing_cos_limit=-2.0)


def test_scan_modes_and_engines(pkg, oracle, synth):
    S = scene(pkg, oracle, synth, "euroc")
    ref = model(S)
    for mode in (0, 1, 2):
        for eng in (0, 1, 2):
            m = pkg.ORBmatcher(0.8, True)
            try:
                m.set_scan_mode(mode)
                m.set_hamming_engine(eng)
                n, _ = check_scene(pkg, oracle, m, S, 5.0, False, 0.0, ref=ref)
                assert n > 100
            finally:
                m.close()


def _batch(pkg, m, S, P, fcnt, mcnt, Tcws, th, bFar, thFar, fstride, mstride):
    """Problem p = S's frame truncated to fcnt[p] keypoints and S's map truncated to mcnt[p] points with pose Tcws[p]; returns the
    per-problem (nmatches, match_of_point, slot, slot_obs, track) of one batched launch."""
    import torch
    dev = "cuda"
    kp = np.zeros((P, fstride, 7), f32)
    de = np.zeros((P, fstride, 32), np.uint8)
    ur = np.full((P, fstride), -1, f32)
    cnt = np.zeros((P, 2), np.int32)
    mc = np.zeros((P, 2), np.int32)
    slot = np.full((P, fstride), -1, np.int32)
    sobs = np.zeros((P, fstride), np.uint8)
    kview = np.ascontiguousarray(S.k1).view(f32).reshape(len(S.k1), 7)
    mp = {k: np.zeros((P, mstride) + sh, dt) for k, sh, dt in (("elig", (), np.uint8), ("Xw", (3,), f32), ("normal", (3,), f32), ("maxd", (), f32),
                                                                 ("mind", (), f32), ("desc", (32,), np.uint8), ("obs", (), np.uint8))}
    for p in range(P):
        n, q = fcnt[p], mcnt[p]
        kp[p, :n], de[p, :n], cnt[p, 0], mc[p, 0] = kview[:n], S.d1[:n], n, q
        slot[p, :n], sobs[p, :n] = S.slot0[:n], S.sobs0[:n]
        if S.u_right is not None:
            ur[p, :n] = S.u_right[:n]
        for k, src in (("elig", S.elig), ("Xw", S.Xw), ("normal", S.normal), ("maxd", S.maxd), ("mind", S.mind), ("desc", S.desc), ("obs", S.obs)):
            mp[k][p, :q] = src[:q]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = {k: t(v) for k, v in mp.items()}
    d_kp, d_de, d_ur, d_cnt, d_mc, d_slot, d_sobs = t(kp), t(de), t(ur), t(cnt), t(mc), t(slot), t(sobs)
    d_T = t(np.stack(Tcws).astype(f32))
    d_moq = torch.full((P, mstride), -7, dtype=torch.int32, device=dev)
    tr = {k: torch.zeros((P, mstride), dtype=torch.uint8 if k == "in_view" else torch.int32 if k == "level" else torch.float32, device=dev)
          for k in FIELDS}
    d_nm = torch.zeros(P, dtype=torch.int32, device=dev)
    fs = pkg.FrameStruct(fstride, d_kp.data_ptr(), d_de.data_ptr(), d_ur.data_ptr() if S.u_right is not None else None, *S.bounds)
    ms = pkg.LocalMapStruct(mstride, d["elig"].data_ptr(), d["Xw"].data_ptr(), d["normal"].data_ptr(), d["maxd"].data_ptr(), d["mind"].data_ptr(),
                            d["desc"].data_ptr(), d["obs"].data_ptr(), d_T.data_ptr())
    ts = pkg.TrackStruct(*[tr[k].data_ptr() for k in FIELDS])
    m.search_local_points_batch_device(fs, fstride, d_cnt.data_ptr(), 2, ms, mstride, d_mc.data_ptr(), 2, P, S.sf, S.log_sf, S.cam_type, S.cam, th,
                                       d_slot.data_ptr(), d_sobs.data_ptr(), d_moq.data_ptr(), ts, d_nm.data_ptr(), bFarPoints=bFar,
                                       thFarPoints=thFar, mbf=S.mbf)
    torch.cuda.synchronize()
    trh = {k: v.cpu().numpy() for k, v in tr.items()}
    return d_nm.cpu().numpy(), d_moq.cpu().numpy(), d_slot.cpu().numpy(), d_sobs.cpu().numpy(), trh


@pytest.mark.parametrize("kind", ["euroc", "stereo"])
def test_batch_equals_host_form(pkg, oracle, synth, matcher, kind):
    S = scene(pkg, oracle, synth, kind)
    P = 16
    n1, nmp = len(S.k1), len(S.Xw)
    fcnt = [max(0, n1 - 37 * p) for p in range(P)]
    mcnt = [nmp - 50 * p for p in range(P)]
    mcnt[3] = 0                                   # a problem with no map points
    fcnt[5] = 0                                   # a problem with no keypoints
    Tcws = []
    for p in range(P):
        T = S.Tcw.copy()
        T[:3, 3] += f32(0.0015) * np.array([p % 4 - 1.5, p // 4 - 1.5, 0.5 * (p % 3)], f32)
        Tcws.append(T)
    nm, moq, slot, sobs, tr = _batch(pkg, matcher, S, P, fcnt, mcnt, Tcws, 3.0, True, 6.0, n1 + 3, nmp + 5)
    total = 0
    for p in range(P):
        n, q = fcnt[p], mcnt[p]
        Sp = Scene()
        Sp.__dict__.update(S.__dict__)
        Sp.k1, Sp.d1, Sp.slot0, Sp.sobs0 = S.k1[:n], S.d1[:n], S.slot0[:n], S.sobs0[:n]
        Sp.u_right = None if S.u_right is None else S.u_right[:n]
        for k in ("Xw", "normal", "maxd", "mind", "desc", "elig", "obs"):
            setattr(Sp, k, getattr(S, k)[:q])
        Sp.Tcw = Tcws[p]
        hn, hmoq, htr, F = run_host(pkg, matcher, Sp, 3.0, True, 6.0)
        assert nm[p] == hn, p
        assert np.array_equal(moq[p, :q], hmoq), p
        assert np.array_equal(slot[p, :n], F.slot) and np.array_equal(sobs[p, :n], F.slot_obs), p
        check_track({k: v[p, :q] for k, v in tr.items()}, htr, Sp.elig)
        if q and n:
            ref = model(Sp)
            check_track(htr, ref, Sp.elig)
        total += hn
    assert total > 1000


def test_random_sweep(pkg, oracle, synth, matcher):
    rng = np.random.default_rng(2024)
    total = 0
    for i in range(40):
        kind = ("euroc", "tumvi", "stereo")[i % 3]
        S = Scene()
        S.__dict__.update(scene(pkg, oracle, synth, kind).__dict__)
        T = S.Tcw.copy()
        T[:3, 3] += rng.normal(scale=0.01, size=3).astype(f32)
        a = rng.normal(scale=0.004)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float64)
        T[:3, :3] = (Rz @ T[:3, :3].astype(np.float64)).astype(f32)
        S.Tcw = T
        sel = rng.random(len(S.Xw)) < rng.uniform(0.3, 1.0)
        for k in ("Xw", "normal", "maxd", "mind", "desc", "elig", "obs"):
            setattr(S, k, np.ascontiguousarray(getattr(S, k)[sel]))
        th = float(rng.choice([1.0, 2.0, 3.0, 5.0, 10.0, 15.0]))
        bFar = bool(rng.random() < 0.5)
        n, _ = check_scene(pkg, oracle, matcher, S, th, bFar, float(rng.uniform(3.0, 9.0)), viewing_cos_limit=float(rng.choice([0.5, 0.3, 0.8])))
        total += n
    assert total > 40 * 50


def test_refusals(pkg, oracle, synth, matcher):
    S = scene(pkg, oracle, synth, "euroc")
    F = pkg.FrameView(S.k1, S.d1, S.bounds)
    args = (S.sf, S.log_sf, S.elig, S.Xw, S.normal, S.maxd, S.mind, S.desc, S.Tcw)
    with pytest.raises(ValueError):
        matcher.SearchLocalPoints(F, *args, 2, S.cam, 1.0)                    # cam_type
    with pytest.raises(ValueError):
        matcher.SearchLocalPoints(F, np.ones(17, f32), *args[1:], 0, S.cam, 1.0)   # nlevels
    big = pkg.FrameView(np.zeros(15361, pkg.KP_DTYPE), np.zeros((15361, 32), np.uint8), S.bounds)
    with pytest.raises(ValueError):
        matcher.SearchLocalPoints(big, *args, 0, S.cam, 1.0)
    # the refusals leave the handle usable
    n, _ = check_scene(pkg, oracle, matcher, S, 1.0, False, 0.0)
    assert n > 100


def test_refusals_with_a_handle(pkg):
    """ORBX_E_ARG from a live handle: nlevels 0 / 17, cam_type 2, each NULL required pointer or struct field, a frame above
    ORBM_MAX_KEYPOINTS, map_stride below the live count - for both entry points, before anything is staged or launched (the arrays
    are host arrays: every call below must be refused)."""
    from test_local_points_abi import _args
    L = pkg.load()
    A, keys, desc, fs, ms, ts = _args(pkg)
    p = lambda a: a.ctypes.data
    host = lambda m, fs_, sf, ms_, cam, slot, sobs, ts_, nlevels=8, cam_type=0: L.orbm_search_local_points(
        m, fs_, sf, nlevels, C.c_float(0.18), ms_, cam_type, cam, C.c_float(0.0), C.c_float(0.5), C.c_float(1.0), 0, C.c_float(0.0),
        C.c_float(0.8), slot, sobs, p(A["moq"]), ts_)
    good = (C.byref(fs), p(A["sf"]), C.byref(ms), p(A["cam"]), p(A["slot"]), p(A["sobs"]), C.byref(ts))
    dev = lambda m, fs_, ms_, ts_, sf, cam, slot, sobs, nm: L.orbm_search_local_points_batch_device(
        m, fs_, 4, None, 0, ms_, 3, None, 0, 1, sf, 8, C.c_float(0.18), 0, cam, C.c_float(0.0), C.c_float(0.5), C.c_float(1.0), 0,
        C.c_float(0.0), C.c_float(0.8), slot, sobs, None, ts_, nm, None)
    m = L.orbm_create(0)
    assert m
    try:
        assert host(m, *good, nlevels=0) == pkg.E_ARG and host(m, *good, nlevels=17) == pkg.E_ARG and host(m, *good, cam_type=2) == pkg.E_ARG
        for i in range(len(good)):
            bad = list(good)
            bad[i] = None
            assert host(m, *bad) == pkg.E_ARG, i
        for field in ("eligible", "Xw", "normal", "max_dist", "min_dist", "mpdesc", "Tcw"):
            ms2 = pkg.LocalMapStruct.from_buffer_copy(ms)
            setattr(ms2, field, None)
            assert host(m, C.byref(fs), p(A["sf"]), C.byref(ms2), p(A["cam"]), p(A["slot"]), p(A["sobs"]), C.byref(ts)) == pkg.E_ARG, field
        for field in ("in_view", "proj_x", "proj_y", "proj_xr", "depth", "view_cos", "level"):
            ts2 = pkg.TrackStruct.from_buffer_copy(ts)
            setattr(ts2, field, None)
            assert host(m, C.byref(fs), p(A["sf"]), C.byref(ms), p(A["cam"]), p(A["slot"]), p(A["sobs"]), C.byref(ts2)) == pkg.E_ARG, field
        fbig = pkg.FrameStruct.from_buffer_copy(fs)
        fbig.n = 15361
        assert host(m, C.byref(fbig), *good[1:]) == pkg.E_ARG
        gd = (C.byref(fs), C.byref(ms), C.byref(ts), p(A["sf"]), p(A["cam"]), p(A["slot"]), p(A["sobs"]), p(A["nm"]))
        for i in range(len(gd)):
            bad = list(gd)
            bad[i] = None
            assert dev(m, *bad) == pkg.E_ARG, i
        short = pkg.LocalMapStruct.from_buffer_copy(ms)
        short.n = 4      # map_stride 3 < live count 4
        assert dev(m, C.byref(fs), C.byref(short), *gd[2:]) == pkg.E_ARG
        for field in ("eligible", "Xw", "normal", "max_dist", "min_dist", "mpdesc", "Tcw"):
            ms2 = pkg.LocalMapStruct.from_buffer_copy(ms)
            setattr(ms2, field, None)
            assert dev(m, C.byref(fs), C.byref(ms2), *gd[2:]) == pkg.E_ARG, field
    finally:
        L.orbm_destroy(m)


_LOGF_HELPER = r"""
#include <math.h>
void logf_array(const float *x, float *y, long n) { for (long i = 0; i < n; i++) y[i] = logf(x[i]); }
"""


def test_device_logf_equals_glibc(pkg, tmp_path):
    """The DEVICE build of csrc/orb_logf.h (orbx_logf_device) against this host's glibc logf: +-4096 ulps around sf^k and 1/sf^k
    (sf in {1.2, 1.5, 2}, k <= 15: the level boundaries of PredictScale), a strided sample of every positive float, the special
    values.  Bit for bit; a NaN result only has to be a NaN (the device's and x86's default NaNs differ in sign)."""
    import shutil
    import subprocess
    import torch
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    (tmp_path / "h.c").write_text(_LOGF_HELPER)
    subprocess.check_call([cc, "-O2", "-shared", "-fPIC", "-o", str(tmp_path / "h.so"), str(tmp_path / "h.c"), "-lm"])
    H = C.CDLL(str(tmp_path / "h.so"))
    H.logf_array.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    bits = lambda x: int(np.array([x], f32).view(np.uint32)[0])
    win = []
    for sf in (1.2, 1.5, 2.0):
        for k in range(16):
            for b in (bits(f32(sf ** k)), bits(f32(sf) ** f32(k)), bits(f32(1.0 / sf ** k))):
                win.append(np.arange(b - 4096, b + 4097, dtype=np.uint64))
    win.append(np.arange(0, 0x80000000, 997, dtype=np.uint64))
    win.append(np.array([0, 0x80000000, 0x3f800000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 1, 0x807fffff, 0xbf800000],
                        np.uint64))
    x = np.concatenate(win).astype(np.uint32).view(f32)
    want = np.empty_like(x)
    H.logf_array(x.ctypes.data, want.ctypes.data, len(x))
    d_x = torch.from_numpy(x).cuda()
    d_y = torch.zeros_like(d_x)
    assert pkg.load().orbx_logf_device(C.c_void_p(d_x.data_ptr()), len(x), C.c_void_p(d_y.data_ptr()), None) == 0
    torch.cuda.synchronize()
    got = d_y.cpu().numpy()
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, "%d mismatches, first x=%r got %r want %r" % (len(bad), x[bad[0]], got[bad[0]], want[bad[0]])


def test_chained_extract_undistort_local_points(pkg, oracle, synth):
    """orbx_extract_batch_device -> orbm_undistort_keypoints_batch_device -> orbm_search_local_points_batch_device on one stream with
    no host synchronisation in between, on the distorted EuRoC geometry, starting from the slots a host-form last-frame search filled
    (as Track() does before TrackLocalMap).  Each frame equals the host form run on the host's extraction and undistortion."""
    import torch
    from test_undistort import D as EUROC_D, K as EUROC_K
    P, H, W = 6, 480, 752
    frames, offs = synth.make_stream(5600, P + 1)
    o = oracle.OracleExtractor(**EUROC)
    ext = [o.extract(f)[1:] for f in frames]
    sf = np.asarray(o.scale_factors, f32)
    log_sf = float(M.glibc_logf(f32(1.2)))
    bounds = pkg.image_bounds(W, H, EUROC_K, EUROC_D)
    m = pkg.ORBmatcher(0.8, True)
    ex = pkg.ORBextractor(device=0, **EUROC)
    try:
        cap = ex.configure(H, W, P)
        nmap = 2500
        mstride = nmap + 3
        host, maps = [], []
        for p in range(P):                       # problem p: the current frame p + 1, its previous frame p
            (k0, d0), (k1, d1) = ext[p], ext[p + 1]
            k0u, k1u = pkg.undistort_keypoints(k0, EUROC_K, EUROC_D), pkg.undistort_keypoints(k1, EUROC_K, EUROC_D)
            shift = (offs[p][0] - offs[p + 1][0], offs[p][1] - offs[p + 1][1])
            L = synth.make_local_map_scene(0, PIN, k0u, d0, k1u, shift, 5600 + p, sf, W, H, nmap=nmap)
            # the last-frame search of Track(): map points on the previous frame's keypoints, pose Tcw, Tlw = I
            Xw0, Tcw, Tlw = synth.make_last_frame_scene(0, PIN, k0u["x"], k0u["y"], shift, 5600 + p)
            has_mp = (np.arange(len(k0u)) % 3 != 0).astype(np.uint8)
            F = pkg.FrameView(k1u, d1, bounds)
            n_lf = m.SearchByProjectionLastFrame(F, sf, has_mp, Xw0, d0, k0u, Tcw, Tlw, 0, PIN, 15.0)
            assert n_lf > 100
            slot0, sobs0 = F.slot.copy(), F.slot_obs.copy()
            n_h, moq_h, tr_h = m.SearchLocalPoints(F, sf, log_sf, L["eligible"], L["Xw"], L["normal"], L["max_dist"], L["min_dist"], L["desc"],
                                                   L["Tcw"], 0, PIN, 5.0, mp_obs=L["obs"])
            host.append((k1, n_h, moq_h, tr_h, F.slot.copy(), F.slot_obs.copy(), slot0, sobs0))
            maps.append(L)
        assert sum(h[1] for h in host) > 300
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        img = t(np.stack(frames[1:]))
        slot = np.full((P, cap), -1, np.int32)
        sobs = np.zeros((P, cap), np.uint8)
        arrs = {k: np.zeros((P, mstride) + sh, dt) for k, sh, dt in (("eligible", (), np.uint8), ("Xw", (3,), f32), ("normal", (3,), f32),
                                                                      ("max_dist", (), f32), ("min_dist", (), f32), ("desc", (32,), np.uint8),
                                                                      ("obs", (), np.uint8))}
        mc = np.zeros((P, 2), np.int32)
        for p in range(P):
            n1 = len(host[p][0])
            slot[p, :n1], sobs[p, :n1] = host[p][6], host[p][7]
            for k in arrs:
                arrs[k][p, :nmap] = maps[p][k]
            mc[p, 0] = nmap
        d = {k: t(v) for k, v in arrs.items()}
        d_T = t(np.stack([mp["Tcw"] for mp in maps]))
        d_slot, d_sobs, d_mc = t(slot), t(sobs), t(mc)
        d_kps = torch.zeros((P, cap, 7), dtype=torch.int32, device="cuda")
        d_kpu = torch.zeros_like(d_kps)
        d_desc = torch.zeros((P, cap, 32), dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros((P, 2), dtype=torch.int32, device="cuda")
        d_moq = torch.full((P, mstride), -7, dtype=torch.int32, device="cuda")
        tr = {k: torch.zeros((P, mstride), dtype=torch.uint8 if k == "in_view" else torch.int32 if k == "level" else torch.float32, device="cuda")
              for k in FIELDS}
        d_nm = torch.zeros(P, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                 # the uploads above are done; from here on one stream, no host synchronisation
        s = torch.cuda.current_stream().cuda_stream
        ex.extract_batch_device(img.data_ptr(), H, W, W, H * W, P, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), cap, stream=s)
        m.undistort_batch_device(d_kps.data_ptr(), cap, d_cnt.data_ptr(), 2, P, EUROC_K, EUROC_D, d_kpu.data_ptr(), stream=s)
        fs = pkg.FrameStruct(cap, d_kpu.data_ptr(), d_desc.data_ptr(), None, *bounds)
        ms = pkg.LocalMapStruct(mstride, d["eligible"].data_ptr(), d["Xw"].data_ptr(), d["normal"].data_ptr(), d["max_dist"].data_ptr(),
                                d["min_dist"].data_ptr(), d["desc"].data_ptr(), d["obs"].data_ptr(), d_T.data_ptr())
        ts = pkg.TrackStruct(*[tr[k].data_ptr() for k in FIELDS])
        m.search_local_points_batch_device(fs, cap, d_cnt.data_ptr(), 2, ms, mstride, d_mc.data_ptr(), 2, P, sf, log_sf, 0, PIN, 5.0,
                                           d_slot.data_ptr(), d_sobs.data_ptr(), d_moq.data_ptr(), ts, d_nm.data_ptr(), stream=s)
        torch.cuda.synchronize()
        cnt, nm, moq = d_cnt.cpu().numpy(), d_nm.cpu().numpy(), d_moq.cpu().numpy()
        slot_d, sobs_d = d_slot.cpu().numpy(), d_sobs.cpu().numpy()
        trd = {k: v.cpu().numpy() for k, v in tr.items()}
        for p in range(P):
            k1, n_h, moq_h, tr_h, slot_h, sobs_h = host[p][:6]
            n1 = len(k1)
            assert cnt[p, 0] == n1, p
            assert nm[p] == n_h, p
            assert np.array_equal(moq[p, :nmap], moq_h), p
            assert np.array_equal(slot_d[p, :n1], slot_h) and np.array_equal(sobs_d[p, :n1], sobs_h), p
            check_track({k: v[p, :nmap] for k, v in trd.items()}, tr_h, maps[p]["eligible"])
    finally:
        m.close()
        ex.close()
