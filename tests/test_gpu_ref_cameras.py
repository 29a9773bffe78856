"""GPU: the device evaluations of the camera models against the reference's own src/CameraModels/Pinhole.cpp and KannalaBrandt8.cpp,
compiled (oracle/_ref/libref_cameras.so: the two files' unmodified text against the stand-in headers of oracle/ref_cam_shim).

The other GPU tests of these paths compare with tests/rig_stereo_model.py and the oracle's orc_project / orc_pinhole_*, restatements by
the same hands as the kernels; a misreading of the two files' own text that all of them share shows here.  Compared, bit for bit:
KannalaBrandt8::TriangulateMatches in orbm_fisheye_triangulate_device and in the rig stereo kernel, Pinhole::project and
KannalaBrandt8::project in the projection kernel of SearchLocalPoints (per call and batched), and both epipolarConstrain members inside
SearchForTriangulation.  Inputs: tests/ref_camera_cases.py.

The library is built by __graft_entry__.build() where the reference tree exists and travels with the tree; these tests only load it
and never look for the reference.  Without it they FAIL: a skip would hide the whole file."""
import numpy as np
import pytest

import ref_camera_cases as RC
import rig_stereo_model as M
import triangulation_kb8_scene as SC

pytestmark = pytest.mark.gpu
f32 = np.float32
FSENT = -777.25
FIELDS = ("in_view", "proj_x", "proj_y", "proj_xr", "depth", "view_cos", "level")


@pytest.fixture(scope="module")
def ref(oracle):
    try:
        oracle.ref_cam_lib(build_if_possible=False)
    except (RuntimeError, OSError) as e:
        pytest.fail("oracle/_ref/libref_cameras.so cannot be loaded (%s): run __graft_entry__.build() where the reference tree exists" % e)
    return oracle


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.ORBmatcher(0.8, True)
    yield m
    m.close()


def bits(a):
    a = np.ascontiguousarray(a, dtype=f32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


# ---- KannalaBrandt8::TriangulateMatches on the device ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def triangulated(ref):
    """The 4096 pairs through the compiled member: computed once, shared, never modified."""
    P = RC.triangulation_pairs()
    depth, p3d, code = ref.ref_triangulate_matches(M.CAM1, M.CAM2, M.TLR, P["kp1"], P["kp2"], P["s1"], P["s2"], p3d_fill=FSENT)
    return dict(P, depth=depth, p3d=p3d, code=code)


@pytest.mark.parametrize("n", [4096, 1, 1000], ids=["all", "one", "not-a-multiple-of-64"])
def test_triangulate_device(pkg, triangulated, n):
    import torch
    T = triangulated
    first = 0 if n != 1 else int(np.flatnonzero(T["code"] == 5)[0])          # the single pair is an accepted one
    sl = slice(first, first + n)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = [t(T[k][sl]) for k in ("kp1", "kp2", "s1", "s2")]
    d_depth, d_p3d = t(np.full(n + 3, FSENT, f32)), t(np.full((n + 3, 3), FSENT, f32))
    assert pkg.fisheye_triangulate_device(n, *[a.data_ptr() for a in d], M.TLR, M.CAM1, M.CAM2, d_depth.data_ptr(), d_p3d.data_ptr()) == 0
    torch.cuda.synchronize()
    depth, p3d = d_depth.cpu().numpy(), d_p3d.cpu().numpy()
    assert np.array_equal(bits(depth[:n]), bits(T["depth"][sl])) and (depth[n:] == f32(FSENT)).all()
    assert np.array_equal(bits(p3d[:n]), bits(T["p3d"][sl])) and (p3d[n:] == f32(FSENT)).all()      # p3D only where the member reaches its end
    if n == 4096:
        assert (np.bincount(T["code"], minlength=6) >= 20).all()


# ---- project in the projection kernel of SearchLocalPoints -----------------------------------------------------------------------------
def projection_problem(pkg, ref, name):
    """The z >= 0 projection points as a local map seen with Tcw = identity (Pc = 1*x + 0*y + 0*z + 0: Xw itself, a -0 becoming +0), every
    point eligible, in a frame whose bounds are the compiled projections of the two corner points; a handful of keypoints, since only
    the projection kernel's outputs are read.  want_x / want_y: the compiled project where it lies inside the bounds, -1 elsewhere."""
    cam_type, cam = RC.CAMERAS[name]
    C = RC.projection_points(name)
    Xw = np.ascontiguousarray(C["X"][:C["nfront"]])
    uv = ref.ref_project(cam_type, cam, Xw + f32(0.0))
    bounds = (float(uv[C["lo"], 0]), float(uv[C["hi"], 0]), float(uv[C["lo"], 1]), float(uv[C["hi"], 1]))
    with np.errstate(invalid="ignore"):
        inside = ~((uv[:, 0] < bounds[0]) | (uv[:, 0] > bounds[1])) & ~((uv[:, 1] < bounds[2]) | (uv[:, 1] > bounds[3]))
    assert inside[C["lo"]] and inside[C["hi"]] and inside.sum() >= 200 and (~inside).sum() >= 200
    n = len(Xw)
    rng = np.random.default_rng(8)
    keys = np.zeros(8, pkg.KP_DTYPE)
    keys["x"], keys["y"] = rng.uniform(bounds[0], bounds[1], 8).astype(f32), rng.uniform(bounds[2], bounds[3], 8).astype(f32)
    nrm = np.zeros((n, 3), f32)
    nrm[:, 2] = 1.0
    return dict(cam_type=cam_type, cam=cam, Xw=Xw, bounds=bounds, keys=keys, desc=rng.integers(0, 256, (8, 32), dtype=np.uint8),
                mpdesc=rng.integers(0, 256, (n, 32), dtype=np.uint8), normal=nrm, maxd=np.full(n, 1e9, f32), mind=np.zeros(n, f32),
                elig=np.ones(n, np.uint8), Tcw=np.eye(4, dtype=f32), sf=SC.scale_factors(), log_sf=float(np.log(f32(1.2))),
                want_x=np.where(inside, uv[:, 0], f32(-1)).astype(f32), want_y=np.where(inside, uv[:, 1], f32(-1)).astype(f32), inside=inside)


@pytest.mark.parametrize("name", list(RC.CAMERAS))
def test_projection_kernel(pkg, ref, matcher, name):
    Q = projection_problem(pkg, ref, name)
    F = pkg.FrameView(Q["keys"], Q["desc"], Q["bounds"])
    _, _, tr = matcher.SearchLocalPoints(F, Q["sf"], Q["log_sf"], Q["elig"], Q["Xw"], Q["normal"], Q["maxd"], Q["mind"], Q["mpdesc"], Q["Tcw"],
                                         Q["cam_type"], Q["cam"], 1.0, viewing_cos_limit=-2.0)
    for k, want in (("proj_x", Q["want_x"]), ("proj_y", Q["want_y"])):
        bad = np.flatnonzero(bits(tr[k]) != bits(want))
        assert len(bad) == 0, (k, len(bad), bad[:5], tr[k][bad[:5]], want[bad[:5]], Q["Xw"][bad[:5]])
    assert not tr["in_view"][~Q["inside"]].any()


@pytest.mark.parametrize("name", ["pinhole", "tumvi-left"])
def test_projection_kernel_batched(pkg, ref, matcher, name):
    """Two problems in one orbm_search_local_points_batch_device launch: all the points, and the first 517 of them."""
    import torch
    Q = projection_problem(pkg, ref, name)
    n, counts, P = len(Q["Xw"]), (len(Q["Xw"]), 517), 2
    fstride, mstride = 8, n + 5
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rep = lambda a, width: np.stack([np.concatenate([a[:c], np.zeros((width - c,) + a.shape[1:], a.dtype)]) for c in counts])
    kp = t(np.stack([np.ascontiguousarray(Q["keys"]).view(f32).reshape(8, 7)] * P))
    de, ur = t(np.stack([Q["desc"]] * P)), t(np.full((P, fstride), -1, f32))
    cnt, mc = t(np.array([[8, 0]] * P, np.int32)), t(np.array([[c, 0] for c in counts], np.int32))
    d = {k: t(rep(Q[k], mstride)) for k in ("elig", "Xw", "normal", "maxd", "mind", "mpdesc")}
    d_obs, d_T = t(np.ones((P, mstride), np.uint8)), t(np.stack([Q["Tcw"]] * P))
    d_slot, d_sobs = t(np.full((P, fstride), -1, np.int32)), t(np.zeros((P, fstride), np.uint8))
    d_moq = torch.full((P, mstride), -7, dtype=torch.int32, device="cuda")
    tr = {k: torch.zeros((P, mstride), dtype=torch.uint8 if k == "in_view" else torch.int32 if k == "level" else torch.float32, device="cuda")
          for k in FIELDS}
    d_nm = torch.zeros(P, dtype=torch.int32, device="cuda")
    fs = pkg.FrameStruct(fstride, kp.data_ptr(), de.data_ptr(), None, *Q["bounds"])
    ms = pkg.LocalMapStruct(mstride, d["elig"].data_ptr(), d["Xw"].data_ptr(), d["normal"].data_ptr(), d["maxd"].data_ptr(), d["mind"].data_ptr(),
                            d["mpdesc"].data_ptr(), d_obs.data_ptr(), d_T.data_ptr())
    ts = pkg.TrackStruct(*[tr[k].data_ptr() for k in FIELDS])
    matcher.search_local_points_batch_device(fs, fstride, cnt.data_ptr(), 2, ms, mstride, mc.data_ptr(), 2, P, Q["sf"], Q["log_sf"], Q["cam_type"], Q["cam"],
                                             1.0, d_slot.data_ptr(), d_sobs.data_ptr(), d_moq.data_ptr(), ts, d_nm.data_ptr(), viewing_cos_limit=-2.0)
    torch.cuda.synchronize()
    for p, c in enumerate(counts):
        for k, want in (("proj_x", Q["want_x"]), ("proj_y", Q["want_y"])):
            got = tr[k][p, :c].cpu().numpy()
            assert np.array_equal(bits(got), bits(want[:c])), (p, k)


# ---- the rig stereo kernel -------------------------------------------------------------------------------------------------------------
def test_rig_stereo_kernel(pkg, ref, matcher):
    """One synthetic rig frame, 300 lapping keypoints per image behind 3 / 5 monocular ones: a left lapping row's partner carries its
    descriptor with 0-10 bits flipped and the right keypoint of a synthetic rig pair.  For every left keypoint the kernel matched,
    depth and p3D equal the compiled TriangulateMatches of that keypoint pair."""
    rng = np.random.default_rng(41)
    mono, lap = (3, 5), 300
    kp1, kp2, _, _ = M.synthetic_pairs(lap, seed=9)
    nL, nR = mono[0] + lap, mono[1] + lap
    kL, kR = np.zeros(nL, pkg.KP_DTYPE), np.zeros(nR, pkg.KP_DTYPE)
    dL, dR = rng.integers(0, 256, (nL, 32), dtype=np.uint8), rng.integers(0, 256, (nR, 32), dtype=np.uint8)
    for k, n in ((kL, nL), (kR, nR)):
        k["x"], k["y"] = rng.uniform(0, 512, n).astype(f32), rng.uniform(0, 512, n).astype(f32)
        k["octave"] = rng.integers(0, 8, n)
    rows = rng.permutation(lap)
    for q in range(lap):
        li, rj = mono[0] + q, mono[1] + int(rows[q])
        kL["x"][li], kL["y"][li] = kp1[q]
        kR["x"][rj], kR["y"][rj] = kp2[q]
        d = dL[li].copy()
        flip = rng.permutation(256)[: int(rng.integers(0, 11))]
        np.bitwise_xor.at(d, flip >> 3, (1 << (flip & 7)).astype(np.uint8))
        dR[rj] = d
    l2r, r2l, depth, p3d, nm = matcher.ComputeStereoFishEyeMatches(kL, dL, mono[0], kR, dR, mono[1], M.LEVEL_SIGMA2, M.TLR, M.CAM1, M.CAM2,
                                                                    p3d=np.full((nL, 3), FSENT, f32))
    hit = np.flatnonzero(l2r >= 0)
    assert len(hit) >= 60 and nm[0] == len(hit) < nm[1]           # matches, and pairs the triangulation rejected
    j = l2r[hit]
    at = lambda k, i: np.stack([k["x"][i], k["y"][i]], axis=1)
    want_d, want_p, code = ref.ref_triangulate_matches(M.CAM1, M.CAM2, M.TLR, at(kL, hit), at(kR, j), M.LEVEL_SIGMA2[kL["octave"][hit]],
                                                       M.LEVEL_SIGMA2[kR["octave"][j]], p3d_fill=FSENT)
    assert (code == 5).all()
    assert np.array_equal(bits(depth[hit]), bits(want_d)) and np.array_equal(bits(p3d[hit]), bits(want_p))


# ---- KannalaBrandt8::epipolarConstrain inside SearchForTriangulation -------------------------------------------------------------------
@pytest.mark.parametrize("rig", [False, True], ids=["mono", "rig"])
def test_kb8_epipolar_constrain_in_the_search(pkg, ref, rig):
    """The smallest scene of tests/triangulation_kb8_scene.py: orbm_search_for_triangulation_kb8 == the oracle's member around a predicate
    that calls the compiled KannalaBrandt8::epipolarConstrain (the route of tests/test_gpu_triangulation_kb8.py with the numpy one)."""
    S = SC.scene(96, rig)
    k1, k2, memo = S["k1"], S["k2"], {}

    def pred(i1, i2):
        if (i1, i2) not in memo:
            a, b = int(rig and i1 >= S["n_left1"]), int(rig and i2 >= S["n_left2"])
            T12 = S["T12"][2 * a + b].reshape(3, 4)
            memo[(i1, i2)] = bool(ref.ref_epipolar_constrain(1, S["cams1"][a], S["cams2"][b], T12[:, :3], T12[:, 3], [k1["x"][i1], k1["y"][i1]],
                                                             [k2["x"][i2], k2["y"][i2]], S["sigma2"][k1["octave"][i1]], S["sigma2"][k2["octave"][i2]])[0])
        return memo[(i1, i2)]

    K1, K2 = SC.product_views(pkg, S, 4)
    O1, O2 = SC.oracle_views(ref, S, 4)
    n_ref, pairs_ref = ref.search_for_triangulation_pred(O1, O2, S["ep"], not rig, pred)
    m = pkg.ORBmatcher(0.6, False)
    try:
        n, pairs = m.SearchForTriangulationKB8(K1, K2, S["ep"], S["cams1"], S["cams2"], S["T12"], S["n_left1"], S["n_left2"])
    finally:
        m.close()
    assert n == n_ref >= 40 and np.array_equal(pairs, pairs_ref)
    verdicts = list(memo.values())
    assert sum(verdicts) >= 40 and len(verdicts) - sum(verdicts) >= 20       # the geometry accepted and rejected


# ---- Pinhole::epipolarConstrain inside SearchForTriangulation --------------------------------------------------------------------------
def test_pinhole_epipolar_constrain_in_the_search(pkg, ref, synth):
    """The scene of tests/test_gpu_match.py::test_search_for_triangulation_m6 (no coarse mode, all keypoints, no orientation check):
    orbm_search_for_triangulation == the oracle's member around the compiled Pinhole::epipolarConstrain, with R12 = R1w*R2w.t() and
    t12 = -R1w*R2w.t()*t2w + t1w formed as ORBmatcher.cc:1007-1008 forms them (a product with a transposed operand accumulates in
    double; the second product is the small-matrix one) and the epipole through the compiled Pinhole::project."""
    from test_gpu_match import _bow, make_frame_pair
    (k0, d0), (k1, d1), offs, sf = make_frame_pair(pkg, ref, synth, 3300)
    rng = np.random.default_rng(5)
    sf = np.asarray(sf, f32)
    sigma2 = (sf * sf).astype(f32)
    cam = RC.PINHOLE
    z = f32(5.0)
    dx, dy = offs[0][0] - offs[1][0], offs[0][1] - offs[1][1]
    R1w, t1w = np.eye(3, dtype=f32), np.zeros(3, f32)
    ang = 0.001
    R2w = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], f32)
    t2w = np.array([dx * z / cam[0], dy * z / cam[1], 0.02], f32)
    Cw1 = np.zeros(3, f32)
    ur0 = np.where(rng.random(len(k0)) < 0.5, k0["x"] - f32(9.0), f32(-1)).astype(f32)
    ur1 = np.where(rng.random(len(k1)) < 0.5, k1["x"] - f32(9.0), f32(-1)).astype(f32)
    mp0, mp1 = (rng.random(len(k0)) < 0.2).astype(np.uint8), (rng.random(len(k1)) < 0.2).astype(np.uint8)
    fv0, fv1 = _bow(d0), _bow(d1)
    KF1 = pkg.KeyFrameView(k0, d0, fv0, sf, sigma2, u_right=ur0, has_mappoint=mp0)
    KF2 = pkg.KeyFrameView(k1, d1, fv1, sf, sigma2, u_right=ur1, has_mappoint=mp1)
    O1 = ref.OracleKeyFrame(k0, d0, fv0, sf, sigma2, u_right=ur0, has_mp=mp0)
    O2 = ref.OracleKeyFrame(k1, d1, fv1, sf, sigma2, u_right=ur1, has_mp=mp1)
    acc = R1w.astype(np.float64) @ R2w.astype(np.float64).T                     # R1w * R2w.t(): double accumulation, rounded once
    R12, Rm = acc.astype(f32), (acc * -1.0).astype(f32)
    t12 = np.array([f32(f32(f32(Rm[i, 0] * t2w[0]) + f32(Rm[i, 1] * t2w[1])) + f32(Rm[i, 2] * t2w[2])).astype(np.float64) + np.float64(t1w[i])
                    for i in range(3)]).astype(f32)
    C2 = (R2w @ Cw1 + t2w).astype(f32)                                          # Cw1 = 0: exactly t2w
    ep = ref.ref_project(0, cam, C2[None])[0]
    ep_o, _ = ref.pinhole_pair_geometry(R1w, t1w, R2w, t2w, Cw1, cam, cam)
    assert ep.tobytes() == ep_o.tobytes()
    memo = {}

    def pred(i1, i2):
        if (i1, i2) not in memo:
            memo[(i1, i2)] = bool(ref.ref_epipolar_constrain(0, cam, cam, R12, t12, [k0["x"][i1], k0["y"][i1]], [k1["x"][i2], k1["y"][i2]],
                                                             sigma2[k0["octave"][i1]], sigma2[k1["octave"][i2]])[0])
        return memo[(i1, i2)]

    n_ref, pairs_ref = ref.search_for_triangulation_pred(O1, O2, ep, True, pred)
    m = pkg.ORBmatcher(0.6, False)
    try:
        n, pairs = m.SearchForTriangulation(KF1, KF2, R1w, t1w, R2w, t2w, Cw1, cam, cam)
    finally:
        m.close()
    assert n == n_ref > 60 and np.array_equal(pairs, pairs_ref)
    verdicts = list(memo.values())
    assert sum(verdicts) > 60 and len(verdicts) - sum(verdicts) >= 5
