"""GPU: the device matcher against the reference's own src/ORBmatcher.cc, compiled (oracle/_ref/libref_matcher.so: the file's unmodified
text against the stand-in headers of oracle/ref_cam_shim, with oracle/ref_match_driver.cc).

The other GPU tests of the matcher compare with oracle/orb_oracle.c and the numpy rule models, restatements by the same hands as the
kernels; a misreading of ORBmatcher.cc's own text that all of them share shows here.  Every pinned member's product entry runs once
through the C ABI on the scenes of tests/ref_matcher_cases.py, and the return value and every output array must equal the compiled
text's: the per-call form, SearchLocalPoints with the projection on the device, the one-call form of SearchByBoW over several candidate
keyframes, and - on the one scene whose shape reaches them (test_search_last_frame_open_windows) - the three match engines.  At the
shapes of the other scenes (windowed queries, more than 128 keypoints in one call) every engine setting runs the vector-ALU walk /
scan, so they are not parametrised over it.

The library is built by __graft_entry__.build() where the reference tree exists and travels with the tree; these tests only load it
and never look for the reference.  They skip where the library is absent.  One process, no subprocesses."""
import re

import numpy as np
import pytest

import ref_matcher_cases as MC

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ref(oracle):
    try:
        oracle.ref_match_lib(build_if_possible=False)
    except (RuntimeError, OSError):
        pytest.skip("no oracle/_ref/libref_matcher.so: __graft_entry__.build() makes it where the reference tree exists")
    return oracle


@pytest.fixture(scope="module")
def matchers(pkg):
    made = {}

    def get(nnratio, check_ori, engine=2):
        key = (float(nnratio), bool(check_ori), int(engine))
        if key not in made:
            made[key] = pkg.ORBmatcher(nnratio, check_ori)
            made[key].set_hamming_engine(engine)
        return made[key]
    yield get
    for m in made.values():
        m.close()


def keys_of(pkg, fr):
    k = np.zeros(len(fr["kx"]), pkg.KP_DTYPE)
    k["x"], k["y"], k["octave"], k["angle"] = fr["kx"], fr["ky"], fr["octave"], fr["angle"]
    return k


def both(pkg, ref, fr, slot=None, slot_obs=None):
    """The product's FrameView and the compiled text's RefFrame over one scene frame, with the scene's occupied slots."""
    V = pkg.FrameView(keys_of(pkg, fr), fr["desc"], fr["bounds"], u_right=fr.get("u_right"))
    O = ref.OracleFrame(fr["kx"], fr["ky"], fr["octave"], fr["angle"], fr["desc"], fr["bounds"], MC.SF, u_right=fr.get("u_right"))
    O.slot[:] = fr["slot"] if slot is None else slot
    O.slot_obs[:] = fr["slot_obs"] if slot_obs is None else slot_obs
    V.slot[:], V.slot_obs[:] = O.slot, O.slot_obs
    return V, ref.RefFrame(O)


def same_slots(V, R, what):
    assert np.array_equal(V.slot, R.slot), "%s: mvpMapPoints differ at %s" % (what, np.flatnonzero(V.slot != R.slot)[:8])
    assert np.array_equal(np.where(V.slot >= 0, V.slot_obs, 0), R.slot_obs), what


# ---- the three small members -------------------------------------------------------------------------------------------------------
def test_small_members(pkg, ref):
    a, b = MC.descriptor_pairs()
    for x, y in zip(a, b):
        assert pkg.ORBmatcher.DescriptorDistance(x, y) == ref.ref_descriptor_distance(x, y)
    for sizes in MC.three_maxima_cases():
        assert tuple(pkg.ORBmatcher.ComputeThreeMaxima(sizes)) == ref.ref_three_maxima(sizes), sizes
    for v in MC.VIEW_COS:
        assert pkg.ORBmatcher.RadiusByViewingCos(v) == ref.ref_radius_by_viewing_cos(v), v


# ---- SearchByProjection(Frame, MapPoints), ORBmatcher.cc:44 -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mono", "stereo", "distorted"])
def test_search_local_points(pkg, ref, matchers, name):
    S = MC.local_points(name)
    fr, q = S["frame"], S["q"]
    V, R = both(pkg, ref, fr)
    xr = q["projXR"] if fr["u_right"] is not None else None
    in_view = q["in_view"] & (1 - q["bad"]) & (q["depth"] <= f32(S["th_far"])).astype(np.uint8)
    n_d, _, _ = matchers(S["nnratio"], True).SearchByProjection(V, in_view, q["desc"], q["projX"], q["projY"], q["viewCos"], q["level"], MC.SF,
                                                                       th=S["th"], mp_obs=q["obs"], mp_projXR=xr)
    n_r = R.search_by_projection_mp(q["in_view"], q["desc"], q["projX"], q["projY"], q["viewCos"], q["level"], S["th"], S["nnratio"], qobs=q["obs"],
                                    projXR=xr, bad=q["bad"], track_depth=q["depth"], far_points=True, th_far=S["th_far"])
    assert n_r > 100 and n_d == n_r
    same_slots(V, R, name)


def test_search_local_points_fisheye(pkg, ref, matchers):
    S = MC.local_points_fisheye()
    q, L, Rt = S["q"], S["left"], S["right"]
    mk = lambda fr: ref.OracleFrame(fr["kx"], fr["ky"], fr["octave"], fr["angle"], fr["desc"], fr["bounds"], MC.SF)
    OF = ref.OracleFisheyeFrame(mk(L), mk(Rt))
    OF.slot[:], OF.slot_obs[:] = S["slot"], S["slot_obs"]
    RF = ref.RefFisheyeFrame(OF)
    V = pkg.FrameView(np.concatenate([keys_of(pkg, L), keys_of(pkg, Rt)]), np.concatenate([L["desc"], Rt["desc"]]), L["bounds"])
    V.slot[:], V.slot_obs[:] = S["slot"], S["slot_obs"]
    n_d, _, _ = matchers(S["nnratio"], True).SearchByProjectionFisheye(V, len(L["kx"]), S["l2r"], S["r2l"], q["desc"], MC.SF, S["th"], q["in_view"],
                                                                       q["projX"], q["projY"], q["viewCos"], q["level"], q["in_view_r"], q["projXR"],
                                                                       q["projYR"], q["viewCosR"], q["levelR"], mp_obs=q["obs"])
    n_r = RF.search_by_projection_mp(S["l2r"], S["r2l"], q["in_view"], q["in_view_r"], q["desc"], q["projX"], q["projY"], q["viewCos"], q["level"],
                                     q["projXR"], q["projYR"], q["viewCosR"], q["levelR"], S["th"], S["nnratio"], qobs=q["obs"])
    assert n_r > 100 and n_d == n_r
    mine = (V.slot >= 0) & (V.slot < 100000)               # orbm_search_by_projection_fisheye numbers its queries 2 * point + camera
    V.slot[mine] //= 2
    same_slots(V, RF, "fisheye")


@pytest.mark.parametrize("name", ["pinhole", "kb8"])
def test_search_local_points_projected_on_device(pkg, ref, matchers, name):
    """Tracking::SearchLocalPoints in one call: the device runs isInFrustum and the search.  The compiled text searches with what the
    device's frustum test wrote into the map points (the test of Frame.cc itself is not pinned) and must fill the same slots."""
    S = MC.reloc_keyframe(name)
    V, R = both(pkg, ref, S["cur"])
    T = S["Tcw"].astype(np.float64)
    Ow = -T[:3, :3].T @ T[:3, 3]
    normal = S["Xw"].astype(np.float64) - Ow               # seen head-on: PO.dot(Pn) == dist
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(f32)
    elig = (S["state"] == 1).astype(np.uint8)
    obs = (np.arange(S["n"]) % 3 != 0).astype(np.uint8)
    n_d, _, track = matchers(0.8, True).SearchLocalPoints(V, MC.SF, MC.LOG_SF, elig, S["Xw"], normal, S["max_dist"], S["min_dist"], S["mpdesc"], S["Tcw"],
                                                           S["cam_type"], S["cam"], 3.0, mp_obs=obs)
    assert int(track["in_view"].sum()) > 60
    n_r = R.search_by_projection_mp(track["in_view"], S["mpdesc"], track["proj_x"], track["proj_y"], track["view_cos"], track["level"], 3.0, 0.8, qobs=obs,
                                    projXR=track["proj_xr"])
    assert n_r > 40 and n_d == n_r
    same_slots(V, R, name)


# ---- SearchByProjection(Frame, Frame), ORBmatcher.cc:2027 ---------------------------------------------------------------------------
def last_keys(pkg, S):
    k = np.zeros(S["n"], pkg.KP_DTYPE)
    k["octave"], k["angle"] = S["last_octave"], S["last_angle"]
    return k


@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("name", ["mono", "stereo-forward", "stereo-backward", "stereo-still", "distorted"])
def test_search_last_frame(pkg, ref, matchers, name, check_ori):
    S = MC.last_frame(name)
    V, R = both(pkg, ref, S["cur"])
    n_d = matchers(0.9, check_ori).SearchByProjectionLastFrame(V, MC.SF, (S["has_mp"] == 1).astype(np.uint8), S["Xw"], S["mpdesc"], last_keys(pkg, S),
                                                                       S["Tcw"], S["Tlw"], S["cam_type"], S["cam"], S["th"], bMono=S["mono"], mb=S["mb"],
                                                                       mbf=S["mbf"], mp_obs=S["obs"])
    n_r = R.search_by_projection_ff(S["has_mp"], S["Xw"], S["mpdesc"], S["last_octave"], S["last_angle"], S["Tcw"], S["Tlw"], S["cam_type"], S["cam"],
                                    S["th"], mono=S["mono"], check_ori=check_ori, mb=S["mb"], mbf=S["mbf"], qobs=S["obs"])
    assert n_r > 60 and n_d == n_r
    same_slots(V, R, name)


FORM = re.compile(r"orbhip: resolve maxn (\d+) fused (\d) dynamic LDS (\d+) bytes")


@pytest.mark.parametrize("engine", [0, 1, 2])
@pytest.mark.parametrize("check_ori", [True, False])
def test_search_last_frame_open_windows(pkg, ref, matchers, capfd, monkeypatch, check_ori, engine):
    """The three match engines against the compiled text.  120 keypoints without right coordinates and only open queries: one
    candidate slice, so engines 1 and 2 take the matrix pipe (orbhip.hip: `mfma` needs nslices == 1 and no u_right, the kernels serve
    pairs whose live queries are all open).  The library's own report of the launch form must say that engine 2 fused this launch;
    engine 1 differs from it by that flag alone."""
    S = MC.last_frame_open()
    V, R = both(pkg, ref, S["cur"])
    assert V.N <= 128 and S["cur"]["u_right"] is None
    monkeypatch.setenv("ORBHIP_PRINT_RESOLVE_LDS", "1")
    capfd.readouterr()
    n_d = matchers(0.9, check_ori, engine).SearchByProjectionLastFrame(V, MC.SF, (S["has_mp"] == 1).astype(np.uint8), S["Xw"], S["mpdesc"], last_keys(pkg, S),
                                                                       S["Tcw"], S["Tlw"], S["cam_type"], S["cam"], S["th"], bMono=False, mb=S["mb"],
                                                                       mbf=S["mbf"], mp_obs=S["obs"])
    forms = FORM.findall(capfd.readouterr().err)
    assert len(forms) == 1 and int(forms[0][0]) == V.N, forms
    assert forms[0][1] == ("1" if engine == 2 else "0"), (engine, forms)
    n_r = R.search_by_projection_ff(S["has_mp"], S["Xw"], S["mpdesc"], S["last_octave"], S["last_angle"], S["Tcw"], S["Tlw"], S["cam_type"], S["cam"],
                                    S["th"], mono=False, check_ori=check_ori, mb=S["mb"], mbf=S["mbf"], qobs=S["obs"])
    assert n_r >= 30 and n_d == n_r
    same_slots(V, R, "open, engine %d" % engine)


@pytest.mark.parametrize("check_ori", [True, False])
def test_search_last_frame_rig(pkg, ref, matchers, check_ori):
    S = MC.last_frame("rig")
    L, Rt = S["cur"], S["right"]
    mk = lambda fr: ref.OracleFrame(fr["kx"], fr["ky"], fr["octave"], fr["angle"], fr["desc"], fr["bounds"], MC.SF)
    OF = ref.OracleFisheyeFrame(mk(L), mk(Rt))
    OF.slot[:], OF.slot_obs[:] = S["slot"], S["slot_obs"]
    RF = ref.RefFisheyeFrame(OF)
    V = pkg.FrameView(np.concatenate([keys_of(pkg, L), keys_of(pkg, Rt)]), np.concatenate([L["desc"], Rt["desc"]]), L["bounds"])
    V.slot[:], V.slot_obs[:] = S["slot"], S["slot_obs"]
    n_d = matchers(0.9, check_ori).SearchByProjectionLastFrameFisheye(V, len(L["kx"]), MC.SF, (S["has_mp"] == 1).astype(np.uint8), S["Xw"], S["mpdesc"],
                                                                      last_keys(pkg, S), S["Tcw"], S["Tlw"], S["Trl"], S["cam_type"], S["cam"], S["th"],
                                                                      bMono=False, mb=S["mb"], mp_obs=S["obs"])
    n_r = RF.search_by_projection_ff(S["has_mp"], S["Xw"], S["mpdesc"], S["last_octave"], S["last_angle"], S["Tcw"], S["Tlw"], S["Trl"], S["cam_type"],
                                     S["cam"], S["th"], mono=False, check_ori=check_ori, mb=S["mb"], qobs=S["obs"])
    assert n_r > 60 and n_d == n_r
    same_slots(V, RF, "rig")


# ---- SearchByProjection(Frame, KeyFrame, sAlreadyFound), ORBmatcher.cc:2291 ----------------------------------------------------------
@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("name", ["pinhole", "distorted", "kb8"])
def test_search_reloc_keyframe(pkg, ref, matchers, name, check_ori):
    S = MC.reloc_keyframe(name)
    V, R = both(pkg, ref, S["cur"])
    before = V.slot.copy()
    V.slot_obs[V.slot >= 0] = 1                            # the entry's contract (include/orbhip.h): every occupant blocks, so all are passed as observed
    n_d = matchers(0.9, check_ori).SearchByProjectionKeyFrame(V, MC.SF, MC.LOG_SF, (S["state"] == 1).astype(np.uint8), S["Xw"], S["mpdesc"],
                                                                      S["kf_angle"], S["max_dist"], S["min_dist"], S["Tcw"], S["cam_type"], S["cam"],
                                                                      S["th"], S["orb_dist"])
    n_r = R.search_by_projection_kf(S["state"], S["Xw"], S["mpdesc"], S["kf_angle"], S["max_dist"], S["min_dist"], S["Tcw"], S["cam_type"], S["cam"],
                                    S["th"], S["orb_dist"], check_ori=check_ori)
    assert n_r > 40 and n_d == n_r
    kept = (V.slot >= 0) & (V.slot == before)
    V.slot_obs[kept] = S["cur"]["slot_obs"][kept]          # the occupants nobody replaced are the caller's own objects
    same_slots(V, R, name)


# ---- SearchByBoW(KeyFrame, Frame), ORBmatcher.cc:273 ---------------------------------------------------------------------------------
def bow_views(pkg, ref, S, has_mp=None):
    ones = np.ones(MC.NLEVELS, f32)
    has_mp = S["has_mp"] if has_mp is None else has_mp
    KV = pkg.KeyFrameView(pkg_keys(pkg, S["kf_keys"]), S["kf_desc"], S["kf_fv"], MC.SF, ones, has_mappoint=(has_mp == 1).astype(np.uint8))
    FV = pkg.KeyFrameView(pkg_keys(pkg, S["f_keys"]), S["f_desc"], S["f_fv"], MC.SF, ones)
    KR = ref.OracleKeyFrame(S["kf_keys"], S["kf_desc"], S["kf_fv"], MC.SF, ones, has_mp=has_mp)
    FR = ref.OracleKeyFrame(S["f_keys"], S["f_desc"], S["f_fv"], MC.SF, ones)
    return KV, FV, KR, FR


def pkg_keys(pkg, k):
    out = np.zeros(len(k), pkg.KP_DTYPE)
    for f in ("x", "y", "octave", "angle"):
        out[f] = k[f]
    return out


@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("name", ["mono", "fisheye", "rig"])
def test_search_by_bow(pkg, ref, matchers, name, check_ori):
    S = MC.bow(name)
    KV, FV, KR, FR = bow_views(pkg, ref, S)
    n_d, m_d = matchers(S["nnratio"], check_ori).SearchByBoW(KV, FV, n_left=None if S["n_left"] == -1 else S["n_left"])
    n_r, m_r = ref.ref_search_by_bow(KR, FR, S["nnratio"], check_ori, n_left=S["n_left"], kf_n_left=S["kf_n_left"])
    assert n_r >= 30 and n_d == n_r
    assert np.array_equal(m_d, m_r)


@pytest.mark.parametrize("name", ["mono", "fisheye"])
def test_search_by_bow_candidates(pkg, ref, matchers, name):
    """Relocalization's loop in one call: three candidate keyframes (the scene's, one with every other map point gone, one with
    none bad) against the one frame; each row is what the compiled member returns for that keyframe."""
    S = MC.bow(name)
    variants = [S["has_mp"], np.where(np.arange(len(S["has_mp"])) % 2 == 0, S["has_mp"], 0).astype(np.uint8), np.minimum(S["has_mp"], 1).astype(np.uint8)]
    views = [bow_views(pkg, ref, S, v) for v in variants]
    nl = None if S["n_left"] == -1 else S["n_left"]
    nm, rows = matchers(S["nnratio"], True).SearchByBoWCandidates([v[0] for v in views], views[0][1], n_left=nl)
    for j, (_, _, KR, FR) in enumerate(views):
        n_r, m_r = ref.ref_search_by_bow(KR, FR, S["nnratio"], True, n_left=S["n_left"], kf_n_left=S["kf_n_left"])
        assert n_r >= 15 and int(nm[j]) == n_r, j
        assert np.array_equal(rows[j], m_r), j


# ---- SearchForInitialization, ORBmatcher.cc:722 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("name", ["euroc", "distorted"])
def test_search_for_initialization(pkg, ref, matchers, name, check_ori):
    S = MC.initialization(name)
    fr = S["f2"]
    F1 = pkg.FrameView(pkg_keys(pkg, S["keys1"]), S["desc1"], fr["bounds"])
    F2 = pkg.FrameView(keys_of(pkg, fr), fr["desc"], fr["bounds"])
    R2 = ref.RefFrame(ref.OracleFrame(fr["kx"], fr["ky"], fr["octave"], fr["angle"], fr["desc"], fr["bounds"], MC.SF))
    p_d, p_r = S["prev"].copy(), S["prev"].copy()
    n_d, m_d = matchers(S["nnratio"], check_ori).SearchForInitialization(F1, F2, p_d, S["window"])
    n_r, m_r = ref.ref_search_for_initialization(S["keys1"], S["desc1"], R2, p_r, S["window"], S["nnratio"], check_ori)
    assert n_r > 60 and n_d == n_r
    assert np.array_equal(m_d, m_r)
    assert np.array_equal(p_d.view(np.uint32), p_r.view(np.uint32))
