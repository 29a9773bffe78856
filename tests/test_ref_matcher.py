"""CPU: the oracle's matcher restatements against the reference's own src/ORBmatcher.cc, compiled.

oracle/_ref/libref_matcher.so is the reference's unmodified ORBmatcher.cc (with Pinhole.cpp and KannalaBrandt8.cpp, which it calls)
built against the stand-in headers of oracle/ref_cam_shim and oracle/ref_match_driver.cc.  Every bit-exact claim about the product's
matcher is "HIP equals oracle/orb_oracle.c"; this file is what ties orb_oracle.c to the text it restates.  A misreading of a tie
rule, of a < against a <=, of a ratio test, a level window, a histogram bin or an occupied-slot rule that the oracle, the numpy models
and the kernels share shows here.  What stays on both sides: the driver's own Frame / KeyFrame / MapPoint members
and the stand-in's reading of the OpenCV primitives.

Every comparison is array_equal of the return value and of every output array.  The library is built here when the reference tree is
present; the tests skip only where there is neither a library nor a tree.  Inputs and the census: tests/ref_matcher_cases.py.
"""
import numpy as np
import pytest

import ref_matcher_cases as MC

f32 = np.float32


@pytest.fixture(scope="module")
def ref(oracle):
    oracle.build_ref()
    try:
        oracle.ref_match_lib()
    except RuntimeError:
        pytest.skip("no oracle/_ref/libref_matcher.so and no reference tree to build it from")
    return oracle


def oracle_frame(oracle, fr, slot=None, slot_obs=None):
    F = oracle.OracleFrame(fr["kx"], fr["ky"], fr["octave"], fr["angle"], fr["desc"], fr["bounds"], MC.SF, u_right=fr.get("u_right"))
    F.slot[:] = fr["slot"] if slot is None else slot
    F.slot_obs[:] = fr["slot_obs"] if slot_obs is None else slot_obs
    return F


def same_slots(F, R, what):
    """slot and slot_obs of the oracle's frame F and the compiled text's R; slot_obs only means something where the slot is taken."""
    assert np.array_equal(F.slot, R.slot), "%s: mvpMapPoints differ at %s" % (what, np.flatnonzero(F.slot != R.slot)[:8])
    assert np.array_equal(np.where(F.slot >= 0, F.slot_obs, 0), R.slot_obs), what


# ---- the three small members -------------------------------------------------------------------------------------------------------
def test_descriptor_distance(ref):
    a, b = MC.descriptor_pairs()
    for x, y in zip(a, b):
        want = ref.ref_descriptor_distance(x, y)
        assert want == MC.hamming(x, y)
        assert ref.descriptor_distance(x, y) == want


def test_three_maxima(ref):
    lone = equal = 0
    for sizes in MC.three_maxima_cases():
        want = ref.ref_three_maxima(sizes)
        assert tuple(ref.three_maxima(sizes)) == want, sizes
        top = np.sort(sizes)[::-1]
        lone += int(top[0] > 0 and want[1] == -1)
        equal += int(top[0] > 0 and top[0] == top[1])
    assert lone >= 1 and equal >= 1


def test_radius_by_viewing_cos(ref):
    for v in MC.VIEW_COS:
        assert ref.radius_by_viewing_cos(v) == ref.ref_radius_by_viewing_cos(v), v


# ---- the driver's own grid against the oracle's: the enumeration order the ties depend on ------------------------------------------------
@pytest.mark.parametrize("name", ["mono", "distorted"])
def test_features_in_area_order(ref, name):
    S = MC.local_points(name)
    F = oracle_frame(ref, S["frame"])
    R = ref.RefFrame(F)
    rng = np.random.default_rng(7)
    b = S["frame"]["bounds"]
    many = 0
    for _ in range(300):
        x, y = float(rng.uniform(b[0] - 30, b[1] + 30)), float(rng.uniform(b[2] - 30, b[3] + 30))
        r, lo = float(rng.choice([3.0, 12.0, 40.0, 300.0])), int(rng.integers(-1, 8))
        hi = int(rng.choice([-1, lo, lo + 1, 7]))
        got, want = F.features_in_area(x, y, r, lo, hi), R.features_in_area(x, y, r, lo, hi)
        assert np.array_equal(got, want)
        many += len(want) > 3
    assert many >= 50


# ---- SearchByProjection(Frame, MapPoints), ORBmatcher.cc:44 -------------------------------------------------------------------------
def run_local(ref, S, far):
    fr, q = S["frame"], S["q"]
    F = oracle_frame(ref, fr)
    R = ref.RefFrame(F)
    in_view = q["in_view"] & (1 - q["bad"])
    if far:
        in_view = in_view & (q["depth"] <= f32(S["th_far"])).astype(np.uint8)
    xr = q["projXR"] if fr["u_right"] is not None else None
    n_o, _ = F.search_by_projection_mp(in_view, q["desc"], q["projX"], q["projY"], q["viewCos"], q["level"], S["th"], S["nnratio"], qobs=q["obs"], projXR=xr)
    n_r = R.search_by_projection_mp(q["in_view"], q["desc"], q["projX"], q["projY"], q["viewCos"], q["level"], S["th"], S["nnratio"], qobs=q["obs"],
                                    projXR=xr, bad=q["bad"], track_depth=q["depth"], far_points=far, th_far=S["th_far"])
    return n_o, n_r, F, R


@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("name", ["mono", "stereo", "distorted"])
def test_search_local_points(ref, name, far):
    n_o, n_r, F, R = run_local(ref, MC.local_points(name), far)
    assert n_r > 100
    assert n_o == n_r
    same_slots(F, R, name)


def test_search_local_points_th_one(ref):
    """th == 1.0 leaves the radius alone (bFactor)."""
    S = dict(MC.local_points("stereo"), th=1.0)
    n_o, n_r, F, R = run_local(ref, S, False)
    assert n_o == n_r and n_r > 30
    same_slots(F, R, "th=1")


def test_search_local_points_fisheye(ref):
    S = MC.local_points_fisheye()
    q = S["q"]
    mk = lambda fr: ref.OracleFrame(fr["kx"], fr["ky"], fr["octave"], fr["angle"], fr["desc"], fr["bounds"], MC.SF)
    OF = ref.OracleFisheyeFrame(mk(S["left"]), mk(S["right"]))
    OF.slot[:], OF.slot_obs[:] = S["slot"], S["slot_obs"]
    RF = ref.RefFisheyeFrame(OF)
    args = (S["l2r"], S["r2l"], q["in_view"], q["in_view_r"], q["desc"], q["projX"], q["projY"], q["viewCos"], q["level"], q["projXR"], q["projYR"],
            q["viewCosR"], q["levelR"], S["th"], S["nnratio"])
    n_o, ml, mr = OF.search_by_projection_mp(*args, qobs=q["obs"])
    n_r = RF.search_by_projection_mp(*args, qobs=q["obs"])
    assert n_r > 100 and (ml >= 0).sum() > 40 and (mr >= 0).sum() > 40
    assert n_o == n_r
    same_slots(OF, RF, "fisheye")


# ---- SearchByProjection(Frame, Frame), ORBmatcher.cc:2027 ---------------------------------------------------------------------------
@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("name", ["mono", "stereo-forward", "stereo-backward", "stereo-still", "distorted"])
def test_search_last_frame(ref, name, check_ori):
    S = MC.last_frame(name)
    F = oracle_frame(ref, S["cur"])
    R = ref.RefFrame(F)
    kw = dict(mono=S["mono"], check_ori=check_ori, mb=S["mb"], mbf=S["mbf"], qobs=S["obs"])
    args = (S["Xw"], S["mpdesc"], S["last_octave"], S["last_angle"], S["Tcw"], S["Tlw"], S["cam_type"], S["cam"], S["th"])
    n_o = F.search_by_projection_ff((S["has_mp"] == 1).astype(np.uint8), *args, **kw)
    n_r = R.search_by_projection_ff(S["has_mp"], *args, **kw)
    assert n_r > 60
    assert n_o == n_r
    same_slots(F, R, name)


@pytest.mark.parametrize("check_ori", [True, False])
def test_search_last_frame_open_windows(ref, check_ori):
    """Every query sees every keypoint (forward motion, octave 0, a window wider than the image): the first of equal distances in
    grid order wins, query after query, with the slots filling up."""
    S = MC.last_frame_open()
    F = oracle_frame(ref, S["cur"])
    R = ref.RefFrame(F)
    b = S["cur"]["bounds"]
    assert len(R.features_in_area(float(b[1]) - 1.0, float(b[2]) + 1.0, S["th"], 0, -1)) == len(S["cur"]["kx"]) - 4      # open: all of the grid
    kw = dict(mono=False, check_ori=check_ori, mb=S["mb"], mbf=S["mbf"], qobs=S["obs"])
    args = (S["Xw"], S["mpdesc"], S["last_octave"], S["last_angle"], S["Tcw"], S["Tlw"], S["cam_type"], S["cam"], S["th"])
    n_o = F.search_by_projection_ff((S["has_mp"] == 1).astype(np.uint8), *args, **kw)
    n_r = R.search_by_projection_ff(S["has_mp"], *args, **kw)
    assert n_r >= 30 and n_o == n_r                      # a quarter of the 120 keypoints: the scene is not idle
    same_slots(F, R, "open")
    # the scene decides ties: at least 20 accepted matches went to a keypoint whose descriptor another free keypoint shares
    taken = np.flatnonzero((R.slot >= 0) & (R.slot < 100000))
    shared = sum(1 for m in taken if (S["letter"] == S["letter"][m]).sum() > 1)
    assert shared >= 20, shared


@pytest.mark.parametrize("check_ori", [True, False])
def test_search_last_frame_rig(ref, check_ori):
    S = MC.last_frame("rig")
    mk = lambda fr: ref.OracleFrame(fr["kx"], fr["ky"], fr["octave"], fr["angle"], fr["desc"], fr["bounds"], MC.SF)
    OF = ref.OracleFisheyeFrame(mk(S["cur"]), mk(S["right"]))
    OF.slot[:], OF.slot_obs[:] = S["slot"], S["slot_obs"]
    RF = ref.RefFisheyeFrame(OF)
    args = (S["Xw"], S["mpdesc"], S["last_octave"], S["last_angle"], S["Tcw"], S["Tlw"], S["Trl"], S["cam_type"], S["cam"], S["th"])
    kw = dict(mono=False, check_ori=check_ori, mb=S["mb"], qobs=S["obs"])
    n_o = OF.search_by_projection_ff((S["has_mp"] == 1).astype(np.uint8), *args, **kw)
    n_r = RF.search_by_projection_ff(S["has_mp"], *args, **kw)
    nl = len(S["cur"]["kx"])
    assert n_r > 60 and (RF.slot[nl:] < 100000).sum() - (RF.slot[nl:] < 0).sum() > 20      # the right image took matches of its own
    assert n_o == n_r
    same_slots(OF, RF, "rig")


# ---- SearchByProjection(Frame, KeyFrame, sAlreadyFound), ORBmatcher.cc:2291 ----------------------------------------------------------
@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("name", ["pinhole", "distorted", "kb8"])
def test_search_reloc_keyframe(ref, name, check_ori):
    S = MC.reloc_keyframe(name)
    F = oracle_frame(ref, S["cur"])
    R = ref.RefFrame(F)
    n_o = ref.search_by_projection_kf(F, (S["state"] == 1).astype(np.uint8), S["Xw"], S["mpdesc"], S["kf_angle"], S["max_dist"], S["min_dist"], S["Tcw"],
                                      S["cam_type"], S["cam"], MC.LOG_SF, S["th"], S["orb_dist"], check_ori=check_ori)
    n_r = R.search_by_projection_kf(S["state"], S["Xw"], S["mpdesc"], S["kf_angle"], S["max_dist"], S["min_dist"], S["Tcw"], S["cam_type"], S["cam"],
                                    S["th"], S["orb_dist"], check_ori=check_ori)
    assert n_r > 40
    assert n_o == n_r
    same_slots(F, R, name)


# ---- SearchByBoW(KeyFrame, Frame), ORBmatcher.cc:273 ---------------------------------------------------------------------------------
def bow_sides(oracle, S):
    ones = np.ones(MC.NLEVELS, f32)
    KF = oracle.OracleKeyFrame(S["kf_keys"], S["kf_desc"], S["kf_fv"], MC.SF, ones, has_mp=(S["has_mp"] == 1).astype(np.uint8))
    KFr = oracle.OracleKeyFrame(S["kf_keys"], S["kf_desc"], S["kf_fv"], MC.SF, ones, has_mp=S["has_mp"])        # 2 = a bad point
    F = oracle.OracleKeyFrame(S["f_keys"], S["f_desc"], S["f_fv"], MC.SF, ones)
    return KF, KFr, F


@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("name", ["mono", "fisheye", "rig"])
def test_search_by_bow(ref, name, check_ori):
    S = MC.bow(name)
    KF, KFr, F = bow_sides(ref, S)
    n_o, m_o = ref.search_by_bow(KF, F, S["nnratio"], check_ori, n_left=S["n_left"])
    n_r, m_r = ref.ref_search_by_bow(KFr, F, S["nnratio"], check_ori, n_left=S["n_left"], kf_n_left=S["kf_n_left"])
    assert n_r >= 30                                        # a tenth of the keyframe's keypoints: the scene is not idle
    if S["n_left"] != -1:
        assert (m_r[S["n_left"]:] >= 0).sum() > 10
    assert n_o == n_r
    assert np.array_equal(m_o, m_r)


# ---- SearchForInitialization, ORBmatcher.cc:722 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("name", ["euroc", "distorted"])
def test_search_for_initialization(ref, name, check_ori):
    S = MC.initialization(name)
    fr = S["f2"]
    F2 = ref.OracleFrame(fr["kx"], fr["ky"], fr["octave"], fr["angle"], fr["desc"], fr["bounds"], MC.SF)
    R2 = ref.RefFrame(F2)
    p_o, p_r = S["prev"].copy(), S["prev"].copy()
    n_o, m_o = ref.search_for_initialization(S["keys1"], S["desc1"], F2, p_o, S["window"], S["nnratio"], check_ori)
    n_r, m_r = ref.ref_search_for_initialization(S["keys1"], S["desc1"], R2, p_r, S["window"], S["nnratio"], check_ori)
    assert n_r > 60
    assert n_o == n_r
    assert np.array_equal(m_o, m_r)
    assert np.array_equal(p_o.view(np.uint32), p_r.view(np.uint32))
    assert not np.array_equal(p_r, S["prev"])


# ---- the census: the decisive rules actually decide on these inputs (DESIGN.md section 2 has the table) -----------------------------------
def at_least(c, minimum, *keys):
    for k in keys:
        print("census %-32s %4d (minimum %d)" % (k, c.get(k, 0), minimum))
    short = {k: c.get(k, 0) for k in keys if c.get(k, 0) < minimum}
    assert not short, "census below the minimum of %d: %r" % (minimum, short)


def planted(slot_of, S, th):
    """How many planted pairs exactly at the threshold were kept, and how many one bit beyond it were dropped."""
    kept = sum(1 for q, m, d in S["edge"] if d == th and slot_of(m) == q)
    dropped = sum(1 for q, m, d in S["edge"] if d == th + 1 and slot_of(m) != q)
    return kept, dropped


def test_census_local_points(ref):
    total = MC.Census()
    for name in ("mono", "stereo", "distorted"):
        S = MC.local_points(name)
        n_o, n_r, F, R = run_local(ref, S, False)
        RA = ref.RefFrame(oracle_frame(ref, S["frame"]))
        n_m, slot, obs, c = MC.census_local_points(S, RA.features_in_area)
        assert n_m == n_r and np.array_equal(slot, R.slot) and np.array_equal(np.where(slot >= 0, obs, 0), R.slot_obs), "the replay is wrong"
        kept, dropped = planted(lambda m: R.slot[m], S, MC.TH_HIGH)
        assert kept >= 5 and dropped >= 5, (name, kept, dropped)
        for k, v in c.items():
            total.hit(k, v)
    at_least(total, 20, "tie", "same-level", "other-level", "ratio-near")
    at_least(total, 10, "occupied-observed", "occupied-unobserved", "level-0", "level-top", "er-edge")
    at_least(total, 5, "at-TH_HIGH")


@pytest.mark.parametrize("name", ["mono", "stereo-still", "distorted"])
def test_census_last_frame(ref, name):
    S = MC.last_frame(name)
    F = oracle_frame(ref, S["cur"])
    R = ref.RefFrame(F)
    n = R.search_by_projection_ff(S["has_mp"], S["Xw"], S["mpdesc"], S["last_octave"], S["last_angle"], S["Tcw"], S["Tlw"], S["cam_type"], S["cam"],
                                  S["th"], mono=S["mono"], check_ori=False, mb=S["mb"], mbf=S["mbf"], qobs=S["obs"])
    assert n > 60
    kept, dropped = planted(lambda m: R.slot[m], S, MC.TH_HIGH)
    assert kept >= 5 and dropped >= 5, (kept, dropped)
    wraps = sum(1 for i, m in S["wrap"] if R.slot[m] == i and MC.rot_bin(S["last_angle"][i], S["cur"]["angle"][m]) == MC.HISTO_LENGTH)
    assert wraps >= 3, wraps
    c = MC.census_projections(S, S["Xw"], S["has_mp"] == 1, S["Tcw"])
    at_least(c, 10, "behind", "outside-by-less-than-a-pixel", "inside-by-less-than-a-pixel")


@pytest.mark.parametrize("name", ["pinhole", "distorted", "kb8"])
def test_census_reloc_keyframe(ref, name):
    S = MC.reloc_keyframe(name)
    R = ref.RefFrame(oracle_frame(ref, S["cur"]))
    n = R.search_by_projection_kf(S["state"], S["Xw"], S["mpdesc"], S["kf_angle"], S["max_dist"], S["min_dist"], S["Tcw"], S["cam_type"], S["cam"], S["th"],
                                  S["orb_dist"], check_ori=False)
    assert n > 40
    kept, dropped = planted(lambda m: R.slot[m], S, S["orb_dist"])
    assert kept >= 5 and dropped >= 5, (kept, dropped)
    wraps = sum(1 for i, m in S["wrap"] if R.slot[m] == i and MC.rot_bin(S["kf_angle"][i], S["cur"]["angle"][m]) == MC.HISTO_LENGTH)
    assert wraps >= 3, wraps
    at_least(MC.census_predicted_levels(S), 10, "level-0", "level-top", "out-of-band")


def test_census_bow(ref):
    S = MC.bow("mono")
    KF, KFr, F = bow_sides(ref, S)
    n_r, m_r = ref.ref_search_by_bow(KFr, F, S["nnratio"], False)
    n_m, m_m, c = MC.census_bow(S)
    assert n_m == n_r and np.array_equal(m_m, m_r), "the replay is wrong"
    kept, dropped = planted(lambda fi: m_r[fi], S, MC.TH_LOW)
    assert kept >= 5 and dropped >= 5, (kept, dropped)
    wraps = sum(1 for ki, fi in S["wrap"] if m_r[fi] == ki and MC.rot_bin(S["kf_keys"]["angle"][ki], S["f_keys"]["angle"][fi]) == MC.HISTO_LENGTH)
    assert wraps >= 3, wraps
    at_least(c, 20, "tie", "ratio-near")
    at_least(c, 10, "two-claims")
    at_least(c, 5, "at-TH_LOW")


@pytest.mark.parametrize("name", ["fisheye", "rig"])
def test_census_bow_right_image(ref, name):
    """The right image's own edge and wrap of the fisheye-stereo branch (ORBmatcher.cc:407-436) decide."""
    S = MC.bow(name)
    KF, KFr, F = bow_sides(ref, S)
    n_r, m_r = ref.ref_search_by_bow(KFr, F, S["nnratio"], False, n_left=S["n_left"], kf_n_left=S["kf_n_left"])
    kept = sum(1 for ki, fj, d in S["edge_r"] if d == MC.TH_LOW and m_r[fj] == ki)
    dropped = sum(1 for ki, fj, d in S["edge_r"] if d == MC.TH_LOW + 1 and m_r[fj] != ki)
    assert kept >= 5 and dropped >= 5, (kept, dropped)
    ang_k, ang_f = S["kf_keys"]["angle"], S["f_keys"]["angle"]
    wraps = sum(1 for ki, fj in S["wrap_r"] if m_r[fj] == ki and MC.rot_bin(ang_k[ki], ang_f[fj]) == MC.HISTO_LENGTH)
    assert wraps >= 3, wraps
    n_c, m_c = ref.ref_search_by_bow(KFr, F, S["nnratio"], True, n_left=S["n_left"], kf_n_left=S["kf_n_left"])
    assert all(m_c[fj] == -1 for ki, fj in S["wrap_r"]), "bin 0 is not among the three maxima: the wrapped pairs are pruned"


def test_census_initialization(ref):
    total = MC.Census()
    for name in ("euroc", "distorted"):
        S = MC.initialization(name)
        fr = S["f2"]
        R2 = ref.RefFrame(ref.OracleFrame(fr["kx"], fr["ky"], fr["octave"], fr["angle"], fr["desc"], fr["bounds"], MC.SF))
        n_r, m_r = ref.ref_search_for_initialization(S["keys1"], S["desc1"], R2, S["prev"].copy(), S["window"], S["nnratio"], False)
        n_m, m_m, c = MC.census_initialization(S, R2.features_in_area)
        assert n_m == n_r and np.array_equal(m_m, m_r), "the replay is wrong"
        kept, dropped = planted(lambda m, m_r=m_r: int(np.flatnonzero(m_r == m)[0]) if (m_r == m).any() else -1, S, MC.TH_LOW)
        assert kept >= 5 and dropped >= 5, (kept, dropped)
        wraps = sum(1 for i, m in S["wrap"] if m_r[i] == m and MC.rot_bin(S["keys1"]["angle"][i], fr["angle"][m]) == MC.HISTO_LENGTH)
        assert wraps >= 3, wraps
        for k, v in c.items():
            total.hit(k, v)
    at_least(total, 20, "tie", "ratio-near")
    at_least(total, 10, "two-claims")
    at_least(total, 5, "at-TH_LOW")
