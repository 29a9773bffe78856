"""GPU: SearchForTriangulation for KannalaBrandt8 keyframes and two-camera KannalaBrandt8 rigs with the epipolar test on the device
(orbm_search_for_triangulation_kb8: candidate lists, KannalaBrandt8::TriangulateMatches on every candidate, minimum accepted key).

The reference on both sides is the oracle's restatement of the member (oracle.search_for_triangulation_pred, ORBmatcher.cc:981-1222)
around the numpy model's epipolarConstrain, np.float32(triangulate_matches(...)[0]) > np.float32(0.0001) - independent of the product's
source.  The results are indices, so every comparison is exact.  The entry must also equal the route it replaces, the library's own
orbm_search_for_triangulation_pred around the same Python predicate.  The scene is tests/triangulation_kb8_scene.py; the model's
verdict on a keypoint pair is computed once per scene and shared."""
import ctypes as C

import numpy as np
import pytest

import triangulation_kb8_scene as SC

pytestmark = pytest.mark.gpu

_verdicts = {}


def pred_of(S):
    """The model's predicate with the verdicts of this scene kept (n_left decides the camera pair, so it is part of the key)."""
    memo = _verdicts.setdefault((id(S["k1"]), S["n_left1"], S["n_left2"]), {})
    raw = SC.predicate(S)

    def pred(i1, i2):
        if (i1, i2) not in memo:
            memo[(i1, i2)] = raw(i1, i2)
        return memo[(i1, i2)]
    return pred


@pytest.fixture()
def matcher(pkg):
    m = pkg.ORBmatcher(0.6, False)
    yield m
    m.close()


def kb8(m, S, K1, K2, **kw):
    return m.SearchForTriangulationKB8(K1, K2, S["ep"], S["cams1"], S["cams2"], S["T12"], S["n_left1"], S["n_left2"], **kw)


def check(pkg, oracle, m, S, nodes, check_ori=False, only_stereo=False, ur1=None, ur2=None, fv1=None, fv2=None, route=True):
    """new entry == oracle + model (== the predicate route); returns (nmatches, pairs)."""
    m.mbCheckOrientation = check_ori
    K1, K2 = SC.product_views(pkg, S, nodes, ur1, ur2, fv1, fv2)
    O1, O2 = SC.oracle_views(oracle, S, nodes, None if S["rig"] else ur1, None if S["rig"] else ur2, fv1, fv2)   # a rig's oracle is fed -1
    n_ref, pairs_ref = oracle.search_for_triangulation_pred(O1, O2, S["ep"], not S["rig"], pred_of(S), only_stereo=only_stereo, check_ori=check_ori)
    n, pairs = kb8(m, S, K1, K2, bOnlyStereo=only_stereo)
    assert n == n_ref and np.array_equal(pairs, pairs_ref)
    if route:
        P1, P2 = SC.product_views(pkg, S, nodes, None if S["rig"] else ur1, None if S["rig"] else ur2, fv1, fv2)
        n_old, pairs_old = m.SearchForTriangulationPred(P1, P2, S["ep"], not S["rig"], pred_of(S), bOnlyStereo=only_stereo)
        assert n == n_old and np.array_equal(pairs, pairs_old)
    return n, pairs


@pytest.mark.parametrize("check_ori", [False, True])
@pytest.mark.parametrize("n,nodes", [(96, 4), (400, 16)])
@pytest.mark.parametrize("rig", [False, True])
def test_parity_with_oracle_and_model_and_predicate_route(pkg, oracle, matcher, rig, n, nodes, check_ori):
    S = SC.scene(n, rig)
    nm, pairs = check(pkg, oracle, matcher, S, nodes, check_ori)
    assert nm >= (10 if check_ori else 40)
    if not check_ori:   # the geometry decided: some answers are not the nearest, latest candidate
        O1, O2 = SC.oracle_views(oracle, S, nodes)
        st, i2, _ = oracle.triangulation_candidates(O1, O2, S["ep"], not rig)
        assert sum(1 for a, b in pairs if i2[st[a]] != b) >= 8


@pytest.mark.parametrize("only_stereo", [True, False])
def test_stereo_keypoints_of_keyframes_without_a_second_camera(pkg, oracle, matcher, only_stereo):
    """40 % of the keypoints on both sides with mvuRight >= 0: bOnlyStereo keeps only them (:1057-1061, :1088-1090), and the epipole
    gate applies only where neither keypoint is stereo (:1105); the epipole of the forward pose is inside the image."""
    S = SC.scene(96, False, SC.FORWARD)
    rng = np.random.default_rng(3)
    ur1 = np.where(rng.random(len(S["k1"])) < 0.4, S["k1"]["x"] - np.float32(9), np.float32(-1)).astype(np.float32)
    ur2 = np.where(rng.random(len(S["k2"])) < 0.4, S["k2"]["x"] - np.float32(9), np.float32(-1)).astype(np.float32)
    nm, _ = check(pkg, oracle, matcher, S, 4, only_stereo=only_stereo, ur1=ur1, ur2=ur2)
    assert nm >= 3
    O1, O2 = SC.oracle_views(oracle, S, 4, ur1, ur2)
    mono = SC.oracle_views(oracle, S, 4)
    gated = lambda a, b: len(oracle.triangulation_candidates(a, b, S["ep"], True)[1])
    assert gated(*mono) < gated(O1, O2) or only_stereo        # stereo keypoints escape the gate


@pytest.mark.parametrize("rig", [False, True])
def test_coarse_takes_the_first_entry_of_every_list(pkg, oracle, matcher, rig):
    S = SC.scene(96, rig)
    K1, K2 = SC.product_views(pkg, S, 4)
    O1, O2 = SC.oracle_views(oracle, S, 4)
    st, i2, _ = oracle.triangulation_candidates(O1, O2, S["ep"], not rig)
    first = np.array([(i, i2[st[i]]) for i in range(len(st) - 1) if st[i + 1] > st[i]], np.int64)
    n, pairs = kb8(matcher, S, K1, K2, bCoarse=True)
    assert n == len(first) > 40 and np.array_equal(pairs, first)
    n_ref, pairs_ref = oracle.search_for_triangulation_pred(O1, O2, S["ep"], not rig, lambda a, b: False, coarse=True)
    assert n == n_ref and np.array_equal(pairs, pairs_ref)


def test_rigs_ignore_u_right(pkg, oracle, matcher):
    """bStereo = !mpCamera2 && mvuRight >= 0 (:1057, :1086): whatever mvuRight holds on a rig, the result is that of all -1, and
    bOnlyStereo leaves nothing."""
    S = SC.scene(96, True)
    rng = np.random.default_rng(4)
    ur1, ur2 = rng.uniform(0, 500, len(S["k1"])).astype(np.float32), rng.uniform(0, 500, len(S["k2"])).astype(np.float32)
    a = check(pkg, oracle, matcher, S, 4, ur1=ur1, ur2=ur2)
    b = check(pkg, oracle, matcher, S, 4, route=False)
    assert a[0] == b[0] > 40 and np.array_equal(a[1], b[1])
    assert check(pkg, oracle, matcher, S, 4, only_stereo=True, ur1=ur1, ur2=ur2)[0] == 0


@pytest.mark.parametrize("n,nodes", [(96, 4), (400, 16)])
def test_forward_pose_epipole_inside_the_image(pkg, oracle, matcher, n, nodes):
    S = SC.scene(n, False, SC.FORWARD)
    assert check(pkg, oracle, matcher, S, nodes)[0] >= 40
    O1, O2 = SC.oracle_views(oracle, S, nodes)
    assert len(oracle.triangulation_candidates(O1, O2, S["ep"], True)[1]) < len(oracle.triangulation_candidates(O1, O2, S["ep"], False)[1])


@pytest.mark.parametrize("rig", [False, True])
def test_one_node_wider_than_a_wavefront(pkg, oracle, matcher, rig):
    S = SC.scene(400, rig)
    fv1, fv2 = {9: list(range(len(S["k1"])))}, {9: list(range(len(S["k2"])))}
    assert check(pkg, oracle, matcher, S, 1, fv1=fv1, fv2=fv2)[0] >= 200
    assert check(pkg, oracle, matcher, S, 1, check_ori=True, fv1=fv1, fv2=fv2, route=False)[0] >= 40


def test_no_shared_node(pkg, matcher):
    S = SC.scene(96, True)
    K1, K2 = SC.product_views(pkg, S, 1, fv1={3: list(range(len(S["k1"])))}, fv2={5: list(range(len(S["k2"])))})
    n, pairs = kb8(matcher, S, K1, K2)
    assert n == 0 and len(pairs) == 0


@pytest.mark.parametrize("left1,left2", [(False, False), (True, True), (False, True), (True, False)])
def test_all_left_and_all_right_rigs(pkg, oracle, matcher, left1, left2):
    """n_left = n (every keypoint the left camera's) and n_left = 0 (every keypoint the right camera's): one camera pair for all."""
    base = SC.scene(96, True)
    S = dict(base, n_left1=len(base["k1"]) if left1 else 0, n_left2=len(base["k2"]) if left2 else 0)
    check(pkg, oracle, matcher, S, 4)


def test_empty_keyframes(pkg, matcher):
    S = SC.scene(96, True)
    K1, K2 = SC.product_views(pkg, S, 4)
    none = pkg.KeyFrameView(np.zeros(0, pkg.KP_DTYPE), np.zeros((0, 32), np.uint8), {}, S["sf"], S["sigma2"])
    for a, b, nl1, nl2 in ((none, K2, 0, S["n_left2"]), (K1, none, S["n_left1"], 0), (none, none, 0, 0)):
        n, pairs = matcher.SearchForTriangulationKB8(a, b, S["ep"], S["cams1"], S["cams2"], S["T12"], nl1, nl2)
        assert n == 0 and len(pairs) == 0
    mono = SC.scene(96, False)
    M1, _ = SC.product_views(pkg, mono, 4)
    n, pairs = matcher.SearchForTriangulationKB8(M1, none, mono["ep"], mono["cams1"], mono["cams2"], mono["T12"])
    assert n == 0 and len(pairs) == 0


def test_refusals(pkg, matcher):
    """Every ORBX_E_ARG of include/orbhip.h, next to a live handle; the handle works afterwards."""
    S, R = SC.scene(96, False), SC.scene(96, True)
    K1, K2 = SC.product_views(pkg, S, 4)
    Q1, Q2 = SC.product_views(pkg, R, 4)
    m = matcher
    refused = lambda: pytest.raises(ValueError, match="bad argument")
    rig_args = (R["ep"], R["cams1"], R["cams2"], R["T12"])
    for miss in range(3):                                                      # NULL cams1 / cams2 / T12
        args = [S["cams1"], S["cams2"], S["T12"]]
        args[miss] = None
        with refused():
            m.SearchForTriangulationKB8(K1, K2, S["ep"], *args)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    s1, s2, m12 = K1.struct(), K2.struct(), np.full(K1.N, -1, np.int32)
    T12, c1, c2 = np.ascontiguousarray(S["T12"]), np.ascontiguousarray(S["cams1"]), np.ascontiguousarray(S["cams2"])
    raw = lambda a, b, out: m.L.orbm_search_for_triangulation_kb8(m.m, a, -1, b, -1, C.c_float(0), C.c_float(0), p(c1), p(c2), p(T12), 0, 0, 0, out)
    assert raw(None, C.byref(s2), p(m12)) == pkg.E_ARG and raw(C.byref(s1), None, p(m12)) == pkg.E_ARG and raw(C.byref(s1), C.byref(s2), None) == pkg.E_ARG
    for field in ("keys_un", "descriptors", "u_right", "has_mappoint", "node_id", "node_start", "node_idx", "scale_factors", "level_sigma2"):
        for side in (0, 1):                                                    # a NULL array inside either keyframe
            t = [K1.struct(), K2.struct()]
            setattr(t[side], field, None)
            assert raw(C.byref(t[0]), C.byref(t[1]), p(m12)) == pkg.E_ARG, (field, side)
    for side, K in ((0, K1), (1, K2)):                                         # a feature vector that is not one
        back = K.node_start.copy()
        K.node_start[1] = K.node_start[2] + 1                                  # node_start decreases
        t = [K1.struct(), K2.struct()]
        rc = raw(C.byref(t[0]), C.byref(t[1]), p(m12))
        K.node_start[:] = back
        assert rc == pkg.E_ARG, side
    for K in (K1, K2):                                                         # a member of a node outside [0, n)
        for bad_idx in (-1, K.N):
            keep = int(K.node_idx[0])
            K.node_idx[0] = bad_idx
            rc = raw(C.byref(s1), C.byref(s2), p(m12))
            K.node_idx[0] = keep
            assert rc == pkg.E_ARG, bad_idx
    for nl1, nl2 in ((-1, R["n_left2"]), (R["n_left1"], -1)):                  # one keyframe with, one without a second camera
        with refused():
            m.SearchForTriangulationKB8(Q1, Q2, *rig_args, nl1, nl2)
    for nl1, nl2 in ((Q1.N + 1, R["n_left2"]), (R["n_left1"], Q2.N + 1), (-2, R["n_left2"]), (R["n_left1"], -2)):
        with refused():
            m.SearchForTriangulationKB8(Q1, Q2, *rig_args, nl1, nl2)
    for levels in (0, 17):                                                     # nlevels outside [1, ORBX_MAX_LEVELS], either keyframe
        tab = np.ones(max(levels, 1), np.float32)[:levels]
        bad = pkg.KeyFrameView(S["k1"], S["d1"], SC.bow(S["d1"], 4), tab, tab)
        with refused():
            m.SearchForTriangulationKB8(bad, K2, S["ep"], S["cams1"], S["cams2"], S["T12"])
        bad = pkg.KeyFrameView(S["k2"], S["d2"], SC.bow(S["d2"], 4), tab, tab)
        with refused():
            m.SearchForTriangulationKB8(K1, bad, S["ep"], S["cams1"], S["cams2"], S["T12"])
    for octave in (8, -1):                                                     # mvLevelSigma2[octave] would be read out of range
        for side in (1, 2):
            keys = S["k%d" % side].copy()
            keys["octave"][len(keys) // 2] = octave
            bad = pkg.KeyFrameView(keys, S["d%d" % side], SC.bow(S["d%d" % side], 4), S["sf"], S["sigma2"])
            with refused():
                m.SearchForTriangulationKB8(*((bad, K2) if side == 1 else (K1, bad)), S["ep"], S["cams1"], S["cams2"], S["T12"])
    big = 65536                                                                # a vocabulary node of KF2 with more than 65535 members
    node = next(iter(SC.bow(S["d1"], 4)))
    wide = pkg.KeyFrameView(np.zeros(big, pkg.KP_DTYPE), np.zeros((big, 32), np.uint8), {node: list(range(big))}, S["sf"], S["sigma2"])
    with refused():
        m.SearchForTriangulationKB8(K1, wide, S["ep"], S["cams1"], S["cams2"], S["T12"])
    n, _ = kb8(m, S, K1, K2)
    assert n >= 40


def test_handle_reuse_across_scenes(pkg, oracle, matcher):
    """Two scenes of different sizes through one handle, in both orders: best[], the candidate total and the output are per call."""
    A, B = SC.scene(400, True), SC.scene(96, False)
    first = check(pkg, oracle, matcher, A, 16, route=False)
    small = check(pkg, oracle, matcher, B, 4, route=False)
    again = check(pkg, oracle, matcher, A, 16, route=False)
    assert first[0] == again[0] and np.array_equal(first[1], again[1])
    assert check(pkg, oracle, matcher, B, 4, check_ori=True, route=False)[0] <= small[0]
