"""GPU: SearchForTriangulation of one keyframe against all its neighbours in one call (orbm_search_for_triangulation_neighbours,
orbm_search_for_triangulation_kb8_neighbours; the loop of LocalMapping::CreateNewMapPoints, LocalMapping.cc:475-583).

Expected values: the oracle's per-pair member (Pinhole) and the oracle's member around the numpy model's epipolarConstrain
(KannalaBrandt8, tests/triangulation_kb8_scene.py), independent of the product's source; every row must also equal the per-pair device
entry it replaces.  The results are keypoint indices, so every comparison is exact.  The scenes are built once per process and shared
(tests/triangulation_neighbours_scene.py, tests/triangulation_kb8_scene.py); tests/test_triangulation_neighbours_abi.py shows on the
oracle alone that they reach what is claimed here."""
import ctypes as C
import threading

import numpy as np
import pytest

import triangulation_kb8_scene as SC
import triangulation_neighbours_scene as NS
from test_gpu_triangulation_kb8 import check as kb8_check
from test_gpu_triangulation_kb8 import pred_of
from test_triangulation_neighbours_abi import kb8_scenes

pytestmark = pytest.mark.gpu


@pytest.fixture()
def matcher(pkg):
    m = pkg.ORBmatcher(0.6, False)
    yield m
    m.close()


def pinhole(m, pkg, S, mp=None, which=None, **kw):
    """(rows [K, n1], nmatches [K], views) of the one-call entry for the neighbours `which` of S."""
    nbs = S["nbs"] if which is None else [S["nbs"][j] for j in which]
    views = [NS.product_nb(pkg, nb) for nb in nbs]
    rows, nm = m.SearchForTriangulationNeighbours(NS.product_kf1(pkg, S, mp), views, S["R1w"], S["t1w"], S["Cw1"], S["cam"], [nb["R2w"] for nb in nbs],
                                                  [nb["t2w"] for nb in nbs], [S["cam"]] * len(nbs), **kw)
    return rows, nm


def per_pair_row(m, pkg, S, j, **kw):
    nb = S["nbs"][j]
    n, pairs = m.SearchForTriangulation(NS.product_kf1(pkg, S), NS.product_nb(pkg, nb), S["R1w"], S["t1w"], nb["R2w"], nb["t2w"], S["Cw1"], S["cam"], S["cam"], **kw)
    row = np.full(len(S["k1"]), -1, np.int32)
    row[pairs[:, 0]] = pairs[:, 1]
    return n, row


@pytest.mark.parametrize("only_stereo,coarse", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("skip", [None, (0, 0, 0, 1)])
def test_pinhole_rows_equal_oracle_and_per_pair_entry(pkg, oracle, matcher, skip, only_stereo, coarse):
    """K = 4: a neighbour with a node of more than 64 members, one without a shared node, one with n = 0, one skipped (or searched);
    different n and nlevels, map points and stereo keypoints on both sides."""
    S = NS.scene(NS.MAIN)
    rows, nm = pinhole(matcher, pkg, S, skip=skip, bOnlyStereo=only_stereo, bCoarse=coarse)
    assert rows.shape == (4, len(S["k1"])) and rows.dtype == np.int32
    for j, nb in enumerate(S["nbs"]):
        if skip is not None and skip[j]:
            assert np.all(rows[j] == -1) and nm[j] == 0
            continue
        want = NS.oracle_row(oracle, S, j, only_stereo=only_stereo, coarse=coarse)
        assert np.array_equal(rows[j], want), j
        n_dev, row_dev = per_pair_row(matcher, pkg, S, j, bOnlyStereo=only_stereo, bCoarse=coarse)
        assert np.array_equal(rows[j], row_dev) and nm[j] == n_dev == (want >= 0).sum()
        assert nm[j] >= 10 if nb["kind"] == "real" else nm[j] == 0


def test_pinhole_second_trip_of_a_wavefront(pkg, oracle, matcher):
    """The wide node's answers lie beyond position 64 of the node."""
    S = NS.scene(NS.MAIN)
    rows, _ = pinhole(matcher, pkg, S)
    members = S["nbs"][0]["fv"][NS.WIDE_KEY]
    assert len(members) > 64
    assert sum(1 for v in rows[0] if v >= 0 and v in members and members.index(v) >= 64) >= 3
    assert np.array_equal(rows[0], NS.oracle_row(oracle, S, 0))


@pytest.mark.parametrize("kinds", [NS.MAIN, NS.REPLAY], ids=["main", "replay"])
def test_pinhole_tie_the_later_node_position_wins_in_every_row(pkg, oracle, matcher, kinds):
    S = NS.scene(kinds)
    rows, _ = pinhole(matcher, pkg, S)
    for j, nb in enumerate(S["nbs"]):
        if nb["kind"] != "real":
            continue
        first, later = {a for a, _ in nb["twins"]}, {b for _, b in nb["twins"]}
        assert sum(1 for v in rows[j] if v in later) >= 5 and not any(v in first for v in rows[j]), j
        assert np.array_equal(rows[j], NS.oracle_row(oracle, S, j))


@pytest.mark.parametrize("only_stereo,coarse", [(False, False), (True, False), (False, True)])
def test_replay_of_the_sequential_loop_proves_the_masking_rule(pkg, oracle, matcher, only_stereo, coarse):
    """The reference's loop on the oracle, KF1's keypoints receiving map points after every neighbour, against ONE call made from the
    state at loop entry and masked by the same evolving flags: identical for every neighbour."""
    S = NS.scene(NS.REPLAY)
    seq, flags = NS.replay(S, lambda j, has: NS.oracle_row(oracle, S, j, mp=has, only_stereo=only_stereo, coarse=coarse))
    rows, nm = pinhole(matcher, pkg, S, bOnlyStereo=only_stereo, bCoarse=coarse)
    got = NS.masked(rows, S, flags)
    changed = 0
    for j in range(len(seq)):
        assert np.array_equal(got[j], seq[j]), j
        changed += int((got[j] != rows[j]).sum())
    assert changed >= 10 and np.all(nm >= 10)


def kb8_call(m, pkg, Ss, nodes=4, **kw):
    K1, _ = SC.product_views(pkg, Ss[0], nodes)
    views = [SC.product_views(pkg, S, nodes)[1] for S in Ss]
    rig = Ss[0]["rig"]
    return m.SearchForTriangulationKB8Neighbours(K1, views, [S["ep"] for S in Ss], Ss[0]["cams1"], [S["cams2"] for S in Ss], [S["T12"] for S in Ss],
                                                 Ss[0]["n_left1"], [S["n_left2"] for S in Ss] if rig else None, **kw)


def kb8_row(n1, pairs):
    row = np.full(n1, -1, np.int32)
    row[pairs[:, 0]] = pairs[:, 1]
    return row


@pytest.mark.parametrize("coarse", [False, True])
@pytest.mark.parametrize("rig", [False, True])
def test_kb8_rows_equal_oracle_model_and_per_pair_entry(pkg, oracle, matcher, rig, coarse):
    """K = 3 scenes that share KF1, the second with the epipole inside the neighbour's image."""
    Ss = kb8_scenes(rig)
    rows, nm = kb8_call(matcher, pkg, Ss, bCoarse=coarse)
    n1 = len(Ss[0]["k1"])
    assert rows.shape == (3, n1)
    for j, S in enumerate(Ss):
        O1, O2 = SC.oracle_views(oracle, S, 4)
        n_ref, pairs_ref = oracle.search_for_triangulation_pred(O1, O2, S["ep"], not rig, pred_of(S), coarse=coarse, check_ori=False)
        assert np.array_equal(rows[j], kb8_row(n1, pairs_ref)) and nm[j] == n_ref, j
        K1, K2 = SC.product_views(pkg, S, 4)
        n_dev, pairs_dev = matcher.SearchForTriangulationKB8(K1, K2, S["ep"], S["cams1"], S["cams2"], S["T12"], S["n_left1"], S["n_left2"], bCoarse=coarse)
        assert np.array_equal(rows[j], kb8_row(n1, pairs_dev)) and nm[j] == n_dev
        assert nm[j] >= 10 and (rows[j] < 0).sum() >= 1
    skipped, nm_s = kb8_call(matcher, pkg, Ss, skip=[0, 1, 0], bCoarse=coarse)
    assert np.array_equal(skipped[0], rows[0]) and np.array_equal(skipped[2], rows[2]) and np.all(skipped[1] == -1) and list(nm_s) == [nm[0], 0, nm[2]]


def test_kb8_a_rig_next_to_a_single_camera_keyframe_is_refused(pkg, matcher):
    Ss = kb8_scenes(True)
    K1, _ = SC.product_views(pkg, Ss[0], 4)
    views = [SC.product_views(pkg, S, 4)[1] for S in Ss]
    args = ([S["ep"] for S in Ss], Ss[0]["cams1"], [S["cams2"] for S in Ss], [S["T12"] for S in Ss])
    with pytest.raises(ValueError, match="neighbour 1: n_left"):
        matcher.SearchForTriangulationKB8Neighbours(K1, views, *args, Ss[0]["n_left1"], [Ss[0]["n_left2"], -1, Ss[2]["n_left2"]])
    rows, nm = matcher.SearchForTriangulationKB8Neighbours(K1, views, *args, Ss[0]["n_left1"], [Ss[0]["n_left2"], -1, Ss[2]["n_left2"]], skip=[0, 1, 0])
    assert nm[0] >= 10 and nm[1] == 0 and nm[2] >= 10        # a skipped neighbour is not validated


def test_nothing_to_search_returns_zero(pkg, matcher):
    """K == 0 and all neighbours skipped: 0, rows of -1, with tables that only searched neighbours need left out."""
    S = NS.scene(NS.MAIN)
    K1 = NS.product_kf1(pkg, S)
    rows, nm = matcher.SearchForTriangulationNeighbours(K1, [], S["R1w"], S["t1w"], S["Cw1"], S["cam"], [], [], [])
    assert rows.shape == (0, K1.N) and len(nm) == 0
    rows, nm = pinhole(matcher, pkg, S, skip=[1, 1, 1, 1])
    assert np.all(rows == -1) and np.all(nm == 0)
    views = [NS.product_nb(pkg, nb) for nb in S["nbs"]]
    rows, nm = matcher.SearchForTriangulationNeighbours(K1, views, None, None, None, None, None, None, None, skip=[1, 1, 1, 1])
    assert np.all(rows == -1) and np.all(nm == 0)
    Ss = kb8_scenes(False)
    rows, nm = kb8_call(matcher, pkg, Ss, skip=[1, 1, 1])
    assert np.all(rows == -1) and np.all(nm == 0)
    Q1, _ = SC.product_views(pkg, Ss[0], 4)
    rows, nm = matcher.SearchForTriangulationKB8Neighbours(Q1, [], [], Ss[0]["cams1"], [], [])
    assert rows.shape == (0, Q1.N) and len(nm) == 0


def test_refusals_name_the_neighbour(pkg, matcher):
    """A fault in neighbour 2 only: ORBX_E_ARG, orbm_last_error names neighbour 2; the handle works afterwards."""
    S = NS.scene(NS.REPLAY)
    K1 = NS.product_kf1(pkg, S)
    args = (S["R1w"], S["t1w"], S["Cw1"], S["cam"], [nb["R2w"] for nb in S["nbs"]], [nb["t2w"] for nb in S["nbs"]], [S["cam"]] * 4)

    def views_with(j, **change):
        return [NS.product_nb(pkg, dict(nb, **change) if i == j else nb) for i, nb in enumerate(S["nbs"])]

    nb2 = S["nbs"][2]
    for octave in (nb2["nlevels"], -1):                                          # an octave outside [0, nlevels) of neighbour 2
        keys = nb2["k"].copy()
        keys["octave"][len(keys) // 2] = octave
        with pytest.raises(ValueError, match="neighbour 2: keypoint octave"):
            matcher.SearchForTriangulationNeighbours(K1, views_with(2, k=keys), *args)
    assert b"neighbour 2" in matcher.L.orbm_last_error(matcher.m)
    for bad in (-1, len(nb2["k"])):                                              # a node member outside [0, n)
        fv = {k: list(v) for k, v in nb2["fv"].items()}
        fv[next(iter(fv))][0] = bad
        with pytest.raises(ValueError, match="neighbour 2: feature vector"):
            matcher.SearchForTriangulationNeighbours(K1, views_with(2, fv=fv), *args)
    for levels in (0, 17):                                                       # nlevels outside [1, ORBX_MAX_LEVELS]
        tab = np.ones(max(levels, 1), np.float32)[:levels]
        with pytest.raises(ValueError, match="neighbour 2: nlevels"):
            matcher.SearchForTriangulationNeighbours(K1, views_with(2, sf=tab, sigma2=tab), *args)
    views = views_with(2)
    views[2].node_start[1] = views[2].node_start[2] + 1                          # node_start decreases
    with pytest.raises(ValueError, match="neighbour 2: feature vector: node_start"):
        matcher.SearchForTriangulationNeighbours(K1, views, *args)
    s1 = K1.struct()
    raw = lambda K, tab: matcher.L.orbm_search_for_triangulation_neighbours(matcher.m, C.byref(s1), K, tab, None, None, None, None, None, None, None, None, 0, 0,
                                                                            None, None)
    assert raw(-1, None) == pkg.E_ARG and b"K < 0" in matcher.L.orbm_last_error(matcher.m)
    assert raw(4, None) == pkg.E_ARG and b"NULL neighbour table" in matcher.L.orbm_last_error(matcher.m)
    assert raw(0, None) == 0
    with pytest.raises(ValueError, match="NULL pose or camera table"):
        matcher.SearchForTriangulationNeighbours(K1, views_with(2), None, *args[1:])
    # the KannalaBrandt8 form: the same fault in neighbour 2
    Ss = kb8_scenes(False)
    Q1, _ = SC.product_views(pkg, Ss[0], 4)
    qviews = [SC.product_views(pkg, T, 4)[1] for T in Ss]
    keys = Ss[2]["k2"].copy()
    keys["octave"][3] = 8
    qviews[2] = pkg.KeyFrameView(keys, Ss[2]["d2"], SC.bow(Ss[2]["d2"], 4), Ss[2]["sf"], Ss[2]["sigma2"], has_mappoint=Ss[2]["mp2"])
    with pytest.raises(ValueError, match="neighbour 2: keypoint octave"):
        matcher.SearchForTriangulationKB8Neighbours(Q1, qviews, [T["ep"] for T in Ss], Ss[0]["cams1"], [T["cams2"] for T in Ss], [T["T12"] for T in Ss])
    rows, nm = pinhole(matcher, pkg, S)
    assert np.all(nm >= 10)


# ---- the per-pair entries (KannalaBrandt8: the one-call form with K = 1 and the rotation histogram behind it) ----------------------
def pinhole_pair(m, pkg, oracle, S, nb, check_ori=False, only_stereo=False):
    """(nmatches, pairs) of orbm_search_for_triangulation for KF1 of S and the neighbour nb, equal to the oracle's member."""
    m.mbCheckOrientation = check_ori
    n, pairs = m.SearchForTriangulation(NS.product_kf1(pkg, S), NS.product_nb(pkg, nb), S["R1w"], S["t1w"], nb["R2w"], nb["t2w"], S["Cw1"], S["cam"], S["cam"],
                                        bOnlyStereo=only_stereo)
    n_ref, pairs_ref = oracle.search_for_triangulation(NS.oracle_kf1(oracle, S), NS.oracle_nb(oracle, nb), S["R1w"], S["t1w"], nb["R2w"], nb["t2w"], S["Cw1"],
                                                       S["cam"], S["cam"], only_stereo=only_stereo, coarse=False, check_ori=check_ori)
    assert n == n_ref == len(pairs) and np.array_equal(pairs, pairs_ref)
    return n, pairs


def node_of_65(fv, shared):
    """(feature vector, key): a copy of fv in which the largest node that is also in `shared` holds exactly 65 keypoints, a wavefront
    and one: short of that, members taken from the front of the other nodes stand IN FRONT of its own (random descriptors, far from
    everything the node is asked for); beyond that, its first members move into a node nobody shares."""
    fv = {k: list(v) for k, v in fv.items()}
    key = max((k for k in fv if k in shared), key=lambda k: len(fv[k]))
    if len(fv[key]) > 65:
        fv[max(max(fv), max(shared)) + 1], fv[key] = fv[key][:-65], fv[key][-65:]
    pad = []
    for k in fv:
        while k != key and len(fv[key]) + len(pad) < 65 and len(fv[k]) > 1:
            pad.append(fv[k].pop(0))
    fv[key] = pad + fv[key]
    assert len(fv[key]) == 65
    return fv, key


def answer_in_the_last_place(fv, key, answers):
    """fv with a keypoint that the search answers with moved to position 64 of node `key`, the one lane of the second trip.  It had the
    smallest distance among the accepted candidates of its keypoint of KF1; a later position only helps it (`dist > bestDist -> skip`,
    update on <=), so it stays an answer."""
    last = next(int(v) for v in answers(fv) if v in fv[key])
    fv = dict(fv)
    fv[key] = [v for v in fv[key] if v != last] + [last]
    assert fv[key].index(last) == 64 and last in answers(fv)
    return fv


@pytest.mark.parametrize("only_stereo", [False, True])
def test_pinhole_pair_entry_prunes_by_rotation(pkg, oracle, matcher, only_stereo):
    """checkOri exists on the pair entry alone.  The keypoint angles are random on both sides, so the three fullest of the 30 bins keep
    a fraction of the pairs.  mvuRight is >= 0 for 60 % of the keypoints of both keyframes: bOnlyStereo drops the rest (:1057-1061,
    :1088-1090)."""
    S = NS.scene(NS.MAIN)
    nb = S["nbs"][0]
    assert all((ur >= 0).any() and (ur < 0).any() for ur in (S["ur1"], nb["ur"]))
    plain, pairs = pinhole_pair(matcher, pkg, oracle, S, nb, only_stereo=only_stereo)
    pruned, _ = pinhole_pair(matcher, pkg, oracle, S, nb, check_ori=True, only_stereo=only_stereo)
    assert 1 <= pruned < plain
    mono = (S["ur1"][pairs[:, 0]] < 0) | (nb["ur"][pairs[:, 1]] < 0)
    assert not mono.any() if only_stereo else mono.any()


def test_pinhole_pair_entry_node_of_65_members(pkg, oracle, matcher):
    S = NS.scene(NS.MAIN)
    nb = S["nbs"][3]
    fv, key = node_of_65(nb["fv"], S["fv1"])
    answers = lambda f: pinhole_pair(matcher, pkg, oracle, S, dict(nb, fv=f))[1][:, 1]
    fv = answer_in_the_last_place(fv, key, answers)
    assert pinhole_pair(matcher, pkg, oracle, S, dict(nb, fv=fv), check_ori=True)[0] >= 1


def test_pinhole_pair_entry_nothing_to_search(pkg, matcher):
    """n1 = 0, n2 = 0, no shared node: 0 and a row of -1 (written by the entry: the row arrives full of 7)."""
    S = NS.scene(NS.MAIN)
    none = pkg.KeyFrameView(np.zeros(0, SC.KP_DTYPE), np.zeros((0, 32), np.uint8), {}, S["sf1"], S["sigma2_1"], u_right=np.zeros(0, np.float32),
                            has_mappoint=np.zeros(0, np.uint8))
    K1, real, nonode, empty = NS.product_kf1(pkg, S), NS.product_nb(pkg, S["nbs"][0]), NS.product_nb(pkg, S["nbs"][1]), NS.product_nb(pkg, S["nbs"][2])
    f = lambda v: np.ascontiguousarray(v, np.float32)
    nb = S["nbs"][0]
    poses = [f(v) for v in (S["R1w"], S["t1w"], nb["R2w"], nb["t2w"], S["Cw1"], S["cam"], S["cam"])]
    for a, b in ((none, real), (K1, empty), (K1, nonode), (none, empty)):
        s1, s2, row = a.struct(), b.struct(), np.full(max(a.N, 1), 7, np.int32)
        for check_ori in (0, 1):
            row[:] = 7
            rc = matcher.L.orbm_search_for_triangulation(matcher.m, C.byref(s1), C.byref(s2), *[pkg._p(v) for v in poses], 0, 0, check_ori, pkg._p(row))
            assert rc == 0 and np.all(row[:a.N] == -1) and np.all(row[a.N:] == 7)


@pytest.mark.parametrize("rig", [False, True])
def test_kb8_pair_entry_prunes_by_rotation(pkg, oracle, matcher, rig):
    S = SC.scene(96, rig)
    plain, _ = kb8_check(pkg, oracle, matcher, S, 4, route=False)
    pruned, _ = kb8_check(pkg, oracle, matcher, S, 4, check_ori=True, route=False)
    assert 1 <= pruned < plain


@pytest.mark.parametrize("rig", [False, True])
def test_kb8_pair_entry_node_of_65_members(pkg, oracle, matcher, rig):
    S = SC.scene(96, rig)
    fv2, key = node_of_65(SC.bow(S["d2"], 4), SC.bow(S["d1"], 4))
    answers = lambda f: kb8_check(pkg, oracle, matcher, S, 4, fv2=f, route=False)[1][:, 1]
    fv2 = answer_in_the_last_place(fv2, key, answers)
    assert kb8_check(pkg, oracle, matcher, S, 4, check_ori=True, fv2=fv2, route=False)[0] >= 1


def test_two_handles_on_two_threads(pkg, oracle):
    """Two orbm_t on two host threads, concurrently, with different K: the rows of serial calls."""
    S = NS.scene(NS.REPLAY)
    jobs = {"a": (None, 4), "b": ((1, 3), 2)}
    ms = {k: pkg.ORBmatcher(0.6, False) for k in jobs}
    try:
        serial = {k: pinhole(ms[k], pkg, S, which=w)[0] for k, (w, _) in jobs.items()}
        out, errs = {k: [] for k in jobs}, []
        start = threading.Barrier(2)

        def run(k):
            try:
                start.wait()
                for _ in range(8):
                    out[k].append(pinhole(ms[k], pkg, S, which=jobs[k][0])[0])
            except Exception as e:          # noqa: BLE001
                errs.append(e)

        ts = [threading.Thread(target=run, args=(k,)) for k in jobs]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        for k, (w, K) in jobs.items():
            assert len(out[k]) == 8 and all(r.shape == (K, len(S["k1"])) and np.array_equal(r, serial[k]) for r in out[k])
        assert np.array_equal(serial["b"], serial["a"][[1, 3]])
        for j in range(4):
            assert np.array_equal(serial["a"][j], NS.oracle_row(oracle, S, j))
    finally:
        for m in ms.values():
            m.close()
