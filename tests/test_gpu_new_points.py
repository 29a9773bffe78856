"""GPU: LocalMapping::CreateNewMapPoints in one call (orbm_create_new_map_points, orbm_create_new_map_points_kb8) and the body of its loop
over device arrays (orbm_new_point_geometry_device).

Expected values: the oracle's search, the numpy model of the body (tests/new_points_model.py) and the replay of the reference's
sequential loop (tests/new_points_scene.py), independent of the product's source; tests/test_new_points_model.py shows on the CPU that the
scenes reach what is claimed here.  Indices, status bytes and the bits of x3D: every comparison is exact."""
import ctypes as C
import threading

import numpy as np
import pytest

import new_points_model as NM
import new_points_scene as PS
import triangulation_kb8_scene as SC
import triangulation_neighbours_scene as NS
from test_gpu_triangulation_kb8 import pred_of
from test_triangulation_neighbours_abi import KB8_CENTRES, kb8_scenes

pytestmark = pytest.mark.gpu


@pytest.fixture()
def matcher(pkg):
    m = pkg.ORBmatcher(0.6, False)
    yield m
    m.close()


def pinhole_call(m, pkg, S, **kw):
    K1, G1, views, Gs = PS.product_pinhole(pkg, S)
    nbs = S["nbs"]
    return m.CreateNewMapPoints(K1, G1, PS.SCALE_FACTOR, views, Gs, S["R1w"], S["t1w"], S["Cw1"], S["cam"], [nb["R2w"] for nb in nbs], [nb["t2w"] for nb in nbs],
                                [S["cam"]] * len(nbs), **kw)


def kb8_call(m, pkg, Ss, E, **kw):
    K1, G1, views, Gs = PS.product_kb8(pkg, Ss, E.c1, E.c2)
    rig = Ss[0]["rig"]
    return m.CreateNewMapPointsKB8(K1, G1, PS.SCALE_FACTOR, views, Gs, [S["ep"] for S in Ss], Ss[0]["cams1"], [S["cams2"] for S in Ss], [S["T12"] for S in Ss],
                                   Ss[0]["n_left1"], [S["n_left2"] for S in Ss] if rig else None, **kw)


def check(E, got, skip=None):
    """The four outputs of a one-call entry against the loop-entry tables and the replay of the sequential loop."""
    pts, st, m12, nm = got
    rows, nmatches, status, _ = E.tables(skip)
    assert np.array_equal(m12, rows) and np.array_equal(nm, nmatches)
    assert np.array_equal(st, status), [(j, i, NM.STATUS[a], NM.STATUS[b]) for (j, i), a, b in zip(np.argwhere(st != status), st[st != status], status[st != status])][:5]
    want = E.replay(skip)
    assert PS.same_list(PS.as_list(pts), want), (len(pts), len(want))
    return want


@pytest.mark.parametrize("far,th_far", [(False, 0.0), (True, 6.0)])
@pytest.mark.parametrize("coarse", [False, True])
@pytest.mark.parametrize("skip", [None, (0, 1, 0, 0)])
def test_pinhole_equals_replay_and_model(pkg, oracle, matcher, skip, coarse, far, th_far):
    S = PS.pinhole(NS.REPLAY)
    E = PS.expected_pinhole(oracle, S, coarse=coarse, far=far, th_far=th_far)
    want = check(E, pinhole_call(matcher, pkg, S, skip=skip, bCoarse=coarse, far_points=far, th_far_points=th_far), skip)
    assert len(want) >= 15
    pts, st, m12, nm = pinhole_call(matcher, pkg, S, skip=skip, bCoarse=coarse, far_points=far, th_far_points=th_far, status=False, matches=False)
    assert st is None and m12 is None and nm is None and PS.same_list(PS.as_list(pts), want)     # matches12 = NULL: not downloaded


def test_pinhole_neighbours_without_work(pkg, oracle, matcher):
    """MAIN: a neighbour without a shared node and one with n = 0 between two real ones."""
    S = PS.pinhole(NS.MAIN)
    want = check(PS.expected_pinhole(oracle, S), pinhole_call(matcher, pkg, S))
    assert {p[0] for p in want} == {0, 3}


@pytest.mark.parametrize("coarse", [False, True])
@pytest.mark.parametrize("rig", [False, True], ids=["single", "rig"])
def test_kb8_equals_replay_and_model(pkg, oracle, matcher, rig, coarse):
    Ss = kb8_scenes(rig)
    E = PS.expected_kb8(oracle, Ss, KB8_CENTRES, pred_of, coarse=coarse)
    want = check(E, kb8_call(matcher, pkg, Ss, E, bCoarse=coarse))
    assert len(want) >= 20
    check(E, kb8_call(matcher, pkg, Ss, E, bCoarse=coarse, skip=[0, 1, 0]), (0, 1, 0))
    Ef = PS.expected_kb8(oracle, Ss, KB8_CENTRES, pred_of, coarse=coarse, far=True, th_far=3.0)
    far = check(Ef, kb8_call(matcher, pkg, Ss, Ef, bCoarse=coarse, far_points=True, th_far_points=3.0))
    assert 0 < len(far) < len(want)


def test_body_over_device_arrays_equals_the_host_form(pkg):
    import torch
    groups = [(c1, c2, o1, o2, far, th) for _, c1, c2, o1, o2, far, th in PS.planted()]
    Ss = kb8_scenes(True)
    c1, c2 = PS.make_kb8(Ss, KB8_CENTRES)
    rng = np.random.default_rng(3)
    i1, i2 = rng.integers(0, len(Ss[0]["k1"]), 300), rng.integers(0, len(Ss[0]["k2"]), 300)     # any pairs: 300 = one block and a partial one
    o1 = PS.observations(Ss[0]["k1"], None, None, None, i1, Ss[0]["n_left1"])
    o2 = PS.observations(Ss[0]["k2"], None, None, None, i2, Ss[0]["n_left2"])
    groups.append((c1, c2[0], o1, o2, False, 0.0))
    seen = set()
    for c1, c2, o1, o2, far, th in groups:
        st, X = pkg.new_point_geometry(c1, c2, o1, o2, PS.SCALE_FACTOR, far, th)
        n = len(o1)
        d1 = torch.from_numpy(np.ascontiguousarray(o1).view(np.uint8).reshape(-1).copy()).cuda()
        d2 = torch.from_numpy(np.ascontiguousarray(o2).view(np.uint8).reshape(-1).copy()).cuda()
        dst, dX = torch.full((n,), 99, dtype=torch.uint8, device="cuda"), torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        pkg.new_point_geometry_device(n, c1, c2, d1.data_ptr(), d2.data_ptr(), PS.SCALE_FACTOR, far, th, dst.data_ptr(), dX.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), st) and np.array_equal(dX.cpu().numpy().view(np.uint32), X.view(np.uint32))
        seen |= set(st.tolist())
    assert seen == set(range(1, len(NM.STATUS)))


_small = {}


def small_scene(K, n1, seed=11):
    if (K, n1, seed) not in _small:
        kinds = tuple(("real", (140, 120, 130, 150)[j], (8, 6, 7, 8)[j], False) for j in range(K))
        _small[(K, n1, seed)] = PS.make_pinhole(kinds, n1=n1, seed=seed)
    return _small[(K, n1, seed)]


@pytest.mark.parametrize("K,n1", [(1, 65), (1, 200), (2, 128), (2, 130), (3, 256), (2, 300)])
def test_shapes_at_the_lane_block_and_chunk_boundaries(pkg, oracle, matcher, K, n1):
    """K * n1 lanes: across one 64-lane boundary (65), exactly one block (2 * 128), a block and a partial one (2 * 130), whole blocks
    (3 * 256); k_new_points_emit walks a row 256 keypoints at a time: n1 = 256 exactly and 300.  K = 1: every entry of one neighbour."""
    S = small_scene(K, n1)
    want = check(PS.expected_pinhole(oracle, S), pinhole_call(matcher, pkg, S))
    assert len(want) >= 5


def test_list_at_cap_and_one_over(pkg, oracle, matcher):
    S = PS.pinhole(NS.REPLAY)
    want = PS.expected_pinhole(oracle, S).replay()
    pts, _, _, _ = pinhole_call(matcher, pkg, S, cap=len(want))
    assert PS.same_list(PS.as_list(pts), want)
    over, st, m12, _ = pinhole_call(matcher, pkg, S, cap=len(want) - 1)
    assert over == len(want) and (st == NM.ACCEPTED).sum() >= len(want) and (m12 >= 0).sum() > len(want)     # the count; the tables are still delivered
    assert pinhole_call(matcher, pkg, S, cap=0)[0] == len(want)


def test_one_idx2_matched_by_two_idx1_is_emitted_twice(pkg, oracle, matcher):
    """Sixty keypoints of KF1 twice (same pixel, descriptor, depth): both copies match the same idx2 and, as in the reference - pKF2's
    AddMapPoint(pMP, idx2) at :893 overwrites, nothing reads it - both create a point."""
    S = PS.with_duplicates(PS.pinhole(NS.REPLAY), 60)
    want = check(PS.expected_pinhole(oracle, S), pinhole_call(matcher, pkg, S))
    assert len(PS.shared_idx2(want)) >= 4


def test_seeded_sweep_of_random_scenes(pkg, oracle, matcher):
    """20 scenes: poses, stereo share, octaves (through the seed), th_far_points."""
    total = 0
    for seed in range(100, 120):
        rng = np.random.default_rng(seed)
        poses = tuple((float(rng.uniform(-0.04, 0.04)), float(rng.uniform(-0.03, 0.03)), tuple(float(v) for v in rng.uniform(-0.35, 0.35, 3))) for _ in range(3))
        kinds = tuple(("real", int(rng.integers(30, 48)), int(rng.integers(5, 9)), False) for _ in range(3))
        S = PS.make_pinhole(kinds, n1=48, seed=seed, poses=poses, stereo_share=float(rng.uniform(0.0, 0.9)))
        far, th_far = bool(seed % 2), float(rng.uniform(3.0, 9.0))
        E = PS.expected_pinhole(oracle, S, far=far, th_far=th_far)
        total += len(check(E, pinhole_call(matcher, pkg, S, far_points=far, th_far_points=th_far)))
    assert total >= 60


def test_two_handles_on_two_threads(pkg, oracle):
    S = PS.pinhole(NS.REPLAY)
    Ss = kb8_scenes(True)
    Ek = PS.expected_kb8(oracle, Ss, KB8_CENTRES, pred_of)
    want = {"a": PS.expected_pinhole(oracle, S).replay(), "b": Ek.replay()}
    ms = {k: pkg.ORBmatcher(0.6, False) for k in want}
    run_one = {"a": lambda: pinhole_call(ms["a"], pkg, S)[0], "b": lambda: kb8_call(ms["b"], pkg, Ss, Ek)[0]}
    try:
        out, errs = {k: [] for k in want}, []
        start = threading.Barrier(2)

        def run(k):
            try:
                start.wait()
                for _ in range(6):
                    out[k].append(run_one[k]())
            except Exception as e:          # noqa: BLE001
                errs.append(e)

        ts = [threading.Thread(target=run, args=(k,)) for k in want]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        for k in want:
            assert len(out[k]) == 6 and all(PS.same_list(PS.as_list(p), want[k]) for p in out[k])
    finally:
        for m in ms.values():
            m.close()


def test_search_only_entries_are_untouched_by_a_call_on_the_same_handle(pkg, oracle, matcher):
    S = PS.pinhole(NS.REPLAY)
    K1, _, views, _ = PS.product_pinhole(pkg, S)
    args = (S["R1w"], S["t1w"], S["Cw1"], S["cam"], [nb["R2w"] for nb in S["nbs"]], [nb["t2w"] for nb in S["nbs"]], [S["cam"]] * 4)
    before = matcher.SearchForTriangulationNeighbours(K1, views, *args)
    pinhole_call(matcher, pkg, S)
    after = matcher.SearchForTriangulationNeighbours(K1, views, *args)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(before[0], PS.expected_pinhole(oracle, S).tables()[0])
    Ss = kb8_scenes(True)
    Q1, _, qviews, _ = PS.product_kb8(pkg, Ss, *PS.make_kb8(Ss, KB8_CENTRES))
    kargs = ([T["ep"] for T in Ss], Ss[0]["cams1"], [T["cams2"] for T in Ss], [T["T12"] for T in Ss], Ss[0]["n_left1"], [T["n_left2"] for T in Ss])
    before = matcher.SearchForTriangulationKB8Neighbours(Q1, qviews, *kargs)
    E = PS.expected_kb8(oracle, Ss, KB8_CENTRES, pred_of)
    kb8_call(matcher, pkg, Ss, E)
    after = matcher.SearchForTriangulationKB8Neighbours(Q1, qviews, *kargs)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_refusals_name_the_neighbour_and_empty_calls_return_empty_lists(pkg, oracle, matcher):
    S = PS.pinhole(NS.REPLAY)
    K1, G1, views, Gs = PS.product_pinhole(pkg, S)
    nbs = S["nbs"]
    args = (S["R1w"], S["t1w"], S["Cw1"], S["cam"], [nb["R2w"] for nb in nbs], [nb["t2w"] for nb in nbs], [S["cam"]] * 4)
    call = lambda G1_=G1, Gs_=Gs, views_=views, **kw: matcher.CreateNewMapPoints(K1, G1_, PS.SCALE_FACTOR, views_, Gs_, *args, **kw)

    def without(G, *names):
        g = PS.geometry_view(pkg, S["c2"][2], nbs[2]["depth"], nbs[2]["keys"])
        for n in names:
            setattr(g, n, None)
        return [g if j == 2 else x for j, x in enumerate(G)]

    for name in ("Tcw", "Ow"):
        with pytest.raises(ValueError, match="neighbour 2: NULL pose"):
            call(Gs_=without(Gs, name))
    for name in ("depth", "keys", "Twc"):
        with pytest.raises(ValueError, match="neighbour 2: NULL mvDepth, mvKeys or Twc"):
            call(Gs_=without(Gs, name))
    assert b"neighbour 2" in matcher.L.orbm_last_error(matcher.m)
    g1 = PS.geometry_view(pkg, S["c1"], None, S["keys1"])
    with pytest.raises(ValueError, match="kf1: NULL mvDepth"):
        call(G1_=g1)
    with pytest.raises(ValueError, match="NULL keyframe geometry table"):
        call(G1_=None)
    keys = nbs[2]["k"].copy()
    keys["octave"][5] = nbs[2]["nlevels"]                                       # a refusal of the search entry, through this one
    bad = [pkg.KeyFrameView(keys, nbs[2]["d"], nbs[2]["fv"], nbs[2]["sf"], nbs[2]["sigma2"], u_right=nbs[2]["ur"], has_mappoint=nbs[2]["mp"]) if j == 2 else v
           for j, v in enumerate(views)]
    with pytest.raises(ValueError, match="neighbour 2: keypoint octave"):
        call(views_=bad)
    pts, st, m12, nm = call(Gs_=without(Gs, "Tcw", "depth"), skip=[0, 0, 1, 0])     # a skipped neighbour is not validated
    assert PS.same_list(PS.as_list(pts), PS.expected_pinhole(oracle, S).replay((0, 0, 1, 0)))
    # the KannalaBrandt8 form: a rig without its right pose
    Ss = kb8_scenes(True)
    E = PS.expected_kb8(oracle, Ss, KB8_CENTRES, pred_of)
    Q1, H1, qviews, Hs = PS.product_kb8(pkg, Ss, E.c1, E.c2)
    Hs[1].Tcw_right = None
    kargs = ([T["ep"] for T in Ss], Ss[0]["cams1"], [T["cams2"] for T in Ss], [T["T12"] for T in Ss], Ss[0]["n_left1"], [T["n_left2"] for T in Ss])
    with pytest.raises(ValueError, match="neighbour 1: NULL pose"):
        matcher.CreateNewMapPointsKB8(Q1, H1, PS.SCALE_FACTOR, qviews, Hs, *kargs)
    # nothing to do: K == 0, every neighbour skipped (tables only searched neighbours need left out), raw all-NULL next to a live handle
    pts, st, m12, nm = matcher.CreateNewMapPoints(K1, G1, PS.SCALE_FACTOR, [], [], S["R1w"], S["t1w"], S["Cw1"], S["cam"], [], [], [])
    assert len(pts) == 0 and st.shape == (0, K1.N) and len(nm) == 0
    pts, st, m12, nm = matcher.CreateNewMapPoints(K1, None, PS.SCALE_FACTOR, views, None, None, None, None, None, None, None, None, skip=[1, 1, 1, 1])
    assert len(pts) == 0 and not st.any() and np.all(m12 == -1) and not nm.any()
    L = matcher.L
    assert L.orbm_create_new_map_points(matcher.m, None, None, 1.2, 0, *[None] * 10, 0, 0, 0.0, None, 0, None, None, None) == pkg.E_ARG
    assert L.orbm_create_new_map_points_kb8(matcher.m, None, None, 1.2, -1, 0, *[None] * 8, 0, 0, 0.0, None, 0, None, None, None) == pkg.E_ARG
    s1 = K1.struct()
    assert L.orbm_create_new_map_points(matcher.m, C.byref(s1), None, 1.2, 4, *[None] * 10, 0, 0, 0.0, None, 0, None, None, None) == pkg.E_ARG
    assert b"NULL neighbour table" in L.orbm_last_error(matcher.m)
    check(PS.expected_pinhole(oracle, S), call())                               # the handle works afterwards
