"""GPU: the Sim3 overload of ORBmatcher::Fuse for one point list into all corrected keyframes in one call (orbm_fuse_sim3_keyframes,
k_fuse_sim3_gate + k_fuse_sim3_search; LoopClosing::SearchAndFuse, LoopClosing.cc:2631-2707).  Every comparison is on integers and exact.

  * Every row of the one-call entry equals the reference's search (oracle.fuse_sim3) for that target AND the per-target entry
    orbm_fuse_sim3_cam that it replaces - best_idx, best_dist, nfused - on the scene of tests/fuse_sim3_keyframes_scene.py, at th 4.0 and
    8.0; the scale-1 target with the pose as Scw.
  * nP = 1 / T = 1; nP = 257 (a second block with one lane); a target whose first block has no live lane while the second has; keypoint
    counts around the LDS chunk; kf.n == 0, the all-zero valid row and a target with valid points and no live pair; a Scw without a
    usable scale.
  * A small call, the full one and the small one again on one handle (the staged block grows and stays); two handles on two host
    threads; what the entry refuses, with the target named.
  * The SEARCH-AND-FUSE RULE of include/orbhip.h replayed with the rows and the subset searches taken from the device
    (tests/fuse_sim3_rule_model.py)."""
import ctypes as C
import threading

import numpy as np
import pytest

import fuse_sim3_keyframes_scene as SS
import fuse_sim3_rule_model as RM

pytestmark = pytest.mark.gpu
T = len(SS.SCALES)
TH = 4.0


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.ORBmatcher(0.8, False)
    yield m
    m.close()


_rows = {}


def oracle_rows(oracle, S, th, key):
    """The reference's rows of scene S, computed once per (scene key, th) and left unchanged."""
    if (key, th) not in _rows:
        _rows[(key, th)] = [SS.oracle_row(oracle, S, t, th) for t in range(len(S["targets"]))]
    return _rows[(key, th)]


def one_call(pkg, m, S, th):
    return m.FuseSim3KeyFrames([SS.product_target(pkg, tg) for tg in S["targets"]], S["valid"], S["Xw"], S["normal"], S["mpdesc"], S["max_dist"],
                               S["min_dist"], th)


def check(pkg, oracle, m, S, th, key):
    total, bi, bd, nf = one_call(pkg, m, S, th)
    want = oracle_rows(oracle, S, th, key)
    assert bi.shape == bd.shape == (len(S["targets"]), S["nP"])
    for t, (n, wi, wd) in enumerate(want):
        assert np.array_equal(bi[t], wi) and np.array_equal(bd[t], wd) and nf[t] == n, t
    assert total == sum(n for n, _, _ in want)
    return total, bi, bd, nf


@pytest.mark.parametrize("th", [4.0, 8.0])
def test_rows_equal_the_reference_and_the_per_target_entry(pkg, oracle, matcher, th):
    S = SS.scene()
    total, bi, bd, nf = check(pkg, oracle, matcher, S, th, "full")
    assert all(nf[t] >= 100 for t in SS.REAL) and nf[4] == 0 and nf[5] == 0
    assert np.all(bi[4] == -1) and np.all(bd[4] == 256) and np.all(bi[5] == -1) and np.all(bd[5] == 256)   # kf.n == 0; a valid row of zeros
    for t in range(T):
        n, pi, pd = SS.product_row(pkg, matcher, S, t, th)
        assert n == nf[t] and np.array_equal(pi, bi[t]) and np.array_equal(pd, bd[t]), t
    tg = S["targets"][SS.DUP]                                     # the walk order decided, against the index and the chunk
    assert sum(1 for i, b in tg["dupB"].items() if bi[SS.DUP][i] == b and b >= 2 * SS.CHUNK > tg["dupA"][i]) >= 3


def test_the_pose_target_equals_the_per_target_entry_with_the_pose(pkg, matcher):
    """The overload that passes GetPose() (LoopClosing.cc:2686): Scw is the keyframe's 4x4 pose."""
    S = SS.subset(SS.scene(), [SS.POSE], np.arange(SS.NP))
    tg = S["targets"][0]
    assert tg["scale"] == 1.0
    total, bi, bd, nf = one_call(pkg, matcher, S, TH)
    KF = pkg.FrameView(tg["k"], tg["d"], tg["bounds"])
    n, pi, pd = matcher.FuseSim3(KF, tg["sf"], tg["log_sf"], S["valid"][0], S["Xw"], S["normal"], S["mpdesc"], S["max_dist"], S["min_dist"], tg["Tcw"],
                                 tg["cam"], TH, cam_type=tg["cam_type"])
    assert total == n >= 100 and np.array_equal(bi[0], pi) and np.array_equal(bd[0], pd)


def test_one_point_one_target(pkg, oracle, matcher):
    S0 = SS.scene()
    hit = int(np.nonzero(SS.oracle_row(oracle, S0, 0, TH)[1] >= 0)[0][0])
    for i in (hit, int(np.nonzero(S0["group"] == SS.GROUPS.index("behind"))[0][0])):
        S = SS.subset(S0, [0], [i])
        total, bi, bd, nf = check(pkg, oracle, matcher, S, TH, ("one", i))
        assert total == (1 if i == hit else 0)


def test_a_second_block_with_one_lane(pkg, oracle, matcher):
    S0 = SS.scene()
    last = int(np.nonzero((SS.oracle_row(oracle, S0, 0, TH)[1] >= 0) & (SS.oracle_row(oracle, S0, 2, TH)[1] >= 0))[0][-1])
    pts = np.concatenate([np.arange(256), [last]])                # nP = 257: lane 0 of block 1 holds a point that fuses
    S = SS.subset(S0, [0, 2, 3], pts)
    total, bi, bd, nf = check(pkg, oracle, matcher, S, TH, "257")
    assert S["nP"] == 257 and bi[0][256] >= 0 and bi[1][256] >= 0


def test_first_block_without_a_live_lane(pkg, oracle, matcher):
    """No point of block 0 is valid for target 1: the gate kernel writes -1 / 256 for all of its lanes and lists nothing, the list of target 1
    starts with points of block 1, and its last search block is empty; target 0 searches in all."""
    S = SS.subset(SS.scene(), [0, 1], np.arange(SS.NP))
    S["valid"][1][:256] = 0
    total, bi, bd, nf = check(pkg, oracle, matcher, S, TH, "dead-first-block")
    assert np.all(bi[1][:256] == -1) and np.all(bd[1][:256] == 256) and (bi[1][256:512] >= 0).sum() >= 20 and (bi[1][512:] >= 0).sum() >= 5
    assert (bi[0][:256] >= 0).sum() >= 20


def test_a_target_without_a_live_pair(pkg, oracle, matcher):
    """Target 0 looks the other way (rows 0 and 2 of Scw negated: a half turn about y): its points are valid, every pair dies in the gate
    kernel, its list stays empty and every search block of the target leaves at once; target 1 beside it is searched as usual."""
    S = SS.subset(SS.scene(), [0, 3], np.arange(SS.NP))
    S["targets"] = [dict(tg) for tg in S["targets"]]
    Scw = S["targets"][0]["Scw"].copy()
    Scw[0] *= -1.0
    Scw[2] *= -1.0
    S["targets"][0]["Scw"] = Scw
    S["valid"][0][S["group"] == SS.GROUPS.index("behind")] = 0   # the mirrored points would be the ones in front of it
    assert S["valid"][0].sum() >= 500
    total, bi, bd, nf = check(pkg, oracle, matcher, S, TH, "no-live-pair")
    assert nf[0] == 0 and np.all(bi[0] == -1) and np.all(bd[0] == 256) and nf[1] >= 100
    n, pi, pd = SS.product_row(pkg, matcher, S, 0, TH)
    assert n == 0 and np.array_equal(pi, bi[0]) and np.array_equal(pd, bd[0])


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_keypoint_counts_around_the_chunk(pkg, oracle, matcher, n):
    S = SS.truncated(SS.scene(), SS.DUP, n)
    total, bi, bd, nf = check(pkg, oracle, matcher, S, TH, ("cut", n))
    assert total >= 20 and bi.max() < n
    pn, pi, pd = SS.product_row(pkg, matcher, S, 0, TH)
    assert pn == total and np.array_equal(pi, bi[0]) and np.array_equal(pd, bd[0])


@pytest.mark.parametrize("what", ["zero", "nan", "inf"])
def test_a_scw_without_a_usable_scale_is_not_refused(pkg, matcher, what):
    """scw = 0, NaN or infinite: the per-target entry does not refuse it and neither does this one; T is then not finite, nothing passes
    IsInImage, and both give -1 / 256 (the kernel clamps PredictScale's level and the cell window: no table index depends on T)."""
    S = SS.subset(SS.scene(), [0, 2], np.arange(SS.NP))
    S["targets"] = [dict(tg) for tg in S["targets"]]
    for tg in S["targets"]:
        Scw = tg["Scw"].copy()
        if what == "zero":
            Scw[0, :3] = 0.0
        elif what == "nan":
            Scw[0, 1] = np.nan
        else:
            Scw[0, 0] = np.inf
        tg["Scw"] = Scw
    total, bi, bd, nf = one_call(pkg, matcher, S, TH)
    assert total == 0 and np.all(bi == -1) and np.all(bd == 256) and np.all(nf == 0)
    for t in range(2):
        n, pi, pd = SS.product_row(pkg, matcher, S, t, TH)
        assert n == 0 and np.array_equal(pi, bi[t]) and np.array_equal(pd, bd[t])


def test_more_parts_than_a_block_holds_inline(pkg, oracle, matcher):
    """T = 12 targets of 3 to 8 keypoints and nP = 5: 7 + 2 T + 4 = 35 parts, where a staged block holds 32 before it grows.  Targets 0
    and 1 take all five points in the full scene and their six copies keep those keypoints: 30 fused at least."""
    S0 = SS.scene()
    S = SS.many_small_targets(S0, oracle_rows(oracle, S0, TH, "full"))
    assert len(S["targets"]) == 12 and S["nP"] == 5 and all(3 <= len(tg["k"]) <= 8 for tg in S["targets"])
    total, bi, bd, nf = check(pkg, oracle, matcher, S, TH, "many small")
    assert total >= 30


def test_the_staged_block_grows_and_stays(pkg, oracle):
    m = pkg.ORBmatcher(0.8, False)                                # a fresh handle: nothing is allocated yet
    try:
        S0 = SS.scene()
        small = SS.subset(S0, [1, 2], np.arange(50))
        a = check(pkg, oracle, m, small, TH, "small")
        check(pkg, oracle, m, S0, TH, "full")
        b = check(pkg, oracle, m, small, TH, "small")
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    finally:
        m.close()


def test_two_handles_on_two_threads(pkg, oracle):
    S = SS.scene()
    want = oracle_rows(oracle, S, TH, "full")
    out, ms = {}, [pkg.ORBmatcher(0.8, False) for _ in range(2)]

    def work(j):
        try:
            out[j] = [one_call(pkg, ms[j], S, TH) for _ in range(3)]
        except Exception as e:                                     # reported by the assertion below
            out[j] = e

    try:
        ths = [threading.Thread(target=work, args=(j,)) for j in range(2)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    finally:
        for m in ms:
            m.close()
    for j in range(2):
        assert isinstance(out[j], list), out[j]
        for total, bi, bd, nf in out[j]:
            assert all(np.array_equal(bi[t], want[t][1]) and np.array_equal(bd[t], want[t][2]) and nf[t] == want[t][0] for t in range(T))


def test_refusals_name_the_target(pkg, matcher):
    S = SS.subset(SS.scene(), [0, 1, 2], np.arange(40))
    L = pkg.load()

    def call(structs, T_=None, nP=None, tab=True, valid=True):
        tabv = (pkg.FuseSim3TargetStruct * len(structs))(*structs)
        n = S["nP"] if nP is None else nP
        bi, bd, nf = np.full((len(structs), S["nP"]), -7, np.int32), np.full((len(structs), S["nP"]), -7, np.int32), np.full(len(structs), -7, np.int32)
        p = pkg._p
        rc = L.orbm_fuse_sim3_keyframes(matcher.m, len(structs) if T_ is None else T_, C.cast(tabv, C.c_void_p) if tab else None, n,
                                        p(S["valid"]) if valid else None, p(S["Xw"]), p(S["normal"]), p(S["mpdesc"]), p(S["max_dist"]), p(S["min_dist"]),
                                        C.c_float(TH), p(bi), p(bd), p(nf))
        return rc, L.orbm_last_error(matcher.m).decode(), bi, bd, nf

    views = [SS.product_target(pkg, tg) for tg in S["targets"]]
    good = lambda: [v.struct() for v in views]
    rc, _, bi, bd, nf = call(good())
    assert rc >= 0 and not np.any(bi == -7)
    rc, _, bi, bd, nf = call(good(), T_=0)                         # nothing to do: 0, the tables untouched
    assert rc == 0 and np.all(bi == -7)
    rc, _, bi, bd, nf = call(good(), nP=0)
    assert rc == 0 and np.all(bi == -7) and np.all(nf == 0)
    for kw in (dict(T_=-1), dict(nP=-1), dict(tab=False), dict(valid=False)):
        rc, err, bi, bd, nf = call(good(), **kw)
        assert rc == pkg.E_ARG and np.all(bi == -7) and np.all(bd == -7) and np.all(nf == -7) and not err.startswith("target "), (kw, err)
    big = np.zeros(15361, pkg.KP_DTYPE)
    bigd = np.zeros((15361, 32), np.uint8)
    bad_oct = S["targets"][1]["k"].copy()
    bad_oct["octave"][5] = 8
    neg_oct = S["targets"][1]["k"].copy()
    neg_oct["octave"][0] = -1

    def edit(s, **kw):
        for k, v in kw.items():
            setattr(s.kf if k in ("n", "keys_un", "descriptors", "min_x", "max_x", "min_y", "max_y") else s, k, v)

    cases = [(dict(n=-1), "n < 0"), (dict(n=15361, keys_un=pkg._p(big), descriptors=pkg._p(bigd)), "15360"), (dict(keys_un=None), "NULL"),
             (dict(descriptors=None), "NULL"), (dict(max_x=0.0), "bounds"), (dict(min_y=480.0), "bounds"), (dict(nlevels=0), "nlevels"),
             (dict(nlevels=17), "nlevels"), (dict(keys_un=pkg._p(bad_oct)), "octave"), (dict(keys_un=pkg._p(neg_oct)), "octave"),
             (dict(cam_type=2), "cam_type"), (dict(cam_type=-1), "cam_type"), (dict(scale_factors=None), "NULL"), (dict(Scw=None), "NULL"),
             (dict(cam_params=None), "NULL")]
    for kw, word in cases:
        st = good()
        edit(st[1], **kw)
        rc, err, bi, bd, nf = call(st)
        assert rc == pkg.E_ARG and err.startswith("target 1: ") and word in err and np.all(bi == -7) and np.all(bd == -7) and np.all(nf == -7), (kw, err)


def test_search_and_fuse_rule_replay_on_the_device(pkg, oracle, matcher):
    """The sequential loop (per-target orbm_fuse_sim3_cam from the live state) against the rule (orbm_fuse_sim3_keyframes at loop entry,
    orbm_fuse_sim3_cam on the dirty subset): identical observation tables, bad flags, descriptors and nFused per target."""
    S, W, points, kfs = RM.replay_scene(oracle)
    search = lambda t, valid, desc: SS.product_row(pkg, matcher, S, t, RM.TH, valid=valid, mpdesc=desc)[1]
    nf_seq = RM.run_sequential(S, W, points, kfs, search)
    seq = W.state()
    S, W, points, kfs = RM.replay_scene(oracle)
    total, rows0, _, nf0 = one_call(pkg, matcher, S, RM.TH)
    log = {}
    nf_one = RM.run_one_call(S, W, points, kfs, rows0, search, log)
    assert nf_one == nf_seq and W.state() == seq
    assert W.replaced_kf >= 30 and len(log["dirty"]) >= 5
    h = S["hand"]
    assert (RM.HAND_LATER, h["point"]) in log["changed"] and rows0[RM.HAND_LATER][h["point"]] == h["m1"]
