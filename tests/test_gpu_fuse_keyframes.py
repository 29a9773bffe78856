"""GPU: ORBmatcher::Fuse of one point list into all target keyframes in one call (orbm_fuse_keyframes, k_fuse_keyframes;
LocalMapping::SearchInNeighbors, LocalMapping.cc:909-1058).  Every comparison is on integers and exact.

  * Every row of the one-call entry equals the reference's search (oracle.fuse) for that target AND the per-target entry orbm_fuse that
    it replaces - best_idx, best_dist, nfused - on the scene of tests/fuse_keyframes_scene.py, at th 3.0 and 8.0.
  * nP = 1 / T = 1; a small call, the full one and the small one again on one handle (the staged block grows and stays); two handles on
    two host threads; what the entry refuses, with the target named.
  * The FUSE RULE of include/orbhip.h replayed with the rows and the subset searches taken from the device (tests/fuse_rule_model.py)."""
import ctypes as C
import threading

import numpy as np
import pytest

import fuse_keyframes_scene as FS
import fuse_rule_model as RM

pytestmark = pytest.mark.gpu
T = len(FS.TARGETS)


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.ORBmatcher(0.6, False)
    yield m
    m.close()


_rows = {}


def oracle_rows(oracle, S, th, key):
    """The reference's rows of scene S, computed once per (scene key, th) and left unchanged."""
    if (key, th) not in _rows:
        _rows[(key, th)] = [FS.oracle_row(oracle, S, t, th) for t in range(len(S["targets"]))]
    return _rows[(key, th)]


def one_call(pkg, m, S, th):
    return m.FuseKeyFrames([FS.product_target(pkg, tg) for tg in S["targets"]], S["valid"], S["Xw"], S["normal"], S["mpdesc"], S["max_dist"],
                           S["min_dist"], th)


def check(pkg, oracle, m, S, th, key):
    total, bi, bd, nf = one_call(pkg, m, S, th)
    want = oracle_rows(oracle, S, th, key)
    assert bi.shape == bd.shape == (len(S["targets"]), S["nP"])
    for t, (n, wi, wd) in enumerate(want):
        assert np.array_equal(bi[t], wi) and np.array_equal(bd[t], wd) and nf[t] == n, t
    assert total == sum(n for n, _, _ in want)
    return total, bi, bd, nf


@pytest.mark.parametrize("th", [3.0, 8.0])
def test_rows_equal_the_reference_and_the_per_target_entry(pkg, oracle, matcher, th):
    S = FS.scene()
    total, bi, bd, nf = check(pkg, oracle, matcher, S, th, "full")
    assert all(nf[t] >= 30 for t in FS.REAL) and nf[4] == 0 and nf[5] == 0
    assert np.all(bi[4] == -1) and np.all(bd[4] == 256) and np.all(bi[5] == -1) and np.all(bd[5] == 256)
    for t in range(T):
        n, pi, pd = FS.product_row(pkg, matcher, S, t, th)
        assert n == nf[t] and np.array_equal(pi, bi[t]) and np.array_equal(pd, bd[t]), t
    tg = S["targets"][FS.DUP]                                     # the walk order decided, against the index and the chunk
    assert sum(1 for i, b in tg["dupB"].items() if bi[FS.DUP][i] == b and b >= 2 * FS.CHUNK > tg["dupA"][i]) >= 3


def test_one_point_one_target(pkg, oracle, matcher):
    S0 = FS.scene()
    hit = int(np.nonzero(FS.oracle_row(oracle, S0, 0, 3.0)[1] >= 0)[0][0])
    for i in (hit, int(np.nonzero(S0["group"] == FS.GROUPS.index("behind"))[0][0])):
        S = FS.subset(S0, [0], [i])
        total, bi, bd, nf = check(pkg, oracle, matcher, S, 3.0, ("one", i))
        assert total == (1 if i == hit else 0)


def test_more_parts_than_a_block_holds_inline(pkg, oracle, matcher):
    """T = 12 targets of 3 to 8 keypoints, each with mvuRight, and nP = 5: 7 + 3 T + 2 = 45 parts, where a staged block holds 32 before
    it grows.  Targets 0 and 1 take all five points in the full scene and their six copies keep those keypoints: 30 fused at least."""
    S0 = FS.scene()
    S = FS.many_small_targets(S0, oracle_rows(oracle, S0, 3.0, "full"), all_ur=True)
    assert len(S["targets"]) == 12 and S["nP"] == 5 and all(3 <= len(tg["k"]) <= 8 and tg["ur"] is not None for tg in S["targets"])
    total, bi, bd, nf = check(pkg, oracle, matcher, S, 3.0, "many small")
    assert total >= 30


def test_the_staged_block_grows_and_stays(pkg, oracle):
    m = pkg.ORBmatcher(0.6, False)                                # a fresh handle: nothing is allocated yet
    try:
        S0 = FS.scene()
        small = FS.subset(S0, [1, 2], np.arange(50))
        a = check(pkg, oracle, m, small, 3.0, "small")
        check(pkg, oracle, m, S0, 3.0, "full")
        b = check(pkg, oracle, m, small, 3.0, "small")
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    finally:
        m.close()


def test_two_handles_on_two_threads(pkg, oracle):
    S = FS.scene()
    want = oracle_rows(oracle, S, 3.0, "full")
    out, ms = {}, [pkg.ORBmatcher(0.6, False) for _ in range(2)]

    def work(j):
        try:
            out[j] = [one_call(pkg, ms[j], S, 3.0) for _ in range(3)]
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
    S = FS.subset(FS.scene(), [0, 1, 2], np.arange(40))
    L = pkg.load()

    def call(structs, T_=None, nP=None, tab=True, valid=True):
        tabv = (pkg.FuseTargetStruct * len(structs))(*structs)
        n = S["nP"] if nP is None else nP
        bi, bd, nf = np.full((len(structs), S["nP"]), 7, np.int32), np.full((len(structs), S["nP"]), 7, np.int32), np.full(len(structs), 7, np.int32)
        p = pkg._p
        rc = L.orbm_fuse_keyframes(matcher.m, len(structs) if T_ is None else T_, C.cast(tabv, C.c_void_p) if tab else None, n,
                                   p(S["valid"]) if valid else None, p(S["Xw"]), p(S["normal"]), p(S["mpdesc"]), p(S["max_dist"]), p(S["min_dist"]),
                                   C.c_float(3.0), p(bi), p(bd), p(nf))
        return rc, L.orbm_last_error(matcher.m).decode(), bi, nf

    views = [FS.product_target(pkg, tg) for tg in S["targets"]]
    good = lambda: [v.struct() for v in views]
    rc, _, bi, nf = call(good())
    assert rc >= 0 and not np.any(bi == 7)
    rc, _, bi, nf = call(good(), T_=0)                             # nothing to do: 0, the tables untouched
    assert rc == 0 and np.all(bi == 7)
    rc, _, bi, nf = call(good(), nP=0)
    assert rc == 0 and np.all(bi == 7) and np.all(nf == 0)
    for kw in (dict(T_=-1), dict(nP=-1), dict(tab=False), dict(valid=False)):
        rc, err, bi, nf = call(good(), **kw)
        assert rc == pkg.E_ARG and np.all(bi == 7) and not err.startswith("target "), (kw, err)
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
             (dict(cam_type=2), "cam_type"), (dict(cam_type=-1), "cam_type"), (dict(scale_factors=None), "NULL"), (dict(inv_level_sigma2=None), "NULL"),
             (dict(Tcw=None), "NULL"), (dict(Ow=None), "NULL"), (dict(cam_params=None), "NULL")]
    for kw, word in cases:
        st = good()
        edit(st[1], **kw)
        rc, err, bi, nf = call(st)
        assert rc == pkg.E_ARG and err.startswith("target 1: ") and word in err and np.all(bi == 7), (kw, err)


def test_fuse_rule_replay_on_the_device(pkg, oracle, matcher):
    """The sequential loop (per-target orbm_fuse from the live state) against the rule (orbm_fuse_keyframes at loop entry, orbm_fuse on the
    dirty subset): identical observation tables, bad flags, descriptors and nFused per target."""
    S, W, points, kf_of = RM.replay_scene(oracle)
    search = lambda t, valid, desc: FS.product_row(pkg, matcher, S, t, 3.0, valid=valid, mpdesc=desc)[1]
    nf_seq = RM.run_sequential(S, W, points, kf_of, search)
    seq = W.state()
    S, W, points, kf_of = RM.replay_scene(oracle)
    total, rows0, _, nf0 = one_call(pkg, matcher, S, 3.0)
    log = {}
    nf_one = RM.run_one_call(S, W, points, kf_of, rows0, search, log)
    assert nf_one == nf_seq and W.state() == seq
    assert W.replaced_searched >= 10 and W.replaced_kf >= 10 and len(log["dirty"]) >= 5
    h = S["hand"]
    assert (RM.HAND_LATER, h["point"]) in log["changed"] and rows0[RM.HAND_LATER][h["point"]] == h["m1"]
