"""GPU: SearchByBoW of one frame or keyframe against all candidates in one call (orbm_search_by_bow_candidates: the loop of
Tracking::Relocalization, Tracking.cc:3796-3816; orbm_search_by_bow_keyframes_candidates: the loop of
LoopClosing::DetectCommonRegionsFromBoW, LoopClosing.cc:724-739).

Expected values: the oracle's per-pair member, looped (independent of the product's source); every row must also equal the per-pair
device entry it replaces, called on the same handle.  The results are keypoint indices and counts, so every comparison is exact.  The
scene is built once per process and shared (tests/bow_candidates_scene.py); tests/test_bow_candidates_abi.py shows on the oracle alone
that it reaches what is claimed here: rows of 40 and more matches next to empty ones and one below 15, partners at positions 63, 64 and
129 of the second operand's nodes, twins that need the `taken` bits, matches the rotation histogram removes."""
import ctypes as C

import numpy as np
import pytest

import bow_candidates_scene as BS

pytestmark = pytest.mark.gpu
K = len(BS.KINDS)


def views_of(pkg, S, what, fisheye=False, which=None):
    which = range(K) if which is None else which
    return BS.product_fixed(pkg, S, what, fisheye), [BS.product_cand(pkg, S, j, what) for j in which]


def one_call(m, what, fixed, views, n_left=None, skip=None):
    if what == "kf":
        return m.SearchByBoWKeyFramesCandidates(fixed, views, skip=skip)
    return m.SearchByBoWCandidates(views, fixed, n_left=n_left, skip=skip)


def per_pair(m, what, fixed, view, n_left=None):
    return m.SearchByBoWKeyFrames(fixed, view) if what == "kf" else m.SearchByBoW(view, fixed, n_left=n_left)


@pytest.fixture(params=["frame", "kf"])
def what(request):
    return request.param


@pytest.mark.parametrize("nodes", [6, 64])
@pytest.mark.parametrize("check_ori", [False, True])
def test_rows_equal_oracle_loop_and_per_pair_entry(pkg, oracle, what, check_ori, nodes):
    S = BS.scene(nodes)
    fixed, views = views_of(pkg, S, what)
    want_n, want = BS.oracle_rows(oracle, S, what, check_ori=check_ori)
    m = pkg.ORBmatcher(BS.NNRATIO[what], check_ori)
    try:
        nm, rows = one_call(m, what, fixed, views)
        assert rows.shape == (K, fixed.N) and rows.dtype == np.int32 and nm.shape == (K,)
        assert np.array_equal(rows, want) and np.array_equal(nm, want_n)
        for j in range(K):
            n_dev, row_dev = per_pair(m, what, fixed, views[j])
            assert np.array_equal(rows[j], row_dev) and nm[j] == n_dev, j
        assert nm[0] >= 40 and nm[2] >= 40 and 1 <= nm[5] <= 14 and nm[1] == nm[3] == nm[4] == 0
    finally:
        m.close()


@pytest.mark.parametrize("nodes", [6, 64])
def test_fisheye_frame_equals_oracle_and_per_pair_entry(pkg, oracle, nodes):
    S = BS.scene(nodes)
    fixed, views = views_of(pkg, S, "frame", fisheye=True)
    n_left = len(S["base"]["k"])
    want_n, want = BS.oracle_rows(oracle, S, "frame", check_ori=True, fisheye=True)
    m = pkg.ORBmatcher(BS.NNRATIO["frame"], True)
    try:
        nm, rows = one_call(m, "frame", fixed, views, n_left=n_left)
        assert np.array_equal(rows, want) and np.array_equal(nm, want_n)
        for j in range(K):
            n_dev, row_dev = per_pair(m, "frame", fixed, views[j], n_left=n_left)
            assert np.array_equal(rows[j], row_dev) and nm[j] == n_dev, j
        assert (rows[0][n_left:] >= 0).sum() >= 10 and (rows[2][n_left:] >= 0).sum() >= 10
    finally:
        m.close()


def test_skip_and_empty_calls(pkg, oracle, what):
    S = BS.scene()
    fixed, views = views_of(pkg, S, what)
    want_n, want = BS.oracle_rows(oracle, S, what)
    m = pkg.ORBmatcher(BS.NNRATIO[what], True)
    try:
        skip = np.array([0, 0, 1, 0, 0, 0], np.uint8)                  # a "real" candidate is bad
        nm, rows = one_call(m, what, fixed, views, skip=skip)
        assert np.all(rows[2] == -1) and nm[2] == 0
        keep = skip == 0
        assert np.array_equal(rows[keep], want[keep]) and np.array_equal(nm[keep], want_n[keep])
        nm, rows = one_call(m, what, fixed, [])                         # K == 0
        assert nm.shape == (0,) and rows.shape == (0, fixed.N)
        nm, rows = one_call(m, what, fixed, views, skip=np.ones(K, np.uint8))
        assert np.all(rows == -1) and np.all(nm == 0)
        # a skipped candidate is not validated: a table entry of NULL pointers and a negative count goes through
        tab = (pkg.KeyFrameStruct * K)(*[v.struct() for v in views])
        tab[2] = pkg.KeyFrameStruct(-5, None, None, None, None, -1, None, None, None, None, None, 0)
        out, cnt = np.full(K * fixed.N, 7, np.int32), np.full(K, 7, np.int32)
        rc = raw(pkg, m, what, fixed.struct(), tab, K, out, cnt, skip=skip)
        assert rc == int(want_n[keep].sum()) and np.array_equal(out.reshape(K, -1)[keep], want[keep]) and np.all(out.reshape(K, -1)[2] == -1)
        # an empty fixed operand: 0, the counts written
        empty = pkg.KeyFrameView(S["base"]["k"][:0], S["base"]["d"][:0], {}, S["sf"], S["sigma2"])
        cnt = np.full(K, 7, np.int32)
        rc = raw(pkg, m, what, empty.struct(), (pkg.KeyFrameStruct * K)(*[v.struct() for v in views]), K, np.zeros(1, np.int32), cnt)
        assert rc == 0 and np.all(cnt == 0)
    finally:
        m.close()


def raw(pkg, m, what, fixed_struct, tab, k, rows, nm, skip=None, n_left=-1):
    """The C entry itself, on caller-owned outputs."""
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    L = pkg.load()
    if what == "kf":
        return L.orbm_search_by_bow_keyframes_candidates(m.m, C.byref(fixed_struct), k, C.cast(tab, C.c_void_p), p(skip), C.c_float(m.mfNNratio),
                                                         int(m.mbCheckOrientation), p(rows), p(nm))
    return L.orbm_search_by_bow_candidates(m.m, k, C.cast(tab, C.c_void_p), C.byref(fixed_struct), n_left, p(skip), C.c_float(m.mfNNratio),
                                           int(m.mbCheckOrientation), p(rows), p(nm))


def last_error(pkg, m):
    return pkg.load().orbm_last_error(m.m).decode()


def big_node_view(pkg, S, key, members, partners_from):
    """A keyframe of `members` keypoints, all in vocabulary node `key`; its last keypoints are copies of the base keypoints
    `partners_from` (with map points), the others random."""
    rng = np.random.default_rng(members)
    d = rng.integers(0, 256, (members, 32), dtype=np.uint8)
    k = np.zeros(members, BS.SC.KP_DTYPE)
    k["angle"] = rng.uniform(0, 360, members)
    src = list(partners_from)
    d[members - len(src):] = S["base"]["d"][src]
    k["angle"][members - len(src):] = S["base"]["k"]["angle"][src]
    return k, d, {key: list(range(members))}


@pytest.mark.parametrize("members", [2048, 2049])
def test_a_node_of_2048_second_operand_members_is_the_limit(pkg, oracle, what, members):
    """2049 members: ORBX_E_ARG naming candidate 3, nothing written.  2048: accepted, equal to the oracle, the partners (the node's last
    members, in its 32nd trip) matched."""
    S = BS.scene()
    key = sorted(k for k in S["base"]["fv"] if k not in (3, 10, 17))[0]          # a node of the base outside the wide ones
    in_node = S["base"]["fv"][key]
    partners = [i for i in in_node if S["base"]["mpW"][i]][:8]
    k, d, fv = big_node_view(pkg, S, key, members, partners)
    mp = np.ones(members, np.uint8)
    big = pkg.KeyFrameView(k, d, fv, S["sf"], S["sigma2"], has_mappoint=mp)
    obig = oracle.OracleKeyFrame(k, d, fv, S["sf"], S["sigma2"], has_mp=mp)
    m = pkg.ORBmatcher(BS.NNRATIO[what], True)
    try:
        if what == "kf":     # the big keyframe is the second operand of pair 3
            fixed, views = views_of(pkg, S, what)
            views[3] = big
            skip = None
            want_n, want = oracle.search_by_bow_keyframes(BS.oracle_fixed(oracle, S, what), obig, BS.NNRATIO[what], True)
        else:                # the big frame is the second operand of every pair: candidates 0..2 are bad, 3 is the first one searched
            fixed = big
            views = [BS.product_cand(pkg, S, j, what) for j in (0, 1, 2, 2, 4, 5)]
            skip = np.array([1, 1, 1, 0, 0, 0], np.uint8)
            want_n, want = oracle.search_by_bow(BS.oracle_cand(oracle, S, 2, what), obig, BS.NNRATIO[what], True)
        tab = (pkg.KeyFrameStruct * K)(*[v.struct() for v in views])
        rows, nm = np.full(K * fixed.N, 7, np.int32), np.full(K, 7, np.int32)
        rc = raw(pkg, m, what, fixed.struct(), tab, K, rows, nm, skip=skip)
        if members == 2049:
            assert rc == pkg.E_ARG and last_error(pkg, m).startswith("candidate 3:"), last_error(pkg, m)
            assert np.all(rows == 7) and np.all(nm == 7)
        else:
            assert rc >= 0 and nm[3] == want_n and np.array_equal(rows.reshape(K, -1)[3], want)
            assert want_n >= 3
    finally:
        m.close()


def test_a_member_index_outside_the_keyframe_is_refused(pkg, what):
    S = BS.scene()
    fixed, views = views_of(pkg, S, what)
    m = pkg.ORBmatcher(BS.NNRATIO[what], True)
    try:
        for j in (0, 2):
            assert S["base"]["fv"].keys() & S["cands"][j]["fv"].keys() >= {min(S["cands"][j]["fv"])}      # node_idx[0] lies in a shared node
            bad = BS.product_cand(pkg, S, j, what)
            for value in (bad.N, -1):
                bad.node_idx[0] = value
                tab = (pkg.KeyFrameStruct * K)(*[(bad if i == j else v).struct() for i, v in enumerate(views)])
                rows, nm = np.full(K * fixed.N, 7, np.int32), np.full(K, 7, np.int32)
                rc = raw(pkg, m, what, fixed.struct(), tab, K, rows, nm)
                assert rc == pkg.E_ARG and last_error(pkg, m).startswith("candidate %d:" % j), last_error(pkg, m)
                assert np.all(rows == 7) and np.all(nm == 7)
        # a node_start that decreases
        bad = BS.product_cand(pkg, S, 2, what)
        bad.node_start[1] = bad.node_start[2] + 1
        tab = (pkg.KeyFrameStruct * K)(*[(bad if i == 2 else v).struct() for i, v in enumerate(views)])
        rows, nm = np.full(K * fixed.N, 7, np.int32), np.full(K, 7, np.int32)
        assert raw(pkg, m, what, fixed.struct(), tab, K, rows, nm) == pkg.E_ARG and last_error(pkg, m).startswith("candidate 2:")
        assert np.all(rows == 7) and np.all(nm == 7)
        # K < 0, NULL tables, n_left_f outside [-1, f->n]
        tab = (pkg.KeyFrameStruct * K)(*[v.struct() for v in views])
        assert raw(pkg, m, what, fixed.struct(), tab, -1, rows, nm) == pkg.E_ARG
        assert raw(pkg, m, what, fixed.struct(), tab, K, None, nm) == pkg.E_ARG and raw(pkg, m, what, fixed.struct(), tab, K, rows, None) == pkg.E_ARG
        if what == "frame":
            assert raw(pkg, m, what, fixed.struct(), tab, K, rows, nm, n_left=fixed.N + 1) == pkg.E_ARG
            assert raw(pkg, m, what, fixed.struct(), tab, K, rows, nm, n_left=-2) == pkg.E_ARG
        assert np.all(rows == 7) and np.all(nm == 7)
    finally:
        m.close()


def test_handle_reuse_with_fewer_and_more_candidates(pkg, oracle, what):
    """K = 6, then a subset of two, then K = 6 again on one handle: stale staging, records or counts would show."""
    S = BS.scene(64)
    fixed, views = views_of(pkg, S, what)
    want_n, want = BS.oracle_rows(oracle, S, what)
    m = pkg.ORBmatcher(BS.NNRATIO[what], True)
    try:
        nm, rows = one_call(m, what, fixed, views)
        assert np.array_equal(rows, want) and np.array_equal(nm, want_n)
        nm2, rows2 = one_call(m, what, fixed, [views[2], views[0]])
        assert np.array_equal(rows2, rows[[2, 0]]) and np.array_equal(nm2, nm[[2, 0]])
        nm3, rows3 = one_call(m, what, fixed, views)
        assert np.array_equal(rows3, rows) and np.array_equal(nm3, nm)
    finally:
        m.close()


def test_per_pair_call_between_two_one_call_searches(pkg, oracle, what):
    """The per-pair entry shares the handle's staging block: its result stays the oracle's, and so does the next one-call search's."""
    S = BS.scene()
    fixed, views = views_of(pkg, S, what)
    want_n, want = BS.oracle_rows(oracle, S, what)
    m = pkg.ORBmatcher(BS.NNRATIO[what], True)
    try:
        nm, rows = one_call(m, what, fixed, views)
        n_dev, row_dev = per_pair(m, what, fixed, views[2])
        assert n_dev == want_n[2] and np.array_equal(row_dev, want[2])
        nm2, rows2 = one_call(m, what, fixed, views)
        for got_n, got in ((nm, rows), (nm2, rows2)):
            assert np.array_equal(got, want) and np.array_equal(got_n, want_n)
    finally:
        m.close()
