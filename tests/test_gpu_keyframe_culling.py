"""GPU: LocalMapping::KeyFrameCulling on the device (orbm_keyframe_culling, orbm_keyframe_culling_open / _step; k_cull_count, k_cull_walk;
LocalMapping.cc:1158-1310, KeyFrame.cc:670-677, MapPoint.cc:168-240).  Every comparison is exact: all outputs are integers.

  * The one-call form equals the literal model of tests/keyframe_culling_model.py on every scene of tests/keyframe_culling_scene.py:
    n_mps, n_red, culled, n_obs_out, bad_out.
  * The stepwise form, driven with the model's decisions and with "never applied", returns the model's passing keyframes in order with
    the model's counts; driven with the one-call form's own `culled` it gives the one-call form's counts.
  * A small call after a large one on one handle; open twice (an unfinished walk is discarded); another orbm_* call between steps.
  * What is refused leaves sentinel-filled outputs untouched; K = 0 returns 0; step without open is refused."""
import ctypes as C

import numpy as np
import pytest

import keyframe_culling_model as KM
import keyframe_culling_scene as KS

pytestmark = pytest.mark.gpu
NAMES = ("culled_to_kept", "kept_to_culled", "float_product", "erase_cases", "list_cases", "mono", "k1", "k2", "k8", "k101", "wide")
OUT = ("n_mps", "n_red", "culled", "n_obs", "bad")
_want = {}


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.ORBmatcher(0.8, False)
    yield m
    m.close()


def want(name, mode="erasable"):
    """The model's result on a scene, computed once per driving mode and left unchanged."""
    if (name, mode) not in _want:
        sc = KS.scenes()[name]
        _want[(name, mode)] = (KM.run(sc, sc["erasable"]) if mode == "erasable" else
                               KM.run(sc, applied=(lambda k: True) if mode == "always" else (lambda k: False)))
    return _want[(name, mode)]


def walk(m, sc, applied):
    """Steps through an open walk: applied(k) decides for each returned keyframe.  Returns (the keyframes returned, n_mps, n_red)."""
    K = len(sc["row_start"]) - 1
    m.KeyFrameCullingOpen(KS.arrays(sc))
    got, last, n_mps, n_red = [], False, None, None
    for _ in range(K + 1):
        k, n_mps, n_red = m.KeyFrameCullingStep(last)
        if k >= K:
            break
        got.append(k)
        last = applied(k)
    else:
        raise AssertionError("the walk did not end")
    return got, n_mps, n_red


def test_scenes_are_all_named():
    assert set(NAMES) == set(KS.scenes())


@pytest.mark.parametrize("name", NAMES)
def test_one_call_equals_the_model(pkg, matcher, name):
    sc = KS.scenes()[name]
    got = matcher.KeyFrameCulling(KS.arrays(sc), sc["erasable"])
    w = want(name)
    for g, key in zip(got, OUT):
        diff = np.nonzero(g != w[key])[0]
        assert diff.size == 0, (key, diff[:10], g[diff[:10]], w[key][diff[:10]])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", ["always", "never"])
def test_stepwise_equals_the_model(pkg, matcher, name, mode):
    sc = KS.scenes()[name]
    w = want(name, mode)
    got, n_mps, n_red = walk(matcher, sc, (lambda k: True) if mode == "always" else (lambda k: False))
    assert got == w["passing"]
    assert np.array_equal(n_mps, w["n_mps"]) and np.array_equal(n_red, w["n_red"])


@pytest.mark.parametrize("name", ["erase_cases", "k101"])
def test_stepwise_equals_one_call(pkg, matcher, name):
    sc = KS.scenes()[name]
    n_mps, n_red, culled, _, _ = matcher.KeyFrameCulling(KS.arrays(sc), sc["erasable"])
    assert 0 < culled.sum() < len(want(name)["passing"])                     # a passing keyframe that is not erasable is among them
    got, s_mps, s_red = walk(matcher, sc, lambda k: bool(culled[k]))
    assert got == want(name)["passing"] and np.array_equal(s_mps, n_mps) and np.array_equal(s_red, n_red)


def test_step_writes_only_the_keyframes_it_walked(pkg, matcher):
    sc = KS.scenes()["erase_cases"]
    w = want("erase_cases")                                                  # keyframe 3 passes and is not erased
    assert w["passing"] == [0, 3, 4] and list(np.nonzero(w["culled"])[0]) == [0, 4]
    matcher.KeyFrameCullingOpen(KS.arrays(sc))
    k, n_mps, n_red = matcher.KeyFrameCullingStep(False)
    assert k == 0 and n_mps[0] == w["n_mps"][0] and np.all(n_mps[1:] == -1) and np.all(n_red[1:] == -1)
    k, n_mps, n_red = matcher.KeyFrameCullingStep(True)
    assert k == 3 and np.array_equal(n_mps[:4], w["n_mps"][:4]) and n_mps[2] == 0 and np.all(n_mps[4:] == -1)
    k, n_mps, n_red = matcher.KeyFrameCullingStep(False)
    assert k == 4
    for _ in range(2):                                                       # the end, and a step behind the end
        k, n_mps, n_red = matcher.KeyFrameCullingStep(True)
        assert k == 6 and np.array_equal(n_mps, w["n_mps"]) and np.array_equal(n_red, w["n_red"])


def test_a_small_call_after_a_large_one(pkg):
    m = pkg.ORBmatcher(0.8, False)                                           # a fresh handle: the staged block grows, then is reused
    try:
        for name in ("mono", "k101", "culled_to_kept", "wide", "list_cases"):
            sc = KS.scenes()[name]
            got = m.KeyFrameCulling(KS.arrays(sc), sc["erasable"])
            assert all(np.array_equal(g, want(name)[key]) for g, key in zip(got, OUT)), name
            steps = walk(m, sc, lambda k: True)
            assert steps[0] == want(name, "always")["passing"] and np.array_equal(steps[1], want(name, "always")["n_mps"]), name
    finally:
        m.close()


def test_open_twice_discards_the_unfinished_walk(pkg, matcher):
    big, small = KS.scenes()["k101"], KS.scenes()["kept_to_culled"]
    matcher.KeyFrameCullingOpen(KS.arrays(big))
    k, _, _ = matcher.KeyFrameCullingStep(False)
    assert k == want("k101", "always")["passing"][0]
    got, n_mps, n_red = walk(matcher, small, lambda k: True)                 # opens again: the pending erase of `big` is dropped
    w = want("kept_to_culled", "always")
    assert got == w["passing"] == [0, 1] and np.array_equal(n_mps, w["n_mps"]) and np.array_equal(n_red, w["n_red"])
    got, n_mps, n_red = walk(matcher, big, lambda k: True)
    assert got == want("k101", "always")["passing"] and np.array_equal(n_red, want("k101", "always")["n_red"])


def test_other_calls_between_steps(pkg, matcher):
    """The walk's tables and state live in a buffer of their own: a one-call culling of another scene and a Hamming matrix, which both
    restage the handle's shared block, change nothing."""
    sc, other = KS.scenes()["k8"], KS.scenes()["wide"]
    w = want("k8", "always")
    assert len(w["passing"]) >= 3
    rng = np.random.RandomState(5)
    q = rng.randint(0, 256, (700, 32)).astype(np.uint8)
    matcher.KeyFrameCullingOpen(KS.arrays(sc))
    got, last = [], False
    while True:
        k, n_mps, n_red = matcher.KeyFrameCullingStep(last)
        if k >= 8:
            break
        got.append(k)
        last = True
        o = matcher.KeyFrameCulling(KS.arrays(other), other["erasable"])
        assert np.array_equal(o[2], want("wide")["culled"])
        d = np.zeros((700, 700), np.uint16)
        assert pkg.load().orbm_hamming_matrix(matcher.m, pkg._p(q), 700, pkg._p(q), 700, pkg._p(d)) == 0 and d[3, 3] == 0 and d.max() > 100
    assert got == w["passing"] and np.array_equal(n_mps, w["n_mps"]) and np.array_equal(n_red, w["n_red"])


def raw_call(pkg, m, A, erasable=None, drop_out=None, struct=True):
    c, keep = pkg.culling_struct(A)
    K, P = max(c.K, 1), max(c.P, 1)
    out = [np.full(K, -9, np.int32), np.full(K, -9, np.int32), np.full(K, 77, np.uint8), np.full(P, -9, np.int32), np.full(P, 77, np.uint8)]
    args = [pkg._p(o) for o in out]
    if drop_out is not None:
        args[drop_out] = None
    rc = pkg.load().orbm_keyframe_culling(m.m, C.byref(c) if struct else None, pkg._p(erasable), *args)
    return rc, out


def untouched(out):
    return all(np.all(o == (77 if o.dtype == np.uint8 else -9)) for o in out)


def test_refusals_leave_the_outputs_untouched(pkg, matcher):
    L = pkg.load()
    A = KS.arrays(KS.scenes()["erase_cases"])
    rc, out = raw_call(pkg, matcher, A)
    assert rc == 0 and not np.any(out[0] == -9) and not np.any(out[4] == 77)
    rc, out = raw_call(pkg, matcher, A, drop_out=3)                          # n_obs_out and bad_out may be NULL
    assert rc == 0 and np.all(out[3] == -9) and not np.any(out[4] == 77)
    empty = dict(A, row_start=np.zeros(1, np.int32))                         # K == 0
    rc, out = raw_call(pkg, matcher, empty)
    assert rc == 0 and untouched(out)

    def refused(B, word, **kw):
        rc, out = raw_call(pkg, matcher, B, **kw)
        assert rc == pkg.E_ARG and untouched(out), word
        assert word in L.orbm_last_error(matcher.m), (word, L.orbm_last_error(matcher.m))
        c, keep = pkg.culling_struct(B)
        assert L.orbm_keyframe_culling_open(matcher.m, C.byref(c)) == pkg.E_ARG, word

    def changed(key, at, value):
        B = dict(A, **{key: A[key].copy()})
        B[key][at] = value
        return B

    refused(changed("row_start", 0, 1), b"row_start[0]")
    refused(changed("obs_start", 0, 1), b"obs_start[0]")
    refused(changed("row_start", 2, A["row_start"][1] - 1), b"row_start decreases")
    refused(changed("obs_start", 5, A["obs_start"][4] - 1), b"obs_start decreases")
    refused(changed("row_point", 7, len(A["bad"])), b"row_point")
    refused(changed("row_point", 7, -2), b"row_point")
    refused(changed("obs_kf", 9, 6), b"obs_kf")
    refused(changed("obs_kf", 9, -2), b"obs_kf")
    refused(changed("obs_w", 3, 0), b"obs_w")
    refused(changed("obs_w", 3, 3), b"obs_w")
    e0 = A["obs_start"][KS.scenes()["erase_cases"]["named"]["no_entry_of_0"]]
    refused(changed("obs_kf", slice(e0, e0 + 2), 1), b"same obs_kf")         # two entries of one point for keyframe 1
    refused(dict(A, redundant_th=np.float32(np.nan)), b"NaN")
    many = dict(A, row_start=np.concatenate([A["row_start"], np.full(pkg.CULL_MAX_KEYFRAMES, A["row_start"][-1], np.int32)]))
    refused(many, b"ORBM_CULL_MAX_KEYFRAMES")
    wide = KS.arrays(KS.scenes()["wide"])
    grown = dict(wide, row_start=wide["row_start"] + np.array([0, 0, 1, 1], np.int32), row_point=np.append(wide["row_point"], -1).astype(np.int32),
                 row_level=np.append(wide["row_level"], 0).astype(np.int32), row_depth=np.append(wide["row_depth"], 1).astype(np.float32))
    refused(grown, b"15360")
    for key in ("skip", "th_depth", "row_start", "row_point", "row_level", "row_depth", "bad", "n_obs", "obs_start", "obs_kf", "obs_level", "obs_w"):
        if key in ("row_start", "obs_start"):                                # K / P come from these in culling_struct: set them by hand
            c, keep = pkg.culling_struct(A)
            setattr(c, key, None)
            out = [np.full(6, -9, np.int32), np.full(6, -9, np.int32), np.full(6, 77, np.uint8)]
            assert L.orbm_keyframe_culling(matcher.m, C.byref(c), None, *[pkg._p(o) for o in out], None, None) == pkg.E_ARG and untouched(out), key
        else:
            refused(dict(A, **{key: None}), b"NULL")
    for drop in range(3):
        rc, out = raw_call(pkg, matcher, A, drop_out=drop)
        assert rc == pkg.E_ARG and untouched(out), drop
    rc, out = raw_call(pkg, matcher, A, struct=False)
    assert rc == pkg.E_ARG and untouched(out)
    got = matcher.KeyFrameCulling(A, KS.scenes()["erase_cases"]["erasable"])   # and the handle still works
    assert np.array_equal(got[2], want("erase_cases")["culled"])


def test_step_without_open_is_refused(pkg):
    m = pkg.ORBmatcher(0.8, False)
    try:
        k, a, b = np.full(1, -9, np.int32), np.full(8, -9, np.int32), np.full(8, -9, np.int32)
        assert pkg.load().orbm_keyframe_culling_step(m.m, 0, pkg._p(k), pkg._p(a), pkg._p(b)) == pkg.E_ARG
        assert k[0] == -9 and np.all(a == -9) and np.all(b == -9) and b"without open" in pkg.load().orbm_last_error(m.m)
        empty = dict(KS.arrays(KS.scenes()["mono"]), row_start=np.zeros(1, np.int32))
        m.KeyFrameCullingOpen(empty)                                         # K == 0: open, and the first step is the end
        assert m.KeyFrameCullingStep(False)[0] == 0
        A = KS.arrays(KS.scenes()["mono"])
        m.KeyFrameCullingOpen(A)
        bad = dict(A, obs_w=np.zeros_like(A["obs_w"]))
        with pytest.raises(ValueError):
            m.KeyFrameCullingOpen(bad)                                       # a refused open changes nothing: the walk goes on
        assert m.KeyFrameCullingStep(False)[0] == want("mono", "never")["passing"][0]
    finally:
        m.close()
