"""GPU: MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth for all map points of one call (orbm_update_map_points,
k_update_map_points; MapPoint.cc:350-436, :467-547, LocalMapping.cc:1040-1053).  Every comparison is exact: integers, and float bits
(NaN masks where the arithmetic gives NaN).

  * The one call on the scene of tests/map_point_update_scene.py equals the numpy model of tests/map_point_update_model.py: best, normal,
    min_dist, max_dist - entry counts 0, 1, 2, 3, 63, 64, 65, 129, 1024, unflagged entries, twins, rig entries, a point in a camera centre
    and a subnormal tie.
  * best equals orbm_distinctive_descriptors on the flagged subsets.
  * The scene split into nmp = 1 calls gives the same rows; a small call after the large one on the same handle.
  * What is refused leaves sentinel-filled outputs untouched; nmp = 0 returns 0; the empty point's floats are untouched."""
import ctypes as C

import numpy as np
import pytest

import map_point_update_model as MM
import map_point_update_scene as MS

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-123.25)
KEYS = ("start", "desc", "centre", "in_desc", "pos", "ref_centre", "ref_scale", "ref_max_scale")
_want = []


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.ORBmatcher(0.8, False)
    yield m
    m.close()


def want(oracle):
    """The model's outputs over the scene, computed once and left unchanged."""
    if not _want:
        _want.append(MM.update(oracle, MS.scene(), SENTINEL))
    return _want[0]


def raw_call(pkg, m, A, nmp=None):
    n = next(len(A[k]) for k in ("pos", "ref_scale") if A[k] is not None)
    u = pkg.MapPointUpdateStruct(n if nmp is None else nmp, *[pkg._p(A[k]) if A[k] is not None else None for k in KEYS])
    out = (np.full(max(n, 1), -9, np.int32), np.full((max(n, 1), 3), SENTINEL), np.full(max(n, 1), SENTINEL), np.full(max(n, 1), SENTINEL))
    rc = pkg.load().orbm_update_map_points(m.m, C.byref(u), *[pkg._p(o) for o in out])
    return rc, out


def untouched(out):
    return np.all(out[0] == -9) and all(np.all(o == SENTINEL) for o in out[1:])


def test_the_scene_equals_the_model(pkg, oracle, matcher):
    pts = MS.scene()
    best, normal, mn, mx = matcher.UpdateMapPoints(pts, fill=SENTINEL)
    wb, wn, wmn, wmx = want(oracle)
    assert np.array_equal(best, wb)
    bad = [p for p in range(len(pts)) if not (MM.same_bits(normal[p], wn[p]) and MM.same_bits(mn[p], wmn[p]) and MM.same_bits(mx[p], wmx[p]))]
    assert not bad, (bad[:10], [len(pts[p]["desc"]) for p in bad[:10]])
    e, c, t = MS.NAMED["n0"], MS.NAMED["in_centre"], MS.NAMED["tiny_tie"]
    assert best[e] == -1 and np.all(normal[e] == SENTINEL) and mn[e] == SENTINEL and mx[e] == SENTINEL   # the empty point's floats are untouched
    assert np.all(np.isnan(normal[c])) and np.isfinite(mn[c]) and best[MS.NAMED["none_flagged"]] == -1
    assert normal[t, 2] == np.float32(2.0 ** -149)


def test_best_equals_the_descriptor_entry_on_the_flagged_subsets(pkg, oracle, matcher):
    pts = MS.scene()
    best = matcher.UpdateMapPoints(pts)[0]
    rows = [np.nonzero(pt["in_desc"])[0] for pt in pts]
    sub = matcher.ComputeDistinctiveDescriptors([pt["desc"][r] for pt, r in zip(pts, rows)])
    assert np.array_equal(best, [int(r[b]) if b >= 0 else -1 for r, b in zip(rows, sub)])


def test_one_point_per_call_gives_the_same_rows(pkg, oracle, matcher):
    pts = MS.scene()
    wb, wn, wmn, wmx = want(oracle)
    named = sorted(MS.NAMED.values())
    for p in named + [q for q in range(len(pts)) if q not in named][:40]:
        best, normal, mn, mx = matcher.UpdateMapPoints([pts[p]], fill=SENTINEL)
        assert best[0] == wb[p] and MM.same_bits(normal[0], wn[p]) and MM.same_bits(mn[0], wmn[p]) and MM.same_bits(mx[0], wmx[p]), p


def test_a_small_call_after_the_large_one(pkg, oracle):
    m = pkg.ORBmatcher(0.8, False)                                # a fresh handle: the staged block grows, then is reused
    try:
        pts = MS.scene()
        wb, wn, wmn, wmx = want(oracle)
        for sel in (slice(0, 5), slice(None), slice(0, 5), slice(100, 103)):
            best, normal, mn, mx = m.UpdateMapPoints(pts[sel], fill=SENTINEL)
            assert np.array_equal(best, wb[sel]) and MM.same_bits(normal, wn[sel]) and MM.same_bits(mn, wmn[sel]) and MM.same_bits(mx, wmx[sel])
    finally:
        m.close()


def test_a_point_listed_twice(pkg, oracle, matcher):
    pts = MS.scene()
    p = MS.NAMED["n65"]
    best, normal, mn, mx = matcher.UpdateMapPoints([pts[p], pts[3], pts[p]])
    assert best[0] == best[2] == want(oracle)[0][p] and MM.same_bits(normal[0], normal[2]) and mn[0] == mn[2] and mx[0] == mx[2]


def test_refusals_leave_the_outputs_untouched(pkg, matcher):
    pts = MS.scene()[:12]
    A = pkg.pack_map_points(pts)
    rc, out = raw_call(pkg, matcher, A)
    assert rc == 0 and not np.any(out[0] == -9)
    rc, out = raw_call(pkg, matcher, A, nmp=0)                    # nothing to do
    assert rc == 0 and untouched(out)
    rc, out = raw_call(pkg, matcher, A, nmp=-1)
    assert rc == pkg.E_ARG and untouched(out)
    B = dict(A, start=A["start"].copy())                          # a start that decreases
    B["start"][5] = B["start"][4] - 1
    rc, out = raw_call(pkg, matcher, B)
    assert rc == pkg.E_ARG and untouched(out) and b"start" in pkg.load().orbm_last_error(matcher.m)
    B = dict(A, start=A["start"].copy())                          # start[0] != 0
    B["start"][0] = 1
    rc, out = raw_call(pkg, matcher, B)
    assert rc == pkg.E_ARG and untouched(out)
    big = dict(MS.scene()[MS.NAMED["n1024"]])                     # 1025 entries of one point
    for k in ("desc", "centre", "in_desc"):
        big[k] = np.concatenate([big[k], big[k][:1]])
    rc, out = raw_call(pkg, matcher, pkg.pack_map_points(pts + [big]))
    assert rc == pkg.E_ARG and untouched(out) and b"1024" in pkg.load().orbm_last_error(matcher.m)
    for k in KEYS:                                                # a NULL array
        rc, out = raw_call(pkg, matcher, dict(A, **{k: None}))
        assert rc == pkg.E_ARG and untouched(out), k
    u = pkg.MapPointUpdateStruct(12, *[pkg._p(A[k]) for k in KEYS])
    for drop in range(4):                                         # a NULL output
        out = [np.full(12, -9, np.int32), np.full((12, 3), SENTINEL), np.full(12, SENTINEL), np.full(12, SENTINEL)]
        args = [pkg._p(o) for o in out]
        args[drop] = None
        assert pkg.load().orbm_update_map_points(matcher.m, C.byref(u), *args) == pkg.E_ARG and untouched(out), drop
    assert pkg.load().orbm_update_map_points(matcher.m, None, *[pkg._p(o) for o in out]) == pkg.E_ARG and untouched(out)
    best, normal, mn, mx = matcher.UpdateMapPoints(pts, fill=0.0)   # and the handle still works
    assert not np.any(np.isnan(mn)) and np.any(mx > 0)
