"""CPU: Tracking::UpdateLocalMap and KeyFrame::UpdateConnections as csrc/orb_ref_localmap.h states them (orbm_update_local_map_host,
orbm_update_connections_host) against the literal model of tests/update_local_map_model.py, exactly: every output is an integer.

  * Both host forms equal the model on every scene of tests/local_map_scene.py, with the keyframes' addresses in slot order, reversed
    and shuffled.
  * What each hand-built scene is there for is asserted on the MODEL's trace alone, so that a scene cannot go quiet.
  * The CONNECTIONS RULE: on 200 seeded random scripts the sequential loop of UpdateConnections on live objects leaves every keyframe in
    the state that replaying the one-call rows (computed at loop entry) through the adapter helper's logic leaves it in.
  * Refusals leave sentinel-filled outputs untouched; capacities one short answer ORBX_E_CAP; N == 0 and T == 0 return 0.
  * The entries are declared, exported and listed."""
import ctypes as C
import os

import numpy as np
import pytest

import update_local_map_model as LM
import local_map_scene as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = ("identity", "reversed", 5)
KEYS = ("local_kf", "kf_max", "max_votes", "slot_bad", "local_point")
CKEYS = ("conn_kf", "conn_w", "ord_kf", "ord_w", "kf_max", "nmax")


def same(got, want, keys):
    return all(np.array_equal(got[k], want[k]) for k in keys)


def model(name, order="identity", **kw):
    S = LS.build(name, order)
    out, tr = LM.run_local_map(S["world"], S["frame_point"], S["inertial"], S["last_kf"], **kw)
    return S, out, tr


@pytest.mark.parametrize("name,order", [(n, o) for n in sorted(LS.CASES) for o in ORDERS] + [(n, "identity") for n in sorted(LS.SHAPES)])
def test_host_forms_equal_the_model(pkg, name, order):
    S = LS.build(name, order)
    A = LM.flatten(S["world"])
    rows = LM.connection_rows(S["world"], S["targets"])                   # before the local-map run: it writes only stamps, but keep the entry state
    got = pkg.update_local_map_host(A, S["frame_point"], S["inertial"], S["last_kf"])
    want, _ = LM.run_local_map(S["world"], S["frame_point"], S["inertial"], S["last_kf"])
    assert same(got, want, KEYS), {k: (got[k], want[k]) for k in KEYS if not np.array_equal(got[k], want[k])}
    got = pkg.update_connections_host(A, S["targets"])
    assert len(got) == len(rows) and all(same(g, w, CKEYS) for g, w in zip(got, rows))


def test_scene_tie_bad_holds_its_cases():
    S, out, tr = model("tie_bad")
    W = S["world"]
    assert tr["tie"] and out["kf_max"] == 1                                 # keyframes 1 and 2 tie; the lower address wins
    assert model("tie_bad", "reversed")[1]["kf_max"] == 2                   # ... so the other one wins when the addresses are reversed
    assert [k.slot for k in tr["voted_bad"]] == [3]
    fp = list(S["frame_point"])
    assert fp.count(0) == 2 and out["max_votes"] == 4                       # point 0 in two slots votes twice: 2 + 1 + 1
    assert tr["nulled"] == [4] and W.pts[5].bad and list(out["slot_bad"]) == [0, 0, 0, 0, 1, 0]
    last = int(out["local_kf"][-1])
    taken_last = {int(p) for p, j in zip(out["local_point"], tr["taken_at"]) if j == len(out["local_kf"]) - 1}
    elsewhere = {mp.idx for g in out["local_kf"][:-1] for mp in W.kfs[g].mvpMapPoints if mp}
    assert taken_last & elsewhere, (last, taken_last, elsewhere)            # first occurrence in the last-listed keyframe
    twice = [mp.idx for mp in W.kfs[1].mvpMapPoints if mp]
    assert twice.count(2) == 2 and list(out["local_point"]).count(2) == 1


def test_scenes_first_list_79_80_81_and_the_end_at_83():
    ends = {}
    for n in (79, 80, 81):
        S, out, tr = model("first%d" % n)
        assert tr["first"] == n
        ends[n] = len(out["local_kf"])
    assert ends == {79: 82, 80: 83, 81: 81}
    S, out, tr = model("first80")
    W = S["world"]
    (by, X, skipped), = tr["neighbour"]
    assert skipped == ("marked", "bad") and X.slot == 80                    # a marked and a bad neighbour in front of the taken one
    (by, child, skipped), = tr["child"]
    assert child.slot == 82 and "marked" in skipped                         # C1: the first good child in set order; C2 would do as well
    assert model("first80", "reversed")[2]["child"][0][1].slot == 83        # ... and is the one taken when the addresses are reversed
    (by, parent), = tr["parent"]
    assert parent.bad and parent.slot == 85 and int(out["local_kf"][-1]) == 85   # a bad parent is appended


def test_scene_parent_break_cuts_the_expansion():
    S, out, tr = model("parent_break")
    assert tr["parent_break_at"] == 0
    S2, out2, tr2 = model("parent_break", no_parent_break=True)
    assert len(out2["local_kf"]) > len(out["local_kf"]) and list(out2["local_kf"][:len(out["local_kf"])]) == list(out["local_kf"])


def test_scenes_tail_stops():
    S, out, tr = model("tail_marked")
    assert [k.slot for k in tr["tail"]] == [7, 6, 5] and tr["tail_stop"] == "marked"
    S, out, tr = model("tail_end")
    assert [k.slot for k in tr["tail"]] == [7, 6, 5] and tr["tail_stop"] == "null"


def test_scene_connections_holds_its_cases():
    S = LS.build("connections")
    W = S["world"]
    rows = dict(zip(S["targets"], LM.connection_rows(W, S["targets"])))
    r0 = rows[0]
    assert dict(zip(r0["conn_kf"], r0["conn_w"])) == {1: 15, 2: 14, 3: 15}  # 14 and 15 around th; 4 (bad), 5 (other map) and 0 itself do not count
    assert all(W.kfs[g] in W.pts[0].obs for g in (0, 4, 5))
    assert list(r0["ord_kf"]) == [3, 1] and list(r0["ord_w"]) == [15, 15]   # equal weights: the higher address first
    rr = dict(zip(S["targets"], LM.connection_rows(LS.build("connections", "reversed")["world"], S["targets"])))
    assert list(rr[0]["ord_kf"]) == [1, 3]
    assert dict(zip(rows[1]["conn_kf"], rows[1]["conn_w"]))[0] == 14        # the rig point: 0 -> 1 weighs 15, 1 -> 0 weighs 14
    assert list(rows[6]["ord_kf"]) == [8] and list(rows[6]["ord_w"]) == [3] and rows[6]["conn_w"].max() < 15   # no pair at th: the fallback
    assert len(rows[7]["conn_kf"]) == 0 and rows[7]["kf_max"] == -1         # the empty counter


@pytest.mark.parametrize("order", ORDERS)
def test_scene_rows_holds_its_two_keyframes(order):
    S, out, tr = model("rows", order)
    A = LM.flatten(LS.build("rows", order)["world"])
    n = np.diff(A["kf_row_start"])
    local = list(out["local_kf"])
    assert n[5] == 0 and 5 in local and 5 in S["targets"] and not A["kf_bad"][5]          # a keyframe of 0 rows, listed and a target
    assert n[3] == 15360 and 3 in local and local.index(3) < len(local) - 1 and 3 in S["targets"]   # 15 360 rows, not walked first
    assert any(j == local.index(3) for j in tr["taken_at"])                               # and local points are taken from it
    assert min(np.diff(LM.flatten(LS.build(name)["world"])["kf_row_start"]).min() for name in LS.ALL) == 0


def test_one_target_with_a_counter(pkg):
    S = LS.build("connections")
    rows = LM.connection_rows(S["world"], S["targets"][:1])
    assert len(rows[0]["conn_kf"]) == 3 and len(rows[0]["ord_kf"]) == 2                   # T = 1 and the counter is not empty
    got = pkg.update_connections_host(LM.flatten(S["world"]), S["targets"][:1])
    assert len(got) == 1 and same(got[0], rows[0], CKEYS)


def script_world(seed):
    r = np.random.RandomState(seed)
    G, P = r.randint(3, 14), r.randint(20, 90)
    S = LS.random_world(1000 + seed, G, P, seed, obs=(1, min(G, 6)), frame_n=0)
    W = S["world"]
    for kf in W.kfs:                                                         # a consistent graph to start from: none
        kf.mvpOrderedConnectedKeyFrames, kf.mspChildrens, kf.mpParent = [], set(), None
    targets = [int(t) for t in r.permutation(G)[:r.randint(1, G + 1)]]
    return W, targets, int(r.choice([1, 2, 3, 15]))


def test_connections_rule_on_200_scripts(pkg):
    for seed in range(200):
        W, targets, th = script_world(seed)
        for t in targets:                                                    # the reference's loop
            LM.update_connections(W.kfs[t], W.init_kf_id, th)
        want = LM.connection_state(W)
        W2, targets2, _ = script_world(seed)
        rows = pkg.update_connections_host(LM.flatten(W2), targets2, th=th)  # all counted at loop entry
        assert all(same(g, w, CKEYS) for g, w in zip(rows, LM.connection_rows(W2, targets2, th)))
        for t, row in zip(targets2, rows):
            LM.apply_rows(W2, W2.kfs[t], row, th)
        assert LM.connection_state(W2) == want, seed


def raw_local_map(pkg, A, frame, inertial=0, last_kf=-1, cap_kf=200, cap_pts=400, struct=True, drop=None, host=True, m=None):
    g, keep = pkg.map_graph(A)
    fp = None if frame is None else np.ascontiguousarray(frame, np.int32)
    N = 0 if fp is None else len(fp)
    out = [np.full(max(cap_kf, 1), -9, np.int32), np.full(1, -9, np.int32), np.full(1, -9, np.int32), np.full(1, -9, np.int32), np.full(max(N, 1), 77, np.uint8),
           np.full(max(cap_pts, 1), -9, np.int32), np.full(1, -9, np.int32)]
    args = [pkg._p(o) for o in out]
    if drop is not None:
        args[drop] = None
    L = pkg.load()
    head = [C.byref(g) if struct else None, N, pkg._p(fp), inertial, last_kf, cap_kf, cap_pts]
    rc = L.orbm_update_local_map_host(*head, *args) if host else L.orbm_update_local_map(m.m, *head, *args)
    return rc, out


def untouched(out):
    return all(np.all(o == (77 if o.dtype == np.uint8 else -9)) for o in out)


def graph_refusals(A):
    """(changed tables, a word of the message) for everything the tables are refused for."""
    def changed(key, at, value):
        B = dict(A, **{key: np.array(A[key]).copy()})
        B[key][at] = value
        return B
    G = len(A["kf_rank"])
    yield changed("kf_row_start", 0, 1), b"kf_row_start[0]"
    yield changed("kf_child_start", 0, 1), b"kf_child_start[0]"
    yield changed("obs_start", 0, 1), b"obs_start[0]"
    yield changed("kf_row_start", 2, A["kf_row_start"][1] - 1), b"kf_row_start decreases"
    yield changed("kf_child_start", 2, -1), b"kf_child_start decreases"
    yield changed("obs_start", 3, A["obs_start"][2] - 1), b"obs_start decreases"
    yield changed("row_point", 1, len(A["pt_bad"])), b"row_point"
    yield changed("row_point", 1, -2), b"row_point"
    yield changed("kf_child", 0, G), b"kf_child"
    yield changed("kf_best", 3, G), b"kf_best"
    yield changed("kf_best", 3, -2), b"kf_best"
    yield changed("kf_parent", 0, G), b"kf_parent"
    yield changed("kf_prev", 0, -2), b"kf_prev"
    yield changed("kf_rank", 0, A["kf_rank"][1]), b"duplicate ranks"
    live = next(p for p in range(len(A["pt_bad"])) if not A["pt_bad"][p] and A["obs_start"][p + 1] - A["obs_start"][p] >= 2)
    e0 = A["obs_start"][live]
    yield changed("obs_kf", e0, A["obs_kf"][e0 + 1]), b"same keyframe"
    yield changed("obs_kf", e0, G), b"obs_kf"
    yield changed("obs_kf", e0, -1), b"obs_kf"
    many = dict(A)
    extra = 16384 + 1 - G
    for k in ("kf_rank", "kf_bad", "kf_map", "kf_parent", "kf_prev"):
        many[k] = np.concatenate([A[k], np.arange(10 ** 6, 10 ** 6 + extra).astype(A[k].dtype) if k == "kf_rank" else np.zeros(extra, A[k].dtype) - (k in ("kf_parent", "kf_prev"))])
    for k in ("kf_row_start", "kf_child_start"):
        many[k] = np.concatenate([A[k], np.full(extra, A[k][-1], np.int32)])
    many["kf_best"] = np.concatenate([A["kf_best"], np.full(10 * extra, -1, np.int32)])
    yield many, b"ORBM_MAP_MAX_KEYFRAMES"
    for key in ("kf_rank", "kf_bad", "kf_map", "row_point", "kf_best", "kf_child", "kf_parent", "pt_bad", "obs_kf"):
        yield dict(A, **{key: None}), b"NULL"


def test_refusals_leave_the_outputs_untouched(pkg):
    L = pkg.load()
    S = LS.build("random")
    A, frame = LM.flatten(S["world"]), S["frame_point"]
    rc, out = raw_local_map(pkg, A, frame)
    assert rc == 0 and not untouched(out) and out[1][0] > 0 and out[6][0] > 0
    need_kf, need_pts = int(out[1][0]), int(out[6][0])

    def refused(B, word, **kw):
        rc, out = raw_local_map(pkg, B, kw.pop("frame", frame), **kw)
        assert rc == pkg.E_ARG and untouched(out), word
        assert word in L.orbm_update_local_map_host_error(), (word, L.orbm_update_local_map_host_error())

    for B, word in graph_refusals(A):
        refused(B, word)
        g, keep = pkg.map_graph(B)
        tg = np.array(S["targets"], np.int32)
        o = [np.full(64, -9, np.int32) for _ in range(8)]
        assert L.orbm_update_connections_host(C.byref(g), len(tg), pkg._p(tg), 15, 16, *[pkg._p(x) for x in o]) == pkg.E_ARG and untouched(o), word
    refused(dict(A, kf_prev=None), b"kf_prev == NULL", inertial=1)
    rc, out = raw_local_map(pkg, dict(A, kf_prev=None), frame)               # kf_prev may be NULL when the call is not inertial
    assert rc == 0
    bad_frame = frame.copy()
    bad_frame[3] = len(A["pt_bad"])
    refused(A, b"frame_point", frame=bad_frame)
    refused(A, b"last_kf", last_kf=len(A["kf_rank"]))
    refused(A, b"negative", cap_kf=-1)
    refused(A, b"negative", cap_pts=-1)
    for drop in range(7):
        refused(A, b"NULL", drop=drop)
    rc, out = raw_local_map(pkg, A, frame, struct=False)
    assert rc == pkg.E_ARG and untouched(out)
    rc, out = raw_local_map(pkg, A, np.zeros(0, np.int32))                   # N == 0
    assert rc == 0 and out[1][0] == 0 and out[6][0] == 0 and out[2][0] == -1 and out[3][0] == 0 and np.all(out[0] == -9) and np.all(out[5] == -9)
    for kw in (dict(cap_kf=need_kf - 1), dict(cap_pts=need_pts - 1)):        # one short
        rc, out = raw_local_map(pkg, A, frame, **kw)
        assert rc == pkg.E_CAP and out[1][0] == need_kf and out[6][0] == need_pts and np.all(out[0] == -9) and np.all(out[5] == -9)
    rc, out = raw_local_map(pkg, A, frame, cap_kf=need_kf, cap_pts=need_pts)
    assert rc == 0


def raw_connections(pkg, A, targets, cap, th=15, drop=None):
    g, keep = pkg.map_graph(A)
    tg = np.ascontiguousarray(targets, np.int32)
    T = len(tg)
    out = [np.full(T + 1, -9, np.int32), np.full(max(cap, 1), -9, np.int32), np.full(max(cap, 1), -9, np.int32), np.full(T + 1, -9, np.int32),
           np.full(max(cap, 1), -9, np.int32), np.full(max(cap, 1), -9, np.int32), np.full(max(T, 1), -9, np.int32), np.full(max(T, 1), -9, np.int32)]
    args = [pkg._p(o) for o in out]
    if drop is not None:
        args[drop] = None
    return pkg.load().orbm_update_connections_host(C.byref(g), T, pkg._p(tg), th, cap, *args), out


def test_connections_refusals_and_capacity(pkg):
    L = pkg.load()
    S = LS.build("random_dense")
    A, targets = LM.flatten(S["world"]), S["targets"]
    rc, out = raw_connections(pkg, A, targets, 2000)
    assert rc == 0
    need = int(out[0][-1])
    assert need > 10
    rc, out = raw_connections(pkg, A, targets, need - 1)
    assert rc == pkg.E_CAP and out[0][-1] == need and np.all(out[1] == -9) and np.all(out[4] == -9) and not np.any(out[6] == -9)
    assert raw_connections(pkg, A, targets, need)[0] == 0
    for t2, word in ((targets[:2] + [targets[0]], b"listed twice"), ([len(A["kf_rank"])], b"target outside"), ([-1], b"target outside")):
        rc, out = raw_connections(pkg, A, t2, 2000)
        assert rc == pkg.E_ARG and untouched(out) and word in L.orbm_update_local_map_host_error()
    for drop in (0, 1, 3, 6, 7):
        rc, out = raw_connections(pkg, A, targets, 2000, drop=drop)
        assert rc == pkg.E_ARG and untouched(out)
    rc, out = raw_connections(pkg, A, targets, -1)
    assert rc == pkg.E_ARG and untouched(out)
    rc, out = raw_connections(pkg, A, [], 10)                                # T == 0
    assert rc == 0 and untouched(out)


def test_entries_declared_exported_listed(pkg):
    header = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    L = pkg.load()
    for name, nargs in (("orbm_update_local_map", 15), ("orbm_update_local_map_device", 16), ("orbm_update_local_map_host", 14),
                        ("orbm_update_connections", 14), ("orbm_update_connections_host", 13), ("orbm_gather_local_map_device", 17)):
        assert ("int %s(" % name) in header and name in pkg.ABI_SYMBOLS and len(getattr(L, name).argtypes) == nargs
    assert "const char *orbm_update_local_map_host_error(void);" in header and "orbm_update_local_map_host_error" in pkg.ABI_SYMBOLS
    for rule in ("RANK RULE", "STAMP NOTE", "CONNECTIONS RULE", "Tracking.cc:3658", "KeyFrame.cc:477"):
        assert rule in header
    assert C.sizeof(pkg.MapGraph) == 15 * 8 and pkg.MAP_MAX_KEYFRAMES == 16384
