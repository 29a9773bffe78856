"""GPU: Tracking::UpdateLocalMap and KeyFrame::UpdateConnections on the device (orbm_update_local_map, orbm_update_local_map_device,
orbm_update_connections, orbm_gather_local_map_device; k_covis_vote, k_local_kf_walk, k_lp_first / _count / _write, k_conn_walk / _pack,
k_gather_local_map).  Every comparison is exact: all outputs are integers (the gathered floats are copies).

  * Every device form equals the literal model of tests/update_local_map_model.py on every scene of tests/local_map_scene.py, with the
    keyframes' addresses in slot order, reversed and shuffled.  The shape scenes cover N = 1, 63, 64, 65, 15 360; observation lists of 0, 1,
    63, 64, 65, 129 entries; G = 1, 2, 65, 16 384; T = 1, 2, 65; voted sets of 1, 64, 65, 1025; keyframes of 0 and 15 360 rows.
  * The device-table form equals the upload form; capacities one short: ORBX_E_CAP from the synchronous form, a count above the capacity
    and nothing written past it from the device form; N == 0.
  * T = 1 with a counter that is not empty; the measurement-only vote form (ORBM_VOTE_FORM=1) against the model.
  * A small call after a large one; two calls back to back (the per-point word is cleared between them); four host threads on one handle.
  * The chain UpdateLocalMapDevice -> GatherLocalMapDevice -> orbm_search_local_points_batch_device equals orbm_search_local_points on
    host-gathered arrays, slot for slot."""
import threading

import numpy as np
import pytest

import local_map_scene as LS
import update_local_map_model as LM
import test_local_map_abi as TA

pytestmark = pytest.mark.gpu
ORDERS = ("identity", "reversed", 5)
KEYS, CKEYS = TA.KEYS, TA.CKEYS
_want = {}


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.ORBmatcher(0.8, False)
    yield m
    m.close()


def want(name, order="identity"):
    """(tables, scene, the model's local map, the model's connection rows), computed once per scene and order and left unchanged."""
    if (name, order) not in _want:
        S = LS.build(name, order)
        A = LM.flatten(S["world"])
        rows = LM.connection_rows(S["world"], S["targets"])
        out, _ = LM.run_local_map(S["world"], S["frame_point"], S["inertial"], S["last_kf"])
        _want[(name, order)] = (A, S, out, rows)
    return _want[(name, order)]


def device_call(pkg, m, A, frame, inertial, last_kf, cap_kf, cap_pts):
    """orbm_update_local_map_device with fresh sentinel-filled outputs.  Returns (the result as the upload form returns it, clipped at the
    capacities; the raw arrays: local_kf, counts [n_kf, kf_max, max_votes, n_pts], slot_bad, local_point; what has to stay alive)."""
    import torch
    g, keep = pkg.map_graph_device(A)
    N = len(frame)
    d_fp = torch.from_numpy(np.ascontiguousarray(frame, np.int32) if N else np.zeros(1, np.int32)).cuda()
    d_kf = torch.full((cap_kf + 8,), -9, dtype=torch.int32, device="cuda")
    d_pts = torch.full((cap_pts + 8,), -9, dtype=torch.int32, device="cuda")
    d_sb = torch.full((max(N, 1),), 77, dtype=torch.uint8, device="cuda")
    d_res = torch.full((4,), -9, dtype=torch.int32, device="cuda")
    r = d_res.data_ptr()
    m.UpdateLocalMapDevice(g, N, d_fp.data_ptr(), inertial, last_kf, cap_kf, cap_pts, d_kf.data_ptr(), r, r + 4, r + 8, d_sb.data_ptr(), d_pts.data_ptr(), r + 12)
    torch.cuda.synchronize()
    kf, res, sb, pts = d_kf.cpu().numpy(), d_res.cpu().numpy(), d_sb.cpu().numpy(), d_pts.cpu().numpy()
    out = dict(local_kf=kf[:min(res[0], cap_kf)], kf_max=int(res[1]), max_votes=int(res[2]), slot_bad=sb[:N], local_point=pts[:min(res[3], cap_pts)])
    return out, (kf, res, sb, pts), (keep, d_fp, d_kf, d_pts, d_sb, d_res)


def diff(got, wanted, keys):
    return {k: (got[k], wanted[k]) for k in keys if not np.array_equal(got[k], wanted[k])}


def test_scenes_are_all_named():
    assert set(LS.ALL) == set(LS.CASES) | set(LS.SHAPES) and len(LS.ALL) == len(LS.CASES) + len(LS.SHAPES)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sorted(LS.ALL))
def test_upload_form_equals_the_model(pkg, matcher, name, order):
    A, S, out, rows = want(name, order)
    got = matcher.UpdateLocalMap(A, S["frame_point"], S["inertial"], S["last_kf"])
    assert not diff(got, out, KEYS)
    got = matcher.UpdateConnections(A, S["targets"])
    assert len(got) == len(rows) and all(not diff(g, w, CKEYS) for g, w in zip(got, rows))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sorted(LS.ALL))
def test_device_table_form_equals_the_model_and_the_upload_form(pkg, matcher, name, order):
    A, S, out, rows = want(name, order)
    G, P = len(A["kf_rank"]), len(A["pt_bad"])
    got, raw, keep = device_call(pkg, matcher, A, S["frame_point"], S["inertial"], S["last_kf"], G + 24, P)
    assert not diff(got, out, KEYS)
    assert raw[1][0] == len(out["local_kf"]) and raw[1][3] == len(out["local_point"])
    assert np.all(raw[0][raw[1][0]:] == -9) and np.all(raw[3][raw[1][3]:] == -9)       # nothing behind the lists
    up = matcher.UpdateLocalMap(A, S["frame_point"], S["inertial"], S["last_kf"])
    assert not diff(got, up, KEYS)


def test_connection_thresholds(pkg, matcher):
    for name in ("connections", "random_dense"):
        for th in (1, 14, 15, 16, 1000):
            S = LS.build(name)
            A = LM.flatten(S["world"])
            got = matcher.UpdateConnections(A, S["targets"], th=th)
            assert all(not diff(g, w, CKEYS) for g, w in zip(got, LM.connection_rows(S["world"], S["targets"], th)))


def test_one_target_with_a_counter(pkg, matcher):
    """T = 1 where block 0 of k_conn_pack is also the last: conn_start[T] and the lists of a counter that is not empty."""
    for order in ORDERS:
        S = LS.build("connections", order)
        rows = LM.connection_rows(S["world"], S["targets"][:1])
        assert len(rows[0]["conn_kf"]) == 3
        got = matcher.UpdateConnections(LM.flatten(S["world"]), S["targets"][:1])
        assert len(got) == 1 and not diff(got[0], rows[0], CKEYS)


def test_the_measurement_vote_form_equals_the_model(pkg, monkeypatch):
    """ORBM_VOTE_FORM=1 (one global atomic per vote, read when a handle is created; kept for tools/local_map_bench.py) gives the same counts."""
    monkeypatch.setenv("ORBM_VOTE_FORM", "1")
    m = pkg.ORBmatcher(0.8, False)
    try:
        for name in ("tie_bad", "random_dense", "lists", "n15360", "rows", "connections"):
            A, S, out, rows = want(name)
            assert not diff(m.UpdateLocalMap(A, S["frame_point"], S["inertial"], S["last_kf"]), out, KEYS), name
            got = m.UpdateConnections(A, S["targets"])
            assert all(not diff(g, w, CKEYS) for g, w in zip(got, rows)), name
    finally:
        m.close()


def test_empty_frame_and_no_targets(pkg, matcher):
    A, S, out, rows = want("random")
    got = matcher.UpdateLocalMap(A, np.zeros(0, np.int32))
    assert len(got["local_kf"]) == 0 and len(got["local_point"]) == 0 and got["kf_max"] == -1 and got["max_votes"] == 0
    got, raw, keep = device_call(pkg, matcher, A, np.zeros(0, np.int32), False, -1, 16, 16)
    assert np.all(raw[0] == -9) and np.all(raw[1] == -9) and np.all(raw[3] == -9)      # N == 0 launches nothing
    assert matcher.UpdateConnections(A, []) == []
    none = np.full(7, -1, np.int32)                                                     # a frame without a single map point
    got = matcher.UpdateLocalMap(A, none)
    assert len(got["local_kf"]) == 0 and len(got["local_point"]) == 0 and got["kf_max"] == -1 and not got["slot_bad"].any()


def test_capacities_one_short(pkg, matcher):
    A, S, out, rows = want("random")
    nk, npt = len(out["local_kf"]), len(out["local_point"])
    assert nk > 2 and npt > 2
    for kw in (dict(cap_kf=nk - 1, cap_pts=npt), dict(cap_kf=nk, cap_pts=npt - 1)):
        rc, o = TA.raw_local_map(pkg, A, S["frame_point"], int(S["inertial"]), S["last_kf"], host=False, m=matcher, **kw)
        assert rc == pkg.E_CAP and o[1][0] == nk and o[6][0] == npt and np.all(o[0] == -9) and np.all(o[5] == -9)
        got, raw, keep = device_call(pkg, matcher, A, S["frame_point"], S["inertial"], S["last_kf"], kw["cap_kf"], kw["cap_pts"])
        assert raw[1][0] == nk and raw[1][3] == npt                                     # the counts say what was needed
        assert np.array_equal(raw[0][:kw["cap_kf"]], out["local_kf"][:kw["cap_kf"]]) and np.all(raw[0][kw["cap_kf"]:] == -9)
        assert np.array_equal(raw[3][:kw["cap_pts"]], out["local_point"][:kw["cap_pts"]]) and np.all(raw[3][kw["cap_pts"]:] == -9)
    rc, o = TA.raw_local_map(pkg, A, S["frame_point"], int(S["inertial"]), S["last_kf"], cap_kf=nk, cap_pts=npt, host=False, m=matcher)
    assert rc == 0 and np.array_equal(o[0][:nk], out["local_kf"]) and np.array_equal(o[5][:npt], out["local_point"])
    A, S, out, rows = want("random_dense")
    need = sum(len(r["conn_kf"]) for r in rows)
    with pytest.raises(pkg.OrbError, match="needs %d" % need):
        matcher.UpdateConnections(A, S["targets"], cap=need - 1)
    got = matcher.UpdateConnections(A, S["targets"], cap=need)
    assert all(not diff(g, w, CKEYS) for g, w in zip(got, rows))


def test_refusals_on_the_handle(pkg, matcher):
    L = pkg.load()
    A, S, out, rows = want("random")
    for B, word in TA.graph_refusals(A):
        rc, o = TA.raw_local_map(pkg, B, S["frame_point"], host=False, m=matcher)
        assert rc == pkg.E_ARG and TA.untouched(o) and word in L.orbm_last_error(matcher.m), word
    rc, o = TA.raw_local_map(pkg, dict(A, kf_prev=None), S["frame_point"], inertial=1, host=False, m=matcher)
    assert rc == pkg.E_ARG and TA.untouched(o) and b"kf_prev == NULL" in L.orbm_last_error(matcher.m)
    with pytest.raises(ValueError, match="listed twice"):
        matcher.UpdateConnections(A, [1, 2, 1])
    got = matcher.UpdateLocalMap(A, S["frame_point"], S["inertial"], S["last_kf"])      # and the handle still works
    assert not diff(got, out, KEYS)


def test_a_small_call_after_a_large_one_and_back_to_back(pkg):
    m = pkg.ORBmatcher(0.8, False)                                                      # a fresh handle: the buffers grow, then are reused
    try:
        for name in ("tie_bad", "n15360", "g1", "rows", "voted1025", "first80", "first80", "tail_end"):
            A, S, out, rows = want(name)
            assert not diff(m.UpdateLocalMap(A, S["frame_point"], S["inertial"], S["last_kf"]), out, KEYS), name
            for _ in range(2):                                                          # the same call twice: the per-point word starts clear
                got, raw, keep = device_call(pkg, m, A, S["frame_point"], S["inertial"], S["last_kf"], len(A["kf_rank"]) + 24, len(A["pt_bad"]))
                assert not diff(got, out, KEYS), name
            got = m.UpdateConnections(A, S["targets"])
            assert all(not diff(g, w, CKEYS) for g, w in zip(got, rows)), name
    finally:
        m.close()


def test_four_threads_on_one_handle(pkg, matcher):
    names = ("random", "random_dense", "g65", "lists")
    for n in names:
        want(n)
    res = {}

    def work(j):
        try:
            A, S, out, rows = want(names[j])
            ok = True
            for _ in range(3):
                ok = ok and not diff(matcher.UpdateLocalMap(A, S["frame_point"], S["inertial"], S["last_kf"]), out, KEYS)
                got = matcher.UpdateConnections(A, S["targets"])
                ok = ok and all(not diff(g, w, CKEYS) for g, w in zip(got, rows))
            res[j] = ok
        except Exception as e:                                                          # reported by the assertion below
            res[j] = e

    ths = [threading.Thread(target=work, args=(j,)) for j in range(4)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert res == {0: True, 1: True, 2: True, 3: True}, res


def test_chain_into_the_local_map_search(pkg, oracle, synth, matcher):
    import torch
    import test_gpu_local_points as TLP
    f32 = np.float32
    S = TLP.make_scene(pkg, oracle, synth, 5150, "euroc", nmap=700)
    P, N = len(S.Xw), len(S.k1)
    held = np.nonzero(np.asarray(S.slot0) >= 0)[0]                                      # the slots that hold a map point: give each a point of the tables
    held = held[:P // 3]
    frame = np.full(N, -1, np.int32)
    frame[held] = np.random.RandomState(9).choice(P, size=len(held), replace=False)
    assert len(held) > 20
    Sc = LS.random_world(77, 14, P, 3, obs=(1, 5), frame_n=0)
    W = Sc["world"]
    for p in frame[frame >= 0]:
        W.pts[int(p)].bad = False                                                       # no slot is set to NULL: the frame goes on as it is
    A = LM.flatten(W)
    out, _ = LM.run_local_map(W, frame, False, -1)
    lp = out["local_point"]
    assert len(lp) > 300
    # the host's own gather, and orbm_search_local_points on it
    elig = ((A["pt_bad"][lp] == 0) & ~np.isin(lp, frame[frame >= 0])).astype(np.uint8)
    assert 0 < elig.sum() < len(lp)
    F = pkg.FrameView(S.k1, S.d1, S.bounds, u_right=S.u_right)
    F.slot[:], F.slot_obs[:] = S.slot0, S.sobs0
    n_h, moq_h, tr_h = matcher.SearchLocalPoints(F, S.sf, S.log_sf, elig, S.Xw[lp], S.normal[lp], S.maxd[lp], S.mind[lp], S.desc[lp], S.Tcw, S.cam_type,
                                                 S.cam, 3.0, mp_obs=S.obs[lp])
    assert n_h > 10
    # the chain, nothing downloaded in between
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g, keep = pkg.map_graph_device(A)
    cap = P
    d_fp, d_lp, d_res = t(frame), torch.full((cap,), -9, dtype=torch.int32, device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda")
    d_lkf, d_sb = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    tab = dict(bad=t(A["pt_bad"]), Xw=t(S.Xw.astype(f32)), nrm=t(S.normal.astype(f32)), maxd=t(S.maxd.astype(f32)), mind=t(S.mind.astype(f32)),
               desc=t(S.desc), obs=t(S.obs.astype(np.uint8)))
    o = dict(elig=torch.zeros(cap, dtype=torch.uint8, device="cuda"), Xw=torch.zeros(cap, 3, device="cuda"), nrm=torch.zeros(cap, 3, device="cuda"),
             maxd=torch.zeros(cap, device="cuda"), mind=torch.zeros(cap, device="cuda"), desc=torch.zeros(cap, 32, dtype=torch.uint8, device="cuda"),
             obs=torch.zeros(cap, dtype=torch.uint8, device="cuda"))
    d_T = t(np.asarray(S.Tcw, f32))
    ms = pkg.LocalMapStruct(cap, o["elig"].data_ptr(), o["Xw"].data_ptr(), o["nrm"].data_ptr(), o["maxd"].data_ptr(), o["mind"].data_ptr(),
                            o["desc"].data_ptr(), o["obs"].data_ptr(), d_T.data_ptr())
    r = d_res.data_ptr()
    matcher.UpdateLocalMapDevice(g, N, d_fp.data_ptr(), False, -1, 64, cap, d_lkf.data_ptr(), r, r + 4, r + 8, d_sb.data_ptr(), d_lp.data_ptr(), r + 12)
    matcher.GatherLocalMapDevice(P, N, d_fp.data_ptr(), d_lp.data_ptr(), r + 12, cap, tab["bad"].data_ptr(), tab["Xw"].data_ptr(), tab["nrm"].data_ptr(),
                                 tab["maxd"].data_ptr(), tab["mind"].data_ptr(), tab["desc"].data_ptr(), tab["obs"].data_ptr(), ms, r + 16)
    kview = np.ascontiguousarray(S.k1).view(f32).reshape(N, 7)
    d_kp, d_de, d_cnt = t(kview), t(S.d1), t(np.array([N, 0], np.int32))
    d_slot, d_sobs = t(np.asarray(S.slot0, np.int32)), t(np.asarray(S.sobs0, np.uint8))
    d_moq = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    tr = {k: torch.zeros(cap, dtype=torch.uint8 if k == "in_view" else torch.int32 if k == "level" else torch.float32, device="cuda") for k in TLP.FIELDS}
    d_nm = torch.zeros(1, dtype=torch.int32, device="cuda")
    fs = pkg.FrameStruct(N, d_kp.data_ptr(), d_de.data_ptr(), None, *S.bounds)
    ts = pkg.TrackStruct(*[tr[k].data_ptr() for k in TLP.FIELDS])
    matcher.search_local_points_batch_device(fs, N, d_cnt.data_ptr(), 2, ms, cap, r + 16, 1, 1, S.sf, S.log_sf, S.cam_type, S.cam, 3.0, d_slot.data_ptr(),
                                             d_sobs.data_ptr(), d_moq.data_ptr(), ts, d_nm.data_ptr(), mbf=S.mbf)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy()
    n = len(lp)
    assert res[3] == n and res[4] == n and np.array_equal(d_lp.cpu().numpy()[:n], lp)
    assert np.array_equal(o["elig"].cpu().numpy()[:n], elig) and np.array_equal(o["desc"].cpu().numpy()[:n], S.desc[lp])
    assert np.array_equal(o["Xw"].cpu().numpy()[:n], S.Xw[lp].astype(f32)) and np.array_equal(o["maxd"].cpu().numpy()[:n], S.maxd[lp].astype(f32))
    assert int(d_nm.cpu().numpy()[0]) == n_h and np.array_equal(d_moq.cpu().numpy()[:n], moq_h)
    assert np.array_equal(d_slot.cpu().numpy(), F.slot) and np.array_equal(d_sobs.cpu().numpy(), F.slot_obs)
