"""GPU: Tracking::SearchLocalPoints for a fisheye-stereo frame on the device (orbm_search_local_points_fisheye,
orbm_search_local_points_fisheye_batch_device): Frame::isInFrustumChecks per camera (k_local_map_project_rig), both halves of
SearchByProjection(Frame&, const vector<MapPoint*>&, ...) with the partner writes, the slot conversion (k_rig_slot_convert).

Expected values: tests/rig_local_model.py followed by OracleFisheyeFrame.search_by_projection_mp.  Everything is compared bit for
bit: the twelve track arrays as bit patterns over their whole length (the model starts from the caller's values and writes what the
reference writes, so entries the call must leave alone are covered; NaN equals NaN), slots, slot_obs, both halves of
match_of_point, nmatches.  tests/test_rig_local_abi.py holds the conditions under which the scenes exercise every branch."""
import ctypes as C

import numpy as np
import pytest

import rig_local_model as RL
import rig_model as RM
from conftest import EUROC

pytestmark = pytest.mark.gpu

f32 = np.float32
ISENT = -12345
FS, MS = 2100, 1500                    # frame / map strides of the batches: above every live count, no multiples of 256


def poison_track(n):
    return {k: np.full(n, -777 if t == np.int32 else (9 if t == np.uint8 else RL.POISON), t) for k, t in RL.FIELDS}


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return np.array_equal(a, b)


def check_track(tr, ref):
    for k, _ in RL.FIELDS:
        assert bits_equal(tr[k], ref[k]), k


def frame_of(pkg, S, slots=None):
    F = pkg.FrameView(np.concatenate([S["kl"], S["kr"]]).astype(pkg.KP_DTYPE), np.concatenate([S["dl"], S["dr"]]), S["bounds"])
    F.slot[:], F.slot_obs[:] = (S["slot0"], S["sobs0"]) if slots is None else slots
    return F


def run_host(pkg, m, S, th, bFar=False, thFar=0.0, obs="scene", partners=True, track0=None, limit=0.5, slots=None):
    F = frame_of(pkg, S, slots)
    tr = poison_track(len(S["Xw"])) if track0 is None else {k: v.copy() for k, v in track0.items()}
    n, mop, tr = m.SearchLocalPointsFisheye(F, len(S["kl"]), S["l2r"] if partners else None, S["r2l"] if partners else None, S["sf"], S["log_sf"],
                                            S["eligible"], S["Xw"], S["normal"], S["max_dist"], S["min_dist"], S["desc"], S["Tcw"], S["Trl"], S["tlr"],
                                            S["cam"], S["cam_params"], S["cam2"], S["cam_params2"], th, bFarPoints=bFar, thFarPoints=thFar,
                                            viewing_cos_limit=limit, mp_obs=S["obs"] if isinstance(obs, str) else obs, track=tr)
    return dict(n=n, mop=mop, track=tr, slot=F.slot.copy(), slot_obs=F.slot_obs.copy())


def check_result(r, E):
    check_track(r["track"], E["track"])
    assert r["n"] == E["n"]
    assert np.array_equal(r["mop"], E["mop"])
    assert np.array_equal(r["slot"], E["slot"]) and np.array_equal(r["slot_obs"], E["slot_obs"])


def same_result(a, b):
    check_track(a["track"], b["track"])
    assert a["n"] == b["n"] and np.array_equal(a["mop"], b["mop"]) and np.array_equal(a["slot"], b["slot"]) and np.array_equal(a["slot_obs"], b["slot_obs"])


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.ORBmatcher(RL.NNRATIO, True)
    yield m
    m.set_scan_mode(0); m.set_hamming_engine(2)
    m.close()


_expected = {}


def expected(oracle, synth, cam, p, th, **kw):
    key = (cam, p, th, tuple(sorted((k, v if not isinstance(v, np.ndarray) else v.tobytes()) for k, v in kw.items())))
    if key not in _expected:
        _expected[key] = RL.expected(oracle, RL.cached_scene(oracle, synth, cam, p), th, **kw)
    return _expected[key]


# ---- per-frame form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", [0, 1])
def test_per_frame_equals_model_and_oracle(pkg, oracle, synth, matcher, cam):
    """Pinhole and KannalaBrandt8; th 1 and 4; obs NULL, all 1 and mixed; with and without partner tables; the far-point gate."""
    S = RL.cached_scene(oracle, synth, cam)
    nmp = len(S["Xw"])
    tr = expected(oracle, synth, cam, 0, 1.0)["track"]
    thFar = float(np.median(tr["depth"][tr["in_view"] != 0]))
    for th in (1.0, 4.0):
        for obs in ("scene", None, np.ones(nmp, np.uint8)):
            for partners in (True, False):
                kw = dict(partners=partners) if isinstance(obs, str) else dict(partners=partners, obs=obs)
                E = expected(oracle, synth, cam, 0, th, **kw)
                r = run_host(pkg, matcher, S, th, obs=obs, partners=partners)
                print("cam %d th %g obs %s partners %d: nmatches %d (model + oracle %d)" % (cam, th, "mixed" if isinstance(obs, str) else "all", partners, r["n"], E["n"]))
                check_result(r, E)
        check_result(run_host(pkg, matcher, S, th, bFar=True, thFar=thFar), expected(oracle, synth, cam, 0, th, bFar=True, thFar=thFar))
    F = pkg.FrameView(np.zeros(0, pkg.KP_DTYPE), np.zeros((0, 32), np.uint8), S["bounds"])    # a frame without keypoints still gets its track fields
    t0 = poison_track(nmp)
    n, mop, t1 = matcher.SearchLocalPointsFisheye(F, 0, None, None, S["sf"], S["log_sf"], S["eligible"], S["Xw"], S["normal"], S["max_dist"], S["min_dist"],
                                                  S["desc"], S["Tcw"], S["Trl"], S["tlr"], S["cam"], S["cam_params"], S["cam2"], S["cam_params2"], 1.0, track=t0)
    assert n == 0 and (mop == -1).all()
    check_track(t1, tr)


def test_constructed_branches(pkg, oracle, synth, matcher):
    """The hand-placed points of rig_local_model.constructed: every rejection on each side, a NaN projection, the far-point skip decided
    by a stale incoming depth, a partner write that releases a claim held with observations, the level clamped at both ends."""
    S, track0, ix = RL.constructed(RM.stream(oracle, synth)[3])
    for kw in (dict(bFar=True, thFar=10.0), dict(bFar=False), dict(bFar=True, thFar=10.0, partners=False)):
        E = RL.expected(oracle, S, 1.0, track0=track0, **kw)
        r = run_host(pkg, matcher, S, 1.0, track0=track0, **kw)
        print(kw, "nmatches", r["n"], "slot", r["slot"].tolist(), "mop", r["mop"].tolist())
        check_result(r, E)
    E = RL.expected(oracle, S, 1.0, track0=track0, bFar=True, thFar=10.0)
    assert E["slot"][ix["kp_b"]] == ix["C"] and E["mop"][2 * ix["right_only_stale"] + 1] == -1


# ---- batch form -----------------------------------------------------------------------------------------------------------------------
def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return torch.from_numpy(a).cuda()


def pack(pkg, P, fs=FS, ms=MS, track0=None):
    """Host arrays of a batch: problem p at element offset p * fs / p * ms; junk inputs and poisoned outputs beyond the live counts."""
    n = len(P)
    rng = np.random.default_rng(5)
    B = dict(keys=np.zeros((n, fs), pkg.KP_DTYPE), desc=rng.integers(0, 256, (n, fs, 32), dtype=np.uint8), cnt=np.zeros((n, 2), np.int32),
             l2r=rng.integers(0, 50, (n, fs)).astype(np.int32), r2l=rng.integers(0, 50, (n, fs)).astype(np.int32),
             elig=np.ones((n, ms), np.uint8), Xw=rng.uniform(-1, 1, (n, ms, 3)).astype(f32) + f32([0, 0, 5]), normal=np.tile(f32([0, 0, 1]), (n, ms, 1)),
             maxd=np.full((n, ms), 10, f32), mind=np.full((n, ms), 1, f32), mpdesc=rng.integers(0, 256, (n, ms, 32), dtype=np.uint8),
             obs=np.ones((n, ms), np.uint8), Tcw=np.zeros((n, 16), f32), mn=np.zeros(n, np.int32), slot=np.full((n, fs), ISENT, np.int32),
             sobs=np.full((n, fs), 7, np.uint8), mop=np.full((n, 2 * ms), ISENT, np.int32), nm=np.full(n, ISENT, np.int32))
    B["keys"]["x"], B["keys"]["y"] = 100.0, 100.0
    for k, t in RL.FIELDS:
        B["t_" + k] = np.stack([poison_track(ms)[k]] * n)
    for p, S in enumerate(P):
        nl, nr, nmp = len(S["kl"]), len(S["kr"]), len(S["Xw"])
        assert nl + nr <= fs and nmp <= ms
        B["keys"][p, :nl + nr], B["desc"][p, :nl + nr] = np.concatenate([S["kl"], S["kr"]]), np.concatenate([S["dl"], S["dr"]])
        B["cnt"][p], B["mn"][p] = (nl + nr, nl), nmp
        B["l2r"][p, :nl], B["r2l"][p, :nr] = S["l2r"], S["r2l"]
        B["elig"][p, :nmp], B["Xw"][p, :nmp], B["normal"][p, :nmp], B["maxd"][p, :nmp], B["mind"][p, :nmp] = S["eligible"], S["Xw"], S["normal"], S["max_dist"], S["min_dist"]
        B["mpdesc"][p, :nmp], B["obs"][p, :nmp], B["Tcw"][p] = S["desc"], S["obs"], S["Tcw"].reshape(-1)
        B["slot"][p, :nl + nr], B["sobs"][p, :nl + nr] = S["slot0"], S["sobs0"]
        if track0 is not None:
            for k, _ in RL.FIELDS:
                B["t_" + k][p, :nmp] = track0[p][k]
    return B


def structs(pkg, B, D, obs=True):
    cur = pkg.FrameStruct(int(B["cnt"][0, 0]), D["keys"].data_ptr(), D["desc"].data_ptr(), None, *[C.c_float(b) for b in RM.BOUNDS])
    mp = pkg.LocalMapStruct(int(B["mn"][0]), D["elig"].data_ptr(), D["Xw"].data_ptr(), D["normal"].data_ptr(), D["maxd"].data_ptr(), D["mind"].data_ptr(),
                            D["mpdesc"].data_ptr(), D["obs"].data_ptr() if obs else None, D["Tcw"].data_ptr())
    ts = pkg.TrackRigStruct(*[D["t_" + k].data_ptr() for k, _ in RL.FIELDS])
    return cur, mp, ts


def run_batch(pkg, m, P, th, bFar=False, thFar=0.0, obs=True, partners=True, counts_on_device=True, nleft_on_device=True, fs=FS, ms=MS, track0=None,
              stream=None):
    """One call of the batch form over the scenes P -> per problem the dict run_host returns; what lies beyond the live counts is checked
    against its poison here."""
    import torch
    B = pack(pkg, P, fs, ms, track0)
    n, S0 = len(P), P[0]
    D = {k: to_dev(v) for k, v in B.items()}
    cur, mp, ts = structs(pkg, B, D, obs)
    dn, dmn = (D["cnt"].data_ptr(), D["mn"].data_ptr()) if counts_on_device else (None, None)
    dnl = D["cnt"].data_ptr() + 4 if nleft_on_device else None
    rc = m.search_local_points_fisheye_batch_device(cur, fs, dn, 2, dnl, 2, D["l2r"].data_ptr() if partners else None, D["r2l"].data_ptr() if partners else None,
                                                    mp, ms, dmn, 1, n, S0["sf"], S0["log_sf"], S0["Trl"], S0["tlr"], S0["cam"], S0["cam_params"], S0["cam2"],
                                                    S0["cam_params2"], th, D["slot"].data_ptr(), D["sobs"].data_ptr(), D["mop"].data_ptr(), ts,
                                                    D["nm"].data_ptr(), n_left=int(B["cnt"][0, 1]), bFarPoints=bFar, thFarPoints=thFar, stream=stream)
    assert rc == 0
    torch.cuda.synchronize()
    H = {k: v.cpu().numpy() for k, v in D.items()}
    for k in ("keys", "desc", "cnt", "l2r", "r2l", "elig", "Xw", "normal", "maxd", "mind", "mpdesc", "obs", "Tcw", "mn"):      # inputs are inputs
        assert np.array_equal(H[k].view(np.uint8).reshape(-1), np.ascontiguousarray(B[k]).view(np.uint8).reshape(-1)), k
    out = []
    pz = poison_track(ms)
    for p in range(n):
        N, nmp = int(B["cnt"][p, 0]), int(B["mn"][p])
        assert (H["slot"][p, N:] == ISENT).all() and (H["sobs"][p, N:] == 7).all() and (H["mop"][p, 2 * nmp:] == ISENT).all()
        for k, _ in RL.FIELDS:
            assert bits_equal(H["t_" + k][p, nmp:], pz[k][nmp:]), k
        out.append(dict(n=int(H["nm"][p]), mop=H["mop"][p, :2 * nmp].copy(), track={k: H["t_" + k][p, :nmp].copy() for k, _ in RL.FIELDS},
                        slot=H["slot"][p, :N].copy(), slot_obs=H["sobs"][p, :N].copy()))
    return out


def variant(S, nleft0=False, nleftN=False, nomap=False):
    """A scene with every keypoint in the right image (Nleft = 0), in the left image (Nleft = N), or with an empty local map."""
    V = dict(S)
    nl, nr = len(S["kl"]), len(S["kr"])
    if nleft0:
        V.update(kl=S["kl"][:0], dl=S["dl"][:0], l2r=S["l2r"][:0], r2l=np.full(nr, -1, np.int32), slot0=S["slot0"][nl:], sobs0=S["sobs0"][nl:])
    if nleftN:
        V.update(kr=S["kr"][:0], dr=S["dr"][:0], r2l=S["r2l"][:0], l2r=np.full(nl, -1, np.int32), slot0=S["slot0"][:nl], sobs0=S["sobs0"][:nl])
    if nomap:
        for k in ("Xw", "normal", "max_dist", "min_dist", "eligible", "obs", "desc"):
            V[k] = S[k][:0]
    return V


@pytest.mark.parametrize("cam", [0, 1])
def test_batch_equals_oracle_all_modes(pkg, oracle, synth, matcher, cam):
    """Four problems with different N, Nleft and map counts from device counts; both forced scan modes and the vote on the device; the
    three Hamming engines (rig problems never take the matrix-pipe forms, so the engines must agree bit for bit)."""
    P = [RL.cached_scene(oracle, synth, cam, p) for p in range(4)]
    assert len(set(len(S["kl"]) for S in P)) == 4 and len(set(len(S["kl"]) + len(S["kr"]) for S in P)) == 4 and len(set(len(S["Xw"]) for S in P)) == 4
    assert all(len(S["kl"]) + len(S["kr"]) < FS and len(S["Xw"]) < MS for S in P) and FS % 256 and MS % 256
    for th in (1.0, 4.0):
        ref = [expected(oracle, synth, cam, p, th) for p in range(4)]
        for mode, engine in ((0, 2), (1, 0), (2, 1), (1, 2), (2, 0), (0, 1)) if th == 4.0 else ((0, 2),):
            matcher.set_scan_mode(mode); matcher.set_hamming_engine(engine)
            res = run_batch(pkg, matcher, P, th)
            for p, (r, E) in enumerate(zip(res, ref)):
                print("cam %d th %g mode %d engine %d problem %d: nmatches %d (model + oracle %d)" % (cam, th, mode, engine, p, r["n"], E["n"]))
                check_result(r, E)
    matcher.set_scan_mode(0); matcher.set_hamming_engine(2)


def test_batch_equals_per_frame_form(pkg, oracle, synth, matcher):
    """The batch call equals four calls of the per-frame form; obs NULL (the search is not serial then) and without partner tables;
    constant counts (npairs = 1) with Nleft constant and from device memory."""
    P = [RL.cached_scene(oracle, synth, 1, p) for p in range(4)]
    for kw_b, kw_h in ((dict(), dict()), (dict(obs=False), dict(obs=None)), (dict(partners=False), dict(partners=False))):
        res = run_batch(pkg, matcher, P, 4.0, **kw_b)
        for S, r in zip(P, res):
            same_result(r, run_host(pkg, matcher, S, 4.0, **kw_h))
    S = P[2]
    N, nmp = len(S["kl"]) + len(S["kr"]), len(S["Xw"])
    ref = run_host(pkg, matcher, S, 4.0)
    for nld in (False, True):
        same_result(run_batch(pkg, matcher, [S], 4.0, counts_on_device=False, nleft_on_device=nld, fs=N, ms=nmp)[0], ref)


def test_batch_degenerate_problems(pkg, oracle, synth, matcher):
    """One call over: a full problem, one with 0 live map points, one with Nleft = 0, one with Nleft = N; strides above the live counts."""
    S = RL.cached_scene(oracle, synth, 0, 1)
    P = [S, variant(S, nomap=True), variant(S, nleft0=True), variant(S, nleftN=True)]
    res = run_batch(pkg, matcher, P, 4.0)
    for p, (V, r) in enumerate(zip(P, res)):
        E = RL.expected(oracle, V, 4.0)
        print("problem %d: N %d Nleft %d map %d nmatches %d (model + oracle %d)" % (p, len(V["kl"]) + len(V["kr"]), len(V["kl"]), len(V["Xw"]), r["n"], E["n"]))
        check_result(r, E)
    assert res[1]["n"] == 0 and res[2]["n"] > 50 and res[3]["n"] > 50
    assert (res[2]["mop"][0::2] == -1).all() and (res[3]["mop"][1::2] == -1).all()


def test_batch_partner_entries_out_of_range(pkg, oracle, synth, matcher):
    """The batch form cannot refuse data it has not seen: a partner index outside the other image's live range counts as -1."""
    S = dict(RL.cached_scene(oracle, synth, 0, 3))
    nl, nr = len(S["kl"]), len(S["kr"])
    rng = np.random.default_rng(8)
    bad_l, bad_r = rng.permutation(nl)[:80], rng.permutation(nr)[:80]
    V = dict(S, l2r=S["l2r"].copy(), r2l=S["r2l"].copy())
    V["l2r"][bad_l] = rng.choice(np.array([nr, nr + 7, FS - 1, 2 ** 30, -5], np.int32), 80)
    V["r2l"][bad_r] = rng.choice(np.array([nl, nl + 3, FS - 1, 2 ** 30, -2], np.int32), 80)
    C_ = dict(S, l2r=S["l2r"].copy(), r2l=S["r2l"].copy())
    C_["l2r"][bad_l], C_["r2l"][bad_r] = -1, -1
    check_result(run_batch(pkg, matcher, [V], 4.0)[0], RL.expected(oracle, C_, 4.0))
    with pytest.raises(ValueError):                                   # the per-frame form refuses it
        run_host(pkg, matcher, dict(V, l2r=np.where(V["l2r"] < 0, -1, V["l2r"])), 4.0)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", [0, 1])
def test_chain_from_extraction(pkg, oracle, synth, matcher, cam):
    """Two rig frames: extraction of the left and the right images, orbm_rig_concat_batch_device and the new batch call on one stream
    without a synchronisation in between; the result equals the per-frame form (and model + oracle) on the downloaded extraction."""
    import torch
    frames, offs, ext, sf = RM.stream(oracle, synth)
    H, W = frames.shape[1:]
    n = len(RM.CHAIN_FRAMES)
    exL, exR = pkg.ORBextractor(**EUROC), pkg.ORBextractor(**EUROC)
    cap = exL.configure(H, W, n)
    assert exR.configure(H, W, n) == cap and 2 * cap <= pkg.FISHEYE_MAX_KEYPOINTS
    base = RL.scene(oracle, synth, cam, 0, nextra=100, nedge=100, ndup=0)          # the local map, pose and rig; keypoints come from the device
    nmp = len(base["Xw"])
    rng = np.random.default_rng(21)
    l2r, r2l = rng.integers(-1, cap, (n, 2 * cap)).astype(np.int32), rng.integers(-1, cap, (n, 2 * cap)).astype(np.int32)   # some beyond the live counts
    l2r[rng.random(l2r.shape) < 0.5] = -1
    r2l[rng.random(r2l.shape) < 0.5] = -1
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        rep = lambda a: t(np.stack([a] * n))
        d_L, d_R = t(np.stack([frames[c[0]] for c in RM.CHAIN_FRAMES])), t(np.stack([frames[c[1]] for c in RM.CHAIN_FRAMES]))
        D = dict(elig=rep(base["eligible"]), Xw=rep(base["Xw"]), normal=rep(base["normal"]), maxd=rep(base["max_dist"]), mind=rep(base["min_dist"]),
                 mpdesc=rep(base["desc"]), obs=rep(base["obs"]), Tcw=rep(base["Tcw"].reshape(-1)), l2r=t(l2r), r2l=t(r2l))
        for k, _ in RL.FIELDS:
            D["t_" + k] = rep(poison_track(nmp)[k])
        mk = lambda: (torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda"), torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda"),
                      torch.zeros((n, 2), dtype=torch.int32, device="cuda"))
        (kL, dL, cL), (kR, dR, cR) = mk(), mk()
        d_keys = torch.zeros((n, 2 * cap, 28), dtype=torch.uint8, device="cuda")
        d_desc = torch.zeros((n, 2 * cap, 32), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        d_slot = torch.full((n, 2 * cap), -1, dtype=torch.int32, device="cuda")
        d_sobs = torch.zeros((n, 2 * cap), dtype=torch.uint8, device="cuda")
        d_mop = torch.full((n, 2 * nmp), ISENT, dtype=torch.int32, device="cuda")
        d_nm = torch.zeros((n,), dtype=torch.int32, device="cuda")
        st.synchronize()                                                # the inputs are in place; from here on nothing waits
        s = st.cuda_stream
        exL.extract_batch_device(d_L.data_ptr(), H, W, W, H * W, n, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), cap, RM.CHAIN_LAP[0], stream=s)
        exR.extract_batch_device(d_R.data_ptr(), H, W, W, H * W, n, kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap, RM.CHAIN_LAP[1], stream=s)
        assert pkg.rig_concat_batch_device(n, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap,
                                           d_keys.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), stream=s) == 0
        cur = pkg.FrameStruct(2 * cap, d_keys.data_ptr(), d_desc.data_ptr(), None, *[C.c_float(b) for b in RM.BOUNDS])
        mp = pkg.LocalMapStruct(nmp, D["elig"].data_ptr(), D["Xw"].data_ptr(), D["normal"].data_ptr(), D["maxd"].data_ptr(), D["mind"].data_ptr(),
                                D["mpdesc"].data_ptr(), D["obs"].data_ptr(), D["Tcw"].data_ptr())
        ts = pkg.TrackRigStruct(*[D["t_" + k].data_ptr() for k, _ in RL.FIELDS])
        matcher.search_local_points_fisheye_batch_device(cur, 2 * cap, d_n.data_ptr(), 2, d_n.data_ptr() + 4, 2, D["l2r"].data_ptr(), D["r2l"].data_ptr(), mp, nmp,
                                                         None, 0, n, sf, base["log_sf"], base["Trl"], base["tlr"], cam, base["cam_params"], cam,
                                                         base["cam_params2"], 4.0, d_slot.data_ptr(), d_sobs.data_ptr(), d_mop.data_ptr(), ts, d_nm.data_ptr(),
                                                         stream=s)
    torch.cuda.synchronize()                                            # the one synchronisation of the chain
    nn, slot, sobs, nm, mop = d_n.cpu().numpy(), d_slot.cpu().numpy(), d_sobs.cpu().numpy(), d_nm.cpu().numpy(), d_mop.cpu().numpy()
    keys = d_keys.cpu().numpy().reshape(n, 2 * cap * 28).view(pkg.KP_DTYPE).reshape(n, 2 * cap)
    desc = d_desc.cpu().numpy()
    for f in range(n):
        N, nl = int(nn[f, 0]), int(nn[f, 1])
        assert nl > 500 and N - nl > 500
        a, b = l2r[f, :nl].copy(), r2l[f, :N - nl].copy()
        a[a >= N - nl], b[b >= nl] = -1, -1
        S = dict(base, kl=keys[f, :nl], dl=desc[f, :nl], kr=keys[f, nl:N], dr=desc[f, nl:N], l2r=a, r2l=b, slot0=np.full(N, -1, np.int32),
                 sobs0=np.zeros(N, np.uint8))
        r = dict(n=int(nm[f]), mop=mop[f], track={k: D["t_" + k].cpu().numpy()[f] for k, _ in RL.FIELDS}, slot=slot[f, :N], slot_obs=sobs[f, :N])
        same_result(r, run_host(pkg, matcher, S, 4.0))
        E = RL.expected(oracle, S, 4.0)
        print("cam %d frame %d: N %d Nleft %d nmatches %d (model + oracle %d), %d right" % (cam, f, N, nl, nm[f], E["n"], int((E["mR"] >= 0).sum())))
        check_result(r, E)
        assert (slot[f, N:] == -1).all()
        if f == 0:                                                      # the map was placed for this frame's left image
            assert E["n"] > 100 and (E["mR"] >= 0).sum() >= 20
    exL.close(); exR.close()


# ---- seeded sweep ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", range(4))
def test_random_sweep(pkg, oracle, synth, matcher, chunk):
    """20 cases in four chunks: a random subset of the map, random pose and rig perturbations, bounds, eligibility, observations,
    pre-occupied slots, incoming track values, th, the far-point gate and the viewing-cosine limit."""
    for case in range(5 * chunk, 5 * chunk + 5):
        rng = np.random.default_rng(7000 + case)
        cam = case & 1
        S = dict(RL.cached_scene(oracle, synth, cam, case % 4))
        nmp = len(S["Xw"])
        keep = np.sort(rng.permutation(nmp)[: int(rng.integers(250, 500))])
        for k in ("Xw", "normal", "max_dist", "min_dist", "desc"):
            S[k] = np.ascontiguousarray(S[k][keep])
        n = len(keep)
        S["eligible"], S["obs"] = (rng.random(n) < rng.uniform(0.5, 1.0)).astype(np.uint8), (rng.random(n) < rng.uniform(0.3, 1.0)).astype(np.uint8)
        T = S["Tcw"].astype(np.float64)
        dR = RL.rot(0, rng.normal() * 0.02) @ RL.rot(1, rng.normal() * 0.02) @ RL.rot(2, rng.normal() * 0.02)
        T[:3, :3], T[:3, 3] = dR @ T[:3, :3], dR @ T[:3, 3] + rng.normal(size=3) * 0.05
        S["Tcw"] = T.astype(f32)
        G = S["Trl"].astype(np.float64)
        G[:3, :3], G[:3, 3] = RL.rot(1, rng.normal() * 0.01) @ G[:3, :3], G[:3, 3] + rng.normal(size=3) * 0.01
        S["Trl"], S["tlr"] = G.astype(f32), (-(G[:3, :3].T @ G[:3, 3]) + rng.normal(size=3) * 0.002).astype(f32)
        p2 = S["cam_params2"].copy()
        p2[:4] = (p2[:4] * rng.uniform(0.995, 1.005, 4)).astype(f32)
        S["cam_params2"] = p2
        S["bounds"] = (float(rng.uniform(0, 60)), float(rng.uniform(690, 752)), float(rng.uniform(0, 40)), float(rng.uniform(440, 480)))
        N = len(S["kl"]) + len(S["kr"])
        pre = rng.random(N) < rng.uniform(0.0, 0.3)
        S["slot0"], S["sobs0"] = np.where(pre, RL.PRE_VALUE, -1).astype(np.int32), (pre & (rng.random(N) < 0.5)).astype(np.uint8)
        t0 = poison_track(n)
        t0["depth"] = rng.uniform(0, 12, n).astype(f32)
        kw = dict(bFar=bool(rng.random() < 0.5), thFar=float(rng.uniform(4, 7)), limit=float(rng.choice([0.5, 0.2, 0.9])), partners=bool(rng.random() < 0.8))
        th = float(rng.choice([1.0, 2.0, 3.0, 5.0, 10.0, 15.0]))
        E = RL.expected(oracle, S, th, track0=t0, **kw)
        r = run_host(pkg, matcher, S, th, track0=t0, **kw)
        print("case %d cam %d th %g %s: map %d classes %s nmatches %d (model + oracle %d)" % (case, cam, th, kw, n, RL.classes(E["track"], S["eligible"]), r["n"], E["n"]))
        check_result(r, E)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_handle(pkg, oracle, synth, matcher):
    """Every refusal leaves the outputs as they were (nothing is launched)."""
    import torch
    S = RL.cached_scene(oracle, synth, 0, 0)
    nl, nr, nmp = len(S["kl"]), len(S["kr"]), len(S["Xw"])
    N = nl + nr
    # per-frame form, straight at the library
    F = frame_of(pkg, S)
    slot0, sobs0 = F.slot.copy(), F.slot_obs.copy()
    tr = poison_track(nmp)
    mop = np.full(2 * nmp, ISENT, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    keep = dict(sf=np.ascontiguousarray(S["sf"], f32), Trl=np.ascontiguousarray(S["Trl"], f32), tlr=np.ascontiguousarray(S["tlr"], f32), Tcw=np.ascontiguousarray(S["Tcw"], f32),
                cp=np.ascontiguousarray(S["cam_params"], f32), cp2=np.ascontiguousarray(S["cam_params2"], f32), l2r=S["l2r"].copy(), r2l=S["r2l"].copy())

    def host(**kw):
        a = dict(n=N, n_left=nl, l2r=keep["l2r"], r2l=keep["r2l"], nlevels=len(S["sf"]), Trl=keep["Trl"], tlr=keep["tlr"], cam_type=0, cp=keep["cp"], cam_type2=0,
                 cp2=keep["cp2"], slot=F.slot, sobs=F.slot_obs, elig=S["eligible"], track=tr, bounds=S["bounds"])
        a.update(kw)
        fs = F.struct()
        fs.n = a["n"]
        fs.min_x, fs.max_x, fs.min_y, fs.max_y = a["bounds"]
        ms = pkg.LocalMapStruct(nmp, p(a["elig"]), p(S["Xw"]), p(S["normal"]), p(S["max_dist"]), p(S["min_dist"]), p(S["desc"]), p(S["obs"]), p(keep["Tcw"]))
        ts = pkg.TrackRigStruct(*[p(a["track"][k]) for k, _ in RL.FIELDS])
        return matcher.L.orbm_search_local_points_fisheye(matcher.m, C.byref(fs), a["n_left"], p(a["l2r"]), p(a["r2l"]), p(keep["sf"]), a["nlevels"],
                                                          C.c_float(S["log_sf"]), C.byref(ms), p(a["Trl"]), p(a["tlr"]), a["cam_type"], p(a["cp"]), a["cam_type2"],
                                                          p(a["cp2"]), C.c_float(0.5), C.c_float(1.0), 0, C.c_float(0.0), C.c_float(0.8), p(a["slot"]), p(a["sobs"]), p(mop),
                                                          C.byref(ts))
    bad_l2r, bad_r2l = keep["l2r"].copy(), keep["r2l"].copy()
    bad_l2r[5], bad_r2l[7] = nr, nl
    bad = [dict(Trl=None), dict(tlr=None), dict(cp2=None), dict(cp=None), dict(cam_type2=2), dict(cam_type=-1), dict(n_left=-1), dict(n_left=N + 1), dict(nlevels=0),
           dict(nlevels=17), dict(n=pkg.FISHEYE_MAX_KEYPOINTS + 1, n_left=0), dict(l2r=bad_l2r), dict(r2l=bad_r2l), dict(slot=None), dict(sobs=None),
           dict(elig=None), dict(track=dict(tr, depth_r=None)), dict(track=dict(tr, in_view_r=None)), dict(bounds=(0.0, 0.0, 0.0, 480.0))]
    for c in bad:
        assert host(**c) == pkg.E_ARG, c
    assert np.array_equal(F.slot, slot0) and np.array_equal(F.slot_obs, sobs0) and (mop == ISENT).all()
    check_track(tr, poison_track(nmp))
    # batch form next to live device buffers
    B = pack(pkg, [S])
    D = {k: to_dev(v) for k, v in B.items()}
    before = {k: D[k].clone() for k in D}

    def batch(cur=None, mp=None, track=None, **kw):
        cs, ls, ts = structs(pkg, B, D)
        for k, v in (cur or {}).items():
            setattr(cs, k, v)
        for k, v in (mp or {}).items():
            setattr(ls, k, v)
        for k, v in (track or {}).items():
            setattr(ts, k, v)
        a = dict(frame_stride=FS, d_frame_n=None, frame_n_stride=0, d_n_left=None, n_left_stride=0, d_left_to_right=D["l2r"].data_ptr(),
                 d_right_to_left=D["r2l"].data_ptr(), map_stride=MS, d_map_n=None, map_n_stride=0, npairs=1, scale_factors=S["sf"], log_scale_factor=S["log_sf"],
                 Trl=S["Trl"], tlr=S["tlr"], cam_type=0, cam_params=S["cam_params"], cam_type2=0, cam_params2=S["cam_params2"], th=1.0, d_slot=D["slot"].data_ptr(),
                 d_slot_obs=D["sobs"].data_ptr(), d_match_of_point=D["mop"].data_ptr(), track0=ts, d_nmatches=D["nm"].data_ptr(), n_left=nl)
        a.update(kw)
        return matcher.search_local_points_fisheye_batch_device(cs, a.pop("frame_stride"), a.pop("d_frame_n"), a.pop("frame_n_stride"), a.pop("d_n_left"),
                                                                a.pop("n_left_stride"), a.pop("d_left_to_right"), a.pop("d_right_to_left"), ls, a.pop("map_stride"),
                                                                a.pop("d_map_n"), a.pop("map_n_stride"), a.pop("npairs"), **a)
    badb = [dict(cur=dict(keys_un=None)), dict(cur=dict(descriptors=None)), dict(cur=dict(max_x=0.0)), dict(cur=dict(n=0)), dict(cur=dict(n=FS + 1)),
            dict(mp=dict(eligible=None)), dict(mp=dict(Xw=None)), dict(mp=dict(normal=None)), dict(mp=dict(max_dist=None)), dict(mp=dict(min_dist=None)),
            dict(mp=dict(mpdesc=None)), dict(mp=dict(Tcw=None)), dict(mp=dict(n=0)), dict(mp=dict(n=MS + 1)), dict(track=dict(proj_yr=None)),
            dict(track=dict(level_r=None)), dict(Trl=None), dict(tlr=None), dict(n_left=-1), dict(n_left=N + 1), dict(npairs=-1), dict(cam_type=2), dict(cam_type2=2),
            dict(scale_factors=np.ones(17, f32)), dict(d_slot=None), dict(d_slot_obs=None), dict(d_nmatches=None),
            dict(frame_stride=pkg.FISHEYE_MAX_KEYPOINTS + 1, d_frame_n=D["cnt"].data_ptr(), frame_n_stride=2)]
    for c in badb:
        with pytest.raises(ValueError):
            batch(**c)
    assert batch(npairs=0) == 0
    torch.cuda.synchronize()
    for k in D:
        assert torch.equal(D[k], before[k]), k
