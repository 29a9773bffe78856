"""orbm_rig_concat_batch_device (the Frame of a two-camera fisheye rig, Frame.cc:1162-1164, :1201) and
orbm_search_by_projection_last_frame_fisheye_batch_device (ORBmatcher.cc:2027-2289 for CurrentFrame.Nleft != -1, with the
right-camera pass :2189-2256) for frames that stay on the device.

Reference: the oracle's restatement of the member (OracleFisheyeFrame.search_by_projection_ff), index-exact; the concatenation
against np.concatenate by bytes.  Entries the calls must leave alone keep a sentinel.  tests/test_rig_abi.py holds the conditions
under which the scenes of tests/rig_model.py exercise both images and the rotation histogram."""
import ctypes as C

import numpy as np
import pytest

import rig_model as RM
from conftest import EUROC

pytestmark = pytest.mark.gpu

ISENT = -12345
FS, LS = 2000, 1024                    # frame / last-frame strides of the batches: above every count of the scenes, Key32 frames


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.names:                                    # keypoints: 28 bytes each
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return torch.from_numpy(a).cuda()


def pack(pkg, P, fs=FS, ls=LS):
    """Host arrays of a batch: problem p at element offset p * fs / p * ls, junk beyond the live counts."""
    n = len(P)
    rng = np.random.default_rng(5)
    B = dict(keys=np.zeros((n, fs), pkg.KP_DTYPE), desc=rng.integers(0, 256, (n, fs, 32), dtype=np.uint8), cnt=np.zeros((n, 2), np.int32),
             has=np.ones((n, ls), np.uint8), Xw=rng.uniform(-1, 1, (n, ls, 3)).astype(np.float32) + np.float32([0, 0, 5]),
             mpdesc=rng.integers(0, 256, (n, ls, 32), dtype=np.uint8), lk=np.zeros((n, ls), pkg.KP_DTYPE), obs=np.ones((n, ls), np.uint8),
             Tcw=np.zeros((n, 16), np.float32), Tlw=np.zeros((n, 16), np.float32), ln=np.zeros(n, np.int32),
             slot=np.full((n, fs), ISENT, np.int32), sobs=np.full((n, fs), 7, np.uint8))
    B["keys"]["x"], B["keys"]["y"] = 100.0, 100.0        # junk keypoints beyond N lie inside the image: reading one would show
    for p, q in enumerate(P):
        nl, nr, n0 = len(q["kl"]), len(q["kr"]), len(q["k0"])
        assert nl + nr <= fs and n0 <= ls
        B["keys"][p, :nl + nr] = np.concatenate([q["kl"], q["kr"]])
        B["desc"][p, :nl + nr] = np.concatenate([q["dl"], q["dr"]])
        B["cnt"][p] = (nl + nr, nl)
        B["has"][p, :n0], B["Xw"][p, :n0], B["mpdesc"][p, :n0], B["lk"][p, :n0], B["obs"][p, :n0] = q["has_mp"], q["Xw"], q["d0"], q["k0"], q["obs"]
        B["Tcw"][p], B["Tlw"][p], B["ln"][p] = q["Tcw"].reshape(-1), q["Tlw"].reshape(-1), n0
        B["slot"][p, :nl + nr], B["sobs"][p, :nl + nr] = q["slots"] if "slots" in q else RM.initial_slots(q)
    return B


def run_batch(pkg, m, P, th, mono=False, cam=None, Trl=None, counts_on_device=True, stream=None, fs=FS, ls=LS):
    """One call of the batch form over the problems P -> per problem (nmatches, slot[:N], slot_obs[:N], moq[:2 nLast]); the entries
    beyond the live counts are checked against their sentinels here."""
    import torch
    B = pack(pkg, P, fs, ls)
    n = len(P)
    D = {k: to_dev(v) for k, v in B.items()}
    d_moq = torch.full((n, 2 * ls), ISENT, dtype=torch.int32, device="cuda")
    d_nm = torch.full((n,), ISENT, dtype=torch.int32, device="cuda")
    cam = P[0]["cam"] if cam is None else cam
    cur = pkg.FrameStruct(int(B["cnt"][0, 0]), D["keys"].data_ptr(), D["desc"].data_ptr(), None, *[C.c_float(b) for b in RM.BOUNDS])
    last = pkg.LastFrameStruct(int(B["ln"][0]), D["has"].data_ptr(), D["Xw"].data_ptr(), D["mpdesc"].data_ptr(), D["lk"].data_ptr(), D["obs"].data_ptr(),
                               D["Tcw"].data_ptr(), D["Tlw"].data_ptr())
    if counts_on_device:
        dn, dnl, dln = D["cnt"].data_ptr(), D["cnt"].data_ptr() + 4, D["ln"].data_ptr()
    else:
        assert n == 1
        dn = dnl = dln = None
    rc = m.search_by_projection_last_frame_fisheye_batch_device(cur, fs, dn, 2, dnl, 2, last, ls, dln, 1, n, P[0]["sf"], P[0]["Trl"] if Trl is None else Trl,
                                                                cam, RM.CAMS[cam], th, D["slot"].data_ptr(), D["sobs"].data_ptr(), d_moq.data_ptr(),
                                                                d_nm.data_ptr(), n_left=int(B["cnt"][0, 1]), bMono=mono, mb=RM.MB, stream=stream)
    assert rc == 0
    torch.cuda.synchronize()
    slot, sobs, moq, nm = D["slot"].cpu().numpy(), D["sobs"].cpu().numpy(), d_moq.cpu().numpy(), d_nm.cpu().numpy()
    out = []
    for p in range(n):
        N, n0 = int(B["cnt"][p, 0]), int(B["ln"][p])
        assert (slot[p, N:] == ISENT).all() and (sobs[p, N:] == 7).all() and (moq[p, 2 * n0:] == ISENT).all()
        out.append((int(nm[p]), slot[p, :N].copy(), sobs[p, :N].copy(), moq[p, :2 * n0].copy()))
    return out


def check_moq(q, res, slots0=None):
    """match_of_query against the slots: entry 2i / 2i + 1 points into the left / right image; a keypoint that holds a new point
    was matched by some query, and where a matched keypoint still holds a point that is the LAST query that matched it (>> 1)."""
    nm, slot, sobs, moq = res
    nl, N = len(q["kl"]), len(q["kl"]) + len(q["kr"])
    s0 = (q["slots"] if "slots" in q else RM.initial_slots(q))[0] if slots0 is None else slots0
    L, R = moq[0::2], moq[1::2]
    assert ((L == -1) | ((L >= 0) & (L < nl))).all() and ((R == -1) | ((R >= nl) & (R < N))).all()
    assert (L[q["has_mp"] == 0] == -1).all() and (R[q["has_mp"] == 0] == -1).all()
    last = np.full(N, -1, np.int64)
    for j in np.nonzero(moq >= 0)[0]:
        last[moq[j]] = j                                  # ascending j: the last writer stays
    changed = (slot != s0) & (slot >= 0)                  # an occupied slot without observations that was taken and pruned ends at -1
    assert (last[changed] >= 0).all() and (s0[(slot != s0) & (slot < 0)] >= 0).all()
    held = (last >= 0) & (slot >= 0)
    assert np.array_equal(slot[held], last[held] >> 1)
    assert nm == int((moq >= 0).sum())                    # every surviving query counts, two on one keypoint twice (:2281-2282)


_oracle_cache = {}


def oracle_results(oracle, synth, cam, th, mono=False):
    key = (cam, th, mono)
    if key not in _oracle_cache:
        _oracle_cache[key] = [RM.oracle_search(oracle, q, th, mono=mono) for q in RM.problems(oracle, synth, cam)]
    return _oracle_cache[key]


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.ORBmatcher(0.9, True)
    yield m
    m.set_scan_mode(0); m.set_hamming_engine(2)
    m.close()


def test_concat_equals_numpy(pkg):
    import torch
    cap, counts = 40, ((17, 0), (0, 23), (31, 29))
    n = len(counts)
    rng = np.random.default_rng(11)
    kL, kR = rng.integers(0, 256, (n, cap, 28), dtype=np.uint8), rng.integers(0, 256, (n, cap, 28), dtype=np.uint8)
    dL, dR = rng.integers(0, 256, (n, cap, 32), dtype=np.uint8), rng.integers(0, 256, (n, cap, 32), dtype=np.uint8)
    cL = np.array([[c[0], -3] for c in counts], np.int32)             # element 1 = monoIndex: not read
    cR = np.array([[c[1], 99] for c in counts], np.int32)
    D = [to_dev(a) for a in (kL, dL, cL, kR, dR, cR)]
    d_keys = torch.full((n, 2 * cap, 28), 0xA5, dtype=torch.uint8, device="cuda")
    d_desc = torch.full((n, 2 * cap, 32), 0x5A, dtype=torch.uint8, device="cuda")
    d_n = torch.full((n, 2), ISENT, dtype=torch.int32, device="cuda")
    assert pkg.rig_concat_batch_device(n, *[d.data_ptr() for d in D], cap, d_keys.data_ptr(), d_desc.data_ptr(), d_n.data_ptr()) == 0
    torch.cuda.synchronize()
    keys, desc, nn = d_keys.cpu().numpy(), d_desc.cpu().numpy(), d_n.cpu().numpy()
    for f, (nl, nr) in enumerate(counts):
        assert tuple(nn[f]) == (nl + nr, nl)
        assert np.array_equal(keys[f, :nl + nr], np.concatenate([kL[f, :nl], kR[f, :nr]]))
        assert np.array_equal(desc[f, :nl + nr], np.concatenate([dL[f, :nl], dR[f, :nr]]))
        assert (keys[f, nl + nr:] == 0xA5).all() and (desc[f, nl + nr:] == 0x5A).all()
    # a partial batch leaves the other frames alone
    d_n.fill_(ISENT); d_keys.fill_(0xA5)
    assert pkg.rig_concat_batch_device(1, *[d.data_ptr() for d in D], cap, d_keys.data_ptr(), d_desc.data_ptr(), d_n.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (d_n.cpu().numpy()[1:] == ISENT).all() and (d_keys.cpu().numpy()[1:] == 0xA5).all()


@pytest.mark.parametrize("cam", [0, 1])
def test_batch_equals_oracle(pkg, oracle, synth, matcher, cam):
    """Four problems per call (forward, backward, neutral level windows; N, Nleft and nLast read from device counts), two values of
    th, the bMono form through a second call; scan, walk and the vote on the device; Hamming engines 0 and 2 (rig problems are
    never routed to the matrix-pipe or fused forms, so the engines must agree bit for bit)."""
    P = RM.problems(oracle, synth, cam)
    assert len(set(len(q["kl"]) for q in P)) == 4 and len(set(len(q["kl"]) + len(q["kr"]) for q in P)) == 4
    seen = {}
    for mode in (1, 2, 0):
        for engine in (0, 2):
            matcher.set_scan_mode(mode); matcher.set_hamming_engine(engine)
            for th in RM.THS:
                res = run_batch(pkg, matcher, P, th)
                ref = oracle_results(oracle, synth, cam, th)
                for p, (q, r, o) in enumerate(zip(P, res, ref)):
                    nl = len(q["kl"])
                    s0 = RM.initial_slots(q)[0]
                    new = (o[1] != s0) & (o[1] >= 0)
                    print("cam %d mode %d engine %d th %g problem %d: nmatches %d (oracle %d), %d left %d right" %
                          (cam, mode, engine, th, p, r[0], o[0], int(new[:nl].sum()), int(new[nl:].sum())))
                    assert r[0] == o[0] and np.array_equal(r[1], o[1]) and np.array_equal(r[2], o[2])
                    check_moq(q, r)
                    assert all(np.array_equal(a, b) for a, b in zip(seen.setdefault((th, p), r), r))
    matcher.set_scan_mode(0); matcher.set_hamming_engine(2)
    for th in RM.THS:                                                 # bMono: the pose of problem 0 gives the neutral window
        r = run_batch(pkg, matcher, P[:1], th, mono=True)[0]
        o = oracle_results(oracle, synth, cam, th, mono=True)[0]
        assert r[0] == o[0] and np.array_equal(r[1], o[1]) and np.array_equal(r[2], o[2])
        assert not np.array_equal(r[1], oracle_results(oracle, synth, cam, th)[0][1])
        check_moq(P[0], r)


def test_batch_equals_per_frame_form(pkg, oracle, synth, matcher):
    """The same four problems through four calls of orbm_search_by_projection_last_frame_fisheye: the same bits, and the batch
    form with constant counts (npairs = 1, no device counts) as well."""
    for cam in (0, 1):
        P = RM.problems(oracle, synth, cam)
        for th in RM.THS:
            res = run_batch(pkg, matcher, P, th)
            for q, r in zip(P, res):
                F = pkg.FrameView(np.concatenate([q["kl"], q["kr"]]), np.concatenate([q["dl"], q["dr"]]), RM.BOUNDS)
                F.slot[:], F.slot_obs[:] = RM.initial_slots(q)
                n = matcher.SearchByProjectionLastFrameFisheye(F, len(q["kl"]), q["sf"], q["has_mp"], q["Xw"], q["d0"], q["k0"], q["Tcw"], q["Tlw"],
                                                               q["Trl"], cam, RM.CAMS[cam], th, bMono=False, mb=RM.MB, mp_obs=q["obs"])
                assert n == r[0] and np.array_equal(F.slot, r[1]) and np.array_equal(F.slot_obs, r[2])
        q = P[2]
        r1 = run_batch(pkg, matcher, [q], RM.THS[0], counts_on_device=False, fs=len(q["kl"]) + len(q["kr"]), ls=len(q["k0"]))[0]
        assert all(np.array_equal(a, b) for a, b in zip(r1, run_batch(pkg, matcher, P, RM.THS[0])[2]))


# ---- hand-placed points ------------------------------------------------------------------------------------------------------------
def px(u, v, z=RM.Z):
    """The point of the left camera (Tcw = I) that Pinhole projects to (u, v)."""
    fx, fy, cx, cy = [float(x) for x in RM.CAMS[0]]
    return [(u - cx) / fx * z, (v - cy) / fy * z, z]


def hand(pkg, sf, left, right, points, Trl, nlevels_octave=None):
    """left / right: [(x, y, octave, angle, descriptor id)], points: [(Xw, octave, angle, descriptor id, obs)]."""
    rng = np.random.default_rng(99)
    bank = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    def keys(rows):
        k = np.zeros(len(rows), pkg.KP_DTYPE)
        for i, r in enumerate(rows):
            k[i]["x"], k[i]["y"], k[i]["octave"], k[i]["angle"], k[i]["size"] = r[0], r[1], r[2], r[3], 31.0
        return k, (bank[[r[4] for r in rows]] if rows else np.zeros((0, 32), np.uint8))
    kl, dl = keys(left)
    kr, dr = keys(right)
    k0 = np.zeros(len(points), pkg.KP_DTYPE)
    for i, pt in enumerate(points):
        k0[i]["octave"], k0[i]["angle"] = pt[1], pt[2]
    return dict(kl=kl, dl=dl, kr=kr, dr=dr, k0=k0, d0=bank[[pt[3] for pt in points]], Xw=np.array([pt[0] for pt in points], np.float32),
                has_mp=np.ones(len(points), np.uint8), obs=np.array([pt[4] for pt in points], np.uint8), Tcw=np.eye(4, dtype=np.float32),
                Tlw=np.eye(4, dtype=np.float32), Trl=Trl, cam=0, sf=sf, pre=np.zeros(0, np.int64), pre_obs=np.zeros(0, np.uint8))


def constructed(pkg, sf):
    """The hand-placed problems (a) .. (f) that share one rig pose, then (c) and (e) with their own calls."""
    fx = float(RM.CAMS[0][0])
    Trl = np.eye(4, dtype=np.float32)
    Trl[0, 3] = 40.0 * RM.Z / fx                                      # the right camera sees a point 40 px further right
    far = (600.0, 400.0, 0, 0.0, 9)                                   # a keypoint no window reaches
    P = {}
    # (a) left projection inside the bounds, nothing in its window; the right projection is on a keypoint with the point's descriptor
    P["a"] = hand(pkg, sf, [far], [(340.0, 200.0, 0, 0.0, 1)], [(px(300, 200), 0, 0.0, 1, 1)], Trl)
    P["a2"] = hand(pkg, sf, [far, (300.0, 200.0, 0, 0.0, 1)], [(340.0, 200.0, 0, 0.0, 1)], [(px(300, 200), 0, 0.0, 1, 1)], Trl)   # with a left keypoint: both
    # (b) left projection outside the bounds, the right one on a keypoint
    P["b"] = hand(pkg, sf, [far], [(20.0, 200.0, 0, 0.0, 1)], [(px(-20, 200), 0, 0.0, 1, 1)], Trl)
    # (d) two points with one descriptor and no observations on one keypoint: the later one holds it, both count
    P["d"] = hand(pkg, sf, [far, (300.0, 200.0, 0, 100.0, 1)], [], [(px(300, 200), 0, 100.0, 1, 0), (px(300, 200), 0, 100.0, 1, 0)], Trl)
    # ... and both are pruned: three fuller bins (3 matches each, rotations 30, 60 and 90 degrees) beside their bin (2 entries)
    fill_l, fill_p = [], []
    for g, ang in enumerate((70.0, 40.0, 10.0)):
        for k in range(3):
            u, v = 100.0 + 60 * k, 60.0 + 40 * g
            fill_l.append((u, v, 0, ang, 10 + 3 * g + k))
            fill_p.append((px(u, v), 0, 100.0, 10 + 3 * g + k, 1))
    P["d2"] = hand(pkg, sf, [far, (300.0, 200.0, 0, 100.0, 1)] + fill_l, [], [(px(300, 200), 0, 100.0, 1, 0)] + fill_p + [(px(300, 200), 0, 100.0, 1, 0)], Trl)
    # (f) Nleft = 0 (every keypoint is a right one: no left window is ever non-empty) and Nleft = N
    P["f0"] = hand(pkg, sf, [], [(340.0, 200.0, 0, 0.0, 1), (300.0, 200.0, 0, 0.0, 1)], [(px(300, 200), 0, 0.0, 1, 1)], Trl)
    P["fN"] = hand(pkg, sf, [(340.0, 200.0, 0, 0.0, 1), (300.0, 200.0, 0, 0.0, 1)], [], [(px(300, 200), 0, 0.0, 1, 1)], Trl)
    # (c) the right camera sees the point at negative depth (finite coordinates): Pinhole projects it all the same, and the reference
    # has no test that would drop it - whatever the oracle gives
    Tneg = np.eye(4, dtype=np.float32)
    Tneg[2, 3] = -6.0                                                 # x3Dr = (0.3, 0.25, -1) -> (cx - 0.3 fx, cy - 0.25 fy)
    fy, cx, cy = float(RM.CAMS[0][1]), float(RM.CAMS[0][2]), float(RM.CAMS[0][3])
    c = hand(pkg, sf, [far, (cx + 0.06 * fx, cy + 0.05 * fy, 0, 0.0, 1)], [(cx - 0.3 * fx, cy - 0.25 * fy, 0, 0.0, 1)], [([0.3, 0.25, 5.0], 0, 0.0, 1, 1)], Tneg)
    # (e) a last point whose octave is nlevels takes no part (the oracle would index its scale factors out of range: not asked)
    e = hand(pkg, sf, [far, (300.0, 200.0, 0, 0.0, 1)], [(340.0, 200.0, 0, 0.0, 1)], [(px(300, 200), len(sf), 0.0, 1, 1), (px(300, 200), 0, 0.0, 1, 1)], Trl)
    return P, c, e


def test_constructed_branches(pkg, oracle, synth, matcher):
    sf = RM.stream(oracle, synth)[3]
    P, c, e = constructed(pkg, sf)
    names = list(P)
    res = dict(zip(names, run_batch(pkg, matcher, [P[k] for k in names], 7.0, mono=True, fs=16, ls=12)))
    for k in names:
        o = RM.oracle_search(oracle, P[k], 7.0, mono=True)
        print(k, "nmatches", res[k][0], "slot", res[k][1].tolist(), "moq", res[k][3].tolist(), "oracle", o[0], o[1].tolist())
        assert res[k][0] == o[0] and np.array_equal(res[k][1], o[1]) and np.array_equal(res[k][2], o[2]), k
        check_moq(P[k], res[k])
    assert res["a"][0] == 0 and (res["a"][1] == -1).all() and (res["a"][3] == -1).all()
    assert res["a2"][0] == 2 and res["a2"][1].tolist() == [-1, 0, 0] and res["a2"][3].tolist() == [1, 2]
    assert res["b"][0] == 0 and (res["b"][1] == -1).all()
    assert res["d"][0] == 2 and res["d"][1].tolist() == [-1, 1] and res["d"][2].tolist() == [0, 0] and res["d"][3].tolist() == [1, -1, 1, -1]
    assert res["d2"][0] == 9 and res["d2"][1][1] == -1 and res["d2"][3][0] == -1 and res["d2"][3][20] == -1 and (res["d2"][1][2:] >= 1).all()
    assert res["f0"][0] == 0 and (res["f0"][1] == -1).all()
    assert res["fN"][0] == 1 and res["fN"][1].tolist() == [-1, 0]
    # (c): nothing is filtered that the reference does not filter - the right match at negative depth is there
    r = run_batch(pkg, matcher, [c], 7.0, mono=True, fs=16, ls=12)[0]
    o = RM.oracle_search(oracle, c, 7.0, mono=True)
    assert r[0] == o[0] and np.array_equal(r[1], o[1]) and np.array_equal(r[2], o[2])
    assert r[0] == 2 and r[3].tolist() == [1, 2]
    # (e): the point with octave = nlevels makes no query, the one behind it matches both images
    r = run_batch(pkg, matcher, [e], 7.0, mono=True, fs=16, ls=12)[0]
    assert r[0] == 2 and r[1].tolist() == [-1, 1, 1] and r[3].tolist() == [-1, -1, 1, 2]


@pytest.mark.parametrize("cam", [0, 1])
def test_chain_from_extraction(pkg, oracle, synth, matcher, cam):
    """Two rig frames: extraction of the left images with lapping area {0, 400} and of the right images with {352, 752}, the
    concatenation and the search on one stream without a synchronisation in between; the oracle gets the downloaded extraction
    outputs, and its result meets the scene conditions of tests/test_rig_abi.py (both images matched, matches pruned)."""
    import torch
    frames, offs, ext, sf = RM.stream(oracle, synth)
    H, W = frames.shape[1:]
    n = len(RM.CHAIN_FRAMES)
    exL, exR = pkg.ORBextractor(**EUROC), pkg.ORBextractor(**EUROC)
    cap = exL.configure(H, W, n)
    assert exR.configure(H, W, n) == cap and 2 * cap <= pkg.FISHEYE_MAX_KEYPOINTS
    k0, d0 = ext[0]
    n0 = len(k0)
    scenes = RM.chain_problems(oracle, synth, cam)                      # map points and poses; the keypoints come from the device below
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        d_L, d_R = t(np.stack([frames[c[0]] for c in RM.CHAIN_FRAMES])), t(np.stack([frames[c[1]] for c in RM.CHAIN_FRAMES]))
        d_Xw, d_Tcw = t(np.stack([S["Xw"] for S in scenes])), t(np.stack([S["Tcw"].reshape(-1) for S in scenes]))
        d_Tlw = t(np.stack([np.eye(4, dtype=np.float32).reshape(-1)] * n))
        d_has, d_md, d_lk = t(np.ones((n, n0), np.uint8)), t(np.stack([d0, d0])), to_dev(np.stack([k0, k0]))
        mk = lambda: (torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda"), torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda"),
                      torch.zeros((n, 2), dtype=torch.int32, device="cuda"))
        (kL, dL, cL), (kR, dR, cR) = mk(), mk()
        d_keys = torch.zeros((n, 2 * cap, 28), dtype=torch.uint8, device="cuda")
        d_desc = torch.zeros((n, 2 * cap, 32), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        d_slot = torch.full((n, 2 * cap), -1, dtype=torch.int32, device="cuda")
        d_sobs = torch.zeros((n, 2 * cap), dtype=torch.uint8, device="cuda")
        d_nm = torch.zeros((n,), dtype=torch.int32, device="cuda")
        st.synchronize()                                                # the inputs are in place; from here on nothing waits
        s = st.cuda_stream
        exL.extract_batch_device(d_L.data_ptr(), H, W, W, H * W, n, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), cap, RM.CHAIN_LAP[0], stream=s)
        exR.extract_batch_device(d_R.data_ptr(), H, W, W, H * W, n, kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap, RM.CHAIN_LAP[1], stream=s)
        assert pkg.rig_concat_batch_device(n, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap,
                                           d_keys.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), stream=s) == 0
        cur = pkg.FrameStruct(2 * cap, d_keys.data_ptr(), d_desc.data_ptr(), None, *[C.c_float(b) for b in RM.BOUNDS])
        last = pkg.LastFrameStruct(n0, d_has.data_ptr(), d_Xw.data_ptr(), d_md.data_ptr(), d_lk.data_ptr(), None, d_Tcw.data_ptr(), d_Tlw.data_ptr())
        Trl = RM.rig_pose(cam, offs)
        matcher.search_by_projection_last_frame_fisheye_batch_device(cur, 2 * cap, d_n.data_ptr(), 2, d_n.data_ptr() + 4, 2, last, n0, None, 0, n, sf, Trl, cam,
                                                                     RM.CAMS[cam], RM.CHAIN_TH, d_slot.data_ptr(), d_sobs.data_ptr(), None, d_nm.data_ptr(),
                                                                     mb=RM.MB, stream=s)
    torch.cuda.synchronize()                                            # the one synchronisation of the chain
    nn, slot, sobs, nm = d_n.cpu().numpy(), d_slot.cpu().numpy(), d_sobs.cpu().numpy(), d_nm.cpu().numpy()
    keys = d_keys.cpu().numpy().reshape(n, 2 * cap * 28).view(pkg.KP_DTYPE).reshape(n, 2 * cap)
    desc = d_desc.cpu().numpy()
    hl, hr = (kL.cpu().numpy(), dL.cpu().numpy(), cL.cpu().numpy()), (kR.cpu().numpy(), dR.cpu().numpy(), cR.cpu().numpy())
    ext_dev = []
    for f in range(n):
        N, nl = int(nn[f, 0]), int(nn[f, 1])
        assert nl == hl[2][f, 0] and N - nl == hr[2][f, 0] and nl > 500 and N - nl > 500
        ext_dev.append((keys[f, :nl], desc[f, :nl], keys[f, nl:N], desc[f, nl:N]))
    P = RM.chain_problems(oracle, synth, cam, ext=ext_dev)
    for f in range(n):
        N, nl = int(nn[f, 0]), int(nn[f, 1])
        assert np.array_equal(keys[f, :N].view(np.uint8).reshape(N, 28), np.concatenate([hl[0][f, :nl], hr[0][f, :N - nl]]))
        assert np.array_equal(desc[f, :N], np.concatenate([hl[1][f, :nl], hr[1][f, :N - nl]]))
        o = RM.oracle_search(oracle, P[f], RM.CHAIN_TH)
        _, left, right, pruned = RM.scene_counts(oracle, P[f], RM.CHAIN_TH)
        print("cam %d frame %d: N %d Nleft %d nmatches %d (oracle %d), %d left %d right %d pruned" % (cam, f, N, nl, nm[f], o[0], left, right, pruned))
        assert nm[f] == o[0] and np.array_equal(slot[f, :N], o[1]) and np.array_equal(sobs[f, :N], o[2])
        assert (slot[f, N:] == -1).all() and left >= 50 and right >= 50 and pruned >= 1
    assert len(set(int(x) for x in nn[:, 1])) == 2                      # the two frames differ in Nleft
    exL.close(); exR.close()


def test_refusals_with_live_buffers(pkg, oracle, synth, matcher):
    """The refusals next to device memory: a refused call raises and leaves every output as it was."""
    import torch
    P = RM.problems(oracle, synth, 0)[:1]
    B = pack(pkg, P)
    D = {k: to_dev(v) for k, v in B.items()}
    d_moq = torch.full((1, 2 * LS), ISENT, dtype=torch.int32, device="cuda")
    d_nm = torch.full((1,), ISENT, dtype=torch.int32, device="cuda")
    before = {k: D[k].clone() for k in ("slot", "sobs")}
    N, nl, n0 = int(B["cnt"][0, 0]), int(B["cnt"][0, 1]), int(B["ln"][0])
    def call(cur=None, last=None, **kw):
        cur = dict(dict(n=N, keys=D["keys"].data_ptr(), desc=D["desc"].data_ptr(), bounds=RM.BOUNDS), **(cur or {}))
        last = dict(dict(n=n0, has=D["has"].data_ptr(), Xw=D["Xw"].data_ptr(), md=D["mpdesc"].data_ptr(), lk=D["lk"].data_ptr(), Tcw=D["Tcw"].data_ptr(),
                         Tlw=D["Tlw"].data_ptr()), **(last or {}))
        cs = pkg.FrameStruct(cur["n"], cur["keys"], cur["desc"], None, *[C.c_float(b) for b in cur["bounds"]])
        ls = pkg.LastFrameStruct(last["n"], last["has"], last["Xw"], last["md"], last["lk"], None, last["Tcw"], last["Tlw"])
        a = dict(frame_stride=FS, d_frame_n=None, frame_n_stride=0, d_n_left=None, n_left_stride=0, last_stride=LS, d_last_n=None, last_n_stride=0, npairs=1,
                 scale_factors=P[0]["sf"], Trl=P[0]["Trl"], cam_type=0, cam_params=RM.CAMS[0], th=7.0, d_slot=D["slot"].data_ptr(),
                 d_slot_obs=D["sobs"].data_ptr(), d_match_of_query=d_moq.data_ptr(), d_nmatches=d_nm.data_ptr(), n_left=nl, mb=RM.MB)
        a.update(kw)
        return matcher.search_by_projection_last_frame_fisheye_batch_device(cs, a.pop("frame_stride"), a.pop("d_frame_n"), a.pop("frame_n_stride"),
                                                                            a.pop("d_n_left"), a.pop("n_left_stride"), ls, a.pop("last_stride"),
                                                                            a.pop("d_last_n"), a.pop("last_n_stride"), a.pop("npairs"), **a)
    bad = [dict(cur=dict(keys=None)), dict(cur=dict(desc=None)), dict(cur=dict(bounds=(0.0, 0.0, 0.0, 480.0))), dict(cur=dict(n=0)), dict(cur=dict(n=FS + 1)),
           dict(last=dict(has=None)), dict(last=dict(Xw=None)), dict(last=dict(md=None)), dict(last=dict(lk=None)), dict(last=dict(Tcw=None)),
           dict(last=dict(Tlw=None)), dict(last=dict(n=0)), dict(last=dict(n=LS + 1)), dict(Trl=None), dict(n_left=-1), dict(n_left=N + 1), dict(npairs=-1),
           dict(cam_type=2), dict(scale_factors=np.ones(17, np.float32)), dict(d_slot=None), dict(d_slot_obs=None), dict(d_nmatches=None),
           dict(frame_stride=pkg.FISHEYE_MAX_KEYPOINTS + 1, d_frame_n=D["cnt"].data_ptr(), frame_n_stride=2)]
    for c in bad:
        with pytest.raises(ValueError):
            call(**c)
    with pytest.raises(ValueError):                                     # the library's own refusal, past the mirror's checks
        rc = matcher.L.orbm_search_by_projection_last_frame_fisheye_batch_device(matcher.m, None, FS, None, 0, None, 0, nl, None, LS, None, 0, 1, None, 8, None,
                                                                                 0, None, C.c_float(0), C.c_float(7), 0, 1, None, None, None, None, None)
        matcher._check(rc, "orbm_search_by_projection_last_frame_fisheye_batch_device")
    assert call(npairs=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(D["slot"], before["slot"]) and torch.equal(D["sobs"], before["sobs"])
    assert (d_moq.cpu().numpy() == ISENT).all() and (d_nm.cpu().numpy() == ISENT).all()
    # the concatenation
    cap = 8
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")
    k, d, c = z(2, cap, 28), z(2, cap, 32), torch.zeros((2, 2), dtype=torch.int32, device="cuda")
    ok, od, on = torch.full((2, 2 * cap, 28), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((2, 2 * cap, 32), 0x5A, dtype=torch.uint8, device="cuda"), \
        torch.full((2, 2), ISENT, dtype=torch.int32, device="cuda")
    good = dict(nframes=2, d_keysL=k.data_ptr(), d_descL=d.data_ptr(), d_countsL=c.data_ptr(), d_keysR=k.data_ptr(), d_descR=d.data_ptr(), d_countsR=c.data_ptr(),
                cap=cap, d_keys=ok.data_ptr(), d_desc=od.data_ptr(), d_n=on.data_ptr())
    for c_ in [dict(nframes=-1), dict(cap=0), dict(cap=pkg.FISHEYE_MAX_KEYPOINTS // 2 + 1), dict(d_keysL=0), dict(d_descR=0), dict(d_countsL=0), dict(d_keys=0),
               dict(d_desc=0), dict(d_n=0)]:
        with pytest.raises(ValueError):
            pkg.rig_concat_batch_device(**dict(good, **c_))
    assert pkg.rig_concat_batch_device(**dict(good, nframes=0)) == 0
    torch.cuda.synchronize()
    assert (ok.cpu().numpy() == 0xA5).all() and (od.cpu().numpy() == 0x5A).all() and (on.cpu().numpy() == ISENT).all()
