"""The fisheye-rig chain with Frame::ComputeStereoFishEyeMatches on the device: two extractions, orbm_rig_concat_batch_device,
orbm_stereo_fisheye_matches_batch_device, orbm_search_local_points_fisheye_batch_device fed the produced partner tables and
orbx_close_points_batch_device fed the produced mvDepth, on one stream without a synchronisation in between.  The tables are compared
with tests/rig_stereo_model.py on the downloaded extractions, the search with tests/rig_local_model.py + the oracle fed the MODEL's
tables, the close points with tests/rgbd_model.py on the model's depths."""
import ctypes as C

import numpy as np
import pytest

import local_map_model as LM
import rgbd_model
import rig_local_model as RL
import rig_stereo_model as M
from conftest import TUMVI
from test_gpu_rig_local import ISENT, check_result, poison_track

pytestmark = pytest.mark.gpu
f32 = np.float32
H = W = 512
Z = 5.0                       # depth of the scene plane: the rig's baseline turns the shift between the two images into this depth
SEED = 4100
RIG_FRAMES = ((1, 2), (0, 1))  # (left, right) stream frames of the two rig frames; the rig is built for the first
LAP = ((64, 511), (0, 447))
FSENT = -777.25


def test_chain_from_extraction(pkg, oracle, synth):
    import torch
    frames, offs = synth.make_stream(SEED, 3, H=H, W=W)
    shift = (offs[1] - offs[2]).astype(np.float64)                  # a scene point at (x, y) on the left is at (x, y) + shift on the right
    assert np.abs(shift).sum() >= 4
    cam = M.CAM1                                                    # both cameras: a pure shift is then what a translated camera sees
    t = np.array([shift[0] * Z / cam[0], shift[1] * Z / cam[1], 0.0])
    Trl, Tlr = np.eye(4, dtype=f32), np.eye(4, dtype=f32)[:3]
    Trl[:3, 3], Tlr[:3, 3] = t, -t
    tlr = np.ascontiguousarray(Tlr[:3, 3])
    n = len(RIG_FRAMES)
    exL, exR = pkg.ORBextractor(**TUMVI), pkg.ORBextractor(**TUMVI)
    cap = exL.configure(H, W, n)
    assert exR.configure(H, W, n) == cap and 2 * cap <= min(pkg.FISHEYE_MAX_KEYPOINTS, pkg.CLOSE_MAX_KEYPOINTS)
    # the local map: the oracle's keypoints of the first left image inside the 90-degree cone, on the plane z = Z, seen from Tcw = I
    oex = oracle.OracleExtractor(**TUMVI)
    sf = np.asarray(oex.scale_factors, f32)
    _, k0, d0 = oex.extract(frames[RIG_FRAMES[0][0]])
    near = np.hypot(k0["x"] - cam[2], k0["y"] - cam[3]) < 240
    k0, d0 = k0[near], d0[near]
    rays = synth.kb8_unproject(cam, k0["x"].astype(np.float64), k0["y"].astype(np.float64))
    Xw = np.ascontiguousarray((rays * (Z / rays[:, 2:3])).astype(f32))
    nmp = len(Xw)
    dist = np.linalg.norm(Xw.astype(np.float64), axis=1)
    maxd = (dist * sf[k0["octave"]]).astype(f32)
    base = dict(sf=sf, log_sf=float(LM.glibc_logf(f32(1.2))), bounds=(0.0, float(W), 0.0, float(H)), cam=1, cam_params=cam, cam2=1, cam_params2=cam, Trl=Trl,
                tlr=tlr, Tcw=np.eye(4, dtype=f32), Xw=Xw, desc=np.ascontiguousarray(d0), normal=np.ascontiguousarray((Xw / dist[:, None]).astype(f32)),
                max_dist=maxd, min_dist=(maxd / sf[-1]).astype(f32), eligible=np.ones(nmp, np.uint8), obs=np.ones(nmp, np.uint8))
    sigma2 = (sf * sf).astype(f32)                                  # mvLevelSigma2 (ORBextractor.cc:420)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        rep = lambda a: t_(np.stack([a] * n))
        d_L, d_R = t_(np.stack([frames[c[0]] for c in RIG_FRAMES])), t_(np.stack([frames[c[1]] for c in RIG_FRAMES]))
        D = dict(elig=rep(base["eligible"]), Xw=rep(base["Xw"]), normal=rep(base["normal"]), maxd=rep(base["max_dist"]), mind=rep(base["min_dist"]),
                 mpdesc=rep(base["desc"]), obs=rep(base["obs"]), Tcw=rep(base["Tcw"].reshape(-1)))
        for k, _ in RL.FIELDS:
            D["t_" + k] = rep(poison_track(nmp)[k])
        mk = lambda: (torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda"), torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda"),
                      torch.zeros((n, 2), dtype=torch.int32, device="cuda"))
        (kL, dL, cL), (kR, dR, cR) = mk(), mk()
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
        d_keys, d_desc = full((n, 2 * cap, 28), 0, torch.uint8), full((n, 2 * cap, 32), 0, torch.uint8)
        d_n = full((n, 2), 0, torch.int32)
        d_l2r, d_r2l = full((n, 2 * cap), ISENT, torch.int32), full((n, 2 * cap), ISENT, torch.int32)
        d_depth, d_p3d = full((n, 2 * cap), FSENT, torch.float32), full((n, 2 * cap, 3), FSENT, torch.float32)
        d_snm = full((n, 2), ISENT, torch.int32)
        d_slot, d_sobs = full((n, 2 * cap), -1, torch.int32), full((n, 2 * cap), 0, torch.uint8)
        d_mop, d_nm = full((n, 2 * nmp), ISENT, torch.int32), full((n,), 0, torch.int32)
        d_order, d_nvisit = full((n, 2 * cap), ISENT, torch.int32), full((n,), ISENT, torch.int32)
        st.synchronize()                                                # the inputs are in place; from here on nothing waits
        s = st.cuda_stream
        matcher = pkg.ORBmatcher(RL.NNRATIO, True)
        exL.extract_batch_device(d_L.data_ptr(), H, W, W, H * W, n, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), cap, LAP[0], stream=s)
        exR.extract_batch_device(d_R.data_ptr(), H, W, W, H * W, n, kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap, LAP[1], stream=s)
        ins = [a.data_ptr() for a in (kL, dL, cL, kR, dR, cR)]
        assert pkg.rig_concat_batch_device(n, *ins, cap, d_keys.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), stream=s) == 0
        matcher.stereo_fisheye_matches_batch_device(n, *ins, cap, sigma2, Tlr, cam, cam, 2 * cap, d_l2r.data_ptr(), d_r2l.data_ptr(), d_depth.data_ptr(),
                                                    d_p3d.data_ptr(), d_snm.data_ptr(), stream=s)
        cur = pkg.FrameStruct(2 * cap, d_keys.data_ptr(), d_desc.data_ptr(), None, *[C.c_float(b) for b in base["bounds"]])
        mp = pkg.LocalMapStruct(nmp, D["elig"].data_ptr(), D["Xw"].data_ptr(), D["normal"].data_ptr(), D["maxd"].data_ptr(), D["mind"].data_ptr(),
                                D["mpdesc"].data_ptr(), D["obs"].data_ptr(), D["Tcw"].data_ptr())
        ts = pkg.TrackRigStruct(*[D["t_" + k].data_ptr() for k, _ in RL.FIELDS])
        matcher.search_local_points_fisheye_batch_device(cur, 2 * cap, d_n.data_ptr(), 2, d_n.data_ptr() + 4, 2, d_l2r.data_ptr(), d_r2l.data_ptr(), mp, nmp,
                                                         None, 0, n, sf, base["log_sf"], Trl, tlr, 1, cam, 1, cam, 4.0, d_slot.data_ptr(), d_sobs.data_ptr(),
                                                         d_mop.data_ptr(), ts, d_nm.data_ptr(), stream=s)
        pkg.close_points_batch_device(n, d_depth.data_ptr(), d_n.data_ptr() + 4, 2, 2 * cap, 3.0, 100, d_order.data_ptr(), d_nvisit.data_ptr(), stream=s)
    torch.cuda.synchronize()                                            # the one synchronisation of the chain
    g = lambda a: a.cpu().numpy()
    nn, slot, sobs, nm, mop, snm = g(d_n), g(d_slot), g(d_sobs), g(d_nm), g(d_mop), g(d_snm)
    l2r, r2l, depth, p3d, order, nvisit = g(d_l2r), g(d_r2l), g(d_depth), g(d_p3d), g(d_order), g(d_nvisit)
    keys = g(d_keys).reshape(n, 2 * cap * 28).view(pkg.KP_DTYPE).reshape(n, 2 * cap)
    desc, monoL, monoR = g(d_desc), g(cL)[:, 1], g(cR)[:, 1]
    for f in range(n):
        N, nl = int(nn[f, 0]), int(nn[f, 1])
        nr = N - nl
        assert nl > 500 and nr > 500
        kl, dl, kr, dr = keys[f, :nl], desc[f, :nl], keys[f, nl:N], desc[f, nl:N]
        E = M.stereo_fisheye_matches(kl, dl, int(monoL[f]), kr, dr, int(monoR[f]), sigma2, Tlr, cam, cam, p3d=np.full((nl, 3), FSENT, f32))
        print("rig frame %d: Nleft %d (mono %d) Nright %d (mono %d): nMatches %d, descMatches %d" % (f, nl, monoL[f], nr, monoR[f], E[4][0], E[4][1]))
        assert np.array_equal(l2r[f, :nl], E[0]) and (l2r[f, nl:] == ISENT).all()
        assert np.array_equal(r2l[f, :nr], E[1]) and (r2l[f, nr:] == ISENT).all()
        assert depth[f, :nl].view(np.uint32).tolist() == E[2].view(np.uint32).tolist() and (depth[f, nl:] == f32(FSENT)).all()
        assert np.array_equal(p3d[f, :nl].view(np.uint32), E[3].view(np.uint32)) and (p3d[f, nl:] == f32(FSENT)).all()
        assert tuple(snm[f]) == E[4]
        if f == 0:
            # The rig was built for this frame, so it triangulates.  A constant pixel shift is what the translated camera sees of the
            # plane z = Z only next to the principal point: at the angle theta off the axis the shift of that plane shrinks like
            # cos^2(theta), so the constant shift puts the point at about Z cos^2(theta).  Within 60 px (theta < 0.32) that is above 0.9 Z.
            central = (E[2] > 0) & (np.hypot(kl["x"] - cam[2], kl["y"] - cam[3]) < 60)
            assert E[4][0] >= 50 and central.sum() >= 20 and 0.85 * Z < float(np.median(E[2][central])) < 1.05 * Z
        S = dict(base, kl=kl, dl=dl, kr=kr, dr=dr, l2r=E[0], r2l=E[1], slot0=np.full(N, -1, np.int32), sobs0=np.zeros(N, np.uint8))
        X = RL.expected(oracle, S, 4.0)
        r = dict(n=int(nm[f]), mop=mop[f], track={k: g(D["t_" + k])[f] for k, _ in RL.FIELDS}, slot=slot[f, :N], slot_obs=sobs[f, :N])
        print("    local-map search: nmatches %d (model + oracle %d)" % (nm[f], X["n"]))
        check_result(r, X)
        want, _, _ = rgbd_model.close_points(E[2], 3.0, 100)
        assert int(nvisit[f]) == len(want) and order[f, :len(want)].tolist() == want and (order[f, len(want):] == ISENT).all()
    matcher.close(); exL.close(); exR.close()
