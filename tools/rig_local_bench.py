"""The local-map search of a two-camera fisheye rig on resident batches (orbm_search_local_points_fisheye_batch_device) against 256
calls of the per-frame form, against the monocular batch form at the same counts, and inside the chained rig step.

256 synthetic rig frames as tools/rig_bench.py builds them (TUM-VI 512 x 512 settings: 1500 features per camera, KannalaBrandt8;
the left image is the last frame's image shifted by (3, -2) px, the right image the left one shifted by (4, 0) px), extracted once and
resident in HBM.  The local map of a problem has --map points (3000, the size tools/local_points_bench.py uses): the last frame's
keypoints un-projected through the camera model at z = 5 from the pixel where they appear in the left image, filled up with random
points in and around the view (random descriptors); mfMaxDistance / normals / eligibility / observations drawn as
synth.make_local_map_scene draws them; 45 % of the keypoints have a stereo partner.  The right camera is the translation that gives
the right image's shift at z = 5, turned by 2 mrad, with focal lengths 0.2 % off the left camera's.  Legs, alternated over --rounds:

  (a) orbm_search_local_points_fisheye_batch_device for all frames (with the reset of the slots), HIP-event time per batch;
      (a0) the same with obs = NULL, i.e. without the serial claim loop that partner tables + observations select;
  (b) 256 calls of orbm_search_local_points_fisheye on the same data held on the host, wall time;
  (c) orbm_search_local_points_batch_device (monocular form) over the same concatenated frames and the same maps: the yardstick
      for what the second camera costs;
  (d) extract left, extract right, concatenate, last-frame search, on one stream - without and with the new call behind it.

After the timing the outputs of (a) and (b) are compared for all frames.  Exit status 1 if they differ.  Prints text lines and one
JSON line and writes them to --out.  --one-call: set up, run the batch call twice and leave (for a kernel trace).  Needs a GPU.

    python tools/rig_local_bench.py [--frames 256] [--map 3000] [--rounds 5] [--window 0.25] [--out profiles/rig_local_bench.txt]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TUMVI = dict(nfeatures=1500, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7)   # Examples/Stereo/TUM_VI_512.yaml
CAM = np.array([190.978477, 190.973307, 254.931706, 256.897442, 0.003482389402, 0.000715034845, -0.002053236141, 0.000202936736], np.float32)
Z, MB, TH_LAST, TH = 5.0, 0.11, 7.0, 3.0
SHIFT_L, SHIFT_R = (3, -2), (4, 0)      # last -> left, left -> right, in pixels
MONO_FIELDS = ("in_view", "proj_x", "proj_y", "proj_xr", "depth", "view_cos", "level")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--map", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of timed work per leg and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--one-call", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_local_bench.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rig_local_bench: no GPU (there is no fallback)")
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    synth = importlib.import_module("3_orb_slam3_selfnote_amd.synth")
    P, H, W, M, NMP = a.frames, 512, 512, 16, a.map
    canv = [synth.make_frame(9100 + c, H + 2 * M, W + 2 * M) for c in range(min(32, P))]
    offs = [(2 * k, 14 - 2 * k) for k in range(8)]
    def crop(p, dx, dy):
        ox, oy = M // 2 + offs[(p // 32) % 8][0] + dx, M // 2 + offs[(p // 32) % 8][1] + dy
        return canv[p % 32][oy:oy + H, ox:ox + W]
    img_last = np.stack([crop(p, 0, 0) for p in range(P)])
    img_l = np.stack([crop(p, -SHIFT_L[0], -SHIFT_L[1]) for p in range(P)])
    img_r = np.stack([crop(p, -SHIFT_L[0] - SHIFT_R[0], -SHIFT_L[1] - SHIFT_R[1]) for p in range(P)])
    dev = torch.device("cuda", 0)
    exL, exR, exP = pkg.ORBextractor(**TUMVI), pkg.ORBextractor(**TUMVI), pkg.ORBextractor(**TUMVI)
    m = pkg.ORBmatcher(0.8, True)
    cap = exL.configure(H, W, P)
    assert exR.configure(H, W, P) == cap and exP.configure(H, W, P) == cap and NMP >= cap
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_il, d_ir, d_ip = t(img_l), t(img_r), t(img_last)
    mk = lambda n: (torch.zeros((P, n, 28), dtype=torch.uint8, device=dev), torch.zeros((P, n, 32), dtype=torch.uint8, device=dev),
                    torch.zeros((P, 2), dtype=torch.int32, device=dev))
    (kL, dL, cL), (kR, dR, cR), (kP, dP, cP), (kC, dC, cC) = mk(cap), mk(cap), mk(cap), mk(2 * cap)
    s = torch.cuda.current_stream().cuda_stream
    sf = exL.GetScaleFactors()
    log_sf = float(pkg.load().orbx_ref_logf(1.2))            # Frame::mfLogScaleFactor = log(1.2f), glibc logf
    bounds = (0.0, float(W), 0.0, float(H))
    ang = 0.002
    Trl = np.eye(4)
    Trl[:2, :2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]
    Trl[:3, 3] = [SHIFT_R[0] * Z / CAM[0], SHIFT_R[1] * Z / CAM[1], 0.0]
    tlr = (-(Trl[:3, :3].T @ Trl[:3, 3])).astype(np.float32)
    Trl = Trl.astype(np.float32)
    CAM2 = CAM.copy()
    CAM2[:2] = (CAM[:2].astype(np.float64) * 1.002).astype(np.float32)

    def extract_lr():
        exL.extract_batch_device(d_il.data_ptr(), H, W, W, H * W, P, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), cap, (0, 400), stream=s)
        exR.extract_batch_device(d_ir.data_ptr(), H, W, W, H * W, P, kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap, (112, 512), stream=s)

    def concat():
        pkg.rig_concat_batch_device(P, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap, kC.data_ptr(), dC.data_ptr(),
                                    cC.data_ptr(), stream=s)

    exP.extract_batch_device(d_ip.data_ptr(), H, W, W, H * W, P, kP.data_ptr(), dP.data_ptr(), cP.data_ptr(), cap, (0, 0), stream=s)
    extract_lr()
    concat()
    torch.cuda.synchronize()
    h_kP = kP.cpu().numpy().reshape(P, cap * 28).view(pkg.KP_DTYPE).reshape(P, cap)
    h_dP, h_cP = dP.cpu().numpy(), cP.cpu().numpy()[:, 0].copy()
    h_cC = cC.cpu().numpy()
    # the local maps
    rng = np.random.default_rng(77)
    sfd = np.asarray(sf, np.float64)
    Xw, desc = np.zeros((P, NMP, 3), np.float32), rng.integers(0, 256, (P, NMP, 32), dtype=np.uint8)
    octv = rng.integers(0, 8, (P, NMP))
    has = np.zeros((P, cap), np.uint8)
    Xw_last = np.zeros((P, cap, 3), np.float32)
    for p in range(P):
        n = int(h_cP[p])
        rays = synth.kb8_unproject(CAM, h_kP["x"][p, :n].astype(np.float64) + SHIFT_L[0], h_kP["y"][p, :n].astype(np.float64) + SHIFT_L[1])
        Xw_last[p, :n] = (rays * (Z / rays[:, 2:3])).astype(np.float32)
        has[p, :n] = 1
        ne = NMP - n
        Xe = synth.kb8_unproject(CAM, rng.uniform(-60, W + 60, ne), rng.uniform(-60, H + 60, ne)) * rng.uniform(0.5, 12.0, ne)[:, None]
        Xe[rng.random(ne) < 0.05, 2] *= -1
        perm = rng.permutation(NMP)                          # local-map order mixes both kinds (claims are sequential)
        Xw[p] = np.concatenate([Xw_last[p, :n], Xe.astype(np.float32)])[perm]
        desc[p, :n] = h_dP[p, :n]
        desc[p] = desc[p][perm]
        octv[p, :n] = h_kP["octave"][p, :n]
        octv[p] = octv[p][perm]
    dist = np.linalg.norm(Xw.astype(np.float64), axis=2)     # Tcw = I: the camera centre is the origin
    maxd = dist * sfd[octv] * rng.uniform(0.93, 1.02, (P, NMP))
    gate = rng.random((P, NMP))
    maxd[gate < 0.03] *= 0.6
    mind = maxd / sfd[-1]
    near = (gate >= 0.03) & (gate < 0.06)
    mind[near] = dist[near] * 1.5
    dirn = Xw.astype(np.float64) / np.maximum(dist, 1e-9)[..., None]
    tilt = np.where(rng.random((P, NMP)) < 0.25, rng.uniform(0, 1.4, (P, NMP)), rng.uniform(0, 0.08, (P, NMP)))
    perp = np.cross(dirn, rng.normal(size=(P, NMP, 3)))
    perp /= np.linalg.norm(perp, axis=2)[..., None]
    normal = (dirn * np.cos(tilt)[..., None] + perp * np.sin(tilt)[..., None]).astype(np.float32)
    elig, obs = (rng.random((P, NMP)) < 0.9).astype(np.uint8), (rng.random((P, NMP)) < 0.9).astype(np.uint8)
    maxd, mind = maxd.astype(np.float32), mind.astype(np.float32)
    l2r, r2l = np.full((P, 2 * cap), -1, np.int32), np.full((P, 2 * cap), -1, np.int32)
    for p in range(P):
        nl, nr = int(h_cC[p, 1]), int(h_cC[p, 0] - h_cC[p, 1])
        k = int(0.45 * min(nl, nr))
        pl, pr = rng.permutation(nl)[:k], rng.permutation(nr)[:k]
        l2r[p, pl], r2l[p, pr] = pr, pl
    I4 = np.eye(4, dtype=np.float32)
    D = dict(elig=t(elig), Xw=t(Xw), normal=t(normal), maxd=t(maxd), mind=t(mind), desc=t(desc), obs=t(obs), l2r=t(l2r), r2l=t(r2l))
    eye = torch.eye(4, device=dev).reshape(1, 16).repeat(P, 1).contiguous()
    d_Xwl, d_has = t(Xw_last), t(has)
    d_slot = torch.full((P, 2 * cap), -1, dtype=torch.int32, device=dev)
    d_sobs = torch.zeros((P, 2 * cap), dtype=torch.uint8, device=dev)
    d_nm, d_nm2 = torch.zeros((P,), dtype=torch.int32, device=dev), torch.zeros((P,), dtype=torch.int32, device=dev)
    tt = lambda k: torch.uint8 if k.startswith("in_view") else torch.int32 if k.startswith("level") else torch.float32
    tr = {k: torch.zeros((P, NMP), dtype=tt(k), device=dev) for k, _ in pkg.TRACK_RIG_FIELDS}
    cur = pkg.FrameStruct(2 * cap, kC.data_ptr(), dC.data_ptr(), None, *[C.c_float(b) for b in bounds])
    last = pkg.LastFrameStruct(cap, d_has.data_ptr(), d_Xwl.data_ptr(), dP.data_ptr(), kP.data_ptr(), None, eye.data_ptr(), eye.data_ptr())
    mapS = lambda with_obs: pkg.LocalMapStruct(NMP, D["elig"].data_ptr(), D["Xw"].data_ptr(), D["normal"].data_ptr(), D["maxd"].data_ptr(), D["mind"].data_ptr(),
                                               D["desc"].data_ptr(), D["obs"].data_ptr() if with_obs else None, eye.data_ptr())
    map1, map0 = mapS(True), mapS(False)
    ts = pkg.TrackRigStruct(*[tr[k].data_ptr() for k, _ in pkg.TRACK_RIG_FIELDS])
    tsm = pkg.TrackStruct(*[tr[k].data_ptr() for k in MONO_FIELDS])

    def rig_local(mp=map1, reset=True):
        if reset:
            d_slot.fill_(-1); d_sobs.zero_()
        m.search_local_points_fisheye_batch_device(cur, 2 * cap, cC.data_ptr(), 2, cC.data_ptr() + 4, 2, D["l2r"].data_ptr(), D["r2l"].data_ptr(), mp, NMP, None, 0, P,
                                                   sf, log_sf, Trl, tlr, 1, CAM, 1, CAM2, TH, d_slot.data_ptr(), d_sobs.data_ptr(), None, ts, d_nm.data_ptr(), stream=s)

    def rig_local_noobs():
        rig_local(map0)

    def mono_local():
        d_slot.fill_(-1); d_sobs.zero_()
        m.search_local_points_batch_device(cur, 2 * cap, cC.data_ptr(), 2, map1, NMP, None, 0, P, sf, log_sf, 1, CAM, TH, d_slot.data_ptr(), d_sobs.data_ptr(), None,
                                           tsm, d_nm2.data_ptr(), stream=s)

    def chain(with_local):
        extract_lr()
        concat()
        d_slot.fill_(-1); d_sobs.zero_()
        m.search_by_projection_last_frame_fisheye_batch_device(cur, 2 * cap, cC.data_ptr(), 2, cC.data_ptr() + 4, 2, last, cap, cP.data_ptr(), 2, P, sf, Trl, 1, CAM,
                                                               TH_LAST, d_slot.data_ptr(), d_sobs.data_ptr(), None, d_nm2.data_ptr(), mb=MB, stream=s)
        if with_local:
            rig_local(reset=False)

    chain0, chain1 = (lambda: chain(False)), (lambda: chain(True))
    if a.one_call:
        rig_local(); rig_local()
        torch.cuda.synchronize()
        print("rig_local_bench --one-call: %d frames, two batch calls" % P)
        m.close(); exL.close(); exR.close(); exP.close()
        return 0

    # (b): the same data on the host
    h_kC = kC.cpu().numpy().reshape(P, 2 * cap * 28).view(pkg.KP_DTYPE).reshape(P, 2 * cap)
    h_dC = dC.cpu().numpy()
    views = []
    for p in range(P):
        N, nl = int(h_cC[p, 0]), int(h_cC[p, 1])
        views.append((pkg.FrameView(h_kC[p, :N], h_dC[p, :N], bounds), nl, l2r[p, :nl].copy(), r2l[p, :N - nl].copy()))
    out_b = [None] * P
    trh = {k: np.zeros(NMP, ty) for k, ty in pkg.TRACK_RIG_FIELDS}

    def per_frame():
        for p, (F, nl, a_, b_) in enumerate(views):
            F.slot[:] = -1; F.slot_obs[:] = 0
            out_b[p] = m.SearchLocalPointsFisheye(F, nl, a_, b_, sf, log_sf, elig[p], Xw[p], normal[p], maxd[p], mind[p], desc[p], I4, Trl, tlr, 1, CAM, 1, CAM2, TH,
                                                  mp_obs=obs[p], track=trh)[0]

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, (time.perf_counter() - t0) * 1e3 / reps

    legs = dict(a=rig_local, a0=rig_local_noobs, c=mono_local, d0=chain0, d1=chain1)
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    per_frame()
    est = {k: timed(fn, 2)[0] for k, fn in legs.items()}
    est["b"] = timed(per_frame, 1)[1]
    reps = {k: max(2 if k != "b" else 1, int(a.window * 1e3 / max(v, 1e-3)) + 1) for k, v in est.items()}
    T = {k: [] for k in est}
    for r in range(a.rounds):
        for k, fn in legs.items():
            T[k].append(timed(fn, reps[k])[0])
        T["b"].append(timed(per_frame, reps["b"])[1])
    T = {k: np.array(v) for k, v in T.items()}
    mono_local()
    torch.cuda.synchronize()
    nm_mono = d_nm2.cpu().numpy().copy()
    rig_local()
    torch.cuda.synchronize()
    slot, sobs, nm = d_slot.cpu().numpy(), d_sobs.cpu().numpy(), d_nm.cpu().numpy()
    per_frame()
    differing, left, right = 0, 0, 0
    for p, (F, nl, *_) in enumerate(views):
        N = F.N
        differing += not (out_b[p] == nm[p] and np.array_equal(F.slot, slot[p, :N]) and np.array_equal(F.slot_obs, sobs[p, :N]))
        left += int((slot[p, :nl] >= 0).sum()); right += int((slot[p, nl:N] >= 0).sum())
    spread = lambda x: "mean %.4f, min %.4f, max %.4f" % (x.mean(), x.min(), x.max())
    rnd = lambda x, k=4: round(float(x), k)
    res = dict(frames=P, keypoints_per_rig_frame=float(h_cC[:, 0].mean()), left_per_frame=float(h_cC[:, 1].mean()), map_points=NMP, frame_stride=2 * cap, th=TH,
               rounds=a.rounds, reps=reps, outputs_identical=differing == 0, frames_differing=int(differing), matches_per_frame=float(nm.mean()),
               left_slots_per_frame=left / P, right_slots_per_frame=right / P, mono_matches_per_frame=float(nm_mono.mean()),
               chain_rig_frames_per_s_without=rnd(P / T["d0"].mean() * 1e3, 1), chain_rig_frames_per_s_with=rnd(P / T["d1"].mean() * 1e3, 1),
               device=torch.cuda.get_device_name(0))
    names = dict(a="batch_ms", a0="batch_no_obs_ms", b="per_frame_wall_ms", c="mono_same_counts_ms", d0="chain_without_ms", d1="chain_with_ms")
    for k, nme in names.items():
        res[nme], res[nme + "_min"], res[nme + "_max"] = rnd(T[k].mean()), rnd(T[k].min()), rnd(T[k].max())
    res["a_against_b"], res["a_against_c"] = rnd(T["b"].mean() / T["a"].mean(), 1), rnd(T["a"].mean() / T["c"].mean(), 2)
    lines = ["(a) orbm_search_local_points_fisheye_batch_device, %d rig frames, %.0f keypoints per frame (%.0f left), %d local map points, frame stride %d, th %g: %s ms per batch (%d rounds x %d)"
             % (P, h_cC[:, 0].mean(), h_cC[:, 1].mean(), NMP, 2 * cap, TH, spread(T["a"]), a.rounds, reps["a"]),
             "(a0) the same with obs = NULL (no serial claim loop): %s ms per batch" % spread(T["a0"]),
             "(b) %d calls of orbm_search_local_points_fisheye on the same data: %s ms wall (%d rounds x %d)" % (P, spread(T["b"]), a.rounds, reps["b"]),
             "(c) orbm_search_local_points_batch_device (monocular) over the same concatenated frames and maps: %s ms per batch; %.0f matches per frame"
             % (spread(T["c"]), nm_mono.mean()),
             "(a) against (b): %.1f x faster; (a) against (c): %.2f x the monocular form's time" % (T["b"].mean() / T["a"].mean(), T["a"].mean() / T["c"].mean()),
             "(d) extract left + extract right + concat + last-frame search, one stream: %s ms per %d rig frames = %.0f rig frames/s"
             % (spread(T["d0"]), P, P / T["d0"].mean() * 1e3),
             "    ... + the local-map search behind it: %s ms = %.0f rig frames/s; %.0f matches per frame in (a) (%.0f left slots, %.0f right slots)"
             % (spread(T["d1"]), P / T["d1"].mean() * 1e3, nm.mean(), left / P, right / P),
             "outputs of (a) and (b): %s" % ("identical for all %d frames" % P if differing == 0 else "%d frames DIFFER" % differing),
             json.dumps(res)]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    m.close(); exL.close(); exR.close(); exP.close()
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
