"""The last-frame search of a two-camera fisheye rig on resident batches (orbm_rig_concat_batch_device,
orbm_search_by_projection_last_frame_fisheye_batch_device) against 256 calls of the per-frame form, and the whole rig step on one
stream.

256 synthetic rig pairs (TUM-VI 512 x 512 settings: 1500 features, KannalaBrandt8; images cut from 32 synthetic canvases at 8
offsets; the left image is the last frame's image shifted by (3, -2) px, the right image the left one shifted by (4, 0) px) are
extracted once and stay in HBM.  The map points of a problem are the last frame's keypoints, un-projected through the camera
model at z = 5 from the pixel where they appear in the left image; the right camera is the translation that gives the right
image's shift at that depth.  Legs, alternated over --rounds:

  (a) orbm_search_by_projection_last_frame_fisheye_batch_device for all pairs (with the reset of the slots), HIP-event time per batch;
      the concatenation alone is timed as well;
  (b) 256 calls of orbm_search_by_projection_last_frame_fisheye on the same data held on the host, wall time;
  (m) for information: orbm_search_by_projection_last_frame_batch_device (monocular form) over the same concatenated frames, i.e.
      at the same total keypoint count, one query per point instead of two;
  (c) extract left (lapping area {0, 400}), extract right ({112, 512}), concatenate, search, on one stream, as rig frames/s.

After the timing the outputs of (a) and (b) are compared for all pairs.  Exit status 1 if they differ.  Prints text lines and one
JSON line and writes them to --out.  Needs a GPU; there is no fallback.

    python tools/rig_bench.py [--frames 256] [--rounds 5] [--window 0.25] [--out profiles/rig_batch_bench.txt]
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
Z, MB, TH = 5.0, 0.11, 7.0
SHIFT_L, SHIFT_R = (3, -2), (4, 0)      # last -> left, left -> right, in pixels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of timed work per leg and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_batch_bench.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rig_bench: no GPU (there is no fallback)")
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    synth = importlib.import_module("3_orb_slam3_selfnote_amd.synth")
    P, H, W, M = a.frames, 512, 512, 16
    canv = [synth.make_frame(9100 + c, H + 2 * M, W + 2 * M) for c in range(min(32, P))]
    offs = [(2 * k, 14 - 2 * k) for k in range(8)]
    def crop(p, dx, dy):
        ox, oy = M // 2 + offs[(p // 32) % 8][0] + dx, M // 2 + offs[(p // 32) % 8][1] + dy
        return canv[p % 32][oy:oy + H, ox:ox + W]
    # a scene point at (x, y) of the crop at offset o is at (x - d, y - d') of the crop at offset o + (d, d')
    img_last = np.stack([crop(p, 0, 0) for p in range(P)])
    img_l = np.stack([crop(p, -SHIFT_L[0], -SHIFT_L[1]) for p in range(P)])
    img_r = np.stack([crop(p, -SHIFT_L[0] - SHIFT_R[0], -SHIFT_L[1] - SHIFT_R[1]) for p in range(P)])
    dev = torch.device("cuda", 0)
    exL, exR, exP = pkg.ORBextractor(**TUMVI), pkg.ORBextractor(**TUMVI), pkg.ORBextractor(**TUMVI)
    m = pkg.ORBmatcher(0.9, True)
    cap = exL.configure(H, W, P)
    assert exR.configure(H, W, P) == cap and exP.configure(H, W, P) == cap
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_il, d_ir, d_ip = t(img_l), t(img_r), t(img_last)
    mk = lambda n: (torch.zeros((P, n, 28), dtype=torch.uint8, device=dev), torch.zeros((P, n, 32), dtype=torch.uint8, device=dev),
                    torch.zeros((P, 2), dtype=torch.int32, device=dev))
    (kL, dL, cL), (kR, dR, cR), (kP, dP, cP), (kC, dC, cC) = mk(cap), mk(cap), mk(cap), mk(2 * cap)
    s = torch.cuda.current_stream().cuda_stream
    sf = exL.GetScaleFactors()
    bounds = (0.0, float(W), 0.0, float(H))
    Trl = np.eye(4, dtype=np.float32)
    Trl[:3, 3] = [SHIFT_R[0] * Z / CAM[0], SHIFT_R[1] * Z / CAM[1], 0.0]

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
    h_cP = cP.cpu().numpy()[:, 0].copy()
    Xw = np.zeros((P, cap, 3), np.float32)
    has = np.zeros((P, cap), np.uint8)
    for p in range(P):
        n = int(h_cP[p])
        rays = synth.kb8_unproject(CAM, h_kP["x"][p, :n].astype(np.float64) + SHIFT_L[0], h_kP["y"][p, :n].astype(np.float64) + SHIFT_L[1])
        Xw[p, :n] = (rays * (Z / rays[:, 2:3])).astype(np.float32)
        has[p, :n] = 1
    d_Xw, d_has = t(Xw), t(has)
    eye = torch.eye(4, device=dev).reshape(1, 16).repeat(P, 1).contiguous()
    d_slot = torch.full((P, 2 * cap), -1, dtype=torch.int32, device=dev)
    d_sobs = torch.zeros((P, 2 * cap), dtype=torch.uint8, device=dev)
    d_nm = torch.zeros((P,), dtype=torch.int32, device=dev)
    cur = pkg.FrameStruct(2 * cap, kC.data_ptr(), dC.data_ptr(), None, *[C.c_float(b) for b in bounds])
    last = pkg.LastFrameStruct(cap, d_has.data_ptr(), d_Xw.data_ptr(), dP.data_ptr(), kP.data_ptr(), None, eye.data_ptr(), eye.data_ptr())
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)

    def search():
        d_slot.fill_(-1); d_sobs.zero_()
        m.search_by_projection_last_frame_fisheye_batch_device(cur, 2 * cap, cC.data_ptr(), 2, cC.data_ptr() + 4, 2, last, cap, cP.data_ptr(), 2, P, sf, Trl, 1, CAM,
                                                               TH, d_slot.data_ptr(), d_sobs.data_ptr(), None, d_nm.data_ptr(), mb=MB, stream=s)

    def mono():
        d_slot.fill_(-1); d_sobs.zero_()
        rc = m.L.orbm_search_by_projection_last_frame_batch_device(
            m.m, C.byref(cur), 2 * cap, C.c_void_p(cC.data_ptr()), 2, C.byref(last), cap, C.c_void_p(cP.data_ptr()), 2, P, ptr(sf), len(sf), 1, ptr(CAM),
            C.c_float(MB), C.c_float(0.0), C.c_float(TH), 1, 1, C.c_void_p(d_slot.data_ptr()), C.c_void_p(d_sobs.data_ptr()), None, C.c_void_p(d_nm.data_ptr()),
            C.c_void_p(s))
        if rc != 0:
            raise SystemExit("monocular last-frame search rc=%d: %s" % (rc, m.L.orbm_last_error(m.m)))

    def chain():
        extract_lr()
        concat()
        search()

    # (b): the same data on the host
    h_kC = kC.cpu().numpy().reshape(P, 2 * cap * 28).view(pkg.KP_DTYPE).reshape(P, 2 * cap)
    h_dC, h_cC, h_dP = dC.cpu().numpy(), cC.cpu().numpy(), dP.cpu().numpy()
    views = []
    for p in range(P):
        N, n0 = int(h_cC[p, 0]), int(h_cP[p])
        views.append((pkg.FrameView(h_kC[p, :N], h_dC[p, :N], bounds), int(h_cC[p, 1]), has[p, :n0], Xw[p, :n0], h_dP[p, :n0], h_kP[p, :n0]))
    I4 = np.eye(4, dtype=np.float32)
    out_b = [None] * P

    def per_frame():
        for p, (F, nl, hp, xw, dp, kp) in enumerate(views):
            F.slot[:] = -1; F.slot_obs[:] = 0
            n = m.SearchByProjectionLastFrameFisheye(F, nl, sf, hp, xw, dp, kp, I4, I4, Trl, 1, CAM, TH, bMono=False, mb=MB)
            out_b[p] = n

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

    for _ in range(a.warmup):
        search(); mono(); concat(); chain()
    per_frame()
    est = dict(a=timed(search, 3)[0], m=timed(mono, 3)[0], k=timed(concat, 3)[0], c=timed(chain, 2)[0], b=timed(per_frame, 1)[1])
    reps = {k: max(2 if k != "b" else 1, int(a.window * 1e3 / max(v, 1e-3)) + 1) for k, v in est.items()}
    T = {k: [] for k in est}
    for r in range(a.rounds):
        T["a"].append(timed(search, reps["a"])[0])
        T["b"].append(timed(per_frame, reps["b"])[1])
        T["m"].append(timed(mono, reps["m"])[0])
        T["k"].append(timed(concat, reps["k"])[0])
        T["c"].append(timed(chain, reps["c"])[0])
    T = {k: np.array(v) for k, v in T.items()}
    mono()
    torch.cuda.synchronize()
    nm_mono = d_nm.cpu().numpy().copy()
    search()
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
    res = dict(frames=P, keypoints_per_rig_frame=float(h_cC[:, 0].mean()), left_per_frame=float(h_cC[:, 1].mean()), last_points_per_frame=float(h_cP.mean()),
               frame_stride=2 * cap, rounds=a.rounds, reps=reps,
               batch_ms=rnd(T["a"].mean()), batch_ms_min=rnd(T["a"].min()), batch_ms_max=rnd(T["a"].max()),
               per_frame_wall_ms=rnd(T["b"].mean(), 3), per_frame_wall_ms_min=rnd(T["b"].min(), 3), per_frame_wall_ms_max=rnd(T["b"].max(), 3),
               speedup=rnd(T["b"].mean() / T["a"].mean(), 1),
               mono_same_keypoints_ms=rnd(T["m"].mean()), mono_same_keypoints_ms_min=rnd(T["m"].min()), mono_same_keypoints_ms_max=rnd(T["m"].max()),
               concat_ms=rnd(T["k"].mean()), concat_ms_min=rnd(T["k"].min()), concat_ms_max=rnd(T["k"].max()),
               chain_ms=rnd(T["c"].mean(), 3), chain_ms_min=rnd(T["c"].min(), 3), chain_ms_max=rnd(T["c"].max(), 3),
               chain_rig_frames_per_s=rnd(P / T["c"].mean() * 1e3, 1), matches_per_frame=float(nm.mean()), left_matches_per_frame=left / P,
               right_matches_per_frame=right / P, mono_matches_per_frame=float(nm_mono.mean()), outputs_identical=differing == 0,
               frames_differing=int(differing), device=torch.cuda.get_device_name(0))
    lines = ["(a) orbm_search_by_projection_last_frame_fisheye_batch_device, %d rig frames, %.0f keypoints per frame (%.0f left), %.0f last-frame points, frame stride %d: %s ms per batch (%d rounds x %d)"
             % (P, h_cC[:, 0].mean(), h_cC[:, 1].mean(), h_cP.mean(), 2 * cap, spread(T["a"]), a.rounds, reps["a"]),
             "    orbm_rig_concat_batch_device alone: %s ms per batch" % spread(T["k"]),
             "(b) %d calls of orbm_search_by_projection_last_frame_fisheye on the same data: %s ms wall (%d rounds x %d)" % (P, spread(T["b"]), a.rounds, reps["b"]),
             "(a) against (b): %.1f x" % (T["b"].mean() / T["a"].mean()),
             "(m) for information, orbm_search_by_projection_last_frame_batch_device over the same concatenated frames (one query per point): %s ms per batch; %.0f matches per frame"
             % (spread(T["m"]), nm_mono.mean()),
             "(c) extract left + extract right + concat + search, one stream: %s ms per %d rig frames = %.0f rig frames/s; %.0f matches per frame (%.0f left, %.0f right)"
             % (spread(T["c"]), P, P / T["c"].mean() * 1e3, nm.mean(), left / P, right / P),
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
