"""Frame::ComputeStereoFishEyeMatches on resident rig batches (orbm_stereo_fisheye_matches_batch_device) against 256 calls of the
per-frame form, against the round trip through the host that it replaces, and inside the resident part of the rig step.

256 synthetic rig pairs (TUM-VI 512 x 512 settings: 1500 features, lapping area 0..511 in both images, the KannalaBrandt8 parameter
sets and Tlr of Examples/Stereo/TUM_512.yaml; images cut from 32 synthetic canvases at 8 offsets; the right image is the left one
shifted by (-8, -9) px, about what that rig sees of a plane 2.4 m away near the image centre) are extracted once and stay in HBM.
Legs, alternated over --rounds:

  (a) orbm_stereo_fisheye_matches_batch_device for all frames, HIP-event time per batch;
  (b) 256 calls of orbm_stereo_fisheye_matches on the same data held on the host, wall time;
  (h) the round trip (a) replaces: synchronise, download both extractions, orbm_knn_match2 per frame, the ratio test and the
      triangulation on the CPU (orbm_fisheye_triangulate, the library's host evaluation, standing in for the reference's), upload
      mvLeftToRightMatch, mvRightToLeftMatch and mvDepth; wall time;
  (c) extract left + extract right + orbm_rig_concat_batch_device + (a) + orbx_close_points_batch_device on one stream, and
  (d) the same without (a) and the close points (which need its mvDepth), as rig frames/s.  The searches that follow in a tracking
      step are timed by tools/rig_bench.py and tools/rig_local_bench.py.

After the timing the outputs of (a) and (b) are compared for all frames.  Exit status 1 if they differ.  Prints text lines and one
JSON line and writes them to --out.  Needs a GPU; there is no fallback.

    python tools/rig_stereo_bench.py [--frames 256] [--rounds 5] [--window 0.25] [--out profiles/rig_stereo_bench.txt]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TUMVI = dict(nfeatures=1500, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7)
# Examples/Stereo/TUM_512.yaml:9-47
CAM1 = np.array([190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504,
                 0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182], np.float32)
CAM2 = np.array([190.44236969414825, 190.4344384721956, 252.59949716835982, 254.91723064636983,
                 0.0034003170790442797, 0.001766278153469831, -0.00266312569781606, 0.0003299517423931039], np.float32)
TLR = np.array([[0.999999445773493, 0.000791687752817, 0.000694034010224, 0.101063427414194],
                [-0.000823363992158, 0.998899461915674, 0.046895490788700, 0.001946204678584],
                [-0.000656143613644, -0.046896036240590, 0.998899560146304, 0.001015350132563]], np.float32)
SHIFT_R = (-8, -9)      # left -> right, in pixels
LAP = (0, 511)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of timed work per leg and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_stereo_bench.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rig_stereo_bench: no GPU (there is no fallback)")
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    synth = importlib.import_module("3_orb_slam3_selfnote_amd.synth")
    P, H, W, M = a.frames, 512, 512, 32
    canv = [synth.make_frame(9300 + c, H + 2 * M, W + 2 * M) for c in range(min(32, P))]
    offs = [(2 * k, 14 - 2 * k) for k in range(8)]
    def crop(p, dx, dy):
        ox, oy = M // 2 + offs[(p // 32) % 8][0] + dx, M // 2 + offs[(p // 32) % 8][1] + dy
        return canv[p % 32][oy:oy + H, ox:ox + W]
    # a scene point at (x, y) of the crop at offset o is at (x - d, y - d') of the crop at offset o + (d, d')
    img_l = np.stack([crop(p, 0, 0) for p in range(P)])
    img_r = np.stack([crop(p, -SHIFT_R[0], -SHIFT_R[1]) for p in range(P)])
    dev = torch.device("cuda", 0)
    exL, exR = pkg.ORBextractor(**TUMVI), pkg.ORBextractor(**TUMVI)
    m = pkg.ORBmatcher(0.9, True)
    cap = exL.configure(H, W, P)
    assert exR.configure(H, W, P) == cap
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_il, d_ir = t(img_l), t(img_r)
    mk = lambda n: (torch.zeros((P, n, 28), dtype=torch.uint8, device=dev), torch.zeros((P, n, 32), dtype=torch.uint8, device=dev),
                    torch.zeros((P, 2), dtype=torch.int32, device=dev))
    (kL, dL, cL), (kR, dR, cR), (kC, dC, cC) = mk(cap), mk(cap), mk(2 * cap)
    s = torch.cuda.current_stream().cuda_stream
    sf = np.asarray(exL.GetScaleFactors(), np.float32)
    sigma2 = (sf * sf).astype(np.float32)
    FS = 2 * cap
    d_l2r = torch.full((P, FS), -1, dtype=torch.int32, device=dev)
    d_r2l = torch.full((P, FS), -1, dtype=torch.int32, device=dev)
    d_depth = torch.full((P, FS), -1.0, dtype=torch.float32, device=dev)
    d_p3d = torch.zeros((P, FS, 3), dtype=torch.float32, device=dev)
    d_nm = torch.zeros((P, 2), dtype=torch.int32, device=dev)
    d_order = torch.zeros((P, FS), dtype=torch.int32, device=dev)
    d_nvisit = torch.zeros((P,), dtype=torch.int32, device=dev)
    ins = [x.data_ptr() for x in (kL, dL, cL, kR, dR, cR)]

    def extract_lr():
        exL.extract_batch_device(d_il.data_ptr(), H, W, W, H * W, P, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), cap, LAP, stream=s)
        exR.extract_batch_device(d_ir.data_ptr(), H, W, W, H * W, P, kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap, LAP, stream=s)

    def concat():
        pkg.rig_concat_batch_device(P, *ins, cap, kC.data_ptr(), dC.data_ptr(), cC.data_ptr(), stream=s)

    def stereo():
        m.stereo_fisheye_matches_batch_device(P, *ins, cap, sigma2, TLR, CAM1, CAM2, FS, d_l2r.data_ptr(), d_r2l.data_ptr(), d_depth.data_ptr(), d_p3d.data_ptr(),
                                              d_nm.data_ptr(), stream=s)

    def close():
        if FS <= pkg.CLOSE_MAX_KEYPOINTS:
            pkg.close_points_batch_device(P, d_depth.data_ptr(), cC.data_ptr() + 4, 2, FS, 3.0, 100, d_order.data_ptr(), d_nvisit.data_ptr(), stream=s)

    def chain():
        extract_lr(); concat(); stereo(); close()

    def chain_without():
        extract_lr(); concat()

    extract_lr()
    concat()
    torch.cuda.synchronize()
    kview = lambda k: k.cpu().numpy().reshape(P, cap * 28).view(pkg.KP_DTYPE).reshape(P, cap)
    h_kL, h_kR, h_dL, h_dR, h_cL, h_cR = kview(kL), kview(kR), dL.cpu().numpy(), dR.cpu().numpy(), cL.cpu().numpy(), cR.cpu().numpy()
    out_b = [None] * P

    def per_frame():
        for p in range(P):
            nl, nr = int(h_cL[p, 0]), int(h_cR[p, 0])
            out_b[p] = m.ComputeStereoFishEyeMatches(h_kL[p, :nl], h_dL[p, :nl], int(h_cL[p, 1]), h_kR[p, :nr], h_dR[p, :nr], int(h_cR[p, 1]), sigma2, TLR, CAM1, CAM2)

    def host_round_trip():
        torch.cuda.synchronize()
        kl, kr, dl, dr, cl, cr = kview(kL), kview(kR), dL.cpu().numpy(), dR.cpu().numpy(), cL.cpu().numpy(), cR.cpu().numpy()
        l2r, r2l, depth = np.full((P, FS), -1, np.int32), np.full((P, FS), -1, np.int32), np.full((P, FS), -1.0, np.float32)
        for p in range(P):
            nl, ml, nr, mr = int(cl[p, 0]), int(cl[p, 1]), int(cr[p, 0]), int(cr[p, 1])
            if nl - ml < 1 or nr - mr < 2:
                continue
            idx, dist = m.knnMatch2(dl[p, ml:nl], dr[p, mr:nr])
            good = np.flatnonzero(dist[:, 0].astype(np.float32) < dist[:, 1].astype(np.float32) * 0.7)
            li, rj = good + ml, idx[good, 0] + mr
            z, _ = pkg.fisheye_triangulate(np.stack([kl["x"][p, li], kl["y"][p, li]], 1), np.stack([kr["x"][p, rj], kr["y"][p, rj]], 1),
                                           sigma2[kl["octave"][p, li]], sigma2[kr["octave"][p, rj]], TLR, CAM1, CAM2)
            ok = z > np.float32(0.0001)
            l2r[p, li[ok]], r2l[p, rj[ok]], depth[p, li[ok]] = rj[ok], li[ok], z[ok]      # ascending left order: the last one stays
        d_l2r.copy_(torch.from_numpy(l2r)); d_r2l.copy_(torch.from_numpy(r2l)); d_depth.copy_(torch.from_numpy(depth))
        torch.cuda.synchronize()

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
        stereo(); chain(); chain_without()
    per_frame(); host_round_trip()
    est = dict(a=timed(stereo, 3)[0], c=timed(chain, 2)[0], d=timed(chain_without, 2)[0], b=timed(per_frame, 1)[1], h=timed(host_round_trip, 1)[1])
    reps = {k: max(1 if k in "bh" else 2, int(a.window * 1e3 / max(v, 1e-3)) + 1) for k, v in est.items()}
    T = {k: [] for k in est}
    for r in range(a.rounds):
        T["a"].append(timed(stereo, reps["a"])[0])
        T["b"].append(timed(per_frame, reps["b"])[1])
        T["h"].append(timed(host_round_trip, reps["h"])[1])
        T["c"].append(timed(chain, reps["c"])[0])
        T["d"].append(timed(chain_without, reps["d"])[0])
    T = {k: np.array(v) for k, v in T.items()}
    host_round_trip()
    h_l2r, h_r2l, h_depth = d_l2r.cpu().numpy().copy(), d_r2l.cpu().numpy().copy(), d_depth.cpu().numpy().copy()
    stereo()
    torch.cuda.synchronize()
    l2r, r2l, depth, p3d, nm = [x.cpu().numpy() for x in (d_l2r, d_r2l, d_depth, d_p3d, d_nm)]
    per_frame()
    differing = host_differing = 0
    for p in range(P):
        nl, nr = int(h_cL[p, 0]), int(h_cR[p, 0])
        b = out_b[p]
        matched = b[0] >= 0
        differing += not (np.array_equal(b[0], l2r[p, :nl]) and np.array_equal(b[1], r2l[p, :nr]) and b[2].tobytes() == depth[p, :nl].tobytes()
                          and b[3][matched].tobytes() == p3d[p, :nl][matched].tobytes() and b[4] == tuple(nm[p]))
        host_differing += not (np.array_equal(h_l2r[p, :nl], l2r[p, :nl]) and np.array_equal(h_r2l[p, :nr], r2l[p, :nr])
                               and h_depth[p, :nl].tobytes() == depth[p, :nl].tobytes())
    spread = lambda x: "median %.4f, min %.4f, max %.4f" % (np.median(x), x.min(), x.max())
    rnd = lambda x, k=4: round(float(x), k)
    med = {k: float(np.median(v)) for k, v in T.items()}
    res = dict(frames=P, left_per_frame=float(h_cL[:, 0].mean()), right_per_frame=float(h_cR[:, 0].mean()),
               lapping_left=float((h_cL[:, 0] - h_cL[:, 1]).mean()), lapping_right=float((h_cR[:, 0] - h_cR[:, 1]).mean()), cap=cap, out_stride=FS,
               rounds=a.rounds, reps=reps, matches_per_frame=float(nm[:, 0].mean()), desc_matches_per_frame=float(nm[:, 1].mean()),
               **{"%s_ms_%s" % (n, q): rnd(f(T[k]), 4) for k, n in (("a", "batch"), ("b", "per_frame_wall"), ("h", "host_round_trip_wall"), ("c", "chain"),
                                                                     ("d", "chain_without")) for q, f in (("median", np.median), ("min", np.min), ("max", np.max))},
               speedup_over_per_frame=rnd(med["b"] / med["a"], 1), speedup_over_host_round_trip=rnd(med["h"] / med["a"], 1),
               chain_rig_frames_per_s=rnd(P / med["c"] * 1e3, 1), chain_without_rig_frames_per_s=rnd(P / med["d"] * 1e3, 1),
               outputs_identical=differing == 0, frames_differing=int(differing), host_round_trip_frames_differing=int(host_differing),
               device=torch.cuda.get_device_name(0))
    lines = ["(a) orbm_stereo_fisheye_matches_batch_device, %d rig frames, %.0f + %.0f keypoints per frame (%.0f + %.0f lapping), cap %d, out stride %d: %s ms per batch (%d rounds x %d); %.0f matches of %.0f ratio-test passes per frame"
             % (P, h_cL[:, 0].mean(), h_cR[:, 0].mean(), res["lapping_left"], res["lapping_right"], cap, FS, spread(T["a"]), a.rounds, reps["a"], nm[:, 0].mean(), nm[:, 1].mean()),
             "(b) %d calls of orbm_stereo_fisheye_matches on the same data: %s ms wall (%d rounds x %d)" % (P, spread(T["b"]), a.rounds, reps["b"]),
             "(a) against (b): %.1f x" % (med["b"] / med["a"]),
             "(h) the host round trip it replaces (synchronise, download, orbm_knn_match2 per frame, triangulation on the CPU, upload of three tables): %s ms wall (%d rounds x %d)"
             % (spread(T["h"]), a.rounds, reps["h"]),
             "(a) against (h): %.1f x" % (med["h"] / med["a"]),
             "(c) extract left + extract right + concat + stereo matches + close points, one stream: %s ms per %d rig frames = %.0f rig frames/s"
             % (spread(T["c"]), P, P / med["c"] * 1e3),
             "(d) the same without the stereo matches and the close points: %s ms = %.0f rig frames/s; the call adds %.4f ms per batch to the chain"
             % (spread(T["d"]), P / med["d"] * 1e3, med["c"] - med["d"]),
             "outputs of (a) and (b): %s; tables of (h) against (a): %s"
             % ("identical for all %d frames" % P if differing == 0 else "%d frames DIFFER" % differing,
                "identical" if host_differing == 0 else "%d frames differ" % host_differing),
             json.dumps(res)]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    m.close(); exL.close(); exR.close()
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
