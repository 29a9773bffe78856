"""Frame::ComputeStereoMatches for a resident batch (orbx_compute_stereo_matches_batch_device) against a loop of the existing
per-frame entry point (orbx_compute_stereo_matches), and the whole stereo step on one stream.

256 synthetic EuRoC stereo pairs (tests/stereo_model.py's generator: left and right cut from one wider synthetic frame; 752 x 480,
1200 features, mb 0.11, mbf 47.9) are extracted once as two batches and stay in HBM.  Legs, alternated a / b / a / b over --rounds:

  (a) the new call alone, HIP-event time per call;
  (b) the same 256 pairs through orbx_compute_stereo_matches, frame indices 0..255 of the same two batches, keypoints and
      descriptors downloaded once outside the timed window.  The entry point is synchronous, so its HIP-event time (events on the
      default stream around the loop) and its wall time are the same thing; both are printed;
  (c) extract left, extract right, (a), and orbm_search_by_projection_last_frame_batch_device with bMono = 0 and
      u_right = d_uRight, on one stream, as frames/s.  The last frame of a pair is its own left frame (map points on the keypoints'
      rays at the stereo depth, identity poses): every map point projects onto a keypoint with a right coordinate.

After the timing the outputs of (a) and (b) are compared bit for bit for all pairs.  Exit status 1 if they differ, 2 if (a) is not
faster than (b).  Prints text lines and one JSON line.  Needs a GPU; there is no fallback.

    python tools/stereo_bench.py [--pairs 256] [--rounds 5] [--window 0.25]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/stereo_bench.py --rounds 1 --window 0.05
    python tools/stereo_bench.py --kernel-stats DIR/.../..._kernel_stats.csv     # device time of the new kernels against k_stereo_match
"""
import argparse
import csv
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CAM = np.array([435.2046959714599, 435.2046959714599, 367.4517211914062, 252.2008514404297], np.float32)   # Examples/Stereo/EuRoC.yaml
NEW_KERNELS = ("k_stereo_rows", "k_stereo_search", "k_stereo_median")


def kernel_stats(path, pairs):
    """Summed device time of the new kernels per batch call against `pairs` average k_stereo_match dispatches, from a
    rocprofv3 --kernel-trace --stats CSV of a run of this tool."""
    rows = {}
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            rows[r["Name"].split("(")[0].strip()] = (int(r["Calls"]), float(r["TotalDurationNs"]), float(r["AverageNs"]))
    calls = rows["k_stereo_search"][0]
    new_us = sum(rows[k][1] for k in NEW_KERNELS) / calls / 1e3
    old_avg_us = rows["k_stereo_match"][2] / 1e3
    res = dict(pairs=pairs, batch_calls=calls, new_kernels_us_per_batch=round(new_us, 2), k_stereo_match_avg_us=round(old_avg_us, 3),
               k_stereo_match_us_per_batch=round(old_avg_us * pairs, 2), ratio_old_over_new=round(old_avg_us * pairs / new_us, 3),
               per_kernel_avg_us={k: round(rows[k][2] / 1e3, 2) for k in NEW_KERNELS})
    print("new kernels, %d pairs: %.1f us per batch (%s); k_stereo_match: %.2f us per dispatch, %.1f us for %d: ratio %.2f"
          % (pairs, new_us, ", ".join("%s %.1f" % (k, rows[k][2] / 1e3) for k in NEW_KERNELS), old_avg_us, old_avg_us * pairs, pairs,
             old_avg_us * pairs / new_us))
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of timed work per leg and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.pairs)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("stereo_bench: no GPU (there is no fallback)")
    import stereo_model as SM
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    synth = importlib.import_module("3_orb_slam3_selfnote_amd.synth")
    P, H, W = a.pairs, 480, 752
    mb, mbf = SM.MB, SM.MBF
    # 32 canvases x 8 disparities: 256 distinct pairs; odd pairs with noise on the right image
    rng = np.random.default_rng(5)
    canv = [synth.make_frame(7500 + c, H, W + 64) for c in range(min(32, P))]
    disps = np.array([(3, 9, 17, 25, 33, 40, 49, 58)[(p // 32) % 8] for p in range(P)])
    L = np.stack([canv[p % 32][:, :W] for p in range(P)])
    R = np.stack([canv[p % 32][:, disps[p]:disps[p] + W] for p in range(P)])
    for p in range(1, P, 2):
        R[p] = (R[p].astype(np.int32) + rng.integers(-6, 7, R[p].shape)).clip(0, 255).astype(np.uint8)
    dev = torch.device("cuda", 0)
    exL, exR = pkg.ORBextractor(**SM.EUROC_STEREO), pkg.ORBextractor(**SM.EUROC_STEREO)
    m = pkg.ORBmatcher(0.9, True)
    cap = max(exL.configure(H, W, P), exR.configure(H, W, P))
    d_L, d_R = torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)
    mk = lambda: (torch.zeros((P, cap, 7), dtype=torch.float32, device=dev), torch.zeros((P, cap, 32), dtype=torch.uint8, device=dev),
                  torch.zeros((P, 2), dtype=torch.int32, device=dev))
    (kL, dL, cL), (kR, dR, cR) = mk(), mk()
    d_uR = torch.full((P, cap), -9.0, device=dev)
    d_z = torch.full((P, cap), -9.0, device=dev)
    d_ns = torch.zeros((P,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    s = st.cuda_stream

    def extract():
        exL.extract_batch_device(d_L.data_ptr(), H, W, W, H * W, P, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), cap, (0, 0), stream=s)
        exR.extract_batch_device(d_R.data_ptr(), H, W, W, H * W, P, kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap, (0, 0), stream=s)

    def leg_a():
        exL.compute_stereo_matches_batch_device(exR, P, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap, mb, mbf,
                                                d_uR.data_ptr(), d_z.data_ptr(), d_ns.data_ptr(), stream=s)

    extract()
    leg_a()
    torch.cuda.synchronize()
    # leg (b): host copies of what the extractions wrote, made once
    nL, nR = cL[:, 0].cpu().numpy(), cR[:, 0].cpu().numpy()
    hkL, hkR = kL.cpu().numpy().view(np.uint8).reshape(P, cap, 28), kR.cpu().numpy().view(np.uint8).reshape(P, cap, 28)
    hdL, hdR = dL.cpu().numpy(), dR.cpu().numpy()
    host = [(np.ascontiguousarray(hkL[f, :nL[f]]), np.ascontiguousarray(hdL[f, :nL[f]]), np.ascontiguousarray(hkR[f, :nR[f]]),
             np.ascontiguousarray(hdR[f, :nR[f]])) for f in range(P)]
    out_b = [(np.zeros(nL[f], np.float32), np.zeros(nL[f], np.float32)) for f in range(P)]
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    args_b = [(exL.h, f, exR.h, f, int(nL[f]), ptr(host[f][0]), ptr(host[f][1]), int(nR[f]), ptr(host[f][2]), ptr(host[f][3]), C.c_float(mb), C.c_float(mbf),
               ptr(out_b[f][0]), ptr(out_b[f][1])) for f in range(P)]
    fn_b = exL.L.orbx_compute_stereo_matches

    def leg_b():
        for f in range(P):
            rc = fn_b(*args_b[f])
            if rc < 0:
                raise SystemExit("orbx_compute_stereo_matches rc=%d" % rc)

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
        leg_a()
    leg_b()
    est_a, est_b = timed(leg_a, 3)[0], timed(leg_b, 1)[1]
    reps_a, reps_b = max(3, int(a.window * 1e3 / max(est_a, 1e-3)) + 1), max(1, int(a.window * 1e3 / max(est_b, 1e-3)) + 1)
    A, B = [], []
    for r in range(a.rounds):
        A.append(timed(leg_a, reps_a))
        B.append(timed(leg_b, reps_b))
    a_ms, b_ms, b_wall = np.array([x[0] for x in A]), np.array([x[0] for x in B]), np.array([x[1] for x in B])
    # (c) the chain.  Map points: the left keypoints un-projected at the stereo depth of their pair
    z = torch.from_numpy((np.float32(47.90639384423901) / disps).astype(np.float32)).to(dev)[:, None]
    Xw = torch.stack([(kL[:, :, 0] - CAM[2]) * z / CAM[0], (kL[:, :, 1] - CAM[3]) * z / CAM[1], z.expand(P, cap)], dim=2).contiguous()
    kP, dP, cP = kL.clone(), dL.clone(), cL.clone()
    has = torch.ones((P, cap), dtype=torch.uint8, device=dev)
    eye = torch.eye(4, device=dev).reshape(1, 16).repeat(P, 1).contiguous()
    d_slot = torch.full((P, cap), -1, dtype=torch.int32, device=dev)
    d_sobs = torch.zeros((P, cap), dtype=torch.uint8, device=dev)
    d_nm = torch.zeros((P,), dtype=torch.int32, device=dev)
    sf = exL.GetScaleFactors()
    cur = pkg.FrameStruct(cap, kL.data_ptr(), dL.data_ptr(), d_uR.data_ptr(), 0.0, float(W), 0.0, float(H))
    last = pkg.LastFrameStruct(cap, has.data_ptr(), Xw.data_ptr(), dP.data_ptr(), kP.data_ptr(), None, eye.data_ptr(), eye.data_ptr())
    mbc = float(np.float32(47.90639384423901) / CAM[0])

    def chain():
        d_slot.fill_(-1); d_sobs.zero_()
        extract()
        leg_a()
        rc = m.L.orbm_search_by_projection_last_frame_batch_device(
            m.m, C.byref(cur), cap, C.c_void_p(cL.data_ptr()), 2, C.byref(last), cap, C.c_void_p(cP.data_ptr()), 2, P, ptr(sf), len(sf), 0, ptr(CAM),
            C.c_float(mbc), C.c_float(47.90639384423901), C.c_float(7.0), 0, 1, C.c_void_p(d_slot.data_ptr()), C.c_void_p(d_sobs.data_ptr()), None,
            C.c_void_p(d_nm.data_ptr()), C.c_void_p(s))
        if rc != 0:
            raise SystemExit("last-frame search rc=%d: %s" % (rc, m.L.orbm_last_error(m.m)))

    chain()
    est_c = timed(chain, 2)[0]
    reps_c = max(2, int(a.window * 1e3 / max(est_c, 1e-3)) + 1)
    Cc = np.array([timed(chain, reps_c)[0] for _ in range(a.rounds)])
    nm_chain = d_nm.cpu().numpy()
    # bit-for-bit comparison of (a) and (b)
    leg_a()
    torch.cuda.synchronize()
    leg_b()
    uRa, za, ns = d_uR.cpu().numpy(), d_z.cpu().numpy(), d_ns.cpu().numpy()
    differing = 0
    for f in range(P):
        n = int(nL[f])
        same = (np.array_equal(uRa[f, :n].view(np.uint32), out_b[f][0].view(np.uint32)) and np.array_equal(za[f, :n].view(np.uint32), out_b[f][1].view(np.uint32))
                and int((out_b[f][0] >= 0).sum()) == ns[f])
        differing += not same
    spread = lambda x: "mean %.3f, min %.3f, max %.3f" % (x.mean(), x.min(), x.max())
    res = dict(pairs=P, keypoints_per_image=float(nL.mean()), stereo_matches_per_pair=float(ns.mean()), rounds=a.rounds, reps_a=reps_a, reps_b=reps_b,
               batch_call_ms=round(float(a_ms.mean()), 4), batch_call_ms_min=round(float(a_ms.min()), 4), batch_call_ms_max=round(float(a_ms.max()), 4),
               loop_ms=round(float(b_ms.mean()), 3), loop_ms_min=round(float(b_ms.min()), 3), loop_ms_max=round(float(b_ms.max()), 3),
               loop_wall_ms=round(float(b_wall.mean()), 3), speedup=round(float(b_ms.mean() / a_ms.mean()), 2),
               chain_ms=round(float(Cc.mean()), 3), chain_ms_min=round(float(Cc.min()), 3), chain_ms_max=round(float(Cc.max()), 3),
               chain_frames_per_s=round(P / float(Cc.mean()) * 1e3, 1), chain_matches_per_pair=float(nm_chain.mean()),
               outputs_identical=differing == 0, pairs_differing=int(differing), device=torch.cuda.get_device_name(0))
    print("(a) orbx_compute_stereo_matches_batch_device, %d pairs, %.0f keypoints per image, %.0f stereo matches per pair: %s ms per call (%d rounds x %d calls)"
          % (P, nL.mean(), ns.mean(), spread(a_ms), a.rounds, reps_a))
    print("(b) %d x orbx_compute_stereo_matches: %s ms per pass (HIP events; wall %.3f; %d rounds x %d passes)" % (P, spread(b_ms), b_wall.mean(), a.rounds, reps_b))
    print("(a) against (b): %.1f x" % (b_ms.mean() / a_ms.mean()))
    print("(c) extract L + extract R + stereo matches + last-frame search (bMono = 0, u_right = d_uRight), one stream: %s ms per %d pairs = %.0f frames/s; %.0f matches per pair"
          % (spread(Cc), P, P / Cc.mean() * 1e3, nm_chain.mean()))
    print("outputs of (a) and (b): %s" % ("identical for all %d pairs" % P if differing == 0 else "%d pairs DIFFER" % differing))
    print(json.dumps(res))
    m.close(); exL.close(); exR.close()
    if differing:
        return 1
    return 0 if a_ms.mean() < b_ms.mean() else 2


if __name__ == "__main__":
    sys.exit(main())
