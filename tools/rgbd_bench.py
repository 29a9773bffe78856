"""Frame::ComputeStereoFromRGBD and the close-point rule for a resident batch (orbx_stereo_from_rgbd_batch_device,
orbx_close_points_batch_device) against the round trip through the host that they replace, and the whole RGB-D step on one stream.

256 synthetic TUM1 RGB-D frames (Examples/RGB-D/TUM1.yaml: 640 x 480, 1000 features, DepthMapFactor 5000, bf 40, ThDepth 40, so
th_depth = 40 * 40 / fx; images cut from 32 synthetic canvases at 8 offsets, depth images from tests/rgbd_model.py's generator)
are extracted and undistorted once and stay in HBM.  Legs, alternated a / b / a / b over --rounds:

  (a) the two new calls (the second with the unprojection), HIP-event time per batch; each call alone is timed as well;
  (b) what there was before for the same step: synchronise, download keys and keys_un, the model's arithmetic in numpy (array
      operations, not the model's Python loops: the comparison is against a host path written to be fast; it is checked against the
      literal model on one frame), upload uRight.  The depth images are on the host already, as a host-side pipeline has them.  Wall time;
  (c) colour -> gray, extract, undistort, (a), and orbm_search_by_projection_last_frame_batch_device with bMono = 0 and
      u_right = d_uRight, on one stream, as frames/s.  The last frame of a problem is the frame itself, its map points the unprojected
      keypoints the selection call wrote (identity poses): every map point with depth projects onto a keypoint with a right coordinate.

After the timing the outputs of (a) and (b) are compared bit for bit for all frames.  Exit status 1 if they differ, 2 if (a) is not
faster than (b).  Prints text lines and one JSON line.  Needs a GPU; there is no fallback.

    python tools/rgbd_bench.py [--frames 256] [--rounds 5] [--window 0.25] [--nfeatures 1000]
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
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def host_step(keys, keys_un, counts, raw, factor, mbf, th_depth, max_point):
    """The model's arithmetic (tests/rgbd_model.py) as array operations, per frame.  keys / keys_un: [P][cap] structured, raw [P][H][W]."""
    P, cap = keys.shape
    H, W = raw.shape[1:]
    uR, z = np.full((P, cap), -1, np.float32), np.full((P, cap), -1, np.float32)
    order, nvisit = [], np.zeros(P, np.int32)
    idx = np.arange(cap, dtype=np.uint64)
    with np.errstate(all="ignore"):
        for f in range(P):
            n = int(counts[f])
            v, u = keys["y"][f, :n].astype(np.int64), keys["x"][f, :n].astype(np.int64)      # float -> int truncates
            inside = (v >= 0) & (v < H) & (u >= 0) & (u < W)
            d = np.where(inside, raw[f, np.clip(v, 0, H - 1), np.clip(u, 0, W - 1)].astype(np.float32) * factor, np.float32(-1))
            ok = d > 0
            z[f, :n] = np.where(ok, d, np.float32(-1))
            uR[f, :n] = np.where(ok, keys_un["x"][f, :n] - mbf / d, np.float32(-1))
            zi = z[f, :n]
            key = np.sort(((zi.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[:n])[zi > 0])
            m, c = len(key), int(((zi > 0) & ~(zi > th_depth)).sum())
            nvisit[f] = min(m, max(c, max_point) + 1)
            order.append((key[:nvisit[f]] & np.uint64(0xffffffff)).astype(np.int32))
    return uR, z, order, nvisit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of timed work per leg and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nfeatures", type=int, default=1000)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rgbd_bench: no GPU (there is no fallback)")
    import rgbd_model as RM
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    synth = importlib.import_module("3_orb_slam3_selfnote_amd.synth")
    P, H, W = a.frames, 480, 640
    K, D = RM.TUM1_K, RM.TUM1_D
    factor, mbf, th_depth, max_point = RM.TUM1_FACTOR, RM.TUM1_BF, RM.TUM1_TH_DEPTH, 100
    canv = [synth.make_frame(8100 + c, H + 16, W + 16) for c in range(min(32, P))]
    offs = [(2 * k, 16 - 2 * k) for k in range(8)]
    gray = np.stack([canv[p % 32][offs[(p // 32) % 8][1]:, offs[(p // 32) % 8][0]:][:H, :W] for p in range(P)])
    raw = np.stack([RM.depth_u16(8100 + p, H, W) for p in range(P)])
    dev = torch.device("cuda", 0)
    ex = pkg.ORBextractor(**dict(RM.TUM1, nfeatures=a.nfeatures))
    m = pkg.ORBmatcher(0.9, True)
    cap = ex.configure(H, W, P)
    d_rgb = torch.from_numpy(np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=3))).to(dev)      # R = G = B: cvtColor gives `gray` back
    d_gray = torch.zeros((P, H, W), dtype=torch.uint8, device=dev)
    d_raw = torch.from_numpy(raw.view(np.int16)).to(dev)
    d_k, d_un = torch.zeros((P, cap, 7), device=dev), torch.zeros((P, cap, 7), device=dev)
    d_d = torch.zeros((P, cap, 32), dtype=torch.uint8, device=dev)
    d_c = torch.zeros((P, 2), dtype=torch.int32, device=dev)
    d_uR, d_z = torch.full((P, cap), -9.0, device=dev), torch.full((P, cap), -9.0, device=dev)
    d_ns, d_nv = torch.zeros((P,), dtype=torch.int32, device=dev), torch.zeros((P,), dtype=torch.int32, device=dev)
    d_order = torch.full((P, cap), -9, dtype=torch.int32, device=dev)
    d_close = torch.zeros((P, 2), dtype=torch.int32, device=dev)
    d_xc, d_xw = torch.zeros((P, cap, 3), device=dev), torch.zeros((P, cap, 3), device=dev)
    d_pose = torch.eye(4, device=dev)[:3].reshape(1, 12).repeat(P, 1).contiguous()
    s = torch.cuda.current_stream().cuda_stream
    L = pkg.load()

    def front():
        rc = L.orbx_cvt_color_gray_device(C.c_void_p(d_rgb.data_ptr()), P * H, W, C.c_size_t(3 * W), 3, 1, C.c_void_p(d_gray.data_ptr()), C.c_size_t(W), C.c_void_p(s))
        if rc != 0:
            raise SystemExit("orbx_cvt_color_gray_device rc=%d" % rc)
        ex.extract_batch_device(d_gray.data_ptr(), H, W, W, H * W, P, d_k.data_ptr(), d_d.data_ptr(), d_c.data_ptr(), cap, (0, 0), stream=s)
        m.undistort_batch_device(d_k.data_ptr(), cap, d_c.data_ptr(), 2, P, K, D, d_un.data_ptr(), stream=s)

    def lookup():
        pkg.stereo_from_rgbd_batch_device(P, d_k.data_ptr(), d_un.data_ptr(), d_c.data_ptr(), 2, cap, d_raw.data_ptr(), 0, H, W, 2 * W, 2 * W * H, float(factor),
                                          float(mbf), d_uR.data_ptr(), d_z.data_ptr(), d_ns.data_ptr(), stream=s)

    def select():
        pkg.close_points_batch_device(P, d_z.data_ptr(), d_c.data_ptr(), 2, cap, float(th_depth), max_point, d_order.data_ptr(), d_nv.data_ptr(),
                                      d_close=d_close.data_ptr(), d_keys_un=d_un.data_ptr(), fx=float(K[0]), fy=float(K[1]), cx=float(K[2]), cy=float(K[3]),
                                      d_x3Dc=d_xc.data_ptr(), d_pose=d_pose.data_ptr(), d_x3Dw=d_xw.data_ptr(), stream=s)

    def leg_a():
        lookup()
        select()

    out_b = {}

    def leg_b():
        torch.cuda.synchronize()
        keys = d_k.cpu().numpy().view(pkg.KP_DTYPE).reshape(P, cap)
        keys_un = d_un.cpu().numpy().view(pkg.KP_DTYPE).reshape(P, cap)
        counts = d_c[:, 0].cpu().numpy()
        uR, z, order, nvisit = host_step(keys, keys_un, counts, raw, factor, mbf, th_depth, max_point)
        out_b.update(uR=uR, z=z, order=order, nvisit=nvisit, counts=counts, d_uR=torch.from_numpy(uR).to(dev))
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

    front()
    for _ in range(a.warmup):
        leg_a()
    leg_b()
    est_a, est_b = timed(leg_a, 3)[0], timed(leg_b, 1)[1]
    reps_a, reps_b = max(3, int(a.window * 1e3 / max(est_a, 1e-3)) + 1), max(1, int(a.window * 1e3 / max(est_b, 1e-3)) + 1)
    A, B, A1, A2 = [], [], [], []
    for r in range(a.rounds):
        A.append(timed(leg_a, reps_a)[0])
        B.append(timed(leg_b, reps_b)[1])
        A1.append(timed(lookup, reps_a)[0])
        A2.append(timed(select, reps_a)[0])
    a_ms, b_ms, a1_ms, a2_ms = np.array(A), np.array(B), np.array(A1), np.array(A2)
    # (c) the chain: the frame is its own last frame, its map points are what the selection call unprojected
    d_has = (d_z > 0).to(torch.uint8).contiguous()
    eye = torch.eye(4, device=dev).reshape(1, 16).repeat(P, 1).contiguous()
    d_slot = torch.full((P, cap), -1, dtype=torch.int32, device=dev)
    d_sobs = torch.zeros((P, cap), dtype=torch.uint8, device=dev)
    d_nm = torch.zeros((P,), dtype=torch.int32, device=dev)
    sf = ex.GetScaleFactors()
    bounds = pkg.image_bounds(W, H, K, D)
    cur = pkg.FrameStruct(cap, d_un.data_ptr(), d_d.data_ptr(), d_uR.data_ptr(), *[C.c_float(b) for b in bounds])
    last = pkg.LastFrameStruct(cap, d_has.data_ptr(), d_xw.data_ptr(), d_d.data_ptr(), d_k.data_ptr(), None, eye.data_ptr(), eye.data_ptr())
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)

    def chain():
        d_slot.fill_(-1); d_sobs.zero_()
        front()
        leg_a()
        rc = m.L.orbm_search_by_projection_last_frame_batch_device(
            m.m, C.byref(cur), cap, C.c_void_p(d_c.data_ptr()), 2, C.byref(last), cap, C.c_void_p(d_c.data_ptr()), 2, P, ptr(sf), len(sf), 0, ptr(K),
            C.c_float(float(mbf / K[0])), C.c_float(float(mbf)), C.c_float(7.0), 0, 1, C.c_void_p(d_slot.data_ptr()), C.c_void_p(d_sobs.data_ptr()), None,
            C.c_void_p(d_nm.data_ptr()), C.c_void_p(s))
        if rc != 0:
            raise SystemExit("last-frame search rc=%d: %s" % (rc, m.L.orbm_last_error(m.m)))

    chain()
    est_c = timed(chain, 2)[0]
    reps_c = max(2, int(a.window * 1e3 / max(est_c, 1e-3)) + 1)
    Cc = np.array([timed(chain, reps_c)[0] for _ in range(a.rounds)])
    nm_chain = d_nm.cpu().numpy()
    # bit-for-bit comparison of (a) and (b), and of the array form of (b) with the literal model on frame 0
    leg_a()
    leg_b()
    uRa, za, ns, nv, order = d_uR.cpu().numpy(), d_z.cpu().numpy(), d_ns.cpu().numpy(), d_nv.cpu().numpy(), d_order.cpu().numpy()
    counts = out_b["counts"]
    differing = 0
    for f in range(P):
        n = int(counts[f])
        same = (np.array_equal(uRa[f, :n].view(np.uint32), out_b["uR"][f, :n].view(np.uint32)) and np.array_equal(za[f, :n].view(np.uint32), out_b["z"][f, :n].view(np.uint32))
                and int((out_b["z"][f, :n] > 0).sum()) == ns[f] and nv[f] == out_b["nvisit"][f] and np.array_equal(order[f, :nv[f]], out_b["order"][f]))
        differing += not same
    n0 = int(counts[0])
    k0, ku0 = d_k[0, :n0].cpu().numpy().view(pkg.KP_DTYPE).reshape(n0), d_un[0, :n0].cpu().numpy().view(pkg.KP_DTYPE).reshape(n0)
    uR_m, z_m = RM.compute_stereo_from_rgbd(k0, ku0, raw[0], factor, mbf)
    model_ok = (np.array_equal(uR_m.view(np.uint32), out_b["uR"][0, :n0].view(np.uint32)) and np.array_equal(z_m.view(np.uint32), out_b["z"][0, :n0].view(np.uint32))
                and RM.close_points(z_m, th_depth, max_point)[0] == out_b["order"][0].tolist())
    spread = lambda x: "mean %.4f, min %.4f, max %.4f" % (x.mean(), x.min(), x.max())
    res = dict(frames=P, keypoints_per_frame=float(counts.mean()), with_depth_per_frame=float(ns.mean()), visited_per_frame=float(nv.mean()), rounds=a.rounds,
               reps_a=reps_a, reps_b=reps_b, two_calls_ms=round(float(a_ms.mean()), 4), two_calls_ms_min=round(float(a_ms.min()), 4),
               two_calls_ms_max=round(float(a_ms.max()), 4), lookup_ms=round(float(a1_ms.mean()), 4), selection_ms=round(float(a2_ms.mean()), 4),
               host_round_trip_wall_ms=round(float(b_ms.mean()), 3), host_round_trip_wall_ms_min=round(float(b_ms.min()), 3),
               host_round_trip_wall_ms_max=round(float(b_ms.max()), 3), speedup=round(float(b_ms.mean() / a_ms.mean()), 1),
               chain_ms=round(float(Cc.mean()), 3), chain_ms_min=round(float(Cc.min()), 3), chain_ms_max=round(float(Cc.max()), 3),
               chain_frames_per_s=round(P / float(Cc.mean()) * 1e3, 1), chain_matches_per_frame=float(nm_chain.mean()),
               outputs_identical=differing == 0, frames_differing=int(differing), host_arrays_equal_model=bool(model_ok), device=torch.cuda.get_device_name(0))
    print("(a) orbx_stereo_from_rgbd_batch_device + orbx_close_points_batch_device, %d frames, %.0f keypoints per frame, %.0f with depth, %.0f visited: %s ms per batch (%d rounds x %d)"
          % (P, counts.mean(), ns.mean(), nv.mean(), spread(a_ms), a.rounds, reps_a))
    print("    alone: lookup %s ms; selection + unprojection %s ms" % (spread(a1_ms), spread(a2_ms)))
    print("(b) synchronise, download keys + keys_un, numpy, upload uRight: %s ms wall per batch (%d rounds x %d)" % (spread(b_ms), a.rounds, reps_b))
    print("(a) against (b): %.0f x" % (b_ms.mean() / a_ms.mean()))
    print("(c) colour -> gray + extract + undistort + (a) + last-frame search (bMono = 0, u_right = d_uRight), one stream: %s ms per %d frames = %.0f frames/s; %.0f matches per frame"
          % (spread(Cc), P, P / Cc.mean() * 1e3, nm_chain.mean()))
    print("outputs of (a) and (b): %s; array form of (b) against the literal model on frame 0: %s"
          % ("identical for all %d frames" % P if differing == 0 else "%d frames DIFFER" % differing, "identical" if model_ok else "DIFFERENT"))
    print(json.dumps(res))
    m.close(); ex.close()
    if differing or not model_ok:
        return 1
    return 0 if a_ms.mean() < b_ms.mean() else 2


if __name__ == "__main__":
    sys.exit(main())
