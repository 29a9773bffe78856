"""Device time of Tracking::SearchLocalPoints on the device (orbm_search_local_points_batch_device: k_local_map_project + the M2
search) for a batch of (frame, local map) problems, against the existing M2 batched form (orbm_search_by_projection_batch_device) fed
the same queries precomputed.  The difference is what the frustum kernel costs in place of the host loop it replaces.

Each problem: one synthetic EuRoC frame (about 1000 keypoints) and 3000 local map points (synth.make_local_map_scene, the generator
tests/test_gpu_local_points.py uses as well), with a slightly different pose per problem.  Times are HIP-event times around each call
on one stream (slot resets outside the events), averaged over --iters calls after --warmup.  Prints text lines and one JSON line.

    python tools/local_points_bench.py [--problems 256] [--map 3000] [--iters 20] [--warmup 5]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS = ("in_view", "proj_x", "proj_y", "proj_xr", "depth", "view_cos", "level")
EUROC = dict(nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7)   # Examples/Monocular/EuRoC.yaml:34-47
PIN = np.array([458.654, 457.296, 367.215, 248.375], np.float32)                   # Examples/Monocular/EuRoC.yaml:9-12


class Scene:
    pass


def make_scene(pkg, oracle, synth, seed, nmap):
    """One synthetic EuRoC frame pair (oracle extraction) and the local map synth.make_local_map_scene builds over it."""
    S = Scene()
    H, W = 480, 752
    frames, offs = synth.make_stream(seed, 2, H=H, W=W)
    o = oracle.OracleExtractor(**EUROC)
    _, k0, d0 = o.extract(frames[0])
    _, S.k1, S.d1 = o.extract(frames[1])
    S.sf = np.asarray(o.scale_factors, np.float32)
    S.log_sf = float(pkg.load().orbx_ref_logf(1.2))          # Frame::mfLogScaleFactor = log(1.2f), glibc logf
    S.bounds, S.cam_type, S.cam = (0.0, float(W), 0.0, float(H)), 0, PIN
    L = synth.make_local_map_scene(0, PIN, k0, d0, S.k1, (offs[0][0] - offs[1][0], offs[0][1] - offs[1][1]), seed, S.sf, W, H, nmap=nmap)
    S.Xw, S.desc, S.normal, S.maxd, S.mind = L["Xw"], L["desc"], L["normal"], L["max_dist"], L["min_dist"]
    S.elig, S.obs, S.Tcw, S.slot0, S.sobs0 = L["eligible"], L["obs"], L["Tcw"], L["slot"], L["slot_obs"]
    return S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--map", type=int, default=3000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--th", type=float, default=3.0)
    a = ap.parse_args()
    import torch
    from oracle import oracle_py as oracle
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    synth = importlib.import_module("3_orb_slam3_selfnote_amd.synth")
    oracle.build()
    S = make_scene(pkg, oracle, synth, 5100, a.map)
    P, n1, nmp = a.problems, len(S.k1), len(S.Xw)
    fstride, mstride = (n1 + 63) // 64 * 64, (nmp + 63) // 64 * 64
    f32 = np.float32
    dev = "cuda"
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rep = lambda x, stride: np.concatenate([x, np.zeros((stride - len(x),) + x.shape[1:], x.dtype)])[None].repeat(P, 0)
    kview = np.ascontiguousarray(S.k1).view(f32).reshape(n1, 7)
    d_kp, d_de = t(rep(kview, fstride)), t(rep(S.d1, fstride))
    d_cnt = t(np.tile(np.int32([n1, 0]), (P, 1)))
    d_mc = t(np.tile(np.int32([nmp, 0]), (P, 1)))
    slot0 = t(rep(S.slot0, fstride))
    sobs0 = t(rep(S.sobs0, fstride))
    d = {k: t(rep(getattr(S, k), mstride)) for k in ("elig", "Xw", "normal", "maxd", "mind", "desc", "obs")}
    Tcws = []
    for p in range(P):
        Tp = S.Tcw.copy()
        Tp[:3, 3] += f32(0.001) * np.array([p % 8 - 3.5, (p // 8) % 8 - 3.5, 0.2 * (p % 5)], f32)
        Tcws.append(Tp)
    d_T = t(np.stack(Tcws))
    d_slot, d_sobs = slot0.clone(), sobs0.clone()
    d_moq = torch.zeros((P, mstride), dtype=torch.int32, device=dev)
    tr = {k: torch.zeros((P, mstride), dtype=torch.uint8 if k == "in_view" else torch.int32 if k == "level" else torch.float32, device=dev)
          for k in FIELDS}
    d_nm = torch.zeros(P, dtype=torch.int32, device=dev)
    fs = pkg.FrameStruct(fstride, d_kp.data_ptr(), d_de.data_ptr(), None, *S.bounds)
    ms = pkg.LocalMapStruct(mstride, d["elig"].data_ptr(), d["Xw"].data_ptr(), d["normal"].data_ptr(), d["maxd"].data_ptr(), d["mind"].data_ptr(),
                            d["desc"].data_ptr(), d["obs"].data_ptr(), d_T.data_ptr())
    ts = pkg.TrackStruct(*[tr[k].data_ptr() for k in FIELDS])
    m = pkg.ORBmatcher(0.8, True)
    stream = torch.cuda.current_stream().cuda_stream

    def local():
        m.search_local_points_batch_device(fs, fstride, d_cnt.data_ptr(), 2, ms, mstride, d_mc.data_ptr(), 2, P, S.sf, S.log_sf, S.cam_type, S.cam,
                                           a.th, d_slot.data_ptr(), d_sobs.data_ptr(), d_moq.data_ptr(), ts, d_nm.data_ptr(), stream=stream)

    # the same queries, precomputed from one local-points run (ORBmatcher.cc:52-73), for the plain M2 batched form
    d_slot.copy_(slot0); d_sobs.copy_(sobs0)
    local()
    torch.cuda.synchronize()
    nm_local = d_nm.cpu().numpy().copy()
    iv, lvl, vc = tr["in_view"], tr["level"].long().clamp(0, len(S.sf) - 1), tr["view_cos"]
    sf = torch.from_numpy(S.sf).to(dev)
    r = torch.where(vc.double() > 0.998, torch.tensor(2.5, device=dev), torch.tensor(4.0, device=dev)).float()
    if a.th != 1.0:
        r = r * f32(a.th)
    rad = (r * sf[lvl]).contiguous()
    take = (iv != 0) & (d["elig"] != 0) & ~torch.isnan(tr["proj_x"]) & ~torch.isnan(tr["proj_y"])
    flags = (take.to(torch.uint8) | (d["obs"] << 1)).contiguous()
    qu, qv = tr["proj_x"].clone(), tr["proj_y"].clone()
    qlo, qhi = (lvl - 1).int().contiguous(), lvl.int().contiguous()
    qs = pkg.QueryStruct(mstride, d["desc"].data_ptr(), qu.data_ptr(), qv.data_ptr(), rad.data_ptr(), qlo.data_ptr(), qhi.data_ptr(), None,
                         flags.data_ptr())
    d_moq2 = torch.zeros((P, mstride), dtype=torch.int32, device=dev)

    def m2():
        rc = m.L.orbm_search_by_projection_batch_device(m.m, C.byref(fs), fstride, C.c_void_p(d_cnt.data_ptr()), 2, C.byref(qs), mstride,
                                                        C.c_void_p(d_mc.data_ptr()), 2, P, C.c_float(0.8), 100, 1, C.c_void_p(d_slot.data_ptr()),
                                                        C.c_void_p(d_sobs.data_ptr()), C.c_void_p(d_moq2.data_ptr()), None,
                                                        C.c_void_p(d_nm.data_ptr()), C.c_void_p(stream))
        assert rc == 0, m.L.orbm_last_error(m.m)

    def timed(fn):
        ms_ = []
        for it in range(a.warmup + a.iters):
            d_slot.copy_(slot0); d_sobs.copy_(sobs0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                ms_.append(e0.elapsed_time(e1))
        return float(np.mean(ms_)), float(np.min(ms_))

    t_local, t_local_min = timed(local)
    t_m2, t_m2_min = timed(m2)
    torch.cuda.synchronize()
    same = bool(np.array_equal(d_nm.cpu().numpy(), nm_local) and torch.equal(d_moq2, d_moq))
    res = dict(problems=P, keypoints=n1, map_points=nmp, th=a.th, iters=a.iters, local_points_ms=round(t_local, 4),
               local_points_min_ms=round(t_local_min, 4), m2_precomputed_ms=round(t_m2, 4), m2_precomputed_min_ms=round(t_m2_min, 4),
               frustum_cost_ms=round(t_local - t_m2, 4), matches_per_problem=float(nm_local.mean()), m2_equals_local=same,
               device=torch.cuda.get_device_name(0))
    print("local points (k_local_map_project + M2), %d problems x %d keypoints x %d map points: %.3f ms (min %.3f)" % (P, n1, nmp, t_local, t_local_min))
    print("M2 batched form, same queries precomputed: %.3f ms (min %.3f)" % (t_m2, t_m2_min))
    print("difference (the frustum kernel and its query preparation): %.3f ms; %.1f matches per problem; results equal: %s"
          % (t_local - t_m2, nm_local.mean(), same))
    print(json.dumps(res))
    m.close()


if __name__ == "__main__":
    main()
