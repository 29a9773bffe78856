"""CLAHE and stereo rectification for a resident batch (orbx_clahe_batch_device, orbx_remap_linear_batch_device) against the loop of
per-image calls they replace (orbx_clahe_device, orbx_remap_linear_device), and the two resident steps they stand in front of.

256 synthetic 512 x 512 frames for CLAHE (3.0, 8 x 8: the TUM-VI examples), 256 synthetic 752 x 480 stereo pairs (tests/stereo_model.py's
set-up, as tools/stereo_bench.py) and one rectification-like float map pair for remap; everything stays in HBM.  Legs, alternated over
--rounds in one process, HIP events on one stream:

  (a) the batch call (CLAHE out of place, remap of the left images);
  (b) the loop of 256 per-image calls on the same resident frames, argument objects made beforehand;
  (c) TUM-VI step: restore the frames (a device copy that stands for whatever wrote them: CLAHE in place would otherwise equalise its
      own output on the next repetition), CLAHE in place, orbx_extract_batch_device, last-frame search (bMono = 1, KannalaBrandt8);
      next to it the same step without the CLAHE call;
  (d) EuRoC stereo step: remap left and right, extract left and right, orbx_compute_stereo_matches_batch_device; next to it the same
      step on the unrectified buffers, as if they were rectified already.

After the timing (a) and (b) are compared byte for byte for all frames of both operations: exit status 1 on a difference, 2 if the
batch call took longer than the loop in any round.  Prints the bytes each operation must move (CLAHE: source twice, destination once;
remap: source, destination, and the maps once per frame chunk) and the resulting bytes/s next to the 6.3 TB/s an MI355X reaches from
HBM.  Writes the text to --out.  Needs a GPU; there is no fallback.

    python tools/preops_bench.py [--frames 256] [--rounds 5] [--window 0.25] [--out profiles/preops_batch_bench.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/preops_bench.py --rounds 1 --window 0.05
    python tools/preops_bench.py --kernel-stats DIR/.../..._kernel_stats.csv      # device time and bytes/s per kernel
"""
import argparse
import csv
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_ACHIEVABLE = 6.3e12
TUMVI = dict(nfeatures=1500, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7)   # Examples/Monocular/TUM_512.yaml
TUMVI_TH = 15.0
KERNELS = ("k_clahe_lut_batch", "k_clahe_interp_batch", "k_remap_linear_batch", "k_clahe_lut", "k_clahe_interp", "k_remap_linear")


def rectify_maps(H, W, seed=0):
    """A rectification-like map pair: small rotation + radial term, reaching outside the source near the corners."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy, f = W / 2 + rng.uniform(-5, 5), H / 2 + rng.uniform(-5, 5), 0.6 * W
    a = np.deg2rad(rng.uniform(-2, 2))
    xn, yn = (xs - cx) / f, (ys - cy) / f
    xr, yr = np.cos(a) * xn - np.sin(a) * yn, np.sin(a) * xn + np.cos(a) * yn
    r2 = xr * xr + yr * yr
    d = 1 + 0.28 * r2 + 0.07 * r2 * r2
    return (xr * d * f + cx).astype(np.float32), (yr * d * f + cy).astype(np.float32)


def must_move(P, chunk):
    """Bytes per batch call: (k_clahe_lut_batch, k_clahe_interp_batch, k_remap_linear_batch)."""
    nchunks = (P + chunk - 1) // chunk
    return P * 512 * 512, 2 * P * 512 * 512, 2 * P * 480 * 752 + nchunks * 8 * 480 * 752


def kernel_stats(path, P, chunk):
    rows = {}
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r["Name"].split("(")[0].split("<")[0].replace("void ", "").strip()     # k_remap_linear_batch<true> counts as k_remap_linear_batch
            c, t = rows.get(name, (0, 0.0))
            rows[name] = (c + int(r["Calls"]), t + float(r["TotalDurationNs"]))
    rows = {k: (c, t, t / c) for k, (c, t) in rows.items()}
    nbytes = dict(zip(KERNELS[:3], must_move(P, chunk)))
    res = {}
    for k in KERNELS:
        if k not in rows:
            continue
        calls, total, avg = rows[k]
        res[k] = dict(calls=calls, avg_us=round(avg / 1e3, 2))
        line = "%-22s %6d calls, %9.2f us each" % (k, calls, avg / 1e3)
        if k in nbytes:
            res[k]["bytes"] = nbytes[k]
            res[k]["TB_per_s"] = round(nbytes[k] / avg / 1e3, 3)
            line += ", %.1f MB to move: %.2f TB/s (%.0f %% of %.1f TB/s)" % (nbytes[k] / 1e6, nbytes[k] / avg / 1e3, 100 * nbytes[k] / avg * 1e9 / HBM_ACHIEVABLE,
                                                                             HBM_ACHIEVABLE / 1e12)
        print(line)
    print(json.dumps(res))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of timed work per leg and round")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preops_batch_bench.txt"))
    ap.add_argument("--no-chains", action="store_true", help="legs (a) and (b) and the comparison only")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.frames, pkg.REMAP_FRAME_CHUNK)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("preops_bench: no GPU (there is no fallback)")
    import stereo_model as SM
    synth = importlib.import_module("3_orb_slam3_selfnote_amd.synth")
    P = a.frames
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    L = pkg.load()
    vp, sz = C.c_void_p, C.c_size_t
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def alternate(legs):
        """Every leg warmed up, then timed once per round in turn.  Returns one array of per-round milliseconds per leg."""
        reps = []
        for fn in legs:
            for _ in range(a.warmup):
                fn()
            reps.append(max(2, int(a.window * 1e3 / max(timed(fn, 2), 1e-3)) + 1))
        out = [[] for _ in legs]
        for _ in range(a.rounds):
            for k, fn in enumerate(legs):
                out[k].append(timed(fn, reps[k]))
        return [np.array(o) for o in out], reps

    spread = lambda x: "median %.4f, min %.4f, max %.4f" % (float(np.median(x)), x.min(), x.max())

    # ---- CLAHE: 512 x 512, the frames of bench.py --config tumvi
    H, W = 512, 512
    groups = [synth.make_stream(1000 + g, min(P, 64), H, W) for g in range((P + 63) // 64)]
    raw = np.concatenate([f for f, _ in groups])[:P]
    offs = [o for _, oo in groups for o in oo][:P]
    d_raw = torch.from_numpy(raw).to(dev)
    d_eq_a, d_eq_b = torch.zeros_like(d_raw), torch.zeros_like(d_raw)
    d_lut = torch.zeros(P * 64 * 256, dtype=torch.uint8, device=dev)

    def clahe_a(src=d_raw, dst=d_eq_a):
        rc = L.orbx_clahe_batch_device(P, vp(src.data_ptr()), H, W, sz(W), sz(H * W), C.c_double(3.0), 8, 8, vp(d_lut.data_ptr()), vp(dst.data_ptr()), sz(W),
                                       sz(H * W), vp(s))
        if rc != 0:
            raise SystemExit("orbx_clahe_batch_device rc=%d" % rc)

    clahe_args = [(vp(d_raw.data_ptr() + f * H * W), H, W, sz(W), C.c_double(3.0), 8, 8, vp(d_lut.data_ptr()), vp(d_eq_b.data_ptr() + f * H * W), sz(W), vp(s))
                  for f in range(P)]

    def clahe_b():
        fn = L.orbx_clahe_device
        for args in clahe_args:
            if fn(*args) != 0:
                raise SystemExit("orbx_clahe_device failed")

    # ---- remap: 752 x 480 stereo pairs as tools/stereo_bench.py makes them
    SH, SW = 480, 752
    rng = np.random.default_rng(5)
    canv = [synth.make_frame(7500 + c, SH, SW + 64) for c in range(min(32, P))]
    disps = np.array([(3, 9, 17, 25, 33, 40, 49, 58)[(p // 32) % 8] for p in range(P)])
    imL = np.stack([canv[p % 32][:, :SW] for p in range(P)])
    imR = np.stack([canv[p % 32][:, disps[p]:disps[p] + SW] for p in range(P)])
    for p in range(1, P, 2):
        imR[p] = (imR[p].astype(np.int32) + rng.integers(-6, 7, imR[p].shape)).clip(0, 255).astype(np.uint8)
    d_L, d_R = torch.from_numpy(imL).to(dev), torch.from_numpy(imR).to(dev)
    d_rL, d_rR, d_rB = torch.zeros_like(d_L), torch.zeros_like(d_R), torch.zeros_like(d_L)
    mx, my = rectify_maps(SH, SW, 3)
    d_mx, d_my = torch.from_numpy(mx).to(dev), torch.from_numpy(my).to(dev)

    def remap_a(src=d_L, dst=d_rL):
        rc = L.orbx_remap_linear_batch_device(P, vp(src.data_ptr()), SH, SW, sz(SW), sz(SH * SW), vp(d_mx.data_ptr()), vp(d_my.data_ptr()), sz(SW), SH, SW,
                                              vp(dst.data_ptr()), sz(SW), sz(SH * SW), vp(s))
        if rc != 0:
            raise SystemExit("orbx_remap_linear_batch_device rc=%d" % rc)

    remap_args = [(vp(d_L.data_ptr() + f * SH * SW), SH, SW, sz(SW), vp(d_mx.data_ptr()), vp(d_my.data_ptr()), sz(SW), SH, SW, vp(d_rB.data_ptr() + f * SH * SW),
                   sz(SW), vp(s)) for f in range(P)]

    def remap_b():
        fn = L.orbx_remap_linear_device
        for args in remap_args:
            if fn(*args) != 0:
                raise SystemExit("orbx_remap_linear_device failed")

    (ca, cb, ra, rb), reps = alternate([clahe_a, clahe_b, remap_a, remap_b])
    b_lut, b_interp, b_remap = must_move(P, pkg.REMAP_FRAME_CHUNK)
    say("device: %s; %d frames; band of %d rows, chunk of %d frames" % (torch.cuda.get_device_name(0), P, pkg.CLAHE_BAND_ROWS, pkg.REMAP_FRAME_CHUNK))
    say("CLAHE 512 x 512, clip 3.0, 8 x 8 tiles")
    say("  (a) orbx_clahe_batch_device: %s ms per batch (%d rounds x %d)" % (spread(ca), a.rounds, reps[0]))
    say("  (b) %d x orbx_clahe_device:   %s ms per batch (%d rounds x %d)" % (P, spread(cb), a.rounds, reps[1]))
    say("  (b) / (a): %.1f at the medians; (a) <= (b) in every round: %s" % (np.median(cb) / np.median(ca), bool((ca <= cb).all())))
    say("  must move %.1f MB (source twice, destination once): %.2f TB/s for the call, %.0f %% of %.1f TB/s"
        % ((b_lut + b_interp) / 1e6, (b_lut + b_interp) / np.median(ca) / 1e9, 100 * (b_lut + b_interp) / np.median(ca) * 1e3 / HBM_ACHIEVABLE, HBM_ACHIEVABLE / 1e12))
    say("remap 752 x 480, float maps, INTER_LINEAR")
    say("  (a) orbx_remap_linear_batch_device: %s ms per batch (%d rounds x %d)" % (spread(ra), a.rounds, reps[2]))
    say("  (b) %d x orbx_remap_linear_device:   %s ms per batch (%d rounds x %d)" % (P, spread(rb), a.rounds, reps[3]))
    say("  (b) / (a): %.1f at the medians; (a) <= (b) in every round: %s" % (np.median(rb) / np.median(ra), bool((ra <= rb).all())))
    say("  must move %.1f MB (source, destination, maps once per chunk): %.2f TB/s, %.0f %% of %.1f TB/s; the loop reads %.1f MB of maps"
        % (b_remap / 1e6, b_remap / np.median(ra) / 1e9, 100 * b_remap / np.median(ra) * 1e3 / HBM_ACHIEVABLE, HBM_ACHIEVABLE / 1e12, P * 8 * SH * SW / 1e6))
    res = dict(frames=P, rounds=a.rounds, band_rows=pkg.CLAHE_BAND_ROWS, frame_chunk=pkg.REMAP_FRAME_CHUNK,
               clahe_batch_ms=[round(float(x), 4) for x in ca], clahe_loop_ms=[round(float(x), 4) for x in cb],
               remap_batch_ms=[round(float(x), 4) for x in ra], remap_loop_ms=[round(float(x), 4) for x in rb],
               clahe_TB_per_s=round((b_lut + b_interp) / float(np.median(ca)) / 1e9, 3), remap_TB_per_s=round(b_remap / float(np.median(ra)) / 1e9, 3))

    if not a.no_chains:
        # ---- (c) the TUM-VI step
        ex = pkg.ORBextractor(**TUMVI)
        mt = pkg.ORBmatcher(0.9, True)
        cap = ex.configure(H, W, P)
        d_img = d_raw.clone()
        d_k = torch.zeros((P + 1, cap, 7), device=dev)
        d_d = torch.zeros((P + 1, cap, 32), dtype=torch.uint8, device=dev)
        d_c = torch.zeros((P + 1, 2), dtype=torch.int32, device=dev)
        d_slot = torch.empty((P, cap), dtype=torch.int32, device=dev)
        d_sobs = torch.empty((P, cap), dtype=torch.uint8, device=dev)
        d_nm = torch.zeros((P,), dtype=torch.int32, device=dev)
        sf = np.ascontiguousarray(ex.GetScaleFactors(), dtype=np.float32)
        kb8 = np.ascontiguousarray(synth.TUMVI_KB8)
        fs = pkg.FrameStruct(cap, d_k[1:].data_ptr(), d_d[1:].data_ptr(), None, 0.0, float(W), 0.0, float(H))
        ptr = lambda x: x.ctypes.data_as(vp)

        def extract_c():
            ex.extract_batch_device(d_img.data_ptr(), H, W, W, H * W, P, d_k[1:].data_ptr(), d_d[1:].data_ptr(), d_c[1:].data_ptr(), cap, (0, 1000), stream=s)
            d_k[0].copy_(d_k[P]); d_d[0].copy_(d_d[P]); d_c[0].copy_(d_c[P])     # the predecessor of frame 0 is the last frame

        def scene(with_clahe):
            """The map of bench.py --config tumvi: the keypoints of frame p - 1 un-projected at their position in frame p."""
            d_img.copy_(d_raw)
            if with_clahe:
                clahe_a(d_img, d_img)
            extract_c()
            torch.cuda.synchronize()
            cnt, kk = d_c[1:].cpu().numpy(), d_k[1:].cpu().numpy()
            Xw, Tcw, Tlw = np.zeros((P, cap, 3), np.float32), np.zeros((P, 16), np.float32), np.zeros((P, 16), np.float32)
            has = np.zeros((P, cap), np.uint8)
            for p in range(P):
                l = (p - 1) % P
                n = int(cnt[l, 0])
                x, T, Tl = synth.make_last_frame_scene(1, kb8, kk[l, :n, 0], kk[l, :n, 1], (offs[l][0] - offs[p][0], offs[l][1] - offs[p][1]), 7000 + p)
                Xw[p, :n] = x; Tcw[p] = T.reshape(-1); Tlw[p] = Tl.reshape(-1); has[p, :n] = 1
            return {k: torch.from_numpy(v).to(dev) for k, v in (("Xw", Xw), ("Tcw", Tcw), ("Tlw", Tlw), ("has", has))}, float(cnt[:, 0].mean())

        def tumvi_step(sc, with_clahe):
            def step():
                d_img.copy_(d_raw)
                if with_clahe:
                    clahe_a(d_img, d_img)
                extract_c()
                d_slot.fill_(-1); d_sobs.zero_()
                last = pkg.LastFrameStruct(cap, sc["has"].data_ptr(), sc["Xw"].data_ptr(), d_d.data_ptr(), d_k.data_ptr(), None, sc["Tcw"].data_ptr(), sc["Tlw"].data_ptr())
                rc = mt.L.orbm_search_by_projection_last_frame_batch_device(
                    mt.m, C.byref(fs), cap, vp(d_c[1:].data_ptr()), 2, C.byref(last), cap, vp(d_c.data_ptr()), 2, P, ptr(sf), len(sf), 1, ptr(kb8),
                    C.c_float(0.0), C.c_float(0.0), C.c_float(TUMVI_TH), 1, 1, vp(d_slot.data_ptr()), vp(d_sobs.data_ptr()), None, vp(d_nm.data_ptr()), vp(s))
                if rc < 0:
                    raise SystemExit("last-frame search rc=%d %s" % (rc, mt.L.orbm_last_error(mt.m)))
            return step

        (sc1, n1), (sc0, n0) = scene(True), scene(False)
        with_c, without_c = tumvi_step(sc1, True), tumvi_step(sc0, False)
        with_c(); torch.cuda.synchronize(); nm1 = float(d_nm.float().mean())
        without_c(); torch.cuda.synchronize(); nm0 = float(d_nm.float().mean())
        (c1, c0), _ = alternate([with_c, without_c])
        say("(c) TUM-VI step, %d frames: restore + CLAHE in place + extract + last-frame search: %s ms = %.0f frames/s (%.0f keypoints, %.0f matches per frame)"
            % (P, spread(c1), P / np.median(c1) * 1e3, n1, nm1))
        say("    the same without CLAHE:                                                  %s ms = %.0f frames/s (%.0f keypoints, %.0f matches per frame)"
            % (spread(c0), P / np.median(c0) * 1e3, n0, nm0))
        res.update(tumvi_step_ms=round(float(np.median(c1)), 4), tumvi_step_without_ms=round(float(np.median(c0)), 4))
        mt.close(); ex.close()
        del d_img, d_k, d_d, d_c, sc1, sc0

        # ---- (d) the EuRoC stereo step
        exL, exR = pkg.ORBextractor(**SM.EUROC_STEREO), pkg.ORBextractor(**SM.EUROC_STEREO)
        cap = max(exL.configure(SH, SW, P), exR.configure(SH, SW, P))
        mk = lambda: (torch.zeros((P, cap, 7), device=dev), torch.zeros((P, cap, 32), dtype=torch.uint8, device=dev), torch.zeros((P, 2), dtype=torch.int32, device=dev))
        (kL, dL, cL), (kR, dR, cR) = mk(), mk()
        d_uR, d_z = torch.full((P, cap), -9.0, device=dev), torch.full((P, cap), -9.0, device=dev)
        d_ns = torch.zeros((P,), dtype=torch.int32, device=dev)

        def stereo_step(rectify):
            def step():
                if rectify:
                    remap_a(d_L, d_rL)
                    remap_a(d_R, d_rR)
                l, r = (d_rL, d_rR) if rectify else (d_L, d_R)
                exL.extract_batch_device(l.data_ptr(), SH, SW, SW, SH * SW, P, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), cap, (0, 0), stream=s)
                exR.extract_batch_device(r.data_ptr(), SH, SW, SW, SH * SW, P, kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap, (0, 0), stream=s)
                exL.compute_stereo_matches_batch_device(exR, P, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap,
                                                        SM.MB, SM.MBF, d_uR.data_ptr(), d_z.data_ptr(), d_ns.data_ptr(), stream=s)
            return step

        with_r, without_r = stereo_step(True), stereo_step(False)
        with_r(); torch.cuda.synchronize(); ns1 = float(d_ns.float().mean())
        without_r(); torch.cuda.synchronize(); ns0 = float(d_ns.float().mean())
        (s1, s0), _ = alternate([with_r, without_r])
        say("(d) EuRoC stereo step, %d pairs: remap L + R, extract L + R, stereo matches: %s ms = %.0f pairs/s (%.0f stereo matches per pair)"
            % (P, spread(s1), P / np.median(s1) * 1e3, ns1))
        say("    the same on input taken as rectified:                               %s ms = %.0f pairs/s (%.0f stereo matches per pair)"
            % (spread(s0), P / np.median(s0) * 1e3, ns0))
        res.update(stereo_step_ms=round(float(np.median(s1)), 4), stereo_step_without_ms=round(float(np.median(s0)), 4))
        exL.close(); exR.close()

    # ---- byte for byte
    d_eq_a.zero_(); d_eq_b.zero_(); d_rL.zero_(); d_rB.zero_()
    clahe_a(); clahe_b(); remap_a(); remap_b()
    torch.cuda.synchronize()
    diff_c = int((d_eq_a != d_eq_b).flatten(1).any(1).sum())
    diff_r = int((d_rL != d_rB).flatten(1).any(1).sum())
    border = int((d_rL == 0).sum())
    say("outputs of (a) and (b): CLAHE %s, remap %s (%d border pixels)"
        % ("identical for all %d frames" % P if diff_c == 0 else "%d frames DIFFER" % diff_c, "identical for all %d frames" % P if diff_r == 0 else "%d frames DIFFER" % diff_r, border))
    res.update(clahe_frames_differing=diff_c, remap_frames_differing=diff_r, device=torch.cuda.get_device_name(0))
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    if diff_c or diff_r:
        return 1
    return 0 if bool((ca <= cb).all() and (ra <= rb).all()) else 2


if __name__ == "__main__":
    sys.exit(main())
