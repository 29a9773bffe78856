#!/usr/bin/env python3
"""Randomised parity sweep (run ON THE GPU BOX from the repo root):  python tests/fuzz_parity.py [--n 200] [--seed 1]

Draws random extractor configurations (image size, nfeatures, scaleFactor, nlevels, thresholds, lapping area, image
statistics) and random window-search problems (query count, radii, level windows, pre-occupied keypoints, observation
flags, ratio / distance thresholds), runs each through the C ABI and through the CPU oracle and reports every
difference.  Test infrastructure: the oracle is only the checker here.  Exit status 1 on any mismatch."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def random_image(rng, H, W, synth):
    kind = rng.integers(0, 5)
    if kind == 0:
        return synth.make_frame(int(rng.integers(1, 1 << 30)), H, W)
    if kind == 1:   # noise: corners everywhere, quotas and the octree are stressed
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == 2:   # low contrast: the per-cell minThFAST fallback decides
        base = synth.make_frame(int(rng.integers(1, 1 << 30)), H, W).astype(np.int32)
        return (128 + (base - 128) // int(rng.integers(3, 9))).clip(0, 255).astype(np.uint8)
    if kind == 3:   # blocks: many equal scores (NMS and octree ties)
        s = int(rng.integers(4, 17))
        small = rng.integers(0, 4, ((H + s - 1) // s, (W + s - 1) // s), dtype=np.uint8) * 80
        return np.kron(small, np.ones((s, s), np.uint8))[:H, :W].copy()
    img = synth.make_frame(int(rng.integers(1, 1 << 30)), H, W)   # half flat: empty cells and levels
    img[:, W // 2:] = 90
    return img


def fuzz_extract(pkg, oracle, synth, rng, log, cache):
    H, W = int(rng.integers(96, 640)), int(rng.integers(96, 800))
    cfg = dict(nfeatures=int(rng.choice([30, 200, 500, 1000, 1500, 3000])), scaleFactor=float(rng.choice([1.1, 1.2, 1.25, 1.5, 2.0])),
               nlevels=int(rng.integers(1, 17)), iniThFAST=int(rng.integers(8, 41)), minThFAST=int(rng.integers(2, 12)))
    if cfg["minThFAST"] > cfg["iniThFAST"]:
        cfg["minThFAST"] = cfg["iniThFAST"]
    img = random_image(rng, H, W, synth)
    lap = (0, 0) if rng.random() < 0.5 else tuple(sorted(int(v) for v in rng.integers(0, W, 2)))
    try:
        e = pkg.ORBextractor(**cfg)
    except pkg.OrbError as err:
        log("extract cfg rejected by the library: %s %s" % (cfg, err))
        return True
    try:
        o = oracle.OracleExtractor(**cfg)
        try:
            mono, kps, desc = e(img, None, lap)
        except (pkg.OrbError, ValueError) as err:   # documented limits of orbx_configure (include/orbhip.h): refused loudly, never wrong
            log("extract refused: %s %dx%d: %s" % (cfg, W, H, err))
            return True
        mono_r, kps_r, desc_r = o.extract(img, lap)
        cache.setdefault("stats", {}).setdefault("keypoints", []).append(len(kps_r))
        ok = mono == mono_r and len(kps) == len(kps_r)
        if ok:
            for f in ("x", "y", "size", "angle", "response", "octave"):
                ok = ok and np.array_equal(kps[f], kps_r[f])
            ok = ok and np.array_equal(desc, desc_r)
        if not ok:
            log("EXTRACT MISMATCH cfg=%s size=%dx%d lap=%s n=%d/%d mono=%s/%s" % (cfg, W, H, lap, len(kps), len(kps_r), mono, mono_r))
        return ok
    finally:
        e.close()


def fuzz_reuse(pkg, oracle, synth, rng, log, cache):
    """One long-lived extractor handle fed images of changing size: workspace re-sizing and re-capture of the per-frame hipGraph."""
    if "reuse" not in cache:
        cache["reuse"] = (pkg.ORBextractor(700, 1.2, 8, 20, 7), oracle.OracleExtractor(700, 1.2, 8, 20, 7))
    e, o = cache["reuse"]
    H, W = int(rng.integers(120, 500)), int(rng.integers(160, 760))
    img = random_image(rng, H, W, synth)
    lap = (0, 0) if rng.random() < 0.5 else (int(W * 0.25), int(W * 0.6))
    try:
        mono, kps, desc = e(img, None, lap)
    except (pkg.OrbError, ValueError) as err:
        log("reuse refused %dx%d: %s" % (W, H, err))
        return True
    mono_r, kps_r, desc_r = o.extract(img, lap)
    ok = mono == mono_r and len(kps) == len(kps_r) and np.array_equal(desc, desc_r)
    if ok:
        for f in ("x", "y", "angle", "response", "octave"):
            ok = ok and np.array_equal(kps[f], kps_r[f])
    if not ok:
        log("REUSE MISMATCH size=%dx%d lap=%s n=%d/%d" % (W, H, lap, len(kps), len(kps_r)))
    return ok


EUROC_K = np.array([458.654, 457.296, 367.215, 248.375], np.float32)                       # Examples/Monocular/EuRoC.yaml:9-12
EUROC_D = np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05], np.float32)       # EuRoC.yaml:14-17


def random_geometry(pkg, oracle, rng, keys, W=752, H=480):
    """The frame geometry as the Frame constructor makes it (Frame.cc:837-899, :379-380): with probability 0.3 the image rectangle
    and distorted = undistorted keypoints (zero distortion), else undistorted keypoints (EuRoC coefficients, or random ones of
    either sign) with the undistorted-corner bounds or - a third of those - arbitrary bounds with origin in [-80, 0] and an extent
    of at least the image.  Returns (keys_un, bounds, D)."""
    kind = rng.random()
    if kind < 0.3:
        return keys, (0.0, float(W), 0.0, float(H)), np.zeros(4, np.float32)
    if kind < 0.6:
        D = EUROC_D
    else:
        D = np.array([rng.uniform(-0.35, 0.25), rng.uniform(-0.1, 0.1), rng.uniform(-1e-3, 1e-3), rng.uniform(-1e-3, 1e-3)], np.float32)
    keys_un = pkg.undistort_keypoints(keys, EUROC_K, D)
    bounds = pkg.image_bounds(W, H, EUROC_K, D)
    if bounds != oracle.image_bounds(W, H, EUROC_K, D) and not any(np.isnan(b) for b in bounds):
        raise AssertionError("image bounds differ from the oracle for D=%s" % D)
    if not (np.isfinite(bounds).all() and bounds[1] > bounds[0] + 64 and bounds[3] > bounds[2] + 48 and np.isfinite(keys_un["x"]).all() and np.isfinite(keys_un["y"]).all()):
        # the 5-step iteration of cv::undistortPoints diverges in the corners for some coefficient draws (the reference would build a
        # frame with NaN bounds, which the library refuses): draw the headline calibration instead
        D = EUROC_D
        keys_un = pkg.undistort_keypoints(keys, EUROC_K, D)
        bounds = pkg.image_bounds(W, H, EUROC_K, D)
    if rng.random() < 0.33:
        bounds = tuple(float(np.float32(b)) for b in (rng.uniform(-80, 0), W + rng.uniform(0, 80), rng.uniform(-80, 0), H + rng.uniform(0, 80)))
    return keys_un, bounds, D


def fuzz_match(pkg, oracle, synth, rng, log, cache):
    if "frames" not in cache:
        frames, offs = synth.make_stream(77, 2)
        o = oracle.OracleExtractor(1000, 1.2, 8, 20, 7)
        cache["frames"] = [o.extract(f)[1:] for f in frames]
        cache["sf"] = o.scale_factors
        cache["offs"] = offs
    (k0, d0), (k1, d1) = cache["frames"]
    sf, offs = cache["sf"], cache["offs"]
    nc = int(rng.integers(1, len(k1) + 1))
    sel = np.sort(rng.choice(len(k1), nc, replace=False))
    kc, dc = k1[sel], d1[sel]
    nq = int(rng.integers(1, len(k0) + 1))
    qs = rng.choice(len(k0), nq, replace=rng.random() < 0.3)      # repeated queries: claims and ties
    kq, dq = k0[qs], d0[qs].copy()
    if rng.random() < 0.3:                                        # corrupt some descriptors: ratio test and TH_HIGH edges
        flip = rng.random(dq.shape) < 0.02
        dq ^= flip.astype(np.uint8) * rng.integers(1, 256, dq.shape, dtype=np.uint8)
    if rng.random() < 0.5:                                        # a few keypoints on the outermost pixels: undistorted, they leave the grid
        nb = int(rng.integers(1, 9))
        kc = kc.copy()
        pick = rng.choice(nc, min(nb, nc), replace=False)
        kc["x"][pick] = rng.choice(np.array([0.0, 0.5, 751.0, 751.5], np.float32), len(pick))
        kc["y"][pick] = rng.choice(np.array([0.0, 0.5, 479.0, 479.5], np.float32), len(pick))
    kc, bounds, D = random_geometry(pkg, oracle, rng, kc)
    kq = pkg.undistort_keypoints(kq, EUROC_K, D)
    F = pkg.FrameView(kc, dc, bounds)
    OF = oracle.OracleFrame(kc["x"], kc["y"], kc["octave"], kc["angle"], dc, bounds, sf)
    u = (kq["x"] + np.float32(offs[0][0] - offs[1][0]) + rng.normal(0, 2, nq)).astype(np.float32)
    v = (kq["y"] + np.float32(offs[0][1] - offs[1][1]) + rng.normal(0, 2, nq)).astype(np.float32)
    radius = rng.choice(np.array([0.5, 3, 7, 15, 40, 200, 1e4], np.float32), nq).astype(np.float32)
    lvl = kq["octave"].astype(np.int32)
    mode = rng.integers(0, 3)
    minl = lvl - 1 if mode == 0 else (np.full(nq, -1, np.int32) if mode == 1 else lvl)
    maxl = lvl + 1 if mode == 0 else (np.full(nq, -1, np.int32) if mode == 1 else lvl)
    occupied = rng.random(nc) < rng.choice([0.0, 0.1, 0.5])
    obs_occ = rng.random(nc) < 0.7
    qobs = (rng.random(nq) < rng.choice([1.0, 0.8, 0.3])).astype(np.uint8)
    in_view = (rng.random(nq) < 0.9).astype(np.uint8)
    nnratio = float(rng.choice([0.6, 0.75, 0.8, 0.9, 1.0]))
    th = int(rng.choice([30, 50, 100, 255]))   # 256 would accept "no candidate" (bestDist starts at 256): undefined in the reference
    second = bool(rng.integers(0, 2))
    for X in (F, OF):
        X.slot[:] = np.where(occupied, 1 << 20, -1)
        X.slot_obs[:] = (occupied & obs_occ).astype(np.uint8)
    m = cache.setdefault("matcher", pkg.ORBmatcher(0.8, True))
    flags = (in_view | (qobs << 1)).astype(np.uint8)
    n_gpu, moq_gpu, bd_gpu = m.search_window(F, dq, u, v, radius, minl, maxl, flags=flags, nnratio=nnratio, th_dist=th, use_second=second)
    n_ref, moq_ref, bd_ref = OF.search_by_projection_win(dq, u, v, radius, minl, maxl, nnratio, th, second, qobs=qobs, in_view=in_view)
    cache.setdefault("stats", {}).setdefault("window_matches", []).append(n_ref)
    ok = n_gpu == n_ref and np.array_equal(moq_gpu, moq_ref) and np.array_equal(F.slot, OF.slot) and np.array_equal(F.slot_obs, OF.slot_obs)
    if not ok:
        log("MATCH MISMATCH nq=%d nc=%d mode=%d nnratio=%s th=%d second=%s n=%d/%d bounds=%s D=%s" % (nq, nc, mode, nnratio, th, second, n_gpu, n_ref, bounds, D))
    return ok


def fuzz_last_frame(pkg, oracle, synth, rng, log, cache):
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:2027-2289): random pose, depths, camera model, stereo."""
    if "frames" not in cache:
        fuzz_match(pkg, oracle, synth, np.random.default_rng(0), log, cache)
    (k0, d0), (k1, d1) = cache["frames"]
    sf, offs = cache["sf"], cache["offs"]
    fx, fy, cx, cy = 458.654, 457.296, 367.215, 248.375
    n0 = len(k0)
    z = rng.uniform(1.5, 20.0, n0).astype(np.float32)
    Xw = np.stack([(k0["x"] - np.float32(cx)) / np.float32(fx) * z, (k0["y"] - np.float32(cy)) / np.float32(fy) * z, z], axis=1).astype(np.float32)
    Xw[rng.random(n0) < 0.03, 2] = -1.0
    ax = rng.normal(0, 1, 3); ax /= np.linalg.norm(ax)
    ang = rng.normal(0, 0.004)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    Tcw = np.eye(4, dtype=np.float32)
    Tcw[:3, :3] = R.astype(np.float32)
    dx, dy = offs[0][0] - offs[1][0], offs[0][1] - offs[1][1]
    stereo = bool(rng.integers(0, 2))
    Tcw[:3, 3] = [dx * 5.0 / fx + rng.normal(0, 0.01), dy * 5.0 / fy + rng.normal(0, 0.01), rng.choice([0.0, -0.3, 0.3]) if stereo else rng.normal(0, 0.05)]
    Tlw = np.eye(4, dtype=np.float32)
    has_mp = (rng.random(n0) < 0.8).astype(np.uint8)
    obs = (rng.random(n0) < 0.9).astype(np.uint8)
    cam = int(rng.integers(0, 2))
    if cam == 0:
        params = np.array([fx, fy, cx, cy], np.float32)
    else:
        params = np.array([190.978477 * 2, 190.973307 * 2, 376.0, 240.0, 0.003482389402, 0.000715034845, -0.002053236141, 0.000202936736], np.float32)
    u_right = None
    if stereo:
        u_right = np.where(rng.random(len(k1)) < 0.7, k1["x"] - np.float32(47.9) / np.float32(5.0), np.float32(-1)).astype(np.float32)
    k1, bounds, D = random_geometry(pkg, oracle, rng, k1)         # current frame: undistorted keypoints, undistorted-corner (or arbitrary) bounds
    th = float(rng.choice([7.0, 15.0, 30.0]))
    F = pkg.FrameView(k1, d1, bounds, u_right=u_right)
    OF = oracle.OracleFrame(k1["x"], k1["y"], k1["octave"], k1["angle"], d1, bounds, sf, u_right=u_right)
    mb, mbf = (0.11, 47.9) if stereo else (0.0, 0.0)
    m = cache.setdefault("matcher", pkg.ORBmatcher(0.8, True))
    n_gpu = m.SearchByProjectionLastFrame(F, sf, has_mp, Xw, d0, k0, Tcw, Tlw, cam, params, th, bMono=not stereo, mb=mb, mbf=mbf, mp_obs=obs)
    n_ref = OF.search_by_projection_ff(has_mp, Xw, d0, k0["octave"], k0["angle"], Tcw, Tlw, cam, params, th, mono=not stereo,
                                       check_ori=True, mb=mb, mbf=mbf, qobs=obs)
    cache.setdefault("stats", {}).setdefault("last_frame_matches", []).append(n_ref)
    ok = n_gpu == n_ref and np.array_equal(F.slot, OF.slot) and np.array_equal(F.slot_obs, OF.slot_obs)
    if not ok:
        log("LAST-FRAME MISMATCH cam=%d stereo=%s th=%s n=%d/%d bounds=%s D=%s" % (cam, stereo, th, n_gpu, n_ref, bounds, D))
    return ok


def _random_bow(rng, desc):
    """Stand-in for a DBoW2 FeatureVector: a random hash of descriptor bits into a random number of nodes (sparse, unordered ids)."""
    nodes = int(rng.choice([8, 32, 128, 512]))
    b0, b1 = int(rng.integers(0, 32)), int(rng.integers(0, 32))
    ids = ((desc[:, b0].astype(np.int64) >> 2) * 2 + (desc[:, b1].astype(np.int64) >> 7)) % nodes
    fv = {}
    for i, nid in enumerate(ids):
        fv.setdefault(int(nid) * 7 + 3, []).append(i)
    return fv


def fuzz_bow_and_triangulation(pkg, oracle, synth, rng, log, cache):
    """SearchByBoW (keyframe->frame, keyframe<->keyframe) and SearchForTriangulation on random keypoint subsets, vocabulary
    partitions, map-point masks, stereo coordinates and relative poses."""
    if "frames" not in cache:
        fuzz_match(pkg, oracle, synth, np.random.default_rng(0), log, cache)
    (k0, d0), (k1, d1) = cache["frames"]
    sf, offs = cache["sf"], cache["offs"]
    sigma2 = (sf * sf).astype(np.float32)
    s0 = np.sort(rng.choice(len(k0), int(rng.integers(1, len(k0) + 1)), replace=False))
    s1 = np.sort(rng.choice(len(k1), int(rng.integers(1, len(k1) + 1)), replace=False))
    ka, da, kb, db = k0[s0], d0[s0], k1[s1], d1[s1]
    fva, fvb = _random_bow(rng, da), _random_bow(rng, db)
    if rng.random() < 0.5:       # same hash on both sides: many shared nodes; otherwise mostly disjoint ones
        st = rng.bit_generator.state
        fva = _random_bow(rng, da); rng.bit_generator.state = st; fvb = _random_bow(rng, db)
    mpa = (rng.random(len(ka)) < rng.choice([0.2, 0.8, 1.0])).astype(np.uint8)
    mpb = (rng.random(len(kb)) < rng.choice([0.2, 0.8, 1.0])).astype(np.uint8)
    check_ori = bool(rng.integers(0, 2))
    ok = True
    # keyframe -> frame (:273-469)
    KF, F = pkg.KeyFrameView(ka, da, fva, sf, sigma2, has_mappoint=mpa), pkg.KeyFrameView(kb, db, fvb, sf, sigma2)
    OKF, OF = oracle.OracleKeyFrame(ka, da, fva, sf, sigma2, has_mp=mpa), oracle.OracleKeyFrame(kb, db, fvb, sf, sigma2)
    nn = float(rng.choice([0.6, 0.7, 0.9]))
    m = pkg.ORBmatcher(nn, check_ori)
    try:
        n_gpu, m_gpu = m.SearchByBoW(KF, F)
        n_ref, m_ref = oracle.search_by_bow(OKF, OF, nn, check_ori)
        if not (n_gpu == n_ref and np.array_equal(m_gpu, m_ref)):
            ok = False
            log("BOW KF-F MISMATCH n=%d/%d" % (n_gpu, n_ref))
        cache.setdefault("stats", {}).setdefault("bow_matches", []).append(n_ref)
        # keyframe <-> keyframe (:839-979)
        K2 = pkg.KeyFrameView(kb, db, fvb, sf, sigma2, has_mappoint=mpb)
        O2 = oracle.OracleKeyFrame(kb, db, fvb, sf, sigma2, has_mp=mpb)
        n_gpu, m_gpu = m.SearchByBoWKeyFrames(KF, K2)
        n_ref, m_ref = oracle.search_by_bow_keyframes(OKF, O2, nn, check_ori)
        if not (n_gpu == n_ref and np.array_equal(m_gpu, m_ref)):
            ok = False
            log("BOW KF-KF MISMATCH n=%d/%d" % (n_gpu, n_ref))
        # SearchForTriangulation (:981-1222), pinhole
        cam = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
        z = 5.0
        dx, dy = offs[0][0] - offs[1][0], offs[0][1] - offs[1][1]
        ang = rng.normal(0, 0.002)
        R1w, t1w = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        R2w = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], np.float32)
        t2w = np.array([dx * z / cam[0] + rng.normal(0, 0.01), dy * z / cam[1] + rng.normal(0, 0.01), rng.choice([0.02, -0.02, 0.1])], np.float32)
        Cw1 = np.zeros(3, np.float32)
        ura = np.where(rng.random(len(ka)) < 0.5, ka["x"] - np.float32(9.0), np.float32(-1)).astype(np.float32)
        urb = np.where(rng.random(len(kb)) < 0.5, kb["x"] - np.float32(9.0), np.float32(-1)).astype(np.float32)
        mta = (rng.random(len(ka)) < 0.2).astype(np.uint8); mtb = (rng.random(len(kb)) < 0.2).astype(np.uint8)
        T1 = pkg.KeyFrameView(ka, da, fva, sf, sigma2, u_right=ura, has_mappoint=mta)
        T2 = pkg.KeyFrameView(kb, db, fvb, sf, sigma2, u_right=urb, has_mappoint=mtb)
        P1 = oracle.OracleKeyFrame(ka, da, fva, sf, sigma2, u_right=ura, has_mp=mta)
        P2 = oracle.OracleKeyFrame(kb, db, fvb, sf, sigma2, u_right=urb, has_mp=mtb)
        only_stereo, coarse = bool(rng.random() < 0.25), bool(rng.random() < 0.3)
        n_gpu, pairs_gpu = m.SearchForTriangulation(T1, T2, R1w, t1w, R2w, t2w, Cw1, cam, cam, bOnlyStereo=only_stereo, bCoarse=coarse)
        n_ref, pairs_ref = oracle.search_for_triangulation(P1, P2, R1w, t1w, R2w, t2w, Cw1, cam, cam, only_stereo=only_stereo, coarse=coarse,
                                                           check_ori=check_ori)
        cache.setdefault("stats", {}).setdefault("triangulation_pairs", []).append(n_ref)
        if not (n_gpu == n_ref and np.array_equal(pairs_gpu, pairs_ref)):
            ok = False
            log("TRIANGULATION MISMATCH n=%d/%d stereo=%s coarse=%s" % (n_gpu, n_ref, only_stereo, coarse))
    finally:
        m.close()
    return ok


def fuzz_stereo(pkg, oracle, synth, rng, log, cache):
    """Frame::ComputeStereoMatches (Frame.cc:901-1079): random image sizes, disparities, noise between the two views, baselines."""
    H, W = int(rng.integers(160, 420)), int(rng.integers(240, 640))
    disp = int(rng.integers(1, 60))
    big = synth.make_frame(int(rng.integers(1, 1 << 30)), H, W + 64)
    imgL = np.ascontiguousarray(big[:, 0:W])
    imgR = np.ascontiguousarray(big[:, disp:disp + W])
    if rng.random() < 0.5:       # the right camera sees a slightly different image: SAD minima move, some matches fail
        imgR = (imgR.astype(np.int32) + rng.integers(-6, 7, imgR.shape)).clip(0, 255).astype(np.uint8)
    if rng.random() < 0.3:       # one row of vertical misalignment
        imgR = np.roll(imgR, 1, axis=0)
    cfg = dict(nfeatures=int(rng.choice([300, 800, 1200])), scaleFactor=1.2, nlevels=int(rng.integers(3, 9)), iniThFAST=20, minThFAST=7)
    try:
        exL, exR = pkg.ORBextractor(**cfg), pkg.ORBextractor(**cfg)
    except (pkg.OrbError, ValueError):
        return True
    try:
        try:
            _, kL, dL = exL(imgL, None, (0, 0))
            _, kR, dR = exR(imgR, None, (0, 0))
        except (pkg.OrbError, ValueError) as err:
            log("stereo refused %dx%d: %s" % (W, H, err))
            return True
        mbf = float(rng.uniform(20.0, 80.0)); mb = mbf / float(rng.uniform(300.0, 500.0))
        uR_gpu, z_gpu = exL.ComputeStereoMatches(exR, kL, dL, kR, dR, mb, mbf)
        o = oracle.OracleExtractor(**cfg)
        uR_ref, z_ref = o.compute_stereo_matches(imgL, imgR, kL, dL, kR, dR, mb, mbf)
        cache.setdefault("stats", {}).setdefault("stereo_matches", []).append(int((uR_ref >= 0).sum()))
        ok = np.array_equal(uR_gpu.view(np.uint32), uR_ref.view(np.uint32)) and np.array_equal(z_gpu.view(np.uint32), z_ref.view(np.uint32))
        if not ok:
            log("STEREO MISMATCH %dx%d disp=%d cfg=%s: %d differing" % (W, H, disp, cfg, int((uR_gpu.view(np.uint32) != uR_ref.view(np.uint32)).sum())))
        return ok
    finally:
        exL.close(); exR.close()


def fuzz_batch_open(pkg, oracle, synth, rng, log, cache):
    """Batch launches of the window search (orbm_search_by_projection_batch_device) with 9-14 frame pairs: most pairs search
    open windows (the matrix-pipe scan / the fused resolve, orbm_set_hamming_engine 1 / 2), some are windowed, partly windowed or
    dead; random keypoint subsets, duplicated descriptors, pre-occupied keypoints, keypoints outside the grid, query flags,
    thresholds, bounds.  One engine per case (drawn), every pair against the oracle's in-order loop."""
    import test_gpu_mfma as T
    if "frames" not in cache:
        fuzz_match(pkg, oracle, synth, np.random.default_rng(0), log, cache)
    (k0, d0), (k1, d1) = cache["frames"]
    sf, offs = cache["sf"], cache["offs"]
    npairs = int(rng.integers(9, 15))
    kc_all, bounds, D = random_geometry(pkg, oracle, rng, k1)
    kq_all = pkg.undistort_keypoints(k0, EUROC_K, D)
    cand, qry = [], []
    for p in range(npairs):
        nc = int(rng.choice([1, 17, 33, 200, 640, len(k1), len(k1), len(k1)]))
        sel = np.sort(rng.choice(len(k1), nc, replace=False))
        kc, dc = kc_all[sel].copy(), d1[sel].copy()
        if rng.random() < 0.5 and nc > 20:
            dup = rng.random(nc) < 0.4
            dc[dup] = dc[rng.integers(0, nc, int(dup.sum()))]
        if rng.random() < 0.3 and nc > 8:
            out = rng.choice(nc, 3, replace=False)
            kc["x"][out] = np.float32(bounds[0] - 30.0)
        c = T.free_frame(kc, dc)
        occ = rng.random(nc) < rng.choice([0.0, 0.2, 0.6])
        c["slot"][occ] = 1 << 20
        c["sobs"][occ] = rng.random(int(occ.sum())) < 0.6
        cand.append(c)
        nq = int(rng.choice([1, 40, 256, 257, 600, len(k0), len(k0)]))
        qs = rng.choice(len(k0), nq, replace=rng.random() < 0.3)
        q = T.open_queries(kq_all[qs], d0[qs].copy(), (offs[0][0] - offs[1][0], offs[0][1] - offs[1][1]))
        q["u"] = (q["u"] + rng.normal(0, 2, nq)).astype(np.float32)
        inv = (rng.random(nq) < 0.93).astype(np.uint8); obs = (rng.random(nq) < rng.choice([1.0, 0.7])).astype(np.uint8)
        q["flags"] = (inv | (obs << 1)).astype(np.uint8)
        kind = rng.random()
        if kind < 0.15:                                   # the whole pair windowed
            q["r"][:] = rng.choice([10.0, 25.0, 60.0]); lvl = kq_all[qs]["octave"].astype(np.int32); q["lo"] = lvl - 1; q["hi"] = lvl + 1
        elif kind < 0.3 and nq > 10:                      # a few windowed queries: their block is not open
            w = rng.choice(nq, max(1, nq // 20), replace=False)
            q["r"][w] = 30.0; q["lo"][w] = 0; q["hi"][w] = 4
        elif kind < 0.4:                                  # a smaller radius that still covers the grid for most queries only
            q["r"][:] = 1200.0
        qry.append(q)
    nnratio, th, second = float(rng.choice([0.6, 0.8, 1.0])), int(rng.choice([40, 100, 255])), bool(rng.integers(0, 2))
    engine = int(rng.integers(0, 3))
    ref = [T.oracle_pair(oracle, c, q, bounds, sf, nnratio, th, second) for c, q in zip(cand, qry)]
    m = pkg.ORBmatcher(nnratio, True)
    try:
        m.set_hamming_engine(engine)
        got = T.run_batch(pkg, m, cand, qry, bounds, nnratio, th, second)
    finally:
        m.close()
    ok = True
    for p, (g, r) in enumerate(zip(got, ref)):
        if not (g[0] == r[0] and np.array_equal(g[1], r[1]) and np.array_equal(g[2], r[2]) and np.array_equal(g[3], r[3]) and np.array_equal(g[4], r[4])):
            ok = False
            log("BATCH MISMATCH engine=%d pair %d of %d n=%d nq=%d nnratio=%s th=%d second=%s n=%d/%d" % (engine, p, npairs, len(cand[p]["k"]), len(qry[p]["u"]), nnratio, th, second, g[0], r[0]))
    cache.setdefault("stats", {}).setdefault("batch_matches", []).append(int(np.mean([r[0] for r in ref])))
    return ok


def fuzz_batch_extract(pkg, oracle, synth, rng, log, cache):
    """orbx_extract_batch_device on 1-12 distinct frames laid out at random in one device buffer: base offset, row padding and gaps
    between frames (aligned and unaligned level-0 planes, often both in one launch), random padding bytes; a random configuration as
    in fuzz_extract on small frames.  Every frame against the oracle."""
    import torch
    H, W = int(rng.integers(64, 241)), int(rng.integers(64, 321))
    cfg = dict(nfeatures=int(rng.choice([30, 200, 500, 1000, 1500])), scaleFactor=float(rng.choice([1.1, 1.2, 1.25, 1.5, 2.0])),
               nlevels=int(rng.integers(1, 17)), iniThFAST=int(rng.integers(8, 41)), minThFAST=int(rng.integers(2, 12)))
    cfg["minThFAST"] = min(cfg["minThFAST"], cfg["iniThFAST"])
    n = int(rng.integers(1, 13))
    frames = [np.ascontiguousarray(random_image(rng, H, W, synth)) for _ in range(n)]
    off, stride = int(rng.integers(0, 8)), W + int(rng.choice([0, 0, int(rng.integers(1, 10)), 64]))
    fs = H * stride + int(rng.choice([0, 0, int(rng.integers(1, 8)), int(rng.integers(8, 300))]))
    lap = (0, 0) if rng.random() < 0.5 else tuple(sorted(int(v) for v in rng.integers(0, W, 2)))
    buf = rng.integers(0, 256, off + (n - 1) * fs + (H - 1) * stride + W, dtype=np.uint8)
    for k, f in enumerate(frames):
        for y in range(H):
            buf[off + k * fs + y * stride:off + k * fs + y * stride + W] = f[y]
    try:
        e = pkg.ORBextractor(**cfg)
    except pkg.OrbError as err:
        log("batch cfg rejected by the library: %s %s" % (cfg, err))
        return True
    try:
        try:
            cap = e.configure(H, W, n)
        except ValueError as err:   # documented limits of orbx_configure: refused loudly, never wrong
            log("batch refused: %s %dx%d: %s" % (cfg, W, H, err))
            return True
        d_buf = torch.from_numpy(buf).cuda()
        d_kps = torch.zeros((n, cap, 7), dtype=torch.int32, device="cuda")
        d_desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        e.extract_batch_device(d_buf.data_ptr() + off, H, W, stride, fs, n, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), cap, lap,
                               stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        cnt, kps, desc = d_cnt.cpu().numpy(), d_kps.cpu().numpy(), d_desc.cpu().numpy()
        ok = np.array_equal(d_buf.cpu().numpy(), buf)
        if not ok:
            log("BATCH EXTRACT wrote its input: cfg=%s size=%dx%d n=%d" % (cfg, W, H, n))
        o = oracle.OracleExtractor(**cfg)
        for k, img in enumerate(frames):
            mono_r, kps_r, desc_r = o.extract(img, lap)
            m = int(cnt[k, 0])
            if not (m == len(kps_r) and int(cnt[k, 1]) == mono_r and kps[k, :m].tobytes() == kps_r.tobytes() and np.array_equal(desc[k, :m], desc_r)):
                ok = False
                log("BATCH EXTRACT MISMATCH cfg=%s size=%dx%d n=%d frame %d offset=%d stride=%d frame_stride=%d lap=%s n=%d/%d" %
                    (cfg, W, H, n, k, off, stride, fs, lap, m, len(kps_r)))
        return ok
    finally:
        e.close()


def run(pkg, oracle, synth, n, seed, log=lambda msg: print(msg, flush=True), first=0, verbose=False):
    """Cases first .. first+n-1 of stream `seed`; every case draws from its own generator, so one case can be replayed alone."""
    bad, cache, t0 = 0, {}, time.time()
    try:
        for i in range(first, first + n):
            if verbose:
                log("case %d" % i)
            ok1 = fuzz_extract(pkg, oracle, synth, np.random.default_rng([seed, i, 0]), log, cache)
            ok2 = fuzz_match(pkg, oracle, synth, np.random.default_rng([seed, i, 1]), log, cache)
            ok3 = fuzz_last_frame(pkg, oracle, synth, np.random.default_rng([seed, i, 2]), log, cache)
            ok4 = fuzz_reuse(pkg, oracle, synth, np.random.default_rng([seed, i, 3]), log, cache)
            ok5 = fuzz_bow_and_triangulation(pkg, oracle, synth, np.random.default_rng([seed, i, 4]), log, cache)
            ok6 = fuzz_stereo(pkg, oracle, synth, np.random.default_rng([seed, i, 5]), log, cache)
            ok7 = fuzz_batch_open(pkg, oracle, synth, np.random.default_rng([seed, i, 6]), log, cache)
            ok8 = fuzz_batch_extract(pkg, oracle, synth, np.random.default_rng([seed, i, 7]), log, cache)
            if not (ok1 and ok2 and ok3 and ok4 and ok5 and ok6 and ok7 and ok8):
                log("   ^ case %d of seed %d" % (i, seed))
            bad += (not ok1) + (not ok2) + (not ok3) + (not ok4) + (not ok5) + (not ok6) + (not ok7) + (not ok8)
            if (i + 1 - first) % 20 == 0:
                log("%d / %d cases, %d mismatches, %.0f s" % (i + 1 - first, n, bad, time.time() - t0))
    finally:
        if "matcher" in cache:
            cache["matcher"].close()
        if "reuse" in cache:
            cache["reuse"][0].close()
    for k, v in cache.get("stats", {}).items():
        log("   %s: %d cases, mean %.0f, min %d, max %d" % (k, len(v), np.mean(v), min(v), max(v)))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--verbose", action="store_true")
    args = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    synth = importlib.import_module("3_orb_slam3_selfnote_amd.synth")
    from oracle import oracle_py as oracle   # the checker
    bad = run(pkg, oracle, synth, args.n, args.seed, first=args.first, verbose=args.verbose)
    print("fuzz: %d cases each of: extractor configuration, window search, last-frame search, handle reuse, BoW x2 + triangulation, stereo matches, batch search (all three Hamming engines), batched extraction at random layouts; %d mismatches" % (args.n, bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
