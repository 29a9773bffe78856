"""orbx_stereo_from_rgbd_batch_device (Frame::ComputeStereoFromRGBD, Frame.cc:1082-1103) and orbx_close_points_batch_device (the
depth-ordered rule of Tracking.cc:2808-2860 / :3345-3416, the close counts of :3190-3200, Frame::UnprojectStereo) for frames that
stay on the device.

Reference everywhere: the literal-loop numpy model of tests/rgbd_model.py, compared by bit pattern; entries the calls must leave
alone (beyond N, beyond nvisit, keypoints without depth) keep a sentinel.  tests/test_rgbd_abi.py holds the conditions under which
the synthetic scenes of the chain test exercise the rule."""
import ctypes as C

import numpy as np
import pytest

import rgbd_model as RM

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-777.25)
ISENT = -12345
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.names:                                    # keypoints: 28 bytes each
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return torch.from_numpy(a).cuda()


def sentinel(shape, dtype=np.float32):
    import torch
    if dtype == np.float32:
        return torch.full(shape, float(SENTINEL), dtype=torch.float32, device="cuda")
    return torch.full(shape, ISENT, dtype=torch.int32, device="cuda")


# ---- 1: the lookup on hand-made keypoints ---------------------------------------------------------------------------------------
H1, W1, CAP1 = 48, 64, 40
COUNTS1 = (0, 1, 37)
# (x, y, value planted at the pixel of a float image).  The pixel is (int(y), int(x)); "in" = an ordinary depth, "out" = no pixel.
SPECIAL = [(12.999999, 7.9999995, "in"),            # fractions just below an integer: column 12, row 7
           (63.99999, 47.99999, "in"),              # the last column and row
           (0.0, 0.0, "in"), (-0.5, 3.0, "in"),     # -0.5 truncates to column 0
           (64.0, 10.0, "out"), (5.0, 48.0, "out"), (-1.0, 5.0, "out"), (20.0, -1.5, "out"),   # outside: -1, never read
           (3.0, 4.0, 0.0), (4.0, 4.0, -0.0), (5.0, 4.0, -2.5), (6.0, 4.0, np.nan), (7.0, 4.0, np.inf), (8.0, 4.0, -np.inf),
           (9.0, 4.0, 1e-39), (10.0, 4.0, 3e-42),   # denormals: times 1 / 5000 still positive, or rounded to zero
           (11.0, 4.0, 65535.0), (12.0, 4.0, 1.0)]


def lookup_case(pkg, depth_type):
    """Three frames of keypoints and depth images; frame 2 starts with the special coordinates and values."""
    rng = np.random.default_rng(17)
    keys = np.zeros((3, CAP1), pkg.KP_DTYPE)
    keys_un = np.zeros((3, CAP1), pkg.KP_DTYPE)
    raw = np.stack([RM.depth_u16(40 + f, H1, W1) for f in range(3)])
    raw[2, 30:34, 30:34] = (0, 1, 65535, 30000)
    img = raw.astype(np.float32) if depth_type == 1 else raw
    for f, n in enumerate(COUNTS1):
        xs, ys = rng.uniform(0, W1, CAP1).astype(np.float32), rng.uniform(0, H1, CAP1).astype(np.float32)
        if f == 2:
            for i, (x, y, val) in enumerate(SPECIAL):
                xs[i], ys[i] = x, y
                if val == "in":
                    img[2, int(y), int(x)] = 12345
                elif val != "out":
                    img[2, int(y), int(x)] = val if depth_type == 1 else (0, 65535, 1, 2)[i % 4]
            xs[len(SPECIAL):len(SPECIAL) + 4] = (30.5, 31.5, 32.5, 33.5)
            ys[len(SPECIAL):len(SPECIAL) + 4] = (30.5, 31.5, 32.5, 33.5)
        keys["x"][f], keys["y"][f] = xs, ys
        keys_un["x"][f], keys_un["y"][f] = xs + np.float32(0.37), ys - np.float32(0.21)
    return keys, keys_un, img


@pytest.mark.parametrize("depth_type,pad,factor,nstereo", [(0, 0, RM.TUM1_FACTOR, True), (0, 6, RM.TUM1_FACTOR, False), (1, 0, RM.TUM1_FACTOR, True),
                                                           (1, 12, np.float32(1.0), True)])
def test_lookup_hand_made(pkg, depth_type, pad, factor, nstereo):
    """1: three frames (0, 1 and 37 keypoints) on 48 x 64 depth images of both types, with and without row padding, with and without
    d_nstereo, factor 1 on float input: truncated coordinates, the image's last row and column, pixels outside, and every kind of
    depth value (0, -0, negative, NaN, +-inf, denormal products, 65535)."""
    import torch
    keys, keys_un, img = lookup_case(pkg, depth_type)
    assert len(SPECIAL) + 4 <= COUNTS1[2]
    elem = img.dtype.itemsize
    padded = np.full((3, H1, W1 + pad // elem), 9, img.dtype)       # the padding holds a positive depth: reading it would show
    padded[:, :, :W1] = img
    cnt = np.array([[n, -7] for n in COUNTS1], np.int32)
    d_keys, d_un, d_cnt, d_img = to_dev(keys), to_dev(keys_un), to_dev(cnt), to_dev(padded)
    d_uR, d_z, d_ns = sentinel((3, CAP1)), sentinel((3, CAP1)), sentinel((3,), np.int32)
    rc = pkg.stereo_from_rgbd_batch_device(3, d_keys.data_ptr(), d_un.data_ptr(), d_cnt.data_ptr(), 2, CAP1, d_img.data_ptr(), depth_type, H1, W1,
                                           padded.strides[1], padded.strides[0], float(factor), float(RM.TUM1_BF), d_uR.data_ptr(), d_z.data_ptr(),
                                           d_ns.data_ptr() if nstereo else None)
    assert rc == 0
    torch.cuda.synchronize()
    uR, z, ns = d_uR.cpu().numpy(), d_z.cpu().numpy(), d_ns.cpu().numpy()
    kinds = set()
    for f, n in enumerate(COUNTS1):
        uR_m, z_m = RM.compute_stereo_from_rgbd(keys[f, :n], keys_un[f, :n], img[f], factor, RM.TUM1_BF)
        bad = np.nonzero((bits(uR[f, :n]) != bits(uR_m)) | (bits(z[f, :n]) != bits(z_m)))[0]
        assert len(bad) == 0, (f, [(int(i), float(keys["x"][f, i]), float(keys["y"][f, i]), float(z[f, i]), float(z_m[i]), float(uR[f, i]), float(uR_m[i])) for i in bad[:4]])
        assert (uR[f, n:] == SENTINEL).all() and (z[f, n:] == SENTINEL).all()
        assert ns[f] == (int((z_m > 0).sum()) if nstereo else ISENT)
        if f == 2:
            assert (z_m[4:8] == -1).all() and z_m[0] > 0 and z_m[1] > 0 and z_m[2] > 0 and z_m[3] > 0
            if depth_type == 1:
                assert (z_m[8:12] == -1).all() and np.isinf(z_m[12]) and uR_m[12] == keys_un["x"][2, 12] and z_m[13] == -1
                assert z_m[14] > 0 if factor == 1 else (0 < z_m[14] < 1e-40 and np.isinf(uR_m[14]))
                assert z_m[15] > 0 if factor == 1 else z_m[15] == -1
                assert z_m[16] == np.float32(65535.0) * factor
        kinds |= {"none"} if n == 0 else {"some"}
    assert kinds == {"none", "some"}


# ---- 2: the selection on hand-made depths ---------------------------------------------------------------------------------------
CAP2 = 320


def selection_frames():
    """One frame per (m, c) of tests/test_rgbd_abi.py::test_closed_form_equals_the_loop, then the special ones."""
    th = RM.TEST_TH_DEPTH
    rng = np.random.default_rng(29)
    frames = []
    for m in (0, 1, 99, 100, 101, 102, 300):
        for c in sorted(set(min(c, m) for c in (0, 99, 100, 101, m))):
            close = rng.uniform(0.4, 3.1, c).astype(np.float32)
            if c:
                close[0] = th                                                   # exactly on the threshold: close for the break, not for the counts
            if c > 10:
                close[1:9] = close[9]                                           # equal depths: the index decides
            far = (th + rng.uniform(0.001, 5.0, m - c)).astype(np.float32)
            z = np.concatenate([close, far, np.array([0, -1, np.nan], np.float32)])
            frames.append(z[rng.permutation(len(z))])
    frames.append(np.full(150, 2.5, np.float32))                                # all equal, all close: order = index
    frames.append(np.full(150, 4.5, np.float32))                                # all equal, all far: the first max_point + 1 indices
    z = rng.uniform(0.4, 6.0, 200).astype(np.float32)
    z[rng.choice(200, 12, replace=False)] = np.inf                              # +inf sorts last, ties by index
    frames.append(z)
    z = rng.uniform(0.4, 3.0, 60).astype(np.float32)
    z[rng.choice(60, 50, replace=False)] = np.inf                               # fewer than 100 finite: the infinite ones are visited
    frames.append(z)
    frames.append(np.array([0, -1, -np.inf, np.nan, -0.0] * 8, np.float32))     # only non-positive depths: nvisit 0
    frames.append(np.zeros(0, np.float32))                                      # N = 0
    frames.append(rng.uniform(0.4, 6.0, CAP2).astype(np.float32))               # N = cap
    return frames


@pytest.mark.parametrize("max_point,tracked,unproject", [(100, True, "world"), (0, False, "none"), (100, False, "camera"), (0, True, "world")])
def test_selection_hand_made(pkg, max_point, tracked, unproject):
    """2: 29 frames in one call: every (m, c) of the closed-form test, equal depths, a depth exactly on the threshold, +inf, frames
    without any depth, N = 0 and N = cap; max_point 100 and 0, d_tracked given and NULL, no unprojection / camera / camera + world."""
    import torch
    frames = selection_frames()
    nf = len(frames)
    rng = np.random.default_rng(31)
    depth = np.full((nf, CAP2), 1.0, np.float32)         # beyond N: a close depth that must not be looked at
    cnt = np.zeros((nf, 2), np.int32)
    for f, z in enumerate(frames):
        depth[f, :len(z)] = z
        cnt[f] = (len(z), 99)
    keys_un = np.zeros((nf, CAP2), pkg.KP_DTYPE)
    keys_un["x"], keys_un["y"] = rng.uniform(0, 640, (nf, CAP2)).astype(np.float32), rng.uniform(0, 480, (nf, CAP2)).astype(np.float32)
    trk = (rng.random((nf, CAP2)) < 0.4).astype(np.uint8)
    pose = rng.normal(0, 1, (nf, 3, 4)).astype(np.float32)
    th = RM.TEST_TH_DEPTH
    d_z, d_cnt, d_un, d_trk, d_pose = to_dev(depth), to_dev(cnt), to_dev(keys_un), to_dev(trk), to_dev(pose)
    d_order, d_nv, d_close = sentinel((nf, CAP2), np.int32), sentinel((nf,), np.int32), sentinel((nf, 2), np.int32)
    d_xc, d_xw = sentinel((nf, CAP2, 3)), sentinel((nf, CAP2, 3))
    kw = {}
    if unproject != "none":
        kw = dict(d_keys_un=d_un.data_ptr(), fx=float(RM.TUM1_K[0]), fy=float(RM.TUM1_K[1]), cx=float(RM.TUM1_K[2]), cy=float(RM.TUM1_K[3]), d_x3Dc=d_xc.data_ptr())
    if unproject == "world":
        kw.update(d_pose=d_pose.data_ptr(), d_x3Dw=d_xw.data_ptr())
    rc = pkg.close_points_batch_device(nf, d_z.data_ptr(), d_cnt.data_ptr(), 2, CAP2, float(th), max_point, d_order.data_ptr(), d_nv.data_ptr(),
                                       d_tracked=d_trk.data_ptr() if tracked else None, d_close=d_close.data_ptr() if tracked or unproject == "camera" else None, **kw)
    assert rc == 0
    torch.cuda.synchronize()
    order, nv, close, xc, xw = d_order.cpu().numpy(), d_nv.cpu().numpy(), d_close.cpu().numpy(), d_xc.cpu().numpy(), d_xw.cpu().numpy()
    seen = set()
    for f, z in enumerate(frames):
        n = len(z)
        want, nt, nn = RM.close_points(z, th, max_point, trk[f] if tracked else None)
        assert nv[f] == len(want), (f, nv[f], len(want))
        assert order[f, :nv[f]].tolist() == want, f
        assert (order[f, nv[f]:] == ISENT).all(), f
        if tracked or unproject == "camera":
            assert close[f].tolist() == [nt, nn], (f, close[f], nt, nn)
        else:
            assert (close[f] == ISENT).all()
        has = np.zeros(CAP2, bool)
        has[:n] = z > 0
        xc_m, xw_m = RM.unproject_stereo(keys_un[f, :n], z, RM.TUM1_K, pose[f] if unproject == "world" else None)
        if unproject == "none":
            assert (xc[f] == SENTINEL).all()
        else:
            assert np.array_equal(bits(xc[f][has]), bits(xc_m[z > 0])) and (xc[f][~has] == SENTINEL).all(), f
        if unproject == "world":
            assert np.array_equal(bits(xw[f][has]), bits(xw_m[z > 0])) and (xw[f][~has] == SENTINEL).all(), f
        else:
            assert (xw[f] == SENTINEL).all()
        m, c = int((z > 0).sum()), int(((z > 0) & (z <= th)).sum())
        seen.add("all" if len(want) == m else ("close+1" if c > max_point else "max_point+1"))
    assert seen == {"all", "close+1", "max_point+1"}
    assert nv[nf - 7] == 150 and order[nf - 7, :150].tolist() == list(range(150))                                    # all equal and close
    assert nv[nf - 6] == max_point + 1 and order[nf - 6, :max_point + 1].tolist() == list(range(max_point + 1))      # all equal and far
    assert nv[nf - 3] == 0 and nv[nf - 2] == 0                                                                       # non-positive only, and N = 0


def test_selection_up_to_the_limit(pkg):
    """cap = ORBX_CLOSE_MAX_KEYPOINTS with N = cap, N = 1500 and N = 1025: the sizes at which a thread holds more than one key of a
    sorting step, powers of two and not.  Depths in steps of 1 / 64, so most keypoints share theirs."""
    import torch
    cap = pkg.CLOSE_MAX_KEYPOINTS
    rng = np.random.default_rng(37)
    ns = (cap, 1500, 1025)
    depth = (rng.integers(-8, 400, (3, cap)) / 64.0).astype(np.float32)
    cnt = np.array([[n] for n in ns], np.int32)
    d_z, d_cnt = to_dev(depth), to_dev(cnt)
    d_order, d_nv = sentinel((3, cap), np.int32), sentinel((3,), np.int32)
    assert pkg.close_points_batch_device(3, d_z.data_ptr(), d_cnt.data_ptr(), 1, cap, float(RM.TEST_TH_DEPTH), 100, d_order.data_ptr(), d_nv.data_ptr()) == 0
    torch.cuda.synchronize()
    order, nv = d_order.cpu().numpy(), d_nv.cpu().numpy()
    for f, n in enumerate(ns):
        want = RM.close_points(depth[f, :n], RM.TEST_TH_DEPTH, 100)[0]
        assert len(want) > n // 3 and nv[f] == len(want)
        assert order[f, :nv[f]].tolist() == want and (order[f, nv[f]:] == ISENT).all()


# ---- 3: the chain ------------------------------------------------------------------------------------------------------------------
def test_chain_on_one_stream(pkg, oracle, synth):
    """Two TUM1 frames: extract -> undistort -> lookup -> selection (with the unprojection) -> stereo-mode last-frame search, on a
    stream of the caller's with one synchronise at the end.  The last frame of each problem is the frame itself, its map points the
    unprojected keypoints (identity poses), so every map point with depth projects onto its keypoint and passes the
    right-coordinate gate (ORBmatcher.cc:2139-2146) only if d_uRight is what the model says."""
    import torch
    H, W, n = 480, 640, 2
    scenes = [RM.scene(oracle, synth, s, H, W) for s in (1000, 1001)]
    K, D = RM.TUM1_K, RM.TUM1_D
    bounds = pkg.image_bounds(W, H, K, D)
    mbf = float(RM.TUM1_BF); mb = float(RM.TUM1_BF / K[0]); th = RM.TEST_TH_DEPTH
    ex, m = pkg.ORBextractor(**RM.TUM1), pkg.ORBmatcher(0.9, True)
    cap = ex.configure(H, W, n)
    assert cap <= pkg.CLOSE_MAX_KEYPOINTS
    sf = scenes[0]["scale_factors"]
    eye4 = np.stack([np.eye(4, dtype=np.float32).reshape(-1)] * n)
    eye34 = np.stack([np.eye(4, dtype=np.float32)[:3].reshape(-1)] * n)
    pad = lambda a, fill: np.concatenate([a, np.full((cap - len(a),) + a.shape[1:], fill, a.dtype)])
    st = torch.cuda.Stream()
    s = st.cuda_stream
    with torch.cuda.stream(st):
        d_img, d_raw = to_dev(np.stack([S["img"] for S in scenes])), to_dev(np.stack([S["raw"] for S in scenes]))
        d_has = to_dev(np.stack([pad((S["depth"] > 0).astype(np.uint8), 0) for S in scenes]))
        d_uR_model = to_dev(np.stack([pad(S["uRight"], -1) for S in scenes]))
        d_T, d_pose = to_dev(eye4), to_dev(eye34)
        d_k = torch.zeros((n, cap, 7), dtype=torch.float32, device="cuda")
        d_d = torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda")
        d_c = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        d_un = torch.zeros((n, cap, 7), dtype=torch.float32, device="cuda")
        d_uR, d_z, d_ns = sentinel((n, cap)), sentinel((n, cap)), sentinel((n,), np.int32)
        d_order, d_nv, d_close = sentinel((n, cap), np.int32), sentinel((n,), np.int32), sentinel((n, 2), np.int32)
        d_xc, d_xw = sentinel((n, cap, 3)), sentinel((n, cap, 3))
        ex.extract_batch_device(d_img.data_ptr(), H, W, W, H * W, n, d_k.data_ptr(), d_d.data_ptr(), d_c.data_ptr(), cap, (0, 0), stream=s)
        m.undistort_batch_device(d_k.data_ptr(), cap, d_c.data_ptr(), 2, n, K, D, d_un.data_ptr(), stream=s)
        pkg.stereo_from_rgbd_batch_device(n, d_k.data_ptr(), d_un.data_ptr(), d_c.data_ptr(), 2, cap, d_raw.data_ptr(), 0, H, W, 2 * W, 2 * W * H,
                                          float(RM.TUM1_FACTOR), mbf, d_uR.data_ptr(), d_z.data_ptr(), d_ns.data_ptr(), stream=s)
        pkg.close_points_batch_device(n, d_z.data_ptr(), d_c.data_ptr(), 2, cap, float(th), 100, d_order.data_ptr(), d_nv.data_ptr(), d_close=d_close.data_ptr(),
                                      d_keys_un=d_un.data_ptr(), fx=float(K[0]), fy=float(K[1]), cx=float(K[2]), cy=float(K[3]), d_x3Dc=d_xc.data_ptr(),
                                      d_pose=d_pose.data_ptr(), d_x3Dw=d_xw.data_ptr(), stream=s)
        results = []
        for d_ur in (d_uR, d_uR_model):
            d_slot = torch.full((n, cap), -1, dtype=torch.int32, device="cuda")
            d_sobs = torch.zeros((n, cap), dtype=torch.uint8, device="cuda")
            d_nm = torch.zeros((n,), dtype=torch.int32, device="cuda")
            cur = pkg.FrameStruct(cap, d_un.data_ptr(), d_d.data_ptr(), d_ur.data_ptr(), *[C.c_float(b) for b in bounds])
            last = pkg.LastFrameStruct(cap, d_has.data_ptr(), d_xw.data_ptr(), d_d.data_ptr(), d_k.data_ptr(), None, d_T.data_ptr(), d_T.data_ptr())
            rc = m.L.orbm_search_by_projection_last_frame_batch_device(
                m.m, C.byref(cur), cap, C.c_void_p(d_c.data_ptr()), 2, C.byref(last), cap, C.c_void_p(d_c.data_ptr()), 2, n, sf.ctypes.data_as(C.c_void_p), len(sf),
                0, K.ctypes.data_as(C.c_void_p), C.c_float(mb), C.c_float(mbf), C.c_float(7.0), 0, 1, C.c_void_p(d_slot.data_ptr()), C.c_void_p(d_sobs.data_ptr()),
                None, C.c_void_p(d_nm.data_ptr()), C.c_void_p(s))
            assert rc == 0, m.L.orbm_last_error(m.m)
            results.append((d_slot, d_sobs, d_nm))
    torch.cuda.synchronize()          # the one synchronisation of the chain
    cnt, keys, desc = d_c.cpu().numpy(), d_k.cpu().numpy().view(np.uint8).reshape(n, cap, 28), d_d.cpu().numpy()
    uR, z, ns, order, nv, close = [t.cpu().numpy() for t in (d_uR, d_z, d_ns, d_order, d_nv, d_close)]
    xc, xw = d_xc.cpu().numpy(), d_xw.cpu().numpy()
    for f, S in enumerate(scenes):
        N = len(S["keys"])
        assert cnt[f, 0] == N and keys[f, :N].tobytes() == S["keys"].tobytes() and np.array_equal(desc[f, :N], S["desc"])
        assert np.array_equal(bits(uR[f, :N]), bits(S["uRight"])) and np.array_equal(bits(z[f, :N]), bits(S["depth"]))
        assert (uR[f, N:] == SENTINEL).all() and (z[f, N:] == SENTINEL).all() and ns[f] == int((S["depth"] > 0).sum())
        want, nt, nn = RM.close_points(S["depth"], th, 100)
        assert nv[f] == len(want) > 101 and order[f, :nv[f]].tolist() == want and (order[f, nv[f]:] == ISENT).all()
        assert close[f].tolist() == [nt, nn]
        has = S["depth"] > 0
        xc_m, xw_m = RM.unproject_stereo(S["keys_un"], S["depth"], K, np.eye(4, dtype=np.float32)[:3])
        assert np.array_equal(bits(xc[f, :N][has]), bits(xc_m[has])) and np.array_equal(bits(xw[f, :N][has]), bits(xw_m[has]))
        assert (xc[f, :N][~has] == SENTINEL).all() and (xc[f, N:] == SENTINEL).all()
    (slot_a, sobs_a, nm_a), (slot_b, sobs_b, nm_b) = [[t.cpu().numpy() for t in r] for r in results]
    print("chain: matches per frame", nm_a.tolist(), "keypoints with depth", ns.tolist())
    assert np.array_equal(nm_a, nm_b) and np.array_equal(slot_a, slot_b) and np.array_equal(sobs_a, sobs_b)
    assert (nm_a > ns // 2).all()              # most map points find their own keypoint again
    m.close(); ex.close()


# ---- 4: refusals next to live buffers ---------------------------------------------------------------------------------------------
def test_refusals_with_live_buffers(pkg):
    """4: a cap beyond ORBX_CLOSE_MAX_KEYPOINTS, strides smaller than a row / an image or not a multiple of the element, a float
    image described with 16-bit strides: ORBX_E_ARG (ValueError), nothing launched, the buffers keep their sentinels."""
    import torch
    n, cap, H, W = 2, 64, 48, 64
    big = pkg.CLOSE_MAX_KEYPOINTS + 1
    d_keys = torch.zeros((n, cap, 7), dtype=torch.float32, device="cuda")
    d_cnt = torch.full((n, 2), cap, dtype=torch.int32, device="cuda")
    d_img = torch.full((n, H, W), 5000, dtype=torch.int16, device="cuda")
    d_uR, d_z = sentinel((n, big)), sentinel((n, big))
    d_order, d_nv = sentinel((n, big), np.int32), sentinel((n,), np.int32)
    look = dict(nframes=n, d_keys=d_keys.data_ptr(), d_keys_un=d_keys.data_ptr(), d_counts=d_cnt.data_ptr(), count_stride=2, cap=cap,
                d_depth_image=d_img.data_ptr(), depth_type=0, rows=H, cols=W, row_stride=2 * W, frame_stride=2 * W * H, depth_factor=float(RM.TUM1_FACTOR),
                mbf=40.0, d_uRight=d_uR.data_ptr(), d_depth=d_z.data_ptr())
    for c in (dict(row_stride=2 * W - 2), dict(row_stride=2 * W + 1), dict(frame_stride=2 * W * H - 2), dict(frame_stride=2 * W * H + 1), dict(depth_type=1),
              dict(depth_type=3), dict(cap=0), dict(nframes=-1)):
        with pytest.raises(ValueError):
            pkg.stereo_from_rgbd_batch_device(**dict(look, **c))
    sel = dict(nframes=n, d_depth=d_z.data_ptr(), d_counts=d_cnt.data_ptr(), count_stride=2, cap=cap, th_depth=3.2, max_point=100, d_order=d_order.data_ptr(),
               d_nvisit=d_nv.data_ptr())
    for c in (dict(cap=big), dict(cap=0), dict(count_stride=0), dict(nframes=-1)):
        with pytest.raises(ValueError):
            pkg.close_points_batch_device(**dict(sel, **c))
    torch.cuda.synchronize()
    assert (d_uR == float(SENTINEL)).all() and (d_z == float(SENTINEL)).all() and (d_order == ISENT).all() and (d_nv == ISENT).all()
    assert pkg.stereo_from_rgbd_batch_device(**look) == 0          # and the good call still works
    torch.cuda.synchronize()
    one = float(np.float32(5000) * RM.TUM1_FACTOR)
    assert (d_z.reshape(-1)[:n * cap] == one).all() and (d_z.reshape(-1)[n * cap:] == float(SENTINEL)).all()
