"""numpy float32 restatement, as literal loops, of the three reference fragments behind orbx_stereo_from_rgbd_batch_device and
orbx_close_points_batch_device, plus the synthetic depth images and scenes of their tests (tests/test_rgbd_abi.py,
tests/test_gpu_rgbd.py, tools/rgbd_bench.py).

  compute_stereo_from_rgbd   Frame::ComputeStereoFromRGBD (Frame.cc:1082-1103) on the depth image as Tracking::GrabImageRGBD
                             (Tracking.cc:1075-1076) converts it: d = float32(raw) * float32(factor)
  close_points               the depth-ordered loop of Tracking::UpdateLastFrame (Tracking.cc:2808-2860) and
                             Tracking::CreateNewKeyFrame (:3345-3416), and the close counts of NeedNewKeyFrame (:3190-3200)
  unproject_stereo           Frame::UnprojectStereo (Frame.cc:1105-1116)

Every scalar is an np.float32, so every operation rounds once to single precision, in the reference's source order."""
import numpy as np

F32 = np.float32

# Examples/RGB-D/TUM1.yaml
TUM1 = dict(nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7)
TUM1_K = np.array([517.306408, 516.469215, 318.643040, 255.313989], np.float32)
TUM1_D = np.array([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], np.float32)
TUM1_BF = F32(40.0)
TUM1_FACTOR = F32(1.0) / F32(5000.0)                   # mDepthMapFactor = 1.0f / 5000 (Tracking.cc:755)
TUM1_TH_DEPTH = TUM1_BF * F32(40.0) / TUM1_K[0]        # mThDepth = mbf * ThDepth / fx = 3.093 (tools/rgbd_bench.py)
TEST_TH_DEPTH = F32(3.2)                               # the tests' threshold: raw depths up to 16000 are close


def depth_u16(seed, H, W):
    """A slanted plane in raw 16-bit units with a quarter of its 16 x 16 blocks missing (0, as a depth camera reports them)."""
    y, x = np.mgrid[0:H, 0:W]
    d = (2500 + 40 * x + 5 * y).astype(np.uint16)
    hole = np.random.default_rng(seed).random((H // 16, W // 16)) < 0.25
    d[:H // 16 * 16, :W // 16 * 16][np.kron(hole, np.ones((16, 16), bool))] = 0
    return d


def compute_stereo_from_rgbd(keys, keys_un, raw, factor, mbf):
    """raw: H x W uint16 or float32.  A keypoint whose pixel is outside the image gives -1 (the stated deviation: the reference
    reads out of bounds there)."""
    N = len(keys)
    H, W = raw.shape
    factor, mbf = F32(factor), F32(mbf)
    uRight, depth = np.full(N, -1, np.float32), np.full(N, -1, np.float32)
    with np.errstate(all="ignore"):
        for i in range(N):
            v, u = int(keys["y"][i]), int(keys["x"][i])            # at<float>(v, u): float -> int truncates
            if not (0 <= v < H and 0 <= u < W):
                continue
            d = F32(raw[v, u]) * factor
            if d > 0:
                depth[i] = d
                uRight[i] = F32(keys_un["x"][i]) - mbf / d
    return uRight, depth


def close_points(depth, th_depth, max_point, tracked=None):
    """Returns (order, nTrackedClose, nNonTrackedClose): the keypoint indices the two Tracking loops visit, in order."""
    th_depth = F32(th_depth)
    vDepthIdx = []
    nTrackedClose = nNonTrackedClose = 0
    for i in range(len(depth)):
        z = F32(depth[i])
        if z > 0:
            vDepthIdx.append((z, i))
            if z < th_depth:
                if tracked is not None and tracked[i]:
                    nTrackedClose += 1
                else:
                    nNonTrackedClose += 1
    vDepthIdx = sorted(vDepthIdx)
    order, nPoints = [], 0
    for j in range(len(vDepthIdx)):
        order.append(vDepthIdx[j][1])
        nPoints += 1
        if vDepthIdx[j][0] > th_depth and nPoints > max_point:
            break
    return order, nTrackedClose, nNonTrackedClose


def nvisit_closed_form(m, c, max_point):
    """m = #{z > 0}, c = #{0 < z <= th_depth}."""
    return min(m, max(c, max_point) + 1)


def unproject_stereo(keys_un, depth, K, pose=None):
    """x3Dc [N][3] and, with pose = [Rwc | Ow] (3 x 4), x3Dw = mRwc * x3Dc + mOw as cv::Mat evaluates it: the 3-term products summed
    in float, the addition in double (csrc/orb_ref_geometry.h, mat3_mul_add).  Rows of keypoints without depth are NaN."""
    fx, fy, cx, cy = [F32(v) for v in K]
    invfx, invfy = F32(1.0) / fx, F32(1.0) / fy
    N = len(depth)
    x3Dc = np.full((N, 3), np.nan, np.float32)
    x3Dw = np.full((N, 3), np.nan, np.float32) if pose is not None else None
    with np.errstate(all="ignore"):
        for i in range(N):
            z = F32(depth[i])
            if not z > 0:
                continue
            u, v = F32(keys_un["x"][i]), F32(keys_un["y"][i])
            p = [(u - cx) * z * invfx, (v - cy) * z * invfy, z]
            x3Dc[i] = p
            if pose is not None:
                for r in range(3):
                    R = [F32(pose[r, k]) for k in range(3)]
                    t0 = R[0] * p[0] + R[1] * p[1] + R[2] * p[2]
                    x3Dw[i, r] = F32(np.float64(t0) + np.float64(pose[r, 3]))
    return x3Dc, x3Dw


_scenes = {}


def scene(oracle, synth, seed, H=480, W=640):
    """One synthetic TUM1 RGB-D frame through the oracle: image, raw depth, mvKeys, descriptors, mvKeysUn, and the model's mvuRight /
    mvDepth for it."""
    key = (seed, H, W)
    if key not in _scenes:
        img = synth.make_frame(seed, H, W)
        raw = depth_u16(seed, H, W)
        o = oracle.OracleExtractor(**TUM1)
        _, keys, desc = o.extract(img, (0, 0))
        keys_un = keys.copy()
        xy = oracle.undistort_points(np.stack([keys["x"], keys["y"]], axis=1), TUM1_K, TUM1_D)
        keys_un["x"], keys_un["y"] = xy[:, 0], xy[:, 1]
        uRight, depth = compute_stereo_from_rgbd(keys, keys_un, raw, TUM1_FACTOR, TUM1_BF)
        _scenes[key] = dict(img=img, raw=raw, keys=keys, desc=desc, keys_un=keys_un, uRight=uRight, depth=depth,
                            scale_factors=np.ascontiguousarray(o.scale_factors, np.float32))
    return _scenes[key]
