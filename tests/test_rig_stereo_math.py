"""CPU: the arithmetic of Frame::ComputeStereoFishEyeMatches, each host evaluation of the one host/device definition
(csrc/orb_ref_triangulate.h) against tests/rig_stereo_model.py bit for bit: KannalaBrandt8::unproject (orbm_unproject),
TriangulateMatches with the restated Jacobi SVD (orbm_fisheye_triangulate) and the ratio test of Frame.cc:1253
(orbm_fisheye_ratio_test); and the model's SVD against numpy's in float64, a check on the restatement's form."""
import collections
import math

import numpy as np
import pytest

import rig_stereo_model as M

f32 = np.float32
NPAIRS = 4000
SENTINEL = -777.25


def grid(cam):
    """Every 8th pixel of the 512x512 image, the corners of the last row / column, points outside the image, the principal point
    (theta_d <= 1e-8) and its neighbours one ulp away."""
    pts = [(u, v) for v in list(range(0, 512, 8)) + [511] for u in list(range(0, 512, 8)) + [511]]
    pts += [(u, v) for v in (-300.0, -40.5, 255.25, 560.0, 900.0) for u in (-500.0, -1.0, 256.5, 513.0, 1200.0)]
    cx, cy = float(cam[2]), float(cam[3])
    pts += [(cx, cy), (float(np.nextafter(f32(cx), f32(1e9))), cy), (cx, float(np.nextafter(f32(cy), f32(-1e9))))]
    return np.array(pts, f32)


@pytest.mark.parametrize("cam", [M.CAM1, M.CAM2], ids=["left", "right"])
def test_unproject_equals_model(pkg, cam):
    xy = grid(cam)
    got = pkg.unproject(cam, xy)
    want = np.array([M.unproject(cam, float(u), float(v)) for u, v in xy], f32)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    centre = np.flatnonzero((xy[:, 0] == cam[2]) & (xy[:, 1] == cam[3]))
    assert len(centre) == 1 and got[centre[0]].tolist() == [0.0, 0.0, 1.0]      # scale stays 1: theta_d <= 1e-8


# project(unproject(p)) on the grid points whose distorted angle is below the clamp at pi/2 (beyond it unproject is not an inverse):
# the model's own maximum is 9.77e-05 px (left) and 9.16e-05 px (right); the bound is four times the larger
ROUND_TRIP_TOL = 4 * 9.78e-05


@pytest.mark.parametrize("cam", [M.CAM1, M.CAM2], ids=["left", "right"])
def test_project_unproject_round_trip(pkg, cam):
    xy = np.array([(u, v) for v in range(0, 512, 8) for u in range(0, 512, 8)
                   if math.hypot((u - cam[2]) / cam[0], (v - cam[3]) / cam[1]) < 1.5], f32)
    rays = pkg.unproject(cam, xy)
    worst = 0.0
    for (u, v), ray in zip(xy, rays):
        a = pkg.project(1, cam, *[float(t) for t in ray])
        worst = max(worst, math.hypot(a[0] - float(u), a[1] - float(v)))
    print("round trip: %d points, worst %.3g px (bound %.3g)" % (len(xy), worst, ROUND_TRIP_TOL))
    assert worst <= ROUND_TRIP_TOL


@pytest.fixture(scope="module")
def pairs():
    """The synthetic rig's keypoint pairs and the model's results: computed once, shared, never modified."""
    kp1, kp2, s1, s2 = M.synthetic_pairs(NPAIRS)
    depth, p3d, outcome, infos = np.zeros(NPAIRS, f32), np.full((NPAIRS, 3), SENTINEL, f32), [], []
    for i in range(NPAIRS):
        info = {}
        z, x, o = M.triangulate_matches(M.CAM1, M.CAM2, kp1[i], kp2[i], M.TLR, s1[i], s2[i], info)
        depth[i] = z
        if x is not None:
            p3d[i] = x
        outcome.append(o)
        infos.append(info)
    return dict(kp1=kp1, kp2=kp2, s1=s1, s2=s2, depth=depth, p3d=p3d, outcome=outcome, infos=infos)


def test_input_set_reaches_every_outcome(pairs):
    """From the model alone: every exit of TriangulateMatches at least 20 times, an SVD of three sweeps or more, none at the cap."""
    cnt = collections.Counter(pairs["outcome"])
    print(dict(cnt))
    for o in (M.PARALLAX, M.Z1, M.Z2, M.REPROJ1, M.REPROJ2, M.ACCEPT):
        assert cnt[o] >= 20, (o, cnt)
    sweeps = [i["sweeps"] for i in pairs["infos"] if "sweeps" in i]
    assert max(sweeps) >= 3
    assert not any(i["capped"] for i in pairs["infos"] if "capped" in i)


def test_triangulate_equals_model(pkg, pairs):
    depth, p3d = pkg.fisheye_triangulate(pairs["kp1"], pairs["kp2"], pairs["s1"], pairs["s2"], M.TLR, M.CAM1, M.CAM2, p3d_fill=SENTINEL)
    bad = np.flatnonzero(depth.view(np.uint32) != pairs["depth"].view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:5], depth[bad[:5]], pairs["depth"][bad[:5]])
    bad = np.flatnonzero((p3d.view(np.uint32) != pairs["p3d"].view(np.uint32)).any(axis=1))
    assert len(bad) == 0, (len(bad), bad[:5], p3d[bad[:5]], pairs["p3d"][bad[:5]])


# Maximum over the accepted pairs of max|x3D - x3D_numpy| / |x3D_numpy| measured for this input set: 1.913e-04 (1655 pairs; the
# null vector of a 4x4 float matrix whose two smallest singular values are close at small parallax).  Bound: four times that.
SVD_REL_BOUND = 4 * 1.92e-04


def test_model_svd_agrees_with_numpy(pairs):
    Tcw2 = np.array(M.rig_tcw2(M.TLR), np.float64)
    worst, n = 0.0, 0
    for i in range(NPAIRS):
        if pairs["outcome"][i] != M.ACCEPT:
            continue
        r1 = M.unproject(M.CAM1, *pairs["kp1"][i])
        r2 = M.unproject(M.CAM2, *pairs["kp2"][i])
        A = np.array([[-1, 0, r1[0], 0], [0, -1, r1[1], 0], r2[0] * Tcw2[2] - Tcw2[0], r2[1] * Tcw2[2] - Tcw2[1]], np.float64)
        vt = np.linalg.svd(A)[2]
        ref = vt[3, :3] / vt[3, 3]
        worst = max(worst, float(np.max(np.abs(pairs["p3d"][i].astype(np.float64) - ref)) / np.linalg.norm(ref)))
        n += 1
    print("model x3D against numpy.linalg.svd (float64): %d accepted pairs, worst relative deviation %.4g (bound %.4g)" % (n, worst, SVD_REL_BOUND))
    assert n >= 20 and worst <= SVD_REL_BOUND


def test_ratio_test_all_pairs(pkg):
    f = pkg.load().orbm_fisheye_ratio_test
    for d0 in range(257):
        for d1 in range(257):
            assert bool(f(d0, d1)) == (d0 < d1 * 0.7), (d0, d1)
            assert M.ratio_test(d0, d1) == (d0 < d1 * 0.7), (d0, d1)
