"""CPU: the host evaluations of the camera models, the oracle and the numpy models against the reference's own
src/CameraModels/Pinhole.cpp and KannalaBrandt8.cpp, compiled.

oracle/_ref/libref_cameras.so is the reference's unmodified text of the two files built against the stand-in headers of
oracle/ref_cam_shim (a float cv::Mat whose lazy expressions fold as OpenCV's MatExpr folds them, OpenCV's own float Jacobi SVD, Eigen's
fixed matrices as aggregates) and oracle/ref_cam_driver.cc.  The stand-in shares no code with the product, the oracle or the models, so
a misreading of the two files' own text that those three share shows here.  What stays on both sides is the stand-in's reading of
the OpenCV primitives.  Every comparison is equality of bits (a NaN equals a NaN).

The library is built here when the reference tree is present; the tests skip only where there is neither a library nor a tree.
Inputs: tests/ref_camera_cases.py."""
import collections
import math

import numpy as np
import pytest

import new_points_model as NP
import ref_camera_cases as RC
import rig_stereo_model as M

f32 = np.float32
SENTINEL = -777.25
KB8 = ("tumvi-left", "tumvi-right", "distorted")


@pytest.fixture(scope="module")
def ref(oracle):
    oracle.build_ref()
    try:
        oracle.ref_cam_lib()
    except RuntimeError:
        pytest.skip("no oracle/_ref/libref_cameras.so and no reference tree to build it from")
    return oracle


def bits(a):
    """float32 bit patterns with every NaN mapped onto one."""
    a = np.ascontiguousarray(a, dtype=f32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def assert_same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, what
    bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
    assert len(bad) == 0, "%s: %d differ, first at %d: %r != %r" % (what, len(bad), bad[0], np.asarray(got)[bad[0]], np.asarray(want)[bad[0]])


# ---- project ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.CAMERAS))
def test_project(ref, pkg, name):
    """Compiled project(cv::Point3f) == orbm_project == orc_project == the numpy model, the z < 0 entries included."""
    cam_type, cam = RC.CAMERAS[name]
    X = RC.projection_points(name)["X"]
    want = ref.ref_project(cam_type, cam, X)
    rows = [tuple(float(v) for v in x) for x in X]
    assert_same(np.array([pkg.project(cam_type, cam, *x) for x in rows], f32), want, "orbm_project")
    assert_same(np.array([ref.project(cam_type, cam, *x) for x in rows], f32), want, "orc_project")
    with np.errstate(all="ignore"):
        model = [NP.project(cam_type, cam, *x) for x in rows if x[2] != 0.0] if cam_type == 0 else [M.project(cam, *x) for x in rows]
    keep = np.array([x[2] != 0.0 for x in rows]) if cam_type == 0 else np.ones(len(rows), bool)     # the Pinhole model divides in Python
    assert_same(np.array(model, f32), want[keep], "model")
    assert keep.sum() >= len(rows) - 8


# ---- unproject -------------------------------------------------------------------------------------------------------------------------
def unproject_census(cam, xy):
    """(not entered, entered, early break, ten iterations, clamp acting, clamp idle) of KannalaBrandt8::unproject over the pixels, from
    the numpy model - which test_unproject has just shown to equal the compiled reference bit for bit on these pixels; the compiled
    text itself offers no way to observe its branches."""
    c = collections.Counter()
    for u, v in xy:
        info = {}
        M.unproject(cam, float(u), float(v), info)
        pwx, pwy = M.r(M.r(float(u) - float(cam[2])) / float(cam[0])), M.r(M.r(float(v) - float(cam[3])) / float(cam[1]))
        theta_d = M.r(math.sqrt(M.r(M.r(pwx * pwx) + M.r(pwy * pwy))))
        c["clamp" if theta_d > M.r(M.CV_PI / 2.0) else "no clamp"] += 1
        if "newton" not in info:
            c["not entered"] += 1
        else:
            c["entered"] += 1
            c["early break" if info["newton"] < 10 or tenth_step_broke(cam, u, v) else "ten iterations"] += 1
    return c


def tenth_step_broke(cam, u, v):
    """Whether the tenth iteration met the precision (then the loop left through `break`, not through its end): replays the loop."""
    p = [float(t) for t in cam]
    r = M.r
    pwx, pwy = r(r(float(u) - p[2]) / p[0]), r(r(float(v) - p[3]) / p[1])
    theta_d = r(math.sqrt(r(r(pwx * pwx) + r(pwy * pwy))))
    theta_d = min(max(r(-M.CV_PI / 2.0), theta_d), r(M.CV_PI / 2.0))
    theta = theta_d
    fix = 0.0
    for _ in range(10):
        t2 = r(theta * theta); t4 = r(t2 * t2); t6 = r(t4 * t2); t8 = r(t4 * t4)
        k0, k1, k2, k3 = r(p[4] * t2), r(p[5] * t4), r(p[6] * t6), r(p[7] * t8)
        num = r(r(theta * r(r(r(r(1.0 + k0) + k1) + k2) + k3)) - theta_d)
        den = r(r(r(r(1.0 + r(3.0 * k0)) + r(5.0 * k1)) + r(7.0 * k2)) + r(9.0 * k3))
        fix = r(num / den)
        theta = r(theta - fix)
        if abs(fix) < r(1e-6):
            return True
    return False


@pytest.mark.parametrize("name", KB8)
def test_unproject(ref, pkg, name):
    """Compiled KannalaBrandt8::unproject == orbm_unproject == the numpy model."""
    cam = RC.CAMERAS[name][1]
    xy = RC.unprojection_pixels(name)
    want = ref.ref_unproject(1, cam, xy)
    assert_same(pkg.unproject(cam, xy), want, "orbm_unproject")
    with np.errstate(all="ignore"):
        assert_same(np.array([M.unproject(cam, float(u), float(v)) for u, v in xy], f32), want, "model")


def test_unproject_branches_are_reached(ref):
    """Both outcomes of each branch of KannalaBrandt8::unproject at least 20 times over the three parameter sets."""
    total = collections.Counter()
    for name in KB8:
        total += unproject_census(RC.CAMERAS[name][1], RC.unprojection_pixels(name))
    print(dict(total))
    for k in ("not entered", "entered", "early break", "ten iterations", "clamp", "no clamp"):
        assert total[k] >= 20, (k, dict(total))


def test_pinhole_unproject(ref):
    """Compiled Pinhole::unproject == the Pinhole branch of tests/new_points_model.py."""
    xy = RC.unprojection_pixels("pinhole")
    want = ref.ref_unproject(0, RC.PINHOLE, xy)
    assert_same(np.array([NP.unproject(0, RC.PINHOLE, float(u), float(v)) for u, v in xy], f32), want, "model")


# ---- TriangulateMatches ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def triangulated(ref):
    """The 4096 pairs through the compiled KannalaBrandt8::TriangulateMatches: computed once, shared, never modified."""
    P = RC.triangulation_pairs()
    depth, p3d, code = ref.ref_triangulate_matches(M.CAM1, M.CAM2, M.TLR, P["kp1"], P["kp2"], P["s1"], P["s2"], p3d_fill=SENTINEL)
    return dict(P, depth=depth, p3d=p3d, code=code)


def test_every_exit_is_taken(ref, triangulated):
    """From the compiled reference alone (the exits are told apart by how often the member reached the stand-in's primitives)."""
    cnt = np.bincount(triangulated["code"], minlength=6)
    print(dict(zip(ref.TRIANGULATE_EXITS, cnt.tolist())))
    assert len(triangulated["code"]) == 4096 and (cnt >= 20).all(), cnt
    end = triangulated["code"] == 5
    assert (triangulated["depth"][~end] == -1).all() and (triangulated["p3d"][~end] == f32(SENTINEL)).all()
    assert (triangulated["depth"][end] > 0).all() and (triangulated["depth"][end] == triangulated["p3d"][end, 2]).all()


def test_triangulate_matches(ref, pkg, triangulated):
    """Compiled TriangulateMatches == orbm_fisheye_triangulate (host) == the numpy model: the depth everywhere, p3D where the reference
    reaches its end (elsewhere all three leave it alone), and the model's exit == the compiled one's."""
    T = triangulated
    depth, p3d = pkg.fisheye_triangulate(T["kp1"], T["kp2"], T["s1"], T["s2"], M.TLR, M.CAM1, M.CAM2, p3d_fill=SENTINEL)
    assert_same(depth, T["depth"], "orbm_fisheye_triangulate depth")
    assert_same(p3d, T["p3d"], "orbm_fisheye_triangulate p3D")
    md, mp, mo = np.zeros(4096, f32), np.full((4096, 3), SENTINEL, f32), []
    for i in range(4096):
        z, x, o = M.triangulate_matches(M.CAM1, M.CAM2, T["kp1"][i], T["kp2"][i], M.TLR, T["s1"][i], T["s2"][i])
        md[i] = z
        if x is not None:
            mp[i] = x
        mo.append(RC.EXITS.index(o))
    assert_same(md, T["depth"], "model depth")
    assert_same(mp, T["p3d"], "model p3D")
    assert np.array_equal(np.array(mo, np.uint8), T["code"])


# ---- epipolarConstrain -----------------------------------------------------------------------------------------------------------------
def test_kb8_epipolar_constrain(ref, triangulated):
    """KannalaBrandt8::epipolarConstrain == TriangulateMatches(...) > 0.0001f."""
    T = triangulated
    got = ref.ref_epipolar_constrain(1, M.CAM1, M.CAM2, M.TLR[:, :3], M.TLR[:, 3], T["kp1"], T["kp2"], T["s1"], T["s2"])
    assert np.array_equal(got, T["depth"] > f32(0.0001))
    assert got.sum() >= 20 and (~got).sum() >= 20


def test_pinhole_epipolar_constrain(ref):
    """Pinhole::epipolarConstrain == orc_pinhole_epipolar_constrain(orc_pinhole_F12(...)) on pairs either side of 3.84 * unc, and false
    where den == 0."""
    g1, g2 = RC.epipolar_groups()
    for g in (g1, g2):
        got = ref.ref_epipolar_constrain(0, RC.PINHOLE, RC.PINHOLE, g["R12"], g["t12"], g["kp1"], g["kp2"], 1.0, g["unc"])
        F12 = ref.pinhole_F12(g["R12"], g["t12"], RC.PINHOLE, RC.PINHOLE)
        want = np.array([ref.pinhole_epipolar_constrain(F12, *[float(v) for v in (*a, *b, u)]) for a, b, u in zip(g["kp1"], g["kp2"], g["unc"])])
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        g["verdict"] = got
    assert len(g1["verdict"]) + len(g2["verdict"]) == 2000
    assert g1["verdict"].sum() > 600 and (~g1["verdict"]).sum() > 600
    assert not g2["verdict"].any() and not ref.pinhole_F12(g2["R12"], g2["t12"], RC.PINHOLE, RC.PINHOLE).any()


# ---- the stand-in's SVD ----------------------------------------------------------------------------------------------------------------
# the numpy model's x3D against numpy.linalg.svd in float64 deviates by at most 1.913e-4 (relative) on the accepted
# pairs of rig_stereo_model.synthetic_pairs(4000); tests/test_rig_stereo_math.py asserts four times that.  The same bound - derived from
# the model, not from the stand-in - holds the stand-in's SVD here, on the accepted pairs of this file's set.
SVD_REL_BOUND = 4 * 1.92e-04


def test_shim_svd(ref, triangulated):
    """On the 4 x 4 systems of the accepted pairs: every row of the stand-in's vt (the last one is the solution) equals the model's
    Jacobi bit for bit, w is descending, u and vt are orthonormal; and x3D = vt[3][:3] / vt[3][3] stays within the recorded deviation
    from numpy's float64 SVD."""
    T = triangulated
    TCW1 = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    Tcw2 = M.rig_tcw2(M.TLR)
    T64 = np.array(Tcw2, np.float64)
    worst, n, ortho = 0.0, 0, 0.0
    for i in np.flatnonzero(T["code"] == 5):
        r1, r2 = M.unproject(M.CAM1, *T["kp1"][i]), M.unproject(M.CAM2, *T["kp2"][i])
        A = np.array([[M.r(M.r(p[k] * T[2][c]) - T[k][c]) for c in range(4)] for p, T in ((r1, TCW1), (r2, Tcw2)) for k in (0, 1)], f32)   # :435-438
        w, u, vt = ref.ref_svd(A)
        want, _, _ = M.jacobi_svd_vt([[float(v) for v in row] for row in A])
        assert_same(vt, np.array(want, f32), "vt of pair %d" % i)
        assert (np.diff(w) <= 0).all()
        ortho = max(ortho, float(np.abs(u.astype(np.float64).T @ u - np.eye(4)).max()), float(np.abs(vt.astype(np.float64) @ vt.T - np.eye(4)).max()))
        A64 = np.array([[-1, 0, r1[0], 0], [0, -1, r1[1], 0], r2[0] * T64[2] - T64[0], r2[1] * T64[2] - T64[1]], np.float64)
        v64 = np.linalg.svd(A64)[2]
        x64 = v64[3, :3] / v64[3, 3]
        x = (vt[3, :3].astype(np.float64) * (1.0 / float(vt[3, 3]))).astype(f32)
        assert_same(x[None], T["p3d"][i][None], "x3D of pair %d from the stand-in's vt" % i)
        worst = max(worst, float(np.max(np.abs(x.astype(np.float64) - x64)) / np.linalg.norm(x64)))
        n += 1
    print("stand-in SVD against numpy.linalg.svd (float64): %d accepted pairs, worst relative deviation %.4g (bound %.4g); orthonormal within %.3g"
          % (n, worst, SVD_REL_BOUND, ortho))
    assert n >= 20 and worst <= SVD_REL_BOUND
    assert ortho < 64 * M.FLT_EPSILON          # 4 x 4, a few sweeps of float rotations


def test_shim_svd_other_shapes(ref):
    """The stand-in's SVD is written for any small m x n: reconstruction u * diag(w) * vt within float rounding, both orientations."""
    rng = np.random.default_rng(9)
    for m, n in ((4, 4), (3, 5), (5, 3), (2, 2), (6, 4)):
        A = rng.normal(size=(m, n)).astype(f32)
        w, u, vt = ref.ref_svd(A)
        k = min(m, n)
        rec = u[:, :k].astype(np.float64) @ np.diag(w.astype(np.float64)) @ vt[:k].astype(np.float64)
        assert np.abs(rec - A).max() < 64 * M.FLT_EPSILON * np.abs(A).max(), (m, n)
        assert np.allclose(w, np.linalg.svd(A.astype(np.float64), compute_uv=False), rtol=0, atol=64 * M.FLT_EPSILON * float(w[0]))


# ---- the libm overloads ----------------------------------------------------------------------------------------------------------------
def project_double_reading(p, X, Y, Z):
    """KannalaBrandt8::project(cv::Point3f) where cos(psi) / sin(psi) are ::cos(double) / ::sin(double): everything up to r is float as
    before, then fx * r (float) times the double cosine plus cx in double, rounded once by cv::Point2f's constructor."""
    p = [float(v) for v in p]
    r = M.r
    theta = float(M._libm.atan2f(r(math.sqrt(r(r(X * X) + r(Y * Y)))), Z))
    psi = float(M._libm.atan2f(Y, X))
    t2 = r(theta * theta); t3 = r(theta * t2); t5 = r(t3 * t2); t7 = r(t5 * t2); t9 = r(t7 * t2)
    rad = r(r(r(r(theta + r(p[4] * t3)) + r(p[5] * t5)) + r(p[6] * t7)) + r(p[7] * t9))
    return r(r(p[0] * rad) * math.cos(psi) + p[2]), r(r(p[1] * rad) * math.sin(psi) + p[3])


def test_overload_choice(ref, pkg):
    """Which libm functions the reference's unqualified cos(psi) / sin(psi) are is decided by the headers of the unit.  Built as the
    stand-in's opencv2/opencv.hpp builds it (<math.h>, libstdc++'s wrapper: the float overloads) the compiled text equals the product
    on every angle where cosf / sinf differ from the rounded double functions; built with <cmath> alone it computes the double reading
    (project_double_reading) on the whole projection set, so it differs from the product exactly where that reading's rounded u or v
    differs.  unproject has no such call (std::tan, sqrtf, fminf, fmaxf, fabsf): identical in both builds."""
    try:
        Lc = ref.ref_cam_lib(cmath=True)
    except RuntimeError:
        pytest.skip("no oracle/_ref/libref_cameras_cmath.so and no reference tree to build it from")
    sensitive = differing = 0
    for name in KB8:
        cam = RC.CAMERAS[name][1]
        X = RC.projection_points(name)["X"]
        rows = [tuple(float(v) for v in x) for x in X]
        product = np.array([pkg.project(1, cam, *x) for x in rows], f32)
        as_math_h, as_cmath = ref.ref_project(1, cam, X), ref.ref_project(1, cam, X, L=Lc)
        sens = np.array([RC.overload_sensitive(x[0], x[1]) for x in rows])
        sensitive += int(sens.sum())
        assert_same(as_math_h[sens], product[sens], "<math.h> build on the sensitive angles")
        assert_same(as_math_h, product, "<math.h> build")
        double_reading = np.array([project_double_reading(cam, *x) for x in rows], f32)
        assert_same(as_cmath, double_reading, "<cmath> build against the double reading")
        differs = (bits(as_cmath) != bits(product)).any(axis=1)
        assert np.array_equal(differs, (bits(double_reading) != bits(product)).any(axis=1))
        differing += int(differs.sum())
        xy = RC.unprojection_pixels(name)
        assert_same(ref.ref_unproject(1, cam, xy, L=Lc), ref.ref_unproject(1, cam, xy), "unproject in both builds")
    print("overload-sensitive angles: %d; projections on which the <cmath> build differs from the product: %d of 3000" % (sensitive, differing))
    assert sensitive >= 200 and differing >= 200
    # Pinhole has no libm call at all
    X = RC.projection_points("pinhole")["X"]
    assert_same(ref.ref_project(0, RC.PINHOLE, X, L=Lc), ref.ref_project(0, RC.PINHOLE, X), "Pinhole::project in both builds")
