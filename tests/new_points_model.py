"""numpy restatement of the body of LocalMapping::CreateNewMapPoints' loop (LocalMapping.cc:605-880) for one matched pair, with
KeyFrame::UnprojectStereo (KeyFrame.cc:850-869), Pinhole::unproject / project (Pinhole.cpp:46-49, :78-81) and, through
tests/rig_stereo_model.py, KannalaBrandt8's unproject / project and OpenCV's float Jacobi SVD.  Independent of the product's source.

Evaluation is scalar by scalar under the rules of rig_stereo_model: a single-precision value is a Python float, every single-precision
operation is rounded once through `r`, a double-precision operation is the Python float operation; atan2f and cosf are this host's libm.
A keyframe `c` and a keypoint `o` are mappings with the fields of orbm_new_point_camera_t / orbm_new_point_obs_t (include/orbhip.h);
the status values are the header's ORBM_NP_* (tests/test_new_points_model.py compares the two lists).  A helper, not a conftest."""
import math

import rig_stereo_model as M

r = M.r
STATUS = ("NO_MATCH", "ACCEPTED", "LOW_PARALLAX", "ZERO_W", "EMPTY_STEREO", "BEHIND1", "BEHIND2", "REPROJ1", "REPROJ1_STEREO", "REPROJ2",
          "REPROJ2_STEREO", "ZERO_DIST", "FAR", "SCALE")
(NO_MATCH, ACCEPTED, LOW_PARALLAX, ZERO_W, EMPTY_STEREO, BEHIND1, BEHIND2, REPROJ1, REPROJ1_STEREO, REPROJ2, REPROJ2_STEREO, ZERO_DIST, FAR,
 SCALE) = range(len(STATUS))


def _rows(T):
    return [[float(v) for v in T[4 * i:4 * i + 4]] for i in range(3)]


def unproject(cam_type, p, x, y):
    if cam_type == 0:
        p = [float(v) for v in p]
        return (r(r(x - p[2]) / p[0]), r(r(y - p[3]) / p[1]), 1.0)
    return M.unproject(p, x, y)


def project(cam_type, p, X, Y, Z):
    if cam_type == 0:
        p = [float(v) for v in p]
        return (r(r(r(p[0] * X) / Z) + p[2]), r(r(r(p[1] * Y) / Z) + p[3]))
    return M.project(p, X, Y, Z)


def rotate_to_world(T, x):
    """Rwc * x, Rwc = Rcw.t(): the float sum of products, the (absent) addend in double."""
    return [r(r(r(r(T[0][i] * x[0]) + r(T[1][i] * x[1])) + r(T[2][i] * x[2])) + 0.0) for i in range(3)]


def cos_parallax_stereo(mb, depth):
    return float(M._libm.cosf(r(2.0 * float(M._libm.atan2f(r(mb / 2.0), depth)))))


def unproject_stereo(c, o):
    z = float(o["depth"])
    if not z > 0:
        return None
    x = r(r(r(float(o["key_x"]) - float(c["cx"])) * z) * float(c["invfx"]))
    y = r(r(r(float(o["key_y"]) - float(c["cy"])) * z) * float(c["invfy"]))
    Twc = _rows(c["Twc"])
    return M.mat3_mul_add(Twc, [x, y, z], [Twc[0][3], Twc[1][3], Twc[2][3]])


def row_dot(T, i, X):
    return r(M.dot3(T[i][:3], X) + T[i][3])


def reprojection_fails(c, side, stereo, mbf1, T, X, z, o):
    sigma = float(c["sigma2"][int(o["octave"]) & 15])
    x, y = row_dot(T, 0, X), row_dot(T, 1, X)
    invz = r(1.0 / z)
    ox, oy = float(o["x"]), float(o["y"])
    if not stereo:
        u, v = project(int(c["cam_type"]), c["cam"][side], x, y, z)
        ex, ey = r(u - ox), r(v - oy)
        return r(r(ex * ex) + r(ey * ey)) > 5.991 * sigma
    fx, fy, cx, cy = (float(c[k]) for k in ("fx", "fy", "cx", "cy"))
    u = r(r(r(fx * x) * invz) + cx)
    u_r = r(u - r(mbf1 * invz))
    v = r(r(r(fy * y) * invz) + cy)
    ex, ey, er = r(u - ox), r(v - oy), r(u_r - float(o["u_right"]))
    return r(r(r(ex * ex) + r(ey * ey)) + r(er * er)) > 7.8 * sigma


def geometry(c1, c2, o1, o2, scale_factor1, far_points=False, th_far_points=0.0):
    """(status, x3D or None) of LocalMapping.cc:605-880 for the pair (o1 of keyframe c1, o2 of keyframe c2)."""
    rig1, rig2 = int(c1["n_left"]) != -1, int(c2["n_left"]) != -1
    st1 = (not rig1) and float(o1["u_right"]) >= 0
    st2 = (not rig2) and float(o2["u_right"]) >= 0
    s1 = 1 if (rig1 and rig2 and int(o1["right"])) else 0
    s2 = 1 if (rig1 and rig2 and int(o2["right"])) else 0
    T1, T2 = _rows(c1["Tcw"][s1]), _rows(c2["Tcw"][s2])
    Ow1, Ow2 = [float(v) for v in c1["Ow"][s1]], [float(v) for v in c2["Ow"][s2]]
    xn1 = unproject(int(c1["cam_type"]), c1["cam"][s1], float(o1["x"]), float(o1["y"]))
    xn2 = unproject(int(c2["cam_type"]), c2["cam"][s2], float(o2["x"]), float(o2["y"]))
    ray1, ray2 = rotate_to_world(T1, xn1), rotate_to_world(T2, xn2)
    cos_rays = r(M.dot3(ray1, ray2) / (math.sqrt(M.dot3(ray1, ray1)) * math.sqrt(M.dot3(ray2, ray2))))
    cs1 = cs2 = r(cos_rays + 1.0)
    if st1:
        cs1 = cos_parallax_stereo(float(c1["mb"]), float(o1["depth"]))
    elif st2:
        cs2 = cos_parallax_stereo(float(c2["mb"]), float(o2["depth"]))
    cs = cs2 if cs2 < cs1 else cs1
    if cos_rays < cs and cos_rays > 0 and (st1 or st2 or cos_rays < 0.9998):
        A = [[r(r(xn1[0] * T1[2][k]) - T1[0][k]) for k in range(4)],
             [r(r(xn1[1] * T1[2][k]) - T1[1][k]) for k in range(4)],
             [r(r(xn2[0] * T2[2][k]) - T2[0][k]) for k in range(4)],
             [r(r(xn2[1] * T2[2][k]) - T2[1][k]) for k in range(4)]]
        vt, _, _ = M.jacobi_svd_vt(A)
        if vt[3][3] == 0:
            return ZERO_W, None
        inv = 1.0 / vt[3][3]
        X = [r(vt[3][k] * inv) for k in range(3)]
    elif st1 and cs1 < cs2:
        X = unproject_stereo(c1, o1)
        if X is None:
            return EMPTY_STEREO, None
    elif st2 and cs2 < cs1:
        X = unproject_stereo(c2, o2)
        if X is None:
            return EMPTY_STEREO, None
    else:
        return LOW_PARALLAX, None
    z1 = row_dot(T1, 2, X)
    if z1 <= 0:
        return BEHIND1, None
    z2 = row_dot(T2, 2, X)
    if z2 <= 0:
        return BEHIND2, None
    mbf1 = float(c1["mbf"])
    if reprojection_fails(c1, s1, st1, mbf1, T1, X, z1, o1):
        return (REPROJ1_STEREO if st1 else REPROJ1), None
    if reprojection_fails(c2, s2, st2, mbf1, T2, X, z2, o2):
        return (REPROJ2_STEREO if st2 else REPROJ2), None
    n1, n2 = [r(X[k] - Ow1[k]) for k in range(3)], [r(X[k] - Ow2[k]) for k in range(3)]
    d1, d2 = r(math.sqrt(M.dot3(n1, n1))), r(math.sqrt(M.dot3(n2, n2)))
    if d1 == 0 or d2 == 0:
        return ZERO_DIST, None
    th = r(th_far_points)
    if far_points and (d1 >= th or d2 >= th):
        return FAR, None
    ratio_factor = r(1.5 * r(scale_factor1))
    ratio_dist = r(d2 / d1)
    ratio_octave = r(float(c1["sf"][int(o1["octave"]) & 15]) / float(c2["sf"][int(o2["octave"]) & 15]))
    if r(ratio_dist * ratio_factor) < ratio_octave or ratio_dist > r(ratio_octave * ratio_factor):
        return SCALE, None
    return ACCEPTED, X


def first_accepted(status, rows):
    """The SEQUENTIAL RULE of include/orbhip.h: the list [(j, idx1, idx2)] of the accepted pairs whose neighbour is the smallest accepted
    one of their idx1, j ascending, idx1 ascending.  status / rows: [K][n1]."""
    taken, out = set(), []
    for j in range(len(rows)):
        for i1 in range(len(rows[j])):
            if status[j][i1] == ACCEPTED and i1 not in taken:
                taken.add(i1)
                out.append((j, i1, int(rows[j][i1])))
    return out
