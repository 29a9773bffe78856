"""numpy / float32 restatement of what Tracking::SearchLocalPoints computes per local map point before its search: Frame::isInFrustum
(Frame.cc:572-661, Nleft == -1) with MapPoint::PredictScale (MapPoint.cc:587-602), and the query set SearchByProjection(Frame&,
const vector<MapPoint*>&, th, bFarPoints, thFarPoints) takes from it (ORBmatcher.cc:52-59).  Every step is the IEEE single or
double operation of the reference's expression in source order; the camera is the oracle's (oracle.project), log is the host's
glibc logf.  The expected values of tests/test_gpu_local_points.py come from here followed by OracleFrame.search_by_projection_mp."""
import ctypes as C

import numpy as np

f32 = np.float32
INT_MIN = -2 ** 31

_libm = C.CDLL("libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def glibc_logf(x):
    return f32(_libm.logf(float(x)))


def cvtt_f32_i32(x):
    """(int) of a float as x86 cvttss2si converts it: NaN and values outside the int range give INT_MIN."""
    x = float(x)
    if x != x or x >= 2147483648.0 or x < -2147483648.0:
        return INT_MIN
    return int(x)


def camera_centre(Tcw):
    """mOw = -mRcw.t()*mtcw (Frame.cc:538): the generic gemm path, double accumulation, alpha = -1."""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    Ow = np.zeros(3, f32)
    for a in range(3):
        s = 0.0
        for k in range(3):
            s += float(T[k, a]) * float(T[k, 3])
        Ow[a] = f32(s * -1.0)
    return Ow


def norm3(v):
    s = 0.0
    for k in range(3):
        s += float(v[k]) * float(v[k])
    return f32(np.sqrt(s))


def is_in_frustum(Xw, normal, max_dist, min_dist, eligible, Tcw, cam_type, cam, bounds, nlevels, log_sf, mbf, view_cos_limit, project):
    """Per point: the MapPoint fields isInFrustum writes.  Returns a dict of arrays (in_view, proj_x, proj_y, proj_xr, depth,
    view_cos, level); entries the reference leaves untouched are 0 (ineligible points: everything but in_view)."""
    T = np.asarray(Tcw, f32).reshape(4, 4)
    Xw = np.asarray(Xw, f32).reshape(-1, 3)
    normal = np.asarray(normal, f32).reshape(-1, 3)
    max_dist, min_dist = np.asarray(max_dist, f32), np.asarray(min_dist, f32)
    n = len(Xw)
    min_x, max_x, min_y, max_y = (f32(b) for b in bounds)
    out = dict(in_view=np.zeros(n, np.uint8), proj_x=np.zeros(n, f32), proj_y=np.zeros(n, f32), proj_xr=np.zeros(n, f32),
               depth=np.zeros(n, f32), view_cos=np.zeros(n, f32), level=np.zeros(n, np.int32))
    Ow = camera_centre(T)
    R, t = T[:3, :3], T[:3, 3]
    with np.errstate(all="ignore"):
        # Pc = mRcw*P + mtcw: products summed in float, then + t in double (mat3_mul_add)
        Pc = np.stack([((R[i, 0] * Xw[:, 0] + R[i, 1] * Xw[:, 1]) + R[i, 2] * Xw[:, 2]).astype(np.float64) + np.float64(t[i])
                       for i in range(3)], axis=1).astype(f32)
        for j in range(n):
            if not eligible[j]:
                continue
            pc = Pc[j]
            pc_dist = norm3(pc)
            invz = f32(1.0) / pc[2]
            px = py = f32(-1.0)
            in_view = False
            vcos, lvl = f32(0), 0
            if not pc[2] < f32(0.0):
                ux, vy = (f32(c) for c in project(cam_type, cam, float(pc[0]), float(pc[1]), float(pc[2])))
                if not (ux < min_x or ux > max_x) and not (vy < min_y or vy > max_y):
                    px, py = ux, vy
                    po = Xw[j] - Ow
                    dist = norm3(po)
                    if not (dist < f32(0.8) * min_dist[j] or dist > f32(1.2) * max_dist[j]):
                        d = 0.0
                        for k in range(3):
                            d += float(po[k]) * float(normal[j, k])
                        vcos = f32(np.float64(d) / np.float64(dist))      # IEEE: 0 / 0 is NaN
                        if not vcos < f32(view_cos_limit):
                            ratio = max_dist[j] / dist
                            lvl = cvtt_f32_i32(np.ceil(glibc_logf(ratio) / f32(log_sf)))
                            lvl = 0 if lvl < 0 else (nlevels - 1 if lvl >= nlevels else lvl)
                            in_view = True
            out["in_view"][j] = 1 if in_view else 0
            out["proj_x"][j], out["proj_y"][j] = px, py
            if in_view:
                out["proj_xr"][j] = px - f32(mbf) * invz
                out["depth"][j] = pc_dist
                out["level"][j] = lvl
                out["view_cos"][j] = vcos
    return out


def query_mask(track, eligible, bFarPoints, thFarPoints):
    """The local map points SearchByProjection searches for (ORBmatcher.cc:52-59): in view, eligible, not a far point."""
    m = (track["in_view"] != 0) & (np.asarray(eligible) != 0)
    if bFarPoints:
        m &= ~(track["depth"] > f32(thFarPoints))
    return m.astype(np.uint8)
