"""numpy restatement of Frame::ComputeStereoFishEyeMatches (Frame.cc:1228-1268) and of what it calls in the camera model:
KannalaBrandt8::unproject (KannalaBrandt8.cpp:112-139), TriangulateMatches (:343-412), Triangulate (:431-444) with cv::SVD as
OpenCV's own float one-sided Jacobi (JacobiSVDImpl_<float>; an OpenCV built with LAPACK gives other low bits) and KannalaBrandt8::project
(:29-45).  Independent of the product's source, like tests/stereo_model.py.

Evaluation is scalar by scalar.  A single-precision value is held as a Python float and every single-precision operation is
rounded once through np.float32 (`r`): the double result of +, -, *, / or sqrt of two float32 values rounds to the same float32
as the single operation would (53 >= 2 * 24 + 2 bits).  A double-precision operation is the Python float operation (np.float64
arithmetic).  tanf, atan2f, cosf and sinf are this host's libm through ctypes.  The knn part comes from the full distance matrix."""
import ctypes as C
import math

import numpy as np

f32 = np.float32
_libm = C.CDLL("libm.so.6")
for _n, _k in (("tanf", 1), ("cosf", 1), ("sinf", 1), ("atan2f", 2)):
    getattr(_libm, _n).restype = C.c_float
    getattr(_libm, _n).argtypes = [C.c_float] * _k

FLT_EPSILON = 2.0 ** -23
CV_PI = 3.1415926535897932384626433832795

# Examples/Stereo/TUM_512.yaml:9-47
CAM1 = np.array([190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504,
                 0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182], f32)
CAM2 = np.array([190.44236969414825, 190.4344384721956, 252.59949716835982, 254.91723064636983,
                 0.0034003170790442797, 0.001766278153469831, -0.00266312569781606, 0.0003299517423931039], f32)
TLR = np.array([[0.999999445773493, 0.000791687752817, 0.000694034010224, 0.101063427414194],
                [-0.000823363992158, 0.998899461915674, 0.046895490788700, 0.001946204678584],
                [-0.000656143613644, -0.046896036240590, 0.998899560146304, 0.001015350132563]], f32)


def level_sigma2(nlevels=8, scale_factor=1.2):
    """mvLevelSigma2 of ORBextractor.cc:413-421: the scale factor is a double member initialised from a float."""
    sf, out = f32(1.0), []
    for _ in range(nlevels):
        out.append(f32(sf * sf))
        sf = f32(float(sf) * float(f32(scale_factor)))
    return np.array(out, f32)


LEVEL_SIGMA2 = level_sigma2()

PARALLAX, Z1, Z2, REPROJ1, REPROJ2, ACCEPT = "parallax", "z1", "z2", "reproj1", "reproj2", "accept"


def r(x):
    """Round a double result to single precision."""
    return float(f32(x))


def tanf(x):
    return float(_libm.tanf(x))


def project(p, X, Y, Z):
    """KannalaBrandt8::project(cv::Point3f), :29-45; cos / sin of a float are cosf / sinf."""
    p = [float(v) for v in p]
    x2_plus_y2 = r(r(X * X) + r(Y * Y))
    theta = float(_libm.atan2f(r(math.sqrt(x2_plus_y2)), Z))
    psi = float(_libm.atan2f(Y, X))
    theta2 = r(theta * theta)
    theta3 = r(theta * theta2)
    theta5 = r(theta3 * theta2)
    theta7 = r(theta5 * theta2)
    theta9 = r(theta7 * theta2)
    rad = r(r(r(r(theta + r(p[4] * theta3)) + r(p[5] * theta5)) + r(p[6] * theta7)) + r(p[7] * theta9))
    return (r(r(r(p[0] * rad) * float(_libm.cosf(psi))) + p[2]), r(r(r(p[1] * rad) * float(_libm.sinf(psi))) + p[3]))


def unproject(p, px, py, info=None):
    """KannalaBrandt8::unproject, :112-139.  Returns the ray (x, y, 1)."""
    p = [float(v) for v in p]
    px, py = r(px), r(py)
    pwx, pwy = r(r(px - p[2]) / p[0]), r(r(py - p[3]) / p[1])
    scale = 1.0
    theta_d = r(math.sqrt(r(r(pwx * pwx) + r(pwy * pwy))))
    lo, hi = r(-CV_PI / 2.0), r(CV_PI / 2.0)          # the double constants, converted by fmaxf / fminf
    theta_d = min(max(lo, theta_d), hi) if theta_d == theta_d else lo
    if theta_d > 1e-8:                                 # in double
        theta = theta_d
        steps = 0
        for _ in range(10):
            steps += 1
            theta2 = r(theta * theta)
            theta4 = r(theta2 * theta2)
            theta6 = r(theta4 * theta2)
            theta8 = r(theta4 * theta4)
            k0 = r(p[4] * theta2)
            k1 = r(p[5] * theta4)
            k2 = r(p[6] * theta6)
            k3 = r(p[7] * theta8)
            num = r(r(theta * r(r(r(r(1.0 + k0) + k1) + k2) + k3)) - theta_d)
            den = r(r(r(r(1.0 + r(3.0 * k0)) + r(5.0 * k1)) + r(7.0 * k2)) + r(9.0 * k3))
            theta_fix = r(num / den)
            theta = r(theta - theta_fix)
            if abs(theta_fix) < r(1e-6):
                break
        if info is not None:
            info["newton"] = steps
        scale = r(tanf(theta) / theta_d)
    return (r(pwx * scale), r(pwy * scale), 1.0)


def cv_hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b /= a
        return a * math.sqrt(1 + b * b)
    if b > 0:
        a /= b
        return b * math.sqrt(1 + a * a)
    return 0.0


def jacobi_svd_vt(A):
    """Rows of vt, sorted by descending singular value, of the n x n float matrix A (list of rows) as OpenCV's float one-sided Jacobi
    computes them; also the number of sweeps that rotated and whether the iteration cap was reached."""
    n = len(A)
    At = [[A[k][i] for k in range(n)] for i in range(n)]
    V = [[1.0 if i == k else 0.0 for k in range(n)] for i in range(n)]
    W = []
    for i in range(n):
        sd = 0.0
        for t in At[i]:
            sd += t * t
        W.append(sd)
    eps = 2 * FLT_EPSILON
    max_iter = max(n, 30)
    sweeps, capped = 0, True
    for _ in range(max_iter):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                Ai, Aj = At[i], At[j]
                a, b, p = W[i], W[j], 0.0
                for k in range(n):
                    p += Ai[k] * Aj[k]
                if abs(p) <= eps * math.sqrt(a * b):
                    continue
                p *= 2
                beta = a - b
                gamma = cv_hypot(p, beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = r(math.sqrt(delta / gamma))
                    c = r(p / (gamma * s * 2))
                else:
                    c = r(math.sqrt((gamma + beta) / (gamma * 2)))
                    s = r(p / (gamma * c * 2))
                a = b = 0.0
                for k in range(n):
                    t0 = r(r(c * Ai[k]) + r(s * Aj[k]))
                    t1 = r(r(-s * Ai[k]) + r(c * Aj[k]))
                    Ai[k], Aj[k] = t0, t1
                    a += t0 * t0
                    b += t1 * t1
                W[i], W[j] = a, b
                changed = True
                Vi, Vj = V[i], V[j]
                for k in range(n):
                    t0 = r(r(c * Vi[k]) + r(s * Vj[k]))
                    t1 = r(r(-s * Vi[k]) + r(c * Vj[k]))
                    Vi[k], Vj[k] = t0, t1
        if not changed:
            capped = False
            break
        sweeps += 1
    for i in range(n):
        sd = 0.0
        for t in At[i]:
            sd += t * t
        W[i] = math.sqrt(sd)
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            V[i], V[j] = V[j], V[i]
    return V, sweeps, capped


def rig_tcw2(Tlr):
    """Tcw2 = [R21 | t21], R21 = R12.t(), t21 = -R21 * t12 (:372-374): the small-matrix gemm, float sum, alpha = -1 in double."""
    T = [[float(v) for v in row] for row in np.asarray(Tlr, f32).reshape(3, 4)]
    out = []
    for i in range(3):
        t0 = r(r(r(T[0][i] * T[0][3]) + r(T[1][i] * T[1][3])) + r(T[2][i] * T[2][3]))
        out.append([T[0][i], T[1][i], T[2][i], r(t0 * -1.0 + 0.0)])
    return out


def mat3_mul_add(R, x, t):
    """cv::Mat A * B + C for 3x3 * 3x1: float sum of products, then the addition in double."""
    return [r(r(r(r(R[i][0] * x[0]) + r(R[i][1] * x[1])) + r(R[i][2] * x[2])) + t[i]) for i in range(3)]


def triangulate(p1, p2, Tcw2, info=None):
    """KannalaBrandt8::Triangulate, :431-444, Tcw1 = [I | 0]."""
    Tcw1 = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    A = [[r(r(p1[0] * Tcw1[2][k]) - Tcw1[0][k]) for k in range(4)],
         [r(r(p1[1] * Tcw1[2][k]) - Tcw1[1][k]) for k in range(4)],
         [r(r(p2[0] * Tcw2[2][k]) - Tcw2[0][k]) for k in range(4)],
         [r(r(p2[1] * Tcw2[2][k]) - Tcw2[1][k]) for k in range(4)]]
    vt, sweeps, capped = jacobi_svd_vt(A)
    if info is not None:
        info["sweeps"], info["capped"], info["v"] = sweeps, capped, list(vt[3])
    inv = 1.0 / vt[3][3]
    return [r(vt[3][k] * inv) for k in range(3)]


def dot3(a, b):
    d = 0.0
    for k in range(3):
        d += a[k] * b[k]
    return d


def triangulate_matches(cam1, cam2, kp1, kp2, Tlr, sigma1, sigma2, info=None):
    """KannalaBrandt8::TriangulateMatches, :343-412.  Returns (depth, p3D or None, outcome)."""
    T = [[float(v) for v in row] for row in np.asarray(Tlr, f32).reshape(3, 4)]
    Tcw2 = rig_tcw2(Tlr)
    k1, k2 = (r(kp1[0]), r(kp1[1])), (r(kp2[0]), r(kp2[1]))
    r1 = unproject(cam1, k1[0], k1[1])
    r2 = unproject(cam2, k2[0], k2[1])
    r21 = mat3_mul_add(T, r2, [0.0, 0.0, 0.0])
    cos_parallax = r(dot3(r1, r21) / (math.sqrt(dot3(r1, r1)) * math.sqrt(dot3(r21, r21))))
    if cos_parallax > 0.9998:
        return -1.0, None, PARALLAX
    x3D = triangulate(r1, r2, Tcw2, info)
    z1 = x3D[2]
    if z1 <= 0:
        return -1.0, None, Z1
    z2 = r(dot3(Tcw2[2][:3], x3D) + Tcw2[2][3])
    if z2 <= 0:
        return -1.0, None, Z2
    u, v = project(cam1, *x3D)
    ex, ey = r(u - k1[0]), r(v - k1[1])
    if r(r(ex * ex) + r(ey * ey)) > 5.991 * r(sigma1):
        return -1.0, None, REPROJ1
    x3D2 = mat3_mul_add(Tcw2, x3D, [Tcw2[0][3], Tcw2[1][3], Tcw2[2][3]])
    u, v = project(cam2, *x3D2)
    ex, ey = r(u - k2[0]), r(v - k2[1])
    if r(r(ex * ex) + r(ey * ey)) > 5.991 * r(sigma2):
        return -1.0, None, REPROJ2
    return z1, x3D, ACCEPT


_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def hamming_matrix(q, c):
    q, c = np.asarray(q, np.uint8).reshape(-1, 32), np.asarray(c, np.uint8).reshape(-1, 32)
    out = np.zeros((len(q), len(c)), np.int32)
    for i in range(len(q)):
        out[i] = _POP[q[i][None, :] ^ c].sum(axis=1, dtype=np.int32)
    return out


def knn2(q, c):
    """BFMatcher(NORM_HAMMING).knnMatch(q, c, 2): the two smallest distances of every row, the lower train index first on a tie."""
    D = hamming_matrix(q, c)
    idx = np.argsort(D, axis=1, kind="stable")[:, :2]
    return idx, np.take_along_axis(D, idx, axis=1)


def ratio_test(d0, d1):
    """Frame.cc:1253: float distances, double product."""
    return float(f32(d0)) < float(f32(d1)) * 0.7


def stereo_fisheye_matches(keysL, descL, monoL, keysR, descR, monoR, level_sigma2, Tlr, cam1, cam2, p3d=None):
    """Frame::ComputeStereoFishEyeMatches.  keys: structured arrays with x, y, octave.  Returns (mvLeftToRightMatch, mvRightToLeftMatch,
    mvDepth, mvStereo3Dpoints as [Nleft, 3] float32 over the initial contents p3d, (nMatches, descMatches))."""
    nL, nR = len(keysL), len(keysR)
    l2r, r2l = np.full(nL, -1, np.int32), np.full(nR, -1, np.int32)
    depth = np.full(nL, -1.0, f32)
    pts = np.zeros((nL, 3), f32) if p3d is None else np.array(p3d, f32).reshape(nL, 3)
    n_matches = desc_matches = 0
    nlevels = len(level_sigma2)
    if nL - monoL > 0 and nR - monoR >= 2:
        idx, dist = knn2(np.asarray(descL)[monoL:], np.asarray(descR)[monoR:])
        for q in range(nL - monoL):
            if not ratio_test(dist[q, 0], dist[q, 1]):
                continue
            desc_matches += 1
            li, rj = q + monoL, int(idx[q, 0]) + monoR
            oL, oR = int(keysL["octave"][li]), int(keysR["octave"][rj])
            if not (0 <= oL < nlevels and 0 <= oR < nlevels):
                continue   # mvLevelSigma2[octave] is undefined there: a non-match in the batch form, refused by the per-frame form
            z, x3D, _ = triangulate_matches(cam1, cam2, (keysL["x"][li], keysL["y"][li]), (keysR["x"][rj], keysR["y"][rj]), Tlr,
                                            level_sigma2[oL], level_sigma2[oR])
            if f32(z) > f32(0.0001):
                l2r[li] = rj
                r2l[rj] = li
                pts[li] = x3D
                depth[li] = z
                n_matches += 1
    return l2r, r2l, depth, pts, (n_matches, desc_matches)


def synthetic_pairs(n, seed=11):
    """Keypoint pairs of a synthetic rig with the TUM-VI stereo calibration: points at depths 0.3-20 m (log-uniform) seen by the left
    camera, transformed by Trl into the right one, both projections with 0-3 px of noise; a fifth of the right keypoints replaced
    by random pixels (anywhere, or within 8 px); octaves over all levels.  Returns kp1 [n, 2], kp2 [n, 2], sigma1 [n], sigma2 [n] (float32)."""
    rng = np.random.default_rng(seed)
    Tcw2 = np.array(rig_tcw2(TLR))
    kp1, kp2 = np.zeros((n, 2), f32), np.zeros((n, 2), f32)
    for i in range(n):
        u, v = rng.uniform(20, 492, 2)
        ray = np.array(unproject(CAM1, u, v))
        depth = math.exp(rng.uniform(math.log(0.3), math.log(20.0)))
        X = ray * depth
        X2 = Tcw2[:, :3] @ X + Tcw2[:, 3]
        a = project(CAM1, *[r(t) for t in X])
        b = project(CAM2, *[r(t) for t in X2])
        noise = rng.uniform(0, 3) * (i % 3 != 0)      # a third without noise, a third in both images, a third in the right one only
        ang = rng.uniform(0, 2 * math.pi, 2)
        kp1[i] = (a[0] + noise * (i % 3 == 1) * math.cos(ang[0]), a[1] + noise * (i % 3 == 1) * math.sin(ang[0]))
        kp2[i] = (b[0] + noise * math.cos(ang[1]), b[1] + noise * math.sin(ang[1]))
        if i % 10 == 4:
            kp2[i] = rng.uniform(0, 512, 2)                      # a wrong partner anywhere in the image
        elif i % 10 == 9:
            kp2[i] = np.array(b) + rng.uniform(-8, 8, 2)         # ... and one next to the right place: the octaves decide which gate rejects
    o1, o2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    return kp1, kp2, LEVEL_SIGMA2[o1], LEVEL_SIGMA2[o2]
