"""Inputs for the camera-model tests against the reference's own Pinhole.cpp / KannalaBrandt8.cpp, compiled
(tests/test_ref_cameras.py on the CPU, tests/test_gpu_ref_cameras.py on the device).  A helper, not a conftest: deterministic, seeded,
small, built once per process and never modified.  Nothing here looks at the compiled library or at the product.

Parameter sets: the EuRoC Pinhole, both TUM-VI KannalaBrandt8 cameras with the Tlr of tests/rig_stereo_model.py, and DISTORTED, a
KannalaBrandt8 set made for the Newton loop of unproject: k0 = -0.4 bends theta*(1 + k0*theta^2 + ...) back below pi/2, so that beyond
its maximum (theta_d of about 0.6) there is no root and the loop runs all ten iterations; its principal point is (0, 0), so that float
pixels resolve theta_d = |p - c| / f around the 1e-8 of the branch in front of the loop (next to cx = 255 one ulp of a pixel is already
1.6e-7 in theta_d)."""
import math

import numpy as np

import rig_stereo_model as M

f32 = np.float32
PINHOLE = np.array([458.654, 457.296, 367.215, 248.375], f32)       # Examples/Monocular/EuRoC.yaml:9-12, 752 x 480
DISTORTED = np.array([190.0, 190.0, 0.0, 0.0, -0.4, 0.05, 0.01, -0.002], f32)
CAMERAS = {"pinhole": (0, PINHOLE), "tumvi-left": (1, M.CAM1), "tumvi-right": (1, M.CAM2), "distorted": (1, DISTORTED)}
EXITS = (M.PARALLAX, M.Z1, M.Z2, M.REPROJ1, M.REPROJ2, M.ACCEPT)    # the order of oracle_py.TRIANGULATE_EXITS

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _step(x, k):
    """x moved by k float32 ulps (away from zero for k > 0)."""
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(math.copysign(np.inf, x)) if k > 0 else f32(0))
    return x


def overload_sensitive(x, y):
    """Whether psi = atan2f(y, x) is an angle at which this host's cosf / sinf differ from cos / sin of the double, rounded to float:
    there the libm overload that the reference's unqualified cos(psi) / sin(psi) resolve to shows in the result."""
    psi = float(M._libm.atan2f(float(f32(y)), float(f32(x))))
    return f32(M._libm.cosf(psi)) != f32(math.cos(psi)) or f32(M._libm.sinf(psi)) != f32(math.sin(psi))


# ---- projection ------------------------------------------------------------------------------------------------------------------------
LO, HI = (-0.8, -0.5, 1.0), (0.9, 0.6, 1.0)     # the two points whose projections are the image bounds of the device tests


def projection_points(name):
    """dict(X [n, 3] float32 with z >= 0 first and the z < 0 entries (host entry points only) last, nfront, lo, hi): about 1000 points per
    camera.  X[lo] / X[hi] project onto the (minX, minY) / (maxX, maxY) corner of the frame the device tests use; listed next to them:
    points sharing one coordinate ratio with a corner and points a few ulps either side of it (exactly on / just outside a bound), the
    axis, y = +-0 with x < 0 (psi = +-pi), z tiny against r and z = 0."""
    def make():
        rng = np.random.default_rng({"pinhole": 1, "tumvi-left": 2, "tumvi-right": 3, "distorted": 4}[name])
        pts = [LO, HI]
        for d in (0.37, 2.5, 19.0):                          # the same rays at other depths: not exact multiples, so either side of a bound
            pts += [tuple(d * c for c in LO), tuple(d * c for c in HI)]
        for k in (-3, -2, -1, 1, 2, 3):                      # a few ulps inside / outside each bound, the other coordinate well inside
            pts += [(_step(LO[0], k), 0.1, 1.0), (_step(HI[0], k), -0.1, 1.0), (0.1, _step(LO[1], k), 1.0), (-0.1, _step(HI[1], k), 1.0)]
            pts += [(_step(LO[0], k), LO[1], 1.0), (HI[0], _step(HI[1], k), 1.0)]
        pts += [(LO[0], 0.2, 1.0), (HI[0], -0.3, 1.0), (0.3, LO[1], 1.0), (-0.2, HI[1], 1.0)]      # exactly on one bound
        pts += [(0.0, 0.0, z) for z in (1e-30, 1e-3, 1.0, 7.5, 1e6)] + [(-0.0, 0.0, 2.0), (0.0, -0.0, 2.0), (-0.0, -0.0, 2.0)]
        for x in (-1e-20, -1e-3, -0.25, -1.0, -40.0):
            pts += [(x, 0.0, 1.0), (x, -0.0, 1.0), (x, 1e-38, 1.0), (x, -1e-38, 1.0)]
        for z in (0.0, 1e-38, 1e-20, 1e-8, 1e-4):            # z tiny against r: theta at pi / 2, a Pinhole projection far outside or infinite
            pts += [(1.0, 0.5, z), (-0.3, 0.7, z), (1e-3, -2e-3, z)]
        if CAMERAS[name][0] == 1:                           # 60 points whose psi tells cosf / sinf from the rounded double functions
            found = 0
            while found < 60:
                z = math.exp(rng.uniform(math.log(0.2), math.log(30.0)))
                q = (float(f32(rng.uniform(-1.4, 1.5) * z)), float(f32(rng.uniform(-1.0, 1.1) * z)), z)
                if overload_sensitive(q[0], q[1]):
                    pts.append(q)
                    found += 1
        n_rand = 1000 - len(pts) - 24
        z = np.exp(rng.uniform(math.log(0.2), math.log(30.0), n_rand))
        X = np.stack([rng.uniform(-1.4, 1.5, n_rand) * z, rng.uniform(-1.0, 1.1, n_rand) * z, z], axis=1)
        front = np.concatenate([np.array(pts, np.float64), X]).astype(f32)
        zb = -np.exp(rng.uniform(math.log(1e-3), math.log(10.0), 24))
        back = np.stack([rng.uniform(-1, 1, 24), rng.uniform(-1, 1, 24), zb], axis=1).astype(f32)
        back[:4] = [(0, 0, -1), (0.5, -0.0, -2), (-0.5, 0.0, -1e-30), (1, 1, -0.0)]
        back[3, 2] = f32(-1e-45)                             # the smallest negative float: z < 0 in every reading
        return dict(X=np.concatenate([front, back]), nfront=len(front), lo=0, hi=1)
    return _once(("project", name), make)


# ---- unprojection ----------------------------------------------------------------------------------------------------------------------
def unprojection_pixels(name):
    """xy [n, 2] float32, about 1000 pixels per camera: random pixels inside the image and up to 1500 px outside it (where the clamp at
    +-pi/2 acts), the principal point and its neighbours one ulp away, and for DISTORTED rings at theta_d = 1e-8 * {0.25 .. 4} and the
    region beyond the maximum of its distortion polynomial."""
    def make():
        cam = CAMERAS[name][1]
        rng = np.random.default_rng({"pinhole": 11, "tumvi-left": 12, "tumvi-right": 13, "distorted": 14}[name])
        fx, fy, cx, cy = (float(v) for v in cam[:4])
        w, h = (752, 480) if name == "pinhole" else (512, 512)
        pts = [(cx, cy), (float(_step(cx, 1)), cy), (cx, float(_step(cy, 1))), (float(_step(cx, -1)), float(_step(cy, -1)))]
        if name == "distorted":
            for scale in (0.25, 0.5, 0.9, 0.999, 1.001, 1.1, 2.0, 4.0):          # around theta_d = 1e-8
                for a in np.arange(12) * (2 * math.pi / 12) + 0.1:
                    pts.append((fx * 1e-8 * scale * math.cos(a), fy * 1e-8 * scale * math.sin(a)))
            for rad in np.linspace(0.55, 1.7, 100):                             # across the maximum of the polynomial and the clamp
                a = rng.uniform(0, 2 * math.pi)
                pts.append((fx * rad * math.cos(a), fy * rad * math.sin(a)))
            x0, y0 = -256.0, -256.0
        else:
            x0, y0 = 0.0, 0.0
        n_in = (1000 - len(pts)) * 6 // 10
        n_out = 1000 - len(pts) - n_in
        inside = np.stack([rng.uniform(x0, x0 + w, n_in), rng.uniform(y0, y0 + h, n_in)], axis=1)
        outside = np.stack([rng.uniform(x0 - 1500, x0 + w + 1500, n_out), rng.uniform(y0 - 1500, y0 + h + 1500, n_out)], axis=1)
        return np.concatenate([np.array(pts, np.float64), inside, outside]).astype(f32)
    return _once(("unproject", name), make)


# ---- KannalaBrandt8::TriangulateMatches ------------------------------------------------------------------------------------------------
NPAIRS, NSYNTH, NBUILT = 4096, 3600, 496


def _rig():
    T = np.eye(4)
    T[:3] = np.array(M.rig_tcw2(M.TLR), np.float64)         # left -> right
    return T


def _see(cam, X):
    return M.project(cam, *[M.r(v) for v in X[:3]])


def triangulation_pairs():
    """dict(kp1, kp2 [4096, 2], s1, s2 [4096] float32): rig_stereo_model.synthetic_pairs(3600) and 496 pairs built to leave
    KannalaBrandt8::TriangulateMatches through each exit (the left camera is the world frame, Trl moves a point into the right one):
      parallax   points at 60-2000 m: the rays are parallel within 0.9998;
      z1 <= 0    the rays meet at P BEHIND both cameras: each keypoint is the projection of -P (the same line);
      z2 <= 0    P just in front of the left camera and far off its axis in -y, which the right camera's 2.7 degree tilt puts behind it:
                 left keypoint = projection of P, right keypoint = projection of -P;
      reproj1    a true pair with the left keypoint 7-12 px off in y, both at octave 0: the null vector splits the error, the first test fails;
      reproj2    the same with the left keypoint at octave 7 (threshold 8.8 px) and the right one at octave 0 (2.4 px);
      accept     true pairs at 0.4-2.5 m without noise.
    The recipes aim; what the compiled reference does with each pair is counted in tests/test_ref_cameras.py."""
    def make():
        rng = np.random.default_rng(2025)
        kp1, kp2, s1, s2 = M.synthetic_pairs(NSYNTH)
        Trl = _rig()
        rows = []
        s_lo, s_hi = M.LEVEL_SIGMA2[0], M.LEVEL_SIGMA2[7]

        def point(depth_lo, depth_hi):
            u, v = rng.uniform(60, 452, 2)
            ray = np.array(M.unproject(M.CAM1, u, v))
            return ray * math.exp(rng.uniform(math.log(depth_lo), math.log(depth_hi)))

        for kind, count in (("parallax", 80), ("z1", 80), ("z2", 80), ("reproj1", 80), ("reproj2", 80), ("accept", 96)):
            for _ in range(count):
                if kind == "z2":
                    y = -rng.uniform(1.0, 3.0)
                    P = np.array([rng.uniform(-0.4, 0.4), y, -y / 21.3 * rng.uniform(0.3, 0.9)])
                    P2 = Trl[:3, :3] @ P + Trl[:3, 3]
                    a, b, o1, o2 = _see(M.CAM1, P), _see(M.CAM2, -P2), s_lo, s_lo
                elif kind == "z1":
                    P = -point(0.5, 4.0)
                    P2 = Trl[:3, :3] @ P + Trl[:3, 3]
                    a, b, o1, o2 = _see(M.CAM1, -P), _see(M.CAM2, -P2), s_lo, s_lo
                else:
                    P = point(*{"parallax": (60.0, 2000.0), "accept": (0.4, 2.5)}.get(kind, (0.5, 3.0)))
                    P2 = Trl[:3, :3] @ P + Trl[:3, 3]
                    a, b = _see(M.CAM1, P), _see(M.CAM2, P2)
                    o1, o2 = (s_hi, s_lo) if kind == "reproj2" else (s_lo, s_lo)
                    if kind in ("reproj1", "reproj2"):
                        a = (a[0], a[1] + rng.uniform(7.0, 12.0) * rng.choice([-1.0, 1.0]))
                rows.append((a, b, o1, o2))
        assert len(rows) == NBUILT
        return dict(kp1=np.concatenate([kp1, np.array([r_[0] for r_ in rows], f32)]), kp2=np.concatenate([kp2, np.array([r_[1] for r_ in rows], f32)]),
                    s1=np.concatenate([s1, np.array([r_[2] for r_ in rows], f32)]), s2=np.concatenate([s2, np.array([r_[3] for r_ in rows], f32)]))
    return _once("pairs", make)


# ---- Pinhole::epipolarConstrain --------------------------------------------------------------------------------------------------------
def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def epipolar_groups():
    """Two groups dict(R12 [3, 3], t12 [3], kp1, kp2 [n, 2], unc [n]) for Pinhole::epipolarConstrain with the EuRoC camera on both sides.
    The first, 1950 pairs: a point seen by both cameras, the second keypoint moved off its epipolar line (computed here in float64) by
    f * sqrt(3.84 * unc) px along the line's normal, f in {0, 0.5, 0.9, 0.99, 0.999, 0.9999, 1.0001, 1.001, 1.01, 1.1, 2} on either side,
    unc = mvLevelSigma2 of a random octave.  The second, 50 pairs: t12 = 0, so F12 = 0 and den == 0."""
    def make():
        rng = np.random.default_rng(77)
        fx, fy, cx, cy = (float(v) for v in PINHOLE)
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
        R12 = _rot(0.02, -0.05, 0.01)
        t12 = np.array([0.30, 0.02, 0.05])
        tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
        F12 = np.linalg.inv(K.T) @ tx @ R12 @ np.linalg.inv(K)
        factors = (0.0, 0.5, 0.9, 0.99, 0.999, 0.9999, 1.0001, 1.001, 1.01, 1.1, 2.0)
        n = 1950
        kp1, kp2, unc = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros(n, f32)
        for i in range(n):
            z = math.exp(rng.uniform(math.log(1.0), math.log(20.0)))
            X2 = np.array([rng.uniform(-0.6, 0.6) * z, rng.uniform(-0.4, 0.4) * z, z])
            X1 = R12 @ X2 + t12
            x1 = K @ (X1 / X1[2])
            x2 = K @ (X2 / X2[2])
            line = F12.T @ x1                                 # l = x1' F12 = [a b c]
            nrm = line[:2] / np.linalg.norm(line[:2])
            unc[i] = M.LEVEL_SIGMA2[rng.integers(0, 8)]
            f = factors[i % len(factors)] * (1.0 if (i // len(factors)) % 2 else -1.0)
            x2f = x2[:2] - nrm * (line @ x2) / np.linalg.norm(line[:2])          # onto the line, then off it
            kp1[i], kp2[i] = x1[:2], x2f + nrm * f * math.sqrt(3.84 * float(unc[i]))
        g1 = dict(R12=R12.astype(f32), t12=t12.astype(f32), kp1=kp1.astype(f32), kp2=kp2.astype(f32), unc=unc)
        m = 50
        g2 = dict(R12=_rot(-0.01, 0.03, 0.2).astype(f32), t12=np.zeros(3, f32), kp1=rng.uniform(0, 752, (m, 2)).astype(f32),
                  kp2=rng.uniform(0, 480, (m, 2)).astype(f32), unc=M.LEVEL_SIGMA2[rng.integers(0, 8, m)])
        return [g1, g2]
    return _once("epipolar", make)
