"""Inputs of tests/test_ref_matcher.py and tests/test_gpu_ref_matcher.py: small scenes on which the decisive rules of ORBmatcher.cc decide.

Every scene is a dict of plain numpy arrays in the layout the oracle's orc_* functions take (oracle/orb_oracle.h), so that the compiled
reference text (oracle/ref_match_driver.cc), the oracle and the product get the very same arrays.  The shapes are the smallest at
which the rules still bite, not the workload's: 300 to 500 keypoints per image, 8 levels at 1.2, 200 to 500 map points, a few dozen
BoW nodes.  Keypoints come in small clusters so that a search window holds several candidates; descriptors are a cluster prototype
with a few flipped bits, so that Hamming ties, near-threshold ratios and the <= edges are common instead of one-in-a-million.

census_*() replay one member in plain Python, candidate by candidate, and count the situations DESIGN.md section 2 lists.  The replay
is test infrastructure of the census only: test_ref_matcher.py first asserts that it reproduces the compiled text's outputs on the
scene, then asserts every count at or above its minimum.
"""
import math

import numpy as np

f32 = np.float32
NLEVELS = 8
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30
BOUNDS = {"euroc": (0.0, 752.0, 0.0, 480.0),
          "distorted": (-31.4375, 790.1875, -22.71875, 505.90625)}      # undistorted bounds with a negative origin
PINHOLE = np.array([458.654, 457.296, 367.215, 248.375], f32)
KB8 = np.array([190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504,
                0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182], f32)
KB8_BOUNDS = (0.0, 512.0, 0.0, 512.0)
BOW_LOOKALIKES = 4
COMMON_ROTATIONS, COMMON_SHARES = (37.0, 100.0, 190.0), (0.5, 0.28, 0.22)
COMMON_BOW = (30.0, 120.0, 210.0)             # bins 1, 4 and 7

_cache = {}


def once(key, make):
    """Every scene is made once and shared; tests must leave it unchanged."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def scale_factors(nlevels=NLEVELS, factor=1.2):
    sf = np.ones(nlevels, f32)
    for i in range(1, nlevels):
        sf[i] = f32(sf[i - 1] * f32(factor))
    return sf


SF = scale_factors()
LOG_SF = float(f32(math.log(float(f32(1.2)))))


def flip(d, nbits, rng):
    """d with exactly nbits distinct bits flipped."""
    d = d.copy()
    for b in rng.choice(256, int(nbits), replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def project(cam_type, cam, Xc):
    """float64 projection, good enough to place keypoints; the searches compute their own."""
    Xc = np.asarray(Xc, np.float64)
    x, y, z = Xc[..., 0], Xc[..., 1], Xc[..., 2]
    if cam_type == 0:
        return np.stack([cam[0] * x / z + cam[2], cam[1] * y / z + cam[3]], -1)
    th = np.arctan2(np.hypot(x, y), z)
    psi = np.arctan2(y, x)
    r = th + cam[4] * th ** 3 + cam[5] * th ** 5 + cam[6] * th ** 7 + cam[7] * th ** 9
    return np.stack([cam[0] * r * np.cos(psi) + cam[2], cam[1] * r * np.sin(psi) + cam[3]], -1)


def pose(rng, angle=0.05, shift=0.3):
    """A 4 x 4 float32 rigid transform near the identity."""
    w = rng.uniform(-angle, angle, 3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = rng.uniform(-shift, shift, 3)
    return T.astype(f32)


def clustered_frame(rng, centres, levels, per=6, spread=5.0, bounds=BOUNDS["euroc"], protos=None, max_flips=14, angle0=None):
    """Keypoints in clusters around `centres`: positions within +-spread, octave = the cluster's level or the next one, descriptor =
    the cluster's prototype with up to max_flips bits flipped, angle = angle0 of the cluster + a few degrees."""
    n = len(centres)
    if protos is None:
        protos = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if angle0 is None:
        angle0 = rng.uniform(0, 360, n)
    kx, ky, octv, ang, desc, owner = [], [], [], [], [], []
    for c in range(n):
        for _ in range(per):
            x = float(np.clip(centres[c][0] + rng.uniform(-spread, spread), bounds[0] + 0.5, bounds[1] - 0.5))
            y = float(np.clip(centres[c][1] + rng.uniform(-spread, spread), bounds[2] + 0.5, bounds[3] - 0.5))
            kx.append(x); ky.append(y)
            octv.append(int(np.clip(levels[c] + rng.integers(-1, 2), 0, NLEVELS - 1)))
            ang.append(float((angle0[c] + rng.uniform(-4, 4)) % 360.0))
            desc.append(flip(protos[c], rng.integers(0, max_flips + 1), rng))
            owner.append(c)
    order = rng.permutation(len(kx))                       # keypoint order is not cluster order: the grid cells decide the scan order
    a = lambda v, t: np.ascontiguousarray(np.asarray(v, t)[order])
    return dict(kx=a(kx, f32), ky=a(ky, f32), octave=a(octv, np.int32), angle=a(ang, f32), desc=a(desc, np.uint8), owner=a(owner, np.int32),
                protos=protos, angle0=np.asarray(angle0), bounds=tuple(float(b) for b in bounds))


def centres_in(rng, n, bounds, margin=20.0):
    return np.stack([rng.uniform(bounds[0] + margin, bounds[1] - margin, n), rng.uniform(bounds[2] + margin, bounds[3] - margin, n)], 1)


def occupy(rng, n, share=0.15):
    """slot / slot_obs with `share` of the keypoints taken by points that are no query (tag 100000 + i), half of them observed."""
    slot = np.full(n, -1, np.int32)
    obs = np.zeros(n, np.uint8)
    taken = rng.random(n) < share
    slot[taken] = 100000 + np.flatnonzero(taken)
    obs[taken] = rng.integers(0, 2, int(taken.sum()))
    return slot, obs


# ---- SearchByProjection(Frame, MapPoints) ----------------------------------------------------------------------------------------------
def local_points(name):
    """mono / rectified stereo: name in ("mono", "stereo", "distorted")."""
    def make():
        rng = np.random.default_rng({"mono": 101, "stereo": 102, "distorted": 103}[name])
        bounds = BOUNDS["distorted" if name == "distorted" else "euroc"]
        nc = 70
        centres = centres_in(rng, nc, bounds)
        levels = rng.integers(0, NLEVELS, nc)
        levels[:8] = 0
        levels[8:16] = NLEVELS - 1
        fr = clustered_frame(rng, centres, levels, per=6, bounds=bounds)
        N = len(fr["kx"])
        if name != "mono":
            ur = fr["kx"] - rng.uniform(2, 40, N).astype(f32)
            ur[rng.random(N) < 0.35] = -1.0
            fr["u_right"] = ur.astype(f32)
        else:
            fr["u_right"] = None
        fr["slot"], fr["slot_obs"] = occupy(rng, N)
        nq = 420
        q = dict(in_view=np.ones(nq, np.uint8), bad=np.zeros(nq, np.uint8), desc=np.zeros((nq, 32), np.uint8), projX=np.zeros(nq, f32),
                 projY=np.zeros(nq, f32), projXR=np.zeros(nq, f32), viewCos=np.zeros(nq, f32), level=np.zeros(nq, np.int32),
                 obs=np.ones(nq, np.uint8), depth=rng.uniform(1, 40, nq).astype(f32))
        th = 3.0
        for i in range(nq):
            c = int(rng.integers(0, nc))
            members = np.flatnonzero(fr["owner"] == c)
            m = int(rng.choice(members))
            q["projX"][i] = fr["kx"][m] + f32(rng.uniform(-3, 3))
            q["projY"][i] = fr["ky"][m] + f32(rng.uniform(-3, 3))
            q["level"][i] = int(np.clip(levels[c] + rng.integers(0, 2), 0, NLEVELS - 1))
            q["viewCos"][i] = f32(rng.choice([0.9, 0.9979, 0.998, 0.99801, 0.9999]))
            q["desc"][i] = flip(fr["protos"][c], rng.integers(0, 30), rng)
            r = f32(f32(2.5 if float(q["viewCos"][i]) > 0.998 else 4.0) * f32(th)) * SF[q["level"][i]]
            if fr["u_right"] is not None:
                base = fr["u_right"][m] if fr["u_right"][m] > 0 else q["projX"][i] - f32(10)
                kind = i % 6
                if kind == 0:
                    q["projXR"][i] = f32(base + r)                              # er == r (kept) up to the rounding of the difference
                elif kind == 1:
                    q["projXR"][i] = np.nextafter(f32(base + r), f32(np.inf))   # one step beyond
                elif kind == 2:
                    q["projXR"][i] = np.nextafter(f32(base - r), f32(-np.inf))
                else:
                    q["projXR"][i] = f32(base + rng.uniform(-0.8, 0.8) * r)
        q["obs"][rng.random(nq) < 0.3] = 0
        q["in_view"][rng.random(nq) < 0.05] = 0
        q["bad"][rng.random(nq) < 0.05] = 1
        # the <= TH_HIGH edge: a lone keypoint far from every cluster, its query exactly 100 (kept) or 101 (dropped) bits away
        edge = []
        for k in range(12):
            i = nq - 1 - k
            m = k * 7
            fr["kx"][m], fr["ky"][m] = f32(bounds[0] + 20 + 55 * k), f32(bounds[3] - 12)     # more than two windows apart
            fr["octave"][m] = 2
            fr["slot"][m] = -1
            if fr["u_right"] is not None:
                fr["u_right"][m] = -1.0
            q["projX"][i], q["projY"][i], q["level"][i], q["viewCos"][i] = fr["kx"][m], fr["ky"][m], 2, f32(0.9999)
            q["desc"][i] = flip(fr["desc"][m], TH_HIGH + (k % 2), rng)
            q["in_view"][i], q["bad"][i], q["depth"][i] = 1, 0, 1.0
            edge.append((i, m, TH_HIGH + (k % 2)))
        return dict(frame=fr, q=q, th=th, nnratio=0.8, th_far=20.0, edge=edge)
    return once(("local", name), make)


def local_points_fisheye():
    def make():
        rng = np.random.default_rng(111)
        nc = 55
        cl, cr = centres_in(rng, nc, KB8_BOUNDS), centres_in(rng, nc, KB8_BOUNDS)
        levels = rng.integers(0, NLEVELS, nc)
        protos = rng.integers(0, 256, (nc, 32), dtype=np.uint8)
        L = clustered_frame(rng, cl, levels, per=6, bounds=KB8_BOUNDS, protos=protos)
        R = clustered_frame(rng, cr, levels, per=6, bounds=KB8_BOUNDS, protos=protos)
        nl, nr = len(L["kx"]), len(R["kx"])
        l2r, r2l = np.full(nl, -1, np.int32), np.full(nr, -1, np.int32)
        for a, b in zip(rng.permutation(nl)[:120], rng.permutation(nr)[:120]):
            l2r[a], r2l[b] = b, a
        slot, obs = occupy(rng, nl + nr)
        nq = 320
        q = dict(in_view=(rng.random(nq) < 0.8).astype(np.uint8), in_view_r=(rng.random(nq) < 0.7).astype(np.uint8),
                 desc=np.zeros((nq, 32), np.uint8), obs=(rng.random(nq) < 0.7).astype(np.uint8))
        for k in ("projX", "projY", "projXR", "projYR", "viewCos", "viewCosR"):
            q[k] = np.zeros(nq, f32)
        q["level"], q["levelR"] = np.zeros(nq, np.int32), np.zeros(nq, np.int32)
        for i in range(nq):
            c = int(rng.integers(0, nc))
            q["projX"][i], q["projY"][i] = cl[c] + rng.uniform(-4, 4, 2)
            q["projXR"][i], q["projYR"][i] = cr[c] + rng.uniform(-4, 4, 2)
            q["level"][i] = int(np.clip(levels[c] + rng.integers(0, 2), 0, NLEVELS - 1))
            q["levelR"][i] = -1 if rng.random() < 0.1 else int(np.clip(levels[c] + rng.integers(0, 2), 0, NLEVELS - 1))
            q["viewCos"][i], q["viewCosR"][i] = rng.choice([0.9, 0.998, 0.9999], 2)
            q["desc"][i] = flip(protos[c], rng.integers(0, 30), rng)
        return dict(left=L, right=R, l2r=l2r, r2l=r2l, slot=slot, slot_obs=obs, q=q, th=3.0, nnratio=0.8)
    return once("local-fisheye", make)


# ---- the two pose searches: SearchByProjection(Frame, Frame) and (Frame, KeyFrame) ---------------------------------------------------
def _world_scene(rng, cam_type, cam, bounds, n, Tcw, per=5, max_flips=14):
    """n world points in front of the camera Tcw, each with a cluster of current-frame keypoints around its projection."""
    z = rng.uniform(2.0, 12.0, n)
    if cam_type == 0:
        uv = centres_in(rng, n, bounds, margin=25.0)
        Xc = np.stack([(uv[:, 0] - cam[2]) / cam[0] * z, (uv[:, 1] - cam[3]) / cam[1] * z, z], 1)
    else:
        a, rad = rng.uniform(0, 2 * math.pi, n), rng.uniform(0.05, 1.0, n)
        Xc = np.stack([np.tan(rad) * np.cos(a) * z, np.tan(rad) * np.sin(a) * z, z], 1)
    T = Tcw.astype(np.float64)
    Xw = (Xc - T[:3, 3]) @ T[:3, :3]                      # R^T (Xc - t)
    return Xc, Xw.astype(f32)


def last_frame_open():
    """SearchByProjection(Frame, Frame) with open windows: a stereo frame without right coordinates moving forward, every last
    keypoint at octave 0 (GetFeaturesInArea(u, v, r, 0): no level filter) and th so large that the window holds the whole grid.
    Every query then sees every keypoint, in grid order.  120 keypoints in a 16-descriptor alphabet: most best distances are
    shared by several keypoints, and the first in (cell, index) order must win.  On the device this is the shape (at most 128
    keypoints, no right coordinates, only open queries) at which the matrix-pipe engines serve a single call."""
    def make():
        rng = np.random.default_rng(207)
        bounds = BOUNDS["euroc"]
        N, n = 120, 300
        alphabet = rng.integers(0, 256, (16, 32), dtype=np.uint8)
        letter = rng.integers(0, 16, N)
        cur = dict(kx=rng.uniform(bounds[0] + 2, bounds[1] - 2, N).astype(f32), ky=rng.uniform(bounds[2] + 2, bounds[3] - 12, N).astype(f32),
                   octave=rng.integers(0, NLEVELS, N).astype(np.int32), angle=rng.uniform(0, 360, N).astype(f32),
                   desc=np.ascontiguousarray(alphabet[letter]), bounds=bounds, u_right=None)
        cur["ky"][:4] = f32(bounds[3] - 1)                  # four keypoints PosInGrid leaves out: never candidates
        cur["slot"], cur["slot_obs"] = occupy(rng, N, share=0.2)
        Tcw, Tlw = pose(rng), pose(rng)
        Tlw[2, 3] = Tcw[2, 3] + f32(0.6)                    # forward: tlc.z > mb
        Xc, Xw = _world_scene(rng, 0, PINHOLE, bounds, n, Tcw)
        has_mp = rng.choice([0, 1, 1, 1, 1, 1, 1, 2], n).astype(np.uint8)
        want = rng.integers(0, 16, n)
        flips = rng.choice([0, 0, 3, 40, TH_HIGH, TH_HIGH + 1, 120], n)           # the <= TH_HIGH edge: other letters are ~128 away
        mpdesc = np.stack([flip(alphabet[w], k, rng) for w, k in zip(want, flips)])
        last_angle = ((rng.choice([37.0, 100.0, 190.0], n) + rng.uniform(-5, 5, n)) % 360.0).astype(f32)
        T = Tcw.astype(np.float64)
        for k in range(10):                                  # behind the camera
            Xw[k] = ((np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), -rng.uniform(0.5, 5)]) - T[:3, 3]) @ T[:3, :3]).astype(f32)
        return dict(cur=cur, n=n, has_mp=has_mp, Xw=np.ascontiguousarray(Xw, f32), mpdesc=mpdesc, last_octave=np.zeros(n, np.int32),
                    last_angle=last_angle, Tcw=Tcw, Tlw=Tlw, cam_type=0, cam=PINHOLE, th=4000.0, mono=False, mb=0.11, mbf=50.0,
                    obs=(rng.random(n) < 0.7).astype(np.uint8), letter=letter, want=want, flips=flips)
    return once("last-open", make)


def last_frame(name):
    """name: "mono", "stereo-forward", "stereo-backward", "stereo-still", "distorted", "rig"."""
    def make():
        rng = np.random.default_rng({"mono": 201, "stereo-forward": 202, "stereo-backward": 203, "stereo-still": 204, "distorted": 205, "rig": 206}[name])
        rig = name == "rig"
        cam_type, cam = (1, KB8) if rig else (0, PINHOLE)
        bounds = KB8_BOUNDS if rig else BOUNDS["distorted" if name == "distorted" else "euroc"]
        Tcw, Tlw = pose(rng), pose(rng)
        if name == "stereo-forward":
            Tlw[2, 3] = Tcw[2, 3] + f32(0.6)
        if name == "stereo-backward":
            Tlw[2, 3] = Tcw[2, 3] - f32(0.6)
        n = 300
        Xc, Xw = _world_scene(rng, cam_type, cam, bounds, n, Tcw)
        uv = project(cam_type, cam, Xc)
        levels = rng.integers(0, NLEVELS, n)
        common = 37.0                                     # the camera rolled by this much between the frames
        cur = clustered_frame(rng, uv[:80], levels[:80], per=5, bounds=bounds)
        N = len(cur["kx"])
        mb, mbf = 0.11, 0.11 * float(cam[0])
        if name.startswith("stereo") or name == "distorted":
            zc = Xc[cur["owner"], 2]
            ur = cur["kx"] - (mbf / zc).astype(f32) + rng.uniform(-6, 6, N).astype(f32)
            ur[rng.random(N) < 0.3] = -1.0
            cur["u_right"] = ur.astype(f32)
        else:
            cur["u_right"] = None
        cur["slot"], cur["slot_obs"] = occupy(rng, N)
        owner_of = rng.integers(0, 80, n)                  # every last keypoint looks at one of the 80 clustered points
        Xw = Xw[owner_of] + rng.normal(0, 0.004, (n, 3)).astype(f32)
        has_mp = (rng.random(n) < 0.9).astype(np.uint8)
        has_mp[rng.random(n) < 0.05] = 2
        last_octave = np.clip(levels[owner_of] + rng.integers(-1, 2, n), 0, NLEVELS - 1).astype(np.int32)
        last_angle = ((cur["angle0"][owner_of] + common + rng.uniform(-5, 5, n)) % 360.0).astype(f32)
        wild = rng.random(n) < 0.12                        # rotations that fall outside the three main bins
        last_angle[wild] = rng.uniform(0, 360, int(wild.sum())).astype(f32)
        mpdesc = np.stack([flip(cur["protos"][c], rng.integers(0, 40), rng) for c in owner_of])
        Tc = Tcw.astype(np.float64)
        # the <= TH_HIGH edge and the histogram wrap: lone keypoints below every cluster's reach
        extra, edge, wrap = 16, [], []
        for k in range(extra):
            i, c = n - 1 - k, k                             # one cluster each
            m = int(np.flatnonzero(cur["owner"] == c)[0])
            take = np.flatnonzero(owner_of == c)
            has_mp[take[take < n - extra]] = 0             # nobody else looks at this cluster
            mpdesc[i] = flip(cur["desc"][m], TH_HIGH + (k % 2) if k < 10 else 3, rng)
            owner_of[i], has_mp[i], last_octave[i] = c, 1, cur["octave"][m]
            Xw[i] = ((Xc[c] - Tc[:3, 3]) @ Tc[:3, :3]).astype(f32)
            others = np.flatnonzero(cur["owner"] == c)[1:]
            cur["desc"][others] = rng.integers(0, 256, (len(others), 32), dtype=np.uint8)          # strangers, about 128 bits away
            cur["octave"][m] = last_octave[i]
            cur["slot"][m] = -1
            if cur["u_right"] is not None:
                cur["u_right"][m] = -1.0
            if k >= 10:                                    # rot = 900 +- 14: round(rot / 30) == HISTO_LENGTH, the bin that wraps to 0
                last_angle[i] = f32(cur["angle"][m] + 900.0 + rng.uniform(-14, 14))
                wrap.append((i, m))
            else:
                edge.append((i, m, TH_HIGH + (k % 2)))
        for k in range(14):                                # behind the camera: invzc < 0
            Xcb = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), -rng.uniform(0.5, 5)])
            Xw[k] = ((Xcb - Tc[:3, 3]) @ Tc[:3, :3]).astype(f32)
            has_mp[k] = 1
        if not rig:                                        # just outside and just inside each bound, by less than a pixel
            for k in range(32):
                side, z = k % 4, rng.uniform(3, 8)
                off = rng.uniform(0.05, 0.9) * (1 if k % 8 < 4 else -1)
                u = (bounds[0] - off, bounds[1] + off, rng.uniform(bounds[0] + 30, bounds[1] - 30), rng.uniform(bounds[0] + 30, bounds[1] - 30))[side]
                v = (rng.uniform(bounds[2] + 30, bounds[3] - 30), rng.uniform(bounds[2] + 30, bounds[3] - 30), bounds[2] - off, bounds[3] + off)[side]
                Xce = np.array([(u - cam[2]) / cam[0] * z, (v - cam[3]) / cam[1] * z, z])
                Xw[14 + k] = ((Xce - Tc[:3, 3]) @ Tc[:3, :3]).astype(f32)
                has_mp[14 + k] = 1
        d = dict(edge=edge, wrap=wrap, cur=cur, n=n, has_mp=has_mp, Xw=np.ascontiguousarray(Xw, f32), mpdesc=mpdesc, last_octave=last_octave, last_angle=last_angle,
                 Tcw=Tcw, Tlw=Tlw, cam_type=cam_type, cam=cam, th=7.0 if name == "mono" else 15.0, mono=name == "mono",
                 mb=mb, mbf=mbf, obs=(rng.random(n) < 0.7).astype(np.uint8))
        if rig:
            Trl = np.eye(4, dtype=f32)[:3]
            Trl[:3, :3] = pose(rng, 0.02, 0.0)[:3, :3]
            Trl[0, 3] = f32(-0.101)
            Xr = Xc[:80] @ Trl[:3, :3].astype(np.float64).T + Trl[:3, 3]
            right = clustered_frame(rng, project(1, KB8, Xr), levels[:80], per=5, bounds=bounds, protos=cur["protos"], angle0=cur["angle0"])
            d["right"], d["Trl"] = right, np.ascontiguousarray(Trl)
            d["slot"], d["slot_obs"] = occupy(rng, N + len(right["kx"]))
            d["mono"] = False
        return d
    return once(("last", name), make)


def reloc_keyframe(name):
    """SearchByProjection(Frame, KeyFrame, sAlreadyFound): name in ("pinhole", "distorted", "kb8")."""
    def make():
        rng = np.random.default_rng({"pinhole": 301, "distorted": 302, "kb8": 303}[name])
        cam_type, cam = (1, KB8) if name == "kb8" else (0, PINHOLE)
        bounds = KB8_BOUNDS if name == "kb8" else BOUNDS["distorted" if name == "distorted" else "euroc"]
        Tcw = pose(rng)
        n = 320
        Xc, Xw = _world_scene(rng, cam_type, cam, bounds, 80, Tcw)
        uv = project(cam_type, cam, Xc)
        T = Tcw.astype(np.float64)
        Ow = -T[:3, :3].T @ T[:3, 3]
        dist = np.linalg.norm(Xw.astype(np.float64) - Ow, axis=1)
        want = rng.integers(-2, NLEVELS + 2, 80)          # the predicted level before the clamp: below 0 and beyond the top included
        want[:12], want[12:24] = 0, NLEVELS - 1
        levels = np.clip(want, 0, NLEVELS - 1)
        cur = clustered_frame(rng, uv, levels, per=5, bounds=bounds)
        cur["u_right"] = None
        cur["slot"], cur["slot_obs"] = occupy(rng, len(cur["kx"]))
        owner_of = rng.integers(0, 80, n)
        ratio = 1.2 ** (want[owner_of] - rng.uniform(0.05, 0.95, n))          # ceil(log(ratio) / log 1.2) == want
        max_dist = (dist[owner_of] * ratio).astype(f32)
        min_dist = (max_dist / f32(1.2 ** 7.5)).astype(f32)
        edge = rng.random(n) < 0.1                         # outside the invariance band on either side
        max_dist[edge] = (dist[owner_of][edge] / 1.2 * rng.choice([0.999, 1.001], int(edge.sum()))).astype(f32)
        state = rng.choice([0, 1, 1, 1, 1, 1, 1, 2, 3], n).astype(np.uint8)
        # three common rotations fill bins 1, 3 and 6; the wrapping bin 0 then stays outside the three maxima, so a pair that wraps
        # into it is pruned and one that landed in bin 1 would be kept: the wrap decides
        kf_angle = ((cur["angle0"][owner_of] + rng.choice(COMMON_ROTATIONS, n, p=COMMON_SHARES) + rng.uniform(-5, 5, n)) % 360.0).astype(f32)
        wild = rng.random(n) < 0.12
        kf_angle[wild] = rng.uniform(0, 360, int(wild.sum())).astype(f32)
        mpdesc = np.stack([flip(cur["protos"][c], rng.integers(0, 40), rng) for c in owner_of])
        Xq = Xw[owner_of] + rng.normal(0, 0.003, (n, 3)).astype(f32)
        orb_dist, edge, wrap = 64, [], []
        for k in range(16):                                # the <= ORBdist edge and the wrapping bin, on lone keypoints
            i, c = n - 1 - k, k                             # one cluster each
            m = int(np.flatnonzero(cur["owner"] == c)[0])
            take = np.flatnonzero(owner_of == c)
            state[take[take < n - 16]] = 0
            mpdesc[i] = flip(cur["desc"][m], orb_dist + (k % 2) if k < 10 else 3, rng)
            owner_of[i], state[i] = c, 1
            Xq[i] = Xw[c]
            max_dist[i], min_dist[i] = f32(dist[c] * 1.2 ** (levels[c] - 0.5)), f32(0.01)
            others = np.flatnonzero(cur["owner"] == c)[1:]
            cur["desc"][others] = rng.integers(0, 256, (len(others), 32), dtype=np.uint8)          # strangers, about 128 bits away
            cur["octave"][m] = levels[c]
            cur["slot"][m] = -1
            if k >= 10:
                kf_angle[i] = f32(cur["angle"][m] + 900.0 + rng.uniform(-14, 14))
                wrap.append((i, m))
            else:
                edge.append((i, m, orb_dist + (k % 2)))
        return dict(edge=edge, wrap=wrap, cur=cur, n=n, state=state, Xw=np.ascontiguousarray(Xq, f32), mpdesc=mpdesc, kf_angle=kf_angle, max_dist=max_dist, min_dist=min_dist,
                    Tcw=Tcw, cam_type=cam_type, cam=cam, th=10.0, orb_dist=orb_dist)
    return once(("reloc", name), make)


# ---- SearchByBoW(KeyFrame, Frame) ------------------------------------------------------------------------------------------------------
def bow(name):
    """name: "mono" (F.Nleft == -1), "fisheye" (F.Nleft != -1, keyframe with one camera), "rig" (both with two cameras)."""
    def make():
        rng = np.random.default_rng({"mono": 401, "fisheye": 402, "rig": 403}[name])
        nodes = 44
        node_ids = np.sort(rng.choice(2000, nodes + 4, replace=False))         # each side lacks four of them: the lower_bound jumps
        kf_nodes = set(node_ids[rng.permutation(nodes + 4)[:nodes]].tolist())
        f_nodes = set(node_ids[rng.permutation(nodes + 4)[:nodes]].tolist())
        protos = {int(nid): rng.integers(0, 256, (BOW_LOOKALIKES, 32), dtype=np.uint8) for nid in node_ids}   # a few look-alikes per node

        def side(nset, n, salt):
            ids = sorted(nset)
            node_of = rng.choice(ids, n)
            which = rng.integers(0, BOW_LOOKALIKES, n)
            flips = rng.integers(0, 13, n) if salt else rng.choice([3, 7, 11], n)      # the frame's few distinct counts make ties
            desc = np.stack([flip(protos[int(a)][b], k, rng) for a, b, k in zip(node_of, which, flips)])
            keys = np.zeros(n, dtype=[("x", f32), ("y", f32), ("octave", np.int32), ("angle", f32)])
            keys["x"], keys["y"] = rng.uniform(5, 700, n), rng.uniform(5, 470, n)
            keys["octave"] = rng.integers(0, NLEVELS, n)
            # the keyframe is rolled against the frame by one of three common rotations (bins 1, 4 and 7): bin 0 stays outside the maxima, bin 1 inside
            base = (which * 1.0 + (rng.choice(COMMON_BOW, n) if salt else 0.0) + rng.uniform(-4, 4, n)) % 360.0
            wild = rng.random(n) < 0.1
            base[wild] = rng.uniform(0, 360, int(wild.sum()))
            keys["angle"] = base
            fv = {}
            for i in rng.permutation(n):
                fv.setdefault(int(node_of[i]), []).append(int(i))
            return keys, desc, fv, node_of, which

        kk, kd, kfv, knode, kwhich = side(kf_nodes, 420, 1)
        fk, fd, ffv, fnode, fwhich = side(f_nodes, 440, 0)
        has_mp = rng.choice([0, 1, 1, 1, 1, 1, 2], 420).astype(np.uint8)
        n_left = -1 if name == "mono" else 260
        kf_n_left = 250 if name == "rig" else -1
        # the <= TH_LOW edge: a keyframe keypoint alone in its node against a lone frame keypoint exactly 50 / 51 bits away
        shared = [int(n) for n in node_ids if n in kf_nodes and n in f_nodes]
        if n_left != -1:                                                  # a node needs a left and a right frame keypoint
            shared = [n for n in shared if min(ffv[n]) < n_left <= max(ffv[n])]
        lone = shared[:16]
        assert len(lone) == 16
        edge, wrap, edge_r, wrap_r = [], [], [], []
        for k, nid in enumerate(lone):
            ki = kfv[nid][0]
            for j in kfv[nid][1:]:
                has_mp[j] = 0
            has_mp[ki] = 1
            for j in ffv[nid]:
                fd[j] = rng.integers(0, 256, 32, dtype=np.uint8)         # ~128 bits from everything
            if n_left == -1:
                fi = ffv[nid][0]
                if k >= 12:                                               # the wrapping bin
                    fd[fi] = flip(kd[ki], 2, rng)
                    kk["angle"][ki] = f32(fk["angle"][fi] + 900.0 + rng.uniform(-14, 14))
                    wrap.append((ki, fi))
                else:
                    fd[fi] = flip(kd[ki], TH_LOW + (k % 2), rng)
                    edge.append((ki, fi, TH_LOW + (k % 2)))
                continue
            # a fisheye-stereo frame: the right image's best is accepted only inside `bestDist1 <= TH_LOW` of the left one (:377,
            # :407), so every planted right keypoint has a left partner two bits from the keyframe's descriptor
            fi = next(j for j in ffv[nid] if j < n_left)
            fj = next(j for j in ffv[nid] if j >= n_left)
            fd[fi] = flip(kd[ki], 2, rng)
            if k < 10:                                                    # the right image's own <= TH_LOW edge (:407)
                fd[fj] = flip(kd[ki], TH_LOW + (k % 2), rng)
                kk["angle"][ki] = f32(fk["angle"][fi] + COMMON_BOW[0])
                fk["angle"][fj] = fk["angle"][fi]
                edge_r.append((ki, fj, TH_LOW + (k % 2)))
            elif k < 13:                                                  # both images wrap (one keyframe angle serves both pairs)
                fd[fj] = flip(kd[ki], 3, rng)
                fk["angle"][fj] = f32((fk["angle"][fi] + 1.0) % 360.0)
                kk["angle"][ki] = f32(max(fk["angle"][fi], fk["angle"][fj]) + 900.0 + rng.uniform(-12, 12))
                wrap.append((ki, fi))
                wrap_r.append((ki, fj))
            else:                                                         # three more of the edge, on the kept side
                fd[fj] = flip(kd[ki], TH_LOW, rng)
                kk["angle"][ki] = f32(fk["angle"][fi] + COMMON_BOW[0])
                fk["angle"][fj] = fk["angle"][fi]
                edge_r.append((ki, fj, TH_LOW))
        return dict(edge=edge, wrap=wrap, edge_r=edge_r, wrap_r=wrap_r, kf_keys=kk, kf_desc=kd, kf_fv=kfv, has_mp=has_mp, f_keys=fk, f_desc=fd, f_fv=ffv,
                    n_left=n_left, kf_n_left=kf_n_left, nnratio=0.7)
    return once(("bow", name), make)


# ---- SearchForInitialization -------------------------------------------------------------------------------------------------------
def initialization(name):
    def make():
        rng = np.random.default_rng({"euroc": 501, "distorted": 502}[name])
        bounds = BOUNDS[name]
        nc = 75
        centres = centres_in(rng, nc, bounds, margin=30.0)
        levels = np.zeros(nc, np.int64)
        f2 = clustered_frame(rng, centres, levels, per=5, spread=20.0, bounds=bounds, max_flips=20)
        f2["octave"][rng.random(len(f2["kx"])) < 0.6] = 0
        f2["u_right"] = None
        n1 = 400
        keys1 = np.zeros(n1, dtype=[("x", f32), ("y", f32), ("octave", np.int32), ("angle", f32)])
        c1 = rng.integers(0, nc, n1)
        keys1["x"], keys1["y"] = centres[c1, 0] + rng.uniform(-25, 25, n1), centres[c1, 1] + rng.uniform(-25, 25, n1)
        keys1["octave"] = rng.choice([0, 0, 0, 0, 1, 2], n1)
        ang = (f2["angle0"][c1] + rng.choice(COMMON_ROTATIONS, n1, p=COMMON_SHARES) + rng.uniform(-5, 5, n1)) % 360.0     # see reloc_keyframe
        wild = rng.random(n1) < 0.12
        ang[wild] = rng.uniform(0, 360, int(wild.sum()))
        keys1["angle"] = ang
        desc1 = np.stack([flip(f2["protos"][c], rng.integers(0, 36), rng) for c in c1])
        edge, wrap = [], []
        for k in range(14):                                # the <= TH_LOW edge and the wrapping bin, far from every cluster
            i, m = n1 - 1 - k, k * 5
            f2["kx"][m], f2["ky"][m], f2["octave"][m] = f32(bounds[0] + 8), f32(bounds[2] + 8 + 30 * k), 0
            keys1["x"][i], keys1["y"][i], keys1["octave"][i] = f2["kx"][m], f2["ky"][m], 0
            desc1[i] = flip(f2["desc"][m], TH_LOW + (k % 2) if k < 10 else 2, rng)
            if k >= 10:
                keys1["angle"][i] = f32(f2["angle"][m] + 900.0 + rng.uniform(-14, 14))
                wrap.append((i, m))
            else:
                edge.append((i, m, TH_LOW + (k % 2)))
        prev = np.ascontiguousarray(np.stack([keys1["x"], keys1["y"]], 1), f32)
        return dict(edge=edge, wrap=wrap, f2=f2, keys1=keys1, desc1=desc1, prev=prev, window=14 if name == "euroc" else 20, nnratio=0.9)
    return once(("init", name), make)


# ---- ComputeThreeMaxima / DescriptorDistance / RadiusByViewingCos ----------------------------------------------------------------------
def three_maxima_cases():
    rng = np.random.default_rng(601)
    cases = [np.zeros(30, np.int32), np.full(30, 4, np.int32)]                # nothing; all equal (equal maxima: the first three win)
    a = np.zeros(30, np.int32); a[7] = 100; a[3] = 9; a[20] = 9; cases.append(a)          # max2 < 0.1f * max1: a lone peak
    a = np.zeros(30, np.int32); a[7] = 100; a[3] = 10; a[20] = 9; cases.append(a)         # max2 exactly at a tenth, max3 below
    a = np.zeros(30, np.int32); a[7] = 100; a[3] = 10; a[20] = 10; cases.append(a)
    a = np.zeros(30, np.int32); a[5] = 50; a[6] = 50; a[29] = 50; a[0] = 50; cases.append(a)   # four equal maxima
    a = np.zeros(30, np.int32); a[29] = 3; a[0] = 2; a[1] = 1; cases.append(a)
    a = np.zeros(30, np.int32); a[2] = 70; a[9] = 7; a[11] = 6; cases.append(a)           # 7 == 0.1f * 70 in float? decided by the text
    for _ in range(40):
        cases.append(rng.integers(0, rng.choice([2, 5, 40, 400]), 30).astype(np.int32))
    return cases


def descriptor_pairs():
    rng = np.random.default_rng(602)
    a = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    a[0], b[0] = 0, 255
    a[1], b[1] = 0, 0
    a[2], b[2] = 0x80, 0x01                                # the sign bits of the 32-bit words
    b[3] = a[3]
    return a, b


VIEW_COS = [0.0, 0.5, 0.997, 0.998, float(np.nextafter(f32(0.998), f32(0))), float(f32(0.998)), float(np.nextafter(f32(0.998), f32(1))), 0.9981, 1.0, -1.0]


# ---- the census: one plain replay per member --------------------------------------------------------------------------------------------
class Census(dict):
    def hit(self, key, n=1):
        self[key] = self.get(key, 0) + n


def best_two(cands, dists, levels=None):
    """The first-minimum scan of the searches: (best, second, bestIdx, bestLevel, secondLevel)."""
    bd, bd2, bi, bl, bl2 = 256, 256, -1, -1, -1
    for k, (i, d) in enumerate(zip(cands, dists)):
        if d < bd:
            bd2, bd, bl2, bi = bd, d, bl, i
            bl = levels[k] if levels is not None else -1
        elif d < bd2:
            bd2 = d
            bl2 = levels[k] if levels is not None else -1
    return bd, bd2, bi, bl, bl2


def rot_bin(a1, a2):
    """The histogram bin of the pair before the wrap: round(rot * (1.0f / HISTO_LENGTH)) with rot = a1 - a2 (+ 360 below zero), in float."""
    rot = f32(f32(a1) - f32(a2))
    if rot < 0:
        rot = f32(rot + f32(360.0))
    v = float(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH))))
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)          # round(): halves away from zero


def census_local_points(S, area):
    """Replay of ORBmatcher.cc:44-143 on a mono / rectified scene; area(x, y, r, lo, hi) = the frame's GetFeaturesInArea."""
    fr, q = S["frame"], S["q"]
    slot, obs = fr["slot"].copy(), fr["slot_obs"].copy()
    c, n = Census(), 0
    ratio = f32(S["nnratio"])
    for i in range(len(q["projX"])):
        if not q["in_view"][i] or q["bad"][i]:
            continue
        lvl = int(q["level"][i])
        c.hit("level-0", lvl == 0)
        c.hit("level-top", lvl == NLEVELS - 1)
        r = f32(f32(2.5 if float(q["viewCos"][i]) > 0.998 else 4.0) * f32(S["th"]))
        rs = f32(r * SF[lvl])
        cands, dists, lv = [], [], []
        for j in area(float(q["projX"][i]), float(q["projY"][i]), float(rs), lvl - 1, lvl):
            if slot[j] >= 0:
                c.hit("occupied-observed" if obs[j] else "occupied-unobserved")
                if obs[j]:
                    continue
            if fr["u_right"] is not None and fr["u_right"][j] > 0:
                er = abs(f32(q["projXR"][i] - fr["u_right"][j]))
                c.hit("er-edge", abs(float(er) / float(rs) - 1.0) < 1e-4)
                if er > rs:
                    continue
            cands.append(int(j)); dists.append(hamming(q["desc"][i], fr["desc"][j])); lv.append(int(fr["octave"][j]))
        if not cands:
            continue
        bd, bd2, bi, bl, bl2 = best_two(cands, dists, lv)
        c.hit("tie", sorted(dists)[:2].count(bd) == 2)
        c.hit("at-TH_HIGH", bd == TH_HIGH)
        if bd <= TH_HIGH:
            c.hit("same-level" if bl == bl2 else "other-level")
            if bl == bl2 and f32(bd) > ratio * f32(bd2):
                c.hit("ratio-near", abs(bd - float(ratio) * bd2) <= 2)
                continue
            slot[bi], obs[bi] = i, q["obs"][i]
            n += 1
    return n, slot, obs, c


def census_initialization(S, area):
    """Replay of ORBmatcher.cc:722-804 without the orientation check; area = F2's GetFeaturesInArea."""
    f2, k1 = S["f2"], S["keys1"]
    n2 = len(f2["kx"])
    m12, m21, md = np.full(len(k1), -1, np.int32), np.full(n2, -1, np.int32), np.full(n2, 2 ** 31 - 1, np.int64)
    c, n = Census(), 0
    ratio = f32(S["nnratio"])
    for i in range(len(k1)):
        lvl = int(k1["octave"][i])
        if lvl > 0:
            continue
        cands, dists = [], []
        for j in area(float(S["prev"][i][0]), float(S["prev"][i][1]), float(S["window"]), lvl, lvl):
            d = hamming(S["desc1"][i], f2["desc"][j])
            if md[j] <= d:
                continue
            cands.append(int(j)); dists.append(d)
        if not cands:
            continue
        bd, bd2, bi, _, _ = best_two(cands, dists)
        bd2 = bd2 if len(cands) > 1 else 2 ** 31 - 1           # the text starts from INT_MAX, not 256
        c.hit("tie", sorted(dists)[:2].count(bd) == 2)
        c.hit("at-TH_LOW", bd == TH_LOW)
        if bd <= TH_LOW:
            if f32(bd) < f32(bd2) * ratio:
                if m21[bi] >= 0:
                    c.hit("two-claims")
                    m12[m21[bi]] = -1
                    n -= 1
                m12[i], m21[bi], md[bi] = bi, i, bd
                n += 1
            else:
                c.hit("ratio-near", abs(bd - float(ratio) * bd2) <= 2)
    return n, m12, c


def census_bow(S):
    """Replay of ORBmatcher.cc:289-452 for F.Nleft == -1 without the orientation check."""
    c, n = Census(), 0
    m = np.full(len(S["f_keys"]), -1, np.int32)
    ratio = f32(S["nnratio"])
    for nid in sorted(set(S["kf_fv"]) & set(S["f_fv"])):
        for ki in S["kf_fv"][nid]:
            if S["has_mp"][ki] != 1:
                continue
            cands, dists = [], []
            for fi in S["f_fv"][nid]:
                if m[fi] >= 0:
                    c.hit("two-claims", hamming(S["kf_desc"][ki], S["f_desc"][fi]) <= TH_LOW)      # a good candidate another keypoint holds
                    continue
                cands.append(fi); dists.append(hamming(S["kf_desc"][ki], S["f_desc"][fi]))
            if not cands:
                continue
            bd, bd2, bi, _, _ = best_two(cands, dists)
            c.hit("tie", sorted(dists)[:2].count(bd) == 2)
            c.hit("at-TH_LOW", bd == TH_LOW)
            if bd <= TH_LOW:
                if f32(bd) < ratio * f32(bd2):
                    m[bi] = ki
                    n += 1
                else:
                    c.hit("ratio-near", abs(bd - float(ratio) * bd2) <= 2)
    return n, m, c


def census_projections(S, Xw, live, Tcw):
    """Of the live world points of a pose search: how many lie behind the camera, and how many project within a pixel of a bound on
    either side (float64; the planted points keep 0.05 px away from the bound itself)."""
    T = np.asarray(Tcw, np.float64)
    Xc = np.asarray(Xw, np.float64)[live] @ T[:3, :3].T + T[:3, 3]
    c = Census()
    c.hit("behind", int((Xc[:, 2] < 0).sum()))
    front = Xc[Xc[:, 2] > 0]
    uv = project(S["cam_type"], S["cam"], front)
    b = S["cur"]["bounds"]
    out = np.maximum.reduce([b[0] - uv[:, 0], uv[:, 0] - b[1], b[2] - uv[:, 1], uv[:, 1] - b[3]])
    c.hit("outside-by-less-than-a-pixel", int(((out > 0) & (out < 1)).sum()))
    c.hit("inside-by-less-than-a-pixel", int(((out <= 0) & (out > -1)).sum()))
    return c


def census_predicted_levels(S):
    """Predicted levels of the live, in-band points of a relocalisation scene (float64 replay of MapPoint::PredictScale)."""
    T = S["Tcw"].astype(np.float64)
    Ow = -T[:3, :3].T @ T[:3, 3]
    live = S["state"] == 1
    dist = np.linalg.norm(S["Xw"].astype(np.float64)[live] - Ow, axis=1)
    maxd, mind = S["max_dist"][live].astype(np.float64), S["min_dist"][live].astype(np.float64)
    band = (dist >= 0.8 * mind) & (dist <= 1.2 * maxd)
    lv = np.ceil(np.log(maxd[band] / dist[band]) / math.log(1.2))
    c = Census()
    c.hit("level-0", int((lv <= 0).sum()))
    c.hit("level-top", int((lv >= NLEVELS - 1).sum()))
    c.hit("out-of-band", int((~band).sum()))
    return c
