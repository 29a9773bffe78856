#!/usr/bin/env python3
"""The Sim3 overload of ORBmatcher::Fuse for one point list into all corrected keyframes (the loops of LoopClosing::SearchAndFuse,
LoopClosing.cc:2631-2707): the one-call entry orbm_fuse_sim3_keyframes against the loop of T orbm_fuse_sim3_cam calls it replaces, on the
same inputs and handle.

Three synthetic shapes, built without images.  The points lie all around the origin (azimuth over the full circle, elevation within
+-30 degrees, 2-10 m away) and every keyframe looks outwards from near the origin in its own direction, so that about a fifth of the
points fall inside each keyframe's image - in loop closing most (keyframe, point) pairs fail the depth or the image-bounds gate.  A
keyframe's keypoints are the projections of points it sees, with the point's descriptor and a few flipped bits, between random ones;
Scw = s [R | t] with s in [0.9, 1.1]; 90 % of the pairs valid.
  loop correction   Pinhole, 1000 keypoints per keyframe, 4000 points, T = 40
  merge             KannalaBrandt8, 1500 keypoints per keyframe, 20 000 points, T = 100
  small             Pinhole, 1000 keypoints per keyframe, 1000 points, T = 10
Both routes are called through ctypes on structures built beforehand, so the interpreter adds one foreign call per library call and
nothing else.  --rounds rounds, the two routes alternated inside a round, --calls calls each; wall clock per call of SearchAndFuse's
search (all T keyframes) as the median and range of the rounds' means.  The rows of both routes must be identical: exit status 1
otherwise.  The result is stated by the project's rule: a gain counts when every round of the one call is below every round of the
loop AND the median gain is at least three times the loop's own spread.  Prints text lines and one JSON line and writes them to --out.
Needs a GPU; there is no fallback.

    python tools/fuse_sim3_keyframes_bench.py [--rounds 5] [--calls 20] [--only NAME] [--out profiles/fuse_sim3_keyframes_bench.txt]
"""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fuse_keyframes_scene as FS  # noqa: E402
import fuse_sim3_keyframes_scene as SS  # noqa: E402

P = lambda a: a.ctypes.data_as(C.c_void_p)
f32 = np.float32


def make_case(kind, n_kp, n_points, n_kf, seed):
    """n_kf keyframes around one list of n_points points.  Returns the point arrays, the targets in the layout of
    tests/fuse_sim3_keyframes_scene.py, and `inside`, the achieved fraction of (keyframe, point) pairs inside the image."""
    rng = np.random.default_rng(seed)
    kb8 = kind == "kb8"
    W, H = (512.0, 512.0) if kb8 else (752.0, 480.0)
    cam = FS.KB8 if kb8 else FS.PIN
    az, el = rng.uniform(-math.pi, math.pi, n_points), rng.uniform(-math.radians(30), math.radians(30), n_points)
    r = np.exp(rng.uniform(math.log(2.0), math.log(10.0), n_points))
    X = np.stack([r * np.cos(el) * np.sin(az), r * np.sin(el), r * np.cos(el) * np.cos(az)], 1)
    sf = FS.scale_factors(8, 1.2)
    dist0 = np.linalg.norm(X, axis=1)
    max_dist = dist0 * sf[rng.integers(0, 8, n_points)]
    normal = X / dist0[:, None]                                    # the viewing direction from near the origin, where the keyframes stand
    normal[rng.random(n_points) < 0.1] *= -1.0
    mpdesc = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    pts = dict(nP=n_points, Xw=X.astype(f32), normal=normal.astype(f32), mpdesc=mpdesc, max_dist=max_dist.astype(f32),
               min_dist=(max_dist / sf[7]).astype(f32))
    targets, inside = [], []
    for _ in range(n_kf):
        R = FS._rot(float(rng.uniform(-math.pi, math.pi)), float(rng.uniform(-0.05, 0.05))).T
        t = -R @ rng.uniform(-0.3, 0.3, 3)
        Xc = X @ R.T + t
        front = Xc[:, 2] > 0.05
        proj = np.full((n_points, 2), -1e9)
        proj[front] = FS._project("kb8" if kb8 else "pin", cam, Xc[front])
        inside.append(float((front & (proj[:, 0] >= 0) & (proj[:, 0] < W) & (proj[:, 1] >= 0) & (proj[:, 1] < H)).mean()))
        dist = np.linalg.norm(X - (-R.T @ t), axis=1)
        lvl = np.clip(np.ceil(np.log(max_dist / dist) / math.log(1.2)), 0, 7).astype(int)
        seen = np.nonzero(front & (proj[:, 0] >= 10) & (proj[:, 0] < W - 10) & (proj[:, 1] >= 10) & (proj[:, 1] < H - 10))[0]
        seen = rng.permutation(seen)[:int(0.8 * n_kp)]
        k = np.zeros(n_kp, FS.KP_DTYPE)
        d = rng.integers(0, 256, (n_kp, 32), dtype=np.uint8)
        k["x"], k["y"] = rng.uniform(5, W - 5, n_kp), rng.uniform(5, H - 5, n_kp)
        k["octave"] = rng.integers(0, 8, n_kp)
        slot = rng.permutation(n_kp)[:len(seen)]
        k["x"][slot], k["y"][slot] = proj[seen, 0] + rng.uniform(-0.3, 0.3, len(seen)), proj[seen, 1] + rng.uniform(-0.3, 0.3, len(seen))
        k["octave"][slot] = np.maximum(lvl[seen] - (rng.random(len(seen)) < 0.4), 0)
        d[slot] = mpdesc[seen] ^ np.packbits(rng.random((len(seen), 256)) < 0.02, axis=1)
        k["size"], k["class_id"] = 31.0, -1
        Scw = np.eye(4)
        s = float(rng.uniform(0.9, 1.1))
        Scw[:3, :3], Scw[:3, 3] = s * R, s * t
        targets.append(dict(k=k, d=d, ur=None, bounds=(0.0, W, 0.0, H), sf=sf, log_sf=float(np.log(f32(1.2))), nlevels=8, Scw=Scw.astype(f32),
                            cam_type=1 if kb8 else 0, cam=cam))
    pts["valid"] = np.ascontiguousarray(rng.random((n_kf, n_points)) < 0.9, np.uint8)
    pts["targets"] = targets
    pts["inside"] = float(np.mean(inside))
    return pts


def routes_of(pkg, S, th):
    T, nP = len(S["targets"]), S["nP"]
    views = [SS.product_target(pkg, tg) for tg in S["targets"]]
    structs = [v.struct() for v in views]
    tab = (pkg.FuseSim3TargetStruct * T)(*structs)
    keep = (views, structs, tab)

    def one_call(m, bi, bd, nf):
        return m.L.orbm_fuse_sim3_keyframes(m.m, T, C.cast(tab, C.c_void_p), nP, P(S["valid"]), P(S["Xw"]), P(S["normal"]), P(S["mpdesc"]), P(S["max_dist"]),
                                            P(S["min_dist"]), C.c_float(th), P(bi), P(bd), P(nf))

    def loop(m, bi, bd, nf):
        tot = 0
        for t in range(T):
            g = structs[t]
            rc = m.L.orbm_fuse_sim3_cam(m.m, C.byref(g.kf), g.scale_factors, g.nlevels, g.log_scale_factor, nP, P(S["valid"][t]), P(S["Xw"]), P(S["normal"]),
                                        P(S["mpdesc"]), P(S["max_dist"]), P(S["min_dist"]), g.Scw, g.cam_type, g.cam_params, C.c_float(th), P(bi[t]), P(bd[t]))
            if rc < 0:
                return rc
            nf[t] = rc
            tot += rc
        return tot

    return one_call, loop, keep


def measure(name, desc, pkg, m, S, th, rounds, calls, warmup):
    T, nP = len(S["targets"]), S["nP"]
    one_call, loop, keep = routes_of(pkg, S, th)
    routes = (("one call (orbm_fuse_sim3_keyframes)", one_call), ("loop of T orbm_fuse_sim3_cam calls", loop))
    outs = [(np.full((T, nP), -2, np.int32), np.full((T, nP), -2, np.int32), np.zeros(T, np.int32)) for _ in routes]
    for (label, fn), o in zip(routes, outs):
        for _ in range(warmup):
            rc = fn(m, *o)
            if rc < 0:
                raise SystemExit("%s: %s rc=%d: %s" % (name, label, rc, m.L.orbm_last_error(m.m)))
    means = [[] for _ in routes]
    for _ in range(rounds):
        for r, ((label, fn), o) in enumerate(zip(routes, outs)):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn(m, *o)
            means[r].append((time.perf_counter() - t0) * 1e3 / calls)
    identical = all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))
    res = dict(case=name, T=T, nP=nP, fused=int(outs[0][2].sum()), valid_fraction=float(S["valid"].mean()), inside_fraction=S["inside"],
               identical=bool(identical), rounds=rounds, calls=calls)
    lines = ["%s: %s; %.1f %% of the (keyframe, point) pairs inside the image, %.0f %% valid, %d fused over all keyframes"
             % (name, desc, 100 * res["inside_fraction"], 100 * res["valid_fraction"], res["fused"])]
    for key, (label, _), v in zip(("one_call_ms", "loop_ms"), routes, means):
        res[key] = dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)
        lines.append("  %-38s median %.4f ms per call (range %.4f-%.4f, %d rounds x %d calls)" % (label + ":", res[key]["median"], min(v), max(v), rounds, calls))
    spread = res["loop_ms"]["max"] - res["loop_ms"]["min"]
    gain = res["loop_ms"]["median"] - res["one_call_ms"]["median"]
    res["gain"] = bool(res["one_call_ms"]["max"] < res["loop_ms"]["min"] and gain >= 3 * spread)
    lines.append("  loop / one call: %.2f x; every round of the one call below every round of the loop: %s; median gain %.4f ms against a loop spread of %.4f ms: %s"
                 % (res["loop_ms"]["median"] / res["one_call_ms"]["median"], "yes" if res["one_call_ms"]["max"] < res["loop_ms"]["min"] else "no", gain, spread,
                    "a gain by the rule" if res["gain"] else "NO gain by the rule"))
    lines.append("  rows of the two routes: %s" % ("identical" if identical else "DIFFERENT"))
    return res, lines


CASES = (("loop correction", "Pinhole, 1000 keypoints per keyframe, 4000 points, T = 40", ("pin", 1000, 4000, 40, 41)),
         ("merge", "KannalaBrandt8, 1500 keypoints per keyframe, 20000 points, T = 100", ("kb8", 1500, 20000, 100, 42)),
         ("small", "Pinhole, 1000 keypoints per keyframe, 1000 points, T = 10", ("pin", 1000, 1000, 10, 43)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--th", type=float, default=4.0)
    ap.add_argument("--only", default=None, help="one shape by name (for a device trace of that shape alone)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_sim3_keyframes_bench.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    m = pkg.ORBmatcher(0.8, True)
    results, lines = [], []
    for name, desc, args in CASES:
        if a.only and a.only != name:
            continue
        res, text = measure(name, desc, pkg, m, make_case(*args), a.th, a.rounds, a.calls, a.warmup)
        results.append(res)
        lines += text
    m.close()
    lines.append(json.dumps(dict(th=a.th, cases=results)))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(r["identical"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
