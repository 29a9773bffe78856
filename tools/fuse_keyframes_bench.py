#!/usr/bin/env python3
"""ORBmatcher::Fuse of one point list into all target keyframes (the loops of LocalMapping::SearchInNeighbors, LocalMapping.cc:989-1000
and :1033-1035): the one-call entry orbm_fuse_keyframes against the loop of T orbm_fuse calls it replaces, on the same inputs.

Three synthetic shapes, built without images (points at 2-10 m, keypoints at their projections, descriptors with a few flipped bits,
10 % flipped normals, about 60 % of the points valid per target):
  forward   monocular Pinhole, 1000 keypoints per keyframe, 1000 points, T = 40 targets
  rigs      KannalaBrandt8 rigs, 1500 keypoints per image, 1000 points, T = 20 (10 rigs x left, right)
  reverse   one Pinhole keyframe of 1000 keypoints, 20 000 points, T = 1
Both routes are called through ctypes on structures built beforehand, so the interpreter adds one foreign call per library call and
nothing else.  --rounds rounds, the two routes alternated inside a round, --calls calls each; wall clock per keyframe (per call of
SearchInNeighbors' loop) as the median and range of the rounds' means.  The rows of both routes must be identical: exit status 1
otherwise.  The result is stated by the project's rule: a gain counts when every round of the one call is below every round of the
loop AND the median gain is at least three times the loop's own spread.  Prints text lines and one JSON line and writes them to --out.
Needs a GPU; there is no fallback.

    python tools/fuse_keyframes_bench.py [--rounds 5] [--calls 20] [--out profiles/fuse_keyframes_bench.txt]
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

P = lambda a: a.ctypes.data_as(C.c_void_p)
f32 = np.float32


def make_case(kind, n_kp, n_points, n_kf, seed):
    """n_kf keyframes (rigs: two targets each) around one list of n_points points.  Returns the point arrays and a list of target dicts in
    the layout of tests/fuse_keyframes_scene.py."""
    rng = np.random.default_rng(seed)
    rig = kind == "kb8"
    W, H = (512.0, 512.0) if rig else (752.0, 480.0)
    uv = np.stack([rng.uniform(20, 752 - 20, n_points), rng.uniform(20, 480 - 20, n_points)], 1)
    z = np.exp(rng.uniform(math.log(2.0), math.log(10.0), n_points))
    X = np.stack([(uv[:, 0] - FS.PIN[2]) / FS.PIN[0] * z, (uv[:, 1] - FS.PIN[3]) / FS.PIN[1] * z, z], 1)
    sf = FS.scale_factors(8, 1.2)
    dist0 = np.linalg.norm(X, axis=1)
    max_dist = dist0 * sf[rng.integers(0, 8, n_points)]
    normal = X / dist0[:, None]
    normal[rng.random(n_points) < 0.1] *= -1.0
    mpdesc = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    pts = dict(nP=n_points, Xw=X.astype(f32), normal=normal.astype(f32), mpdesc=mpdesc, max_dist=max_dist.astype(f32),
               min_dist=(max_dist / sf[7]).astype(f32))
    targets, valid = [], []
    for _ in range(n_kf):
        R = FS._rot(float(rng.uniform(-0.03, 0.03)), float(rng.uniform(-0.02, 0.02))).T
        t = -R @ rng.uniform(-0.3, 0.3, 3)
        v = (rng.random(n_points) < 0.6).astype(np.uint8)
        for right in ((False, True) if rig else (False,)):
            if right:
                Rrl, trl = FS._rot(FS.TRL[0], FS.TRL[1]), np.array(FS.TRL[2], np.float64)
                Rt, tt = Rrl @ R, Rrl @ t + trl
            else:
                Rt, tt = R, t
            cam = (FS.KB8_R if right else FS.KB8) if rig else FS.PIN
            Xc = X @ Rt.T + tt
            proj = FS._project("kb8" if rig else "pin", cam, Xc)
            dist = np.linalg.norm(X - (-Rt.T @ tt), axis=1)
            lvl = np.clip(np.ceil(np.log(max_dist / dist) / math.log(1.2)), 0, 7).astype(int)
            seen = np.nonzero((Xc[:, 2] > 0.5) & (proj[:, 0] >= 10) & (proj[:, 0] < W - 10) & (proj[:, 1] >= 10) & (proj[:, 1] < H - 10))[0]
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
            Tcw = np.eye(4)
            Tcw[:3, :3], Tcw[:3, 3] = Rt, tt
            Tcw = Tcw.astype(f32)
            Ow = (-Tcw[:3, :3].T.astype(np.float64) @ Tcw[:3, 3].astype(np.float64)).astype(f32)
            targets.append(dict(k=k, d=d, ur=None, bounds=(0.0, W, 0.0, H), sf=sf, inv_sigma2=(f32(1) / (sf * sf)).astype(f32), log_sf=float(np.log(f32(1.2))),
                                nlevels=8, Tcw=Tcw, Ow=Ow, cam_type=1 if rig else 0, cam=cam, bf=0.0))
            valid.append(v)                                       # IsInKeyFrame is per keyframe: both cameras of a rig share the row
    pts["valid"] = np.ascontiguousarray(valid, np.uint8)
    pts["targets"] = targets
    return pts


def routes_of(pkg, S, th):
    T, nP = len(S["targets"]), S["nP"]
    views = [FS.product_target(pkg, tg) for tg in S["targets"]]
    structs = [v.struct() for v in views]
    tab = (pkg.FuseTargetStruct * T)(*structs)
    keep = (views, structs, tab)

    def one_call(m, bi, bd, nf):
        return m.L.orbm_fuse_keyframes(m.m, T, C.cast(tab, C.c_void_p), nP, P(S["valid"]), P(S["Xw"]), P(S["normal"]), P(S["mpdesc"]), P(S["max_dist"]),
                                       P(S["min_dist"]), C.c_float(th), P(bi), P(bd), P(nf))

    def loop(m, bi, bd, nf):
        tot = 0
        for t in range(T):
            g = structs[t]
            rc = m.L.orbm_fuse(m.m, C.byref(g.kf), g.scale_factors, g.inv_level_sigma2, g.nlevels, g.log_scale_factor, nP, P(S["valid"][t]), P(S["Xw"]),
                               P(S["normal"]), P(S["mpdesc"]), P(S["max_dist"]), P(S["min_dist"]), g.Tcw, g.Ow, g.cam_type, g.cam_params, g.bf, C.c_float(th),
                               P(bi[t]), P(bd[t]))
            if rc < 0:
                return rc
            nf[t] = rc
            tot += rc
        return tot

    return one_call, loop, keep


def measure(name, desc, pkg, m, S, th, rounds, calls, warmup):
    T, nP = len(S["targets"]), S["nP"]
    one_call, loop, keep = routes_of(pkg, S, th)
    routes = (("one call (orbm_fuse_keyframes)", one_call), ("loop of T orbm_fuse calls", loop))
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
    res = dict(case=name, T=T, nP=nP, fused=int(outs[0][2].sum()), valid_fraction=float(S["valid"].mean()), identical=bool(identical), rounds=rounds, calls=calls)
    lines = ["%s: %s; %d fused over all targets, %.0f %% of the (target, point) pairs valid" % (name, desc, res["fused"], 100 * res["valid_fraction"])]
    for key, (label, _), v in zip(("one_call_ms", "loop_ms"), routes, means):
        res[key] = dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)
        lines.append("  %-34s median %.4f ms per keyframe (range %.4f-%.4f, %d rounds x %d calls)" % (label + ":", res[key]["median"], min(v), max(v), rounds, calls))
    spread = res["loop_ms"]["max"] - res["loop_ms"]["min"]
    gain = res["loop_ms"]["median"] - res["one_call_ms"]["median"]
    res["gain"] = bool(res["one_call_ms"]["max"] < res["loop_ms"]["min"] and gain >= 3 * spread)
    lines.append("  loop / one call: %.2f x; every round of the one call below every round of the loop: %s; median gain %.4f ms against a loop spread of %.4f ms: %s"
                 % (res["loop_ms"]["median"] / res["one_call_ms"]["median"], "yes" if res["one_call_ms"]["max"] < res["loop_ms"]["min"] else "no", gain, spread,
                    "a gain by the rule" if res["gain"] else "NO gain by the rule"))
    lines.append("  rows of the two routes: %s" % ("identical" if identical else "DIFFERENT"))
    return res, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--th", type=float, default=3.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_keyframes_bench.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    m = pkg.ORBmatcher(0.6, True)
    cases = (("forward", "monocular Pinhole, 1000 keypoints per keyframe, 1000 points, T = 40", ("pin", 1000, 1000, 40, 31)),
             ("rigs", "KannalaBrandt8 rigs, 1500 keypoints per image, 1000 points, T = 20 (10 rigs x 2)", ("kb8", 1500, 1000, 10, 32)),
             ("reverse", "one Pinhole keyframe of 1000 keypoints, 20000 points, T = 1", ("pin", 1000, 20000, 1, 33)))
    results, lines = [], []
    for name, desc, args in cases:
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
