#!/usr/bin/env python3
"""SearchForTriangulation of one keyframe against all its neighbours (the loop of LocalMapping::CreateNewMapPoints,
LocalMapping.cc:475-583): the one-call entries orbm_search_for_triangulation_neighbours / orbm_search_for_triangulation_kb8_neighbours
against the loop of K per-pair calls they replace, on the same inputs.

Two synthetic cases, built without images: a monocular Pinhole keyframe of --points keypoints in --nodes vocabulary nodes against
K = 20 neighbours (tests/triangulation_neighbours_scene.py), and a KannalaBrandt8 rig keyframe against K = 10 rigs
(tests/triangulation_kb8_scene.py, one scene per neighbour pose, KF1 shared).  Both routes are called through ctypes on structures
built beforehand, so the interpreter adds one foreign call per library call and nothing else.  The one-call form is measured in both
item layouts (ORBM_TRI_LAYOUT, read when a handle is created: 0 neighbour-major, the default, 1 KF1-keypoint-major).  --rounds rounds, the three
routes alternated inside a round, --calls calls each; median and range of the rounds' means.  The rows of all three routes must be
identical: exit status 1 otherwise.  Prints text lines and one JSON line and writes them to --out.  Needs a GPU; there is no fallback.

    python tools/triangulation_batch_bench.py [--points 1000] [--nodes 100] [--rounds 5] [--calls 40] [--out profiles/triangulation_batch_bench.txt]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

P = lambda a: a.ctypes.data_as(C.c_void_p)


def handle(pkg, layout):
    os.environ["ORBM_TRI_LAYOUT"] = str(layout)
    try:
        return pkg.ORBmatcher(0.6, False)
    finally:
        del os.environ["ORBM_TRI_LAYOUT"]


def pinhole_case(pkg, points, nodes, K):
    import triangulation_neighbours_scene as NS
    rng = np.random.default_rng(3)
    poses = tuple((float(rng.uniform(-0.03, 0.03)), float(rng.uniform(-0.02, 0.02)),
                   (float(rng.uniform(-0.4, 0.4)), float(rng.uniform(-0.1, 0.1)), float(rng.uniform(-0.1, 0.3)))) for _ in range(K))
    S = NS.make_scene(tuple(("real", points, 8, False) for _ in range(K)), n1=points, seed=21, nodes=nodes, poses=poses)
    S["ur1"][:] = -1                                            # monocular
    for nb in S["nbs"]:
        nb["ur"][:] = -1
    K1 = NS.product_kf1(pkg, S)
    views = [NS.product_nb(pkg, nb) for nb in S["nbs"]]
    s1 = K1.struct()
    tab = (pkg.KeyFrameStruct * K)(*[v.struct() for v in views])
    R2w, t2w = np.ascontiguousarray([nb["R2w"] for nb in S["nbs"]], np.float32), np.ascontiguousarray([nb["t2w"] for nb in S["nbs"]], np.float32)
    cam2 = np.ascontiguousarray(np.tile(S["cam"], (K, 1)), np.float32)
    n1 = K1.N
    keep = (S, K1, views, tab, R2w, t2w, cam2)

    def one_call(m, out, nm):
        return m.L.orbm_search_for_triangulation_neighbours(m.m, C.byref(s1), K, C.cast(tab, C.c_void_p), P(S["R1w"]), P(S["t1w"]), P(S["Cw1"]), P(S["cam"]),
                                                            P(R2w), P(t2w), P(cam2), None, 0, 0, P(out), P(nm))

    def loop(m, out, nm):
        tot = 0
        for j in range(K):
            rc = m.L.orbm_search_for_triangulation(m.m, C.byref(s1), C.byref(tab[j]), P(S["R1w"]), P(S["t1w"]), P(R2w[j]), P(t2w[j]), P(S["Cw1"]), P(S["cam"]),
                                                   P(cam2[j]), 0, 0, 0, P(out[j]))
            if rc < 0:
                return rc
            nm[j] = rc
            tot += rc
        return tot

    desc = "monocular Pinhole, %d keypoints in KF1, K = %d neighbours of %d-%d keypoints, %d vocabulary nodes" % (
        n1, K, min(v.N for v in views), max(v.N for v in views), len(K1.node_id))
    return desc, n1, one_call, loop, keep


def kb8_case(pkg, points, nodes, K):
    import triangulation_kb8_scene as SC
    rng = np.random.default_rng(4)
    centres = [(float(rng.uniform(-0.4, 0.4)), float(rng.uniform(-0.05, 0.05)), float(rng.uniform(-0.3, 0.1))) for _ in range(K)]
    Ss = [SC.make_scene(points, True, c, max_decoys=1) for c in centres]
    for S in Ss[1:]:
        assert np.array_equal(S["k1"], Ss[0]["k1"]) and np.array_equal(S["d1"], Ss[0]["d1"]) and S["n_left1"] == Ss[0]["n_left1"]
    K1 = SC.product_views(pkg, Ss[0], nodes)[0]
    views = [SC.product_views(pkg, S, nodes)[1] for S in Ss]
    s1 = K1.struct()
    tab = (pkg.KeyFrameStruct * K)(*[v.struct() for v in views])
    nl1 = int(Ss[0]["n_left1"])
    nl2 = np.array([S["n_left2"] for S in Ss], np.int32)
    ep = np.ascontiguousarray([S["ep"] for S in Ss], np.float32)
    cams1 = np.ascontiguousarray(Ss[0]["cams1"], np.float32)
    cams2 = np.ascontiguousarray([S["cams2"] for S in Ss], np.float32)
    T12 = np.ascontiguousarray([S["T12"] for S in Ss], np.float32)
    n1 = K1.N
    keep = (Ss, K1, views, tab)

    def one_call(m, out, nm):
        return m.L.orbm_search_for_triangulation_kb8_neighbours(m.m, C.byref(s1), nl1, K, C.cast(tab, C.c_void_p), P(nl2), P(ep), P(cams1), P(cams2), P(T12), None,
                                                                0, 0, P(out), P(nm))

    def loop(m, out, nm):
        tot = 0
        for j in range(K):
            rc = m.L.orbm_search_for_triangulation_kb8(m.m, C.byref(s1), nl1, C.byref(tab[j]), int(nl2[j]), C.c_float(ep[j, 0]), C.c_float(ep[j, 1]), P(cams1),
                                                       P(cams2[j]), P(T12[j]), 0, 0, 0, P(out[j]))
            if rc < 0:
                return rc
            nm[j] = rc
            tot += rc
        return tot

    desc = "KannalaBrandt8 rigs, %d + %d keypoints (left + right) in KF1, K = %d neighbours of %d-%d keypoints, %d vocabulary nodes" % (
        nl1, n1 - nl1, K, min(v.N for v in views), max(v.N for v in views), len(K1.node_id))
    return desc, n1, one_call, loop, keep


def measure(name, case, ms, K, rounds, calls, warmup):
    desc, n1, one_call, loop, keep = case
    routes = (("one call, neighbour-major items", one_call, ms[0]), ("one call, KF1-keypoint-major items", one_call, ms[1]), ("loop of K per-pair calls", loop, ms[0]))
    outs = [np.full((K, n1), -2, np.int32) for _ in routes]
    nms = [np.zeros(K, np.int32) for _ in routes]
    for (label, fn, m), out, nm in zip(routes, outs, nms):
        for _ in range(warmup):
            rc = fn(m, out, nm)
            if rc < 0:
                raise SystemExit("%s: %s rc=%d: %s" % (name, label, rc, m.L.orbm_last_error(m.m)))
    means = [[] for _ in routes]
    for _ in range(rounds):
        for r, ((label, fn, m), out, nm) in enumerate(zip(routes, outs, nms)):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn(m, out, nm)
            means[r].append((time.perf_counter() - t0) * 1e3 / calls)
    identical = all(np.array_equal(outs[0], o) and np.array_equal(nms[0], n) for o, n in zip(outs[1:], nms[1:]))
    res = dict(case=name, K=K, n1=n1, matches=int(nms[0].sum()), identical=bool(identical), rounds=rounds, calls=calls)
    lines = ["%s: %s; %d matches over all neighbours" % (name, desc, res["matches"])]
    for key, (label, _, _), v in zip(("batch_ms", "batch_keypoint_major_ms", "loop_ms"), routes, means):
        res[key] = dict(median=statistics.median(v), min=min(v), max=max(v))
        lines.append("  %-36s median %.4f ms per keyframe (range %.4f-%.4f, %d rounds x %d calls)" % (label + ":", res[key]["median"], min(v), max(v), rounds, calls))
    best = min(res["batch_ms"]["median"], res["batch_keypoint_major_ms"]["median"])
    loop_range = res["loop_ms"]["max"] - res["loop_ms"]["min"]
    res["faster_than_loop"] = bool(res["loop_ms"]["median"] - res["batch_ms"]["median"] > loop_range)
    lines.append("  loop / one call (neighbour-major, the default): %.2f x; the loop's own range is %.4f ms, the one call is %.4f ms below its median: %s; faster layout: %s"
                 % (res["loop_ms"]["median"] / res["batch_ms"]["median"], loop_range, res["loop_ms"]["median"] - res["batch_ms"]["median"],
                    "faster" if res["faster_than_loop"] else "NOT faster by more than the range",
                    "neighbour-major" if best == res["batch_ms"]["median"] else "KF1-keypoint-major"))
    lines.append("  rows of the three routes: %s" % ("identical" if identical else "DIFFERENT"))
    return res, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulation_batch_bench.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    ms = [handle(pkg, 0), handle(pkg, 1)]
    results, lines = [], []
    for name, make, K in (("pinhole", pinhole_case, 20), ("kb8_rig", kb8_case, 10)):
        res, text = measure(name, make(pkg, a.points, a.nodes, K), ms, K, a.rounds, a.calls, a.warmup)
        results.append(res)
        lines += text
    for m in ms:
        m.close()
    lines.append(json.dumps(dict(points=a.points, nodes=a.nodes, cases=results)))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(r["identical"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
