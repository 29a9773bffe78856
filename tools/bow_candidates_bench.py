#!/usr/bin/env python3
"""SearchByBoW of one frame or keyframe against all candidates (the loops of Tracking::Relocalization, Tracking.cc:3796-3816, and of
LoopClosing::DetectCommonRegionsFromBoW, LoopClosing.cc:724-739): the one-call entries orbm_search_by_bow_candidates /
orbm_search_by_bow_keyframes_candidates against the loop of K per-pair calls they replace, on the same inputs and the same handle.

Three synthetic shapes, built without images (tests/bow_candidates_scene.make_uniform_scene):
  relocalisation, monocular:    K = 10 keyframes of 1000 keypoints against a frame of 1000, nnratio 0.75, checkOri on;
  relocalisation, fisheye rig:  K = 10 keyframes of 3000 keypoints against a frame of 1500 + 1500, nnratio 0.75, checkOri on;
  loop closing:                 one keyframe of 1000 keypoints against K = 18 (3 candidates x 6) of 1000, nnratio 0.9, checkOri on;
each in --nodes vocabulary nodes (100 = DBoW2 levelsup 4 on the k = 10, L = 6 vocabulary).  Both routes are called through ctypes on
structures built beforehand, so the interpreter adds one foreign call per library call and nothing else.  Wall clock per call of the
one-call form resp. per loop of K calls; --rounds rounds, the routes alternated inside a round, --calls calls each; median and range
of the rounds' means.  The project's rule for a gain: every round of the one call lies below every round of the loop, and the median
gain is at least three times the loop's own range.  Rows and counts of both routes must be identical: exit status 1 otherwise.
Prints text lines and one JSON line and writes them to --out.  Needs a GPU; there is no fallback.

    python tools/bow_candidates_bench.py [--nodes 100] [--rounds 5] [--calls 20] [--out profiles/bow_candidates_bench.txt]
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
SHAPES = (("relocalisation, monocular", "frame", 1000, 0, 10, 0.75),
          ("relocalisation, fisheye rig frame", "frame", 1500, 1500, 10, 0.75),
          ("loop closing", "kf", 1000, 0, 18, 0.9))


def make_case(pkg, what, points, n_right, K, nodes):
    import bow_candidates_scene as BS
    S = BS.make_uniform_scene(points, K, nodes, n_right=n_right)
    fisheye = n_right > 0
    fixed = BS.product_fixed(pkg, S, what, fisheye)
    views = [BS.product_cand(pkg, S, j, what) for j in range(K)]
    fs = fixed.struct()
    tab = (pkg.KeyFrameStruct * K)(*[v.struct() for v in views])
    n_left = points if fisheye else -1
    keep = (S, fixed, views, tab)

    def one_call(m, nn, out, nm):
        if what == "kf":
            return m.L.orbm_search_by_bow_keyframes_candidates(m.m, C.byref(fs), K, C.cast(tab, C.c_void_p), None, C.c_float(nn), 1, P(out), P(nm))
        return m.L.orbm_search_by_bow_candidates(m.m, K, C.cast(tab, C.c_void_p), C.byref(fs), n_left, None, C.c_float(nn), 1, P(out), P(nm))

    def loop(m, nn, out, nm):
        tot = 0
        for j in range(K):
            if what == "kf":
                rc = m.L.orbm_search_by_bow_keyframes(m.m, C.byref(fs), C.byref(tab[j]), C.c_float(nn), 1, P(out[j]))
            elif fisheye:
                rc = m.L.orbm_search_by_bow_fisheye(m.m, C.byref(tab[j]), C.byref(fs), n_left, C.c_float(nn), 1, P(out[j]))
            else:
                rc = m.L.orbm_search_by_bow(m.m, C.byref(tab[j]), C.byref(fs), C.c_float(nn), 1, P(out[j]))
            if rc < 0:
                return rc
            nm[j] = rc
            tot += rc
        return tot

    items = sum(len(set(v.node_id.tolist()) & set(fixed.node_id.tolist())) for v in views)
    return fixed.N, one_call, loop, items, keep


def measure(name, case, m, K, nn, rounds, calls, warmup):
    n, one_call, loop, items, keep = case
    routes = (("one call", one_call), ("loop of K per-pair calls", loop))
    outs = [np.full((K, n), -2, np.int32) for _ in routes]
    nms = [np.zeros(K, np.int32) for _ in routes]
    for (label, fn), out, nm in zip(routes, outs, nms):
        for _ in range(warmup):
            rc = fn(m, nn, out, nm)
            if rc < 0:
                raise SystemExit("%s: %s rc=%d: %s" % (name, label, rc, m.L.orbm_last_error(m.m)))
    identical = bool(np.array_equal(outs[0], outs[1]) and np.array_equal(nms[0], nms[1]))   # asserted before timing
    if not identical:
        return dict(shape=name, identical=False), ["%s: rows of the two routes DIFFER" % name]
    means = [[] for _ in routes]
    for _ in range(rounds):
        for r, ((label, fn), out, nm) in enumerate(zip(routes, outs, nms)):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn(m, nn, out, nm)
            means[r].append((time.perf_counter() - t0) * 1e3 / calls)
    identical = bool(np.array_equal(outs[0], outs[1]) and np.array_equal(nms[0], nms[1]))
    res = dict(shape=name, K=K, n=n, items=items, matches=int(nms[0].sum()), identical=identical, rounds=rounds, calls=calls)
    lines = ["%s: K = %d, rows of %d, nnratio %.2f, checkOri on; %d (candidate, shared node) items, %d matches over all candidates" % (
        name, K, n, nn, items, res["matches"])]
    for key, (label, _), v in zip(("batch_ms", "loop_ms"), routes, means):
        res[key] = dict(median=statistics.median(v), min=min(v), max=max(v))
        lines.append("  %-26s median %.4f ms (range %.4f-%.4f, %d rounds x %d calls)" % (label + ":", res[key]["median"], min(v), max(v), rounds, calls))
    spread = res["loop_ms"]["max"] - res["loop_ms"]["min"]
    gain = res["loop_ms"]["median"] - res["batch_ms"]["median"]
    res["gain"] = bool(res["batch_ms"]["max"] < res["loop_ms"]["min"] and gain >= 3.0 * spread)
    lines.append("  loop / one call: %.2f x; every round of the one call below every round of the loop: %s; median gain %.4f ms against a loop "
                 "range of %.4f ms: %s" % (res["loop_ms"]["median"] / res["batch_ms"]["median"],
                                           "yes" if res["batch_ms"]["max"] < res["loop_ms"]["min"] else "NO", gain, spread,
                                           "a gain by the project's rule" if res["gain"] else "NOT a gain by the project's rule"))
    lines.append("  rows and counts of the two routes: %s" % ("identical" if identical else "DIFFERENT"))
    return res, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="0,1,2", help="indices into the three shapes (a kernel trace wants one at a time)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bow_candidates_bench.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    m = pkg.ORBmatcher(0.75, True)
    results, lines = [], []
    for s in [int(x) for x in a.shapes.split(",")]:
        name, what, points, n_right, K, nn = SHAPES[s]
        res, text = measure(name, make_case(pkg, what, points, n_right, K, a.nodes), m, K, nn, a.rounds, a.calls, a.warmup)
        results.append(res)
        lines += text
    m.close()
    lines.append(json.dumps(dict(nodes=a.nodes, shapes=results)))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(r["identical"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
