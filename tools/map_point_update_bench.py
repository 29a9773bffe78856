#!/usr/bin/env python3
"""MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth for all map points of one call (the loop of
LocalMapping.cc:1040-1053 and the pair behind CreateNewMapPoints, :890-897): the one-call entry orbm_update_map_points against the path it
replaces, on the same inputs and handle.  That path is, per map point, one orbm_distinctive_descriptors call with nmp = 1 (what
csrc/adapter/snippets/MapPoint_ComputeDistinctiveDescriptors_hip.cc does: one upload, one single-wavefront launch, one download, one
synchronisation) plus orbm_map_point_normal_depth on the host.

Two synthetic inputs, built without images (descriptors around a per-point base row, camera centres 1-6 m from the point, every entry's
keyframe good):
  keyframe update   1000 map points; entries per point 3 + Gamma(2, 2.2) rounded (median 6-7, most within 3-12), every twentieth point
                    instead uniform in 13-40 (the tail); 10 % of the entries are the second camera of the previous entry's keyframe
  new points        300 map points of 2 entries (what one CreateNewMapPoints creates)
Both routes are called through ctypes on arguments built beforehand, so the interpreter adds one foreign call per library call and
nothing else.  --rounds rounds, the two routes alternated inside a round, --calls calls each; wall clock per call (all points) as the
median and range of the rounds' means.  The outputs of both routes must be identical (best, and the bits of normal, min_dist, max_dist):
exit status 1 otherwise.  The result is stated by the project's rule: a gain counts when every round of the one call is below every
round of the loop AND the median gain is at least three times the loop's own spread.  Prints text lines and one JSON line and writes
them to --out.  Needs a GPU; there is no fallback.

--kernels CALLS instead launches, CALLS times each on the keyframe update, the one call and orbm_distinctive_descriptors over all groups
at once, and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`, which then times k_update_map_points against
k_distinctive on the same groups (the register-resident rows against the re-read ones).

    python tools/map_point_update_bench.py [--rounds 5] [--calls 20] [--out profiles/map_point_update_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o mpu --output-format csv -- python tools/map_point_update_bench.py --kernels 50
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEYS = ("start", "desc", "centre", "in_desc", "pos", "ref_centre", "ref_scale", "ref_max_scale")
SCALES = np.array([np.float32(1.2) ** k for k in range(8)], np.float32)


def make_case(sizes, rig_share, seed):
    rng = np.random.default_rng(seed)
    pts = []
    for n in sizes:
        pos = rng.uniform(-5, 5, 3).astype(np.float32)
        dirs = rng.normal(size=(n, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        centre = (pos.astype(np.float64) - dirs * rng.uniform(1, 6, (n, 1))).astype(np.float32)
        for e in range(1, n):
            if rng.random() < rig_share:
                centre[e] = centre[e - 1] + np.array([0.11, 0, 0], np.float32)
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        desc = base[None, :] ^ np.packbits(rng.random((n, 256)) < rng.uniform(0.01, 0.2, (n, 1)), axis=1)
        pts.append(dict(desc=desc.astype(np.uint8), centre=centre, in_desc=np.ones(n, np.uint8), pos=pos, ref_centre=centre[int(rng.integers(0, n))].copy(),
                        ref_scale=SCALES[int(rng.integers(0, 8))], ref_max_scale=SCALES[7]))
    return pts


def keyframe_sizes(n, seed):
    rng = np.random.default_rng(seed)
    sizes = np.clip(np.rint(3 + rng.gamma(2.0, 2.2, n)), 3, 40).astype(int)
    sizes[::20] = rng.integers(13, 41, len(sizes[::20]))
    return sizes


def routes_of(pkg, m, A):
    n = len(A["pos"])
    L = m.L
    u = pkg.MapPointUpdateStruct(n, *[pkg._p(A[k]) for k in KEYS])
    addr = lambda a, off: C.c_void_p(a.ctypes.data + off)
    starts = [(C.c_int32 * 2)(0, int(A["start"][p + 1] - A["start"][p])) for p in range(n)]

    def one_call(best, normal, mn, mx):
        return L.orbm_update_map_points(m.m, C.byref(u), pkg._p(best), pkg._p(normal), pkg._p(mn), pkg._p(mx))

    def loop_args(best, normal, mn, mx):
        a1, a2 = [], []
        for p in range(n):
            s0 = int(A["start"][p])
            a1.append((m.m, 1, C.cast(starts[p], C.c_void_p), addr(A["desc"], 32 * s0), addr(best, 4 * p)))
            a2.append((starts[p][1], addr(A["centre"], 12 * s0), addr(A["pos"], 12 * p), addr(A["ref_centre"], 12 * p), float(A["ref_scale"][p]),
                       float(A["ref_max_scale"][p]), addr(normal, 12 * p), addr(mn, 4 * p), addr(mx, 4 * p)))
        return a1, a2

    def loop(args):
        f1, f2 = L.orbm_distinctive_descriptors, L.orbm_map_point_normal_depth
        rc = 0
        for x, y in zip(*args):
            rc |= f1(*x) | f2(*y)
        return rc

    def all_groups(best):
        return L.orbm_distinctive_descriptors(m.m, n, pkg._p(A["start"]), pkg._p(A["desc"]), pkg._p(best))

    return one_call, loop_args, loop, all_groups, (u, starts)


def outputs(n):
    return np.full(n, -2, np.int32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)


def measure(name, desc, pkg, m, pts, rounds, calls, warmup):
    A = pkg.pack_map_points(pts)
    n = len(pts)
    one_call, loop_args, loop, _, keep = routes_of(pkg, m, A)
    o1, o2 = outputs(n), outputs(n)
    args = loop_args(*o2)
    routes = (("one call (orbm_update_map_points)", lambda: one_call(*o1)), ("loop of nmp = 1 calls + host normal", lambda: loop(args)))
    for label, fn in routes:
        for _ in range(warmup):
            rc = fn()
            if rc < 0:
                raise SystemExit("%s: %s rc=%d: %s" % (name, label, rc, m.L.orbm_last_error(m.m)))
    means = [[] for _ in routes]
    for _ in range(rounds):
        for r, (label, fn) in enumerate(routes):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            means[r].append((time.perf_counter() - t0) * 1e3 / calls)
    identical = np.array_equal(o1[0], o2[0]) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(o1[1:], o2[1:]))
    sizes = np.diff(A["start"])
    res = dict(case=name, points=n, entries=int(A["start"][-1]), median_entries=float(np.median(sizes)), max_entries=int(sizes.max()), identical=bool(identical),
               rounds=rounds, calls=calls)
    lines = ["%s: %s; %d entries over %d points (median %.0f, largest %d)" % (name, desc, res["entries"], n, res["median_entries"], res["max_entries"])]
    for key, (label, _), v in zip(("one_call_ms", "loop_ms"), routes, means):
        res[key] = dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)
        lines.append("  %-38s median %.4f ms per call (range %.4f-%.4f, %d rounds x %d calls)" % (label + ":", res[key]["median"], min(v), max(v), rounds, calls))
    spread = res["loop_ms"]["max"] - res["loop_ms"]["min"]
    gain = res["loop_ms"]["median"] - res["one_call_ms"]["median"]
    res["gain"] = bool(res["one_call_ms"]["max"] < res["loop_ms"]["min"] and gain >= 3 * spread)
    lines.append("  loop / one call: %.2f x; every round of the one call below every round of the loop: %s; median gain %.4f ms against a loop spread of %.4f ms: %s"
                 % (res["loop_ms"]["median"] / res["one_call_ms"]["median"], "yes" if res["one_call_ms"]["max"] < res["loop_ms"]["min"] else "no", gain, spread,
                    "a gain by the rule" if res["gain"] else "NO gain by the rule"))
    lines.append("  outputs of the two routes: %s" % ("identical" if identical else "DIFFERENT"))
    return res, lines


def cases():
    return (("keyframe update", "1000 map points, 3 + Gamma(2, 2.2) entries, every twentieth point 13-40, 10 % second-camera entries", make_case(keyframe_sizes(1000, 7), 0.1, 8)),
            ("new points", "300 map points of 2 entries", make_case([2] * 300, 0.0, 9)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0, help="only launch both kernels this many times on the keyframe update (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_point_update_bench.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    m = pkg.ORBmatcher(0.8, True)
    if a.kernels:
        A = pkg.pack_map_points(cases()[0][2])
        one_call, _, _, all_groups, keep = routes_of(pkg, m, A)
        o = outputs(len(A["pos"]))
        b2 = np.full(len(A["pos"]), -2, np.int32)
        for _ in range(a.kernels):
            if one_call(*o) < 0 or all_groups(b2) < 0:
                raise SystemExit("kernel run failed: %s" % m.L.orbm_last_error(m.m))
        m.close()
        print("best of both kernels: %s" % ("identical" if np.array_equal(o[0], b2) else "DIFFERENT"))
        return 0 if np.array_equal(o[0], b2) else 1
    results, lines = [], []
    for name, desc, pts in cases():
        res, text = measure(name, desc, pkg, m, pts, a.rounds, a.calls, a.warmup)
        results.append(res)
        lines += text
    m.close()
    lines.append(json.dumps(dict(cases=results)))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(r["identical"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
