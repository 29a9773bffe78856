#!/usr/bin/env python3
"""LocalMapping::CreateNewMapPoints in one call (orbm_create_new_map_points / orbm_create_new_map_points_kb8) on the inputs of
tools/triangulation_batch_bench.py: a monocular Pinhole keyframe of --points keypoints in --nodes vocabulary nodes against K = 20
neighbours, and a KannalaBrandt8 rig keyframe against K = 10 rigs.  Three times per keyframe, wall clock, ctypes on prebuilt structures:

  (a) the one-call entry: searches, the body of the loop on the device, the list of new points downloaded (no status, no rows);
  (b) the search-only entry orbm_search_for_triangulation(_kb8)_neighbours alone - of THIS build and, with --parent-lib, of a library
      built from the parent commit, loaded beside it: (a) - (b) is what the geometry costs on the device, and the two (b) show whether
      the search-only path moved;
  (c) for information only: (b) of this build plus a host loop over the downloaded rows through orbm_new_point_geometry (numpy gathers
      of the matched keypoints, one call per neighbour, the first-accepted rule in Python).  This is new code and no yardstick: it
      stands in for the reference's cv::Mat body, which cannot be built here.

--rounds rounds, the routes alternated inside a round, --calls calls each; median and range of the rounds' means.  The list of (a) must
equal the list of (c): exit status 1 otherwise.  Prints text lines and one JSON line and writes them to --out.  Needs a GPU.

    python tools/new_points_bench.py [--parent-lib PATH] [--points 1000] [--nodes 100] [--rounds 5] [--calls 40] [--out profiles/new_points_bench.txt]
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
SF1 = 1.2


class ParentLib:
    """The three symbols of another build that route (b) needs."""

    def __init__(self, path):
        vp, i32 = C.c_void_p, C.c_int
        self.L = C.CDLL(path)
        self.L.orbm_create.restype = vp
        self.L.orbm_create.argtypes = [i32]
        self.L.orbm_destroy.argtypes = [vp]
        self.L.orbm_search_for_triangulation_neighbours.argtypes = [vp, vp, i32] + [vp] * 9 + [i32, i32, vp, vp]
        self.L.orbm_search_for_triangulation_kb8_neighbours.argtypes = [vp, vp, i32, i32] + [vp] * 7 + [i32, i32, vp, vp]
        self.m = self.L.orbm_create(0)
        if not self.m:
            raise SystemExit("orbm_create of %s failed" % path)

    def close(self):
        self.L.orbm_destroy(self.m)


def host_list(pkg, K, n1, rows, pairs_of, c1, c2):
    """Route (c)'s tail: the body per neighbour on the host, the first accepted neighbour per idx1."""
    taken = np.zeros(n1, bool)
    out = []
    for j in range(K):
        i1 = np.nonzero(rows[j] >= 0)[0]
        if not len(i1):
            continue
        o1, o2 = pairs_of(j, i1, rows[j][i1])
        st, X = pkg.new_point_geometry(c1, c2[j], o1, o2, SF1)
        ok = (st == pkg.NP_ACCEPTED) & ~taken[i1]
        taken[i1[ok]] = True
        out += [(j, int(a), int(b), X[k].tobytes()) for k, (a, b) in enumerate(zip(i1, rows[j][i1])) if ok[k]]
    return out


def pinhole_case(pkg, points, nodes, K):
    import new_points_scene as PS
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
    c1 = PS.camera(S["R1w"], S["t1w"], 0, S["cam"], S["sf1"], S["sigma2_1"], intr=S["cam"])
    c2 = [PS.camera(nb["R2w"], nb["t2w"], 0, S["cam"], nb["sf"], nb["sigma2"], intr=S["cam"]) for nb in S["nbs"]]
    G1, Gs = PS.geometry_view(pkg, c1), [PS.geometry_view(pkg, c) for c in c2]
    s1, g1 = K1.struct(), G1.struct()
    tab = (pkg.KeyFrameStruct * K)(*[v.struct() for v in views])
    gtab = (pkg.KeyFrameGeometryStruct * K)(*[g.struct() for g in Gs])
    R2w, t2w = np.ascontiguousarray([nb["R2w"] for nb in S["nbs"]], np.float32), np.ascontiguousarray([nb["t2w"] for nb in S["nbs"]], np.float32)
    cam2 = np.ascontiguousarray(np.tile(S["cam"], (K, 1)), np.float32)
    n1 = K1.N
    keep = (S, K1, views, tab, gtab, G1, Gs, R2w, t2w, cam2)
    common = (P(S["R1w"]), P(S["t1w"]), P(S["Cw1"]), P(S["cam"]), P(R2w), P(t2w), P(cam2), None)

    def create(m, pts):
        return m.L.orbm_create_new_map_points(m.m, C.byref(s1), C.byref(g1), SF1, K, C.cast(tab, C.c_void_p), C.cast(gtab, C.c_void_p), *common, 0, 0, 0.0,
                                              P(pts), n1, None, None, None)

    def search(m, out, nm):
        return m.L.orbm_search_for_triangulation_neighbours(m.m, C.byref(s1), K, C.cast(tab, C.c_void_p), *common, 0, 0, P(out), P(nm))

    none = np.zeros(0, np.float32)
    pairs_of = lambda j, i1, i2: (PS.observations(S["k1"], S["ur1"], none, S["k1"], i1), PS.observations(S["nbs"][j]["k"], S["nbs"][j]["ur"], none, S["nbs"][j]["k"], i2))
    desc = "monocular Pinhole, %d keypoints in KF1, K = %d neighbours of %d-%d keypoints, %d vocabulary nodes" % (
        n1, K, min(v.N for v in views), max(v.N for v in views), len(K1.node_id))
    return desc, n1, create, search, (pairs_of, c1, c2), keep


def kb8_case(pkg, points, nodes, K):
    import new_points_scene as PS
    import triangulation_kb8_scene as SC
    rng = np.random.default_rng(4)
    centres = [(float(rng.uniform(-0.4, 0.4)), float(rng.uniform(-0.05, 0.05)), float(rng.uniform(-0.3, 0.1))) for _ in range(K)]
    Ss = [SC.make_scene(points, True, c, max_decoys=1) for c in centres]
    for S in Ss[1:]:
        assert np.array_equal(S["k1"], Ss[0]["k1"]) and np.array_equal(S["d1"], Ss[0]["d1"]) and S["n_left1"] == Ss[0]["n_left1"]
    K1 = SC.product_views(pkg, Ss[0], nodes)[0]
    views = [SC.product_views(pkg, S, nodes)[1] for S in Ss]
    c1, c2 = PS.make_kb8(Ss, centres)
    G1, Gs = PS.geometry_view(pkg, c1), [PS.geometry_view(pkg, c) for c in c2]
    s1, g1 = K1.struct(), G1.struct()
    tab = (pkg.KeyFrameStruct * K)(*[v.struct() for v in views])
    gtab = (pkg.KeyFrameGeometryStruct * K)(*[g.struct() for g in Gs])
    nl1 = int(Ss[0]["n_left1"])
    nl2 = np.array([S["n_left2"] for S in Ss], np.int32)
    ep = np.ascontiguousarray([S["ep"] for S in Ss], np.float32)
    cams1 = np.ascontiguousarray(Ss[0]["cams1"], np.float32)
    cams2 = np.ascontiguousarray([S["cams2"] for S in Ss], np.float32)
    T12 = np.ascontiguousarray([S["T12"] for S in Ss], np.float32)
    n1 = K1.N
    keep = (Ss, K1, views, tab, gtab, G1, Gs)
    common = (P(nl2), P(ep), P(cams1), P(cams2), P(T12), None)

    def create(m, pts):
        return m.L.orbm_create_new_map_points_kb8(m.m, C.byref(s1), C.byref(g1), SF1, nl1, K, C.cast(tab, C.c_void_p), C.cast(gtab, C.c_void_p), *common, 0, 0, 0.0,
                                                  P(pts), n1, None, None, None)

    def search(m, out, nm):
        return m.L.orbm_search_for_triangulation_kb8_neighbours(m.m, C.byref(s1), nl1, K, C.cast(tab, C.c_void_p), *common, 0, 0, P(out), P(nm))

    pairs_of = lambda j, i1, i2: (PS.observations(Ss[0]["k1"], None, None, None, i1, nl1), PS.observations(Ss[j]["k2"], None, None, None, i2, int(nl2[j])))
    desc = "KannalaBrandt8 rigs, %d + %d keypoints (left + right) in KF1, K = %d neighbours of %d-%d keypoints, %d vocabulary nodes" % (
        nl1, n1 - nl1, K, min(v.N for v in views), max(v.N for v in views), len(K1.node_id))
    return desc, n1, create, search, (pairs_of, c1, c2), keep


def measure(pkg, name, case, m, parent, K, rounds, calls, warmup):
    desc, n1, create, search, host, keep = case
    pts = np.zeros(n1, pkg.NEW_POINT_DTYPE)
    rows, nm = np.full((K, n1), -2, np.int32), np.zeros(K, np.int32)
    rows_p, nm_p = np.full((K, n1), -2, np.int32), np.zeros(K, np.int32)
    count = [0]

    def route_a():
        count[0] = create(m, pts)
        return count[0]

    def route_c():
        rc = search(m, rows, nm)
        route_c.list = host_list(pkg, K, n1, rows, *host)
        return rc

    routes = [("a", "(a) one call: searches + body + list", route_a), ("b", "(b) search only, this build", lambda: search(m, rows, nm))]
    if parent is not None:
        routes.append(("b_parent", "(b) search only, parent build", lambda: search(parent, rows_p, nm_p)))
    routes.append(("c", "(c) search + host loop (stand-in)", route_c))
    for key, label, fn in routes:
        for _ in range(warmup):
            rc = fn()
            if rc < 0:
                raise SystemExit("%s: %s rc=%d: %s" % (name, label, rc, m.L.orbm_last_error(m.m)))
    means = {key: [] for key, _, _ in routes}
    for _ in range(rounds):
        for key, _, fn in routes:
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            means[key].append((time.perf_counter() - t0) * 1e3 / calls)
    dev = [(int(p["neighbour"]), int(p["idx1"]), int(p["idx2"]), p["x3D"].tobytes()) for p in pts[:count[0]]]
    identical = dev == route_c.list and (parent is None or (np.array_equal(rows, rows_p) and np.array_equal(nm, nm_p)))
    res = dict(case=name, K=K, n1=n1, matches=int(nm.sum()), new_points=count[0], identical=bool(identical), rounds=rounds, calls=calls)
    lines = ["%s: %s; %d matches over all neighbours, %d new points" % (name, desc, res["matches"], count[0])]
    for key, label, _ in routes:
        v = means[key]
        res[key + "_ms"] = dict(median=statistics.median(v), min=min(v), max=max(v))
        lines.append("  %-40s median %.4f ms per keyframe (range %.4f-%.4f, %d rounds x %d calls)" % (label + ":", res[key + "_ms"]["median"], min(v), max(v), rounds, calls))
    med = lambda k: res[k + "_ms"]["median"]
    lines.append("  (a) - (b) = %.4f ms: the body and the list on the device; (c) - (b) = %.4f ms: the stand-in's host loop" % (med("a") - med("b"), med("c") - med("b")))
    if parent is not None:
        spread = res["b_parent_ms"]["max"] - res["b_parent_ms"]["min"]
        res["search_only_no_slower"] = bool(med("b") - med("b_parent") <= spread)
        lines.append("  search only, this build - parent build = %+.4f ms; the parent's own range is %.4f ms: %s" % (
            med("b") - med("b_parent"), spread, "no slower" if res["search_only_no_slower"] else "SLOWER by more than the parent's range"))
    lines.append("  list of (a) against list of (c)%s: %s" % ("" if parent is None else ", rows of the two builds", "identical" if identical else "DIFFERENT"))
    return res, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liborbhip.so built from the parent commit")
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "new_points_bench.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    m = pkg.ORBmatcher(0.6, False)
    parent = ParentLib(a.parent_lib) if a.parent_lib else None
    results, lines = [], []
    for name, make, K in (("pinhole", pinhole_case, 20), ("kb8_rig", kb8_case, 10)):
        res, text = measure(pkg, name, make(pkg, a.points, a.nodes, K), m, parent, K, a.rounds, a.calls, a.warmup)
        results.append(res)
        lines += text
    m.close()
    if parent is not None:
        parent.close()
    lines.append(json.dumps(dict(points=a.points, nodes=a.nodes, parent_lib=bool(a.parent_lib), cases=results)))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(r["identical"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
