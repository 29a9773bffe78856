#!/usr/bin/env python3
"""TwoViewReconstruction::Reconstruct on the device (TwoViewReconstruction.cc:39-127): wall clock of the one-call form
orbm_two_view_reconstruct on synthetic two-view scenes.  There is nothing to compare with:
the parent has no such path and the reference's member is not built here, so NO GAIN IS CLAIMED; the host form
orbm_two_view_reconstruct_host is new code, used here only to check the outputs.

The scenes are INVENTED: a seeded cloud of points at depths 4 to 9 seen by two pinhole cameras (f = 500, 640 x 480) a rotation of 0.05 rad
and a translation of (0.4, 0.05, 0.02) apart, 0.3 px of Gaussian noise on both projections, 5000 keypoints per frame of which N are matched
(the rest only move Normalize), the minimal sets drawn with the reference's loop over Python's seeded generator, iterations = 200.
  N = 300     about what SearchForInitialization leaves on a 1000-feature frame pair
  N = 1500    a 5 x nFeatures initialisation extractor with most keypoints matched
The entry is called through ctypes on arguments built beforehand; --rounds rounds of --calls calls each; wall clock per call as the
median and range of the rounds' means.  The outputs must equal the host form's bit for bit: exit status 1 otherwise.  Prints text
lines and one JSON line and writes them to --out.  Needs a GPU; there is no fallback.  (profiles/two_view_layouts_bench.txt is this
tool's output while a second layout of the hypothesis kernel, one lane per hypothesis, was still in the tree: DESIGN.md section 5.)

Not measured: real matches, the cost of the adapter's copies inside ORB-SLAM3.

--kernels CALLS instead makes CALLS runs of the N = 1500 scene and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats`, which times k_tv_hypotheses, k_tv_score, k_tv_winner, k_tv_check_rt and k_tv_cos_rank.

    python tools/two_view_bench.py [--rounds 5] [--calls 20] [--out profiles/two_view_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o tv --output-format csv -- python tools/two_view_bench.py --kernels 50
"""
import argparse
import ctypes as C
import importlib
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ITERATIONS = 200
KEYPOINTS = 5000
K = np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1]], np.float32)


def make_scene(pkg, N, seed):
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-2, 2, N), rng.uniform(-1.5, 1.5, N), rng.uniform(4, 9, N)]
    a = 0.05
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([0.4, 0.05, 0.02])

    def project(P):
        p = (K.astype(np.float64) @ P.T).T
        return p[:, :2] / p[:, 2:]

    xy1 = rng.uniform((0, 0), (640, 480), (KEYPOINTS, 2))
    xy2 = rng.uniform((0, 0), (640, 480), (KEYPOINTS, 2))
    pos1, pos2 = rng.permutation(KEYPOINTS)[:N], rng.permutation(KEYPOINTS)[:N]
    xy1[pos1] = project(X) + rng.normal(0, 0.3, (N, 2))
    xy2[pos2] = project((R @ X.T).T + t) + rng.normal(0, 0.3, (N, 2))
    keys = []
    for xy in (xy1, xy2):
        k = np.zeros(KEYPOINTS, pkg.KP_DTYPE)
        k["x"], k["y"], k["size"], k["class_id"] = xy[:, 0], xy[:, 1], 31, -1
        keys.append(k)
    m12 = np.full(KEYPOINTS, -1, np.int32)
    m12[pos1] = pos2
    r = random.Random(seed)
    sets = np.zeros((ITERATIONS, 8), np.int32)
    for it in range(ITERATIONS):                      # the reference's draw, TwoViewReconstruction.cc:81-96
        avail = list(range(N))
        for j in range(8):
            i = r.randint(0, len(avail) - 1)
            sets[it, j] = avail[i]
            avail[i] = avail[-1]
            avail.pop()
    return keys[0], keys[1], m12, sets


def call_of(pkg, m, scene):
    k1, k2, m12, sets = scene
    Kf = K.reshape(9).copy()
    out = [np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros(3 * KEYPOINTS, np.float32), np.zeros(KEYPOINTS, np.uint8)]
    args = [pkg._p(k1), KEYPOINTS, pkg._p(k2), KEYPOINTS, pkg._p(m12), pkg._p(Kf), C.c_float(1.0), ITERATIONS, pkg._p(sets)] + [pkg._p(o) for o in out]
    keep = (k1, k2, m12, sets, Kf)

    def call():
        return m.L.orbm_two_view_reconstruct(m.m, *args, None)

    return call, out, keep


def same(a, b):
    return a.tobytes() == b.tobytes()


def measure(name, pkg, m, scene, rounds, calls, warmup):
    want = pkg.two_view_reconstruct_host(scene[0], scene[1], scene[2], K, 1.0, ITERATIONS, scene[3])
    call, out, keep = call_of(pkg, m, scene)
    for _ in range(warmup):
        rc = call()
        if rc < 0:
            raise SystemExit("%s: rc=%d: %s" % (name, rc, m.L.orbm_last_error(m.m)))
    means = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        means.append((time.perf_counter() - t0) * 1e3 / calls)
    identical = rc == int(want.ok)
    if want.ok:
        identical = identical and same(out[0], want.R21) and same(out[1], want.t21) and same(out[2], want.vP3D) and \
            same(out[3], want.vbTriangulated.astype(np.uint8))
    N = int((scene[2] >= 0).sum())
    res = dict(case=name, matches=N, keypoints=KEYPOINTS, iterations=ITERATIONS, reconstructed=bool(want.ok),
               triangulated=int(want.vbTriangulated.sum()) if want.ok else 0, identical=bool(identical), rounds=rounds, calls=calls,
               call_ms=dict(median=statistics.median(means), min=min(means), max=max(means), rounds=means))
    lines = ["%s: %d matches among %d keypoints per frame, %d iterations; Reconstruct returns %s, %d points triangulated"
             % (name, N, KEYPOINTS, ITERATIONS, want.ok, res["triangulated"]),
             "  orbm_two_view_reconstruct: median %.4f ms per call (range %.4f-%.4f, %d rounds x %d calls)"
             % (res["call_ms"]["median"], min(means), max(means), rounds, calls),
             "  outputs against the host form: %s" % ("identical" if identical else "DIFFERENT")]
    return res, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0, help="only make this many runs of the N = 1500 scene (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_bench.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    m = pkg.ORBmatcher(0.9, True)
    if a.kernels:
        scene = make_scene(pkg, 1500, 32)
        call, out, keep = call_of(pkg, m, scene)
        for _ in range(a.kernels):
            if call() < 0:
                raise SystemExit("kernel run failed: %s" % m.L.orbm_last_error(m.m))
        m.close()
        print("N = 1500: %d runs" % a.kernels)
        return 0
    results, lines = [], []
    for name, N, seed in (("N = 300", 300, 31), ("N = 1500", 1500, 32)):
        res, text = measure(name, pkg, m, make_scene(pkg, N, seed), a.rounds, a.calls, a.warmup)
        results.append(res)
        lines += text
    m.close()
    lines.append("the scenes are invented; no gain is claimed: nothing on the parent or in the reference build is measured against these times")
    lines.append(json.dumps(dict(cases=results)))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(r["identical"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
