#!/usr/bin/env python3
"""LocalMapping::KeyFrameCulling on the device (LocalMapping.cc:1158-1310): wall clock of the one-call form orbm_keyframe_culling and of
the stepwise form orbm_keyframe_culling_open + _step on synthetic local maps.  There is nothing to compare with: the parent has no such
path and the reference's member is not built here, so NO GAIN IS CLAIMED; the host form orbm_keyframe_culling_host is new code, used
here only to check the outputs.

Synthetic local maps, built without images: K keyframes of R rows, 70 % of the rows hold a map point, every map point is seen by eight
keyframes of a window of the list and by two observers outside it (ten observations per point; a fifth of them stereo, weight 2), levels
spread over eight octaves so that at most 82 % of a keyframe's rows are redundant, below redundant_th = 0.9.  For "3 culled" the rows of
three keyframes sit at a coarse level, so that every observation of their points counts: exactly these pass and are erased.
  30 x 1000    30 keyframes of 1000 rows, 0 and 3 keyframes culled
  100 x 1500   100 keyframes of 1500 rows, 0 and 3 keyframes culled
Both forms are called through ctypes on arguments built beforehand.  --rounds rounds, the two forms alternated inside a round, --calls
calls each; wall clock per call (a whole loop: for the stepwise form open plus every step, the erases applied as the one-call form
applied them) as the median and range of the rounds' means.  The outputs of both forms must equal the host form's: exit status 1
otherwise.  Prints text lines and one JSON line and writes them to --out.  Needs a GPU; there is no fallback.

Not measured: real observation counts, and the cost of flattening the map inside ORB-SLAM3 (the adapter's constructor).

--kernels CALLS instead makes CALLS one-call runs of "100 x 1500, 3 culled" and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats`, which times k_cull_count and k_cull_walk; --outside N gives every map point N observers outside
the list instead of two (92: lists of 100 entries, which the wavefront walks in tiles), --stragglers N gives N map points 2000 more
observations that never qualify (a few long lists among short ones).

    python tools/keyframe_culling_bench.py [--rounds 5] [--calls 20] [--out profiles/keyframe_culling_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o cull --output-format csv -- python tools/keyframe_culling_bench.py --kernels 50
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


COARSE = 20   # a row level that every observation's level lies below


def make_map(K, rows, culled, seed, outside=2, stragglers=0):
    rng = np.random.default_rng(seed)
    held = int(rows * 0.7)
    P = K * held // 8
    chosen = set(int(k) for k in rng.choice(np.arange(2, K - 2), culled, replace=False)) if culled else set()
    per_kf = [[] for _ in range(K)]
    obs_start, obs_kf, obs_level, obs_w, n_obs = [0], [], [], [], []
    for p in range(P):
        c = int(rng.integers(0, K))
        lo = min(max(0, c - 8), K - 16)
        kfs = lo + rng.choice(16, 8, replace=False)
        base = int(rng.integers(0, 4))
        levels = base + rng.integers(0, 8, 8 + outside)
        w = np.where(rng.random(8 + outside) < 0.2, 2, 1)
        ids = list(kfs) + [-1] * outside
        if stragglers and p % (P // stragglers) == 0:                # a long tail that never hits: the whole list is walked
            ids += [-1] * 2000
            levels = np.append(levels, [99] * 2000)
            w = np.append(w, [1] * 2000)
        for k, lv in zip(kfs, levels[:8]):
            per_kf[int(k)].append((p, int(lv)))
        obs_kf += [int(k) for k in ids]
        obs_level += [int(v) for v in levels]
        obs_w += [int(v) for v in w]
        n_obs.append(int(w.sum()))
        obs_start.append(len(obs_kf))
    row_start, row_point, row_level = [0], [], []
    for k in range(K):
        pts = per_kf[k][:rows]
        filler = rows - len(pts)
        order = rng.permutation(rows)
        rp = np.array([p for p, _ in pts] + [-1] * filler, np.int32)[order]
        rl = np.array([COARSE if k in chosen else lv for _, lv in pts] + [0] * filler, np.int32)[order]
        row_point.append(rp)
        row_level.append(rl)
        row_start.append(row_start[-1] + rows)
    R = row_start[-1]
    skip = np.zeros(K, np.uint8)
    skip[0] = 1                                                      # the map's first keyframe
    return dict(skip=skip, th_depth=np.full(K, 40.0, np.float32), row_start=np.array(row_start, np.int32), row_point=np.concatenate(row_point),
                row_level=np.concatenate(row_level), row_depth=rng.choice(np.array([1.0, 10.0, 39.0], np.float32), R), bad=np.zeros(P, np.uint8),
                n_obs=np.array(n_obs, np.int32), obs_start=np.array(obs_start, np.int32), obs_kf=np.array(obs_kf, np.int32),
                obs_level=np.array(obs_level, np.int32), obs_w=np.array(obs_w, np.uint8), mono=0, redundant_th=np.float32(0.9)), sorted(chosen)


def forms_of(pkg, m, scene, culled):
    L = m.L
    c, keep = pkg.culling_struct(scene)
    K, P = c.K, c.P
    o1 = [np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.uint8), np.zeros(P, np.int32), np.zeros(P, np.uint8)]
    a1 = [pkg._p(o) for o in o1]
    o2 = [np.zeros(K, np.int32), np.zeros(K, np.int32)]
    a2 = [pkg._p(o) for o in o2]
    at = np.zeros(1, np.int32)
    pat = pkg._p(at)
    steps = [0]

    def one_call():
        return L.orbm_keyframe_culling(m.m, C.byref(c), None, *a1)

    def stepwise():
        rc = L.orbm_keyframe_culling_open(m.m, C.byref(c))
        applied, n = 0, 0
        while rc == 0:
            rc = L.orbm_keyframe_culling_step(m.m, applied, pat, *a2)
            n += 1
            if at[0] >= K:
                break
            applied = int(culled[at[0]])
        steps[0] = n
        return rc

    return one_call, stepwise, o1, o2, steps, (c, keep)


def measure(name, pkg, m, scene, chosen, rounds, calls, warmup):
    want = pkg.keyframe_culling_host(scene)
    one_call, stepwise, o1, o2, steps, keep = forms_of(pkg, m, scene, want[2])
    forms = (("one call (orbm_keyframe_culling)", one_call), ("stepwise (open + steps)", stepwise))
    for label, fn in forms:
        for _ in range(warmup):
            rc = fn()
            if rc < 0:
                raise SystemExit("%s: %s rc=%d: %s" % (name, label, rc, m.L.orbm_last_error(m.m)))
    means = [[] for _ in forms]
    for _ in range(rounds):
        for r, (label, fn) in enumerate(forms):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            means[r].append((time.perf_counter() - t0) * 1e3 / calls)
    identical = all(np.array_equal(a, b) for a, b in zip(o1, want)) and np.array_equal(o2[0], want[0]) and np.array_equal(o2[1], want[1])
    K, P = len(scene["skip"]), len(scene["bad"])
    res = dict(case=name, keyframes=K, rows=int(scene["row_start"][-1]), points=P, entries=int(scene["obs_start"][-1]),
               culled=[int(k) for k in np.nonzero(want[2])[0]], intended=chosen, steps=steps[0], identical=bool(identical), rounds=rounds, calls=calls)
    lines = ["%s: %d keyframes, %d rows, %d map points, %d observations (%.1f per point); culled %s; %d steps in the stepwise form"
             % (name, K, res["rows"], P, res["entries"], res["entries"] / max(P, 1), res["culled"], steps[0])]
    for key, (label, _), v in zip(("one_call_ms", "stepwise_ms"), forms, means):
        res[key] = dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)
        lines.append("  %-36s median %.4f ms per loop (range %.4f-%.4f, %d rounds x %d calls)" % (label + ":", res[key]["median"], min(v), max(v), rounds, calls))
    lines.append("  outputs of both forms against the host form: %s" % ("identical" if identical else "DIFFERENT"))
    return res, lines


def cases():
    return (("30 x 1000, 0 culled", 30, 1000, 0, 21), ("30 x 1000, 3 culled", 30, 1000, 3, 21),
            ("100 x 1500, 0 culled", 100, 1500, 0, 22), ("100 x 1500, 3 culled", 100, 1500, 3, 22))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0, help="only make this many one-call runs of the largest case (for a kernel trace)")
    ap.add_argument("--outside", type=int, default=2, help="with --kernels: observers outside the list per map point (92 gives lists of 100 entries)")
    ap.add_argument("--stragglers", type=int, default=0, help="with --kernels: this many map points get 2000 more observations that never qualify")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_culling_bench.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    m = pkg.ORBmatcher(0.8, True)
    if a.kernels:
        name, K, rows, culled, seed = cases()[3]
        scene, chosen = make_map(K, rows, culled, seed, a.outside, a.stragglers)
        want = pkg.keyframe_culling_host(scene)
        one_call, _, o1, _, _, keep = forms_of(pkg, m, scene, want[2])
        for _ in range(a.kernels):
            if one_call() < 0:
                raise SystemExit("kernel run failed: %s" % m.L.orbm_last_error(m.m))
        m.close()
        same = all(np.array_equal(x, y) for x, y in zip(o1, want))
        print("%s: culled %s, outputs against the host form: %s" % (name, list(np.nonzero(want[2])[0]), "identical" if same else "DIFFERENT"))
        return 0 if same else 1
    results, lines = [], []
    for name, K, rows, culled, seed in cases():
        scene, chosen = make_map(K, rows, culled, seed)
        res, text = measure(name, pkg, m, scene, chosen, a.rounds, a.calls, a.warmup)
        results.append(res)
        lines += text
    m.close()
    lines.append("no gain is claimed: nothing on the parent or in the reference build is measured against these times")
    lines.append(json.dumps(dict(cases=results)))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if all(r["identical"] and r["culled"] == r["intended"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
