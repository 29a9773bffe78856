#!/usr/bin/env python3
"""Sim3Solver on the device (Sim3Solver.cc:35-530): wall clock of the one-call form orbm_sim3_solve on invented scenes, its split over the
host's four phases, and the hypothesis stage on the device against the same stage on the host.  There is nothing to compare with: the
parent has no such path and the reference's file is not built here, so NO GAIN IS CLAIMED; the host forms are new code, used here to
check the outputs and to time one stage, and are no yardstick.

The scenes are INVENTED: N pairs of map points 3 to 8 units in front of keyframe 1 (Pinhole 458 / 457 / 367 / 248), the second map a
similarity (scale 1.6, 0.25 rad) and 2 mm of noise away behind another pose and another Pinhole camera, 30 % of the pairs unrelated;
sigma2 from the first four levels of a 1.2 pyramid; sets drawn with the reference's loop over Python's seeded generator.
  N = 30, 100, 300          what SearchByBoW against a candidate and its covisibles leaves (LoopClosing.cc:724-739 keeps 20 and more)
  "full"                    300 iterations, min_inliers = N: no iteration can converge, the whole chunk is scored
  "converges"               the same scene with min_inliers = N / 3 and five sets of unrelated pairs in front: it stops at iteration 5;
                            the call still scores all 300 sets (the SIM3 RULE computes every count, then one ordered pass)
Per case: --rounds rounds of --calls calls; wall clock per call as the median and range of the rounds' means; the mean of
orbm_sim3_details_t::wall_ms over the same calls (constructor on the host; upload, k_sim3_hypotheses, first synchronisation; host tail;
upload, k_sim3_check, k_sim3_winner, second synchronisation); orbm_sim3_hypotheses (device stage and host tail) against
orbm_sim3_hypotheses_host (host Jacobi and host tail) on the same 300 sets.  The outputs must equal the host form's bit for bit: exit
status 1 otherwise.  Prints text lines and one JSON line and writes them to --out.  Needs a GPU; there is no fallback.

Not measured: real BoW matches, the call inside ORB-SLAM3 (the adapter's copies, the loop-closing thread next to the others).

--kernels CALLS instead makes CALLS runs of the N = 300 "full" case and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats`, which times k_sim3_hypotheses, k_sim3_check and k_sim3_winner.

    python tools/sim3_solver_bench.py [--rounds 5] [--calls 20] [--out profiles/sim3_solver_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o sim3 --output-format csv -- python tools/sim3_solver_bench.py --kernels 50
"""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ITERATIONS = 300
F = np.float32


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def make_scene(N, seed, converges):
    rng = np.random.default_rng(seed)
    s, R, t = 1.6, rot(rng.normal(0, 1, 3), 0.25), rng.normal(0, 0.15, 3)
    X1 = np.c_[rng.uniform(-1.5, 1.5, N), rng.uniform(-1.0, 1.0, N), rng.uniform(3.0, 8.0, N)]
    X2 = (X1 - t) @ R / s + rng.normal(0, 0.002, (N, 3))
    n_out = int(round(0.3 * N))
    X2[N - n_out:] = np.c_[rng.uniform(-1.5, 1.5, n_out), rng.uniform(-1.0, 1.0, n_out), rng.uniform(3.0, 8.0, n_out)] / s
    T1, T2 = pose(rot(rng.normal(0, 1, 3), 0.7), rng.normal(0, 2.0, 3)), pose(rot(rng.normal(0, 1, 3), 1.1), rng.normal(0, 3.0, 3))
    n1 = 4 * N
    sigma2 = np.array([1.2 ** (2 * k) for k in range(4)], F)
    prob = dict(n1=n1, idx1=np.sort(rng.choice(n1, N, replace=False)).astype(np.int32), Xw1=((X1 - T1[:3, 3]) @ T1[:3, :3]).astype(F),
                Xw2=((X2 - T2[:3, 3]) @ T2[:3, :3]).astype(F), sigma2_1=sigma2[rng.integers(0, 4, N)], sigma2_2=sigma2[rng.integers(0, 4, N)],
                Tcw1=T1.astype(F), Tcw2=T2.astype(F), cam_type1=0, cam_params1=np.array([458.0, 457.0, 367.0, 248.0], F), cam_type2=0,
                cam_params2=np.array([520.9, 521.0, 325.1, 249.7], F), fix_scale=False, min_inliers=N // 3 if converges else N,
                iterations_done=0, max_iterations=ITERATIONS)
    r = random.Random(seed)
    sets = np.zeros((ITERATIONS, 3), np.int32)
    for it in range(ITERATIONS):                      # the reference's draw, Sim3Solver.cc:199-213
        avail = list(range(N))
        for j in range(3):
            i = r.randint(0, len(avail) - 1)
            sets[it, j] = avail[i]
            avail[i] = avail[-1]
            avail.pop()
    if converges:
        for it in range(5):                           # unrelated pairs in front, then three true pairs
            sets[it] = (N - 1 - it, N - 7 - it, N - 13 - it)
        sets[5] = (0, (N - n_out) // 3, 2 * (N - n_out) // 3)
    return prob, sets


def raw_call(pkg, m, prob, sets):
    """The entry through ctypes on arguments built beforehand; returns (call, result struct, wall_ms [4], everything to keep alive)"""
    P, N, n1, keep = pkg._sim3_problem(prob)
    sets = np.ascontiguousarray(sets, np.int32)
    best_mask, vb, wall = np.zeros(N, np.uint8), np.zeros(n1, np.uint8), np.zeros(4, np.float64)
    r, d = pkg.Sim3ResultStruct(), pkg.Sim3DetailsStruct()
    r.best_mask, r.vbInliers, d.wall_ms = best_mask.ctypes.data, vb.ctypes.data, wall.ctypes.data
    args = (m.m, C.byref(P), len(sets), pkg._p(sets), 0, C.byref(r), C.byref(d))
    return (lambda: m.L.orbm_sim3_solve(*args)), r, wall, (P, keep, sets, best_mask, vb, d)


def timed(fn, rounds, calls):
    means = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        means.append((time.perf_counter() - t0) * 1e3 / calls)
    return dict(median=statistics.median(means), min=min(means), max=max(means), rounds=means)


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def measure(name, pkg, m, prob, sets, rounds, calls, warmup):
    want = pkg.sim3_solve_host(prob, sets, 0)
    call, r, wall, keep = raw_call(pkg, m, prob, sets)
    for _ in range(warmup):
        rc = call()
        if rc < 0:
            raise SystemExit("%s: rc=%d: %s" % (name, rc, m.L.orbm_last_error(m.m)))
    phases = np.zeros(4)

    def counted():
        call()
        phases[:] += wall

    call_ms = timed(counted, rounds, calls)
    phases /= rounds * calls
    got = m.Sim3Solve(prob, sets, 0)
    identical = all(getattr(got, k) == getattr(want, k) for k in ("converged", "it_stop", "best_it", "best_inliers", "improved", "no_more")) and \
        same(got.T12, want.T12) and same(got.best_mask, want.best_mask) and same(got.vbInliers, want.vbInliers) and \
        all(same(v, want.details[k]) for k, v in got.details.items())
    P, N, n1, pk = pkg._sim3_problem(prob)
    s32 = np.ascontiguousarray(sets, np.int32)
    outs = [np.zeros((len(s32), 16), F), np.zeros((len(s32), 16), F), np.zeros((len(s32), 4), F)]
    hyp_args = (C.byref(P), len(s32), pkg._p(s32)) + tuple(pkg._p(o) for o in outs)
    hyp_dev = timed(lambda: m.L.orbm_sim3_hypotheses(m.m, *hyp_args), rounds, calls)
    hyp_host = timed(lambda: m.L.orbm_sim3_hypotheses_host(*hyp_args), rounds, calls)
    res = dict(case=name, pairs=N, iterations=len(s32), converged=want.converged, it_stop=want.it_stop, best_inliers=want.best_inliers,
               identical=bool(identical), rounds=rounds, calls=calls, call_ms=call_ms,
               phase_ms=dict(constructor=phases[0], hypotheses_to_sync1=phases[1], host_tail=phases[2], check_winner_to_sync2=phases[3]),
               hypotheses_stage_ms=dict(device=hyp_dev, host=hyp_host))
    tot = call_ms["median"]
    lines = ["%s: %d pairs, %d iterations; converged %d at it_stop %d, best %d inliers" % (name, N, len(s32), want.converged, want.it_stop, want.best_inliers),
             "  orbm_sim3_solve: median %.4f ms per call (range %.4f-%.4f, %d rounds x %d calls)" % (tot, call_ms["min"], call_ms["max"], rounds, calls),
             "  host clock per phase, mean: constructor %.4f ms; upload + k_sim3_hypotheses + sync 1 %.4f ms (%.0f %%); host tail %.4f ms (%.0f %%); "
             "upload + k_sim3_check + k_sim3_winner + sync 2 %.4f ms (%.0f %%)"
             % (phases[0], phases[1], 100 * phases[1] / tot, phases[2], 100 * phases[2] / tot, phases[3], 100 * phases[3] / tot),
             "  hypothesis stage alone, %d sets: orbm_sim3_hypotheses (device Jacobi, host tail) median %.4f ms (range %.4f-%.4f); "
             "orbm_sim3_hypotheses_host (host Jacobi, host tail) median %.4f ms (range %.4f-%.4f)"
             % (len(s32), hyp_dev["median"], hyp_dev["min"], hyp_dev["max"], hyp_host["median"], hyp_host["min"], hyp_host["max"]),
             "  outputs against the host form: %s" % ("identical" if identical else "DIFFERENT")]
    return res, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0, help="only make this many runs of the N = 300 full case (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_solver_bench.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    m = pkg.ORBmatcher(0.9, True)
    if a.kernels:
        prob, sets = make_scene(300, 53, False)
        call, r, wall, keep = raw_call(pkg, m, prob, sets)
        for _ in range(a.kernels):
            if call() < 0:
                raise SystemExit("kernel run failed: %s" % m.L.orbm_last_error(m.m))
        m.close()
        print("N = 300, full: %d runs" % a.kernels)
        return 0
    results, lines = [], []
    for N, seed in ((30, 51), (100, 52), (300, 53)):
        for kind in ("full", "converges"):
            prob, sets = make_scene(N, seed, kind == "converges")
            res, text = measure("N = %d, %s" % (N, kind), pkg, m, prob, sets, a.rounds, a.calls, a.warmup)
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
