#!/usr/bin/env python3
"""SearchForTriangulation between two KannalaBrandt8 rig keyframes of TUM-VI size: orbm_search_for_triangulation_kb8 (the epipolar test
on the device) against the route it replaces, orbm_search_for_triangulation_pred around a host predicate.

Builds the scene of tests/triangulation_kb8_scene.py at --points (2600 points: 2600 keypoints in KF1, about 3470 in KF2 with one decoy
per third point, both cameras of the rig, 100 vocabulary nodes - DBoW2's level for levelsup = 4 holds about that many), writes it to a
scratch file, compiles tools/triangulation_kb8_harness.c against liborbhip.so and runs it: both routes in one process, alternated over
--rounds, wall time per call.  With --profile a second run of the harness, the device route only, goes under
rocprofv3 --kernel-trace --stats and the device times of its kernels are added (the entry runs the one-call form's kernels with K = 1:
k_triangulation_candidates_neighbours, k_triangulation_kb8_predicate_neighbours, k_triangulation_kb8_result_neighbours).  Exit status 1 if the routes disagree.  Prints text
lines and one JSON line and writes them to --out.  Needs a GPU; there is no fallback.

    python tools/triangulation_kb8_bench.py [--points 2600] [--nodes 100] [--rounds 7] [--calls 200] [--profile] [--out profiles/triangulation_kb8_bench.txt]
"""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def write_scene(path, S, nodes, SC, pkg):
    views = SC.product_views(pkg, S, nodes)
    with open(path, "wb") as f:
        np.array([views[0].N, views[1].N, S["n_left1"], S["n_left2"], len(views[0].node_id), len(views[1].node_id),
                  int(views[0].node_start[-1]), int(views[1].node_start[-1]), len(S["sf"])], np.int32).tofile(f)
        for v in (S["ep"], S["cams1"], S["cams2"], S["T12"], S["sf"], S["sigma2"]):
            np.ascontiguousarray(v, np.float32).tofile(f)
        for K in views:
            K.keys_un.tofile(f); K.descriptors.tofile(f); K.has_mappoint.tofile(f)
            K.node_id.tofile(f); K.node_start.tofile(f); K.node_idx[:int(K.node_start[-1])].tofile(f)
    return views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2600)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulation_kb8_bench.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    pkg.load()                                                   # builds liborbhip.so when the sources are newer
    import triangulation_kb8_scene as SC
    S = SC.make_scene(a.points, True, max_decoys=1)
    build = os.path.join(ROOT, "build")
    os.makedirs(build, exist_ok=True)
    scene = os.path.join(build, "triangulation_kb8_scene.bin")
    K1, K2 = write_scene(scene, S, a.nodes, SC, pkg)
    libdir = os.path.join(ROOT, "3_orb_slam3_selfnote_amd")
    exe = os.path.join(build, "triangulation_kb8_harness")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "triangulation_kb8_harness.c"), "-o", exe,
                           "-L", libdir, "-lorbhip", "-Wl,-rpath," + libdir, "-lm"])
    env = dict(os.environ)
    torch_lib = None
    try:
        import torch
        torch_lib = os.path.join(os.path.dirname(torch.__file__), "lib")
    except Exception:
        pass
    env["LD_LIBRARY_PATH"] = ":".join(x for x in ("/opt/rocm/lib", torch_lib, env.get("LD_LIBRARY_PATH", "")) if x)
    run = subprocess.run([exe, scene, "--rounds", str(a.rounds), "--calls", str(a.calls), "--warmup", str(a.warmup)], env=env, capture_output=True, text=True)
    if run.returncode not in (0, 1) or not run.stdout.strip():
        sys.stderr.write(run.stdout + run.stderr)
        return run.returncode or 3
    res = json.loads(run.stdout.strip().splitlines()[-1])
    members = np.diff(K2.node_start)
    res.update(points=a.points, nodes=a.nodes, node_members_kf2_mean=float(members.mean()), node_members_kf2_max=int(members.max()))
    lines = ["scene: KannalaBrandt8 rig pair, %d + %d keypoints (left + right) in KF1, %d + %d in KF2, %d / %d vocabulary nodes (%.1f members of KF2 per node, at most %d)"
             % (res["n_left1"], res["n1"] - res["n_left1"], res["n_left2"], res["n2"] - res["n_left2"], res["nodes1"], res["nodes2"], members.mean(), members.max()),
             "candidates in front of the epipolar test: %d in %d lists; matches after the orientation check: %d" % (res["candidates"], res["lists"], res["matches_kb8"]),
             "(a) orbm_search_for_triangulation_kb8: median %.4f, min %.4f, max %.4f ms wall per call (%d rounds x %d calls, %d warm-up); %d evaluations of the test per call, all on the device"
             % (res["kb8_ms_median"], res["kb8_ms_min"], res["kb8_ms_max"], res["rounds"], res["calls_per_round"], res["warmup"], res["evals_kb8_per_call"]),
             "(b) orbm_search_for_triangulation_pred around a C predicate (orbm_fisheye_triangulate, n = 1): median %.4f, min %.4f, max %.4f ms wall per call; %.1f evaluations per call, on the calling thread"
             % (res["pred_ms_median"], res["pred_ms_min"], res["pred_ms_max"], res["evals_pred_per_call"]),
             "(b) / (a): %.2f x; extra evaluations of (a): %.1f per call" % (res["pred_ms_median"] / res["kb8_ms_median"], res["evals_kb8_per_call"] - res["evals_pred_per_call"]),
             "matches12 of (a) and (b): %s" % ("identical" if res["identical"] else "DIFFERENT")]
    if a.profile:
        prof = os.path.join(build, "triangulation_kb8_prof")
        shutil.rmtree(prof, ignore_errors=True)
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "--", exe, scene, "--only", "a", "--rounds", "1",
                            "--calls", str(a.calls), "--warmup", "2"], env=env, capture_output=True, text=True)
        stats = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode or not stats:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            return 3
        kernels = {}
        with open(stats[0]) as f:
            for r in csv.DictReader(f):
                if "k_triangulation" in r["Name"] and "_neighbours" in r["Name"]:
                    name = r["Name"].split("(")[0].split()[-1]
                    kernels[name] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
        shutil.rmtree(prof, ignore_errors=True)
        res["kernels_us"] = kernels
        lines.append("device time per launch, rocprofv3 --kernel-trace --stats, a run of its own of the device route: " +
                     "; ".join("%s avg %.1f us (min %.1f, max %.1f, %d launches)" % (k, v["avg_us"], v["min_us"], v["max_us"], v["calls"]) for k, v in kernels.items()))
    os.remove(scene)
    lines.append(json.dumps(res))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if res["identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
