#!/usr/bin/env python3
"""Tracking::UpdateLocalMap (Tracking.cc:3542-3762) and KeyFrame::UpdateConnections (KeyFrame.cc:407-492) on the device: wall clock per call
on a SYNTHETIC map.  There is nothing to compare with: the parent has no such path and the reference's members are not built here, so NO
GAIN IS CLAIMED; the host forms are new code, used here only to check the outputs.  The one comparison made is the device-table form
against the upload form on the same handle, which is a statement about residency and nothing more.

The synthetic map, built without images: 500 keyframes of 1000 rows, 70 % of the rows hold a map point, every map point is seen by eight
keyframes of a window of sixteen (about eight observations per point); every keyframe has ten best covisibles, a parent, a previous
keyframe and up to two children.  The frame has 1000 slots, 300 of which hold a point seen around keyframe 250.
  local map, upload form        orbm_update_local_map: tables uploaded with every call
  local map, device tables      orbm_update_local_map_device + a synchronisation: tables resident
  local map -> search           orbm_update_local_map_device -> orbm_gather_local_map_device -> orbm_search_local_points_batch_device, one
                                synchronisation at the end (a pinhole frame of 1000 keypoints whose descriptors are noisy copies of local points)
  connections T = 40 / T = 150  orbm_update_connections (a loop-closing call / a map merge)
Both vote forms of k_covis_vote are timed (ORBM_VOTE_FORM, read when a handle is created): the LDS table, and one global atomic per vote.
--rounds rounds of --calls calls per form, the forms alternated inside a round; the median and range of the rounds' means.  The outputs
must equal the host forms': exit status 1 otherwise.  Prints text lines and one JSON line and writes them to --out.  Needs a GPU.

Not measured: the cost of flattening the map inside ORB-SLAM3, how often local mapping dirties the resident tables and what rewriting them
costs, real observation counts and real covisibility graphs.

--kernels CALLS instead makes CALLS runs of the chain and of the T = 150 connections call and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats`.

    python tools/local_map_bench.py [--rounds 5] [--calls 20] [--out profiles/local_map_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o lm --output-format csv -- python tools/local_map_bench.py --kernels 50 [--vote-form 1]
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K, ROWS, SLOTS, MATCHED = 500, 1000, 1000, 300
CAM = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
BOUNDS = (0.0, 752.0, 0.0, 480.0)


def make_map(seed=31):
    rng = np.random.default_rng(seed)
    held = int(ROWS * 0.7)
    P = K * held // 8
    per_kf = [[] for _ in range(K)]
    obs_start, obs_kf = [0], []
    centre = rng.integers(0, K, P)
    for p in range(P):
        lo = min(max(0, int(centre[p]) - 8), K - 16)
        kfs = np.sort(lo + rng.choice(16, 8, replace=False))
        for k in kfs:
            per_kf[int(k)].append(p)
        obs_kf += [int(k) for k in kfs]
        obs_start.append(len(obs_kf))
    row_point = []
    for k in range(K):
        pts = per_kf[k][:ROWS]
        row_point.append(np.array(pts + [-1] * (ROWS - len(pts)), np.int32)[rng.permutation(ROWS)])
    best = np.full((K, 10), -1, np.int32)
    child_start, child = [0], []
    for k in range(K):
        near = [g for g in range(k - 6, k + 7) if 0 <= g < K and g != k]
        b = rng.permutation(near)[:10]
        best[k, :len(b)] = b
        child += [g for g in (k + 1, k + 2) if g < K and rng.random() < 0.6]
        child_start.append(len(child))
    graph = dict(kf_rank=rng.permutation(K).astype(np.int32), kf_bad=(rng.random(K) < 0.02).astype(np.uint8), kf_map=np.zeros(K, np.int32),
                 kf_row_start=np.arange(K + 1, dtype=np.int32) * ROWS, row_point=np.concatenate(row_point), kf_best=best.reshape(-1),
                 kf_child_start=np.array(child_start, np.int32), kf_child=np.array(child, np.int32),
                 kf_parent=np.maximum(np.arange(K) - 1, -1).astype(np.int32), kf_prev=np.maximum(np.arange(K) - 1, -1).astype(np.int32),
                 pt_bad=(rng.random(P) < 0.01).astype(np.uint8), obs_start=np.array(obs_start, np.int32), obs_kf=np.array(obs_kf, np.int32))
    # children in ascending rank (RANK RULE)
    for k in range(K):
        c = graph["kf_child"][child_start[k]:child_start[k + 1]]
        graph["kf_child"][child_start[k]:child_start[k + 1]] = c[np.argsort(graph["kf_rank"][c])]
    near = np.nonzero(np.abs(centre - 250) < 6)[0]
    frame = np.full(SLOTS, -1, np.int32)
    frame[rng.choice(SLOTS, MATCHED, replace=False)] = rng.choice(near, MATCHED, replace=False)
    # per-point tables for the chain: points in front of an identity camera, seen head-on
    z = rng.uniform(2.0, 10.0, P).astype(np.float32)
    u, v = rng.uniform(20, 730, P).astype(np.float32), rng.uniform(20, 460, P).astype(np.float32)
    Xw = np.stack([(u - CAM[2]) / CAM[0] * z, (v - CAM[3]) / CAM[1] * z, z], 1).astype(np.float32)
    dist = np.linalg.norm(Xw, axis=1).astype(np.float32)
    tables = dict(Xw=Xw, normal=(Xw / dist[:, None]).astype(np.float32), max_dist=(dist * 1.1).astype(np.float32), min_dist=(dist * 0.5).astype(np.float32),
                  mpdesc=rng.integers(0, 256, (P, 32), dtype=np.uint8), uv=np.stack([u, v], 1))
    return graph, frame, tables


class Chain:
    """The resident forms on one handle: tables, frame and outputs on the device."""

    def __init__(self, pkg, m, graph, frame, tables, want_points):
        import torch
        self.torch, self.pkg, self.m = torch, pkg, m
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.g, self.keep = pkg.map_graph_device(graph)
        P = len(graph["pt_bad"])
        self.P, self.N, self.cap = P, len(frame), 65536
        self.d_fp = t(frame)
        self.d_lkf = torch.zeros(K + 24, dtype=torch.int32, device="cuda")
        self.d_lp = torch.zeros(self.cap, dtype=torch.int32, device="cuda")
        self.d_sb = torch.zeros(self.N, dtype=torch.uint8, device="cuda")
        self.d_res = torch.zeros(6, dtype=torch.int32, device="cuda")
        self.tab = {k: t(tables[k]) for k in ("Xw", "normal", "max_dist", "min_dist", "mpdesc")}
        self.d_bad = self.keep["pt_bad"]
        f = lambda *s: torch.zeros(*s, device="cuda")
        self.o = dict(elig=torch.zeros(self.cap, dtype=torch.uint8, device="cuda"), Xw=f(self.cap, 3), nrm=f(self.cap, 3), maxd=f(self.cap), mind=f(self.cap),
                      desc=torch.zeros(self.cap, 32, dtype=torch.uint8, device="cuda"))
        self.d_T = t(np.eye(4, dtype=np.float32))
        o = self.o
        self.ms = pkg.LocalMapStruct(self.cap, o["elig"].data_ptr(), o["Xw"].data_ptr(), o["nrm"].data_ptr(), o["maxd"].data_ptr(), o["mind"].data_ptr(),
                                     o["desc"].data_ptr(), None, self.d_T.data_ptr())
        # the frame: 1000 keypoints at the projections of local points that are not in a slot, descriptors with a few bits flipped
        rng = np.random.default_rng(5)
        free = np.setdiff1d(want_points, frame[frame >= 0])
        src = rng.choice(free, self.N, replace=False)
        kp = np.zeros(self.N, pkg.KP_DTYPE)
        kp["x"], kp["y"], kp["size"], kp["angle"], kp["octave"] = tables["uv"][src, 0], tables["uv"][src, 1], 31.0, 0.0, 0
        desc = tables["mpdesc"][src].copy()
        desc[:, 0] ^= rng.integers(0, 256, self.N, dtype=np.uint8)
        self.d_kp, self.d_de = t(kp.view(np.float32).reshape(self.N, 7)), t(desc)
        self.slot0 = t(np.where(frame >= 0, 0, -1).astype(np.int32))
        self.d_slot, self.d_sobs = self.slot0.clone(), torch.zeros(self.N, dtype=torch.uint8, device="cuda")
        self.d_moq = torch.zeros(self.cap, dtype=torch.int32, device="cuda")
        self.tr = [torch.zeros(self.cap, dtype=torch.uint8 if k == 0 else torch.int32 if k == 6 else torch.float32, device="cuda") for k in range(7)]
        self.ts = pkg.TrackStruct(*[x.data_ptr() for x in self.tr])
        self.fs = pkg.FrameStruct(self.N, self.d_kp.data_ptr(), self.d_de.data_ptr(), None, *BOUNDS)
        self.sf = np.array([1.2 ** i for i in range(8)], np.float32)
        self.d_nm = torch.zeros(1, dtype=torch.int32, device="cuda")

    def local_map(self, sync=True):
        r = self.d_res.data_ptr()
        self.m.UpdateLocalMapDevice(self.g, self.N, self.d_fp.data_ptr(), True, K - 1, K + 24, self.cap, self.d_lkf.data_ptr(), r, r + 4, r + 8,
                                    self.d_sb.data_ptr(), self.d_lp.data_ptr(), r + 12)
        if sync:
            self.torch.cuda.synchronize()

    def chain(self):
        r = self.d_res.data_ptr()
        self.d_slot.copy_(self.slot0)
        self.local_map(sync=False)
        self.m.GatherLocalMapDevice(self.P, self.N, self.d_fp.data_ptr(), self.d_lp.data_ptr(), r + 12, self.cap, self.d_bad.data_ptr(), self.tab["Xw"].data_ptr(),
                                    self.tab["normal"].data_ptr(), self.tab["max_dist"].data_ptr(), self.tab["min_dist"].data_ptr(),
                                    self.tab["mpdesc"].data_ptr(), None, self.ms, r + 16)
        self.m.search_local_points_batch_device(self.fs, self.N, None, 1, self.ms, self.cap, r + 16, 1, 1, self.sf, math.log(1.2), 0, CAM, 3.0,
                                                self.d_slot.data_ptr(), self.d_sobs.data_ptr(), self.d_moq.data_ptr(), self.ts, self.d_nm.data_ptr())
        self.torch.cuda.synchronize()

    def result(self):
        res = self.d_res.cpu().numpy()
        return dict(local_kf=self.d_lkf.cpu().numpy()[:res[0]], kf_max=int(res[1]), max_votes=int(res[2]), slot_bad=self.d_sb.cpu().numpy(),
                    local_point=self.d_lp.cpu().numpy()[:res[3]]), int(res[4]), int(self.d_nm.cpu().numpy()[0])


def timed(forms, rounds, calls, warmup):
    for _, fn in forms:
        for _ in range(warmup):
            fn()
    means = [[] for _ in forms]
    for _ in range(rounds):
        for r, (_, fn) in enumerate(forms):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            means[r].append((time.perf_counter() - t0) * 1e3 / calls)
    return means


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0, help="only make this many runs of the chain and of the T = 150 call (for a kernel trace)")
    ap.add_argument("--vote-form", type=int, default=0, help="with --kernels: 0 the LDS table, 1 one global atomic per vote")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_map_bench.txt"))
    a = ap.parse_args()
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    graph, frame, tables = make_map()
    want = pkg.update_local_map_host(graph, frame, True, K - 1)
    rng = np.random.default_rng(3)
    targets = {40: np.sort(rng.choice(np.arange(200, 300), 40, replace=False)), 150: np.sort(rng.choice(np.arange(100, 400), 150, replace=False))}
    want_conn = {T: pkg.update_connections_host(graph, t) for T, t in targets.items()}
    same = lambda x, y, keys: all(np.array_equal(x[k], y[k]) for k in keys)
    LKEYS, CKEYS = ("local_kf", "kf_max", "max_votes", "slot_bad", "local_point"), ("conn_kf", "conn_w", "ord_kf", "ord_w", "kf_max", "nmax")
    handles = {}
    for form, label in ((0, "LDS table"), (1, "one global atomic per vote")):
        os.environ["ORBM_VOTE_FORM"] = str(form)
        handles[label] = pkg.ORBmatcher(0.8, False)
    os.environ.pop("ORBM_VOTE_FORM")
    results, lines, ok = [], [], True
    E, P = len(graph["obs_kf"]), len(graph["pt_bad"])
    lines.append("SYNTHETIC map: %d keyframes x %d rows, %d map points, %d observations (%.1f per point); frame of %d slots, %d matched; local map of "
                 "%d keyframes and %d points" % (K, ROWS, P, E, E / P, SLOTS, MATCHED, len(want["local_kf"]), len(want["local_point"])))
    for label, m in handles.items():
        ch = Chain(pkg, m, graph, frame, tables, want["local_point"])
        if a.kernels and label != ("LDS table", "one global atomic per vote")[a.vote_form]:
            continue
        up = lambda m=m: m.UpdateLocalMap(graph, frame, True, K - 1, cap_kf=K + 24, cap_pts=65536)
        c40 = lambda m=m: m.UpdateConnections(graph, targets[40], cap=40 * 64)
        c150 = lambda m=m: m.UpdateConnections(graph, targets[150], cap=150 * 64)
        if a.kernels:
            for _ in range(a.kernels):
                ch.chain()
                c150()
        else:
            forms = (("local map, upload form", up), ("local map, device tables", ch.local_map), ("local map -> search", ch.chain),
                     ("connections T = 40", c40), ("connections T = 150", c150))
            means = timed(forms, a.rounds, a.calls, a.warmup)
            lines.append("k_covis_vote: %s" % label)
            for (name, _), v in zip(forms, means):
                results.append(dict(vote=label, form=name, median=statistics.median(v), min=min(v), max=max(v), rounds=v))
                lines.append("  %-28s median %.4f ms per call (range %.4f-%.4f, %d rounds x %d calls)" % (name + ":", statistics.median(v), min(v), max(v), a.rounds, a.calls))
        ch.chain()
        got, map_n, nmatches = ch.result()
        good = same(got, want, LKEYS) and same(up(), want, LKEYS) and map_n == len(want["local_point"])
        good = good and all(same(g, w, CKEYS) for g, w in zip(c40(), want_conn[40])) and all(same(g, w, CKEYS) for g, w in zip(c150(), want_conn[150]))
        ok = ok and good
        lines.append("  outputs against the host forms: %s; the chain's search matched %d of %d keypoints" % ("identical" if good else "DIFFERENT", nmatches, SLOTS))
    for m in handles.values():
        m.close()
    if a.kernels:
        print("\n".join(lines))
        return 0 if ok else 1
    lines.append("no gain is claimed: nothing on the parent or in the reference build is measured against these times; device tables against upload "
                 "form is a statement about residency only")
    lines.append("not measured: flattening inside ORB-SLAM3, how often local mapping dirties the tables, real observation counts")
    lines.append(json.dumps(dict(cases=results)))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
