#!/usr/bin/env python3
"""Frame::ComputeBoW / KeyFrame::ComputeBoW on the device (orbv_transform, orbv_transform_batch_device): what a call costs.

There is no path in the parent to compare with - the parent cannot compute a FeatureVector at all - so NO GAIN IS CLAIMED here.  The
host form orbv_transform_host is printed beside the device entries; it is new code too (csrc/orb_ref_voc.h in plain C++ with two
std::maps, written to state the reference and not to be fast) and is no yardstick.

The vocabulary is SYNTHETIC: the real ORBvoc.txt is not available (.MISSING_LARGE_BLOBS of the reference tree).  It has ORBvoc's shape,
k = 10, L = 6, 10^6 words, 1 111 111 nodes (35.6 MB of descriptors): every child is a copy of its parent with bits flipped (each bit
with probability 0.16 / 2^level), weights uniform in (0, 9), 1 % stop words, TF_IDF weighting, L1_NORM scoring.  The descriptors are the
extractor's, from synthetic frames.  The memory behaviour of the descent (levels 1-3 cached, a dependent miss per level below) follows
from the shape; which words are hit, how many features share a word, and so how large the BowVector is say NOTHING about real word
occupancy.

  per call   orbv_transform (host pointers: upload, two kernels, download, one synchronisation) on one frame of the EuRoC extractor
             setting (1000 features asked) and one of the TUM-VI setting (1500), and orbv_transform_host on the same frames
  batch      orbv_transform_batch_device on 256 resident frames (the 1500 setting's frame, each copy with 8 random bits flipped per
             descriptor so that the copies descend differently), synchronised after the call, with both descent kernels:
             form 0 = k_voc_descend (a 16-lane row per descriptor), form 1 = k_voc_descend_lane (a lane per descriptor)
--rounds rounds of --calls calls, the routes alternated inside a round; wall clock per call as the median and range of the rounds'
means.  Every route's result is compared with the host form's first (exit status 1 on a difference).

--kernels CALLS launches only the batch form, CALLS times per descent kernel: the run to put under
`rocprofv3 --kernel-trace --stats`, which then gives the device time of k_voc_descend, k_voc_descend_lane and k_voc_collect.

    python tools/bow_transform_bench.py [--rounds 5] [--calls 20] [--out profiles/bow_transform_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o bow --output-format csv -- python tools/bow_transform_bench.py --kernels 20
"""
import argparse
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

K, L = 10, 6
KEYS = ("word", "node", "bow_id", "fv_node_id", "fv_start", "fv_idx")


def make_tree(seed):
    rng = np.random.default_rng(seed)
    levels = [rng.integers(0, 256, (1, 32), dtype=np.uint8)]
    for lvl in range(L):
        par = np.repeat(levels[-1], K, axis=0)
        for lo in range(0, len(par), 1 << 16):                     # in slabs: the last level would need a gigabyte of randoms at once
            hi = min(lo + (1 << 16), len(par))
            par[lo:hi] ^= np.packbits(rng.random((hi - lo, 256), dtype=np.float32) < np.float32(0.16 / (1 << lvl)), axis=1)
        levels.append(par)
    desc = np.concatenate(levels)                                  # breadth first: the children of node i are 10 i + 1 .. 10 i + 10
    n = len(desc)
    parent = np.zeros(n, np.uint32)
    parent[1:] = (np.arange(1, n, dtype=np.int64) - 1) // K
    is_leaf = np.zeros(n, np.uint8)
    is_leaf[n - K ** L:] = 1
    weight = np.where(is_leaf == 1, rng.uniform(1e-3, 9.0, n), 0.0)
    weight[(is_leaf == 1) & (rng.random(n) < 0.01)] = 0.0
    return parent, is_leaf, desc, weight


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS) and np.array_equal(a["bow_val"].view(np.uint64), b["bow_val"].view(np.uint64))


def timed(fn, rounds, calls):
    """fn: dict name -> callable; the routes alternated inside a round.  Returns name -> list of per-round mean ms."""
    out = {k: [] for k in fn}
    for _ in range(rounds):
        for k, f in fn.items():
            f()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            out[k].append((time.perf_counter() - t0) * 1e3 / calls)
    return out


def stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)


def line(label, s, rounds, calls):
    return "  %-58s median %.4f ms per call (range %.4f-%.4f, %d rounds x %d calls)" % (label, s["median"], s["min"], s["max"], rounds, calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    synth = importlib.import_module("3_orb_slam3_selfnote_amd.synth")
    dev = torch.device("cuda", 0)
    parent, is_leaf, desc, weight = make_tree(1)
    voc = pkg.ORBVocabulary.from_nodes(K, L, 0, 0, parent, is_leaf, desc, weight, device=0)
    lines = ["synthetic vocabulary: k = %d, L = %d, %d nodes, %d words, %.1f MB of descriptors; says nothing about real word occupancy"
             % (K, L, voc.n_nodes, voc.n_words, desc.nbytes / 1e6)]
    frames = {}
    for name, nfeat, hw in (("1000 features asked (EuRoC setting, 752 x 480)", 1000, (480, 752)), ("1500 features asked (TUM-VI setting, 512 x 512)", 1500, (512, 512))):
        ex = pkg.ORBextractor(nfeat, 1.2, 8, 20, 7)
        _, _, d = ex(synth.make_frame(41 + nfeat, *hw), None, (0, 1000))
        frames[name] = np.ascontiguousarray(d)
    big = list(frames.values())[-1]
    B, cap = a.frames, len(big)
    rng = np.random.default_rng(2)
    batch = np.repeat(big[None], B, axis=0)
    for _ in range(8):
        bit = rng.integers(0, 256, (B, cap))
        np.bitwise_xor.at(batch.reshape(-1, 32), (np.arange(B * cap), (bit >> 3).reshape(-1)), (1 << (bit & 7)).astype(np.uint8).reshape(-1))
    d_desc = torch.from_numpy(batch).to(dev)
    d_n = torch.full((B,), cap, dtype=torch.int32, device=dev)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    o = dict(word=z((B, cap), torch.int32), node=z((B, cap), torch.int32), bow_id=z((B, cap), torch.int32), bow_val=z((B, cap), torch.float64),
             n_bow=z((B,), torch.int32), fv_node_id=z((B, cap), torch.int32), fv_start=z((B, cap + 1), torch.int32), fv_idx=z((B, cap), torch.int32),
             n_fv=z((B,), torch.int32))
    scratch = z((max(pkg.ORBVocabulary.batch_scratch_bytes(B, cap), 4),), torch.uint8)

    def run_batch(form):
        voc.transform_batch_device(d_desc.data_ptr(), B, cap, d_n.data_ptr(), 1, 4, o["bow_id"].data_ptr(), o["bow_val"].data_ptr(), o["n_bow"].data_ptr(),
                                   o["fv_node_id"].data_ptr(), o["fv_start"].data_ptr(), o["fv_idx"].data_ptr(), o["n_fv"].data_ptr(), scratch.data_ptr(),
                                   d_word=o["word"].data_ptr(), d_node=o["node"].data_ptr(), stream=0, descend_form=form)
        torch.cuda.synchronize()

    if a.kernels:
        for form in (0, 1):
            for _ in range(a.kernels):
                run_batch(form)
        print("launched the batch form %d times per descent kernel on %d frames of %d descriptors" % (a.kernels, B, cap))
        return 0
    ok, res = True, dict(vocabulary=dict(k=K, L=L, nodes=voc.n_nodes, words=voc.n_words), cases=[])
    for name, d in frames.items():
        want = voc.transform_host(d, 4)
        ok &= same(voc.transform(d, 4), want)
        t = timed({"device": lambda: voc.transform(d, 4), "host": lambda: voc.transform_host(d, 4)}, a.rounds, a.calls)
        sd, sh = stat(t["device"]), stat(t["host"])
        lines.append("%s: %d descriptors -> %d words, %d nodes at level 2" % (name, len(d), len(want["bow_id"]), len(want["fv_node_id"])))
        lines.append(line("orbv_transform (upload, 2 kernels, download, 1 sync):", sd, a.rounds, a.calls))
        lines.append(line("orbv_transform_host (new code, no yardstick):", sh, a.rounds, a.calls))
        res["cases"].append(dict(case=name, n=len(d), n_bow=len(want["bow_id"]), n_fv=len(want["fv_node_id"]), device_ms=sd, host_ms=sh))
    for form in (0, 1):
        run_batch(form)
        got = {k: v.cpu().numpy() for k, v in o.items()}
        for p in (0, B // 2, B - 1):
            want = voc.transform_host(batch[p], 4)
            nb, nf = int(got["n_bow"][p]), int(got["n_fv"][p])
            frame = dict(word=got["word"][p].view(np.uint32), node=got["node"][p].view(np.uint32), bow_id=got["bow_id"][p, :nb].view(np.uint32),
                         bow_val=got["bow_val"][p, :nb], fv_node_id=got["fv_node_id"][p, :nf].view(np.uint32), fv_start=got["fv_start"][p, :nf + 1],
                         fv_idx=got["fv_idx"][p, :int(got["fv_start"][p, nf])])
            ok &= same(frame, want)
    t = timed({"rows": lambda: run_batch(0), "lanes": lambda: run_batch(1)}, a.rounds, a.calls)
    sr, sl = stat(t["rows"]), stat(t["lanes"])
    lines.append("batch: %d resident frames of %d descriptors, synchronised after the call" % (B, cap))
    lines.append(line("form 0, k_voc_descend (16-lane row per descriptor):", sr, a.rounds, a.calls))
    lines.append(line("form 1, k_voc_descend_lane (a lane per descriptor):", sl, a.rounds, a.calls))
    lines.append("  per frame: %.4f ms (form 0), %.4f ms (form 1)" % (sr["median"] / B, sl["median"] / B))
    lines.append("results of every route against the host form: %s" % ("identical" if ok else "DIFFERENT"))
    res["batch"] = dict(frames=B, cap=cap, rows_ms=sr, lanes_ms=sl)
    res["identical"] = bool(ok)
    lines.append(json.dumps(res))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
