#!/usr/bin/env python3
"""KeyFrameDatabase on the device (orbd_query_reloc, orbd_query_place, orbd_score_batch_device): what a query costs.

There is no path in the parent to compare with - the parent cannot name a relocalisation or loop candidate at all - and the reference's
member is not built here, so NO GAIN IS CLAIMED and no threshold was set in advance.  The host form orbd_query_reloc_host is printed
beside the device entries; it is new code too (csrc/orb_ref_kfdb.h in plain C++, written to state the reference and not to be fast) and
is no yardstick.  The ONE comparison with a defined baseline is the resident batch call against a loop of single calls on the same
handle, reported under the project's rule (every round of the batch below every round of the loop, and a median gain of at least three
times the loop's own spread); it is a statement about batching, nothing more.

The database is SYNTHETIC: --keyframes keyframes of about 1000 words over 10^6 words.  The keyframes belong to "places" of 20 keyframes;
a place owns 3000 words, a keyframe draws 700 of them and 300 words anywhere, values positive and L1-normalised.  A query is one more
such vector of a random place.  This word occupancy is INVENTED and says nothing about real sequences: how many keyframes share a word
with a frame, how many pass the 0.8 gate and how long the common runs are depend on it.  Not measured: the call inside ORB-SLAM3, real
word occupancy, how often real neighbours carry stale scores.

  reloc      orbd_query_reloc: one upload, five kernels, one download, one synchronisation (a fresh query id per call)
  place      orbd_query_place with 15 connected keyframes
  host       orbd_query_reloc_host on the same queries (a few calls)
  loop       256 orbd_query_reloc calls, one after another
  batch      orbd_score_batch_device on the same 256 queries resident on the device, synchronised after the call
--rounds rounds, the routes alternated inside a round; wall clock per call as the median and range of the rounds' means.  The batch's
lists are compared with the single queries' first (exit status 1 on a difference).

--kernels CALLS runs only CALLS single queries of each form and CALLS batch calls: the run to put under
`rocprofv3 --kernel-trace --stats`, which then gives the device time of the k_kfdb_* kernels.

    python tools/kfdb_bench.py [--keyframes 500 4000] [--rounds 5] [--out profiles/kfdb_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -o kfdb --output-format csv -- python tools/kfdb_bench.py --kernels 20
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_WORDS = 1000000
NQ = 256


def make_vectors(rng, n, n_places):
    place_words = [rng.choice(N_WORDS, 3000, replace=False) for _ in range(n_places)]
    out = []
    for i in range(n):
        ids = np.unique(np.concatenate([rng.choice(place_words[i % n_places], 700, replace=False), rng.integers(0, N_WORDS, 300)])).astype(np.uint32)
        v = rng.random(len(ids)) + 0.05
        out.append((ids, (v / v.sum()).astype(np.float64)))
    return out


def timed(fn, calls):
    t0 = time.perf_counter()
    for c in range(calls):
        fn(c)
    return (time.perf_counter() - t0) * 1e3 / calls


def stat(xs):
    return "median %8.3f ms  range %8.3f .. %8.3f" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="+", default=[500, 4000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    dev = torch.device("cuda", 0)
    lines = ["KeyFrameDatabase on the device: synthetic database over 10^6 words (invented word occupancy; no gain claimed, see tools/kfdb_bench.py)"]
    ok = True
    for nkf in a.keyframes:
        rng = np.random.default_rng(7 + nkf)
        n_places = max(nkf // 20, 1)
        kfs = make_vectors(rng, nkf, n_places)
        queries = make_vectors(rng, NQ, n_places)
        db = pkg.KeyFrameDatabase(N_WORDS, capacity=max(nkf, 8), device=0)
        for i, b in enumerate(kfs):
            db.add(1000 + i, 1, b)
        connected = [1000 + i for i in range(15)]
        cap = max(len(q[0]) for q in queries)
        ids = np.zeros((NQ, cap), np.uint32)
        val = np.zeros((NQ, cap), np.float64)
        n = np.zeros(NQ, np.int32)
        for q, (i, v) in enumerate(queries):
            ids[q, :len(i)], val[q, :len(i)], n[q] = i, v, len(i)
        d_ids, d_val, d_n = torch.from_numpy(ids.view(np.int32)).to(dev), torch.from_numpy(val).to(dev), torch.from_numpy(n).to(dev)
        d_tag = torch.zeros((NQ, nkf), dtype=torch.int64, device=dev)
        d_score = torch.zeros((NQ, nkf), dtype=torch.float32, device=dev)
        d_cnt = torch.zeros((NQ, 4), dtype=torch.int32, device=dev)
        scratch = torch.zeros(db.batch_scratch_bytes(NQ) // 8 + 1, dtype=torch.int64, device=dev)
        next_id = [10]

        def fresh(k=1):
            next_id[0] += k
            return next_id[0] - k

        def batch():
            qid = fresh(NQ)
            db.score_batch_device(np.arange(qid, qid + NQ), d_ids.data_ptr(), d_val.data_ptr(), d_n.data_ptr(), cap, d_tag.data_ptr(),
                                  d_score.data_ptr(), nkf, d_cnt.data_ptr(), scratch.data_ptr(), stream=0)
            torch.cuda.synchronize()

        reloc = lambda c: db.query_reloc(fresh(), queries[c % NQ])
        place = lambda c: db.query_place(fresh(), connected, queries[c % NQ])
        host = lambda c: db.query_reloc_host(fresh(), queries[c % NQ])
        if a.kernels:
            timed(reloc, a.kernels)
            timed(place, a.kernels)
            for _ in range(a.kernels):
                batch()
            continue
        # the batch's lists against the single queries'
        batch()
        tag, score, cnt = d_tag.cpu().numpy().view(np.uint64), d_score.cpu().numpy(), d_cnt.cpu().numpy()
        scored = listed = 0
        for q in range(NQ):
            r = db.query_reloc(fresh(), queries[q])
            same = (np.array_equal(r["tags"], tag[q, :cnt[q, 2]]) and np.array_equal(r["scores"].view(np.uint32), score[q, :cnt[q, 2]].view(np.uint32))
                    and (r["max_common"], r["min_common"], len(r["tags"]), r["n_listed"]) == tuple(int(x) for x in cnt[q]))
            ok = ok and same
            scored += len(r["tags"])
            listed += r["n_listed"]
        for f in (reloc, place):
            timed(f, 5)       # warm-up
        batch()
        t = dict(reloc=[], place=[], host=[], loop=[], batch=[])
        for _ in range(a.rounds):
            t["reloc"].append(timed(reloc, a.calls))
            t["place"].append(timed(place, a.calls))
            t["host"].append(timed(host, 3))
            t["loop"].append(timed(reloc, NQ) * NQ)
            t["batch"].append(timed(lambda c: batch(), 3))
        lines.append("")
        lines.append("%d keyframes, %.0f words each; per query %.1f keyframes listed, %.1f scored; batch lists equal the single queries': %s"
                     % (nkf, np.mean([len(b[0]) for b in kfs]), listed / NQ, scored / NQ, ok))
        lines.append("  orbd_query_reloc        per call        %s" % stat(t["reloc"]))
        lines.append("  orbd_query_place        per call        %s" % stat(t["place"]))
        lines.append("  orbd_query_reloc_host   per call        %s   (new code, no yardstick)" % stat(t["host"]))
        lines.append("  loop of %d single calls per %d queries %s" % (NQ, NQ, stat(t["loop"])))
        lines.append("  orbd_score_batch_device per %d queries %s" % (NQ, stat(t["batch"])))
        gain = statistics.median(t["loop"]) - statistics.median(t["batch"])
        spread = max(t["loop"]) - min(t["loop"])
        lines.append("  batching: every batch round below every loop round: %s; median gain %.3f ms = %.1f x the loop's spread (%.3f ms); rule (>= 3 x): %s"
                     % (max(t["batch"]) < min(t["loop"]), gain, gain / spread if spread > 0 else float("inf"), spread,
                        max(t["batch"]) < min(t["loop"]) and gain >= 3 * spread))
    text = "\n".join(lines) + "\n"
    if not a.kernels:
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
