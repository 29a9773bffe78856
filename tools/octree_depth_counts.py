#!/usr/bin/env python3
"""Split depths and rounds of DistributeOctTree on the bench's own streams, CPU only:
    python tools/octree_depth_counts.py [frames per configuration, default 64] > profiles/octree_codes_depths.txt

The streams are bench.py's: synth.make_stream(1000 + g, 256, H, W) for EuRoC (480 x 752, 1000 features) and TUM-VI (512 x 512,
1500 features), the first frames of group g = 0.  Candidates come from the oracle, the rounds from tests/octree_codes_model.py (the
code form of k_octree), which reports per level the rounds, the deepest depth at which a node was split and whether a round had to
split a node of depth OCT_D (the hand-over to the per-key rounds).  OCT_D of orb_common.h = the deepest depth seen here + 1.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = [("euroc", 480, 752, 1000), ("tumvi", 512, 512, 1500)]
BATCH = 256   # bench.py's default batch: make_stream's frames depend on it


def main():
    nframes = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    synth = __import__("3_orb_slam3_selfnote_amd.synth", fromlist=["make_stream"])
    from oracle import oracle_py
    import octree_codes_model as MC
    oracle_py.build()
    print("OCT_D %d; %d frames per configuration of synth.make_stream(1000, %d, H, W)" % (MC.D_DEFAULT, nframes, BATCH))
    worst = -1
    for name, H, W, nfeatures in CONFIGS:
        o = oracle_py.OracleExtractor(nfeatures=nfeatures, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7)
        frames, _ = synth.make_stream(1000, BATCH, H, W)
        q = o.features_per_level
        nl = len(q)
        keys = np.zeros((nframes, nl), np.int64); rounds = keys.copy(); depth = keys.copy(); over = keys.copy()
        for f in range(nframes):
            for l, p in enumerate(o.pyramid(np.ascontiguousarray(frames[f]))):
                c = o.level_candidates(p)
                info = {}
                MC.distribute(c[:, 0].astype(np.int64), c[:, 1].astype(np.int64), c[:, 2].astype(np.int64), 16, p.shape[1] - 16, 16, p.shape[0] - 16,
                              q[l], info=info)
                keys[f, l], rounds[f, l], depth[f, l], over[f, l] = len(c), info["rounds"], info["depth"], info["handover"] is not None
        print("%s %dx%d nfeatures %d, N per level %s" % (name, H, W, nfeatures, list(q)))
        print("  level   keys min..max   rounds min..max   deepest split depth   levels handed over")
        for l in range(nl):
            print("  %5d   %5d..%-5d     %3d..%-3d           %3d                   %d of %d" %
                  (l, keys[:, l].min(), keys[:, l].max(), rounds[:, l].min(), rounds[:, l].max(), depth[:, l].max(), over[:, l].sum(), nframes))
        print("  deepest split depth %d, levels on the deeper-than-OCT_D path %d" % (depth.max(), over.sum()))
        worst = max(worst, int(depth.max()))
    print("deepest depth seen %d -> D = %d (OCT_D %d)" % (worst, worst + 1, MC.D_DEFAULT))
    return 0 if worst + 1 <= MC.D_DEFAULT else 1


if __name__ == "__main__":
    sys.exit(main())
