"""Frames for k_octree's code form (tests/test_octree_codes_model.py on the CPU, tests/test_gpu_octree_codes.py on the GPU): each
case is (name, image, extractor settings) and is compared with the oracle key for key, in output order, on every level."""
import numpy as np

import ref_cases as R


def cfg(nfeatures, ini=20, mn=7, nlevels=8, sf=1.2):
    return dict(nfeatures=nfeatures, scaleFactor=sf, nlevels=nlevels, iniThFAST=ini, minThFAST=mn)


def flat(rows, cols, v=90):
    return np.full((rows, cols), v, np.uint8)


def blobs(rows, cols, at):
    """Isolated 3 x 3 bright dots on a flat ground: one FAST corner each where the dot survives the level's resize."""
    img = flat(rows, cols)
    for (y, x) in at:
        img[y - 1:y + 2, x - 1:x + 2] = 250
    return img


def patch(rows, cols, y0, x0, side=12, seed=5, dots=60):
    """A side x side noise patch on a flat image: all keys of a level within a few pixels of each other.  DistributeOctTree also
    stops when a round does not lengthen the list (ORBextractor.cc:667), which a lone patch inside one quadrant does at once, so
    isolated dots all over the image keep the list growing until the patch's own cell is small enough to split in every round."""
    img = flat(rows, cols)
    rng = np.random.default_rng(seed + 1)
    for _ in range(dots):
        y, x = int(rng.integers(20, rows - 20)), int(rng.integers(20, cols - 20))
        if abs(y - y0 - side // 2) > side + 8 or abs(x - x0 - side // 2) > side + 8:
            img[y - 1:y + 2, x - 1:x + 2] = 250
    img[y0:y0 + side, x0:x0 + side] = np.random.default_rng(seed).integers(0, 256, (side, side), dtype=np.uint8)
    return img


def half_textured(synth, rows, cols):
    """Texture in the right half only: the left root node of a two-root level stays empty."""
    img = synth.make_frame(77, rows, cols).copy()
    img[:, :cols // 2] = 90
    return img


_cases = None


def cases(synth):
    global _cases
    if _cases is None:
        H, W = 240, 376                       # rectangle 344 x 208: two roots, leaves of 5.4 x 6.5 pixels at depth 5
        _cases = [
            # empty and near-empty levels
            ("flat", flat(H, W), cfg(500)),
            ("one blob", blobs(H, W, [(100, 150)]), cfg(500)),
            ("two blobs", blobs(H, W, [(60, 80), (170, 300)]), cfg(500)),
            # deeper than OCT_D: N is far above the key count, so the rounds go on until every node holds one key
            ("patch inside a cell", patch(H, W, 41, 52), cfg(1000)),
            ("patch across the first split lines", patch(H, W, H // 2 - 6, W // 2 - 6), cfg(1000)),
            ("patch across a root's split lines", patch(H, W, H // 2 - 6, 16 + 86 - 6), cfg(1000)),
            # N per level 1 or 2: the first round is the careful one
            ("small N", synth.make_frame(71, H, W), cfg(9)),
            # N above the key count on every level
            ("N above the keys", synth.make_frame(72, 120, 160), cfg(5000)),
            # one, two and three root nodes, and an empty root
            ("one root", synth.make_frame(73, 200, 216), cfg(300)),
            ("two roots", synth.make_frame(74, H, W), cfg(500)),
            ("three roots", synth.make_frame(75, 160, 420), cfg(500)),
            ("empty root", half_textured(synth, H, W), cfg(500)),
            # equal responses: the first key in vKeys order wins a node
            ("checkerboard", R.checkerboard(H, W), cfg(500)),
            ("squares", R.squares(H, W), cfg(500)),
            # more keys on level 0 than the kernel holds in registers
            ("noise 752x480", R.noise(480, 752), cfg(1000)),
        ]
    return _cases


def level_reference(oracle, img, c):
    """Per level: the oracle's candidates, its DistributeOctTree output, the rectangle and N."""
    o = oracle.OracleExtractor(**c)
    pyr = o.pyramid(img)
    q = o.features_per_level
    out = []
    for l, p in enumerate(pyr):
        cand = o.level_candidates(p)
        rect = (16, p.shape[1] - 16, 16, p.shape[0] - 16)
        out.append(dict(cand=cand, rect=rect, N=q[l], oct=oracle.distribute_octtree(cand, rect[0], rect[1], rect[2], rect[3], q[l])))
    return out
