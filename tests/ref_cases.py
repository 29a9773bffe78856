"""Inputs shared by tests/test_ref_extractor.py (CPU) and tests/test_gpu_ref_extractor.py (GPU): the extractor configurations and
frames compared with the compiled reference extractor (oracle/_ref/libref_extractor.so), the domain on which the reference's
extractor is defined, and built DistributeOctTree inputs.  Not a test module."""
import numpy as np

# ---- the reference's domain ----------------------------------------------------------------------------------------------------
# DistributeOctTree (ORBextractor.cc:541-567) makes nIni = round(w / h) root nodes for a level whose detection rectangle is
# w x h = (lcols - 32) x (lrows - 32), and files every candidate under vpIniNodes[x / hX].  A level taller than twice its width has
# nIni = 0: vpIniNodes is empty, hX = w / 0 = inf, and the first candidate reads vpIniNodes[0] - a null pointer.  (It takes a
# candidate: a level without cells, w < 30 or h < 30, cannot have one.)  w < 1 or h < 1 divides by zero or makes nIni negative.
# So a geometry is inside the domain when every level satisfies the predicate below; outside it the reference is undefined, the
# oracle returns no keypoints for such a level and orbx_configure refuses the geometry.


def level_sizes(rows, cols, scaleFactor, nlevels):
    """(lrows, lcols) per level, ORBextractor.cc:413-429 and :1192-1193: float scale table, cvRound = half-even."""
    sf = [np.float32(1.0)]
    for _ in range(1, nlevels):
        sf.append(np.float32(np.float64(sf[-1]) * np.float64(np.float32(scaleFactor))))
    return [(int(np.rint(np.float32(rows) * (np.float32(1.0) / s))), int(np.rint(np.float32(cols) * (np.float32(1.0) / s)))) for s in sf]


def level_in_domain(lrows, lcols):
    w, h = lcols - 32, lrows - 32
    return w >= 1 and h >= 1 and (w < 30 or h < 30 or 2 * w >= h)


def in_reference_domain(rows, cols, scaleFactor, nlevels):
    return all(level_in_domain(r, c) for r, c in level_sizes(rows, cols, scaleFactor, nlevels))


# ---- whole-extractor cases -----------------------------------------------------------------------------------------------------
def cfg(nfeatures, scaleFactor, nlevels, ini, mn):
    return dict(nfeatures=nfeatures, scaleFactor=scaleFactor, nlevels=nlevels, iniThFAST=ini, minThFAST=mn)


# (rows, cols, configuration, lapping area)
CONFIGS = {
    "euroc": (480, 752, cfg(1000, 1.2, 8, 20, 7), (0, 1000)),
    "tumvi": (512, 512, cfg(1500, 1.2, 8, 20, 7), (0, 0)),
    "half": (240, 376, cfg(500, 1.2, 8, 20, 7), (100, 250)),
    "odd": (131, 173, cfg(300, 1.37, 5, 25, 5), (0, 1000)),
    "dense": (97, 160, cfg(2000, 1.1, 3, 12, 3), (40, 90)),
    "many": (480, 752, cfg(5000, 1.2, 8, 20, 7), (0, 1000)),
}


def noise(rows, cols, seed=7):
    return np.random.default_rng([seed, rows, cols]).integers(0, 256, (rows, cols), dtype=np.uint8)


def checkerboard(rows, cols, cell=6):
    """A periodic board: level 0 has no FAST corner at all (four quadrants meet in a point), the resized levels have a few response
    values repeated many times, so inside an octree node the first maximum decides."""
    y, x = np.mgrid[0:rows, 0:cols]
    return np.ascontiguousarray(np.where(((x // cell) + (y // cell)) & 1, 190, 60).astype(np.uint8))


def squares(rows, cols, cell=6):
    """Bright squares on a dark ground: every corner on level 0 has one and the same response."""
    y, x = np.mgrid[0:rows, 0:cols]
    return np.ascontiguousarray(np.where(((x // cell) & 1) & ((y // cell) & 1), 190, 60).astype(np.uint8))


def low_contrast(synth, rows, cols, seed=11):
    """A synthetic frame squeezed to a tenth of its range: iniThFAST finds nothing in most cells, so they fall back to minThFAST."""
    f = synth.make_frame(seed, rows, cols).astype(np.int32)
    return np.ascontiguousarray((116 + f // 10).astype(np.uint8))


def constant(rows, cols):
    return np.full((rows, cols), 128, np.uint8)


def special_frames(synth, rows, cols):
    return {"noise": noise(rows, cols), "checkerboard": checkerboard(rows, cols), "squares": squares(rows, cols),
            "low_contrast": low_contrast(synth, rows, cols),
            "constant": constant(rows, cols)}


# ---- built DistributeOctTree inputs ----------------------------------------------------------------------------------------------
def _xyr(xs, ys, rs):
    return np.ascontiguousarray(np.stack([np.asarray(xs), np.asarray(ys), np.asarray(rs)], axis=1).astype(np.float32)).reshape(-1, 3)


def _random_points(rng, n, W, H, x0=0, y0=0, x1=None, y1=None, distinct=True):
    x1, y1 = W if x1 is None else x1, H if y1 is None else y1
    if distinct:
        flat = rng.choice((x1 - x0) * (y1 - y0), size=n, replace=False)
        xs, ys = x0 + flat % (x1 - x0), y0 + flat // (x1 - x0)
    else:
        xs, ys = rng.integers(x0, x1, n), rng.integers(y0, y1, n)
    return _xyr(xs, ys, rng.integers(1, 200, n))


def _clusters(W, H, per_side, k):
    """per_side x per_side clusters of k points each, one per cell of a regular grid: after the even splits every node has k
    points, so the size ranking is one long tie."""
    xs, ys, rs = [], [], []
    cw, ch = W // per_side, H // per_side
    for j in range(per_side):
        for i in range(per_side):
            for t in range(k):
                xs.append(i * cw + cw // 2 - 3 + 2 * t)
                ys.append(j * ch + ch // 2 - 3 + (3 * t) % 7)
                rs.append(10 + ((i * 7 + j * 13 + t * 5) % 23))
    return _xyr(xs, ys, rs)


def octree_cases():
    """(name, xyr [n, 3] float32 with integer values, (minX, maxX, minY, maxY), N).  Coordinates are relative to (minX, minY)."""
    rng = np.random.default_rng(2024)
    sq = (16, 16 + 256, 16, 16 + 256)
    out = []
    # equal-sized nodes: N falls inside the round that splits 16 nodes of 5 points each, so the tie rule picks which are split
    for N in (18, 24, 31, 40):
        out.append(("tie_4x4x5_N%d" % N, _clusters(256, 256, 4, 5), sq, N))
    out.append(("tie_8x8x3_N80", _clusters(256, 256, 8, 3), sq, 80))
    out.append(("tie_wide_N30", _clusters(512, 256, 4, 4), (16, 16 + 512, 16, 16 + 256), 30))
    # N against n
    pts = _random_points(rng, 200, 256, 256)
    for N in (1, 50, 199, 200, 201, 5000):
        out.append(("random200_N%d" % N, pts, sq, N))
    out.append(("n0", np.zeros((0, 3), np.float32), sq, 100))
    out.append(("n1", _xyr([100], [37], [55]), sq, 100))
    out.append(("n1_N1", _xyr([0], [0], [1]), sq, 1))
    out.append(("n2_same_node", _xyr([3, 5], [3, 4], [9, 9]), sq, 100))
    # all points in one quadrant (three empty children at the first split), each quadrant once
    for name, (x0, y0) in (("ul", (0, 0)), ("ur", (128, 0)), ("bl", (0, 128)), ("br", (128, 128))):
        out.append(("quadrant_" + name, _random_points(rng, 120, 256, 256, x0, y0, x0 + 128, y0 + 128), sq, 60))
    # duplicated coordinates: nodes that no split separates (the size-unchanged exit) next to size-1 nodes (bNoMore)
    dup = np.concatenate([np.repeat(_random_points(rng, 12, 256, 256), 4, axis=0), _random_points(rng, 30, 256, 256)])
    dup[:, 2] = rng.integers(1, 50, len(dup))
    out.append(("duplicates_N500", dup, sq, 500))
    out.append(("duplicates_N20", dup, sq, 20))
    out.append(("all_same_point", _xyr([77] * 9, [130] * 9, [5, 9, 9, 2, 9, 1, 3, 9, 4]), sq, 50))
    out.append(("equal_responses", np.concatenate([_random_points(rng, 150, 256, 256)[:, :2], np.full((150, 1), 40, np.float32)], axis=1), sq, 40))
    # initial nodes: width / height rounding to 1, 2 and 3 (2.5 rounds away from zero), and uneven hX
    for W, H, nini in ((300, 240, 1), (359, 240, 1), (360, 240, 2), (344, 208, 2), (590, 240, 2), (600, 240, 3), (720, 208, 3), (208, 344, 1)):
        assert int(np.floor(np.float32(W) / np.float32(H) + np.float32(0.5))) == nini
        out.append(("roots%d_%dx%d" % (nini, W, H), _random_points(rng, 300, W, H), (16, 16 + W, 16, 16 + H), 100))
        out.append(("roots%d_%dx%d_right_edge" % (nini, W, H), _random_points(rng, 40, W, H, W - 3, 0), (16, 16 + W, 16, 16 + H), 25))
    # points exactly on the split lines of the first three rounds (x or y = 128, 64, 192, 32, 96, ...)
    lines = np.arange(32, 256, 32)
    gx, gy = np.meshgrid(lines, lines)
    on = _xyr(gx.ravel(), gy.ravel(), rng.integers(1, 99, gx.size))
    near = np.concatenate([on, _xyr(gx.ravel() - 1, gy.ravel(), rng.integers(1, 99, gx.size)), _xyr(gx.ravel(), gy.ravel() - 1, rng.integers(1, 99, gx.size))])
    for N in (20, 49, 120, 1000):
        out.append(("split_lines_N%d" % N, near, sq, N))
    out.append(("split_lines_odd_size", _xyr([64, 65, 66, 32, 33, 97, 98, 130], [50, 51, 25, 26, 75, 76, 100, 101], [5, 6, 7, 8, 9, 10, 11, 12]),
                (16, 16 + 131, 16, 16 + 101), 6))
    return out
