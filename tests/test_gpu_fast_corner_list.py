"""k_fast's NMS over the per-wavefront corner list (pixels with S > t, in raster order) against the CPU oracle: a cell with
one corner fewer than the list holds, exactly as many, and one more (the full-cell walk), neighbours across a cell boundary
inside a 2 x 2 group, and a second detection that follows a first one whose corners all tied."""
import os
import re

import numpy as np
import pytest

from test_gpu_fast_cells import check_levels

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CIRCLE = [(3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1),
          (-3, 0), (-3, -1), (-2, -2), (-1, -3), (0, -3), (1, -3), (2, -2), (3, -1)]
BG = 40


def fast_list_capacity():
    src = open(os.path.join(ROOT, "3_orb_slam3_selfnote_amd", "csrc", "orb_kernels.h")).read()
    return int(re.search(r"#define FAST_LIST (\d+)", src).group(1))


def score_plane(img):
    """Threshold-free FAST score S (corner at t <=> S > t) of every pixel at least 3 from the border, 0 elsewhere."""
    a = img.astype(np.int16)
    h, w = a.shape
    v = a[3:h - 3, 3:w - 3]
    ring = np.stack([a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dy, dx in CIRCLE])
    best = np.full(v.shape, -255, np.int16)
    for sgn in (1, -1):
        d = sgn * (v[None] - ring)
        for k in range(16):
            best = np.maximum(best, d[[(k + j) & 15 for j in range(9)]].min(axis=0))
    S = np.zeros(a.shape, np.int16)
    S[3:h - 3, 3:w - 3] = np.clip(best, 0, 255)
    return S


@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_list_capacity_edge(pkg, oracle, extra):
    """A 91 x 91 frame: level 0 is one cell with a 53 x 53 interior, rows and columns [19, 72).  Bright dots on a lattice
    (even rows, every other column, shifted by one every second row) are corners of score 160 with no other dot on their
    circle or among their 8 neighbours; the first FAST_LIST + extra of the interior's, in raster order, are kept."""
    cap = fast_list_capacity()
    n = cap + extra
    ys, xs = np.mgrid[0:91, 0:91]
    dots = (ys % 2 == 0) & (xs % 2 == (ys // 2) % 2)
    inside = (ys >= 19) & (ys < 72) & (xs >= 19) & (xs < 72)
    order = np.flatnonzero((dots & inside).ravel())
    assert len(order) > n
    dots.ravel()[order[n:]] = False
    img = np.full((91, 91), BG, np.uint8)
    img[dots] = 200
    S = score_plane(img)
    assert (S[19:72, 19:72] > 20).sum() == n
    cfg = dict(nfeatures=1000, scaleFactor=1.2, nlevels=3, iniThFAST=20, minThFAST=7)
    _, cands = check_levels(pkg, oracle, img, cfg)
    assert len(cands[0]) == n


def test_neighbour_across_cell_boundary(pkg, oracle):
    """Pairs of adjacent dots of different brightness across the boundaries of level-0 cells inside a 2 x 2 group (cells
    30 x 32 px; interiors start at column 19 + 30 j and row 19 + 32 i): on the cell's own Mat the neighbour across the boundary
    is 0, so both dots of every pair are kept."""
    img = np.full((480, 752), BG, np.uint8)
    pairs = []
    for gi, gj in [(0, 0), (2, 4), (4, 10)]:                # groups of cells (2 gi .. 2 gi + 1, 2 gj .. 2 gj + 1)
        xb, yb = 19 + 30 * (2 * gj + 1), 19 + 32 * (2 * gi + 1)   # first column / row of the right / lower cells
        pairs += [((yb - 20, xb - 1), (yb - 20, xb)),    # horizontal, upper cells
                  ((yb + 10, xb), (yb + 10, xb - 1)),    # horizontal, lower cells, brighter on the left
                  ((yb - 1, xb - 15), (yb, xb - 15)),    # vertical, left cells
                  ((yb, xb + 12), (yb - 1, xb + 12)),    # vertical, right cells, brighter above
                  ((yb - 1, xb - 1), (yb, xb))]          # diagonal through the group's centre
    for (y0, x0), (y1, x1) in pairs:
        img[y0, x0], img[y1, x1] = 200, 230
    S = score_plane(img)
    assert (S > 20).sum() == 2 * len(pairs)
    _, cands = check_levels(pkg, oracle, img)
    assert len(cands[0]) == 2 * len(pairs)


def test_second_detection_after_tied_corners(pkg, oracle):
    """Cell (0, 0) of level 0 holds only horizontal pairs of equally bright pixels: corners at iniThFAST that suppress each
    other, so the first detection keeps nothing with a non-empty corner list.  Faint dots (score 15) are corners only at
    minThFAST and are what the second detection keeps.  Cell (0, 2) holds tied pairs only and stays empty."""
    img = np.full((480, 752), BG, np.uint8)
    for y in (21, 29, 37, 45):
        for x in (21, 33, 41):
            img[y, x:x + 2] = 200
            img[y, x + 60:x + 62] = 200
    for y in (25, 33, 41, 49):
        for x in (25, 37, 45):
            img[y, x] = BG + 15
    S = score_plane(img)
    cell = S[19:51, 19:49]
    assert (cell > 20).sum() == 24 and (cell == 15).sum() == 12
    _, cands = check_levels(pkg, oracle, img)
    assert len(cands[0]) == 12
