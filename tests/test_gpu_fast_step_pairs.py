"""k_fast with two row steps per loop trip: cells whose number of row steps is odd (the pair's second step is masked), rows of 32
and of 64 lanes, odd cell heights, the survivor queue wrapped many times by dense noise (drained behind the pair's first step and
behind its second), cells with more corners than the corner list holds (the full-cell walk of pass 3, also two steps per trip),
cells whose queue is drained by the tail call alone, and cells that need the minThFAST detection.

Every case is one batch call of 3 levels x 11 distinct frames (nlevels * nframes > 32: k_resize per level, k_octree<256>,
k_describe<8>) and compares every frame's outputs and stage taps - FAST candidates of every level among them - byte for byte with
the oracle (test_gpu_batch_layouts.check_frames).  The cell shapes and corner counts a case is meant to reach are computed on the
CPU, from the cell grid of ORBextractor.cc:771-803 and the segment test itself, and asserted."""
import numpy as np
import pytest

from extract_forms import level_sizes
from test_gpu_batch_layouts import check_frames, pack, run_batch

FAST_LIST = 384   # orb_kernels.h: corners of a cell above this take the full-cell walk
NFRAMES, NLEVELS, SF = 11, 3, 1.2

# (name, H, W, iniThFAST, minThFAST)
CASES = [
    ("126x91", 91, 126, 20, 7),
    ("127x101", 101, 127, 20, 7),
    ("140x110 low thresholds", 110, 140, 7, 3),
    ("100x76 low thresholds", 76, 100, 7, 3),
]

CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]

_frames = {}


def cfg_of(ini, mn):
    return dict(nfeatures=300, scaleFactor=SF, nlevels=NLEVELS, iniThFAST=ini, minThFAST=mn)


def cells(h, w):
    """Interiors (x, y, width, height) of the valid FAST cells of an h x w level (ORBextractor.cc:771-803)."""
    width, height = w - 32, h - 32
    nCols, nRows = width // 30, height // 30
    if nCols < 1 or nRows < 1:
        return []
    wCell, hCell = -(-width // nCols), -(-height // nRows)
    maxBX, maxBY = w - 16, h - 16
    out = []
    for ci in range(nRows):
        for cj in range(nCols):
            iniX, iniY = 16 + cj * wCell, 16 + ci * hCell
            tw = min(iniX + wCell + 6, maxBX) - iniX
            th = min(iniY + hCell + 6, maxBY) - iniY
            if not (iniX >= maxBX - 6 or iniY >= maxBY - 3 or tw - 6 <= 0 or th - 6 <= 0):
                out.append((iniX + 3, iniY + 3, tw - 6, th - 6))
    return out


def corner_mask(img, t):
    """Pixels with 9 contiguous circle pixels all brighter than v + t or all darker than v - t."""
    h, w = img.shape
    v = img[3:h - 3, 3:w - 3].astype(np.int32)
    ring = np.stack([img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx].astype(np.int32) for dx, dy in CIRCLE])
    out = np.zeros(v.shape, bool)
    for m in (ring > v + t, ring < v - t):
        mm = np.concatenate([m, m[:8]])
        for k in range(16):
            out |= mm[k:k + 9].all(axis=0)
    full = np.zeros((h, w), bool)
    full[3:h - 3, 3:w - 3] = out
    return full


def corners_per_cell(img, t):
    m = corner_mask(img, t)
    return [int(m[y:y + ch, x:x + cw].sum()) for x, y, cw, ch in cells(*img.shape)]


def frames_of(H, W, ini):
    """Eleven distinct frames.  0, 5-7: uniform noise; 1: binary noise (nearly every pixel passes the compass pre-test); 2: a few
    isolated dots on a flat ground; 3: noise compressed to less than iniThFAST peak to peak (corners at minThFAST only); 4: flat (no
    corner in either detection); 8: noise, compressed in the right half; 9: dots every 4 pixels; 10: blocks of 4 x 4 under a ramp."""
    key = (H, W, ini)
    if key in _frames:
        return _frames[key]
    rng = np.random.default_rng([H, W, ini])
    noise = lambda: rng.integers(0, 256, (H, W), dtype=np.uint8)
    squeeze = lambda f: np.clip(128.0 + (f.astype(np.float32) - 128.0) * (0.45 * ini / 128.0), 0, 255).astype(np.uint8)
    out = [noise(), (rng.integers(0, 2, (H, W), dtype=np.uint8) * 255).astype(np.uint8)]
    dots = np.full((H, W), 90, np.uint8)
    ys, xs = np.meshgrid(np.arange(20, H - 19, 13), np.arange(21, W - 19, 17), indexing="ij")
    dots[ys, xs] = 200
    out.append(dots)
    out.append(squeeze(noise()))
    out.append(np.full((H, W), 77, np.uint8))
    out += [noise(), noise(), noise()]
    half = noise()
    half[:, W // 2:] = squeeze(half[:, W // 2:])
    out.append(half)
    grid = np.full((H, W), 40, np.uint8)
    grid[1::4, 2::4] = 230
    out.append(grid)
    b = rng.integers(0, 200, ((H + 3) // 4, (W + 3) // 4)).repeat(4, axis=0).repeat(4, axis=1)[:H, :W]
    out.append((b + (np.arange(W)[None, :] * 55 // (W - 1))).astype(np.uint8))
    _frames[key] = [np.ascontiguousarray(f) for f in out]
    return _frames[key]


def shapes(H, W):
    """(lanes per row, steps, cell height) of every cell of every level: rows of 32 lanes take two cell rows per step."""
    out = set()
    for h, w in level_sizes(H, W, SF, NLEVELS):
        for _, _, cw, ch in cells(h, w):
            out.add((32, (ch + 1) // 2, ch) if cw <= 32 else (64, ch, ch))
    return out


def test_cases_reach_every_shape():
    """No GPU: the cell shapes of the cases, and the corner counts of their level-0 frames."""
    all_shapes = set()
    for _, H, W, ini, mn in CASES:
        all_shapes |= shapes(H, W)
    assert any(l == 64 and ch % 2 == 1 for l, s, ch in all_shapes)               # 64-lane rows, odd height = odd number of steps
    assert any(l == 64 and ch % 2 == 0 for l, s, ch in all_shapes)
    assert any(l == 32 and ch % 2 == 1 and s % 2 == 1 for l, s, ch in all_shapes)   # 32-lane rows: last step half empty, odd number of steps
    assert any(l == 32 and ch % 2 == 1 and s % 2 == 0 for l, s, ch in all_shapes)
    assert any(l == 32 and ch % 2 == 0 and s % 2 == 1 for l, s, ch in all_shapes)
    walk32 = walk64 = False
    for _, H, W, ini, mn in CASES:
        fr = frames_of(H, W, ini)
        lanes = [32 if cw <= 32 else 64 for _, _, cw, _ in cells(H, W)]
        for f in (fr[0], fr[5], fr[6], fr[7]):
            for n, l in zip(corners_per_cell(f, ini), lanes):
                walk32 |= n > FAST_LIST and l == 32
                walk64 |= n > FAST_LIST and l == 64
        sparse = corners_per_cell(fr[2], ini)
        assert any(0 < n < 64 for n in sparse), sparse                        # fewer survivors than one scoring call: the tail call alone
        at_ini, at_min = corners_per_cell(fr[3], ini), corners_per_cell(fr[3], mn)
        assert any(a == 0 and b > 0 for a, b in zip(at_ini, at_min))             # a cell that needs the second detection
        assert not any(corners_per_cell(fr[4], mn))
    assert walk32 and walk64                                                     # the corner list overflows in both row forms


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_batch(pkg, oracle, capfd, monkeypatch, case):
    monkeypatch.setenv("ORBHIP_PRINT_EXTRACT_FORMS", "1")
    _, H, W, ini, mn = case
    cfg = cfg_of(ini, mn)
    frames = frames_of(H, W, ini)
    assert len(frames) == NFRAMES and NLEVELS * NFRAMES > 32
    stride = (W + 3) & ~3
    buf = pack(frames, 0, stride, H * stride, np.random.default_rng(9))
    e = pkg.ORBextractor(**cfg)
    try:
        outs, form = run_batch(e, capfd, buf, 0, H, W, stride, H * stride, NFRAMES)
        assert form["nframes"] == NFRAMES and form["pyramid"] == ("2p16", "2p16") and form["octree"][0] == 256, form
        check_frames(e, oracle, cfg, frames, outs)
    finally:
        e.close()
