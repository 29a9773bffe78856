"""k_fast's 16-pixel score on shared 8-pixel runs (csrc/orb_fast_score.h) against the CPU oracle, on hand-placed rings.

Single-level 96 x 96 frames on a flat background: level 0 is one group of 2 x 2 cells (interiors start at 19 and 51), so one
workgroup of k_fast sees every ring.  One blob per (arc start, polarity) with an arc of exactly 9 pixels, the same with 8 (no
corner), blobs whose score is decided by d[k] and by d[k+9] (the two terms the pair step merges), a cell whose only corners lie
between minThFAST and iniThFAST (second detection), and a cell with more than 64 pre-test survivors (full-queue trip and tail
trip: the score is inlined once for each).  FAST candidates, per-level keypoints (x, y, response) and the final keypoints and
descriptors are compared with the oracle byte for byte, through orbx_extract and through orbx_extract_batch_device with 2 and with
40 frames."""
import numpy as np
import pytest

from test_gpu_batch_layouts import pack, run_batch
from test_gpu_fast_corner_list import BG, CIRCLE, score_plane

pytestmark = pytest.mark.gpu

H = W = 96
CFG = dict(nfeatures=1000, scaleFactor=1.2, nlevels=1, iniThFAST=20, minThFAST=7)
# blob centres: a 7 x 7 footprint every 9 pixels, 6 x 6 of them inside the detection interior [19, 77)
CENTRES = [(23 + 9 * i, 23 + 9 * j) for i in range(6) for j in range(6)]


def put_ring(img, cy, cx, margins, sgn):
    """Ring pixel k of the centre (cy, cx) = centre value + sgn * margins[k] (sgn +1: the centre is darker than a positive margin's
    pixel).  The centre keeps the background."""
    for k, (dy, dx) in enumerate(CIRCLE):
        img[cy + dy, cx + dx] = int(img[cy, cx]) + sgn * int(margins[k])


def arc_frames(n):
    """Two frames: arcs of n pixels at margin 60 + start (distinct responses), every start 0..15, ring brighter than the centre in
    the first frame's blobs 0..15 and darker in blobs 16..31; the second frame has the polarities the other way round and the
    arcs at margin 21 (just above iniThFAST) - for n = 9 - or 120."""
    frames, info = [], []
    for f in range(2):
        img = np.full((H, W), 128, np.uint8)
        for b in range(32):
            s, sgn = b % 16, (1 if (b < 16) == (f == 0) else -1)
            m = 60 + s if f == 0 else (21 if n == 9 else 120)
            margins = np.zeros(16, int)
            for j in range(n):
                margins[(s + j) % 16] = m
            cy, cx = CENTRES[b]
            put_ring(img, cy, cx, margins, sgn)
            info.append((f, cy, cx, m))
        frames.append(img)
    return frames, info


def pair_frames():
    """Two frames (ring brighter / darker): for every k the run d[k+1..k+8] at margin 50 with (d[k], d[k+9]) = (30, 10) - decided by
    d[k] - and (10, 30) - decided by d[k+9]: score 30 either way.  Blobs 32..35: both ends equal to the run (a 10-pixel arc, 50),
    both ends above the run (50), both below and equal (30), one end negative (30)."""
    frames, info = [], []
    for sgn in (1, -1):
        img = np.full((H, W), 128, np.uint8)
        cases = [(k, 30, 10, 30) for k in range(16)] + [(k, 10, 30, 30) for k in range(16)]
        cases += [(2, 50, 50, 50), (7, 70, 75, 50), (12, 30, 30, 30), (5, -20, 30, 30)]
        for b, (k, ek, ek9, want) in enumerate(cases):
            margins = np.zeros(16, int)
            for j in range(1, 9):
                margins[(k + j) % 16] = 50
            margins[k], margins[(k + 9) % 16] = ek, ek9
            cy, cx = CENTRES[b]
            put_ring(img, cy, cx, margins, sgn)
            info.append((len(frames), cy, cx, want))
        frames.append(img)
    return frames, info


def two_detection_frame():
    """Cell (0, 0) (interior rows and columns [19, 51)): faint dots of score 15 only, between minThFAST 7 and iniThFAST 20 - the
    first detection keeps nothing, the second keeps them.  Cell (1, 1) (interior [51, 77)): a lattice of bright dots (more than 64, fewer than 128),
    every one a pre-test survivor at iniThFAST - a full-queue trip of 64 and a tail trip.  Cells (0, 1) and (1, 0): one 9-pixel arc each."""
    img = np.full((H, W), BG, np.uint8)
    for y in range(22, 48, 6):
        for x in range(23, 48, 7):
            img[y, x] = BG + 15
    for y in range(52, 77, 2):
        for x in range(52 + (y // 2) % 2, 77, 4):
            img[y, x] = 200
    for cy, cx, s in ((30, 62, 3), (62, 30, 11)):
        margins = np.zeros(16, int)
        for j in range(9):
            margins[(s + j) % 16] = 90
        put_ring(img, cy, cx, margins, 1)
    return img


def all_frames():
    a9, i9 = arc_frames(9)
    a8, i8 = arc_frames(8)
    pf, ip = pair_frames()
    return dict(arc9=(a9, i9), arc8=(a8, i8), pair=(pf, ip), two=([two_detection_frame()], None))


_refs = {}


def reference(oracle, img):
    key = img.tobytes()
    if key not in _refs:
        o = oracle.OracleExtractor(**CFG)
        mono, kps, desc = o.extract(img, (0, 1000))
        cands = o.level_candidates(img)
        octs = oracle.distribute_octtree(cands, 16, W - 16, 16, H - 16, o.features_per_level[0])
        _refs[key] = dict(out=(mono, kps.tobytes(), desc.tobytes()), cands=cands, octs=octs)
    return _refs[key]


def in_cands(cands, cy, cx):
    """The candidate at image pixel (cy, cx), or None: candidates are in detection-rectangle coordinates (image - 16)."""
    hit = cands[(cands[:, 0] == cx - 16) & (cands[:, 1] == cy - 16)]
    return None if len(hit) == 0 else float(hit[0, 2])


def test_frames_hold_what_they_claim(oracle):
    """CPU only in effect (the oracle and a numpy score plane): the blobs have the scores the docstrings state, the 9-pixel arcs and
    the pair blobs are candidates with response S - 1, the 8-pixel arcs are not."""
    fr = all_frames()
    for name in ("arc9", "arc8", "pair"):
        frames, info = fr[name]
        planes = [score_plane(f) for f in frames]
        for f, cy, cx, m in info:
            got = in_cands(reference(oracle, frames[f])["cands"], cy, cx)
            if name == "arc8":
                assert planes[f][cy, cx] == 0 and got is None
            else:
                assert planes[f][cy, cx] == m and got == m - 1, (name, f, cy, cx, m, planes[f][cy, cx], got)
    img = fr["two"][0][0]
    S = score_plane(img)
    c00, c11 = S[19:51, 19:51], S[51:77, 51:77]
    assert c00.max() == 15 and (c00 == 15).sum() == 20
    cands = reference(oracle, img)["cands"]
    in00 = cands[(cands[:, 0] < 51 - 16) & (cands[:, 1] < 51 - 16)]
    assert len(in00) == 20 and (in00[:, 2] == 14).all()
    # pre-test survivors of cell (1, 1) at iniThFAST: at least its corners
    assert (c11 > 20).sum() > 64 and (c11 > 20).sum() < 128


def check_taps(e, oracle, img, frame):
    ref = reference(oracle, img)
    assert e.level_candidates(0, frame=frame).tobytes() == ref["cands"].tobytes(), "frame %d: FAST candidates" % frame
    assert e.level_keypoints(0, frame=frame).tobytes() == ref["octs"].tobytes(), "frame %d: level keypoints" % frame


@pytest.mark.parametrize("name", ["arc9", "arc8", "pair", "two"])
def test_single_frame(pkg, oracle, name):
    frames, _ = all_frames()[name]
    e = pkg.ORBextractor(**CFG)
    try:
        for img in frames:
            mono, kps, desc = e(img, None, (0, 1000))
            ref = reference(oracle, img)
            check_taps(e, oracle, img, 0)
            assert (mono, kps.tobytes(), desc.tobytes()) == ref["out"]
    finally:
        e.close()


@pytest.mark.parametrize("n", [2, 40])
def test_batch(pkg, oracle, capfd, monkeypatch, n):
    """The seven frames in turn: one call of 40 frames (7 does not divide 40, so the batch's last frames differ from its first), or
    four calls of 2 frames.  With one level, 2 frames take the few-frame ("wide") launch form - 1024-thread octree, k_describe<1> - and
    40 the batch form; the form line says which was taken."""
    monkeypatch.setenv("ORBHIP_PRINT_EXTRACT_FORMS", "1")
    fr = all_frames()
    distinct = fr["two"][0] + fr["pair"][0] + fr["arc9"][0] + fr["arc8"][0]
    calls = [[(3 * k) % 7 for k in range(40)]] if n == 40 else [[0, 1], [2, 3], [4, 5], [6, 0]]
    e = pkg.ORBextractor(**CFG)
    try:
        for order in calls:
            frames = [distinct[i] for i in order]
            outs, form = run_batch(e, capfd, pack(frames, 0, W, H * W), 0, H, W, W, H * W, n)
            assert form["nframes"] == n and form["pyramid"] == "none"
            assert form["octree"][0] == (1024 if n == 2 else 256), form   # 2 frames: the wide form; 40: the batch form
            for k, img in enumerate(frames):
                assert outs[k] == reference(oracle, img)["out"], "frame %d" % k
                check_taps(e, oracle, img, k)
    finally:
        e.close()
