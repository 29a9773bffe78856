"""k_fast's score with the packed f16 three-input minimum / maximum (csrc/orb_fast_score.h: on the device fast_min3 / fast_max3 are
v_pk_minimum3_f16 / v_pk_maximum3_f16 on values biased by 2048) against the CPU oracle.

One 160 x 120 frame, 8 levels: saturated black and white blocks side by side (margins of +-255, the ends of the biased range),
one-pixel checkerboards of several amplitudes (every ring pixel differs from the centre, every arc is short), a ramp (small margins of
both signs around every pixel) and blocks on the ramp.  FAST candidates (position and response) and octree keypoints of every level,
every pyramid and blurred level, and the final counts, keypoints and descriptors must equal the oracle's."""
import numpy as np
import pytest

from conftest import EUROC
from test_gpu_batch_layouts import check_frames

pytestmark = pytest.mark.gpu

H, W = 120, 160


def frame():
    img = np.zeros((H, W), np.uint8)
    img[:, :] = (np.arange(W)[None, :] * 255 // (W - 1)).astype(np.uint8)           # the ramp (rows 80 .. 119 keep it)
    img[:44, :80] = 0                                                               # white blocks on black, black blocks on white:
    img[:44, 80:] = 255                                                             # 12 x 12 and 5 x 5, margins of +-255
    for by, n in ((18, 12), (36, 5)):
        for bx in range(18, 142, 2 * n + 3):
            img[by:by + n, bx:bx + n] = 255 - img[by, bx]
    yy, xx = np.mgrid[44:80, 0:W]
    for k, amp in enumerate((255, 60, 21, 8)):                                      # one-pixel checkerboards around 128, 40 columns each
        sel = xx // 40 == k
        img[44:80][sel] = np.where((yy + xx) % 2 == 0, 128 - (amp + 1) // 2, 128 + amp // 2)[sel]
    img[48:74, 66:96] = 0                                                           # a white block on black at the centre: its corners
    img[55:68, 74:89] = 255                                                         # stay inside the small levels' detection rectangles
    for by in range(84, 104, 14):                                                   # blocks on the ramp: corners of every margin
        for bx in range(20, 140, 14):
            img[by:by + 7, bx:bx + 7] = 255 if (by + bx) % 28 else 0
    return img


def test_frame_holds_what_it_claims(oracle):
    img = frame()
    assert (img == 0).sum() > 1000 and (img == 255).sum() > 1000
    o = oracle.OracleExtractor(**EUROC)
    cands = [o.level_candidates(p) for p in o.pyramid(img)]
    resp = np.concatenate([c[:, 2] for c in cands])
    assert len(resp) > 200 and resp.max() == 254 and resp.min() == 20 and len(np.unique(resp)) > 50   # S - 1, clamp to threshold
    assert sum(len(c) > 0 for c in cands) >= 4


def test_frame_equals_oracle(pkg, oracle):
    img = frame()
    e = pkg.ORBextractor(**EUROC)
    try:
        mono, kps, desc = e(img, None, (0, 1000))
        assert len(kps) > 100
        check_frames(e, oracle, EUROC, [img], [(mono, kps.tobytes(), desc.tobytes())])
    finally:
        e.close()
