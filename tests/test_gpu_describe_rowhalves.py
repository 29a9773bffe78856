"""k_describe's block form with the moments taken from aligned row halves of the disc window (lane = row and half: one 16-byte and
one 4-byte LDS read, v_alignbyte_b32 by (X - 15) & 3, signed dot products against per-row weights derived from umax), bit-exact against
the CPU oracle.

Twelve 320 x 480 frames at scale factor 2 with three levels and a FAST threshold of 100 (3 x 12 > 32: the block form), made from
one crafted frame - shifted right by 0..3 pixels, the same upside down, the same inverted:
  * single bright pixels on level 0 at eight consecutive X, so that the window's byte offset (X - 15) & 3 takes all four values,
    and Gaussian blobs that are corners on level 2 only, at level-2 X of all four residues;
  * bright pixels exactly 19 pixels from each border (the minimum: the window ends at the plane's edge);
  * a saturated white square with two black pixels inside: discs that are 255 nearly everywhere (the -128 offset of the signed dot
    products is at its largest and must cancel).
The batch is run from a dword-aligned buffer (every level by LDS-DMA and row halves) and from the same buffer one byte further on
(level 0 by the byte gather of c_disc, the levels above by row halves).  Keypoints - the angles among them - and descriptors must equal
the oracle's byte for byte."""
import numpy as np
import pytest

from test_gpu_batch_layouts import check_frames, pack
from test_gpu_describe_blocks import run

pytestmark = pytest.mark.gpu

H, W = 320, 480
CFG = dict(nfeatures=400, scaleFactor=2.0, nlevels=3, iniThFAST=100, minThFAST=100)
BORDER = [(19, 19), (W - 20, 19), (19, H - 20), (W - 20, H - 20)]
BLOB_X2 = (22, 33, 44, 55)


@pytest.fixture(autouse=True)
def print_forms(monkeypatch):
    monkeypatch.setenv("ORBHIP_PRINT_EXTRACT_FORMS", "1")


def crafted():
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W), np.float64)
    for x2 in BLOB_X2:                                   # corners on level 2 only, at (x2, 21) there
        img += 200.0 * np.exp(-((xx - (4 * x2 + 1.5)) ** 2 + (yy - (4 * 21 + 1.5)) ** 2) / 72.0)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    for k in range(8):                                   # level 0: X = 40 + 13 k + k, residues 0, 2, 0, 2 .. and 1, 3 below
        img[40, 40 + 14 * k] = 255
        img[52, 41 + 14 * k] = 255
    for (x, y) in BORDER:
        img[y, x] = 255
    img[200:240, 60:100] = 255                           # the white square and its two black pixels
    img[218, 78] = 0
    img[222, 84] = 0
    return img


def all_frames():
    f = crafted()
    base = [f, np.ascontiguousarray(f[::-1]), 255 - f]
    return [np.ascontiguousarray(np.roll(b, k, axis=1)) for b in base for k in range(4)]


def test_frames_hold_what_they_claim(oracle):
    f = crafted()
    mono, kps, desc = oracle.OracleExtractor(**CFG).extract(f, (0, 1000))
    x = np.rint(kps["x"] / np.float32(2.0) ** kps["octave"]).astype(int)
    y = np.rint(kps["y"] / np.float32(2.0) ** kps["octave"]).astype(int)
    for l in (0, 2):
        assert {int(v) for v in (x[kps["octave"] == l] - 15) & 3} == {0, 1, 2, 3}, "level %d: window offsets" % l
    at0 = {(int(a), int(b)) for a, b, o in zip(x, y, kps["octave"]) if o == 0}
    assert set(BORDER) <= at0 and (78, 218) in at0 and (84, 222) in at0
    assert len({float(a) for a in kps["angle"]}) > 10
    # every frame of the batch has keypoints on level 0, and all but those shifted by two pixels (a blob centred between two
    # level-2 pixels ties with itself and is suppressed) on level 2
    on2 = 0
    for g in all_frames():
        _, k, _ = oracle.OracleExtractor(**CFG).extract(g, (0, 1000))
        assert (k["octave"] == 0).sum() >= 8
        on2 += int((k["octave"] == 2).sum() >= 2)
    assert on2 >= 9


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned: row halves", "base+1: level 0 gathers"])
def test_batch_equals_oracle(pkg, oracle, capfd, offset):
    frames = all_frames()
    n = len(frames)
    stride, fs = W, H * W
    e = pkg.ORBextractor(**CFG)
    try:
        outs, form, cnt = run(e, capfd, pack(frames, offset, stride, fs, np.random.default_rng(5)), offset, H, W, stride, fs, n, (0, 1000), guard=8)
        assert form > 1, "a batch takes the block form"
        check_frames(e, oracle, CFG, frames, outs, taps=False)
    finally:
        e.close()
