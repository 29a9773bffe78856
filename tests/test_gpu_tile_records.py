"""k_resize's row-tile records and k_blur's tile flags (orbx_configure), through the planes they produce.

Every case runs orbx_extract_batch_device in its batch form (nlevels * nframes > 32: one k_resize launch per level, never the chain
kernel), asserts that form through the library's ORBHIP_PRINT_EXTRACT_FORMS line, and compares orbx_download_level and
orbx_download_blurred_level of every frame and level byte for byte with the oracle's pyramid and gaussian_blur7.  The shapes are the
smallest that reach each path of the two kernels: interior and border blur tiles, the DMA admission limits, one-row and short last
row tiles, a last source row that is clamped, unaligned level-0 planes, 8-row tiles, the one-pass form, and a handle whose records
follow a change of geometry."""
import numpy as np
import pytest

from conftest import EUROC
from extract_forms import level_sizes, resize_forms
from test_gpu_batch_layouts import pack, run_batch

pytestmark = pytest.mark.gpu

_frames = {}
_planes = {}


@pytest.fixture(autouse=True)
def print_forms(monkeypatch):
    monkeypatch.setenv("ORBHIP_PRINT_EXTRACT_FORMS", "1")


def cfg_of(sf, nlevels):
    return dict(nfeatures=300, scaleFactor=sf, nlevels=nlevels, iniThFAST=20, minThFAST=7)


def frames_of(seed, n, H, W):
    """n distinct frames: noise, and noise in blocks of 4 x 4 under a ramp (smooth rows and columns next to hard edges)."""
    key = (seed, n, H, W)
    if key not in _frames:
        rng = np.random.default_rng([seed, n, H, W])
        out = []
        for k in range(n):
            if k % 2 == 0:
                f = rng.integers(0, 256, (H, W), dtype=np.uint8)
            else:
                b = rng.integers(0, 200, ((H + 3) // 4, (W + 3) // 4)).repeat(4, axis=0).repeat(4, axis=1)[:H, :W]
                f = (b + (np.arange(W)[None, :] * 55 // max(W - 1, 1))).astype(np.uint8)
            out.append(np.ascontiguousarray(f))
        _frames[key] = out
    return _frames[key]


def planes_of(oracle, cfg, img):
    """The oracle's pyramid and blurred levels of one image, computed once (they depend on the scale factor and the level count alone)."""
    key = (cfg["scaleFactor"], cfg["nlevels"], img.shape, img.tobytes())
    if key not in _planes:
        pyr = oracle.OracleExtractor(**cfg).pyramid(img)
        _planes[key] = (pyr, [oracle.gaussian_blur7(p) for p in pyr])
    return _planes[key]


def run_and_check(e, oracle, capfd, cfg, frames, offset=0, spad=0, aligned=True):
    H, W = frames[0].shape
    n = len(frames)
    assert cfg["nlevels"] * n > 32, "the case must take the batch form"
    stride = W + spad
    fs = H * stride
    buf = pack(frames, offset, stride, fs, np.random.default_rng(7))
    _, form = run_batch(e, capfd, buf, offset, H, W, stride, fs, n)
    want = resize_forms(H, W, cfg["scaleFactor"], cfg["nlevels"])
    assert form["nframes"] == n and form["pyramid"] == want and form["octree"][0] == 256, "form line %s" % (form,)
    if aligned:
        nal = sum(((offset + k * fs) | stride) % 4 == 0 for k in range(n))
        assert form["aligned0"] == nal, form
        assert form["blur0dma"] == (nal if W >= 160 and H >= 40 and W % 16 == 0 else 0), form
    else:
        assert form["aligned0"] == 0 and form["blur0dma"] == 0, form
    for k, img in enumerate(frames):
        pyr, blur = planes_of(oracle, cfg, img)
        for l in range(cfg["nlevels"]):
            assert np.array_equal(e.image_pyramid_level(l, frame=k), pyr[l]), "frame %d: pyramid level %d" % (k, l)
            assert np.array_equal(e.blurred_level(l, frame=k), blur[l]), "frame %d: blurred level %d" % (k, l)
    return form


# (name, H, W, scaleFactor, nlevels, nframes, level-0 offset, stride - W)
CASES = [
    # interior blur tiles and all four border kinds; five frames: xcd_map's tail (not a multiple of 8)
    ("euroc x5", 480, 752, 1.2, 8, 5, 0, 0),
    # widths that are no multiple of 16, levels under 160 x 40 (k_blur's byte-wise path), single-tile rows (both edges in one tile)
    ("203x157 x9", 157, 203, 1.2, 4, 9, 0, 1),
    # the DMA admission limits of k_blur as level 0; 40 rows give level 1 its 33 = 2 * 16 + 1: a last row tile of one row
    ("160x40", 40, 160, 1.2, 2, 17, 0, 0),
    ("159x40", 40, 159, 1.2, 2, 17, 0, 1),
    ("160x39", 39, 160, 1.2, 2, 17, 0, 0),
    ("159x39", 39, 159, 1.2, 2, 17, 0, 1),
    # level 1 of 81 = 5 * 16 + 1 rows, on a level 0 with interior rows of blur tiles
    ("176x97 rows 16k+1", 97, 176, 1.2, 3, 11, 0, 0),
    # scale 1.01: level 1 has level 0's 40 rows, so its last tile has 8 rows and its last row's lower source row is clamped to row 39
    ("sf1.01 clamped last row", 40, 176, 1.01, 3, 11, 0, 0),
    # unaligned level 0: the byte staging of k_resize, the byte-wise loop of k_blur
    ("base+1", 120, 320, 1.2, 8, 5, 1, 0),
    ("odd stride", 120, 320, 1.2, 8, 5, 0, 5),
    # 8-row tiles; the one-pass form (its y table now staged inside the branch)
    ("sf2.6 x11", 500, 700, 2.6, 3, 11, 0, 0),
    ("sf3.3 x17", 300, 450, 3.3, 2, 17, 0, 2),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_planes(pkg, oracle, capfd, case):
    name, H, W, sf, nlevels, n, off, spad = case
    cfg = cfg_of(sf, nlevels)
    e = pkg.ORBextractor(**cfg)
    try:
        form = run_and_check(e, oracle, capfd, cfg, frames_of(400, n, H, W), off, spad, aligned=(off | (W + spad)) % 4 == 0)
    finally:
        e.close()
    sizes = level_sizes(H, W, sf, nlevels)
    if name == "euroc x5":
        assert form["pyramid"] == ("2p16",) * 7
    if name in ("160x40", "176x97 rows 16k+1"):
        assert sizes[1][0] % 16 == 1 and form["pyramid"][0] == "2p16"
    if name == "sf1.01 clamped last row":
        assert sizes[1][0] == sizes[0][0] == 40 and form["pyramid"] == ("2p16", "2p16")
    if name == "sf2.6 x11":
        assert form["pyramid"] == ("2p8", "2p8")
    if name == "sf3.3 x17":
        assert form["pyramid"] == ("1p",)


def test_reconfigure(pkg, oracle, capfd):
    """One handle from 752 x 480 to 203 x 157 and back: the records follow the geometry."""
    e = pkg.ORBextractor(**EUROC)
    try:
        for H, W in ((480, 752), (157, 203), (480, 752)):
            run_and_check(e, oracle, capfd, EUROC, frames_of(400, 5, H, W), aligned=W % 4 == 0)
    finally:
        e.close()
