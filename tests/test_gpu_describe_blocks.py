"""k_describe's block form (a wavefront owns K consecutive keypoint slots of one frame), bit-exact against the CPU oracle.

The block form is what batch calls run (nlevels * nframes > 32); the library's ORBHIP_PRINT_EXTRACT_FORMS line names it ("describe K",
"describe 1" for the one-keypoint-per-wavefront form of few-frame calls) and every case asserts the form it was built to reach.
What the blocks add over one wavefront per keypoint: level counts that are not multiples of K (0, 1, K - 1, K, K + 1), an empty level
between two that are not, blocks that hold keypoints on both sides of a level's first slot, blocks that are empty altogether, lanes
that take the byte-gather path (unaligned level 0) next to DMA frames in one batch, lapping on and off.

The level counts come from crafted frames at scale factor 2 with three levels and one FAST threshold of 100: a single 255 pixel on
black is one corner on level 0 and none above (its 2 x 2 average, 64, is below the threshold); a Gaussian blob of sigma 6 centred on a
level-2 pixel is flat for a radius-3 circle on levels 0 and 1 and a corner on level 2.  The counts the oracle yields for them were
worked out on the CPU and are asserted, so no case can pass by being empty.

An output `cap` below a frame's total cannot be reached through the API: orbx_extract_batch_device refuses a cap below
orbx_configure()'s bound (which is at least every frame's total) before it launches anything, and orbx_extract always passes that
bound.  The test below checks the refusal and, at the smallest accepted cap, that nothing is written behind a frame's records."""
import re

import numpy as np
import pytest

from conftest import EUROC
from test_gpu_batch_layouts import check_frames, make_frames, pack

pytestmark = pytest.mark.gpu

H, W = 320, 480
CRAFT = dict(nfeatures=400, scaleFactor=2.0, nlevels=3, iniThFAST=100, minThFAST=100)
# blobs placed -> keypoints the oracle finds on level 2 (some blobs give two)
BLOB_COUNT = {0: 0, 1: 1, 5: 5, 6: 6, 7: 7, 13: 15, 14: 16, 15: 17, 29: 33, 32: 36}


def dots_blobs(nd, nb, extra=()):
    """nd single bright pixels (level 0 only), nb blobs (level 2 only), then `extra` bright pixels at the given (x, y)."""
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W), np.float64)
    for k in range(nb):
        cx, cy = 88 + 40 * (k % 8) + 1.5, 84 + 40 * (k // 8) + 1.5
        img += 200.0 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 72.0)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    for k in range(nd):
        img[30 + 12 * (k // 20), 30 + 22 * (k % 20)] = 255
    for (x, y) in extra:
        img[y, x] = 255
    return img


@pytest.fixture(autouse=True)
def print_forms(monkeypatch):
    monkeypatch.setenv("ORBHIP_PRINT_EXTRACT_FORMS", "1")


FORM = re.compile(r"orbhip: extract nframes (\d+) .* describe (\d+)")


def run(e, capfd, buf, offset, Hh, Ww, stride, frame_stride, n, lap, cap=None, guard=0):
    """One orbx_extract_batch_device call; per-frame (mono, kps bytes, desc bytes, count), the describe form and the raw outputs."""
    import torch
    bound = e.configure(Hh, Ww, n)
    cap = bound if cap is None else cap
    d_buf = torch.from_numpy(buf).cuda()
    d_kps = torch.full((n * cap + guard, 7), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_desc = torch.full((n * cap + guard, 32), 0xa5, dtype=torch.uint8, device="cuda")
    d_cnt = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
    capfd.readouterr()
    e.extract_batch_device(d_buf.data_ptr() + offset, Hh, Ww, stride, frame_stride, n, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(),
                           cap, lap, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    m = FORM.findall(capfd.readouterr().err)
    assert len(m) == 1 and int(m[0][0]) == n, m
    cnt, kps, desc = d_cnt.cpu().numpy(), d_kps.cpu().numpy(), d_desc.cpu().numpy()
    outs = []
    for k in range(n):
        c = int(cnt[k, 0])
        assert 0 <= c <= cap
        outs.append((int(cnt[k, 1]), kps[k * cap:k * cap + c].tobytes(), desc[k * cap:k * cap + c].tobytes()))
        # nothing behind the frame's records, up to the next frame's first (and the guard behind the last frame)
        assert (kps[k * cap + c:(k + 1) * cap] == 0x5a5a5a5a).all() and (desc[k * cap + c:(k + 1) * cap] == 0xa5).all(), "frame %d: write past its count" % k
    assert (kps[n * cap:] == 0x5a5a5a5a).all() and (desc[n * cap:] == 0xa5).all(), "write past the output arrays"
    e._keep = d_buf
    return outs, int(m[0][1]), cnt


def level_counts(oracle, cfg, img, lap):
    mono, kps, desc = oracle.OracleExtractor(**cfg).extract(img, lap)
    return [int((kps["octave"] == l).sum()) for l in range(cfg["nlevels"])], mono


# (dots, blobs) per frame: level counts (dots, 0, BLOB_COUNT[blobs]).  With K = 16: 0, 1, K - 1, K, K + 1 on level 0 and on level 2,
# 2 K + 1 / 2 K + 4, an all-empty frame, and level 1 empty between two levels that are not.  K = 8 is covered by 7, 8 (none: 9 = 8 + 1),
# and the same 15 / 16 / 17 as 2 K - 1, 2 K, 2 K + 1.
CRAFTED = [(0, 0), (1, 0), (15, 1), (16, 13), (17, 14), (16, 15), (0, 15), (33, 32), (0, 1), (1, 1), (7, 7), (9, 6), (8, 29), (33, 0)]


@pytest.mark.parametrize("lap", [(0, 0), (0, 1000), (150, 330)], ids=["lap off", "lap all", "lap 150-330"])
def test_level_counts(pkg, oracle, capfd, lap):
    """Counts around the block size on the first and the last level, an empty level between them, an all-empty frame; 14 frames, of
    which four are dword-aligned (odd frame stride), so DMA lanes and byte-gather frames share one launch.  Lapping off, over the
    whole width, and a band with keypoints on both sides (records filled from both ends of the frame's range)."""
    frames = [dots_blobs(nd, nb) for nd, nb in CRAFTED]
    for (nd, nb), f in zip(CRAFTED, frames):
        lc, mono = level_counts(oracle, CRAFT, f, lap)
        assert lc == [nd, 0, BLOB_COUNT[nb]], "the oracle's level counts for %d dots, %d blobs: %s" % (nd, nb, lc)
        if lap == (150, 330) and nd >= 15 and nb >= 13:
            assert 0 < mono < sum(lc), "keypoints on both sides of the lapping band"
    n = len(frames)
    stride, fs = W + 4, H * (W + 4) + 1
    e = pkg.ORBextractor(**CRAFT)
    try:
        outs, form, cnt = run(e, capfd, pack(frames, 0, stride, fs, np.random.default_rng(77)), 0, H, W, stride, fs, n, lap, guard=8)
        assert form > 1, "a batch takes the block form"
        assert [int(c) for c in cnt[:, 0]] == [nd + BLOB_COUNT[nb] for nd, nb in CRAFTED]
        check_frames(e, oracle, CRAFT, frames, outs, lap=lap, taps=False)
    finally:
        e.close()


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_wide_calls_keep_one_keypoint_per_wavefront(pkg, oracle, capfd, n):
    """1-4 frames (nlevels * nframes <= 32): the K = 1 form, same outputs."""
    pick = [(17, 14), (0, 0), (16, 15), (1, 1)][:n]
    frames = [dots_blobs(nd, nb) for nd, nb in pick]
    stride, fs = W, H * W + 2
    e = pkg.ORBextractor(**CRAFT)
    try:
        outs, form, cnt = run(e, capfd, pack(frames, 0, stride, fs), 0, H, W, stride, fs, n, (150, 330))
        assert form == 1
        assert [int(c) for c in cnt[:, 0]] == [nd + BLOB_COUNT[nb] for nd, nb in pick]
        check_frames(e, oracle, CRAFT, frames, outs, lap=(150, 330), taps=False)
    finally:
        e.close()


def test_borders(pkg, oracle, capfd):
    """Keypoints exactly 19 px from each border of level 0 (the disc and patch windows end 4 resp. 1 px inside the plane) and in the
    bottom-right corner of the smallest level, 19 px from its right and bottom edges."""
    corners = [(19, 19), (W - 20, 19), (19, H - 20), (W - 20, H - 20)]
    yy, xx = np.mgrid[0:H, 0:W]
    blob = 200.0 * np.exp(-((xx - (4 * (W // 4 - 20) + 1.5)) ** 2 + (yy - (4 * (H // 4 - 20) + 1.5)) ** 2) / 72.0)
    f = np.maximum(dots_blobs(3, 2, corners), np.clip(np.rint(blob), 0, 255).astype(np.uint8))
    mono, kps, desc = oracle.OracleExtractor(**CRAFT).extract(f, (0, 1000))
    at = {(float(k["x"]), float(k["y"]), int(k["octave"])) for k in kps}
    for (x, y) in corners:
        assert (float(x), float(y), 0) in at
    assert (4.0 * (W // 4 - 20), 4.0 * (H // 4 - 20), 2) in at
    frames = [f] + [dots_blobs(nd, nb, corners) for nd, nb in CRAFTED[:11]]
    n = len(frames)
    stride, fs = W, H * W   # tight: the last frame's last row ends the buffer
    e = pkg.ORBextractor(**CRAFT)
    try:
        outs, form, cnt = run(e, capfd, pack(frames, 0, stride, fs), 0, H, W, stride, fs, n, (0, 1000))
        assert form > 1
        check_frames(e, oracle, CRAFT, frames, outs, taps=False)
    finally:
        e.close()


def kp_bases(oracle, cfg, Hh, Ww):
    """First slot and capacity of every level in a frame's keypoint array, as orbx_configure lays them out: capacity
    max(N + 3, 4 * nIni) + 1 with N the level's quota and nIni = round(width / height) of its detection rectangle."""
    o = oracle.OracleExtractor(**cfg)
    pyr = o.pyramid(np.zeros((Hh, Ww), np.uint8))
    base, out = 0, []
    for l, p in enumerate(pyr):
        h, w = p.shape
        nini = int(np.floor((w - 32) / float(h - 32) + 0.5))
        cap = max(int(o.features_per_level[l]) + 3, 4 * nini) + 1
        out.append((base, cap))
        base += cap
    return out


@pytest.mark.parametrize("case", [("euroc x40", 160, 256, EUROC, 40),
                                  ("16 levels x3", 240, 376, dict(nfeatures=500, scaleFactor=1.1, nlevels=16, iniThFAST=20, minThFAST=7), 3),
                                  ("1 level x40", 96, 128, dict(nfeatures=300, scaleFactor=1.2, nlevels=1, iniThFAST=20, minThFAST=7), 40),
                                  ("5 features x12", 160, 256, dict(nfeatures=5, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7), 12),
                                  ("0 features x12", 160, 256, dict(nfeatures=0, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7), 12)],
                         ids=lambda c: c[0])
def test_rich_frames(pkg, oracle, synth, capfd, case):
    """Frames with more corners than the quotas: full levels, so blocks hold keypoints on both sides of a level's first slot (asserted
    for the EuRoC case from the layout of the slots); 16 levels and one level; quotas so small that most blocks are empty; no
    features at all (the totals are still written).  Mixed alignment through an odd frame stride, lapping band inside the image."""
    name, Hh, Ww, cfg, n = case
    lap = (60, 180)
    frames = make_frames(synth, 400, n, Hh, Ww)
    stride, fs = Ww + 4, Hh * (Ww + 4) + 1
    e = pkg.ORBextractor(**cfg)
    try:
        outs, form, cnt = run(e, capfd, pack(frames, 0, stride, fs, np.random.default_rng(401)), 0, Hh, Ww, stride, fs, n, lap, guard=8)
        assert form > 1
        check_frames(e, oracle, cfg, frames, outs, lap=lap, taps=False)
        totals = [int(c) for c in cnt[:, 0]]
        if name == "euroc x40":
            bases = kp_bases(oracle, cfg, Hh, Ww)
            straddles = 0
            for f in frames[:8]:
                lc, _ = level_counts(oracle, cfg, f, lap)
                for l in range(1, cfg["nlevels"]):
                    b = bases[l][0]
                    first = b - b % form   # the block that holds slot b also holds slots first .. b - 1 of level l - 1
                    straddles += b % form != 0 and lc[l] > 0 and bases[l - 1][0] + lc[l - 1] > first
            assert straddles > 0, "no block with keypoints of two levels"
            assert min(totals) > 200
        elif cfg["nfeatures"] <= 5:
            # (the octree still returns its 4 * nIni initial nodes' worth per level; the totals equal the oracle's - check_frames - and
            # were written: run() filled the counts with -1 before the call)
            bound = e.configure(Hh, Ww, n)
            assert 0 < max(totals) <= bound
        else:
            # (make_frames mixes in low-contrast and half-flat frames, which may yield nothing: most frames must be full)
            assert sum(t > 50 for t in totals) > n // 2
    finally:
        e.close()


def test_cap_below_the_bound_is_refused(pkg, capfd):
    """A capacity below orbx_configure()'s bound never reaches the kernels (see the module docstring)."""
    import torch
    frames = [dots_blobs(17, 14)] * 12
    e = pkg.ORBextractor(**CRAFT)
    try:
        bound = e.configure(H, W, 12)
        d_buf = torch.from_numpy(pack(frames, 0, W, H * W)).cuda()
        d_kps = torch.full((12 * bound, 7), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
        d_desc = torch.full((12 * bound, 32), 0xa5, dtype=torch.uint8, device="cuda")
        d_cnt = torch.full((12, 2), -1, dtype=torch.int32, device="cuda")
        with pytest.raises(pkg.OrbError):
            e.extract_batch_device(d_buf.data_ptr(), H, W, W, H * W, 12, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), bound - 1, (0, 1000),
                                   stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (d_kps.cpu().numpy() == 0x5a5a5a5a).all() and (d_desc.cpu().numpy() == 0xa5).all() and (d_cnt.cpu().numpy() == -1).all()
    finally:
        e.close()
