"""orbx_extract_batch_device at the memory layouts and launch forms that orbx_extract never produces.

orbx_extract stages every image into a 64-byte-aligned pitch and runs the batch entry with one frame, so only the batch API reaches
level-0 planes that are not dword-aligned (k_fast's byte-wise tile, k_resize's byte staging, k_blur's non-DMA loop, k_describe's
gathers), batches that mix aligned and unaligned frames, and the per-level k_resize / 256-thread k_octree launches away from the
headline shapes.  Every case is a batch of distinct frames in a buffer laid out on purpose; every frame is compared bit-exactly
with the CPU oracle (outputs and the per-frame stage taps), and every case asserts the launch form it was built to reach through the
library's ORBHIP_PRINT_EXTRACT_FORMS line, so the coverage does not depend on test order."""
import ctypes as C

import numpy as np
import pytest

from conftest import EUROC
from extract_forms import read_forms, resize_forms
from fuzz_parity import random_image

pytestmark = pytest.mark.gpu

_ref_cache = {}


def make_frames(synth, seed, n, H, W):
    """n distinct frames: synthetic, noise, low-contrast, block and half-flat images (fuzz_parity.random_image)."""
    rng = np.random.default_rng([seed, n, H, W])
    frames = []
    for _ in range(n):
        f = random_image(rng, H, W, synth)
        while any(np.array_equal(f, g) for g in frames):
            f = random_image(rng, H, W, synth)
        frames.append(np.ascontiguousarray(f))
    return frames


def pack(frames, offset, stride, frame_stride, pad_rng=None):
    """The frames at offset + k * frame_stride with `stride` bytes per row in one buffer that ends with the last frame's last pixel.
    Row tails and gaps between frames hold 0x00, or random bytes when pad_rng is given."""
    H, W = frames[0].shape
    end = offset + (len(frames) - 1) * frame_stride + (H - 1) * stride + W
    buf = np.zeros(end, np.uint8) if pad_rng is None else pad_rng.integers(0, 256, end, dtype=np.uint8)
    for k, f in enumerate(frames):
        base = offset + k * frame_stride
        for y in range(H):
            buf[base + y * stride:base + y * stride + W] = f[y]
    return buf


def run_batch(e, capfd, buf, offset, H, W, stride, frame_stride, n, lap=(0, 1000)):
    """One orbx_extract_batch_device call on buf (uploaded as is).  Returns per-frame (mono, kps, desc) and the form line; asserts
    that the input buffer, padding included, is unchanged."""
    import torch
    cap = e.configure(H, W, n)
    d_buf = torch.from_numpy(buf).cuda()
    d_kps = torch.zeros((n, cap, 7), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    capfd.readouterr()
    e.extract_batch_device(d_buf.data_ptr() + offset, H, W, stride, frame_stride, n, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(),
                           cap, lap, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    forms = read_forms(capfd.readouterr().err)
    assert len(forms) == 1, forms
    assert np.array_equal(d_buf.cpu().numpy(), buf), "the input buffer was written"
    cnt, kps, desc = d_cnt.cpu().numpy(), d_kps.cpu().numpy(), d_desc.cpu().numpy()
    outs = []
    for k in range(n):
        m = int(cnt[k, 0])
        assert 0 <= m <= cap
        outs.append((int(cnt[k, 1]), kps[k, :m].tobytes(), desc[k, :m].tobytes()))
    e._keep = d_buf   # level 0 is read in place by the stage taps below: the buffer must outlive them
    return outs, forms[0]


def oracle_ref(oracle, cfg, img, lap):
    key = (tuple(sorted(cfg.items())), img.shape, img.tobytes(), lap)
    if key not in _ref_cache:
        o = oracle.OracleExtractor(**cfg)
        mono, kps, desc = o.extract(img, lap)
        pyr = o.pyramid(img)
        q = o.features_per_level
        cands = [o.level_candidates(p) for p in pyr]
        octs = [oracle.distribute_octtree(c, 16, p.shape[1] - 16, 16, p.shape[0] - 16, q[l]) for l, (c, p) in enumerate(zip(cands, pyr))]
        b0 = np.zeros((img.shape[0] + 38, img.shape[1] + 38), np.uint8)
        oracle.lib().orc_copy_make_border101(img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0], C.c_size_t(img.shape[1]),
                                             b0.ctypes.data_as(C.c_void_p), 19, C.c_size_t(img.shape[1] + 38))
        _ref_cache[key] = dict(out=(mono, kps.tobytes(), desc.tobytes()), pyr=pyr, blur=[oracle.gaussian_blur7(p) for p in pyr],
                               cands=cands, octs=octs, border0=b0)
    return _ref_cache[key]


def check_frames(e, oracle, cfg, frames, outs, lap=(0, 1000), taps=True):
    """Every frame of the last batch against the oracle: counts, monoIndex, keypoints, descriptors and the stage taps."""
    for k, img in enumerate(frames):
        ref = oracle_ref(oracle, cfg, img, lap)
        assert outs[k][0] == ref["out"][0], "frame %d: monoIndex" % k
        assert outs[k][1] == ref["out"][1], "frame %d: keypoints" % k
        assert outs[k][2] == ref["out"][2], "frame %d: descriptors" % k
        if not taps:
            continue
        assert np.array_equal(e.image_pyramid_level(0, frame=k, border=19), ref["border0"]), "frame %d: level 0 with its border" % k
        for l in range(cfg["nlevels"]):
            assert np.array_equal(e.image_pyramid_level(l, frame=k), ref["pyr"][l]), "frame %d: pyramid level %d" % (k, l)
            assert np.array_equal(e.blurred_level(l, frame=k), ref["blur"][l]), "frame %d: blurred level %d" % (k, l)
            assert np.array_equal(e.level_candidates(l, frame=k), ref["cands"][l]), "frame %d: FAST candidates level %d" % (k, l)
            assert np.array_equal(e.level_keypoints(l, frame=k), ref["octs"][l]), "frame %d: octree level %d" % (k, l)


@pytest.fixture(autouse=True)
def print_forms(monkeypatch):
    monkeypatch.setenv("ORBHIP_PRINT_EXTRACT_FORMS", "1")


@pytest.fixture(scope="module")
def shared(pkg):
    """One handle for the whole module: batch sizes and geometries change from test to test (orbx_configure's max_batch resizing)."""
    e = pkg.ORBextractor(**EUROC)
    yield e
    e.close()


def expect(form, nframes, pyramid, octree, aligned0, blur0dma):
    got = (form["nframes"], form["pyramid"], form["octree"], form["aligned0"], form["blur0dma"])
    assert got == (nframes, pyramid, octree, aligned0, blur0dma), "form line %s" % (form,)


# ---- layouts ------------------------------------------------------------------------------------------------------------------
# (name, H, W, offset, stride - W, frame_stride - H * stride, nframes, aligned frames, level-0 blur by DMA)
LAYOUTS = [
    ("base+0", 120, 320, 0, 16, 0, 3, 3, 3),
    ("base+1", 120, 320, 1, 0, 0, 3, 0, 0),
    ("base+2", 120, 320, 2, 8, 0, 3, 0, 0),
    ("base+3", 120, 320, 3, 4, 0, 3, 0, 0),
    ("stride%4=1", 120, 320, 0, 5, 0, 3, 0, 0),
    ("stride%4=2", 120, 320, 0, 6, 0, 3, 0, 0),
    ("stride%4=3", 120, 320, 0, 7, 0, 3, 0, 0),
    ("stride%4=0 padded", 120, 320, 0, 12, 0, 3, 3, 3),
    ("odd frame_stride", 120, 320, 0, 4, 1, 5, 2, 2),          # frames 0 and 4 aligned, 1..3 not, in one launch
    ("gaps between frames", 120, 320, 0, 8, 4100, 3, 3, 3),
    ("tight, cols%4=2", 120, 318, 0, 0, 0, 3, 0, 0),           # the last frame ends at the end of the buffer
    ("cols%16=4, aligned pitch", 120, 324, 0, 0, 0, 3, 3, 0),  # k_blur's non-DMA loop on an aligned level 0
]


@pytest.mark.parametrize("case", LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_layout(shared, oracle, synth, capfd, case):
    name, H, W, off, spad, gap, n, al, dma = case
    stride = W + spad
    fs = H * stride + gap
    frames = make_frames(synth, 300, n, H, W)
    res = []
    for pad_rng in (None, np.random.default_rng(301)):
        buf = pack(frames, off, stride, fs, pad_rng)
        outs, form = run_batch(shared, capfd, buf, off, H, W, stride, fs, n)
        expect(form, n, "chain" if 8 * n <= 32 else resize_forms(H, W, 1.2, 8), (1024, "lds") if 8 * n <= 32 else (256, "lds"), al, dma)
        res.append(outs)
        check_frames(shared, oracle, EUROC, frames, outs, taps=pad_rng is not None)
    assert res[0] == res[1], "padding bytes changed the outputs"


# ---- launch forms ---------------------------------------------------------------------------------------------------------------
CHAIN = [2, 3, 4]


@pytest.mark.parametrize("n", CHAIN)
def test_chain_multi_frame(shared, oracle, synth, capfd, n):
    """k_pyramid_chain with several frames (frame = blockIdx / ntile), one of them unaligned through an odd frame stride."""
    H, W = 200, 336
    frames = make_frames(synth, 310 + n, n, H, W)
    stride, fs = W, H * W + 3
    outs, form = run_batch(shared, capfd, pack(frames, 0, stride, fs), 0, H, W, stride, fs, n)
    expect(form, n, "chain", (1024, "lds"), (n + 3) // 4, (n + 3) // 4)
    check_frames(shared, oracle, EUROC, frames, outs)


# (H, W, cfg, nframes, pyramid form, octree form)
FORMS = [
    # single frames at large scale factors: the chain tables fit, so these run k_pyramid_chain (k_resize's forms for the same
    # geometries are the batches below)
    ("sf2.0 single", 256, 300, dict(nfeatures=64, scaleFactor=2.0, nlevels=3, iniThFAST=30, minThFAST=30), 1, "chain", (1024, "lds")),
    ("sf2.6 single", 500, 700, dict(nfeatures=300, scaleFactor=2.6, nlevels=3, iniThFAST=20, minThFAST=7), 1, "chain", (1024, "lds")),
    ("sf3.3 single", 600, 900, dict(nfeatures=200, scaleFactor=3.3, nlevels=2, iniThFAST=20, minThFAST=7), 1, "chain", (1024, "lds")),
    # batches: 16-row tiles at EuRoC (level 7: 21 source rows of 424 bytes, so the row records follow an offset of 8 mod 16 before
    # padding), KITTI's 8-row level 1 (11 source rows of 2072 bytes: the same), 8-row tiles at scale 2.6, the one-pass form by the
    # horizontal ratio
    ("euroc x5", 480, 752, EUROC, 5, ("2p16",) * 7, (256, "lds")),
    ("kitti x5", 376, 1241, dict(nfeatures=2000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7), 5, ("2p8",) + ("2p16",) * 6, (256, "lds")),
    ("sf2.0 x11", 256, 300, dict(nfeatures=64, scaleFactor=2.0, nlevels=3, iniThFAST=30, minThFAST=30), 11, ("2p16", "2p16"), (256, "lds")),
    ("sf2.6 x11", 500, 700, dict(nfeatures=300, scaleFactor=2.6, nlevels=3, iniThFAST=20, minThFAST=7), 11, ("2p8", "2p8"), (256, "lds")),
    ("sf3.3 x17", 300, 450, dict(nfeatures=200, scaleFactor=3.3, nlevels=2, iniThFAST=20, minThFAST=7), 17, ("1p",), (256, "lds")),
    # the one-pass form through the source-row limit: a 2-column level 1 and a 1-column level 2 (horizontal ratio 2 < 3) whose
    # 8-row tiles span 33 source rows
    ("srcrows x11", 240, 11, dict(nfeatures=100, scaleFactor=4.5, nlevels=3, iniThFAST=20, minThFAST=7), 11, ("1p", "1p"), (256, "lds")),
    # the octree's cell offsets in global memory (6500 features: 1412 on level 0, 102 KB of nodes)
    ("octree 1024 global", 240, 384, dict(nfeatures=6500, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7), 1, "chain", (1024, "global")),
    ("octree 256 global", 240, 384, dict(nfeatures=6500, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7), 5, ("2p16",) * 7, (256, "global")),
    ("ini 5000 x5", 240, 384, dict(nfeatures=5000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7), 5, ("2p16",) * 7, (256, "lds")),
    # XCD full / tail splits of the per-frame work (frames f % 8 per XCD)
    ("xcd x8", 160, 256, EUROC, 8, ("2p16",) * 7, (256, "lds")),
    ("xcd x9", 160, 256, EUROC, 9, ("2p16",) * 7, (256, "lds")),
    ("xcd x17 odd width", 150, 253, EUROC, 17, ("2p16",) * 7, (256, "lds")),
    # level counts at the ends of the range; 16 levels at scale 1.1 have chain tables too large for one launch, so a single frame
    # and a wide pair take the level-by-level k_resize with the 1024-thread octree
    ("1 level x3", 160, 256, dict(nfeatures=300, scaleFactor=1.2, nlevels=1, iniThFAST=20, minThFAST=7), 3, "none", (1024, "lds")),
    ("1 level x40", 96, 128, dict(nfeatures=300, scaleFactor=1.2, nlevels=1, iniThFAST=20, minThFAST=7), 40, "none", (256, "lds")),
    ("16 levels x2", 480, 752, dict(nfeatures=1000, scaleFactor=1.1, nlevels=16, iniThFAST=20, minThFAST=7), 2, ("2p16",) * 15, (1024, "lds")),
    ("16 levels x1", 480, 752, dict(nfeatures=1000, scaleFactor=1.1, nlevels=16, iniThFAST=20, minThFAST=7), 1, ("2p16",) * 15, (1024, "lds")),
    ("16 levels x3", 240, 376, dict(nfeatures=500, scaleFactor=1.1, nlevels=16, iniThFAST=20, minThFAST=7), 3, ("2p16",) * 15, (256, "lds")),
]


@pytest.mark.parametrize("case", FORMS, ids=[c[0] for c in FORMS])
def test_form(pkg, oracle, synth, capfd, case):
    name, H, W, cfg, n, pyramid, octree = case
    if isinstance(pyramid, tuple):
        assert resize_forms(H, W, cfg["scaleFactor"], cfg["nlevels"]) == pyramid   # the host replay agrees with the pinned form
    frames = make_frames(synth, 320, n, H, W)
    # every other case at an unaligned stride (1 mod 4), the others at an aligned stride with an odd frame stride
    unal = FORMS.index(case) % 2 == 1
    stride = (W | 3) + 2 if unal else ((W + 3) & ~3) + 4
    fs = H * stride + (1 if n > 1 else 0)
    e = pkg.ORBextractor(**cfg)
    try:
        outs, form = run_batch(e, capfd, pack(frames, 0, stride, fs, np.random.default_rng(321)), 0, H, W, stride, fs, n)
        al = 0 if unal else (n + 3) // 4
        dma = al if (W >= 160 and H >= 40 and W % 16 == 0) else 0
        expect(form, n, pyramid, octree, al, dma)
        check_frames(e, oracle, cfg, frames, outs, taps=n <= 5 or H * W <= 160 * 256)
    finally:
        e.close()


# ---- position independence, stereo, one handle ---------------------------------------------------------------------------------
def test_position_independence(shared, oracle, synth, capfd):
    """The same frame at positions 0, 7, 8 and 9 (last) of a 10-frame batch with an odd frame stride - alignments 0, 3, 0 and 1 of
    the base - gives identical outputs everywhere, equal to orbx_extract on that frame."""
    H, W = 160, 256
    frames = make_frames(synth, 330, 10, H, W)
    for k in (7, 8, 9):
        frames[k] = frames[0]
    stride, fs = W + 4, H * (W + 4) + 1
    outs, form = run_batch(shared, capfd, pack(frames, 0, stride, fs, np.random.default_rng(331)), 0, H, W, stride, fs, 10)
    expect(form, 10, ("2p16",) * 7, (256, "lds"), 3, 3)
    assert outs[7] == outs[0] and outs[8] == outs[0] and outs[9] == outs[0]
    mono, kps, desc = shared(frames[0], None, (0, 1000))
    assert outs[0] == (mono, kps.tobytes(), desc.tobytes())
    check_frames(shared, oracle, EUROC, frames[:1], outs[:1])
    check_frames(shared, oracle, EUROC, frames[1:7], outs[1:7], taps=False)


def test_stereo_from_batches(pkg, oracle, synth, capfd):
    """Frame::ComputeStereoMatches on frames 2 (left) and 1 (right) of two batches with different strides, the right one unaligned:
    k_stereo_match reads level 0 of both in place (strideL0 / strideR0)."""
    H, W, disp = 240, 384, 21
    big = synth.make_frame(4321, H=H, W=W + 64)
    left = make_frames(synth, 340, 3, H, W)
    right = make_frames(synth, 341, 3, H, W)
    left[2] = np.ascontiguousarray(big[:, :W])
    right[1] = np.ascontiguousarray(big[:, disp:disp + W])
    exL, exR = pkg.ORBextractor(**EUROC), pkg.ORBextractor(**EUROC)
    try:
        sL, fsL = W + 64, H * (W + 64)
        sR, fsR = W + 3, H * (W + 3) + 5
        outL, formL = run_batch(exL, capfd, pack(left, 0, sL, fsL), 0, H, W, sL, fsL, 3, lap=(0, 0))
        outR, formR = run_batch(exR, capfd, pack(right, 1, sR, fsR, np.random.default_rng(342)), 1, H, W, sR, fsR, 3, lap=(0, 0))
        assert formL["aligned0"] == 3 and formR["aligned0"] == 0
        kL = np.frombuffer(outL[2][1], pkg.KP_DTYPE).copy(); dL = np.frombuffer(outL[2][2], np.uint8).reshape(-1, 32).copy()
        kR = np.frombuffer(outR[1][1], pkg.KP_DTYPE).copy(); dR = np.frombuffer(outR[1][2], np.uint8).reshape(-1, 32).copy()
        mb, mbf = 0.11, 47.9
        uR, z = exL.ComputeStereoMatches(exR, kL, dL, kR, dR, mb, mbf, frame_l=2, frame_r=1)
        o = oracle.OracleExtractor(**EUROC)
        uR_ref, z_ref = o.compute_stereo_matches(left[2], right[1], kL, dL, kR, dR, mb, mbf)
        assert np.array_equal(uR.view(np.uint32), uR_ref.view(np.uint32))
        assert np.array_equal(z.view(np.uint32), z_ref.view(np.uint32))
        assert (uR_ref >= 0).sum() > 50
        check_frames(exL, oracle, EUROC, left[2:], outL[2:], lap=(0, 0), taps=False)
        check_frames(exR, oracle, EUROC, right[1:2], outR[1:2], lap=(0, 0), taps=False)
    finally:
        exL.close(); exR.close()


def test_one_handle_batch_sizes(shared, oracle, synth, capfd):
    """The module's handle through batch sizes 2 -> 9 -> 3 and a change of geometry and back: the workspace grows and is re-derived
    (orbx_configure's max_batch), and every batch still matches the oracle."""
    for (H, W, n, pyr, oc) in [(128, 192, 2, "chain", (1024, "lds")), (128, 192, 9, ("2p16",) * 7, (256, "lds")),
                               (144, 200, 3, "chain", (1024, "lds")), (128, 192, 3, "chain", (1024, "lds")),
                               (128, 192, 9, ("2p16",) * 7, (256, "lds"))]:
        frames = make_frames(synth, 350 + n, n, H, W)
        stride, fs = W + 1, H * (W + 1) + 2
        outs, form = run_batch(shared, capfd, pack(frames, 2, stride, fs, np.random.default_rng(351)), 2, H, W, stride, fs, n)
        expect(form, n, pyr, oc, 0, 0)
        check_frames(shared, oracle, EUROC, frames, outs, taps=n <= 3)
