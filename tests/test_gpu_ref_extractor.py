"""GPU: the HIP extractor against the reference's own ORBextractor.cc, compiled (oracle/_ref/libref_extractor.so).

The other GPU tests compare with oracle/orb_oracle.c, a restatement by hand; these compare with the reference's unmodified extractor
source built against stand-in containers, the oracle's OpenCV primitives and a monotone allocator (oracle/ref_driver.cc).  A
misreading of the extractor's own text - cell grid, threshold fallback, DistributeOctTree and its tie order, IC_Angle, the steered
pattern, per-level scaling, the lapping-area order, the pyramid geometry - that the oracle and the kernels share shows here.  Stage
by stage and per level: orbx_download_pyramid, orbx_download_level_keypoints, then the outputs of orbx_extract; the same through
orbx_extract_batch_device.  Equality of bytes everywhere.

The library is built by __graft_entry__.build() where the reference tree exists and travels with the tree; these tests only load it
and never look for the reference.  Without it they FAIL: a skip would hide the whole file.

k_octree has no entry point that takes candidates, so the built octree inputs of tests/test_ref_extractor.py reach it only through
images here; they are compared with the data-parallel model of the kernel (tests/octree_model.py) on the CPU."""
import numpy as np
import pytest

import ref_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(oracle):
    try:
        oracle.ref_lib(build_if_possible=False)
    except (RuntimeError, OSError) as e:
        pytest.fail("oracle/_ref/libref_extractor.so cannot be loaded (%s): run __graft_entry__.build() where the reference tree exists" % e)
    return oracle


_frames, _refs = {}, {}


def frame_of(synth, kind, rows, cols):
    key = (kind, rows, cols)
    if key not in _frames:
        _frames[key] = synth.make_frame(300, rows, cols) if kind == "synth" else R.special_frames(synth, rows, cols)[kind]
    return _frames[key]


def reference_of(ref, name, kind, synth, lap):
    """The compiled reference's stages for one case, computed once."""
    key = (name, kind, lap)
    if key not in _refs:
        rows, cols, cfg, _ = R.CONFIGS[name]
        img = frame_of(synth, kind, rows, cols)
        r = ref.RefExtractor(**cfg)
        mono, kps, desc = r.extract(img, lap)
        _refs[key] = dict(mono=mono, kps=kps.tobytes(), desc=desc.tobytes(), n=len(kps), pyr=r.pyramid(img), pyr19=r.pyramid(img, border=19),
                          levels=r.level_keypoints(img))
    return _refs[key]


def check_stages(e, want, nlevels, frame=0):
    """mvImagePyramid (with and without its border) and the per-level DistributeOctTree output of the last call."""
    for border, key in ((0, "pyr"), (19, "pyr19")):
        got = e.image_pyramid(frame=frame, border=border)
        assert len(got) == nlevels
        for l in range(nlevels):
            assert got[l].shape == want[key][l].shape, "frame %d: level %d shape (border %d)" % (frame, l, border)
            assert np.array_equal(got[l], want[key][l]), "frame %d: pyramid level %d (border %d)" % (frame, l, border)
    for l in range(nlevels):
        k = want["levels"][l]
        xyr = np.stack([k["x"] - np.float32(16), k["y"] - np.float32(16), k["response"]], axis=1).astype(np.float32).reshape(-1, 3)
        got = e.level_keypoints(l, frame=frame)
        assert got.shape == xyr.shape, "frame %d: level %d has %d keypoints, the reference %d" % (frame, l, len(got), len(xyr))
        assert got.tobytes() == xyr.tobytes(), "frame %d: octree output of level %d" % (frame, l)


# (configuration, frame kind): 97 x 160 isolates FAST, orientation and descriptors (nothing is pruned), 131 x 173 has odd sizes, a
# non-default factor and heavy pruning, 240 x 376 a lapping area that splits the keypoints; the two production sizes once each
CASES = [("dense", "synth"), ("odd", "synth"), ("half", "synth"), ("euroc", "synth"), ("tumvi", "synth"),
         ("half", "checkerboard"), ("half", "low_contrast"), ("half", "squares")]


@pytest.mark.parametrize("name,kind", CASES, ids=["%s-%s" % c for c in CASES])
def test_extract_stages(pkg, ref, synth, name, kind):
    rows, cols, cfg, lap = R.CONFIGS[name]
    assert R.in_reference_domain(rows, cols, cfg["scaleFactor"], cfg["nlevels"])
    img = frame_of(synth, kind, rows, cols)
    want = reference_of(ref, name, kind, synth, lap)
    assert want["n"] > 100
    e = pkg.ORBextractor(**cfg)
    try:
        mono, kps, desc = e(img, None, lap)
        check_stages(e, want, cfg["nlevels"])
        assert len(kps) == want["n"], "%d keypoints, the reference %d" % (len(kps), want["n"])
        assert mono == want["mono"]
        assert kps.tobytes() == want["kps"], "keypoints differ from the compiled reference"
        assert desc.tobytes() == want["desc"], "descriptors differ from the compiled reference"
    finally:
        e.close()


def test_extract_constant_image(pkg, ref):
    """No keypoint at all: the release() branch, monoIndex 0."""
    rows, cols, cfg, lap = R.CONFIGS["half"]
    img = R.constant(rows, cols)
    mono_r, kps_r, _ = ref.RefExtractor(**cfg).extract(img, lap)
    e = pkg.ORBextractor(**cfg)
    try:
        mono, kps, desc = e(img, None, lap)
    finally:
        e.close()
    assert (mono, len(kps), len(desc)) == (mono_r, len(kps_r), 0) == (0, 0, 0)


def run_batch(e, frames, stride, frame_stride, offset, lap):
    """orbx_extract_batch_device on the frames laid out at offset + k * frame_stride with `stride` bytes per row; padding holds 0xA5."""
    import torch
    n = len(frames)
    H, W = frames[0].shape
    buf = np.full(offset + (n - 1) * frame_stride + (H - 1) * stride + W, 0xA5, np.uint8)
    for k, f in enumerate(frames):
        rows = np.lib.stride_tricks.as_strided(buf[offset + k * frame_stride:], shape=(H, W), strides=(stride, 1))
        rows[:] = f
    cap = e.configure(H, W, n)
    d_buf = torch.from_numpy(buf).cuda()
    d_kps = torch.zeros((n, cap, 7), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    e.extract_batch_device(d_buf.data_ptr() + offset, H, W, stride, frame_stride, n, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), cap, lap,
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_buf.cpu().numpy(), buf), "the input buffer was written"
    cnt, kps, desc = d_cnt.cpu().numpy(), d_kps.cpu().numpy(), d_desc.cpu().numpy()
    outs = []
    for k in range(n):
        m = int(cnt[k, 0])
        assert 0 <= m <= cap
        outs.append((int(cnt[k, 1]), m, kps[k, :m].tobytes(), desc[k, :m].tobytes()))
    return outs, d_buf   # level 0 is read in place by the stage taps: the caller keeps the buffer alive


# (configuration, three different frames, stride - W, gap between frames, offset of the first)
BATCHES = [("half", ("synth", "checkerboard", "low_contrast"), 0, 0, 0),
           ("half", ("low_contrast", "synth", "squares"), 24, 100, 64),
           ("odd", ("synth", "noise", "low_contrast"), 3, 7, 1)]


@pytest.mark.parametrize("name,kinds,pad,gap,offset", BATCHES, ids=["%s-pad%d" % (b[0], b[2]) for b in BATCHES])
def test_batch_device_stages(pkg, ref, synth, name, kinds, pad, gap, offset):
    rows, cols, cfg, lap = R.CONFIGS[name]
    frames = [frame_of(synth, kind, rows, cols) for kind in kinds]
    stride = cols + pad
    e = pkg.ORBextractor(**cfg)
    try:
        outs, keep = run_batch(e, frames, stride, rows * stride + gap, offset, lap)
        for k, kind in enumerate(kinds):
            want = reference_of(ref, name, kind, synth, lap)
            mono, n, kps, desc = outs[k]
            check_stages(e, want, cfg["nlevels"], frame=k)
            assert n == want["n"], "frame %d: %d keypoints, the reference %d" % (k, n, want["n"])
            assert mono == want["mono"], "frame %d: monoIndex" % k
            assert kps == want["kps"], "frame %d: keypoints differ from the compiled reference" % k
            assert desc == want["desc"], "frame %d: descriptors differ from the compiled reference" % k
        del keep
    finally:
        e.close()


def test_geometry_outside_the_reference_domain_is_refused(pkg):
    """Where a level with cells is taller than twice its width the reference's DistributeOctTree has no root node and reads a null
    pointer at the first candidate (ORBextractor.cc:541-567; tests/ref_cases.py has the domain).  orbx_configure refuses such a
    geometry with ORBX_E_ARG instead of defining a result; the neighbouring geometries inside the domain are accepted."""
    e = pkg.ORBextractor(**R.CONFIGS["euroc"][2])
    try:
        for rows, cols in ((376, 240), (300, 100), (480, 240)):
            assert not R.in_reference_domain(rows, cols, 1.2, 8)
            with pytest.raises(ValueError, match="no root node"):
                e.configure(rows, cols)
        for rows, cols in ((350, 240), (330, 240), (300, 240), (240, 200), (480, 300), (131, 173)):
            assert R.in_reference_domain(rows, cols, 1.2, 8)
            assert e.configure(rows, cols) > 0
    finally:
        e.close()
