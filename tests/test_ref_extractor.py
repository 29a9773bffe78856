"""CPU: the oracle's extractor against the reference's own ORBextractor.cc, compiled.

oracle/_ref/libref_extractor.so is the reference's unmodified extractor source built against stand-in containers (oracle/ref_shim)
with the six OpenCV primitives forwarded to the oracle and a monotone allocator, so that the pointer tie of ORBextractor.cc:682
goes by creation order (oracle/ref_driver.cc).  What these tests pin is therefore the oracle's reading of the extractor's own text:
cell grid, threshold fallback, DistributeOctTree, IC_Angle, the steered pattern, per-level scaling, the lapping-area order and the
pyramid geometry.  They say nothing about the primitives, which are the oracle's on both sides.  Every comparison is equality of
bytes.

The library is built here when the reference tree is present; the tests skip only where there is neither a library nor a tree."""
import ctypes as C

import numpy as np
import pytest

import octree_model as M
import ref_cases as R


@pytest.fixture(scope="module")
def ref(oracle):
    if oracle.build_ref() is None:
        pytest.skip("no oracle/_ref/libref_extractor.so and no reference tree to build it from")
    return oracle


_frames = {}


def frame_of(synth, name, rows, cols, k=0):
    key = (name, rows, cols, k)
    if key not in _frames:
        _frames[key] = synth.make_frame(300 + k, rows, cols) if name == "synth" else R.special_frames(synth, rows, cols)[name]
    return _frames[key]


def assert_same_extraction(ref, cfg, img, lap):
    mono_o, kps_o, desc_o = ref.OracleExtractor(**cfg).extract(img, lap)
    mono_r, kps_r, desc_r = ref.RefExtractor(**cfg).extract(img, lap)
    assert len(kps_r) == len(kps_o), "keypoint count: reference %d, oracle %d" % (len(kps_r), len(kps_o))
    assert mono_r == mono_o, "monoIndex: reference %d, oracle %d" % (mono_r, mono_o)
    assert kps_r.tobytes() == kps_o.tobytes(), "keypoints differ"
    assert desc_r.tobytes() == desc_o.tobytes(), "descriptors differ"
    return mono_r, kps_r


# ---- the domain ------------------------------------------------------------------------------------------------------------------
def test_listed_shapes_are_inside_the_reference_domain():
    for rows, cols, cfg, _ in R.CONFIGS.values():
        assert R.in_reference_domain(rows, cols, cfg["scaleFactor"], cfg["nlevels"])
    # the tall frame on which the compiled reference reads a null root node: level 7 is 67 x 105, its rectangle 35 x 73
    assert not R.in_reference_domain(376, 240, 1.2, 8)
    assert R.level_sizes(376, 240, 1.2, 8)[7] == (105, 67)
    assert [R.in_reference_domain(r, c, 1.2, 8) for r, c in ((300, 240), (330, 240), (350, 240), (240, 200), (480, 300))] == [True] * 5


def test_level_sizes_and_quotas_match(ref, synth):
    for rows, cols, cfg, _ in R.CONFIGS.values():
        o, r = ref.OracleExtractor(**cfg), ref.RefExtractor(**cfg)
        assert r.features_per_level == o.features_per_level
        sizes = r.level_sizes(frame_of(synth, "synth", rows, cols))
        assert sizes == [o.level_size(l, cols, rows) for l in range(cfg["nlevels"])]
        assert [(lr, lc) for lc, lr in sizes] == R.level_sizes(rows, cols, cfg["scaleFactor"], cfg["nlevels"])


def test_outside_the_domain_the_oracle_drops_the_level(ref):
    """376 x 240 (rows x cols) is outside the reference's domain: level 7 has candidates and no root node.  The oracle's definition
    there is 'no keypoints on that level'; the levels below it are unaffected.  (The product refuses the geometry:
    tests/test_gpu_ref_extractor.py.)"""
    img = R.noise(376, 240)
    o = ref.OracleExtractor(**R.CONFIGS["euroc"][2])
    pyr = o.pyramid(img)
    assert len(o.level_candidates(pyr[7])) > 0
    assert len(ref.distribute_octtree(o.level_candidates(pyr[7]), 16, 67 - 16, 16, 105 - 16, 10)) == 0
    _, kps, _ = o.extract(img)
    assert len(kps) > 500 and set(np.unique(kps["octave"]).tolist()) == set(range(7))


# ---- operator() ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_extract_configurations(ref, synth, name, k):
    rows, cols, cfg, lap = R.CONFIGS[name]
    mono, kps = assert_same_extraction(ref, cfg, frame_of(synth, "synth", rows, cols, k), lap)
    assert len(kps) > 200
    # the three lapping areas of the table: one takes every keypoint, one none, one splits them
    if lap == (0, 1000):
        assert mono == 0
    elif lap == (0, 0):
        assert mono == len(kps)
    else:
        assert 0 < mono < len(kps)


@pytest.mark.parametrize("name", ["noise", "checkerboard", "squares", "low_contrast", "constant"])
def test_extract_special_frames(ref, synth, name):
    rows, cols, cfg, _ = R.CONFIGS["euroc"]
    img = frame_of(synth, name, rows, cols)
    mono, kps = assert_same_extraction(ref, cfg, img, (200, 500))
    if name == "constant":
        assert len(kps) == 0 and mono == 0   # the release() branch of ORBextractor.cc:1100-1101
    else:
        assert len(kps) > 300 and 0 < mono < len(kps)
    if name == "checkerboard":   # most keypoints share their response with another one: the first maximum in a node decides
        _, counts = np.unique(kps["response"], return_counts=True)
        assert counts[counts > 1].sum() >= len(kps) // 2
    if name == "squares":        # level 0: one response value for every corner
        r0 = kps["response"][kps["octave"] == 0]
        assert len(r0) > 50 and len(np.unique(r0)) == 1
    if name == "low_contrast":
        o = ref.OracleExtractor(**cfg)
        hi = ref.OracleExtractor(**dict(cfg, minThFAST=cfg["iniThFAST"]))
        lvl0 = o.pyramid(img)[0]
        assert len(hi.level_candidates(lvl0)) < len(o.level_candidates(lvl0)) // 2   # most cells answer only at minThFAST


def test_extract_empty_image(ref):
    r = ref.RefExtractor(**R.CONFIGS["euroc"][2])
    n = C.c_int(5)
    assert r.L.ref_extract(*r.cfg, None, 0, 0, C.c_size_t(0), 0, 1000, None, None, 0, C.byref(n)) == -1 and n.value == 0
    o = ref.OracleExtractor(**R.CONFIGS["euroc"][2])
    assert o.L.orc_extract(C.byref(o.e), None, 0, 0, C.c_size_t(0), 0, 1000, None, None, 0, C.byref(n)) == -1


# ---- ComputePyramid ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "euroc"])
def test_pyramid(ref, synth, name):
    rows, cols, cfg, _ = R.CONFIGS[name]
    img = frame_of(synth, "synth", rows, cols)
    o, r = ref.OracleExtractor(**cfg), ref.RefExtractor(**cfg)
    po, pr, pb = o.pyramid(img), r.pyramid(img), r.pyramid(img, border=19)
    assert len(po) == len(pr) == cfg["nlevels"]
    for l in range(cfg["nlevels"]):
        assert pr[l].shape == po[l].shape, "level %d" % l
        assert np.array_equal(pr[l], po[l]), "level %d" % l
        # the padded buffer behind the view: BORDER_REFLECT_101 of the level itself (ORBextractor.cc:1203-1215)
        b = np.zeros((po[l].shape[0] + 38, po[l].shape[1] + 38), np.uint8)
        ref.lib().orc_copy_make_border101(po[l].ctypes.data_as(C.c_void_p), po[l].shape[1], po[l].shape[0], C.c_size_t(po[l].shape[1]),
                                          b.ctypes.data_as(C.c_void_p), 19, C.c_size_t(b.shape[1]))
        assert np.array_equal(pb[l], b), "level %d with its border" % l


# ---- ComputeKeyPointsOctTree, per level ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frame", [("half", "synth"), ("odd", "synth"), ("dense", "synth"), ("half", "checkerboard"), ("half", "squares"), ("half", "low_contrast")])
def test_level_keypoints(ref, synth, name, frame):
    """allKeypoints before operator() scales them: the oracle's stages chained by hand (candidates, octree, border offset,
    IC_Angle, patch size) against the reference's vectors."""
    rows, cols, cfg, _ = R.CONFIGS[name]
    img = frame_of(synth, frame, rows, cols)
    o, r = ref.OracleExtractor(**cfg), ref.RefExtractor(**cfg)
    got = r.level_keypoints(img)
    pyr, quota, sf = o.pyramid(img), o.features_per_level, o.scale_factors
    for l in range(cfg["nlevels"]):
        h, w = pyr[l].shape
        sel = ref.distribute_octtree(o.level_candidates(pyr[l]), 16, w - 16, 16, h - 16, quota[l]) if w > 32 and h > 32 else np.zeros((0, 3), np.float32)
        want = np.zeros(len(sel), ref.KP_DTYPE)
        want["x"], want["y"], want["response"] = sel[:, 0] + np.float32(16), sel[:, 1] + np.float32(16), sel[:, 2]
        want["size"], want["octave"], want["class_id"] = np.float32(int(np.float32(31) * sf[l])), l, -1
        want["angle"] = [np.float32(o.ic_angle(pyr[l], x, y)) for x, y in zip(want["x"], want["y"])]
        assert got[l].tobytes() == want.tobytes(), "level %d" % l


# ---- DistributeOctTree -----------------------------------------------------------------------------------------------------------------
OCTREE = R.octree_cases()


def model_select(xyr, box, N, **kw):
    idx = M.distribute(xyr[:, 0].astype(np.int64), xyr[:, 1].astype(np.int64), xyr[:, 2].astype(np.int64), *box, N, **kw)
    return xyr[idx].reshape(-1, 3)


@pytest.mark.parametrize("case", OCTREE, ids=[c[0] for c in OCTREE])
def test_distribute_octtree(ref, case):
    _, xyr, box, N = case
    got = ref.ref_distribute_octtree(xyr, *box, N)
    want = ref.distribute_octtree(xyr, *box, N)
    assert got.shape == want.shape, "reference %d keypoints, oracle %d" % (len(got), len(want))
    assert got.tobytes() == want.tobytes()
    assert model_select(xyr, box, N).tobytes() == got.tobytes(), "the data-parallel model differs from the reference"


def test_distribute_octtree_tie_rule_decides(ref):
    """The tie cases are built so that the order among equal-sized nodes changes the answer: the model with the tie reversed must give
    another result there, or the comparison above would not test the rule at all."""
    ties = [c for c in OCTREE if c[0].startswith("tie_")]
    assert len(ties) >= 4
    decided = 0
    for _, xyr, box, N in ties:
        got = ref.ref_distribute_octtree(xyr, *box, N)
        assert model_select(xyr, box, N).tobytes() == got.tobytes()
        if model_select(xyr, box, N, tie_newest_first=False).tobytes() != got.tobytes():
            decided += 1
    assert decided >= 4, "only %d of %d tie cases depend on the tie order" % (decided, len(ties))
