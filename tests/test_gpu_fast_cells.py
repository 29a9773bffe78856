"""k_fast's per-cell detection (one wavefront per cell of a 2 x 2 group, survivor queue, shared score plane) against the CPU
oracle: FAST candidates of every level, bit-exact, on frames chosen to reach the kernel's less common paths."""
import numpy as np
import pytest

from conftest import EUROC
from extract_forms import read_forms

pytestmark = pytest.mark.gpu


def check_levels(pkg, oracle, img, cfg=EUROC):
    """Extract img and compare every level's FAST candidates (and the keypoints) with the oracle's."""
    e = pkg.ORBextractor(**cfg)
    o = oracle.OracleExtractor(**cfg)
    try:
        mono, kps, desc = e(img, None, (0, 1000))
        mono_r, kps_r, desc_r = o.extract(np.ascontiguousarray(img), (0, 1000))
        pyr = o.pyramid(np.ascontiguousarray(img))
        cands = []
        for l in range(cfg["nlevels"]):
            c_ref = o.level_candidates(pyr[l])
            assert np.array_equal(e.level_candidates(l), c_ref), "FAST candidates level %d (%dx%d)" % ((l,) + pyr[l].shape)
            cands.append(c_ref)
        assert mono == mono_r
        assert kps.tobytes() == kps_r.tobytes()
        assert np.array_equal(desc, desc_r)
        return pyr, cands
    finally:
        e.close()


def cell_grid(h, w):
    """The FAST cell grid of a level (ORBextractor.cc:771-803) as orbx_configure groups it: per group the number of valid
    cells, and the cell width."""
    width, height = w - 32, h - 32
    nCols, nRows = width // 30, height // 30
    wCell, hCell = -(-width // nCols), -(-height // nRows)
    maxBX, maxBY = w - 16, h - 16

    def valid(ci, cj):
        iniX, iniY = 16 + cj * wCell, 16 + ci * hCell
        tw = min(iniX + wCell + 6, maxBX) - iniX
        th = min(iniY + hCell + 6, maxBY) - iniY
        return not (iniX >= maxBX - 6 or iniY >= maxBY - 3 or tw - 6 <= 0 or th - 6 <= 0)

    sx = 2 if 3 + 2 * wCell + 6 <= 80 else 1
    sy = 2 if 2 * hCell + 6 <= 76 else 1
    counts = []
    for ci in range(0, nRows, sy):
        for cj in range(0, nCols, sx):
            counts.append(sum(valid(a, b) for a in range(ci, min(ci + sy, nRows)) for b in range(cj, min(cj + sx, nCols))))
    return counts, wCell


def test_dense_noise_queue_wraps(pkg, oracle):
    """Binary noise: most pixels pass the compass pre-test, so every cell's survivor queue wraps many times per detection."""
    rng = np.random.default_rng(71)
    img = (rng.integers(0, 2, (480, 752), dtype=np.uint8) * 255).astype(np.uint8)
    _, cands = check_levels(pkg, oracle, img)
    assert len(cands[0]) > 3000


def test_dot_grid_many_corners_per_cell(pkg, oracle):
    """Isolated bright dots every 4 pixels: ~56 corners in a 30 x 30 cell, all with the same score (NMS ties against the
    dots' own flanks), emitted in raster order through many ballots of one wavefront."""
    img = np.full((480, 752), 40, np.uint8)
    img[1::4, 2::4] = 230
    _, cands = check_levels(pkg, oracle, img)
    assert len(cands[0]) > 10000


def test_fallback_in_one_cell_of_a_group(pkg, oracle):
    """Noise whose odd-row, odd-column cells of level 0 (30 x 32 px) are compressed to +-9 grey levels: those cells have corners
    only below iniThFAST, so in each 2 x 2 group exactly one cell needs the minThFAST detection, and its wavefront runs it while
    the other three are done."""
    rng = np.random.default_rng(72)
    img = rng.integers(0, 256, (480, 752), dtype=np.uint8)
    for ci in range(1, 14, 2):
        for cj in range(1, 24, 2):
            y0, x0 = 16 + 32 * ci, 16 + 30 * cj      # the cell's whole window: interior and its 3-px ring
            blk = img[y0:y0 + 38, x0:x0 + 36].astype(np.float32)
            img[y0:y0 + 38, x0:x0 + 36] = np.clip(128.0 + (blk - 128.0) * 0.07, 0, 255).astype(np.uint8)
    _, cands = check_levels(pkg, oracle, img)
    c0 = cands[0]
    assert (c0[:, 2] < EUROC["iniThFAST"]).sum() > 300 and (c0[:, 2] >= EUROC["iniThFAST"]).sum() > 10000


@pytest.mark.parametrize("H,W,sf", [(241, 377, 1.2), (103, 131, 1.2), (91, 150, 1.3), (200, 230, 1.5), (333, 517, 1.1)])
def test_partial_groups_and_wide_cells(pkg, oracle, frame, H, W, sf):
    """Sizes and scale factors whose levels have groups of 1 and 2 valid cells (idle wavefronts) and cells wider than 35 px
    (1 x N groups).  A group never has exactly 3: a cell's validity depends on its column and its row separately."""
    img = frame(1005, H, W)
    cfg = dict(nfeatures=500, scaleFactor=sf, nlevels=6, iniThFAST=20, minThFAST=7)
    pyr, _ = check_levels(pkg, oracle, img, cfg)
    sizes, wide = set(), False
    for p in pyr:
        if p.shape[0] < 62 or p.shape[1] < 62:
            continue
        counts, wCell = cell_grid(*p.shape)
        sizes.update(counts)
        wide |= wCell > 35
    assert sizes & {1, 2} or wide


def test_partial_groups_coverage():
    """The size list above reaches every group shape (CPU-only arithmetic on the cell grid)."""
    sizes, wide = set(), False
    for H, W, sf in [(241, 377, 1.2), (103, 131, 1.2), (91, 150, 1.3), (200, 230, 1.5), (333, 517, 1.1)]:
        for l in range(6):
            s = sf ** -l
            h, w = int(round(H * s)), int(round(W * s))
            if h < 62 or w < 62:
                continue
            counts, wCell = cell_grid(h, w)
            sizes.update(counts)
            wide |= wCell > 35
    assert {1, 2, 4} <= sizes and 3 not in sizes and wide


@pytest.mark.parametrize("pad", [1, 3])
def test_unaligned_rows(pkg, oracle, frame, capfd, monkeypatch, pad):
    """A row pitch that is not a multiple of 4 and an unaligned first row.  orbx_extract copies such a view into its aligned staging
    buffer, so the same view also goes through the batch API, which reads level 0 in place: there level 0 takes the byte-wise tile
    path (the library's form line reports no aligned level-0 frame)."""
    import torch
    src = frame(1006)
    big = np.zeros((480, 752 + 2 * pad + 1), np.uint8)
    view = big[:, pad:pad + 752]
    view[:] = src
    assert view.strides[0] % 4 != 0
    check_levels(pkg, oracle, view)
    monkeypatch.setenv("ORBHIP_PRINT_EXTRACT_FORMS", "1")
    e = pkg.ORBextractor(**EUROC)
    o = oracle.OracleExtractor(**EUROC)
    try:
        cap = e.configure(480, 752, 1)
        d_big = torch.from_numpy(big).cuda()
        d_kps = torch.zeros((cap, 7), dtype=torch.int32, device="cuda")
        d_desc = torch.zeros((cap, 32), dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
        capfd.readouterr()
        e.extract_batch_device(d_big.data_ptr() + pad, 480, 752, view.strides[0], 480 * view.strides[0], 1, d_kps.data_ptr(), d_desc.data_ptr(),
                               d_cnt.data_ptr(), cap, (0, 1000), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        forms = read_forms(capfd.readouterr().err)
        assert len(forms) == 1 and forms[0]["aligned0"] == 0 and forms[0]["blur0dma"] == 0, forms
        img = np.ascontiguousarray(view)
        pyr = o.pyramid(img)
        for l in range(EUROC["nlevels"]):
            assert np.array_equal(e.level_candidates(l), o.level_candidates(pyr[l])), "batch API: FAST candidates level %d" % l
        mono_r, kps_r, desc_r = o.extract(img, (0, 1000))
        n = int(d_cnt[0])
        assert n == len(kps_r) and int(d_cnt[1]) == mono_r
        assert d_kps[:n].cpu().numpy().tobytes() == kps_r.tobytes()
        assert np.array_equal(d_desc[:n].cpu().numpy(), desc_r)
    finally:
        e.close()
