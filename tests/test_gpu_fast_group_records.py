"""k_fast's group records (orbx_configure: one self-contained record per group of up to 2 x 2 cells, read with scalar loads in front
of the tile DMA) against the CPU oracle: counts, keypoint bytes, descriptors and every level's FAST candidates, frame by frame,
byte-equal, at shapes where a wrong record shows."""
import math

import numpy as np
import pytest

from test_gpu_fast_cells import cell_grid

# (rows, cols, levels, scale factor): small images whose cell grids have odd column and row counts
SIZES = [(190, 250, 4, 1.2), (122, 160, 4, 1.2), (110, 112, 3, 1.2), (200, 170, 4, 1.25)]


def cfg_of(nlevels, sf, nfeatures=500, ini=20, mn=7):
    return dict(nfeatures=nfeatures, scaleFactor=sf, nlevels=nlevels, iniThFAST=ini, minThFAST=mn)


def group_shapes(h, w):
    """(cell columns, cell rows, cell width, cell height, [(gx, gy) of every group]) of an h x w level: orbx_configure's grid
    (ORBextractor.cc:771-785) and its grouping rule - two cells share a workgroup in a direction when both fit the LDS tile."""
    width, height = w - 32, h - 32
    nCols, nRows = width // 30, height // 30
    wCell, hCell = math.ceil(width / nCols), math.ceil(height / nRows)
    sx = 2 if 3 + 2 * wCell + 6 <= 80 else 1
    sy = 2 if 2 * hCell + 6 <= 76 else 1
    shapes = [(min(sx, nCols - cj), min(sy, nRows - ci)) for ci in range(0, nRows, sy) for cj in range(0, nCols, sx)]
    return nCols, nRows, wCell, hCell, shapes


def level_sizes(oracle, H, W, nlevels, sf):
    o = oracle.OracleExtractor(**cfg_of(nlevels, sf))
    return [o.level_size(l, W, H)[::-1] for l in range(nlevels)]   # (rows, cols)


def test_sizes_reach_every_group_shape(oracle):
    """CPU arithmetic only: the size list holds 2 x 2, 1 x 2, 2 x 1 and 1 x 1 groups, levels with an odd number of cell columns and
    of cell rows, a level that is one cell, and an odd number of groups per frame."""
    shapes, odd_cols, odd_rows, single, odd_total = set(), False, False, False, False
    for H, W, nl, sf in SIZES:
        total = 0
        for h, w in level_sizes(oracle, H, W, nl, sf):
            assert h >= 62 and w >= 62, "every level has at least one cell"
            nCols, nRows, _, _, sh = group_shapes(h, w)
            assert len(sh) == len(cell_grid(h, w)[0])   # the grouping the older tests derive
            shapes.update(sh)
            total += len(sh)
            odd_cols |= nCols % 2 == 1 and nCols > 1
            odd_rows |= nRows % 2 == 1 and nRows > 1
            single |= nCols == 1 and nRows == 1
        odd_total |= total % 2 == 1
    assert shapes == {(2, 2), (1, 2), (2, 1), (1, 1)}
    assert odd_cols and odd_rows and single and odd_total


class Batch:
    """B frames on the device with any base offset and row stride, extracted through the resident batch API."""

    def __init__(self, imgs, pad=0, row_extra=0):
        import torch
        self.torch = torch
        self.imgs = [np.ascontiguousarray(i) for i in imgs]
        self.B = len(imgs)
        self.H, self.W = imgs[0].shape
        self.stride = self.W + row_extra
        self.fstride = self.H * self.stride
        host = np.zeros(pad + self.B * self.fstride + 64, np.uint8)
        for f, im in enumerate(self.imgs):
            v = host[pad + f * self.fstride:pad + (f + 1) * self.fstride].reshape(self.H, self.stride)
            v[:, :self.W] = im
        self.d = torch.from_numpy(host).cuda()
        self.ptr = self.d.data_ptr() + pad

    def extract(self, e):
        torch = self.torch
        cap = e.configure(self.H, self.W, self.B)
        d_kps = torch.zeros((self.B, cap, 7), dtype=torch.int32, device="cuda")
        d_desc = torch.zeros((self.B, cap, 32), dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros((self.B, 2), dtype=torch.int32, device="cuda")
        e.extract_batch_device(self.ptr, self.H, self.W, self.stride, self.fstride, self.B, d_kps.data_ptr(), d_desc.data_ptr(),
                               d_cnt.data_ptr(), cap, (0, 1000), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d_cnt.cpu().numpy(), d_kps.cpu().numpy(), d_desc.cpu().numpy()

    def check(self, e, o, nlevels):
        """Every frame byte-equal to the oracle's: counts, keypoints, descriptors, and the FAST candidates of every level.
        Returns the oracle's candidates, [frame][level]."""
        cnt, kps, desc = self.extract(e)
        cands = []
        for f, img in enumerate(self.imgs):
            mono_r, kps_r, desc_r = o.extract(img, (0, 1000))
            n = int(cnt[f, 0])
            assert n == len(kps_r) and int(cnt[f, 1]) == mono_r, "frame %d: counts" % f
            assert kps[f, :n].tobytes() == kps_r.tobytes(), "frame %d: keypoints" % f
            assert np.array_equal(desc[f, :n], desc_r), "frame %d: descriptors" % f
            pyr = o.pyramid(img)
            per_level = []
            for l in range(nlevels):
                assert pyr[l].shape == e.level_shape(l)
                c_ref = o.level_candidates(pyr[l])
                assert np.array_equal(e.level_candidates(l, frame=f), c_ref), "frame %d: FAST candidates level %d" % (f, l)
                per_level.append(c_ref)
            cands.append(per_level)
        return cands


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,nl,sf", SIZES)
def test_edge_groups_three_frames(pkg, oracle, frame, H, W, nl, sf):
    """Three different frames per call: the records are shared by the frames, the per-frame strides of the cell counts, slots and
    pyramid are not.  The sizes hold partial groups at the right and bottom edge of a level and one-cell levels."""
    cfg = cfg_of(nl, sf)
    e, o = pkg.ORBextractor(**cfg), oracle.OracleExtractor(**cfg)
    try:
        cands = Batch([frame(2100 + i, H, W) for i in range(3)]).check(e, o, nl)
        assert all(len(c[0]) > 0 for c in cands)
        assert [e.level_shape(l) for l in range(nl)] == level_sizes(oracle, H, W, nl, sf)   # the grids the CPU test derives the shapes from
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pad,row_extra", [(1, 3), (1, 1)])
def test_unaligned_level0(pkg, oracle, frame, pad, row_extra):
    """Level 0 read in place from a buffer whose base is one byte off and whose row stride is no multiple of 4: the byte-wise tile
    path, with level 0's pitch and base from the call's arguments while levels 1.. take theirs from the record."""
    H, W, nl, sf = 122, 160, 4, 1.2
    assert (W + row_extra) % 4 != 0
    cfg = cfg_of(nl, sf)
    e, o = pkg.ORBextractor(**cfg), oracle.OracleExtractor(**cfg)
    try:
        b = Batch([frame(2200 + i, H, W) for i in range(3)], pad=pad, row_extra=row_extra)
        assert b.ptr % 4 != 0
        b.check(e, o, nl)
    finally:
        e.close()


def second_detection_frame(frame, H, W):
    """Left third as it is, middle third compressed to a few grey levels (corners only below iniThFAST), right third flat."""
    img = frame(2300, H, W).copy()
    mid = img[:, W // 3:2 * W // 3].astype(np.float32)
    img[:, W // 3:2 * W // 3] = np.clip(128.0 + (mid - 128.0) * 0.18, 0, 255).astype(np.uint8)
    img[:, 2 * W // 3:] = 97
    return img


@pytest.mark.gpu
def test_second_detection_cells(pkg, oracle, frame):
    """One frame whose level-0 cells are of all three kinds: detected at iniThFAST, filled only by the minThFAST detection, and
    empty after both.  The kind of a cell is read off the oracle's candidates (a first-detection cell holds only responses
    >= iniThFAST, a second-detection cell only smaller ones)."""
    H, W, nl, sf = 190, 250, 4, 1.2
    cfg = cfg_of(nl, sf)
    e, o = pkg.ORBextractor(**cfg), oracle.OracleExtractor(**cfg)
    try:
        cands = Batch([second_detection_frame(frame, H, W)]).check(e, o, nl)
        nCols, nRows, wCell, hCell, _ = group_shapes(H, W)
        c0 = cands[0][0]
        cell = ((c0[:, 1].astype(int) - 3) // hCell) * nCols + (c0[:, 0].astype(int) - 3) // wCell
        strong = set(cell[c0[:, 2] >= cfg["iniThFAST"]].tolist())
        weak = set(cell[c0[:, 2] < cfg["iniThFAST"]].tolist())
        assert not (strong & weak), "a cell is filled by one detection or by the other"
        empty = set(range(nCols * nRows)) - strong - weak
        assert strong and weak and empty, (len(strong), len(weak), len(empty))
    finally:
        e.close()


@pytest.mark.gpu
def test_records_follow_reconfigure(pkg, oracle, frame):
    """Two image sizes on one handle, and the first again: the records are those of the last orbx_configure, not of the first."""
    nl, sf = 4, 1.2
    cfg = cfg_of(nl, sf)
    e, o = pkg.ORBextractor(**cfg), oracle.OracleExtractor(**cfg)
    try:
        a = Batch([frame(2400 + i, 122, 160) for i in range(2)])
        b = Batch([frame(2410 + i, 190, 250) for i in range(3)])
        a.check(e, o, nl)
        b.check(e, o, nl)
        a.check(e, o, nl)
    finally:
        e.close()
