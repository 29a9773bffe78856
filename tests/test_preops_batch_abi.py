"""CPU: orbx_clahe_batch_device and orbx_remap_linear_batch_device exist on both sides of the ABI, their refusals that need no device
(host arrays stand in for device buffers: a refused call never touches them), the empty batch, and the table rows a band of the
blend kernel stages (orbx_clahe_band_lut_rows, the launch code's own arithmetic) against brute force over every row of the band.
The refusals worth checking next to live buffers are in tests/test_gpu_preops_batch.py::test_refusals_with_live_buffers."""
import inspect
import os

import numpy as np
import pytest

from conftest import ROOT


def test_symbols_and_mirrors(pkg):
    L = pkg.load()
    for name, nargs in (("orbx_clahe_batch_device", 14), ("orbx_remap_linear_batch_device", 15), ("orbx_clahe_band_lut_rows", 6)):
        assert name in pkg.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    sig = inspect.signature(pkg.clahe_batch_device)
    assert list(sig.parameters) == ["nframes", "d_src", "rows", "cols", "src_stride", "src_frame_stride", "clip_limit", "tiles_x", "tiles_y", "d_lut",
                                    "d_dst", "dst_stride", "dst_frame_stride", "stream"]
    assert sig.parameters["stream"].default is None
    sig = inspect.signature(pkg.remap_linear_batch_device)
    assert list(sig.parameters) == ["nframes", "d_src", "src_rows", "src_cols", "src_stride", "src_frame_stride", "d_mapx", "d_mapy", "map_stride_elems",
                                    "rows", "cols", "d_dst", "dst_stride", "dst_frame_stride", "stream"]
    assert sig.parameters["stream"].default is None
    assert pkg.CLAHE_BAND_ROWS >= 1 and pkg.REMAP_FRAME_CHUNK >= 1
    hdr = open(os.path.join(ROOT, "include", "orbhip.h")).read()          # the mirror's constants are the header's
    assert "#define ORBX_CLAHE_BAND_ROWS %d\n" % pkg.CLAHE_BAND_ROWS in hdr and "#define ORBX_REMAP_FRAME_CHUNK %d\n" % pkg.REMAP_FRAME_CHUNK in hdr


def test_clahe_refusals_without_device(pkg):
    n, H, W = 3, 24, 40
    src, dst, lut = np.full(n * H * W + 8, 7, np.uint8), np.full(n * H * W + 8, 9, np.uint8), np.full(n * 64 * 256, 5, np.uint8)
    good = dict(nframes=n, d_src=src.ctypes.data, rows=H, cols=W, src_stride=W, src_frame_stride=H * W, clip_limit=3.0, tiles_x=8, tiles_y=8,
                d_lut=lut.ctypes.data, d_dst=dst.ctypes.data, dst_stride=W, dst_frame_stride=H * W)
    bad = [dict(d_src=0), dict(d_dst=0), dict(d_lut=0), dict(nframes=-1), dict(tiles_x=1, tiles_y=257), dict(tiles_x=257, tiles_y=1),
           dict(tiles_x=W + 1, tiles_y=1),                                   # cols < tiles_x
           dict(tiles_x=1, tiles_y=H + 1),                                   # rows < tiles_y
           dict(tiles_x=0), dict(tiles_y=0), dict(rows=0), dict(cols=0), dict(src_stride=W - 1), dict(dst_stride=W - 1),
           dict(src_frame_stride=H * W - 1), dict(dst_frame_stride=H * W - 1),                                      # one byte short
           dict(src_stride=W + 3, src_frame_stride=(H - 1) * (W + 3) + W - 1),
           dict(clip_limit=float("nan")), dict(clip_limit=-1.0),
           dict(d_dst=src.ctypes.data + 1),                                  # overlap that is not the in-place form
           dict(d_dst=src.ctypes.data, dst_stride=W + 1, dst_frame_stride=H * (W + 1)),
           dict(d_dst=src.ctypes.data + (n - 1) * H * W + (H - 1) * W + W - 1)]        # the last source byte is the first destination byte
    for c in bad:
        with pytest.raises(ValueError):
            pkg.clahe_batch_device(**dict(good, **c))
    assert pkg.clahe_batch_device(**dict(good, nframes=0)) == 0              # nothing to do, nothing launched
    assert pkg.clahe_batch_device(**dict(good, nframes=0, d_dst=src.ctypes.data)) == 0
    # a batch of one does not look at the frame strides; this one is refused for its overlap alone
    with pytest.raises(ValueError):
        pkg.clahe_batch_device(**dict(good, nframes=1, src_frame_stride=0, dst_frame_stride=0, d_dst=src.ctypes.data + W))
    assert (src == 7).all() and (dst == 9).all() and (lut == 5).all()


def test_remap_refusals_without_device(pkg):
    n, SH, SW, H, W = 3, 20, 36, 16, 28
    src, dst = np.full(n * SH * SW + 8, 7, np.uint8), np.full(n * H * W + 8, 9, np.uint8)
    mx, my = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    good = dict(nframes=n, d_src=src.ctypes.data, src_rows=SH, src_cols=SW, src_stride=SW, src_frame_stride=SH * SW, d_mapx=mx.ctypes.data,
                d_mapy=my.ctypes.data, map_stride_elems=W, rows=H, cols=W, d_dst=dst.ctypes.data, dst_stride=W, dst_frame_stride=H * W)
    bad = [dict(d_src=0), dict(d_dst=0), dict(d_mapx=0), dict(d_mapy=0), dict(nframes=-1), dict(src_rows=0), dict(src_cols=0), dict(rows=0), dict(cols=0),
           dict(src_stride=SW - 1), dict(dst_stride=W - 1), dict(map_stride_elems=W - 1),
           dict(src_frame_stride=SH * SW - 1), dict(dst_frame_stride=H * W - 1),                                      # one byte short
           dict(src_cols=32768, src_stride=32768, src_frame_stride=SH * 32768), dict(src_rows=32768, src_frame_stride=32768 * SW),
           dict(d_dst=src.ctypes.data),                                                                                # in place
           dict(d_dst=src.ctypes.data + 5),
           dict(d_dst=src.ctypes.data + (n - 1) * SH * SW + (SH - 1) * SW + SW - 1),                                   # one shared byte
           dict(d_dst=src.ctypes.data - ((n - 1) * H * W + (H - 1) * W + W - 1))]                                      # ... at the other end
    for c in bad:
        with pytest.raises(ValueError):
            pkg.remap_linear_batch_device(**dict(good, **c))
    assert pkg.remap_linear_batch_device(**dict(good, nframes=0)) == 0
    assert (src == 7).all() and (dst == 9).all()


def band_rows_brute(rows, tiles_y, y0, y1):
    """Every table row the blend of k_clahe_interp reads for the image rows y0 .. y1, one image row at a time (float32, each operation
    rounded on its own)."""
    erows = rows if rows % tiles_y == 0 else rows + tiles_y - rows % tiles_y
    inv_th = np.float32(1) / np.float32(erows // tiles_y)
    need = set()
    for y in range(y0, y1 + 1):
        ty1 = int(np.floor(np.float32(np.float32(y) * inv_th) - np.float32(0.5)))
        need.add(max(ty1, 0))
        need.add(min(ty1 + 1, tiles_y - 1))
    return need


@pytest.mark.parametrize("rows,tiles_y", [(64, 16), (67, 8), (300, 5), (512, 8), (480, 8)])
def test_band_table_rows_against_brute_force(pkg, rows, tiles_y):
    """The staged range [first, first + count) holds every table row the band reads and starts and ends on one that is read (nothing
    staged in vain at either end), for every band start and for the band height the kernel uses as well as 1, 4 and 37."""
    seen = set()
    for band in sorted({pkg.CLAHE_BAND_ROWS, 1, 4, 37}):
        for y0 in range(rows):
            y1 = min(y0 + band, rows) - 1
            first, count = pkg.clahe_band_lut_rows(rows, tiles_y, y0, y1)
            need = band_rows_brute(rows, tiles_y, y0, y1)
            assert first == min(need) and first + count - 1 == max(need), (band, y0, first, count, sorted(need))
            assert 0 <= first and first + count <= tiles_y
            seen.add(count)
    assert 1 in seen and 2 in seen          # a band inside the first or last half tile row reads one table row, one inside a tile row two
    if (rows, tiles_y) == (64, 16):
        assert max(seen) >= 5               # 4-pixel tiles: a band spans several tile rows
    for c in (dict(y0=-1), dict(y1=rows), dict(y0=5, y1=4), dict(tiles_y=0), dict(tiles_y=rows + 1)):
        with pytest.raises(ValueError):
            pkg.clahe_band_lut_rows(**dict(dict(rows=rows, tiles_y=tiles_y, y0=0, y1=0), **c))
