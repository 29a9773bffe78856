"""The launch form of orbx_extract_batch_device, two ways.

* `read_forms` parses the line the library prints per call when ORBHIP_PRINT_EXTRACT_FORMS is set:
      orbhip: extract nframes N pyramid P octree T/C aligned0 A blur0dma D
  P is `chain` (k_pyramid_chain), `none` (one level) or the k_resize form of levels 1 .. nlevels-1, comma-separated: `2p16` / `2p8`
  (two-pass, 16- or 8-row tiles) or `1p` (one-pass).  T is k_octree's workgroup size (1024 / 256), C `lds` or `global` (the level's
  cell offsets in LDS or not).  A counts the frames whose level-0 plane is dword-aligned (base and stride), D those whose level 0
  takes k_blur's LDS-DMA tile load.
* `resize_plan` replays orbx_configure's host arithmetic for k_resize (level sizes, the y table, a tile's source rows, the LDS stage)
  and the launch-time choice in orbx_extract_batch_device, so that CPU tests can reason about which branches a geometry reaches."""
import re

import numpy as np

FORM = re.compile(r"orbhip: extract nframes (\d+) pyramid (\S+) octree (1024|256)/(lds|global) aligned0 (\d+) blur0dma (\d+)")

RESIZE_ROWS_MAX = 16
RESIZE_MAXSRC = 32
ORB_LDS_LIMIT = 160 * 1024


def read_forms(text):
    """All form lines in captured stderr, as dicts (in call order)."""
    out = []
    for m in FORM.finditer(text):
        pyr = m.group(2)
        out.append(dict(nframes=int(m.group(1)), pyramid=pyr if pyr in ("chain", "none") else tuple(pyr.split(",")),
                        octree=(int(m.group(3)), m.group(4)), aligned0=int(m.group(5)), blur0dma=int(m.group(6))))
    return out


def _align(v, a):
    return (v + a - 1) // a * a


def level_sizes(rows, cols, sf, nlevels):
    """(h, w) of every level as orbx_create / orbx_configure derive them (float scale table built in double, cvRound = half-even)."""
    scale = [np.float32(1.0)]
    for _ in range(1, nlevels):
        scale.append(np.float32(float(scale[-1]) * float(np.float32(sf))))
    out = []
    for s in scale:
        inv = np.float32(1.0) / s
        out.append((int(np.rint(np.float32(rows) * inv)), int(np.rint(np.float32(cols) * inv))))
    return out


def _src_rows(sy, sh, h, tile):
    m = 0
    for dy0 in range(0, h, tile):
        n = min(tile, h - dy0)
        f = min(max(int(sy[dy0]), 0), sh - 1)
        la = min(max(int(sy[dy0 + n - 1]) + 1, 0), sh - 1)
        m = max(m, la - f + 1)
    return m


def resize_level(sh, sw, h, w):
    """k_resize's choice for one level (h x w) made from the one below (sh x sw).  Returns a dict with the tile height, the tile's
    source rows, the two-pass LDS size and the three conditions of the launch; `form` is `2p16`, `2p8` or `1p`."""
    scale_y = 1.0 / (h / sh)
    sy = np.floor(((np.arange(h, dtype=np.float64) + 0.5) * scale_y - 0.5).astype(np.float32)).astype(np.int64)
    wq = (w + 3) & ~3
    row_bytes = _align(sw + 4, 16)
    t_pitch = _align(wq * 2, 8)
    rows = RESIZE_ROWS_MAX
    src = _src_rows(sy, sh, h, rows)
    if src * (row_bytes + t_pitch) > 64 * 1024 or src > RESIZE_MAXSRC:
        rows = 8
        src = _src_rows(sy, sh, h, 8)
    lds2 = _align(src * row_bytes + src * t_pitch, 16) + 16 * RESIZE_ROWS_MAX
    srcrows_over = src > RESIZE_MAXSRC
    ratio_over = sw / w >= 3.0
    lds_over = lds2 > ORB_LDS_LIMIT - 1024
    two = not (srcrows_over or ratio_over or lds_over)
    return dict(rows=rows, src=src, lds2=lds2, srcrows_over=srcrows_over, ratio_over=ratio_over, lds_over=lds_over,
                form=("2p%d" % rows) if two else "1p")


def resize_plan(rows, cols, sf, nlevels):
    """resize_level for levels 1 .. nlevels-1 of a rows x cols image."""
    sz = level_sizes(rows, cols, sf, nlevels)
    return [resize_level(sz[l - 1][0], sz[l - 1][1], sz[l][0], sz[l][1]) for l in range(1, nlevels)]


def resize_forms(rows, cols, sf, nlevels):
    return tuple(p["form"] for p in resize_plan(rows, cols, sf, nlevels))
