"""k_resize's two-pass form where its loops split into full trips and a tail: pass 1 takes the staged source rows four at a time and
then nsrc % 4 of them, pass 2 takes a row's whole quads 32 at a time, then the quads that are left and the row's tail bytes.

Every case is a batch call (nlevels * nframes > 32: one k_resize launch per level) and compares every frame's pyramid and blurred
levels byte for byte with the oracle (test_gpu_tile_records.run_and_check).  What a geometry reaches is worked out on the CPU from
orbx_configure's arithmetic (extract_forms) and asserted in a test that needs no GPU."""
import numpy as np
import pytest

from extract_forms import level_sizes, resize_plan
from test_gpu_tile_records import cfg_of, frames_of, run_and_check

# (name, H, W, scaleFactor, nlevels, nframes)
CASES = [
    # source rows per tile = 0, 1, 3 (mod 4); last tiles of 12 rows; widths 117 and 97: 29 and 24 quads + 1 byte
    ("140x110", 110, 140, 1.2, 3, 11),
    # 1, 2, 3 (mod 4); last tiles of 5 and 14 rows; widths 104 and 80: no tail bytes
    ("135x131 sf1.3", 131, 135, 1.3, 3, 11),
    # 0, 2, 3 (mod 4); a last tile of 2 rows; width 119: 29 quads + 3 bytes
    ("131x90 sf1.1", 90, 131, 1.1, 3, 11),
    # widths 114 and 99: 2 and 3 tail bytes; last tiles of 13 and 15 rows
    ("131x125 sf1.15", 125, 131, 1.15, 3, 11),
    # width 131: one full trip of 32 quads, none left over, the tail bytes on lane 0
    ("157x90", 90, 157, 1.2, 3, 11),
    # width 127: 31 quads left over and the tail bytes on lane 31
    ("152x97", 97, 152, 1.2, 3, 11),
    # level 1 is 1033 wide: pass 1's third column trip (the x table read directly), eight full quad trips in pass 2; 8-row tiles of 10 and 11 rows
    ("1240x48", 48, 1240, 1.2, 2, 17),
]


def tiles(sh, h, tile):
    """(source rows staged, output rows) of every row tile of a level of h rows made from one of sh rows (orbx_configure's y table)."""
    scale_y = 1.0 / (h / sh)
    sy = np.floor(((np.arange(h, dtype=np.float64) + 0.5) * scale_y - 0.5).astype(np.float32)).astype(np.int64)
    out = []
    for dy0 in range(0, h, tile):
        n = min(tile, h - dy0)
        first = min(max(int(sy[dy0]), 0), sh - 1)
        last = min(max(int(sy[dy0 + n - 1]) + 1, 0), sh - 1)
        out.append((last - first + 1, n))
    return out


def reach(case):
    """What the levels 1 .. of a case reach: residues of the staged rows mod 4, output rows of the tiles, (full quad trips, quads left
    over, tail bytes) per level, and the widest level."""
    _, H, W, sf, nlevels, _ = case
    sz = level_sizes(H, W, sf, nlevels)
    plan = resize_plan(H, W, sf, nlevels)
    res, rows, quads = set(), set(), set()
    for l in range(1, nlevels):
        assert plan[l - 1]["form"] in ("2p16", "2p8")
        for nsrc, n in tiles(sz[l - 1][0], sz[l][0], plan[l - 1]["rows"]):
            res.add(nsrc % 4)
            rows.add(n)
        w = sz[l][1]
        quads.add(((w >> 2) >> 5, (w >> 2) & 31, w & 3))
    return res, rows, quads, max(s[1] for s in sz[1:])


def test_cases_reach_every_trip_shape():
    res, rows, quads, widest = set(), set(), set(), 0
    for case in CASES:
        r, n, q, w = reach(case)
        res |= r
        rows |= n
        quads |= q
        widest = max(widest, w)
    assert res == {0, 1, 2, 3}                                    # pass 1: full trips only, and every tail length
    assert min(rows) < 16 and 16 in rows and 8 in rows            # short last tiles
    assert {t for _, _, t in quads} == {0, 1, 2, 3}               # pass 2: every number of tail bytes
    assert (1, 0, 3) in quads and (0, 31, 3) in quads             # the tail on lane 0 behind a full trip, and on lane 31
    assert any(f >= 2 for f, _, _ in quads) and any(f == 0 for f, _, _ in quads)
    assert widest > 1024                                          # pass 1: more than two column pairs per thread


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_planes(pkg, oracle, capfd, monkeypatch, case):
    monkeypatch.setenv("ORBHIP_PRINT_EXTRACT_FORMS", "1")
    _, H, W, sf, nlevels, n = case
    cfg = cfg_of(sf, nlevels)
    e = pkg.ORBextractor(**cfg)
    try:
        run_and_check(e, oracle, capfd, cfg, frames_of(410, n, H, W), aligned=W % 4 == 0)
    finally:
        e.close()
