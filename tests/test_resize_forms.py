"""k_resize's form choice, replayed on the host (tests/extract_forms.py): every condition of the launch-time choice in
orbx_extract_batch_device is reached by a geometry that tests/test_gpu_batch_layouts.py runs (and pins through the library's own form
line), and the row-record padding of the two-pass LDS stage."""
import numpy as np

from extract_forms import level_sizes, resize_forms, resize_plan, resize_level, ORB_LDS_LIMIT


def test_level_sizes_match_reference_rounding():
    assert level_sizes(480, 752, 1.2, 8) == [(480, 752), (400, 627), (333, 522), (278, 435), (231, 363), (193, 302), (161, 252), (134, 210)]
    assert level_sizes(240, 11, 4.5, 3) == [(240, 11), (53, 2), (12, 1)]


def test_headline_forms():
    assert resize_forms(480, 752, 1.2, 8) == ("2p16",) * 7                      # EuRoC
    assert resize_forms(512, 512, 1.2, 8) == ("2p16",) * 7                      # TUM-VI
    assert resize_forms(376, 1241, 1.2, 8) == ("2p8",) + ("2p16",) * 6          # KITTI: level 1's 16-row stage is above 64 KB
    assert resize_forms(4096, 4096, 1.2, 8) == ("2p8",) * 7


def test_source_row_limit_reached_below_ratio_3():
    """resizeSrcRows > RESIZE_MAXSRC with a horizontal ratio below 3: a 2-column level made 1 column wide while its 8-row tiles span
    33 source rows.  Only degenerate widths (no FAST cell) get there: for real images the two ratios agree and 8 rows at a ratio
    below 3 span at most 7 * 3 + 3 = 24 source rows."""
    p = resize_plan(240, 11, 4.5, 3)
    assert p[1]["srcrows_over"] and not p[1]["ratio_over"] and not p[1]["lds_over"] and p[1]["form"] == "1p"
    for sf in (1.1, 1.2, 1.5, 2.0, 2.6, 2.9):
        for rows, cols in ((480, 752), (376, 1241), (2000, 3000), (4096, 4096)):
            assert not any(q["srcrows_over"] for q in resize_plan(rows, cols, sf, 4))


def test_ratio_condition():
    p = resize_plan(600, 900, 3.3, 2)[0]
    assert p["ratio_over"] and not p["srcrows_over"] and p["form"] == "1p"
    assert resize_forms(500, 700, 2.6, 3) == ("2p8", "2p8")                     # the config matrix's 2.6 case: two-pass, 8-row tiles


def test_lds_condition_margin():
    """lds2 > ORB_LDS_LIMIT - 1024 has not been found reachable: at the widest levels (4096 columns) and every scale factor whose
    horizontal ratio stays below 3 the two-pass stage keeps a margin."""
    worst = 0
    for sf in np.arange(1.02, 3.0, 0.02):
        for rows in (1024, 2048, 4096):
            q = resize_plan(rows, 4096, float(sf), 2)[0]
            if not q["ratio_over"]:
                worst = max(worst, q["lds2"])
    assert worst < ORB_LDS_LIMIT - 1024


def test_row_records_16_byte_aligned():
    """KITTI level 1 (1034 columns: tPitch 2072 = 8 mod 16) with 11 source rows per 8-row tile, and EuRoC level 7 (210 columns, 21
    source rows): the row records start at the next multiple of 16, and the LDS size counts the padding."""
    sz = level_sizes(376, 1241, 1.2, 8)
    q = resize_level(sz[0][0], sz[0][1], sz[1][0], sz[1][1])
    row_bytes, t_pitch = 1248, 2072
    assert q["form"] == "2p8" and q["src"] == 11 and (q["src"] * t_pitch) % 16 == 8
    assert q["lds2"] == q["src"] * row_bytes + q["src"] * t_pitch + 8 + 16 * 16
    sz = level_sizes(480, 752, 1.2, 8)
    q = resize_level(sz[6][0], sz[6][1], sz[7][0], sz[7][1])
    assert q["form"] == "2p16" and q["src"] == 21 and (q["src"] * 424) % 16 == 8
