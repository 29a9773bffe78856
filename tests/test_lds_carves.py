"""Dynamic LDS: every kernel's carve type (csrc/*_kernels.h, orb_sort.h) against the byte counts the host formulas gave before the carve
types existed, restated here as plain arithmetic, and against the CU's 160 KiB together with the kernels' static LDS.  No GPU:
tests/support/lds_carves.hip prints the carves on the host, the static sizes come from the compiled device code's metadata."""
import importlib
import os
import re
import subprocess

import pytest

from conftest import PKG, ROOT
from device_code import static_lds

KIB = 1024
GRID_CELLS, MATCH_NT, MATCH_TOPK, WALK_LIST, WALK_MAX_N, RESIZE_ROWS_MAX, MAX_KEYPOINTS = 64 * 48, 256, 8, 16, 2048, 16, 15360
SCAN_PLAIN, SCAN_UR, SCAN_FISHEYE, SCAN_FUSE = 0, 1, 2, 3


def align_up(x, a):
    return (x + a - 1) // a * a


# ---- the host formulas as they were (search_batch, resize_form, orbx_configure, the launch sites) ----
def resolve_small(n, partner):
    return 4 * ((n + 1) + n + (n + 1) // 2 + ((n + 1) // 2 + 1 if partner else 0) + 2)


def resolve_big(n, partner):
    return resolve_small(n, partner) + 4 * ((n + 3) // 4) + 48 * n


def resolve_fused(n, partner):
    return resolve_small(n, partner) + 4 * ((n + 3) // 4) + 4 * n


def resolve_form(n, partner, fused_ok):
    """(ldscand, fused, bytes) of search_batch"""
    ldscand = resolve_big(n, partner) <= 136 * KIB
    fused = fused_ok and resolve_fused(n, partner) <= 138 * KIB
    return ldscand, fused, resolve_fused(n, partner) if fused else resolve_big(n, partner) if ldscand else resolve_small(n, partner)


def walk_bytes(capn, mode, lpq):
    ur = mode in (SCAN_UR, SCAN_FUSE)   # o.fuse || M.u_right of a problem that is launched in this mode
    return 4 * (GRID_CELLS + 4) + (12 + (4 if ur else 0)) * capn + 2 * WALK_LIST * MATCH_NT + (4 * MATCH_TOPK * MATCH_NT if lpq > 1 else 0)


def resize_bytes(max_src, src_w, wq, two_pass):
    row_bytes, t_pitch = align_up(src_w + 4, 16), align_up(wq * 2, 8)
    return max_src * row_bytes + align_up(max_src * t_pitch, 16) + 16 * RESIZE_ROWS_MAX if two_pass else wq * 8


def octree_bytes(cap, head, cells):
    return head + 40 * cap + 128 + (4 * (cells + 1) if cells else 0)


def oct_table_bytes(n_ini, oct_d=5):   # OCT_TABLE_BYTES of orb_common.h, 16-byte aligned as orbx_configure takes it
    pyr_off0 = n_ini * (((1 << (2 * oct_d + 2)) - 4) // 3)
    return align_up((2 * pyr_off0 + 2 * n_ini + 3) & ~3, 16)


def sort_bytes(n):
    p2 = 2
    while p2 < n:
        p2 <<= 1
    return 8 * p2


def largest(f, bound):
    """the largest n with f(n) <= bound (f increasing)"""
    lo, hi = 0, 1 << 20
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if f(mid) <= bound else (lo, mid - 1)
    return lo


RESOLVE_MAXN = {}
for _p in (False, True):
    _at = [largest(lambda n: resolve_big(n, _p), 136 * KIB), largest(lambda n: resolve_fused(n, _p), 138 * KIB), largest(lambda n: resolve_small(n, _p), 152 * KIB)]
    RESOLVE_MAXN[_p] = sorted({1, 2, 3, 4, 5, 2047, 2048, 2049, MAX_KEYPOINTS} | {n + d for n in _at for d in (0, 1)})

# EuRoC level 1 from level 0: 752 -> 627 columns, wq = 628, tPitch 1256 = 16 * 78 + 8, so an odd row count needs the padding in front
# of the row records; wq = 632: tPitch 1264 = 16 * 79, no padding at any row count
RESIZE_SHAPES = [(21, 752, 628, 1), (20, 752, 628, 1), (21, 752, 632, 1), (0, 752, 628, 0)]
# one node; 100 nodes with the code tables of nIni = 2 (5472 bytes) for a head, beyond 32 * 100; 1003 nodes (nfeatures 1000)
OCTREE_SHAPES = [(cap, head, nt, cells) for cap, head in ((1, 32), (100, oct_table_bytes(2)), (1003, 32 * 1003)) for nt in (256, 1024) for cells in (0, 300)]


def requests():
    req = ["consts"]
    for p in (False, True):
        for n in RESOLVE_MAXN[p]:
            req += ["resolve %d %d %d %d" % (n, p, cand, fused) for cand, fused in ((0, 0), (1, 0), (0, 1))]
            req += ["form %d %d %d" % (n, p, ok) for ok in (0, 1)]
    req += ["init %d" % n for n in (1, 2, 2048, MAX_KEYPOINTS)]
    req += ["walk %d %d %d" % (capn, mode, lpq) for capn in (8, 16, WALK_MAX_N) for mode in range(4) for lpq in (1, 4)]
    req += ["resize %d %d %d %d" % s for s in RESIZE_SHAPES]
    req += ["chain 160 320 9", "chain 0 0 0", "chain 65536 16384 400"]
    req += ["clahe 8 8", "clahe 3 5", "clahe 256 1"]
    req += ["octree %d %d %d %d" % s for s in OCTREE_SHAPES]
    req += ["sort %d" % n for n in (1, 2, 3, 16384)]
    return req


@pytest.fixture(scope="module")
def carves(tmp_path_factory):
    """{request: ([(region, off, size, align, over)], bytes)} from the host program"""
    build = importlib.import_module(PKG + ".build")
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("lds_carves") / "lds_carves")
    subprocess.check_call([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O0", "-Wall", "-Wno-unused-function", "-Wno-pass-failed", "-I", os.path.join(ROOT, "include"),
                           "-I", build.CSRC, os.path.join(ROOT, "tests", "support", "lds_carves.hip"), "-o", exe])
    out = subprocess.run([exe], input="\n".join(requests()) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    got = {}
    for line in out:
        req, body, nbytes = (s.strip() for s in line.split("|"))
        got[req] = ([(f[0],) + tuple(int(x) for x in f[1:]) for f in (w.split(":") for w in body.split())], int(nbytes))
    assert sorted(got) == sorted(set(requests()))
    return got


def layouts(carves):
    return {r: v for r, v in carves.items() if r.split()[0] not in ("consts", "form")}


def test_layout(carves):
    """Regions in order, none over another unless declared so, every offset a multiple of its alignment, bytes behind the last region."""
    for req, (regions, nbytes) in layouts(carves).items():
        end = 0
        for name, off, size, align, over in regions:
            assert off % align == 0 and off >= 0 and size >= 0, (req, name)
            assert off + size <= nbytes, (req, name)
            if not over:
                assert off >= end, (req, name)
                end = off + size
    # what is declared to lie over something does: the winners over the child counts, the code form's tables over the whole head, the
    # nodes' cell codes over npos
    for req, (regions, _) in layouts(carves).items():
        if req.startswith("octree"):
            r = {name: (off, size) for name, off, size, _, _ in regions}
            assert sorted(n for n, _, _, _, over in regions if over) == ["best", "codeA", "codeB", "pyr"]
            assert r["best"][0] == r["chcnt"][0] == r["pyr"][0] == 0 and r["pyr"][1] == r["nodeA"][0] and r["best"][1] <= r["chpos"][0] + r["chpos"][1]
            assert r["codeA"][0] == r["npos"][0] and r["codeB"][0] + r["codeB"][1] == r["npos"][0] + r["npos"][1]
        else:
            assert not [n for n, _, _, _, over in regions if over], req


def test_launch_sizes(carves):
    """bytes of every carve = the host formula it replaced."""
    for req, (_, nbytes) in layouts(carves).items():
        kind, *a = req.split()
        a = [int(x) for x in a]
        want = {"resolve": lambda n, p, cand, fused: resolve_fused(n, p) if fused else resolve_big(n, p) if cand else resolve_small(n, p),
                "init": lambda n: 2 * n + 16,
                "walk": walk_bytes,
                "resize": resize_bytes,
                "chain": lambda b0, b1, tab: b0 + b1 + 8 * tab,
                "clahe": lambda rows, tx: rows * tx * 256,
                "octree": lambda cap, head, nt, cells: octree_bytes(cap, head, cells),
                "sort": sort_bytes}[kind](*a)
        assert nbytes == want, (req, nbytes, want)


def test_resize_row_records_are_aligned(carves):
    """The case that went wrong once: 16-byte row records behind a T plane whose size is a multiple of 8 only."""
    for s in RESIZE_SHAPES[:3]:
        regions, _ = carves["resize %d %d %d %d" % s]
        r = {name: (off, size, align) for name, off, size, align, _ in regions}
        assert r["rowRec"][2] == 16 and r["rowRec"][0] % 16 == 0 and r["rowRec"][0] >= r["t"][0] + r["t"][1] and r["rowRec"][1] == 16 * RESIZE_ROWS_MAX
    assert (21 * 1256) % 16 == 8 and (20 * 1256) % 16 == 0 and (21 * 1264) % 16 == 0   # the shapes are the ones meant


def test_admission(carves):
    """The bounds keep their values, and the records-in-LDS, fused and refusal decisions fall where they fell, on both sides of each."""
    consts = {k: v for k, v in ((f[0], f[1]) for f in carves["consts"][0])}
    assert consts == dict(ORB_LDS_LIMIT=160 * KIB, RESOLVE_LDSCAND_MAX=136 * KIB, RESOLVE_FUSED_MAX=138 * KIB, RESOLVE_LDS_MAX=152 * KIB, OCT_LDS_MAX=160 * KIB - 256,
                          OCT_CELLS_LDS_MAX=96 * KIB, OCT_GROWN_HEAD_MAX=32 * KIB, CHAIN_LDS_MAX=64 * KIB, RESIZE_STAGE_MAX=64 * KIB, RESIZE_LDS_MAX=160 * KIB - 1024,
                          GRID_CELLS=GRID_CELLS, MATCH_NT=MATCH_NT, MATCH_TOPK=MATCH_TOPK, WALK_LIST=WALK_LIST, WALK_MAX_N=WALK_MAX_N, RESIZE_ROWS_MAX=RESIZE_ROWS_MAX,
                          ORBM_MAX_KEYPOINTS=MAX_KEYPOINTS)
    seen = set()
    for p in (False, True):
        for n in RESOLVE_MAXN[p]:
            for ok in (0, 1):
                fields, nbytes = carves["form %d %d %d" % (n, p, ok)]
                got = {f[0]: f[1] for f in fields}
                ldscand, fused, want = resolve_form(n, p, bool(ok))
                assert (got["ldscand"], got["fused"], nbytes, got["refused"]) == (int(ldscand), int(fused), want, int(want > 152 * KIB)), (n, p, ok)
                seen.add((ldscand, fused, want > 152 * KIB))
    assert {(True, False, False), (False, False, False), (True, True, False), (False, True, False), (False, False, True)} <= seen   # both sides of each bound


# mangled-name pattern of every dynamic-LDS kernel instance -> the most dynamic LDS the host admits for it: a bound, or the carve at the
# largest shape the host launches the instance with (Key32 frames, and with them every walk and the fused form: at most 2048 keypoints)
def max_dynamic(carves):
    b = lambda req: carves[req][1]
    return {
        r"k_match_walkI5Key32Li\dELi1E": b("walk %d %d 1" % (WALK_MAX_N, SCAN_FUSE)),
        r"k_match_walkI5Key32Li\dELi4E": b("walk %d %d 4" % (WALK_MAX_N, SCAN_FUSE)),
        r"k_match_resolveI5Key32Lb1ELb0E": min(136 * KIB, b("resolve 2048 1 1 0")),
        r"k_match_resolveI5Key32Lb0ELb0E": b("resolve 2048 1 0 0"),
        r"k_match_resolveI5Key32Lb1ELb1E": min(138 * KIB, b("resolve 2048 1 0 1")),
        r"k_match_resolveI5Key64Lb1ELb0E": 136 * KIB,
        r"k_match_resolveI5Key64Lb0ELb0E": 152 * KIB,
        r"k_init_resolveI5Key\d\dE": b("init %d" % MAX_KEYPOINTS),
        r"k_octreeILi\d+ELb[01]E": 160 * KIB - 256,
        r"k_resize": 160 * KIB - 1024,
        r"k_pyramid_chain": 64 * KIB,
        r"k_clahe_interp(PKh|_batch)": b("clahe 256 1"),   # at most 256 tiles
        r"k_local_kf_walk|k_conn_walk|k_voc_collect|k_kfdb_order": b("sort 16384"),
    }


def test_lds_budget(carves):
    """Static LDS of every dynamic-LDS kernel instance + the most dynamic LDS the host admits for it <= 160 KiB."""
    static = static_lds()
    for pat, dyn in max_dynamic(carves).items():
        hits = {k: v for k, v in static.items() if re.match(r"_Z\d+(?:" + pat + ")", k)}
        assert hits, pat
        for name, fixed in hits.items():
            assert fixed + dyn <= 160 * KIB, (name, fixed, dyn)
