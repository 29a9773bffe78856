"""CPU: MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth for all map points of one call (orbm_update_map_points;
MapPoint.cc:350-436, :467-547, LocalMapping.cc:1040-1053) - what can be shown without a device.

  * The host form orbm_map_point_normal_depth (csrc/orb_ref_mappoint.h, the kernel's own arithmetic) equals the numpy model of
    tests/map_point_update_model.py bit for bit on every point of tests/map_point_update_scene.py.
  * The scene holds what tests/test_gpu_map_point_update.py relies on, and tells the stated cv::scaleAdd form from the fused one, from
    the division by the norm and from a plain x / n in the final scaling.
  * The symbols are on every layer, the struct layouts agree, the header cites the reference and holds the INDEPENDENCE note; NULL
    arguments of both entries are refused without a device.
  * The member swap csrc/adapter/snippets/MapPoint_UpdateBatch_hip.cc type-checks against the reference's unmodified headers (skipped
    where the reference tree is absent)."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import map_point_update_model as MM
import map_point_update_scene as MS
from conftest import ROOT

SENTINEL = np.float32(-123.25)
_model = {}


def model(oracle, form="scaleadd", final="mul"):
    """The model's outputs over the scene, computed once per variant and left unchanged."""
    if (form, final) not in _model:
        _model[(form, final)] = MM.update(oracle if (form, final) == ("scaleadd", "mul") else None, MS.scene(), SENTINEL, form, final)
    return _model[(form, final)]


def test_host_form_equals_the_model_on_every_scene_point(pkg, oracle):
    pts = MS.scene()
    _, normal, mn, mx = model(oracle)
    for p, pt in enumerate(pts):
        if len(pt["desc"]) == 0:
            continue
        got = pkg.map_point_normal_depth(pt["centre"], pt["pos"], pt["ref_centre"], pt["ref_scale"], pt["ref_max_scale"])
        assert MM.same_bits(got[0], normal[p]) and MM.same_bits(got[1], mn[p]) and MM.same_bits(got[2], mx[p]), p


def test_host_form_refuses_null_and_leaves_an_empty_point_alone(pkg):
    L = pkg.load()
    f = lambda *v: np.array(v, np.float32)
    cen, pos, ref = f(0, 0, 0, 1, 0, 0), f(0, 0, 2), f(0, 0, 0)
    p = pkg._p
    for drop in range(6):
        out = [np.full(3, SENTINEL), np.full(1, SENTINEL), np.full(1, SENTINEL)]
        args = [p(cen), p(pos), p(ref), p(out[0]), p(out[1]), p(out[2])]
        args[drop] = None
        rc = L.orbm_map_point_normal_depth(2, args[0], args[1], args[2], 1.0, 2.0, args[3], args[4], args[5])
        assert rc == pkg.E_ARG and all(np.all(o == SENTINEL) for o in out), drop
    out = [np.full(3, SENTINEL), np.full(1, SENTINEL), np.full(1, SENTINEL)]
    assert L.orbm_map_point_normal_depth(-1, p(cen), p(pos), p(ref), 1.0, 2.0, p(out[0]), p(out[1]), p(out[2])) == pkg.E_ARG
    assert L.orbm_map_point_normal_depth(0, None, p(pos), p(ref), 1.0, 2.0, p(out[0]), p(out[1]), p(out[2])) == 0   # observations.empty()
    assert all(np.all(o == SENTINEL) for o in out)
    n, mn, mx = pkg.map_point_normal_depth(cen, pos, ref, 1.5, 2.0)          # two entries: straight below, and one metre aside
    assert mx == np.float32(3.0) and mn == np.float32(1.5) and n[1] == 0 and n[2] > 0.9 and n[0] < 0


def test_null_handle_is_refused_without_a_device(pkg):
    L = pkg.load()
    A = pkg.pack_map_points(MS.scene()[:20])
    u = pkg.MapPointUpdateStruct(20, *[pkg._p(A[k]) for k in ("start", "desc", "centre", "in_desc", "pos", "ref_centre", "ref_scale", "ref_max_scale")])
    best, normal, mn, mx = np.full(20, 7, np.int32), np.full((20, 3), SENTINEL), np.full(20, SENTINEL), np.full(20, SENTINEL)
    p = pkg._p
    assert L.orbm_update_map_points(None, C.byref(u), p(best), p(normal), p(mn), p(mx)) == pkg.E_ARG
    assert np.all(best == 7) and np.all(normal == SENTINEL) and np.all(mn == SENTINEL) and np.all(mx == SENTINEL)


def test_symbols_citations_and_the_independence_note(pkg):
    with open(os.path.join(ROOT, "include", "orbhip.h")) as f:
        header = f.read()
    L = pkg.load()
    for name, nargs in (("orbm_update_map_points", 6), ("orbm_map_point_normal_depth", 9)):
        assert ("int %s(" % name) in header and name in pkg.ABI_SYMBOLS and len(getattr(L, name).argtypes) == nargs
    decl = " ".join(header[header.index("int orbm_update_map_points("):].split(";")[0].split())
    for arg in ("orbm_t *m, const orbm_map_point_update_t *u", "int32_t *best", "float *normal", "float *min_dist", "float *max_dist"):
        assert arg in decl, arg
    end = header.index("} orbm_map_point_update_t;")
    doc = header[header.rindex("/* void MapPoint::ComputeDistinctiveDescriptors()", 0, end):end]
    for line in ("MapPoint.cc:350-436", "MapPoint.cc:467-547", "LocalMapping.cc:1040-1053", "LocalMapping.cc:890-897", "INDEPENDENCE", "listed twice",
                 "LEFT UNTOUCHED", "1024", "orb_ref_mappoint.h", "-1 where no entry has in_desc set"):
        assert line in doc, line
    struct = " ".join(doc[doc.rindex("typedef struct {"):].split())
    fields = [n for n, _ in pkg.MapPointUpdateStruct._fields_]
    assert fields == ["nmp", "start", "desc", "centre", "in_desc", "pos", "ref_centre", "ref_scale", "ref_max_scale"]
    at = [struct.index(" %s;" % n) if n == "nmp" else struct.index("*%s;" % n) for n in fields]
    assert at == sorted(at)
    with open(os.path.join(ROOT, "3_orb_slam3_selfnote_amd", "csrc", "orb_ref_mappoint.h")) as f:
        ref = f.read()
    assert ref.count("[OPENCV-UNVERIFIED]") == 1 and "scaleAdd" in ref and "MapPoint.cc:486-545" in ref
    assert list(inspect.signature(pkg.ORBmatcher.UpdateMapPoints).parameters)[:2] == ["self", "points"]


def test_struct_layout_agrees_with_the_header(pkg, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build environment"
    names = [n for n, _ in pkg.MapPointUpdateStruct._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbhip.h"\nint main(void) {\n  printf("%zu", sizeof(orbm_map_point_update_t));\n' +
                   "".join('  printf(" %%zu", offsetof(orbm_map_point_update_t, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = pkg.MapPointUpdateStruct
    assert got == [C.sizeof(S)] + [getattr(S, n).offset for n in names] and C.sizeof(S) == 72


def test_scene_properties(pkg, oracle):
    pts, N = MS.scene(), MS.NAMED
    best, normal, mn, mx = model(oracle)
    assert 280 <= len(pts) <= 320
    for n in MS.SIZES:
        assert len(pts[N["n%d" % n]]["desc"]) == n
    e = N["n0"]
    assert best[e] == -1 and np.all(normal[e] == SENTINEL) and mn[e] == SENTINEL and mx[e] == SENTINEL
    a = N["none_flagged"]
    assert not pts[a]["in_desc"].any() and best[a] == -1 and np.all(np.isfinite(normal[a])) and np.isfinite(mn[a]) and mx[a] > 0
    b = N["behind_unflagged"]
    allrows = np.ones(len(pts[b]["desc"]), np.uint8)
    assert pts[b]["in_desc"][0] == 0 and best[b] > 0 and MM.best_entry(oracle, pts[b]["desc"], allrows) == 0
    lp = N["long_partial"]
    fl = pts[lp]["in_desc"]
    assert len(fl) == 200 and 40 <= (fl == 0).sum() <= 100 and best[lp] >= 0 and fl[best[lp]] == 1 and (fl[:best[lp]] == 0).any()
    t = N["twins"]
    assert np.array_equal(pts[t]["desc"][2], pts[t]["desc"][5]) and best[t] == 2
    q = N["all_equal"]
    assert len(np.unique(pts[q]["desc"], axis=0)) == 1 and best[q] == 0
    r = N["rig"]
    assert np.allclose(pts[r]["centre"][2] - pts[r]["centre"][1], [0.11, 0, 0], atol=1e-6)
    c = N["in_centre"]
    assert np.array_equal(pts[c]["centre"][1], pts[c]["pos"]) and np.all(np.isnan(normal[c])) and np.isfinite(mn[c]) and np.isfinite(mx[c])
    others = np.array([p for p in range(len(pts)) if p != c and len(pts[p]["desc"])])
    assert np.all(np.isfinite(normal[others])) and np.all(mn[others] > 0) and np.all(mx[others] >= mn[others])
    lens = np.linalg.norm(normal[others].astype(np.float64), axis=1)
    assert np.all(lens <= 1.0 + 1e-5) and lens.min() < 0.9           # a mean of unit vectors
    assert {float(pt["ref_scale"]) for pt in pts} == {float(s) for s in MS.SCALES} and all(pt["ref_max_scale"] == MS.SCALES[7] for pt in pts)
    # the flags matter in more than the hand-made point, and in both of the kernel's forms
    differ = [p for p in others if 0 in pts[p]["in_desc"] and MM.best_entry(oracle, pts[p]["desc"], np.ones(len(pts[p]["desc"]), np.uint8)) != best[p]]
    assert len(differ) >= 3 and any(len(pts[p]["desc"]) > 64 for p in differ) and any(len(pts[p]["desc"]) <= 64 for p in differ)
    assert len({int(x) for x in best}) >= 8 and (best > 0).sum() >= 100


@pytest.mark.parametrize("form,final,least", [("fused", "mul", 10), ("divide", "mul", 10), ("divide64", "mul", 10), ("scaleadd", "div", 1)])
def test_scene_tells_the_stated_forms_from_their_neighbours(oracle, form, final, least):
    """A comparison that passed under the neighbouring form too would show nothing: every candidate changes bits of the scene's normals.
    The three forms of the sum differ in about a sixth of all components.  The final scaling (float)((double)v * (1.0 / (double)n)) differs
    from a plain float v / n only where v / n is a tie between two SUBNORMAL floats (for a normal quotient and n <= 1024 the double
    product lies too close to v / n to cross a rounding midpoint): the hand-made point `tiny_tie` holds one, 147 * 2^-149 / 98."""
    _, normal, mn, mx = model(oracle)
    _, other, omn, omx = model(oracle, form, final)
    ok = ~np.isnan(normal) & ~np.isnan(other)
    changed = (normal.view(np.uint32) != other.view(np.uint32)) & ok
    assert changed.sum() >= least and changed.any(axis=1).sum() >= least, (form, final, int(changed.sum()))
    assert MM.same_bits(mn, omn) and MM.same_bits(mx, omx)            # the distances do not depend on the form
    if final == "div":
        t = MS.NAMED["tiny_tie"]
        assert changed[t, 2] and normal[t, 2] == np.float32(2.0 ** -149) and other[t, 2] == np.float32(2.0 ** -148)


REF = "/root/reference"
REF_INC = os.path.join(REF, "include")
SNIPPET = os.path.join(ROOT, "3_orb_slam3_selfnote_amd", "csrc", "adapter", "snippets", "MapPoint_UpdateBatch_hip.cc")
needs_reference = pytest.mark.skipif(not os.path.exists(os.path.join(REF_INC, "MapPoint.h")) or shutil.which("g++") is None,
                                     reason="reference headers or g++ not available")


def _typecheck(path):
    """The command of tests/test_adapter_typecheck.py::test_member_snippets_typecheck."""
    stub = os.path.join(ROOT, "tests", "support", "slam_typecheck_stub")
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-I", stub, "-I", REF_INC, "-I", os.path.join(REF_INC, "CameraModels"), "-I", REF,
           "-I", os.path.join(ROOT, "include"), path]
    return subprocess.run(cmd, capture_output=True, text=True)


@needs_reference
def test_update_batch_snippet_typechecks():
    r = _typecheck(SNIPPET)
    assert r.returncode == 0, r.stderr[-4000:]


@needs_reference
@pytest.mark.parametrize("member", ["GetObservations", "GetReferenceKeyFrame", "mfMaxDistance", "mvScaleFactors"])
def test_the_check_sees_a_wrong_member(tmp_path, member):
    src = open(SNIPPET).read()
    assert member in src
    bad = tmp_path / "MapPoint_UpdateBatch_bad.cc"
    bad.write_text(src.replace(member, member[:-1] + "z"))
    r = _typecheck(str(bad))
    assert r.returncode != 0 and member[:-1] + "z" in r.stderr, r.stderr[-2000:]
