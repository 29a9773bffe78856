"""CPU: LocalMapping::KeyFrameCulling (orbm_keyframe_culling*, LocalMapping.cc:1158-1310) - what can be shown without a device.

  * The host form orbm_keyframe_culling_host (csrc/orb_ref_culling.h, the kernels' own statement) equals the literal model of
    tests/keyframe_culling_model.py on every scene of tests/keyframe_culling_scene.py, exactly.
  * The scenes hold what tests/test_gpu_keyframe_culling.py relies on; the properties are asserted on the model alone.
  * The stepwise walk replayed in Python over the host statement (counts at loop entry, then an erase per applied keyframe) equals the
    sequential model for "always", "never" and the model's own decisions.
  * The refusals of the host form leave sentinel-filled outputs untouched; a NULL handle is refused without a device.
  * Symbols on every layer, struct layout, citations and the SEQUENTIAL CULLING RULE in the header.
  * The helper csrc/adapter/snippets/LocalMapping_KeyFrameCulling_hip.cc type-checks against the reference's unmodified headers
    (skipped where the reference tree is absent)."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import keyframe_culling_model as KM
import keyframe_culling_scene as KS
from conftest import ROOT

OUT = ("n_mps", "n_red", "culled", "n_obs", "bad")
_want = {}


def want(name, **kw):
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _want:
        sc = KS.scenes()[name]
        _want[key] = KM.run(sc, sc["erasable"], **kw)
    return _want[key]


@pytest.mark.parametrize("name", sorted(KS.scenes()))
def test_host_form_equals_the_model(pkg, name):
    sc = KS.scenes()[name]
    got = pkg.keyframe_culling_host(KS.arrays(sc), sc["erasable"])
    w = want(name)
    for g, key in zip(got, OUT):
        diff = np.nonzero(g != w[key])[0]
        assert diff.size == 0, (key, diff[:10], g[diff[:10]], w[key][diff[:10]])


@pytest.mark.parametrize("name", sorted(KS.scenes()))
@pytest.mark.parametrize("mode", ["always", "never", "erasable"])
def test_stepwise_replay_over_the_host_statement(pkg, name, mode):
    """What orbm_keyframe_culling_step does, replayed with the host form: the counts of the keyframes behind the last returned one come
    from a one-call run in which exactly the applied keyframes are erasable.  Walking to the next passing keyframe of that run, deciding,
    and running again must visit the sequential model's passing keyframes with its counts."""
    sc = KS.scenes()[name]
    K = len(sc["row_start"]) - 1
    decide = {"always": lambda k: True, "never": lambda k: False, "erasable": lambda k: sc["erasable"] is None or bool(sc["erasable"][k])}[mode]
    w = KM.run(sc, applied=decide)
    erasable, got, first = np.zeros(K, np.uint8), [], 0
    n_mps, n_red = np.full(K, -1, np.int32), np.full(K, -1, np.int32)
    while first < K:
        h_mps, h_red, h_culled, _, _ = pkg.keyframe_culling_host(KS.arrays(sc), erasable)
        nxt = next((k for k in range(first, K) if not sc["skip"][k] and KM.passes(h_red[k], sc["redundant_th"], h_mps[k])), K)
        n_mps[first:nxt + 1], n_red[first:nxt + 1] = h_mps[first:nxt + 1], h_red[first:nxt + 1]
        if nxt < K:
            got.append(nxt)
            erasable[nxt] = decide(nxt)
        first = nxt + 1
    assert got == w["passing"] and np.array_equal(n_mps, w["n_mps"]) and np.array_equal(n_red, w["n_red"])


def test_scene_properties():
    S = KS.scenes()
    rows = {n: np.diff(s["row_start"]) for n, s in S.items()}
    assert [len(rows[n]) for n in ("k1", "k2", "k8", "k101")] == [1, 2, 8, 101] and rows["wide"].max() == 15360
    assert all(r.max() <= 600 for n, r in rows.items() if n != "wide") and max(r.max() for n, r in rows.items() if n != "wide") >= 300
    # a cull changes a later keyframe's decision, in both directions
    for name, entry, after in (("culled_to_kept", True, False), ("kept_to_culled", False, True)):
        never, w = KM.run(S[name], applied=lambda k: False), want(name)
        assert w["culled"][0] == 1 and (1 in never["passing"]) == entry and bool(w["culled"][1]) == after, name
    w = want("kept_to_culled")
    assert w["bad"].sum() == 10 and w["n_mps"][1] == 10 and KM.run(S["kept_to_culled"], applied=lambda k: False)["n_mps"][1] == 20
    # the float product
    w = want("float_product")
    assert (w["n_mps"][0], w["n_red"][0], w["culled"][0]) == (10, 9, 0) and S["float_product"]["redundant_th"] == np.float32(0.9)
    assert want("float_product", product="double")["culled"][0] == 1
    assert not np.float32(9) > np.float32(0.9) * np.float32(10) and 9 > float(np.float32(0.9)) * 10
    # the erase, point by point
    sc, w = S["erase_cases"], want("erase_cases")
    N = sc["named"]
    rows0 = sc["row_point"][sc["row_start"][0]:sc["row_start"][1]]
    assert (rows0 == N["two_rows"]).sum() == 2 and sc["n_obs"][N["two_rows"]] == 4
    assert w["culled"][0] == 1 and w["n_obs"][N["two_rows"]] == 3 and not w["bad"][N["two_rows"]]
    per_row = want("erase_cases", erase="per_row")
    assert per_row["n_obs"][N["two_rows"]] == 2 and per_row["bad"][N["two_rows"]] and per_row["n_mps"][1] == w["n_mps"][1] - 1
    assert (w["n_obs"][N["to_two"]], w["bad"][N["to_two"]]) == (2, 1) and (w["n_obs"][N["w2_to_two"]], w["bad"][N["w2_to_two"]]) == (2, 1)
    assert (w["n_obs"][N["w2_to_three"]], w["bad"][N["w2_to_three"]]) == (3, 0) and sc["n_obs"][N["w2_to_three"]] == 5
    assert (w["n_obs"][N["w2_others"]], w["bad"][N["w2_others"]]) == (6, 0)
    assert w["n_obs"][N["no_entry_of_0"]] == sc["n_obs"][N["no_entry_of_0"]] and w["n_obs"][N["bad_on_entry"]] == sc["n_obs"][N["bad_on_entry"]]
    assert 2 in sc["obs_w"] and 2 in S["k101"]["obs_w"]
    assert sc["skip"][2] and KM.passes(12, 0.9, 12) and tuple(w[k][2] for k in OUT[:3]) == (0, 0, 0)       # skipped although it would pass
    assert w["passing"] == [0, 3, 4] and sc["erasable"][3] == 0 and w["culled"][3] == 0 and w["culled"][4] == 1
    assert KM.run(sc, applied=lambda k: True)["passing"] == [0, 3]                                # erasing keyframe 3 would have kept 4
    assert rows["erase_cases"][5] == 0 and w["n_mps"][5] == 0 and w["culled"][5] == 0              # a keyframe with no rows
    # the lists
    sc, w = S["list_cases"], want("list_cases")
    N, ne = sc["named"], np.diff(sc["obs_start"])
    kfs, points = KM.build(sc)

    def redundant(name):
        kf = kfs[0]                                   # keyframe 0 with this one row alone
        i = kf.mvpMapPoints.index(points[N[name]])
        one = KM.KeyFrame(0, 0, kf.mThDepth, kf.mvpMapPoints[i:i + 1], kf.levels[i:i + 1], kf.mvDepth[i:i + 1])
        kept = (kf.mvpMapPoints, kf.levels, kf.mvDepth)
        kf.mvpMapPoints, kf.levels, kf.mvDepth = one.mvpMapPoints, one.levels, one.mvDepth
        try:
            n_mps, n_red = KM.counts(kf, False)
        finally:
            kf.mvpMapPoints, kf.levels, kf.mvDepth = kept
        assert n_mps == 1
        return n_red == 1

    for n in KS.ENTRY_COUNTS:
        assert ne[N["n%d_none" % n]] == n and not redundant("n%d_none" % n)
        assert n < 4 or (ne[N["n%d_all" % n]] == n and redundant("n%d_all" % n))
    for at in KS.FOURTH_AT:
        p = N["fourth_at_%d_hit" % at]
        ent = sc["obs_level"][sc["obs_start"][p]:sc["obs_start"][p + 1]]
        assert len(ent) == at + 1 and list(np.nonzero(ent <= 3)[0]) == [0, 1, 2, at]
        assert redundant("fourth_at_%d_hit" % at) and not redundant("fourth_at_%d_miss" % at) and redundant("fourth_at_%d_long" % at)
    assert redundant("level_plus_1") and not redundant("level_plus_2")
    assert not redundant("own_is_fourth") and redundant("own_and_four") and not redundant("n_obs_3")
    depth = {n: sc["row_depth"][list(sc["row_point"]).index(N[n])] for n in ("at_th_depth", "above_th_depth", "negative_depth", "zero_depth")}
    assert depth["at_th_depth"] == sc["th_depth"][0] and depth["above_th_depth"] > sc["th_depth"][0] and depth["negative_depth"] < 0
    base = KM.run(sc, applied=lambda k: False)["n_mps"][0]
    for n, counted in (("at_th_depth", 1), ("zero_depth", 1), ("above_th_depth", 0), ("negative_depth", 0)):
        other = dict(sc, row_point=np.where(sc["row_point"] == N[n], -1, sc["row_point"]).astype(np.int32))
        assert base - KM.run(other, applied=lambda k: False)["n_mps"][0] == counted, n
    # the random maps cull, skip, keep unerasable keyframes, turn points bad and change later decisions
    for name in ("k1", "k2", "k8", "k101", "wide"):
        assert want(name)["culled"].sum() >= 1 and want(name)["bad"].sum() > S[name]["bad"].sum(), name
    w, never = want("k101"), KM.run(S["k101"], applied=lambda k: False)
    assert w["culled"].sum() >= 20 and len(w["passing"]) > w["culled"].sum() and len(set(never["passing"]) - set(w["passing"])) >= 10
    assert S["k101"]["skip"].sum() == 2 and S["mono"]["row_depth"] is None and S["mono"]["mono"] == 1 and want("mono")["culled"].sum() >= 1


def _host(pkg, A, erasable=None, drop=None, struct=True):
    c, keep = pkg.culling_struct(A)
    K, P = max(c.K, 1), max(c.P, 1)
    out = [np.full(K, -9, np.int32), np.full(K, -9, np.int32), np.full(K, 77, np.uint8), np.full(P, -9, np.int32), np.full(P, 77, np.uint8)]
    args = [pkg._p(o) for o in out]
    if drop is not None:
        args[drop] = None
    rc = pkg.load().orbm_keyframe_culling_host(C.byref(c) if struct else None, pkg._p(erasable), *args)
    return rc, out, pkg.load().orbm_keyframe_culling_host_error()


def _untouched(out):
    return all(np.all(o == (77 if o.dtype == np.uint8 else -9)) for o in out)


def test_host_form_refusals(pkg):
    A = KS.arrays(KS.scenes()["erase_cases"])
    rc, out, _ = _host(pkg, A)
    assert rc == 0 and not np.any(out[0] == -9) and not np.any(out[4] == 77)
    rc, out, _ = _host(pkg, A, drop=4)
    assert rc == 0 and np.all(out[4] == 77) and not np.any(out[3] == -9)
    rc, out, _ = _host(pkg, dict(A, row_start=np.zeros(1, np.int32)))                 # K == 0
    assert rc == 0 and _untouched(out)

    def changed(key, at, value):
        B = dict(A, **{key: A[key].copy()})
        B[key][at] = value
        return B

    e0 = A["obs_start"][KS.scenes()["erase_cases"]["named"]["no_entry_of_0"]]
    wide = KS.arrays(KS.scenes()["wide"])
    grown = dict(wide, row_start=wide["row_start"] + np.array([0, 0, 1, 1], np.int32), row_point=np.append(wide["row_point"], -1).astype(np.int32),
                 row_level=np.append(wide["row_level"], 0).astype(np.int32), row_depth=np.append(wide["row_depth"], 1).astype(np.float32))
    cases = [(changed("row_start", 0, 1), b"row_start[0]"), (changed("obs_start", 0, 1), b"obs_start[0]"),
             (changed("row_start", 2, A["row_start"][1] - 1), b"row_start decreases"), (changed("obs_start", 5, A["obs_start"][4] - 1), b"obs_start decreases"),
             (changed("row_point", 7, len(A["bad"])), b"row_point"), (changed("row_point", 7, -2), b"row_point"),
             (changed("obs_kf", 9, 6), b"obs_kf"), (changed("obs_kf", 9, -2), b"obs_kf"), (changed("obs_w", 3, 0), b"obs_w"), (changed("obs_w", 3, 3), b"obs_w"),
             (changed("obs_kf", slice(e0, e0 + 2), 1), b"same obs_kf"), (dict(A, redundant_th=np.float32(np.nan)), b"NaN"),
             (dict(A, row_start=np.concatenate([A["row_start"], np.full(pkg.CULL_MAX_KEYFRAMES, A["row_start"][-1], np.int32)])), b"ORBM_CULL_MAX_KEYFRAMES"),
             (grown, b"15360")]
    cases += [(dict(A, **{key: None}), b"NULL") for key in ("skip", "th_depth", "row_point", "row_level", "row_depth", "bad", "n_obs", "obs_kf", "obs_level", "obs_w")]
    for B, word in cases:
        rc, out, msg = _host(pkg, B)
        assert rc == pkg.E_ARG and _untouched(out) and word in msg, (word, msg)
    for drop in range(3):
        rc, out, msg = _host(pkg, A, drop=drop)
        assert rc == pkg.E_ARG and _untouched(out) and b"NULL output" in msg
    rc, out, msg = _host(pkg, A, struct=False)
    assert rc == pkg.E_ARG and _untouched(out)
    mono = KS.arrays(KS.scenes()["mono"])
    assert mono["row_depth"] is None and _host(pkg, mono)[0] == 0                     # row_depth may be NULL when mono != 0
    with pytest.raises(ValueError, match="obs_w"):
        pkg.keyframe_culling_host(changed("obs_w", 3, 0))


def test_null_handle_is_refused_without_a_device(pkg):
    L = pkg.load()
    c, keep = pkg.culling_struct(KS.arrays(KS.scenes()["mono"]))
    out = [np.full(3, -9, np.int32), np.full(3, -9, np.int32), np.full(3, 77, np.uint8), np.full(c.P, -9, np.int32), np.full(c.P, 77, np.uint8)]
    assert L.orbm_keyframe_culling(None, C.byref(c), None, *[pkg._p(o) for o in out]) == pkg.E_ARG and _untouched(out)
    assert L.orbm_keyframe_culling_open(None, C.byref(c)) == pkg.E_ARG
    k = np.full(1, -9, np.int32)
    assert L.orbm_keyframe_culling_step(None, 0, pkg._p(k), pkg._p(out[0]), pkg._p(out[1])) == pkg.E_ARG and k[0] == -9 and _untouched(out)


def test_symbols_citations_and_the_sequential_culling_rule(pkg):
    with open(os.path.join(ROOT, "include", "orbhip.h")) as f:
        header = f.read()
    L = pkg.load()
    for name, nargs in (("orbm_keyframe_culling", 8), ("orbm_keyframe_culling_open", 2), ("orbm_keyframe_culling_step", 5), ("orbm_keyframe_culling_host", 7)):
        assert ("int %s(" % name) in header and name in pkg.ABI_SYMBOLS and len(getattr(L, name).argtypes) == nargs
    assert "const char *orbm_keyframe_culling_host_error(void);" in header and "orbm_keyframe_culling_host_error" in pkg.ABI_SYMBOLS
    end = header.index("} orbm_culling_t;")
    doc = header[header.rindex("/* void LocalMapping::KeyFrameCulling()", 0, end):end]
    for line in ("LocalMapping.cc:1158-1310", "LocalMapping.cc:1204-1266", "KeyFrame.cc:670-677", "MapPoint.cc:168-202", "MapPoint.cc:217-226",
                 "MapPoint.cc:179-187", "SEQUENTIAL CULLING RULE", "validity only shrinks", "It is not a double product", "orb_ref_culling.h",
                 "ORBM_CULL_MAX_KEYFRAMES", "ORBM_MAX_KEYPOINTS", "step without open", "no cap on the entries"):
        assert line in doc, line
    struct = " ".join(doc[doc.rindex("typedef struct {"):].split())
    fields = [n for n, _ in pkg.CullingStruct._fields_]
    assert fields == ["K", "skip", "th_depth", "row_start", "row_point", "row_level", "row_depth", "P", "bad", "n_obs", "obs_start", "obs_kf",
                      "obs_level", "obs_w", "mono", "redundant_th"]
    at = [struct.index(" %s;" % n) if n in ("K", "P", "mono", "redundant_th") else struct.index("*%s;" % n) for n in fields]
    assert at == sorted(at)
    with open(os.path.join(ROOT, "3_orb_slam3_selfnote_amd", "csrc", "orb_ref_culling.h")) as f:
        ref = f.read()
    assert "LocalMapping.cc:1204-1266" in ref and "(float)n_red > redundant_th * (float)n_mps" in ref
    with open(os.path.join(ROOT, "3_orb_slam3_selfnote_amd", "csrc", "orb_culling_kernels.h")) as f:
        kernels = f.read()
    assert "void k_cull_count(" in kernels and "void k_cull_walk(" in kernels and '#include "orb_ref_culling.h"' in kernels
    assert list(inspect.signature(pkg.ORBmatcher.KeyFrameCulling).parameters) == ["self", "scene", "erasable"]
    assert list(inspect.signature(pkg.ORBmatcher.KeyFrameCullingStep).parameters) == ["self", "applied"]
    assert list(inspect.signature(pkg.keyframe_culling_host).parameters) == ["scene", "erasable"]
    assert pkg.CULL_MAX_KEYFRAMES == int(header.split("#define ORBM_CULL_MAX_KEYFRAMES")[1].split()[0])


def test_struct_layout_agrees_with_the_header(pkg, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build environment"
    names = [n for n, _ in pkg.CullingStruct._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbhip.h"\nint main(void) {\n  printf("%zu", sizeof(orbm_culling_t));\n' +
                   "".join('  printf(" %%zu", offsetof(orbm_culling_t, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = pkg.CullingStruct
    assert got == [C.sizeof(S)] + [getattr(S, n).offset for n in names] and C.sizeof(S) == 120


REF = "/root/reference"
REF_INC = os.path.join(REF, "include")
SNIPPET = os.path.join(ROOT, "3_orb_slam3_selfnote_amd", "csrc", "adapter", "snippets", "LocalMapping_KeyFrameCulling_hip.cc")
needs_reference = pytest.mark.skipif(not os.path.exists(os.path.join(REF_INC, "LocalMapping.h")) or shutil.which("g++") is None,
                                     reason="reference headers or g++ not available")


def _typecheck(path):
    """The command of tests/test_fuse_keyframes_abi.py for the helpers of LocalMapping."""
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-I", os.path.join(ROOT, "tests", "support", "tracking_typecheck_stub"),
           "-I", os.path.join(ROOT, "tests", "support", "slam_typecheck_stub"), "-I", REF_INC, "-I", os.path.join(REF_INC, "CameraModels"),
           "-I", REF, "-I", os.path.join(ROOT, "include"), path]
    return subprocess.run(cmd, capture_output=True, text=True)


@needs_reference
def test_culling_snippet_typechecks():
    r = _typecheck(SNIPPET)
    assert r.returncode == 0, r.stderr[-4000:]


@needs_reference
@pytest.mark.parametrize("member", ["GetMapPointMatches", "GetInitKFid", "mvKeysRight", "mThDepth", "orbm_keyframe_culling_step"])
def test_the_check_sees_a_wrong_member(tmp_path, member):
    src = open(SNIPPET).read()
    assert member in src
    bad = tmp_path / "LocalMapping_KeyFrameCulling_bad.cc"
    bad.write_text(src.replace(member, member[:-1] + "z"))
    r = _typecheck(str(bad))
    assert r.returncode != 0 and member[:-1] + "z" in r.stderr, r.stderr[-2000:]


def test_snippet_holds_the_three_edits_and_the_two_notes():
    src = open(SNIPPET).read()
    for line in ("KeyFrameCullingCounts cull(vpLocalKeyFrames, mbMonocular, redundant_th);", "cull.counts(pKF, nMPs, nRedundantObservations);",
                 "cull.erased(pKF);", "THE SNAPSHOT", "THE RIG OCTAVE", "mvKeysRight[i - pKF->NLeft].octave", "SEQUENTIAL CULLING RULE"):
        assert line in src, line
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for line in ("LocalMapping_KeyFrameCulling_hip.cc", "cull.erased(pKF);", "mvKeysRight[i]"):
        assert line in doc, line
