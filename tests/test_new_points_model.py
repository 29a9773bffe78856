"""CPU: the body of LocalMapping::CreateNewMapPoints' loop (LocalMapping.cc:605-880) as the library states it for host and device
(csrc/orb_ref_newpoints.h, orbm_new_point_geometry) against the numpy model of tests/new_points_model.py, bit for bit - status and x3D -
and the SEQUENTIAL RULE of include/orbhip.h on the oracle and the model alone.

  * Scenes (tests/new_points_scene.py): Pinhole with mono and stereo keypoints mixed, KannalaBrandt8 single cameras, a rig with all four
    (bRight1, bRight2) arms, and hand-made pairs that reach every status.  That every status occurs is a condition on the scenes and is
    asserted on the MODEL's output.
  * A replay of the reference's loop - the oracle's search with the current map-point flags, the model per pair, the flag set on
    acceptance - equals "first accepted neighbour per idx1" from the loop-entry rows, and every prefix `neighbour < i` equals the replay
    stopped in front of neighbour i.
  * What can be refused without a device: the pair entry's arguments, and the one-call entries without a handle (all-NULL included).  The
    refusals that name a neighbour need a handle: tests/test_gpu_new_points.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import new_points_model as NM
import new_points_scene as PS
import triangulation_neighbours_scene as NS
from conftest import ROOT
from test_gpu_triangulation_kb8 import pred_of
from test_triangulation_neighbours_abi import KB8_CENTRES, kb8_scenes


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_pairs(pkg, c1, c2, o1, o2, far=False, th_far=0.0):
    """Host entry against the model on these pairs; returns the model's status."""
    want_st, want_X = PS.model_status(c1, c2, o1, o2, far, th_far)
    st, X = pkg.new_point_geometry(c1, c2, o1, o2, PS.SCALE_FACTOR, far, th_far)
    assert np.array_equal(st, want_st), [(i, NM.STATUS[a], NM.STATUS[b]) for i, (a, b) in enumerate(zip(st, want_st)) if a != b][:5]
    assert np.array_equal(bits(X), bits(want_X))
    assert np.all(X[st != NM.ACCEPTED] == 0)
    return want_st


def test_layouts_status_codes_and_symbols(pkg):
    assert pkg.NP_CAMERA_DTYPE == PS.CAMERA and pkg.NP_OBS_DTYPE == PS.OBS and pkg.NP_CAMERA_DTYPE.itemsize == 400 and pkg.NP_OBS_DTYPE.itemsize == 32
    assert pkg.NEW_POINT_DTYPE.itemsize == 24
    with open(os.path.join(ROOT, "include", "orbhip.h")) as f:
        header = f.read()
    codes = dict((k, int(v)) for k, v in re.findall(r"ORBM_NP_([A-Z0-9_]+) = (\d+)", header))
    assert codes.pop("NSTATUS") == len(NM.STATUS) == pkg.NP_NSTATUS
    assert codes == {name: i for i, name in enumerate(NM.STATUS)}
    assert all(getattr(pkg, "NP_" + name) == i for i, name in enumerate(NM.STATUS))
    L = pkg.load()
    for name, nargs in (("orbm_new_point_geometry", 10), ("orbm_new_point_geometry_device", 11), ("orbm_create_new_map_points", 23),
                        ("orbm_create_new_map_points_kb8", 22)):
        assert ("int %s(" % name) in header and name in pkg.ABI_SYMBOLS and len(getattr(L, name).argtypes) == nargs
    doc = header[header.index("SEQUENTIAL RULE"):header.index("int orbm_create_new_map_points(")]
    for line in ("LocalMapping.cc:892", "LocalMapping.cc:528", "neighbour < i", "(:893)"):
        assert line in doc, line


def test_planted_pairs_reach_every_status_and_the_host_equals_the_model(pkg):
    seen = {}
    for name, c1, c2, o1, o2, far, th_far in PS.planted():
        for s in check_pairs(pkg, c1, c2, o1, o2, far, th_far):
            seen[int(s)] = seen.get(int(s), 0) + 1
    assert sorted(seen) == list(range(1, len(NM.STATUS))), [NM.STATUS[s] for s in range(1, len(NM.STATUS)) if s not in seen]


@pytest.mark.parametrize("kinds", [NS.REPLAY, NS.MAIN], ids=["replay", "main"])
def test_pinhole_stereo_mix_host_equals_model(pkg, oracle, kinds):
    S = PS.pinhole(kinds)
    seen = set()
    for far, th_far in ((False, 0.0), (True, 6.0)):
        E = PS.expected_pinhole(oracle, S, far=far, th_far=th_far)
        for j in range(E.K):
            row = E.row_of(j, S["mp1"])
            i1, o1, o2 = PS.pinhole_pairs(S, j, row)
            if len(i1):
                seen |= set(check_pairs(pkg, S["c1"], S["c2"][j], o1, o2, far, th_far).tolist())
    # both UnprojectStereo arms and both stereo reprojection forms occur in the natural scene too
    assert {NM.ACCEPTED, NM.REPROJ1_STEREO, NM.REPROJ2_STEREO, NM.FAR} <= seen, sorted(NM.STATUS[s] for s in seen)


@pytest.mark.parametrize("rig", [False, True], ids=["single", "rig"])
def test_kb8_host_equals_model(pkg, oracle, rig):
    Ss = kb8_scenes(rig)
    E = PS.expected_kb8(oracle, Ss, KB8_CENTRES, pred_of)
    arms = set()
    for j in range(E.K):
        row = E.row_of(j, Ss[0]["mp1"])
        i1, o1, o2 = PS.kb8_pairs(Ss, j, row)
        st = check_pairs(pkg, E.c1, E.c2[j], o1, o2)
        assert (st == NM.ACCEPTED).sum() >= 10
        arms |= {(int(a), int(b)) for a, b, s in zip(o1["right"], o2["right"], st) if s == NM.ACCEPTED}
    assert arms == ({(0, 0), (0, 1), (1, 0), (1, 1)} if rig else {(0, 0)})


def check_rule(E, skip=None):
    """Replay == rule, every prefix == the stopped replay; returns the list and the loop-entry status."""
    rows, _, st, _ = E.tables(skip)
    rule = E.rule(skip)
    assert PS.same_list(E.replay(skip), rule)
    for stop in range(E.K + 1):
        assert PS.same_list(E.replay(skip, stop), [p for p in rule if p[0] < stop]), stop
    assert [p[:2] for p in rule] == sorted(p[:2] for p in rule) and len({p[1] for p in rule}) == len(rule)
    return rule, st


@pytest.mark.parametrize("coarse", [False, True])
def test_sequential_rule_pinhole(oracle, coarse):
    S = PS.pinhole(NS.REPLAY)
    E = PS.expected_pinhole(oracle, S, coarse=coarse)
    rule, st = check_rule(E)
    twice = np.nonzero((st == NM.ACCEPTED).sum(0) >= 2)[0]
    assert len(twice) >= 1 and len(rule) >= 20             # an idx1 accepted against two neighbours: the list keeps the earlier one only
    for i1 in twice:
        assert [p[0] for p in rule if p[1] == i1] == [int(np.nonzero(st[:, i1] == NM.ACCEPTED)[0][0])]
    check_rule(E, skip=(0, 1, 0, 0))


@pytest.mark.parametrize("rig", [False, True], ids=["single", "rig"])
def test_sequential_rule_kb8(oracle, rig):
    Ss = kb8_scenes(rig)
    rule, st = check_rule(PS.expected_kb8(oracle, Ss, KB8_CENTRES, pred_of))
    assert ((st == NM.ACCEPTED).sum(0) >= 2).sum() >= 1 and len(rule) >= 20


def test_refusals_without_a_device(pkg):
    L = pkg.load()
    name, c1, c2, o1, o2, _, _ = PS.planted()[0]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    c1, c2 = np.ascontiguousarray(c1), np.ascontiguousarray(c2)
    st, X = np.full(len(o1), 77, np.uint8), np.zeros((len(o1), 3), np.float32)
    good = [len(o1), p(c1), p(c2), p(o1), p(o2), 1.2, 0, 0.0, p(st), p(X)]
    assert L.orbm_new_point_geometry(*good) == 0 and np.all(st != 77)
    for k in (1, 2, 3, 4, 8, 9):                            # each pointer NULL in turn
        assert L.orbm_new_point_geometry(*[None if i == k else a for i, a in enumerate(good)]) == pkg.E_ARG, k
    assert L.orbm_new_point_geometry(*([-1] + good[1:])) == pkg.E_ARG
    assert L.orbm_new_point_geometry(0, p(c1), p(c2), None, None, 1.2, 0, 0.0, None, None) == 0
    bad = c2.copy()
    bad["cam_type"] = 2
    assert L.orbm_new_point_geometry(*(good[:2] + [p(bad)] + good[3:])) == pkg.E_ARG
    assert L.orbm_new_point_geometry_device(len(o1), None, None, None, None, 1.2, 0, 0.0, None, None, None) == pkg.E_ARG
    # the one-call entries: all-NULL, and a complete call without a handle
    assert L.orbm_create_new_map_points(None, None, None, 1.2, 0, *[None] * 10, 0, 0, 0.0, None, 0, None, None, None) == pkg.E_ARG
    assert L.orbm_create_new_map_points_kb8(None, None, None, 1.2, -1, 0, *[None] * 8, 0, 0, 0.0, None, 0, None, None, None) == pkg.E_ARG
    S = PS.pinhole(NS.REPLAY)
    K1, G1, views, Gs = PS.product_pinhole(pkg, S)
    s1, g1 = K1.struct(), G1.struct()
    tab = (pkg.KeyFrameStruct * 4)(*[v.struct() for v in views])
    gtab = (pkg.KeyFrameGeometryStruct * 4)(*[g.struct() for g in Gs])
    R2w, t2w = np.stack([nb["R2w"] for nb in S["nbs"]]), np.stack([nb["t2w"] for nb in S["nbs"]])
    cam2 = np.tile(S["cam"], (4, 1))
    pts = np.zeros(K1.N, pkg.NEW_POINT_DTYPE)
    rc = L.orbm_create_new_map_points(None, C.byref(s1), C.byref(g1), 1.2, 4, C.cast(tab, C.c_void_p), C.cast(gtab, C.c_void_p), p(S["R1w"]), p(S["t1w"]),
                                      p(S["Cw1"]), p(S["cam"]), p(R2w), p(t2w), p(cam2), None, 0, 0, 0.0, p(pts), K1.N, None, None, None)
    assert rc == pkg.E_ARG and not pts["idx1"].any()
