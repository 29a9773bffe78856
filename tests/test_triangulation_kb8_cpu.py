"""CPU: SearchForTriangulation for KannalaBrandt8 keyframes and rigs (orbm_search_for_triangulation_kb8).

  * The synthetic scene of tests/triangulation_kb8_scene.py exercises what the GPU tests rely on - through the oracle's member around
    the numpy model's epipolarConstrain only, no product code: enough matches, answers that are not the first entry of their list
    (the geometry rejected a preferred decoy), every kind of rejection, all four camera pairs of a rig, long lists, and an epipole
    gate that changes the lists when the epipole is inside the image.
  * The entry point exists on every layer and refuses a NULL handle without a device."""
import ctypes as C
import inspect
import os
from collections import Counter

import numpy as np
import pytest

import rig_stereo_model as M
import triangulation_kb8_scene as SC
from conftest import ROOT

NAME = "orbm_search_for_triangulation_kb8"


def _walk(oracle, S, nodes=4):
    O1, O2 = SC.oracle_views(oracle, S, nodes)
    gate = not S["rig"]
    log = []
    n, pairs = oracle.search_for_triangulation_pred(O1, O2, S["ep"], gate, SC.predicate(S, log), check_ori=False)
    st, i2, _ = oracle.triangulation_candidates(O1, O2, S["ep"], gate)
    return n, pairs, st, i2, log


@pytest.mark.parametrize("rig", [False, True])
def test_scene_conditions(oracle, rig):
    S = SC.scene(96, rig)
    n, pairs, st, i2, log = _walk(oracle, S)
    assert n == len(pairs) and n >= 40
    first = {i: i2[st[i]] for i in range(len(st) - 1) if st[i + 1] > st[i]}
    assert sum(1 for a, b in pairs if first[a] != b) >= 8          # a decoy was preferred and rejected
    why = Counter(w for _, _, _, w in log)
    assert why[M.PARALLAX] >= 1 and why[M.Z1] >= 1 and why[M.REPROJ1] + why[M.REPROJ2] >= 1, why
    assert np.diff(st).max() >= 3
    if rig:
        accepted = Counter(p for _, _, p, w in log if w == M.ACCEPT)
        assert all(accepted[p] >= 10 for p in range(4)), accepted
        assert 0 < S["n_left1"] < len(S["k1"]) and 0 < S["n_left2"] < len(S["k2"])
        assert S["T12"].shape == (4, 12) and S["cams1"].shape == (2, 8)
    else:
        assert S["n_left1"] == -1 and S["n_left2"] == -1 and S["T12"].shape == (1, 12)


def test_forward_pose_puts_the_epipole_gate_to_work(oracle):
    S = SC.scene(96, False, SC.FORWARD)
    assert 0 <= S["ep"][0] < 512 and 0 <= S["ep"][1] < 512
    O1, O2 = SC.oracle_views(oracle, S, 4)
    on, off = oracle.triangulation_candidates(O1, O2, S["ep"], True), oracle.triangulation_candidates(O1, O2, S["ep"], False)
    assert len(on[1]) < len(off[1])
    side = SC.scene(96, False)
    assert not (0 <= side["ep"][0] < 512 and 0 <= side["ep"][1] < 512)


def test_descriptors_share_a_node_and_decoys_follow():
    """KF2's copies differ from KF1's descriptors in bytes 8..31 only; the decoys repeat a KF2 descriptor."""
    S = SC.scene(96, True)
    fv1, fv2 = SC.bow(S["d1"], 4), SC.bow(S["d2"], 4)
    assert sum(len(v) for v in fv1.values()) == len(S["k1"]) and sum(len(v) for v in fv2.values()) == len(S["k2"])
    assert len(S["k2"]) > len(S["k1"]) == 96
    assert len({bytes(d) for d in S["d2"]}) == 96
    assert {bytes(d[:8]) for d in S["d2"]} == {bytes(d[:8]) for d in S["d1"]}


def test_symbol_on_every_layer(pkg):
    with open(os.path.join(ROOT, "include", "orbhip.h")) as f:
        header = f.read()
    assert ("int %s(" % NAME) in header
    assert NAME in pkg.ABI_SYMBOLS
    L = pkg.load()
    fn = getattr(L, NAME)                               # exported
    assert fn.argtypes is not None and len(fn.argtypes) == 14
    sig = inspect.signature(pkg.ORBmatcher.SearchForTriangulationKB8)
    assert list(sig.parameters) == ["self", "KF1", "KF2", "ep", "cams1", "cams2", "T12", "n_left1", "n_left2", "bOnlyStereo", "bCoarse"]
    assert sig.parameters["n_left1"].default == -1 and sig.parameters["n_left2"].default == -1


def test_null_handle_is_refused_without_a_device(pkg):
    L = pkg.load()
    S = SC.scene(96, False)
    K1, K2 = SC.product_views(pkg, S, 4)
    s1, s2 = K1.struct(), K2.struct()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    m12 = np.full(K1.N, 7, np.int32)
    T12, c1, c2 = np.ascontiguousarray(S["T12"]), np.ascontiguousarray(S["cams1"]), np.ascontiguousarray(S["cams2"])
    rc = getattr(L, NAME)(None, C.byref(s1), -1, C.byref(s2), -1, C.c_float(0), C.c_float(0), p(c1), p(c2), p(T12), 0, 0, 0, p(m12))
    assert rc == pkg.E_ARG and np.all(m12 == 7)
