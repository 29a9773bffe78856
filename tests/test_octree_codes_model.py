"""CPU: the code form of DistributeOctTree (tests/octree_codes_model.py: column / row tables, leaf histogram, count pyramid, rounds on
the nodes alone, leaf map, hand-over to the per-key rounds) against tests/octree_model.py and the oracle's extractor, key for key
and in output order, and the properties of the cases that tests/test_gpu_octree_codes.py relies on."""
import numpy as np
import pytest

import octree_codes_cases as K
import octree_codes_model as MC
import octree_model as M
import ref_cases as R

_ref = {}


def reference(oracle, synth, name):
    if name not in _ref:
        _, img, c = next(x for x in K.cases(synth) if x[0] == name)
        _ref[name] = K.level_reference(oracle, img, c)
    return _ref[name]


def run_model(lv, D=MC.D_DEFAULT):
    c, (x0, x1, y0, y1) = lv["cand"], lv["rect"]
    info = {}
    if x1 - x0 <= 0 or y1 - y0 <= 0 or len(c) == 0:
        return np.zeros((0, 3), np.float32), dict(handover=None, rounds=0, depth=-1)
    xs, ys, rs = c[:, 0].astype(np.int64), c[:, 1].astype(np.int64), c[:, 2].astype(np.int64)
    idx = MC.distribute(xs, ys, rs, x0, x1, y0, y1, lv["N"], D=D, info=info)
    assert idx == M.distribute(xs, ys, rs, x0, x1, y0, y1, lv["N"]), "code form and per-key form disagree"
    return c[idx], info


NAMES = ["flat", "one blob", "two blobs", "patch inside a cell", "patch across the first split lines", "patch across a root's split lines",
         "small N", "N above the keys", "one root", "two roots", "three roots", "empty root", "checkerboard", "squares", "noise 752x480"]


def test_case_list(synth):
    assert [c[0] for c in K.cases(synth)] == NAMES
    for _, img, _ in K.cases(synth):
        assert img.shape[0] <= 480 and img.shape[1] <= 752 and img.dtype == np.uint8


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_oracle(oracle, synth, name):
    for l, lv in enumerate(reference(oracle, synth, name)):
        got, _ = run_model(lv)
        assert np.array_equal(got, lv["oct"]), "level %d" % l


@pytest.mark.parametrize("name", ["patch inside a cell", "two roots", "small N", "checkerboard"])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_model_equals_oracle_at_shallow_tables(oracle, synth, name, D):
    """Tables of depth 1 .. 3: every case hands over, at different rounds."""
    for l, lv in enumerate(reference(oracle, synth, name)):
        got, _ = run_model(lv, D)
        assert np.array_equal(got, lv["oct"]), "level %d" % l


def test_tables_follow_the_interval_arithmetic():
    """A key's table code is the path that DivideNode's comparisons give it, for odd widths, widths that reach 1 and 0, every root."""
    for (W, H, nIni) in [(344, 208, 2), (720, 448, 2), (388, 128, 3), (184, 168, 1), (37, 21, 2), (5, 3, 2)]:
        D = 5
        tx, ty = MC.tables(W, H, nIni, D)
        hX = np.float32(W) / np.float32(nIni)
        for x in range(W):
            r = min(int(np.float32(x) / hX), nIni - 1)
            ul, ur = int(hX * np.float32(r)), int(hX * np.float32(r + 1))
            path = 0
            for _ in range(D):
                half = (ur - ul + 1) >> 1          # ORBextractor.cc:481
                if x < ul + half:
                    ur, b = ul + half, 0
                else:
                    ul, b = ul + half, 1
                path = path * 2 + b
            assert tx[x] == (r << D) + path
        assert len(ty) == H + 1 and ty[0] == 0 and np.all(np.diff(ty[:H]) >= 0)


def keys_per_level(oracle, synth, name):
    return [len(lv["cand"]) for lv in reference(oracle, synth, name)]


def test_cases_reach_what_they_are_for(oracle, synth):
    # levels with 0, 1 and 2 keys
    assert set(keys_per_level(oracle, synth, "flat")) == {0}
    assert 1 in keys_per_level(oracle, synth, "one blob")
    assert 2 in keys_per_level(oracle, synth, "two blobs")
    # the hand-over runs: on some level a node of depth OCT_D holds more than one key and N is not reached
    for name in ("patch inside a cell", "patch across the first split lines", "patch across a root's split lines"):
        infos = [run_model(lv)[1] for lv in reference(oracle, synth, name)]
        assert any(i["handover"] is not None for i in infos), name
        assert max(i["depth"] for i in infos) >= MC.D_DEFAULT
    # N of 1 or 2 (and 0 on the smallest levels)
    assert {1, 2} <= set(lv["N"] for lv in reference(oracle, synth, "small N")) <= {0, 1, 2}
    # N above the key count: every node of the result holds one key
    for lv in reference(oracle, synth, "N above the keys"):
        assert lv["N"] > len(lv["cand"]) and len(lv["oct"]) == len(lv["cand"])
    assert keys_per_level(oracle, synth, "N above the keys")[0] > 50
    # root nodes
    for name, want in (("one root", 1), ("two roots", 2), ("three roots", 3), ("empty root", 2)):
        x0, x1, y0, y1 = reference(oracle, synth, name)[0]["rect"]
        assert int(np.floor(np.float32(x1 - x0) / np.float32(y1 - y0) + np.float32(0.5))) == want
    lv = reference(oracle, synth, "empty root")[0]
    assert len(lv["cand"]) > 20 and lv["cand"][:, 0].min() >= (lv["rect"][1] - lv["rect"][0]) / 2
    # ties: equal responses inside one node of the result
    for name in ("checkerboard", "squares"):
        tied = False
        for lv in reference(oracle, synth, name):
            r = lv["cand"][:, 2]
            tied = tied or (len(r) > len(lv["oct"]) > 0 and len(np.unique(r)) < len(r) / 4)
        assert tied, name
    # more keys than OCT_REGKEYS on level 0
    assert keys_per_level(oracle, synth, "noise 752x480")[0] > 4096


def test_bench_configurations_stay_inside_the_tables(oracle, synth):
    """The statement behind OCT_D = 5 (profiles/octree_codes_depths.txt has the bench's own streams): no split at depth 5 or deeper
    on a synthetic frame at either bench configuration."""
    for rows, cols, c in ((480, 752, K.cfg(1000)), (512, 512, K.cfg(1500))):
        for lv in K.level_reference(oracle, synth.make_frame(3, rows, cols), c):
            _, info = run_model(lv)
            assert info["handover"] is None and info["depth"] < MC.D_DEFAULT
