"""CPU: TwoViewReconstruction::Reconstruct through the C ABI without a device (orbm_two_view_reconstruct_host, orbm_two_view_models_host,
orbm_two_view_check_rt_host: the statement of csrc/orb_ref_twoview.h that the kernels share) against the literal model of
tests/twoview_model.py.  No tolerance anywhere: floats are compared as bits, NaN by position.

  * The model's cv::SVD::compute equals an independent statement, oracle/ref_cam_shim's, compiled into a stand-alone program, on seeded
    16 x 9, 8 x 9, 3 x 3 and 4 x 4 matrices, among them rank-deficient ones and zero matrices (where the pseudo-random completion decides).
  * The host form equals the model on every scene of tests/twoview_scene.py, on every output; so do both stage entries.
  * The scenes are what they claim to be - asserted on the model alone, so that no scene silently stops testing its case.
  * What is refused; the per-pointer NULL sweep; the adapter snippet type-checks against the reference's unmodified header."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import twoview_model as TM
import twoview_scene as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = tuple(TS.SCENES)

SVD_PROGRAM = r"""
#include <opencv2/core/core.hpp>
#include <stdio.h>
#include <string.h>
// reads "m n" and m*n float bit patterns per matrix, prints the bit patterns of w, u, vt of cv::SVD::compute(MODIFY_A | FULL_UV)
static void dump(const cv::Mat &a) {
  for (int y = 0; y < a.rows; y++)
    for (int x = 0; x < a.cols; x++) { float f = a.at<float>(y, x); unsigned u; memcpy(&u, &f, 4); printf("%08x ", u); }
  printf("\n");
}
int main() {
  int m, n;
  while (scanf("%d %d", &m, &n) == 2) {
    cv::Mat A(m, n, CV_32F), w, u, vt;
    for (int y = 0; y < m; y++)
      for (int x = 0; x < n; x++) { unsigned b; if (scanf("%x", &b) != 1) return 1; float f; memcpy(&f, &b, 4); A.at<float>(y, x) = f; }
    cv::SVD::compute(A, w, u, vt, cv::SVD::MODIFY_A | cv::SVD::FULL_UV);
    dump(w); dump(u); dump(vt);
  }
  return 0;
}
"""


def svd_matrices():
    rng = np.random.default_rng(2024)
    mats = []
    for shape in ((16, 9), (8, 9), (3, 3), (4, 4)):
        for _ in range(3):
            mats.append(rng.normal(0, 1, shape).astype(np.float32))
        mats.append(np.zeros(shape, np.float32))
    a = rng.normal(0, 1, (16, 9)).astype(np.float32)
    a[:, 4] = a[:, 1]                      # two equal columns
    a[:, 7] = 0                            # and a zero column
    mats.append(a)
    b = rng.normal(0, 1, (8, 9)).astype(np.float32)
    b[5] = b[2]                            # two equal rows
    mats.append(b)
    c = rng.normal(0, 1, (3, 3)).astype(np.float32)
    c[:, 2] = 0                            # an exact zero singular value
    mats.append(c)
    d = rng.integers(-3, 4, (3, 3)).astype(np.float32)
    d[2] = d[0] + d[1]                     # rank 2 in small integers
    mats.append(d)
    e = rng.normal(0, 1, (4, 4)).astype(np.float32)
    e[3] = e[0]
    mats.append(e)
    return mats


def test_model_svd_equals_the_stand_in(tmp_path):
    src, exe = tmp_path / "svd_dump.cc", tmp_path / "svd_dump"
    src.write_text(SVD_PROGRAM)
    subprocess.run(["g++", "-std=c++11", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "oracle", "ref_cam_shim"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    mats = svd_matrices()
    text = "".join("%d %d\n%s\n" % (m.shape[0], m.shape[1], " ".join("%08x" % v for v in m.reshape(-1).view(np.uint32))) for m in mats)
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 3 * len(mats)
    for k, A in enumerate(mats):
        m, n = A.shape
        w, u, vt = TM.svd(A)
        want = [np.array([int(x, 16) for x in out[3 * k + j].split()], np.uint32).view(np.float32) for j in range(3)]
        assert TS.same_bits(w, want[0]), "matrix %d (%d x %d): w" % (k, m, n)
        assert TS.same_bits(u, want[1]), "matrix %d (%d x %d): u" % (k, m, n)
        assert TS.same_bits(vt, want[2]), "matrix %d (%d x %d): vt" % (k, m, n)


@pytest.mark.parametrize("name", NAMES)
def test_host_equals_model(pkg, name):
    TS.assert_result(pkg.two_view_reconstruct_host(*TS.model_args(TS.get(name))), TS.reference(name), name)


@pytest.mark.parametrize("name", NAMES)
def test_models_stage_host(pkg, name):
    S = TS.get(name)
    got = pkg.two_view_models_host(S["keys1"], S["keys2"], S["matches12"], S["sigma"], S["iterations"], S["sets"])
    TS.assert_models(got, TS.reference(name)["models"], name)


@pytest.mark.parametrize("name", TS.CHECK_CASES)
def test_check_rt_stage_host(pkg, name):
    TS.assert_checks(pkg.two_view_check_rt_host(*TS.check_args(TS.check_case(name))), TS.check_reference(name), name)


@pytest.mark.parametrize("name", ("first", "last", "twice"))
def test_winner_position_host(pkg, name):
    S = TS.winner_case(name)
    got = pkg.two_view_models_host(S["keys1"], S["keys2"], S["matches12"], S["sigma"], S["iterations"], S["sets"])
    TS.assert_models(got, TS.winner_reference(name), name)


# ---- the scenes are what they claim to be (the model alone) --------------------------------------------------------------------------------
def test_scene_sizes():
    assert [TS.get(n)["N"] for n in ("N8_it1", "N9_it2", "N63", "N64", "N65", "N129")] == [8, 9, 63, 64, 65, 129]
    assert 280 <= TS.get("N300_it64")["N"] <= 320 and 140 <= TS.get("N150_it200")["N"] <= 160
    assert sorted({TS.get(n)["iterations"] for n in NAMES}) == [1, 2, 4, 6, 8, 40, 64, 200]
    for n in ("general", "N300_it64"):
        S = TS.get(n)
        assert len(S["keys1"]) != len(S["keys2"]) and (S["matches12"] < 0).sum() > len(S["keys1"]) - len(S["keys2"]) + 12   # -1 entries beyond the unmatched
        used1, used2 = S["matches12"] >= 0, np.isin(np.arange(len(S["keys2"])), S["matches12"])
        assert (~used1).sum() >= 7 and (~used2).sum() >= 12            # keypoints that no match uses: they still move Normalize


def test_scene_decisions():
    r = TS.reference("planar")
    assert r["used_H"] == 1 and r["ok"] and r["nhyp"] == 8 and r["SH"] / (r["SH"] + r["SF"]) > 0.5
    r = TS.reference("planar_two_solutions")
    assert r["used_H"] == 1 and not r["ok"] and r["why"] == "counts"
    r = TS.reference("general")
    assert r["used_H"] == 0 and r["ok"] and r["nhyp"] == 4
    r = TS.reference("low_parallax")
    assert r["used_H"] == 0 and not r["ok"] and r["why"] == "parallax"      # a clear winner with enough points, below one degree
    assert TM.select_F(list(r["nGood"][:4]), [2.0] * 4, r["N_inliers"]) >= 0
    r = TS.reference("tiny_baseline")
    assert not r["ok"] and r["why"] == "nsimilar > 1"
    r = TS.reference("pure_rotation")
    assert r["used_H"] == 1 and r["nhyp"] == 0 and r["why"].startswith("d1/d2")
    r = TS.reference("coincident")
    assert not r["ok"] and r["SH"] == 0 and r["SF"] == 0 and r["best_it"] == [-1, -1] and r["used_H"] == -1
    assert not r["inliersH"].any() and not r["inliersF"].any()
    assert np.isnan(r["score"]).any() or (r["score"] == 0).all()


def test_scene_degenerate_set_does_not_win():
    r = TS.reference("degenerate_set")
    m = r["models"]
    assert np.isnan(m["score"][0, 0]) and not m["H12"][0].any() and m["best_it"][0] == 1
    assert (m["score"][0, 1:] == m["score"][0, 1]).all()          # equal scores behind it: the first of them stays


def test_scene_winner_positions():
    last = TS.get(TS.WINNER_BASE)["iterations"] - 1
    assert TS.winner_reference("first")["best_it"] == [0, last] and TS.winner_reference("last")["best_it"] == [last, 0]
    tw, base = TS.winner_reference("twice"), TS.reference(TS.WINNER_BASE)
    assert tw["best_it"] == base["best_it"]
    for model in range(2):                                            # the same set scores the same later on and does not replace the winner
        assert TS.same_bits(tw["score"][model, last + 1 + model], tw["score"][model, base["best_it"][model]])


def test_scene_check_rt_cases():
    refs = {n: TS.check_reference(n) for n in TS.CHECK_CASES}
    seen = set()
    for rs in refs.values():
        for r in rs:
            seen |= set(r["status"].tolist())
    for n in NAMES:
        seen |= set(TS.reference(n)["status"].reshape(-1).tolist())
    assert seen == set(range(8)), "every status of CheckRT is reached"
    assert [refs["nGood%d" % k][0]["nGood"] for k in (1, 50, 51, 52, 65)] == [1, 50, 51, 52, 65]
    c = refs["nGood65"][0]["sorted_cos"]
    assert c[49] != c[50] == c[51] == c[54]                           # equal cosParallax values across the rank
    c = refs["nGood52"][0]["sorted_cos"]
    assert c[50] == c[51]
    # both sides of 0.99998 at both depth gates: rejected with parallax ("statuses"), let through without it
    st = refs["statuses"]
    assert (st[1]["status"] == TM.BEHIND1).any() and (st[5]["status"] == TM.BEHIND2).any() and (st[3]["status"] == TM.REPROJ2).any()
    low = refs["gates_low_parallax"][1]
    behind = (low["z1"] <= 0) & (low["z2"] <= 0)
    assert behind.any() and (low["cos"][behind] >= 0.99998).all() and (low["status"][behind] == TM.LOW_PARALLAX).all()
    assert low["nGood"] > 0 and not low["vbGood"].any()               # accepted and counted, but not vbGood


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    S = TS.get("N9_it2")
    args = list(TS.model_args(S))

    def refused(**kw):
        a = dict(zip(("keys1", "keys2", "matches12", "K", "sigma", "iterations", "sets"), args), **kw)
        with pytest.raises(ValueError) as e:
            pkg.two_view_reconstruct_host(a["keys1"], a["keys2"], a["matches12"], a["K"], a["sigma"], a["iterations"], a["sets"])
        return str(e.value)

    few = S["matches12"].copy()
    few[np.flatnonzero(few >= 0)[:2]] = -1
    assert "fewer than 8 matches" in refused(matches12=few)
    assert "iterations < 1" in refused(iterations=0, sets=np.zeros((0, 8), np.int32))
    bad = S["sets"].copy()
    bad[1, 3] = S["N"]
    assert "set index" in refused(sets=bad)
    bad[1, 3] = -1
    assert "set index" in refused(sets=bad)
    far = S["matches12"].copy()
    far[np.flatnonzero(far >= 0)[0]] = len(S["keys2"])
    assert "match index" in refused(matches12=far)
    c = TS.check_case("nGood1")
    with pytest.raises(ValueError):
        pkg.two_view_check_rt_host(c["keys1"], c["keys2"], c["matches12"], c["inliers"], c["K"], 1.0, np.zeros((9, 3, 3)), np.zeros((9, 3)))


def test_every_required_pointer_is_checked(pkg):
    """orbm_two_view_reconstruct_host and the two stage forms with one pointer NULL at a time: ORBX_E_ARG, outputs untouched.  (The
    all-NULL call of every entry is tests/test_abi_null.py's, which enumerates ABI_SYMBOLS.)"""
    L = pkg.load()
    S = TS.get("N9_it2")
    k1, k2, m12, K, sets = S["keys1"], S["keys2"], S["matches12"], S["K"].reshape(9).copy(), S["sets"]
    n1, N, I = len(k1), S["N"], S["iterations"]
    out = dict(R=np.full(9, 7, np.float32), t=np.full(3, 7, np.float32), p=np.full(3 * n1, 7, np.float32), tri=np.full(n1, 7, np.uint8))
    base = [pkg._p(k1), n1, pkg._p(k2), len(k2), pkg._p(m12), pkg._p(K), C.c_float(1.0), I, pkg._p(sets), pkg._p(out["R"]), pkg._p(out["t"]),
            pkg._p(out["p"]), pkg._p(out["tri"]), None]
    for i in (0, 2, 4, 5, 8, 9, 10, 11, 12):
        a = list(base)
        a[i] = None
        assert L.orbm_two_view_reconstruct_host(*a) == pkg.E_ARG, i
        assert b"NULL" in L.orbm_two_view_host_error()
    assert all((v == 7).all() for v in out.values())
    assert L.orbm_two_view_reconstruct_host(*base) in (0, 1)          # the last argument, details, is optional
    bufs = [np.zeros(9 * I, np.float32) for _ in range(3)] + [np.zeros(2 * I, np.float32), np.zeros(2, np.int32), np.zeros(2 * N, np.uint8)]
    base = [pkg._p(k1), n1, pkg._p(k2), len(k2), pkg._p(m12), C.c_float(1.0), I, pkg._p(sets)] + [pkg._p(b) for b in bufs]
    for i in (0, 2, 4, 7, 8, 9, 10, 11, 12, 13):
        a = list(base)
        a[i] = None
        assert L.orbm_two_view_models_host(*a) == pkg.E_ARG, i
    assert L.orbm_two_view_models_host(*base) == 0
    inl, R, t = np.ones(N, np.uint8), np.eye(3, dtype=np.float32).reshape(9), np.array([1, 0, 0], np.float32)
    bufs = [np.zeros(3 * n1, np.float32), np.zeros(n1, np.uint8), np.zeros(N, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.float32),
            np.zeros(1, np.float32)]
    base = [pkg._p(k1), n1, pkg._p(k2), len(k2), pkg._p(m12), pkg._p(inl), pkg._p(K), C.c_float(1.0), 1, pkg._p(R), pkg._p(t)] + [pkg._p(b) for b in bufs]
    for i in (0, 2, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16):
        a = list(base)
        a[i] = None
        assert L.orbm_two_view_check_rt_host(*a) == pkg.E_ARG, i
    assert L.orbm_two_view_check_rt_host(*base) == 0


def test_device_entries_refuse_a_null_handle(pkg):
    L = pkg.load()
    assert L.orbm_two_view_reconstruct(*([None] + [None, 0, None, 0, None, None, C.c_float(1.0), 0] + [None] * 6)) == pkg.E_ARG
    assert L.orbm_two_view_models(*([None] + [None, 0, None, 0, None, C.c_float(1.0), 0] + [None] * 7)) == pkg.E_ARG
    assert L.orbm_two_view_check_rt(*([None] + [None, 0, None, 0, None, None, None, C.c_float(1.0), 0] + [None] * 8)) == pkg.E_ARG


REF_INC = "/root/reference/include"


@pytest.mark.skipif(not os.path.exists(os.path.join(REF_INC, "TwoViewReconstruction.h")) or shutil.which("g++") is None,
                    reason="reference headers or g++ not available")
def test_snippet_typechecks():
    """The drop-in body of TwoViewReconstruction::Reconstruct against the reference's unmodified TwoViewReconstruction.h and its own
    DUtils/Random.h; OpenCV comes from the declaration-only doubles of tests/support/slam_typecheck_stub.  -fsyntax-only."""
    stub = os.path.join(ROOT, "tests", "support", "slam_typecheck_stub")
    cmd = ["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", stub, "-I", REF_INC, "-I", os.path.join(REF_INC, "CameraModels"),
           "-I", "/root/reference", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "3_orb_slam3_selfnote_amd", "csrc", "adapter", "snippets", "TwoViewReconstruction_Reconstruct_hip.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
