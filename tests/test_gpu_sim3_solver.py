"""GPU: Sim3Solver on the device (orbm_sim3_solve, orbm_sim3_hypotheses, orbm_sim3_check; k_sim3_hypotheses, k_sim3_check, k_sim3_winner;
Sim3Solver.cc:35-530).  No tolerance anywhere: floats are compared as bits, NaN by position.

  * The device entry equals the literal model of tests/sim3_model.py on every scene of tests/sim3_scene.py - N = 3, 4, 63, 64, 65, 129, 300;
    iterations 1, 2, 20, 64, 100, 300; both camera models in all four pairings; fixed and free scale - on every output including the optional
    ones, and equals the host entry on the same inputs.
  * Both stage entries equal the model: every iteration's T12, T21 and quaternion row; counts and masks for the model's transforms.
  * Two calls on one handle with other orbm_* calls between them give the first call's bits again.
  * One chained case: a row of SearchByBoWKeyFramesCandidates becomes the solver's pairs (geometry invented on top of the BoW scene), and the
    winning T12 goes into the Sim3 SearchByProjection, which is held against the oracle fed the same transform."""
import numpy as np
import pytest

import bow_candidates_scene as BS
import sim3_model as SM
import sim3_scene as TS

pytestmark = pytest.mark.gpu
NAMES = tuple(TS.SCENES)


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.ORBmatcher(0.9, True)
    yield m
    m.close()


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_model_and_host(pkg, matcher, name):
    S = TS.get(name)
    got = matcher.Sim3Solve(S["prob"], S["sets"], S["best_in"])
    TS.assert_result(got, TS.reference(name), name)
    host = pkg.sim3_solve_host(S["prob"], S["sets"], S["best_in"])
    for k in TS.SCALARS:
        assert getattr(got, k) == getattr(host, k), (name, k)
    for k in ("T12", "R12", "t12", "s12"):
        assert TS.same_bits(getattr(got, k), getattr(host, k)), (name, k)
    assert np.array_equal(got.best_mask, host.best_mask) and np.array_equal(got.vbInliers, host.vbInliers)
    for k, v in got.details.items():
        assert TS.same_bits(v, host.details[k]) if v.dtype == np.float32 else np.array_equal(v, host.details[k]), (name, k)


@pytest.mark.parametrize("name", [n for n in NAMES if n != "few_pairs"])
def test_stage_entries(matcher, name):
    S, ref = TS.get(name), TS.reference(name)["details"]
    got = matcher.Sim3Hypotheses(S["prob"], S["sets"])
    for k in ("T12", "T21", "quat"):
        assert TS.same_bits(got[k], ref[k]), (name, k)
    chk = matcher.Sim3Check(S["prob"], ref["T12"], ref["T21"])
    assert np.array_equal(chk["counts"], ref["counts"]) and np.array_equal(chk["masks"], ref["masks"]), name


def test_two_calls_with_other_entries_between(pkg, matcher):
    S, big = TS.get("N65_mixed"), TS.get("N300_it300")
    first = matcher.Sim3Solve(S["prob"], S["sets"], S["best_in"])
    rng = np.random.default_rng(8)
    q, c = rng.integers(0, 256, (40, 32), dtype=np.uint8), rng.integers(0, 256, (70, 32), dtype=np.uint8)
    idx2, dist2 = np.zeros(80, np.int32), np.zeros(80, np.int32)
    assert matcher.L.orbm_knn_match2(matcher.m, pkg._p(q), 40, pkg._p(c), 70, pkg._p(idx2), pkg._p(dist2)) == 0
    matcher.Sim3Solve(big["prob"], big["sets"], big["best_in"])            # a larger block on the same handle
    ref = TS.reference("N129_it64")["details"]
    matcher.Sim3Check(TS.get("N129_it64")["prob"], ref["T12"][:5], ref["T21"][:5])
    again = matcher.Sim3Solve(S["prob"], S["sets"], S["best_in"])
    TS.assert_result(again, TS.reference("N65_mixed"), "N65_mixed again")
    assert TS.same_bits(first.details["T12"], again.details["T12"]) and np.array_equal(first.details["masks"], again.details["masks"])


def test_chained_from_bow_rows_into_projection_search(pkg, oracle, matcher):
    B = BS.scene()
    base, j = B["base"], 2
    cand = B["cands"][j]
    KF1, KF2 = BS.product_fixed(pkg, B, "kf"), BS.product_cand(pkg, B, j, "kf")
    nm, rows = matcher.SearchByBoWKeyFramesCandidates(KF1, [KF2])
    row = rows[0]
    assert nm[0] >= 20, "the chained case needs matches"
    # geometry on top of the BoW scene: keyframe 1 at its world's origin sees the map point of base keypoint i along that keypoint's ray; the
    # candidate's map of the same points differs by a similarity and sits behind another pose; every ninth candidate point is unrelated
    cam = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
    rng = np.random.default_rng(41)
    nb, nc = len(base["k"]), len(cand["k"])
    z = rng.uniform(3.0, 7.0, nb)
    X1 = np.c_[(base["k"]["x"] - cam[2]) / cam[0] * z, (base["k"]["y"] - cam[3]) / cam[1] * z, z]
    s, R, t = 1.3, TS.rot((0.2, 1.0, 0.1), 0.2), np.array([0.1, -0.05, 0.2])
    src = np.array(cand["src"])
    X2 = np.c_[rng.uniform(-3, 3, nc), rng.uniform(-2, 2, nc), rng.uniform(3, 7, nc)]
    has = src >= 0
    X2[has] = (X1[src[has]] - t) @ R / s + rng.normal(0, 0.002, (int(has.sum()), 3))
    wrong = np.arange(nc) % 9 == 4
    X2[wrong] = np.c_[rng.uniform(-3, 3, int(wrong.sum())), rng.uniform(-2, 2, int(wrong.sum())), rng.uniform(3, 7, int(wrong.sum()))]
    T2 = TS.pose(TS.rot((1.0, 0.3, -0.2), 0.9), np.array([1.0, -2.0, 0.5]))
    Xw2 = ((X2 - T2[:3, 3]) @ T2[:3, :3]).astype(np.float32)
    idx1 = np.flatnonzero(row >= 0).astype(np.int32)
    N = len(idx1)
    prob = dict(n1=nb, idx1=idx1, Xw1=X1[idx1].astype(np.float32), Xw2=Xw2[row[idx1]], sigma2_1=B["sigma2"][base["k"]["octave"][idx1]],
                sigma2_2=B["sigma2"][cand["k"]["octave"][row[idx1]]], Tcw1=np.eye(4, dtype=np.float32), Tcw2=T2.astype(np.float32), cam_type1=0,
                cam_params1=cam, cam_type2=0, cam_params2=cam, fix_scale=False, min_inliers=N // 3,
                max_iterations=SM.ransac_iterations(0.99, N // 3, 300, N))
    sets = TS.draw(N, 20, 5)
    got = matcher.Sim3Solve(prob, sets, 0)
    TS.assert_result(got, SM.solve(prob, sets, 0), "chained")
    assert got.converged and got.best_inliers > N // 3
    # LoopClosing.cc:875-879: gScm = the solver's T12, gScw = gScm * gSmw; the candidate's map points into keyframe 1
    Scw = (got.T12.astype(np.float64) @ T2).astype(np.float32)
    sf = B["sf"]
    log_sf = float(np.log(np.float32(1.2)))
    A = Scw[:3, :3].astype(np.float64)
    Ow = -np.linalg.solve(A, Scw[:3, 3].astype(np.float64))
    d = Xw2.astype(np.float64) - Ow
    dist = np.linalg.norm(d, axis=1)
    normal = (d / dist[:, None]).astype(np.float32)
    octave = np.where(has, base["k"]["octave"][np.maximum(src, 0)], cand["k"]["octave"])
    max_dist = (dist * sf[octave]).astype(np.float32)
    min_dist = (max_dist / sf[-1]).astype(np.float32)
    valid = cand["mpS"].astype(np.uint8)
    bounds = (0.0, 752.0, 0.0, 480.0)
    KF = pkg.FrameView(base["k"], base["d"], bounds)
    OKF = oracle.OracleFrame(base["k"]["x"], base["k"]["y"], base["k"]["octave"], base["k"]["angle"], base["d"], bounds, sf)
    n_gpu = matcher.SearchByProjectionSim3(KF, sf, log_sf, valid, Xw2, normal, cand["d"], max_dist, min_dist, Scw, cam, 8, 1.0, cam_type=0)
    n_ref = oracle.search_by_projection_sim3(OKF, valid, Xw2, normal, cand["d"], max_dist, min_dist, Scw, cam, log_sf, 8, 1.0, cam_type=0)
    assert n_gpu == n_ref and n_ref >= 20
    assert np.array_equal(KF.slot, OKF.slot) and np.array_equal(KF.slot_obs, OKF.slot_obs)
