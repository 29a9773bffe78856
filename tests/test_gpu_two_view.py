"""GPU: TwoViewReconstruction::Reconstruct on the device (orbm_two_view_reconstruct, orbm_two_view_models, orbm_two_view_check_rt;
k_tv_hypotheses, k_tv_score, k_tv_winner, k_tv_check_rt, k_tv_cos_rank; TwoViewReconstruction.cc:39-933).  No tolerance anywhere: floats are
compared as bits, NaN by position.

  * The device entry equals the literal model of tests/twoview_model.py on every scene of tests/twoview_scene.py - N = 8, 9, 63, 64, 65,
    129, 296; iterations 1, 2, 4, 6, 8, 40, 64, 200 - on every output including the optional ones, and equals the host entry on the same inputs.
  * Both stage entries equal the model: every iteration's H21, H12, F21 and score with the winners and their inlier vectors; CheckRT
    for chosen hypotheses that reach every status, nGood = 1, 50, 51, 52 and 65 with equal cosParallax values across the rank.
  * Winners at the first and at the last iteration, and an earlier one of two identical sets.
  * Two calls on one handle with other orbm_* calls between them give the first call's bits again.
  * One chained case: two synthetic frames, the second a known shift of the first, through extraction, SearchForInitialization and the
    new entry, against the model fed the same matches, whichever decision it reaches.
The handle's entries make no promise for two host threads on ONE handle (the reference gives every thread its own matcher), so none is
tested."""
import numpy as np
import pytest

import twoview_model as TM
import twoview_scene as TS

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
    got = matcher.TwoViewReconstruct(*TS.model_args(S))
    TS.assert_result(got, TS.reference(name), name)
    host = pkg.two_view_reconstruct_host(*TS.model_args(S))
    for k, v in got.details.items():
        assert TS.same_bits(v, host.details[k]) if v.dtype == np.float32 else np.array_equal(v, host.details[k]), (name, k)
    assert got.ok == host.ok
    if got.ok:
        assert TS.same_bits(got.R21, host.R21) and TS.same_bits(got.t21, host.t21) and TS.same_bits(got.vP3D, host.vP3D)
        assert np.array_equal(got.vbTriangulated, host.vbTriangulated)


@pytest.mark.parametrize("name", NAMES)
def test_models_stage(matcher, name):
    S = TS.get(name)
    got = matcher.TwoViewModels(S["keys1"], S["keys2"], S["matches12"], S["sigma"], S["iterations"], S["sets"])
    TS.assert_models(got, TS.reference(name)["models"], name)


@pytest.mark.parametrize("name", TS.CHECK_CASES)
def test_check_rt_stage(matcher, name):
    got = matcher.TwoViewCheckRT(*TS.check_args(TS.check_case(name)))
    TS.assert_checks(got, TS.check_reference(name), name)


@pytest.mark.parametrize("name", ("first", "last", "twice"))
def test_winner_position(matcher, name):
    S, ref = TS.winner_case(name), TS.winner_reference(name)
    got = matcher.TwoViewModels(S["keys1"], S["keys2"], S["matches12"], S["sigma"], S["iterations"], S["sets"])
    TS.assert_models(got, ref, name)


def test_two_calls_with_other_entries_between(pkg, matcher):
    S, big = TS.get("N65"), TS.get("N300_it64")
    first = matcher.TwoViewReconstruct(*TS.model_args(S))
    rng = np.random.default_rng(8)
    q, c = rng.integers(0, 256, (40, 32), dtype=np.uint8), rng.integers(0, 256, (70, 32), dtype=np.uint8)
    idx2 = np.zeros(80, np.int32)
    dist2 = np.zeros(80, np.int32)
    assert matcher.L.orbm_knn_match2(matcher.m, pkg._p(q), 40, pkg._p(c), 70, pkg._p(idx2), pkg._p(dist2)) == 0
    matcher.TwoViewReconstruct(*TS.model_args(big))                      # a larger block on the same handle
    matcher.TwoViewCheckRT(*TS.check_args(TS.check_case("nGood51")))
    again = matcher.TwoViewReconstruct(*TS.model_args(S))
    TS.assert_result(again, TS.reference("N65"), "N65 again")
    assert first.ok == again.ok and TS.same_bits(first.details["score"], again.details["score"])


def test_chained_from_extraction(pkg, synth, matcher):
    cfg = dict(nfeatures=500, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7)
    frames, offs = synth.make_stream(77, 2, H=130, W=150, margin=16)
    ex = pkg.ORBextractor(device=0, **cfg)
    views = []
    for f in frames:
        _, kps, desc = ex(f, None, (0, 1000))
        views.append(pkg.FrameView(kps, desc, (0.0, 150.0, 0.0, 130.0)))
    F1, F2 = views
    prev = np.ascontiguousarray(np.c_[F1.keys_un["x"], F1.keys_un["y"]], dtype=np.float32)
    nmatches, m12 = matcher.SearchForInitialization(F1, F2, prev, 20)
    assert nmatches >= 8, "the chained case needs eight matches"
    sets = TS.draw(nmatches, 8, 21)
    K = np.array([[120, 0, 75], [0, 120, 65], [0, 0, 1]], np.float32)
    got = matcher.TwoViewReconstruct(F1.keys_un, F2.keys_un, m12, K, 1.0, 8, sets)
    TS.assert_result(got, TM.reconstruct(F1.keys_un, F2.keys_un, m12, K, 1.0, 8, sets), "chained")
