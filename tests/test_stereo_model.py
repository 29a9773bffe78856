"""CPU: the two pieces of bookkeeping orbx_compute_stereo_matches_batch_device adds (tests/stereo_model.py) against the reference's
own forms, and the model as a whole against the CPU oracle, bit for bit, on the scene list tests/test_gpu_stereo_batch.py runs on
the device.  Also prints, per scene, the accepted matches and what the filter removes: the GPU tests' conditions."""
import numpy as np
import pytest

import stereo_model as SM

_cache = {}


def scenes(synth):
    if "scenes" not in _cache:
        flat = SM.flat_image()
        ordinary = SM.scene_list(synth)
        _cache["scenes"] = ([("disp%d" % d, p) for d, p in zip(SM.DISPARITIES, ordinary)] +
                            [("identical", SM.identical_pair(synth)), ("flat-left", (flat, ordinary[1][1])),
                             ("flat-right", (ordinary[1][0], flat)), ("flat-both", (flat, flat))])
    return _cache["scenes"]


def run(oracle, name, pair):
    if name not in _cache:
        o, lvL, lvR, sf, invsf, kL, dL, kR, dR = SM.oracle_inputs(oracle, SM.EUROC_STEREO, *pair)
        ref = o.compute_stereo_matches(pair[0], pair[1], kL, dL, kR, dR, SM.MB, SM.MBF)
        got = SM.compute_stereo_matches(lvL, lvR, sf, invsf, kL, dL, kR, dR, SM.MB, SM.MBF, order_rng=np.random.default_rng(len(name)))
        _cache[name] = (ref, got, (lvL, sf, kL, kR))
    return _cache[name]


def test_band_candidates_equal_the_row_table(oracle, synth):
    """(i): for every left keypoint, the records of its band that pass the exact row test are vRowIndices[(int)vL] as a set."""
    for name, pair in scenes(synth)[:7]:
        _, (_, _, info), (lvL, sf, kL, kR) = run(oracle, name, pair)
        rows = lvL[0].shape[0]
        ref = SM.reference_row_table(kR["y"], kR["octave"], sf, rows)
        looked = 0
        for iL in range(len(kL)):
            row = int(kL["y"][iL])
            assert 0 <= row < rows
            assert info["candidates"][iL].tolist() == sorted(ref[row]), (name, iL)
            looked += len(ref[row])
        assert looked >= 10 * len(kL)          # about 18 per keypoint at these settings: the comparison is not over empty sets
        start = SM.band_table(kR["y"], kR["octave"], sf, rows)[0]
        assert start[-1] <= len(kR) * SM.max_bands_per_keypoint(sf, rows)      # the host's scratch bound


def test_band_bound_for_every_pyramid():
    """A keypoint covers at most 2r + 3 rows (+ 1 for rounding), r = 2 * scale: the bound on the bands it enters, at the extremes."""
    rng = np.random.default_rng(3)
    for nlevels, factor in ((1, 1.2), (3, 1.2), (8, 1.2), (16, 1.2), (8, 2.0), (5, 1.1)):
        sf = np.array([np.float32(factor) ** l for l in range(nlevels)], np.float32)
        rows = 480
        ky = rng.uniform(-40, rows + 40, 4000).astype(np.float32)
        ky[:rows] = np.arange(rows, dtype=np.float32) + np.float32(0.999)
        octv = rng.integers(0, nlevels, len(ky))
        octv[:rows] = nlevels - 1
        start, idx, _, _ = SM.band_table(ky, octv, sf, rows)
        per = np.bincount(idx, minlength=len(ky)) if len(idx) else np.zeros(len(ky), int)
        assert per.max() <= SM.max_bands_per_keypoint(sf, rows), (nlevels, factor, per.max())


def test_rank_selection_equals_sort(oracle, synth):
    """(ii): two histogram passes + one threshold compare reset exactly what sort + descending loop reset."""
    rng = np.random.default_rng(11)
    cases = [[0], [5], [0, 0, 0], [7, 7, 7, 7], [1, 2], [2, 1, 3], [61710, 0], [255, 256, 257], [65535] * 5 + [0] * 5, list(range(600))]
    for _ in range(300):
        n = int(rng.integers(1, 1500))
        kind = rng.integers(0, 4)
        if kind == 0:
            cases.append(rng.integers(0, 61711, n))
        elif kind == 1:
            cases.append(rng.integers(0, 40, n) * int(rng.integers(1, 300)))       # many ties
        elif kind == 2:
            cases.append((rng.gamma(2.0, 600.0, n)).clip(0, 61710).astype(np.int64))  # shaped like real SADs
        else:
            cases.append(np.full(n, int(rng.integers(0, 61711))))
    for name, pair in scenes(synth)[:7]:
        sad = run(oracle, name, pair)[1][2]["sad"]
        cases.append(sad[sad >= 0])
    for c in cases:
        c = np.asarray(c, np.int64)
        assert SM.rank_select(c) == sorted(c.tolist())[len(c) // 2]
        assert np.array_equal(SM.filter_select(c), SM.filter_sort(c))
    assert len(SM.filter_select([])) == 0


def test_model_equals_oracle(oracle, synth):
    """The whole restatement, band table and selection filter included, against the oracle: bit patterns of mvuRight and mvDepth."""
    for name, pair in scenes(synth):
        (uR_ref, z_ref), (uR, z, info), _ = run(oracle, name, pair)
        print("%-10s keypoints %4d  accepted %4d  removed %4d  remaining %4d" % (name, len(uR), info["accepted"], info["removed"], info["remaining"]))
        assert np.array_equal(uR.view(np.uint32), uR_ref.view(np.uint32)), name
        assert np.array_equal(z.view(np.uint32), z_ref.view(np.uint32)), name
        assert info["remaining"] == int((uR_ref >= 0).sum())
        if name.startswith("disp"):
            assert info["remaining"] >= 500 and info["removed"] >= 20, (name, info["remaining"], info["removed"])
        elif name == "identical":
            assert info["accepted"] >= 300 and info["remaining"] == 0      # SAD 0 everywhere: median 0, thDist 0, all reset
        else:
            assert info["accepted"] == 0 and (len(uR) == 0 or (uR == -1).all())


def test_reference_table_form_gives_the_same(oracle, synth):
    """The model run over the reference's own row table (no bands) gives the same bits: the band form changes nothing."""
    name, pair = scenes(synth)[3]
    o, lvL, lvR, sf, invsf, kL, dL, kR, dR = SM.oracle_inputs(oracle, SM.EUROC_STEREO, *pair)
    a = SM.compute_stereo_matches(lvL, lvR, sf, invsf, kL, dL, kR, dR, SM.MB, SM.MBF, use_bands=False)
    b = run(oracle, name, pair)[1]
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[2]["sad"], b[2]["sad"])
