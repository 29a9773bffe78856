"""Seeded scenes for Sim3Solver (tests/sim3_model.py is the reference): invented pairs of map points seen from two keyframes whose maps
differ by a similarity, with outliers, and the minimal sets of one call of iterate.  Every scene is a dict(prob, sets, best_in); what a
scene claims to hold is asserted on the model alone in tests/test_sim3_solver_abi.py."""
import functools
import math

import numpy as np

import sim3_model as SM

F = np.float32
PINHOLE = (0, np.array([458.0, 457.0, 367.0, 248.0], F))
PINHOLE_B = (0, np.array([520.9, 521.0, 325.1, 249.7], F))
KB8 = (1, np.array([190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504, 0.0034823894022493434, 0.0007150348452162257,
                    -0.0020532361418706202, 0.00020293673591811182], F))
KB8_B = (1, np.array([190.44236969414825, 190.4344384721956, 252.59949716835982, 254.91723064636983, 0.0034003170790442797, 0.001766278153469831,
                      -0.00266312569781606, 0.0003299517423931039], F))


def level_sigma2(scale, nlevels=8):
    """mvLevelSigma2 of a keyframe (ORBextractor.cc:421-428: mvScaleFactor[i] = mvScaleFactor[i-1]*scaleFactor in float, then its square)"""
    sf, out = F(1.0), []
    for _ in range(nlevels):
        out.append(F(sf * sf))
        sf = F(sf * F(scale))
    return np.array(out, F)


def rot(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def draw(N, iterations, seed):
    """Sets as the reference draws them (:199-213) over a seeded stand-in for rand()"""
    rng = np.random.default_rng(seed)
    sets = np.zeros((iterations, 3), np.int32)
    for it in range(iterations):
        avail = list(range(N))
        for j in range(3):
            randi = int((float(rng.integers(0, 2 ** 31)) / 2147483648.0) * len(avail))
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


def make(N, iterations, seed, cams=(PINHOLE, PINHOLE_B), fix_scale=False, scale=1.6, angle=0.25, outliers=0.3, noise=0.002, min_inliers=None,
         scales=(1.2, 1.2), same_pose=False):
    """N pairs: camera-frame points X1 in front of keyframe 1, X2 = R.t() (X1 - t) / s in keyframe 2 (so X1 = s R X2 + t is the truth), both
    taken to their worlds through invented poses, noise on the second, a fraction replaced by unrelated points.  Pair i < the number of
    true pairs is a true pair; the outliers are the last ones."""
    rng = np.random.default_rng(seed)
    s = 1.0 if fix_scale else scale
    R, t = rot(rng.normal(0, 1, 3), angle), rng.normal(0, 0.15, 3)
    X1 = np.c_[rng.uniform(-1.5, 1.5, N), rng.uniform(-1.0, 1.0, N), rng.uniform(3.0, 8.0, N)]
    X2 = (X1 - t) @ R / s + rng.normal(0, noise, (N, 3))
    n_out = int(round(outliers * N)) if N > 4 else 0
    if n_out:
        X2[N - n_out:] = np.c_[rng.uniform(-1.5, 1.5, n_out), rng.uniform(-1.0, 1.0, n_out), rng.uniform(3.0, 8.0, n_out)] / s
    T1 = pose(rot(rng.normal(0, 1, 3), 0.7), rng.normal(0, 2.0, 3))
    T2 = T1.copy() if same_pose else pose(rot(rng.normal(0, 1, 3), 1.1), rng.normal(0, 3.0, 3))
    Xw1 = (X1 - T1[:3, 3]) @ T1[:3, :3]
    Xw2 = (X2 - T2[:3, 3]) @ T2[:3, :3]
    n1 = N + 7 + seed % 5
    idx1 = np.sort(rng.choice(n1, N, replace=False)).astype(np.int32)
    l1, l2 = level_sigma2(scales[0]), level_sigma2(scales[1])
    prob = dict(n1=n1, idx1=idx1, Xw1=Xw1.astype(F), Xw2=Xw2.astype(F), sigma2_1=l1[rng.integers(0, 4, N)], sigma2_2=l2[rng.integers(0, 4, N)],
                Tcw1=T1.astype(F), Tcw2=T2.astype(F), cam_type1=cams[0][0], cam_params1=cams[0][1], cam_type2=cams[1][0], cam_params2=cams[1][1],
                fix_scale=fix_scale, min_inliers=N if min_inliers is None else min_inliers, iterations_done=0, max_iterations=300)
    return dict(prob=prob, sets=draw(N, iterations, seed + 1000), best_in=0, n_true=N - n_out, truth=(s, R, t), level_tables=(l1, l2))


def good_set(S, k=0):
    """Three true pairs, far apart in the list"""
    n = S["n_true"]
    return [k % n, (k + n // 3) % n, (k + 2 * n // 3) % n]


def bad_set(S, k=0):
    """Two outliers and a true pair"""
    N = len(S["prob"]["idx1"])
    return [N - 1 - k, N - 2 - k, k]


def with_sets(S, sets, **kw):
    S = dict(S, sets=np.array(sets, np.int32).reshape(-1, 3))
    S["prob"] = dict(S["prob"], **{k: v for k, v in kw.items() if k != "best_in"})
    if "best_in" in kw:
        S["best_in"] = kw["best_in"]
    return S


def counts_of(S):
    return SM.solve(S["prob"], S["sets"], 0)["details"]["counts"]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def _convergence(where):
    """Twenty iterations over N = 65: sets with two outliers everywhere except one set of true pairs, at the first, a middle or the last
    iteration; min_inliers between the two kinds of count."""
    S = make(65, 20, 11)
    at = dict(first=0, middle=9, last=19)[where]
    sets = [bad_set(S, k) for k in range(20)]
    sets[at] = good_set(S, 3)
    return with_sets(S, sets, min_inliers=20)


def _converge_late():
    """A hundred iterations over N = 65 with the one set of true pairs at iteration 70: the ordered pass on the device walks the counts 64
    at a time, and this one converges in its second stride."""
    S = make(65, 100, 21)
    sets = [bad_set(S, k % 15) for k in range(100)]
    sets[70] = good_set(S, 3)
    return with_sets(S, sets, min_inliers=20)


def _tie():
    """No convergence, the same set of true pairs at iterations 4 and 13 and poorer sets elsewhere: equal counts, the later wins.
    min_inliers is that count exactly: a count equal to min_inliers does not converge."""
    S = make(65, 20, 12)
    sets = [bad_set(S, k) for k in range(20)]
    sets[4] = sets[13] = good_set(S, 1)
    S = with_sets(S, sets)
    c = counts_of(S)
    return with_sets(S, sets, min_inliers=int(c[4]))


def _best_in_above():
    S = _convergence("middle")
    return with_sets(S, S["sets"], best_in=66, min_inliers=20)


def _between_thresholds():
    """Pair 0 (level 0 in keyframe 1, sigma2 = 1: 9.210 truncates to 9) is moved sideways in keyframe 2's map so that its reprojection into
    image 1 under the true transform misses by 3.02 pixels: err1 = 9.12, above 9 and below 9.21.  Every set is the same three true pairs."""
    S = make(64, 2, 13, noise=0.0, outliers=0.25)
    p = dict(S["prob"])
    s, R, t = S["truth"]
    T1, T2 = np.asarray(p["Tcw1"], np.float64), np.asarray(p["Tcw2"], np.float64)
    X1 = T1[:3, :3] @ np.asarray(p["Xw1"][0], np.float64) + T1[:3, 3]
    fx = float(p["cam_params1"][0])
    X1s = X1 + np.array([3.02 * X1[2] / fx, 0.0, 0.0])          # 3.02 pixels to the side in image 1
    X2 = R.T @ (X1s - t) / s
    Xw2 = np.array(p["Xw2"], F)
    Xw2[0] = (T2[:3, :3].T @ (X2 - T2[:3, 3])).astype(F)
    s1, s2 = np.array(p["sigma2_1"], F), np.array(p["sigma2_2"], F)
    s1[0], s2[0] = S["level_tables"][0][0], S["level_tables"][1][3]
    p.update(Xw2=Xw2, sigma2_1=s1, sigma2_2=s2)
    S = dict(S, prob=p)
    return with_sets(S, [good_set(S, 5), good_set(S, 9)], min_inliers=10)


def _other_keyframe():
    """Pair 0 was matched in another keyframe pKFm whose scale factor is 1.2 while pKF2's is 1.1: at level 1 its sigma2_2 is 1.44 (threshold
    13), where pKF2's table says 1.21 (threshold 11).  Its reprojection into image 2 misses by 3.46 pixels (err2 = 12): an inlier with its own
    keyframe's table, an outlier with pKF2's."""
    S = make(64, 2, 14, noise=0.0, outliers=0.25, scales=(1.2, 1.1))
    p = dict(S["prob"])
    s, R, t = S["truth"]
    T1, T2 = np.asarray(p["Tcw1"], np.float64), np.asarray(p["Tcw2"], np.float64)
    X2 = T2[:3, :3] @ np.asarray(p["Xw2"][0], np.float64) + T2[:3, 3]
    fx = float(p["cam_params2"][0])
    X2s = X2 + np.array([3.46 * X2[2] / fx, 0.0, 0.0])
    X1 = s * R @ X2s + t
    Xw1 = np.array(p["Xw1"], F)
    Xw1[0] = (T1[:3, :3].T @ (X1 - T1[:3, 3])).astype(F)
    s1, s2 = np.array(p["sigma2_1"], F), np.array(p["sigma2_2"], F)
    s1[0], s2[0] = S["level_tables"][0][3], level_sigma2(1.2)[1]
    p.update(Xw1=Xw1, sigma2_1=s1, sigma2_2=s2)
    S = dict(S, prob=p)
    return with_sets(S, [good_set(S, 5), good_set(S, 9)], min_inliers=10)


def _degenerate_points():
    """Keyframe 1 at the world's origin (Tcw1 = I): pair 1 lies in its focal plane (z = 0 exactly), pair 2 behind it."""
    S = make(64, 4, 15)
    p = dict(S["prob"])
    Xw1 = np.array(p["Xw1"], F)
    T1 = np.asarray(p["Tcw1"], np.float64)
    Xw1 = ((Xw1.astype(np.float64) @ T1[:3, :3].T) + T1[:3, 3]).astype(F)      # the same camera coordinates, now with Tcw1 = I
    Xw1[1] = (0.3, 0.2, 0.0)
    Xw1[2] = (0.4, -0.1, -2.5)
    p.update(Xw1=Xw1, Tcw1=np.eye(4, dtype=F))
    S = dict(S, prob=p)
    return with_sets(S, [good_set(S, 5), [1, 2, 7], good_set(S, 9), [2, 30, 40]], min_inliers=50)


def _coincident():
    """Pairs 3, 4 and 5 are one point in both maps: their set has zero relative coordinates, M = 0, a zero quaternion axis: NaN."""
    S = make(64, 3, 16)
    p = dict(S["prob"])
    Xw1, Xw2 = np.array(p["Xw1"], F), np.array(p["Xw2"], F)
    Xw1[4] = Xw1[5] = Xw1[3]
    Xw2[4] = Xw2[5] = Xw2[3]
    p.update(Xw1=Xw1, Xw2=Xw2)
    S = dict(S, prob=p)
    return with_sets(S, [good_set(S, 7), [3, 4, 5], good_set(S, 8)], min_inliers=50)


def _identity():
    """Both keyframes share one pose and pairs 3, 4, 5 are the same three points in both maps: P1 == P2 bit for bit, M symmetric, the
    quaternion (1, 0, 0, 0) exactly, norm(vec) == 0: NaN."""
    S = make(64, 3, 17, same_pose=True)
    p = dict(S["prob"])
    Xw2 = np.array(p["Xw2"], F)
    Xw2[3:6] = np.asarray(p["Xw1"], F)[3:6]
    p.update(Xw2=Xw2)
    S = dict(S, prob=p)
    return with_sets(S, [good_set(S, 7), [3, 4, 5], good_set(S, 8)], min_inliers=50)


SCENES = {
    "N3_it1": lambda: make(3, 1, 1, outliers=0.0, min_inliers=2),
    "N4_it2": lambda: make(4, 2, 2, outliers=0.0, min_inliers=3),
    "N63_kb8": lambda: make(63, 20, 3, cams=(KB8, KB8_B)),
    "N64_fixed": lambda: make(64, 20, 4, fix_scale=True),
    "N65_mixed": lambda: make(65, 20, 5, cams=(PINHOLE, KB8)),
    "N129_it64": lambda: make(129, 64, 6, cams=(KB8_B, PINHOLE_B), min_inliers=85),
    "N300_it300": lambda: make(300, 300, 7, outliers=0.5),
    "half_turn": lambda: make(40, 64, 8, angle=3.0, scale=0.7),
    "converge_first": lambda: _convergence("first"),
    "converge_middle": lambda: _convergence("middle"),
    "converge_last": lambda: _convergence("last"),
    "converge_late": _converge_late,
    "tie_later_wins": _tie,
    "best_in_above": _best_in_above,
    "between_thresholds": _between_thresholds,
    "other_keyframe": _other_keyframe,
    "degenerate_points": _degenerate_points,
    "coincident_set": _coincident,
    "identity_set": _identity,
    "few_pairs": lambda: make(10, 2, 18, min_inliers=20),
    "min_inliers_is_N": lambda: (lambda S: with_sets(S, S["sets"], max_iterations=SM.ransac_iterations(0.99, 20, 300, 20)))(
        make(20, 2, 19, outliers=0.0, min_inliers=20)),
    "chunk_behind_max": lambda: (lambda S: with_sets(S, S["sets"], iterations_done=295, max_iterations=300))(make(30, 20, 20)),
}


@functools.lru_cache(maxsize=None)
def get(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    S = get(name)
    return SM.solve(S["prob"], S["sets"], S["best_in"])


def same_bits(a, b):
    """equal bit patterns (the sign of zero included), NaN by position"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


SCALARS = ("converged", "it_stop", "best_it", "best_inliers", "improved", "no_more")


def assert_result(got, ref, what):
    for k in SCALARS:
        assert getattr(got, k) == ref[k], (what, k, getattr(got, k), ref[k])
    for k in ("T12", "R12", "t12", "s12"):
        assert same_bits(getattr(got, k), ref[k]), (what, k)
    assert np.array_equal(got.best_mask, ref["best_mask"]), (what, "best_mask")
    assert np.array_equal(got.vbInliers, ref["vbInliers"]), (what, "vbInliers")
    if ref["details"] is not None:
        assert_details(got.details, ref["details"], what)


def assert_details(got, ref, what):
    assert np.array_equal(got["counts"], ref["counts"]), (what, "counts", got["counts"], ref["counts"])
    for k in ("quat", "T12", "T21"):
        assert same_bits(got[k], ref[k]), (what, k)
    assert np.array_equal(got["masks"], ref["masks"]), (what, "masks")
