"""CPU: tests/local_map_model.py (the expected values of tests/test_gpu_local_points.py) on hand-computed cases of Frame::isInFrustum
(Frame.cc:572-661) and MapPoint::PredictScale (MapPoint.cc:587-602)."""
import numpy as np
import pytest

import local_map_model as M

f32 = np.float32
PIN = np.array([458.654, 457.296, 367.215, 248.375], f32)
KB8 = np.array([190.978477, 190.973307, 254.931706, 256.897442, 0.003482389402, 0.000715034845, -0.002053236141, 0.000202936736], f32)
SF = [f32(1.0)]
for _ in range(7):
    SF.append(f32(SF[-1] * f32(1.2)))
LOG_SF = float(M.glibc_logf(f32(1.2)))


def run(oracle, Xw, maxd, mind, normal=None, cam_type=0, bounds=(0.0, 752.0, 0.0, 480.0), limit=0.5, tz=0.0, elig=None):
    Xw = np.asarray(Xw, f32).reshape(-1, 3)
    n = len(Xw)
    T = np.eye(4, dtype=f32)
    T[2, 3] = tz
    normal = np.tile(f32([0, 0, 1]), (n, 1)) if normal is None else normal
    elig = np.ones(n, np.uint8) if elig is None else elig
    return M.is_in_frustum(Xw, normal, np.asarray(maxd, f32), np.asarray(mind, f32), elig, T, cam_type, PIN if cam_type == 0 else KB8,
                           bounds, 8, LOG_SF, 47.9, limit, oracle.project)


def test_level_of_max_dist_at_scale_factor_powers(oracle):
    d = f32(4.0)
    t = run(oracle, [[0, 0, d]] * 9, [f32(d * SF[k]) for k in range(8)] + [f32(d * SF[7] * f32(1.44))], [f32(1.0)] * 9)
    assert t["in_view"].all()
    assert list(t["level"]) == list(range(8)) + [7]            # the last one clamps at nlevels - 1
    assert (t["depth"] == d).all() and (t["view_cos"] == 1).all()


def test_level_below_zero_clamps():
    assert M.cvtt_f32_i32(f32(-1.0)) == -1 and M.cvtt_f32_i32(f32(-2.5)) == -2 and M.cvtt_f32_i32(f32(2.9)) == 2
    assert M.cvtt_f32_i32(f32(np.nan)) == M.INT_MIN and M.cvtt_f32_i32(f32(np.inf)) == M.INT_MIN and M.cvtt_f32_i32(f32(2.0 ** 31)) == M.INT_MIN


def test_level_clamp_at_the_max_gate(oracle):
    d = f32(4.0)
    maxd = f32(d / f32(1.2))          # dist == 1.2 * max_dist (within float rounding): ratio ~ 1/1.2 -> ceil(-1) -> 0
    t = run(oracle, [[0, 0, d]], [maxd], [f32(1.0)])
    if t["in_view"][0]:
        assert t["level"][0] == 0


def test_negative_zero_depth_passes(oracle):
    # KannalaBrandt8 projects a point with PcZ = -0 inside the image; only PcZ < 0 is rejected
    t = run(oracle, [[-1, -1, -0.0], [-1, -1, -1e-3]], [10, 10], [0.1, 0.1], cam_type=1, bounds=(0.0, 512.0, 0.0, 512.0), tz=-0.0, limit=-2.0)
    assert t["proj_x"][0] != -1 and t["in_view"][0] == 1
    assert t["proj_x"][1] == -1 and t["in_view"][1] == 0
    # Pinhole: PcZ = +0 gives an infinite projection, rejected by the bounds
    t = run(oracle, [[1, 0, 0.0]], [10], [0.1])
    assert t["in_view"][0] == 0 and t["proj_x"][0] == -1


def test_point_at_the_camera_centre(oracle):
    t = run(oracle, [[0, 0, 0]], [1.0], [0.0])
    assert t["in_view"][0] == 1 and np.isnan(t["proj_x"][0]) and np.isnan(t["view_cos"][0])
    assert t["depth"][0] == 0 and t["level"][0] == 0


def test_bounds_are_inclusive(oracle):
    A, B = [-1.0, -0.5, 5.0], [1.0, 0.7, 5.0]
    ua, va = oracle.project(0, PIN, *A)
    ub, vb = oracle.project(0, PIN, *B)
    t = run(oracle, [A, B], [10, 10], [1, 1], bounds=(ua, ub, va, vb))
    assert t["in_view"].all()
    up = lambda x: float(np.nextafter(f32(x), f32(np.inf)))
    dn = lambda x: float(np.nextafter(f32(x), f32(-np.inf)))
    for b in ((up(ua), ub, va, vb), (ua, ub, up(va), vb)):
        t = run(oracle, [A], [10], [1], bounds=b)
        assert t["in_view"][0] == 0 and t["proj_x"][0] == -1
    for b in ((ua, dn(ub), va, vb), (ua, ub, va, dn(vb))):
        t = run(oracle, [B], [10], [1], bounds=b)
        assert t["in_view"][0] == 0 and t["proj_x"][0] == -1


def test_view_cos_at_the_limit(oracle):
    P = [0.3, 0.2, 4.0]
    nrm = np.array([[0.6, 0.0, 0.8]], f32)
    t = run(oracle, [P], [10], [1], normal=nrm, limit=-2.0)
    vc = t["view_cos"][0]
    assert 0 < vc < 1
    assert run(oracle, [P], [10], [1], normal=nrm, limit=float(vc))["in_view"][0] == 1
    t = run(oracle, [P], [10], [1], normal=nrm, limit=float(np.nextafter(vc, f32(2))))
    assert t["in_view"][0] == 0 and t["proj_x"][0] != -1      # the projection is written before the angle test


def test_depth_exactly_th_far(oracle):
    t = run(oracle, [[0.2, 0.1, 3.0], [0.1, 0.1, 8.0]], [20, 20], [1, 1])
    dep = t["depth"][0]
    elig = np.ones(2, np.uint8)
    assert list(M.query_mask(t, elig, True, dep)) == [1, 0]
    assert list(M.query_mask(t, elig, True, np.nextafter(dep, f32(0)))) == [0, 0]
    assert list(M.query_mask(t, elig, False, 0.0)) == [1, 1]


def test_ineligible_points_are_left_alone(oracle):
    t = run(oracle, [[0, 0, 4.0], [0, 0, 4.0]], [10, 10], [1, 1], elig=np.array([0, 1], np.uint8))
    assert t["in_view"][0] == 0 and t["proj_x"][0] == 0 and t["in_view"][1] == 1


@pytest.mark.parametrize("which", ["min", "max"])
def test_distance_gates(oracle, which):
    d = f32(4.0)
    base = [f32(1.0), f32(10.0)]
    got = []
    for k in range(-3, 4):
        if which == "min":
            g = f32(d / f32(0.8))
            mind, maxd = np.nextafter(g, f32(np.inf)) if k > 0 else g, base[1]
            for _ in range(abs(k)):
                mind = np.nextafter(mind, f32(np.inf) if k > 0 else f32(0))
        else:
            g = f32(d / f32(1.2))
            mind, maxd = base[0], g
            for _ in range(abs(k)):
                maxd = np.nextafter(maxd, f32(np.inf) if k > 0 else f32(0))
        got.append(int(run(oracle, [[0, 0, d]], [maxd], [mind])["in_view"][0]))
    assert 0 in got and 1 in got                                # both sides of the gate are reached
    assert got == sorted(got, reverse=(which == "min"))         # and it is a single threshold
