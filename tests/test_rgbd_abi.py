"""CPU: orbx_stereo_from_rgbd_batch_device and orbx_close_points_batch_device exist on both sides of the ABI, their refusals that
need no device, the closed form of the visiting rule against the literal loop of tests/rgbd_model.py, and the conditions the
synthetic RGB-D scenes of tests/test_gpu_rgbd.py must meet for its comparisons to mean something.  The refusals that are worth
checking next to live buffers are in tests/test_gpu_rgbd.py::test_refusals_with_live_buffers."""
import ctypes as C
import inspect

import numpy as np
import pytest

import rgbd_model as RM


def test_symbols_and_mirrors(pkg):
    L = pkg.load()
    for name, nargs in (("orbx_stereo_from_rgbd_batch_device", 18), ("orbx_close_points_batch_device", 20)):
        assert name in pkg.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    sig = inspect.signature(pkg.stereo_from_rgbd_batch_device)
    assert list(sig.parameters) == ["nframes", "d_keys", "d_keys_un", "d_counts", "count_stride", "cap", "d_depth_image", "depth_type", "rows", "cols",
                                    "row_stride", "frame_stride", "depth_factor", "mbf", "d_uRight", "d_depth", "d_nstereo", "stream"]
    assert sig.parameters["d_nstereo"].default is None and sig.parameters["stream"].default is None
    sig = inspect.signature(pkg.close_points_batch_device)
    assert list(sig.parameters) == ["nframes", "d_depth", "d_counts", "count_stride", "cap", "th_depth", "max_point", "d_order", "d_nvisit", "d_tracked",
                                    "d_close", "d_keys_un", "fx", "fy", "cx", "cy", "d_x3Dc", "d_pose", "d_x3Dw", "stream"]
    for name in ("d_tracked", "d_close", "d_keys_un", "d_x3Dc", "d_pose", "d_x3Dw", "stream"):
        assert sig.parameters[name].default is None
    assert pkg.CLOSE_MAX_KEYPOINTS == 4096


def host_buffers(pkg, n=2, cap=8, H=6, W=10):
    """Host arrays standing in for device buffers: a refused call never touches them."""
    B = dict(keys=np.zeros((n, cap), pkg.KP_DTYPE), keys_un=np.zeros((n, cap), pkg.KP_DTYPE), cnt=np.zeros((n, 2), np.int32),
             img=np.zeros((n, H, W), np.uint16), uR=np.zeros((n, cap), np.float32), z=np.zeros((n, cap), np.float32),
             order=np.zeros((n, cap), np.int32), nv=np.zeros(n, np.int32), x3=np.zeros((n, cap, 3), np.float32), pose=np.zeros((n, 12), np.float32))
    return {k: v.ctypes.data for k, v in B.items()}, B


def test_lookup_refusals_without_device(pkg):
    n, cap, H, W = 2, 8, 6, 10
    p, keep = host_buffers(pkg, n, cap, H, W)
    good = dict(nframes=n, d_keys=p["keys"], d_keys_un=p["keys_un"], d_counts=p["cnt"], count_stride=2, cap=cap, d_depth_image=p["img"], depth_type=0,
                rows=H, cols=W, row_stride=2 * W, frame_stride=2 * W * H, depth_factor=1.0, mbf=40.0, d_uRight=p["uR"], d_depth=p["z"])
    bad = [dict(d_keys=0), dict(d_keys_un=0), dict(d_counts=0), dict(d_depth_image=0), dict(d_uRight=0), dict(d_depth=0), dict(nframes=-1), dict(cap=0),
           dict(cap=-3), dict(depth_type=2), dict(depth_type=-1), dict(row_stride=2 * W - 2), dict(row_stride=2 * W + 1), dict(depth_type=1),   # a float row needs 4 W bytes
           dict(depth_type=1, row_stride=4 * W + 2, frame_stride=(4 * W + 2) * H), dict(rows=0), dict(cols=0), dict(count_stride=0),
           dict(frame_stride=2 * W * H - 2), dict(frame_stride=2 * W * H + 1)]
    for c in bad:
        with pytest.raises(ValueError):
            pkg.stereo_from_rgbd_batch_device(**dict(good, **c))
    assert pkg.stereo_from_rgbd_batch_device(**dict(good, nframes=0)) == 0          # nothing to do, nothing launched


def test_close_points_refusals_without_device(pkg):
    n, cap = 2, 8
    p, keep = host_buffers(pkg, n, cap)
    good = dict(nframes=n, d_depth=p["z"], d_counts=p["cnt"], count_stride=2, cap=cap, th_depth=3.2, max_point=100, d_order=p["order"], d_nvisit=p["nv"])
    unproj = dict(d_keys_un=p["keys_un"], fx=500.0, fy=500.0, cx=5.0, cy=3.0, d_x3Dc=p["x3"])
    bad = [dict(d_depth=0), dict(d_counts=0), dict(d_order=0), dict(d_nvisit=0), dict(nframes=-1), dict(cap=0), dict(cap=pkg.CLOSE_MAX_KEYPOINTS + 1),
           dict(count_stride=0), dict(d_x3Dc=p["x3"]),                                       # unprojection without mvKeysUn
           dict(unproj, d_pose=p["pose"]), dict(unproj, d_x3Dw=p["x3"]),                     # pose and world output come together
           dict(d_keys_un=p["keys_un"], d_pose=p["pose"], d_x3Dw=p["x3"])]                   # world output needs the camera output
    for c in bad:
        with pytest.raises(ValueError):
            pkg.close_points_batch_device(**dict(good, **c))
    assert pkg.close_points_batch_device(**dict(good, nframes=0)) == 0


@pytest.mark.parametrize("max_point", [100, 0])
def test_closed_form_equals_the_loop(max_point):
    """nvisit = min(m, max(c, maxPoint) + 1) against the literal loop, m = #{z > 0}, c = #{0 < z <= th}: the c closest depths at or
    below the threshold (the last one exactly on it), the others above, some keypoints without depth in between."""
    th = RM.TEST_TH_DEPTH
    rng = np.random.default_rng(3)
    for m in (0, 1, 99, 100, 101, 102, 300):
        for c in sorted(set(min(c, m) for c in (0, 99, 100, 101, m))):
            z = np.concatenate([np.linspace(0.5, float(th), c).astype(np.float32)[::-1] if c else np.zeros(0, np.float32),
                                (th + np.float32(0.01) * np.arange(1, m - c + 1)).astype(np.float32), np.array([0, -1, np.nan], np.float32)])
            if c:
                z[0] = th
            z = z[rng.permutation(len(z))]
            assert int((z > 0).sum()) == m and int(((z > 0) & (z <= th)).sum()) == c
            order, _, nn = RM.close_points(z, th, max_point)
            assert len(order) == RM.nvisit_closed_form(m, c, max_point), (m, c, max_point, len(order))
            assert nn == int(((z > 0) & (z < th)).sum())
            zo = z[order]
            assert (np.diff(zo) >= 0).all() and sorted(order) == sorted(np.argsort(np.where(z > 0, z, np.inf), kind="stable")[:len(order)].tolist())


@pytest.mark.parametrize("seed", [1000, 1001])
def test_scene_conditions(oracle, synth, seed):
    """The chain test's frames: enough keypoints with and without depth, depth values shared between keypoints (so the order needs
    its tie rule), more close points than the 100 the rule would take anyway."""
    assert RM.TUM1_FACTOR == np.float32(1 / 5000)
    S = RM.scene(oracle, synth, seed)
    z = S["depth"]
    with_depth, without = int((z > 0).sum()), int((z <= 0).sum())
    vals, cnt = np.unique(z[z > 0], return_counts=True)
    shared = int(cnt[cnt > 1].sum())
    order, _, _ = RM.close_points(z, RM.TEST_TH_DEPTH, 100)
    close = int(((z > 0) & (z <= RM.TEST_TH_DEPTH)).sum())
    print("seed %d: %d keypoints, %d with depth, %d without, %d distinct depths, %d sharing one, %d close, %d visited"
          % (seed, len(z), with_depth, without, len(vals), shared, close, len(order)))
    assert with_depth >= 600 and without >= 100 and shared >= 50 and close > 100
    assert len(order) == RM.nvisit_closed_form(with_depth, close, 100) == close + 1
    assert (S["uRight"][z > 0] < S["keys_un"]["x"][z > 0]).all() and (S["uRight"][z <= 0] == -1).all()
