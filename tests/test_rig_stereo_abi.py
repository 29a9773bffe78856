"""CPU: the entry points of Frame::ComputeStereoFishEyeMatches exist on both sides of the ABI, and their refusals that need no
device.  The library's own refusals of the batch call next to a live handle are in tests/test_gpu_rig_stereo.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import rig_stereo_model as M
import test_abi_null
from conftest import ROOT

f32 = np.float32
BATCH = "orbm_stereo_fisheye_matches_batch_device"
HOST = "orbm_stereo_fisheye_matches"


def test_symbols_and_mirrors(pkg):
    L = pkg.load()
    for name, nargs in ((BATCH, 21), (HOST, 19), ("orbm_fisheye_triangulate", 10), ("orbm_fisheye_triangulate_device", 11), ("orbm_unproject", 4),
                        ("orbm_fisheye_ratio_test", 2), ("orbx_ref_tanf", 1), ("orbx_tanf_device", 4)):
        assert name in pkg.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    sig = inspect.signature(pkg.ORBmatcher.stereo_fisheye_matches_batch_device)
    assert list(sig.parameters) == ["self", "nframes", "d_keysL", "d_descL", "d_countsL", "d_keysR", "d_descR", "d_countsR", "cap", "level_sigma2", "Tlr",
                                    "cam_params", "cam_params2", "out_stride", "d_left_to_right", "d_right_to_left", "d_depth", "d_p3d", "d_nmatches", "stream"]
    assert sig.parameters["d_nmatches"].default is None and sig.parameters["stream"].default is None
    assert "monoL" in inspect.signature(pkg.ORBmatcher.ComputeStereoFishEyeMatches).parameters
    with open(os.path.join(ROOT, "include", "orbhip.h")) as f:
        header = f.read()
    for name in (BATCH, HOST, "orbm_fisheye_triangulate", "orbm_fisheye_triangulate_device", "orbm_unproject", "orbx_tanf_device"):
        assert ("int %s(" % name) in header
    assert "float orbx_ref_tanf(float x);" in header


def test_null_sweep_survives_the_new_symbols():
    test_abi_null.test_null_arguments_do_not_crash()


def test_refusals_without_device(pkg):
    """The mirror refuses what needs no device before it calls the library; a matcher without a handle stands in for one, so a call
    that passes the mirror's checks reaches the library's own first refusal, the NULL handle."""
    L = pkg.load()
    m = pkg.ORBmatcher.__new__(pkg.ORBmatcher)
    m.L, m.m = L, None
    buf = np.zeros(64, np.int32).ctypes.data
    good = dict(nframes=1, d_keysL=buf, d_descL=buf, d_countsL=buf, d_keysR=buf, d_descR=buf, d_countsR=buf, cap=4, level_sigma2=M.LEVEL_SIGMA2, Tlr=M.TLR,
                cam_params=M.CAM1, cam_params2=M.CAM2, out_stride=4, d_left_to_right=buf, d_right_to_left=buf, d_depth=buf, d_p3d=buf)
    bad = [(dict(d_keysL=None), "missing input"), (dict(d_descL=None), "missing input"), (dict(d_countsL=None), "missing input"),
           (dict(d_keysR=None), "missing input"), (dict(d_descR=None), "missing input"), (dict(d_countsR=None), "missing input"),
           (dict(d_left_to_right=None), "missing output"), (dict(d_right_to_left=None), "missing output"), (dict(d_depth=None), "missing output"),
           (dict(d_p3d=None), "missing output"), (dict(level_sigma2=None), "missing level_sigma2"), (dict(Tlr=None), "missing level_sigma2"),
           (dict(cam_params=None), "missing level_sigma2"), (dict(cam_params2=None), "missing level_sigma2"), (dict(Tlr=np.eye(3, dtype=f32)), "12 floats"),
           (dict(cam_params=M.CAM1[:4]), "12 floats"), (dict(nframes=-1), "nframes"), (dict(nframes=65536), "nframes"), (dict(cap=0), "cap"),
           (dict(cap=-3), "cap"), (dict(cap=pkg.FISHEYE_MAX_KEYPOINTS // 2 + 1, out_stride=pkg.FISHEYE_MAX_KEYPOINTS), "cap"), (dict(out_stride=3), "out_stride"),
           (dict(level_sigma2=np.ones(0, f32)), "nlevels"), (dict(level_sigma2=np.ones(17, f32)), "nlevels")]
    for c, what in bad:
        with pytest.raises(ValueError, match=what):
            m.stereo_fisheye_matches_batch_device(**dict(good, **c))
    with pytest.raises(ValueError, match="bad argument"):      # passes the mirror, refused by the library: no handle
        m.stereo_fisheye_matches_batch_device(**good)
    # the library itself, where no handle is involved
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    one, two, three = np.zeros(1, f32), np.zeros(2, f32), np.zeros(3, f32)
    T, c1, c2 = np.ascontiguousarray(M.TLR), M.CAM1.copy(), M.CAM2.copy()
    tri = lambda n=1, kp1=two, kp2=two, s1=one, s2=one, Tlr=T, a=c1, b=c2, d=one, x=three: L.orbm_fisheye_triangulate(
        n, *[None if v is None else p(v) for v in (kp1, kp2, s1, s2, Tlr, a, b, d, x)])
    assert tri() == 0
    for c in (dict(n=-1), dict(kp1=None), dict(kp2=None), dict(s1=None), dict(s2=None), dict(Tlr=None), dict(a=None), dict(b=None), dict(d=None), dict(x=None)):
        assert tri(**c) == pkg.E_ARG, c
    assert tri(n=0, kp1=None, kp2=None, s1=None, s2=None, d=None, x=None) == 0
    assert L.orbm_fisheye_triangulate_device(1, None, None, None, None, p(T), p(c1), p(c2), None, None, None) == pkg.E_ARG
    assert L.orbm_fisheye_triangulate_device(0, None, None, None, None, p(T), p(c1), p(c2), None, None, None) == 0
    assert L.orbm_unproject(None, 1, p(two), p(three)) == pkg.E_ARG and L.orbm_unproject(p(c1), -1, p(two), p(three)) == pkg.E_ARG
    assert L.orbm_unproject(p(c1), 1, None, p(three)) == pkg.E_ARG and L.orbm_unproject(p(c1), 0, None, None) == 0
    assert L.orbx_tanf_device(None, 1, None, None) == pkg.E_ARG and L.orbx_tanf_device(None, -1, None, None) == pkg.E_ARG
    assert L.orbx_tanf_device(None, 0, None, None) == 0
    # the per-frame form and the batch form without a handle
    assert L.orbm_stereo_fisheye_matches(None, *([None] * 2), 0, 0, *([None] * 2), 0, 0, p(M.LEVEL_SIGMA2), 8, p(T), p(c1), p(c2), *([None] * 5)) == pkg.E_ARG
