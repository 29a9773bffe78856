"""CPU: orbm_rig_concat_batch_device and orbm_search_by_projection_last_frame_fisheye_batch_device exist on both sides of the ABI,
their refusals that need no device, and the conditions the scenes of tests/rig_model.py must meet for the comparisons of
tests/test_gpu_rig_batch.py to mean something - judged by the oracle alone.  The refusals next to live buffers are in
tests/test_gpu_rig_batch.py::test_refusals_with_live_buffers."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import rig_model as RM
import test_abi_null
from conftest import ROOT

SEARCH = "orbm_search_by_projection_last_frame_fisheye_batch_device"
CONCAT = "orbm_rig_concat_batch_device"


def test_symbols_and_mirrors(pkg):
    L = pkg.load()
    for name, nargs in ((SEARCH, 27), (CONCAT, 12)):
        assert name in pkg.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    sig = inspect.signature(pkg.rig_concat_batch_device)
    assert list(sig.parameters) == ["nframes", "d_keysL", "d_descL", "d_countsL", "d_keysR", "d_descR", "d_countsR", "cap", "d_keys", "d_desc", "d_n", "stream"]
    assert sig.parameters["stream"].default is None
    sig = inspect.signature(pkg.ORBmatcher.search_by_projection_last_frame_fisheye_batch_device)
    assert list(sig.parameters) == ["self", "cur0", "frame_stride", "d_frame_n", "frame_n_stride", "d_n_left", "n_left_stride", "last0", "last_stride", "d_last_n",
                                    "last_n_stride", "npairs", "scale_factors", "Trl", "cam_type", "cam_params", "th", "d_slot", "d_slot_obs",
                                    "d_match_of_query", "d_nmatches", "n_left", "bMono", "mb", "stream"]
    assert sig.parameters["n_left"].default == 0 and sig.parameters["bMono"].default is False and sig.parameters["stream"].default is None
    assert pkg.FISHEYE_MAX_KEYPOINTS == 12960
    with open(os.path.join(ROOT, "include", "orbhip.h")) as f:
        header = f.read()
    assert "#define ORBM_FISHEYE_MAX_KEYPOINTS 12960" in header and ("int %s(" % SEARCH) in header and ("int %s(" % CONCAT) in header


def test_null_sweep_survives_the_new_symbols():
    """tests/test_abi_null.py calls every entry of ABI_SYMBOLS with zeros and NULLs; both new symbols are in that list (above)."""
    test_abi_null.test_null_arguments_do_not_crash()


def test_concat_refusals_without_device(pkg):
    n, cap = 2, 8
    keep = dict(k=np.zeros((n, cap), pkg.KP_DTYPE), d=np.zeros((n, cap, 32), np.uint8), c=np.zeros((n, 2), np.int32),
                ok=np.zeros((n, 2 * cap), pkg.KP_DTYPE), od=np.zeros((n, 2 * cap, 32), np.uint8), on=np.zeros((n, 2), np.int32))
    p = {k: v.ctypes.data for k, v in keep.items()}
    good = dict(nframes=n, d_keysL=p["k"], d_descL=p["d"], d_countsL=p["c"], d_keysR=p["k"], d_descR=p["d"], d_countsR=p["c"], cap=cap, d_keys=p["ok"],
                d_desc=p["od"], d_n=p["on"])
    bad = [dict(d_keysL=0), dict(d_descL=0), dict(d_countsL=0), dict(d_keysR=0), dict(d_descR=0), dict(d_countsR=0), dict(d_keys=0), dict(d_desc=0), dict(d_n=0),
           dict(nframes=-1), dict(cap=0), dict(cap=-4), dict(cap=pkg.FISHEYE_MAX_KEYPOINTS // 2 + 1)]
    for c in bad:
        with pytest.raises(ValueError):
            pkg.rig_concat_batch_device(**dict(good, **c))
    assert pkg.rig_concat_batch_device(**dict(good, nframes=0)) == 0          # nothing to do, nothing launched
    assert pkg.rig_concat_batch_device(**dict(good, nframes=0, cap=pkg.FISHEYE_MAX_KEYPOINTS // 2)) == 0


def _search_args(pkg):
    n, nl = 6, 4
    A = dict(keys=np.zeros(n, pkg.KP_DTYPE), desc=np.zeros((n, 32), np.uint8), has=np.ones(nl, np.uint8), Xw=np.zeros((nl, 3), np.float32),
             md=np.zeros((nl, 32), np.uint8), lk=np.zeros(nl, pkg.KP_DTYPE), T=np.eye(4, dtype=np.float32), slot=np.full(n, -1, np.int32),
             sobs=np.zeros(n, np.uint8), nm=np.zeros(1, np.int32))
    p = lambda a: a.ctypes.data
    fs = pkg.FrameStruct(n, p(A["keys"]), p(A["desc"]), None, 0.0, 600.0, 0.0, 400.0)
    ls = pkg.LastFrameStruct(nl, p(A["has"]), p(A["Xw"]), p(A["md"]), p(A["lk"]), None, p(A["T"]), p(A["T"]))
    good = dict(cur0=fs, frame_stride=n, d_frame_n=None, frame_n_stride=0, d_n_left=None, n_left_stride=0, last0=ls, last_stride=nl, d_last_n=None,
                last_n_stride=0, npairs=1, scale_factors=np.ones(8, np.float32), Trl=np.eye(4, dtype=np.float32), cam_type=0,
                cam_params=np.array([400, 400, 300, 200], np.float32), th=7.0, d_slot=p(A["slot"]), d_slot_obs=p(A["sobs"]), d_match_of_query=None,
                d_nmatches=p(A["nm"]), n_left=3)
    return A, good


def test_search_refusals_without_device(pkg):
    """The mirror refuses what needs no device before it calls the library; a matcher without a handle stands in for one (no GPU
    here), so a call that passes the mirror's checks reaches the library's own first refusal, the NULL handle."""
    L = pkg.load()
    m = pkg.ORBmatcher.__new__(pkg.ORBmatcher)
    m.L, m.m, m.mfNNratio, m.mbCheckOrientation = L, None, 0.9, True
    A, good = _search_args(pkg)
    bad = [(dict(Trl=None), "Trl is missing"), (dict(Trl=np.eye(3, dtype=np.float32)), "12 or 16"), (dict(npairs=-1), "npairs"), (dict(d_slot=None), "missing output"),
           (dict(d_slot_obs=None), "missing output"), (dict(d_nmatches=None), "missing output"), (dict(scale_factors=np.ones(17, np.float32)), "nlevels"),
           (dict(scale_factors=np.ones(0, np.float32)), "nlevels"), (dict(cam_type=2), "camera"), (dict(cam_type=1), "camera"),   # KannalaBrandt8 needs 8 parameters
           (dict(n_left=-1), "n_left"), (dict(n_left=7), "n_left"), (dict(frame_stride=pkg.FISHEYE_MAX_KEYPOINTS + 1), "frame_stride")]
    for c, what in bad:
        with pytest.raises(ValueError, match=what):
            m.search_by_projection_last_frame_fisheye_batch_device(**dict(good, **c))
    with pytest.raises(ValueError, match="null handle"):
        m.search_by_projection_last_frame_fisheye_batch_device(**good)
    with pytest.raises(ValueError, match="null handle"):
        m.search_by_projection_last_frame_fisheye_batch_device(**dict(good, Trl=np.eye(4, dtype=np.float32)[:3], n_left=0))
    # the library itself: a NULL handle is ORBX_E_ARG before anything is staged or launched, for npairs = 0 as well
    p = lambda a: a.ctypes.data
    for npairs in (1, 0):
        rc = L.orbm_search_by_projection_last_frame_fisheye_batch_device(None, C.byref(good["cur0"]), 6, None, 0, None, 0, 3, C.byref(good["last0"]), 4, None, 0, npairs,
                                                                         p(good["scale_factors"]), 8, p(good["Trl"]), 0, p(good["cam_params"]), C.c_float(0.0),
                                                                         C.c_float(7.0), 0, 1, good["d_slot"], good["d_slot_obs"], None, good["d_nmatches"], None)
        assert rc == pkg.E_ARG
    m.m = None


@pytest.mark.parametrize("cam", [0, 1])
def test_scene_conditions(oracle, synth, cam):
    """Every problem the GPU tests compare: the projection of a map point lands within 2 px of its keypoint in the left image
    under the camera model of the problem, and the oracle's result has at least 50 surviving matches in each image and at least
    one match undone by the rotation histogram."""
    P = RM.problems(oracle, synth, cam)
    assert sorted(q["tz"] for q in P) == sorted(RM.TZ) and {0.3, -0.3, 0.0} <= set(RM.TZ) and RM.MB == 0.11
    for p, q in enumerate(P):
        front = np.nonzero(~q["behind"])[0]
        Xc = q["Xw"][front].astype(np.float64) + q["Tcw"][:3, 3].astype(np.float64)
        uv = np.array([oracle.project(cam, RM.CAMS[cam], *[float(np.float32(c)) for c in x]) for x in Xc[::7]])
        err = np.hypot(uv[:, 0] - q["u"][front][::7], uv[:, 1] - q["v"][front][::7])
        assert err.max() < 2.0, (cam, p, float(err.max()))
        frac = (np.mean(q["has_mp"] == 0), np.mean(q["obs"] == 0), np.mean(q["behind"]))
        assert 0.15 < frac[0] < 0.25 and 0.06 < frac[1] < 0.14 and 0.01 < frac[2] < 0.06 and len(q["pre"]) == 60 and 0 < q["pre_obs"].sum() < 60
        for th in RM.THS:
            for mono in ((False, True) if p == 0 else (False,)):
                s0, _ = RM.initial_slots(q)
                n, slot, sobs = RM.oracle_search(oracle, q, th, mono=mono)
                n_unpruned, _, _ = RM.oracle_search(oracle, q, th, mono=mono, check_ori=False)
                new = (slot != s0) & (slot >= 0)
                nl = len(q["kl"])
                left, right = int(new[:nl].sum()), int(new[nl:].sum())
                print("cam %d problem %d th %g mono %d: N %d Nleft %d nLast %d, %d matches, %d left, %d right, %d pruned, projection error %.3f px"
                      % (cam, p, th, mono, len(slot), nl, len(q["k0"]), n, left, right, n_unpruned - n, err.max()))
                assert left >= 50 and right >= 50 and n_unpruned - n >= 1


@pytest.mark.parametrize("cam", [0, 1])
def test_chain_scene_conditions(oracle, synth, cam):
    """The two rig frames of test_chain_from_extraction, here with the oracle's own extraction of the images and lapping areas:
    the same three conditions, and the frames differ in Nleft."""
    P = RM.chain_problems(oracle, synth, cam)
    assert len(set(len(q["kl"]) for q in P)) == len(P) == 2
    for f, q in enumerate(P):
        Xc = q["Xw"].astype(np.float64) + q["Tcw"][:3, 3].astype(np.float64)
        uv = np.array([oracle.project(cam, RM.CAMS[cam], *[float(np.float32(c)) for c in x]) for x in Xc[::7]])
        err = np.hypot(uv[:, 0] - q["u"][::7], uv[:, 1] - q["v"][::7])
        n, left, right, pruned = RM.scene_counts(oracle, q, RM.CHAIN_TH)
        print("cam %d chain frame %d: Nleft %d Nright %d, %d matches, %d left, %d right, %d pruned, projection error %.3f px"
              % (cam, f, len(q["kl"]), len(q["kr"]), n, left, right, pruned, err.max()))
        assert err.max() < 2.0 and left >= 50 and right >= 50 and pruned >= 1
