"""CPU: the refusals of orbm_search_local_points / orbm_search_local_points_batch_device that need no device: a NULL handle gives
ORBX_E_ARG before anything is staged or launched.  The refusals that need a live handle (NULL fields, nlevels, cam_type, frame size,
map stride) are in tests/test_gpu_local_points.py::test_refusals_with_a_handle."""
import ctypes as C

import numpy as np


def _args(pkg):
    n, nmp = 4, 3
    keys = np.zeros(n, pkg.KP_DTYPE)
    desc = np.zeros((n, 32), np.uint8)
    A = dict(elig=np.ones(nmp, np.uint8), Xw=np.zeros((nmp, 3), np.float32), normal=np.zeros((nmp, 3), np.float32),
             maxd=np.ones(nmp, np.float32), mind=np.ones(nmp, np.float32), mpdesc=np.zeros((nmp, 32), np.uint8), Tcw=np.eye(4, dtype=np.float32),
             sf=np.ones(8, np.float32), cam=np.array([400, 400, 300, 200], np.float32), slot=np.full(n, -1, np.int32), sobs=np.zeros(n, np.uint8),
             moq=np.zeros(nmp, np.int32), inv=np.zeros(nmp, np.uint8), f=np.zeros((6, nmp), np.float32), lvl=np.zeros(nmp, np.int32), nm=np.zeros(1, np.int32))
    p = lambda a: a.ctypes.data
    fs = pkg.FrameStruct(n, p(keys), p(desc), None, 0.0, 600.0, 0.0, 400.0)
    ms = pkg.LocalMapStruct(nmp, p(A["elig"]), p(A["Xw"]), p(A["normal"]), p(A["maxd"]), p(A["mind"]), p(A["mpdesc"]), None, p(A["Tcw"]))
    ts = pkg.TrackStruct(p(A["inv"]), p(A["f"][0]), p(A["f"][1]), p(A["f"][2]), p(A["f"][3]), p(A["f"][4]), p(A["lvl"]))
    return A, keys, desc, fs, ms, ts


def test_null_handle(pkg):
    L = pkg.load()
    A, keys, desc, fs, ms, ts = _args(pkg)
    p = lambda a: a.ctypes.data
    host = lambda m, fs_, sf, ms_, cam, slot, sobs, ts_, nlevels=8, cam_type=0: L.orbm_search_local_points(
        m, fs_, sf, nlevels, C.c_float(0.18), ms_, cam_type, cam, C.c_float(0.0), C.c_float(0.5), C.c_float(1.0), 0, C.c_float(0.0),
        C.c_float(0.8), slot, sobs, p(A["moq"]), ts_)
    good = (C.byref(fs), p(A["sf"]), C.byref(ms), p(A["cam"]), p(A["slot"]), p(A["sobs"]), C.byref(ts))
    assert host(None, *good) == pkg.E_ARG
    dev = lambda m, fs_, ms_, ts_, sf, cam, slot, sobs, nm: L.orbm_search_local_points_batch_device(
        m, fs_, 4, None, 0, ms_, 3, None, 0, 1, sf, 8, C.c_float(0.18), 0, cam, C.c_float(0.0), C.c_float(0.5), C.c_float(1.0), 0,
        C.c_float(0.0), C.c_float(0.8), slot, sobs, None, ts_, nm, None)
    assert dev(None, C.byref(fs), C.byref(ms), C.byref(ts), p(A["sf"]), p(A["cam"]), p(A["slot"]), p(A["sobs"]), p(A["nm"])) == pkg.E_ARG
