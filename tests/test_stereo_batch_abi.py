"""CPU: orbx_compute_stereo_matches_batch_device exists on both sides of the ABI, and its refusals that need no device: a NULL
handle, and a NULL required pointer with NULL handles, give ORBX_E_ARG before anything is launched.  The refusals that need live
handles (mismatched extractors, nframes, mb, cap) are in tests/test_gpu_stereo_batch.py::test_refusals_with_live_handles."""
import ctypes as C
import inspect

import numpy as np


def test_symbol_and_method(pkg):
    L = pkg.load()
    assert "orbx_compute_stereo_matches_batch_device" in pkg.ABI_SYMBOLS
    fn = L.orbx_compute_stereo_matches_batch_device
    assert fn.argtypes is not None and len(fn.argtypes) == 16
    sig = inspect.signature(pkg.ORBextractor.compute_stereo_matches_batch_device)
    assert list(sig.parameters)[1:] == ["right", "nframes", "d_keysL", "d_descL", "d_countsL", "d_keysR", "d_descR", "d_countsR", "cap", "mb",
                                        "mbf", "d_uRight", "d_depth", "d_nstereo", "stream"]
    assert sig.parameters["d_nstereo"].default is None and sig.parameters["stream"].default is None


def test_null_handle_and_null_pointers(pkg):
    L = pkg.load()
    n, cap = 1, 8
    keys = np.zeros((n, cap), pkg.KP_DTYPE)
    desc = np.zeros((n, cap, 32), np.uint8)
    cnt = np.zeros((n, 2), np.int32)
    out = np.zeros((2, n, cap), np.float32)
    p = lambda a: a.ctypes.data
    good = [p(keys), p(desc), p(cnt), p(keys), p(desc), p(cnt), cap, C.c_float(0.11), C.c_float(47.9), p(out[0]), p(out[1]), None, None]
    call = lambda hl, hr, rest: L.orbx_compute_stereo_matches_batch_device(hl, hr, n, *rest)
    assert call(None, None, good) == pkg.E_ARG
    for k in (0, 1, 2, 3, 4, 5, 9, 10):          # every required pointer in turn
        bad = list(good)
        bad[k] = None
        assert call(None, None, bad) == pkg.E_ARG
