"""CPU: the device evaluation entries of the scalar replicas (orbx_cosf_device, orbx_sinf_device, orbx_atanf_device, orbx_atan2f_device,
orbx_fast_atan2_device) exist on both sides of the ABI with the contract of orbx_logf_device, and refuse what needs no device.  What
they compute is in tests/test_gpu_libm_device.py; the all-NULL call of each is made by tests/test_abi_null.py, which walks pkg.ABI_SYMBOLS."""
import os
import re

import numpy as np

from conftest import ROOT

UNARY = ("orbx_cosf_device", "orbx_sinf_device", "orbx_atanf_device")
BINARY = ("orbx_atan2f_device", "orbx_fast_atan2_device")


def test_symbols_and_header(pkg):
    L = pkg.load()
    with open(os.path.join(ROOT, "include", "orbhip.h")) as f:
        header = f.read()
    for names, nargs, decl in ((UNARY, 4, "int %s(const float *d_x, int n, float *d_y, void *stream);"),
                               (BINARY, 5, "int %s(const float *d_yin, const float *d_xin, int n, float *d_out, void *stream);")):
        for name in names:
            assert name in pkg.ABI_SYMBOLS and hasattr(L, name)
            fn = getattr(L, name)
            assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
            assert (decl % name) in header
            params = re.search(r"\b%s\(([^)]*)\)" % name, header).group(1)
            assert len(params.split(",")) == nargs, name


def test_refusals_without_device(pkg):
    """n < 0 and a NULL pointer with n > 0 are ORBX_E_ARG, n == 0 is 0 with no launch: all decided before any device work.  The
    pointers that are not NULL here are never read: no call below has n > 0 and all of its pointers."""
    L = pkg.load()
    p = np.zeros(4, np.float32).ctypes.data
    for name in UNARY:
        fn = getattr(L, name)
        for args in ((None, 1, None, None), (p, 1, None, None), (None, 1, p, None), (p, -1, p, None), (None, -1, None, None)):
            assert fn(*args) == pkg.E_ARG, (name, args)
        assert fn(None, 0, None, None) == 0 and fn(p, 0, p, None) == 0
    for name in BINARY:
        fn = getattr(L, name)
        for args in ((None, None, 1, None, None), (None, p, 1, p, None), (p, None, 1, p, None), (p, p, 1, None, None), (p, p, -1, p, None),
                     (None, None, -1, None, None)):
            assert fn(*args) == pkg.E_ARG, (name, args)
        assert fn(None, None, 0, None, None) == 0 and fn(p, p, 0, p, None) == 0
