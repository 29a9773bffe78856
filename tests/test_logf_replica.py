"""CPU: the logf replica compiled into k_local_map_project (csrc/orb_logf.h, evaluated here on the HOST from the same source through
orbx_ref_logf) equals this host's glibc logf bit for bit: the special values, a strided sample of every positive float, and
+-4096 ulps around scaleFactor^k (the level boundaries of MapPoint::PredictScale, MapPoint.cc:587-602).  The sweeps run in a small C
helper compiled here with the host compiler (a function pointer to the product's host evaluation); ORB_EXHAUSTIVE=1 sweeps every
float."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

EXH = os.environ.get("ORB_EXHAUSTIVE") == "1"

HELPER = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>
typedef float (*fn_t)(float);
/* bit patterns lo..hi (inclusive) with `step`: mismatches against libm's logf; first mismatching pattern in *first */
long sweep(fn_t f, uint32_t lo, uint32_t hi, uint32_t step, uint32_t *first) {
  long bad = 0;
  for (uint64_t u = lo; u <= hi; u += step) {
    const uint32_t b = (uint32_t)u;
    float x, a, r;
    memcpy(&x, &b, 4);
    a = logf(x);
    r = f(x);
    if (memcmp(&a, &r, 4) != 0) { if (!bad) *first = b; bad++; }
  }
  return bad;
}
"""


@pytest.fixture(scope="module")
def helper(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no host C compiler")
    d = tmp_path_factory.mktemp("logf")
    src, so = d / "sweep.c", d / "sweep.so"
    src.write_text(HELPER)
    subprocess.check_call([cc, "-O2", "-shared", "-fPIC", "-o", str(so), str(src), "-lm"])
    L = C.CDLL(str(so))
    L.sweep.restype = C.c_long
    L.sweep.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    return L


def _bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _run(helper, pkg, lo, hi, step):
    fn = C.cast(pkg.load().orbx_ref_logf, C.c_void_p)
    first = C.c_uint32(0)
    bad = helper.sweep(fn, lo, hi, step, C.byref(first))
    assert bad == 0, "%d mismatches in [%08x, %08x] step %d, first at %08x" % (bad, lo, hi, step, first.value)


def test_special_values(pkg):
    L = pkg.load()
    libm = C.CDLL("libm.so.6")
    libm.logf.restype = C.c_float
    libm.logf.argtypes = [C.c_float]
    vals = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 3.4028235e38, 2.0, 0.5,
            -1e-40, -3.0, 1.2, 1.0000001, 0.99999994]
    for v in vals:
        a = np.float32(libm.logf(v)).view(np.uint32)
        b = np.float32(L.orbx_ref_logf(v)).view(np.uint32)
        assert a == b, (v, hex(a), hex(b))


def test_strided_positive_floats(pkg, helper):
    # every positive float (subnormals, normals, inf, the NaN range) in a stride prime to the mantissa; negatives by a coarser stride
    _run(helper, pkg, 0, 0x7fffffff, 1 if EXH else 997)
    _run(helper, pkg, 0x80000000, 0xffffffff, 1 if EXH else 100003)


@pytest.mark.parametrize("sf", [1.2, 1.5, 2.0])
def test_predict_scale_boundaries(pkg, helper, sf):
    for k in range(16):
        for b in (_bits(np.float32(sf ** k)), _bits(np.float32(sf) ** np.float32(k)), _bits(np.float32(1.0 / sf ** k))):
            _run(helper, pkg, b - 4096, b + 4096, 1)
