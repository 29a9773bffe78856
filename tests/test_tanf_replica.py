"""CPU: the tanf replica of KannalaBrandt8::unproject (csrc/orb_tanf.h, evaluated here on the HOST from the same source through
orbx_ref_tanf) equals this host's glibc tanf bit for bit.  libm's tanf is called through ctypes.  Covered: the special values, a
strided sample of [-2, 2] (the unprojection's theta starts in [0, pi/2] and moves by Newton steps), +-4096 ulps around every
breakpoint of the replica: the direct / reduced switch at pi/4, the quadrant changes of the double reduction (odd multiples of
pi/4), the kernel's |x| >= 0.6744 and |x| < 2^-13 branches on a direct and on a reduced argument, pi/2 itself, and the switch of
the reduction at 120; and a strided sample of [120, FLT_MAX], where a diverged Newton iteration of a strongly distorted camera ends
(tests/test_ref_cameras.py) and the reduction is the integer one.

While authoring, every float of [0, pi/2] (1 070 141 404 values) and of [-119.99, 119.99] (2 246 047 172 values) was compared on
glibc 2.35: 0 mismatches; so was every float of [119.9, 256] and every 37th bit pattern from there to FLT_MAX, both signs
(73 486 962 values).  glibc 2.41 and later round tanf correctly and differ from the replica in the last bit for some arguments;
on such a host these tests fail, which is the statement that the reference's libm is not pinned."""
import ctypes as C

import numpy as np

libm = C.CDLL("libm.so.6")
libm.tanf.restype = C.c_float
libm.tanf.argtypes = [C.c_float]


def _bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def _compare(pkg, patterns):
    """Both functions on the float32 bit patterns; NaN results compare as NaN (the payload of an invalid operation is the host's)."""
    x = np.asarray(patterns, np.uint32).view(np.float32)
    f = pkg.load().orbx_ref_tanf
    a = np.array(list(map(libm.tanf, x.tolist())), np.float32).view(np.uint32)
    b = np.array(list(map(f, x.tolist())), np.float32).view(np.uint32)
    nan = lambda u: (u & 0x7fffffff) > 0x7f800000
    bad = np.flatnonzero((a != b) & ~(nan(a) & nan(b)))
    assert len(bad) == 0, "%d mismatches, first at x = %r (%08x): libm %08x, replica %08x" % (
        len(bad), float(x[bad[0]]), int(x.view(np.uint32)[bad[0]]), int(a[bad[0]]), int(b[bad[0]]))


def test_special_values(pkg):
    vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 2.0 ** -13, 2.0 ** -14,
                     0.5, 1.0, -1.0, 2.0, -2.0, np.pi / 4, np.pi / 2, -np.pi / 2, 3 * np.pi / 4, np.pi, 100.0, 119.99999,
                     120.0, -120.0, 131.875137, -811.621765, 1e6, -1e6, 1e20, 3.4028235e38, -3.4028235e38], np.float32)
    _compare(pkg, vals.view(np.uint32))
    f = pkg.load().orbx_ref_tanf
    for v in (120.0, -120.0, 1e6, 3.4028235e38):          # finite beyond 120: a number, as in libm
        assert np.isfinite(f(v)), v


def test_strided_minus_two_to_two(pkg):
    top = _bits(2.0)
    pos = np.arange(0, top + 1, 4999, dtype=np.uint32)    # a stride prime to the mantissa: about 215 000 values per sign
    _compare(pkg, pos)
    _compare(pkg, pos | np.uint32(0x80000000))


def test_around_breakpoints(pkg):
    hpi = np.pi / 2
    points = [np.pi / 4, 3 * np.pi / 4, 5 * np.pi / 4, 7 * np.pi / 4, hpi, 2 * hpi, 0.6744, hpi - 0.6744, hpi + 0.6744, 2.0 ** -13,
              hpi - 2.0 ** -13, hpi + 2.0 ** -13, np.pi / 4 - 2.0 ** -13, 2.0, 120.0]
    centres = [_bits(p) for p in points] + [0x3f490fda, 0x3f2ca140, 0x39000000]
    for c in centres:
        pat = np.arange(c - 4096, c + 4097, dtype=np.uint32)   # at 120 the reduction changes from the double one to the integer one
        _compare(pkg, pat)
        _compare(pkg, pat | np.uint32(0x80000000))


def test_strided_beyond_120(pkg):
    """The integer reduction: every exponent from 2^6 to 2^127 (the word of 2/pi and the shift both depend on it)."""
    pos = np.arange(_bits(120.0), 0x7f800000, 9973, dtype=np.uint32)     # about 105 000 values per sign
    _compare(pkg, pos)
    _compare(pkg, pos | np.uint32(0x80000000))
