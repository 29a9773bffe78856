"""The DEVICE builds of the scalar functions the kernels restate by hand - cosf / sinf (csrc/orb_sincos.h), atanf / atan2f
(csrc/orb_atan2f.h) and the kernels' cv::fastAtan2 (fast_atan2_deg of csrc/orb_kernels.h) - evaluated densely through
orbx_cosf_device .. orbx_fast_atan2_device on the input sets of tests/libm_device_cases.py: one upload, one call, one synchronisation
per function.  Bit for bit, the sign of zero included; a NaN only has to be a NaN (the device's and x86's default NaNs differ in sign):
  against orbx_ref_*, the host build of the same source - the contract the headers state;
  against this host's glibc (orc_libm_*) - the contract the product needs;
  fast_atan2_deg, which has no host build, against the oracle's restatement orc_fast_atan2, which
  tests/test_libm_device_cases.py holds to OpenCV's accuracy statement.
tests/test_libm_device_cases.py checks on the CPU what the sets hold and that the host build equals glibc on them."""
import ctypes as C

import numpy as np
import pytest

import libm_device_cases as D

pytestmark = pytest.mark.gpu
f32 = np.float32
SENT = f32(-777.25)                                          # no function here returns it: every result is in [-pi, 360] or a NaN
ENTRIES = ("cosf", "sinf", "atanf", "atan2f", "fast_atan2")


def device(pkg, name, inputs, pad=0, stream=None):
    """orbx_<name>_device on the float32 arrays `inputs`, in an output buffer of len + pad elements preset to SENT; the whole buffer."""
    import torch
    n = len(inputs[0])
    d_in = [torch.from_numpy(np.array(a, f32)).cuda() for a in inputs]       # the sets are read-only: a copy
    d_out = torch.full((n + pad,), float(SENT), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    args = [C.c_void_p(t.data_ptr()) for t in d_in] + [n, C.c_void_p(d_out.data_ptr()), None if stream is None else C.c_void_p(stream.cuda_stream)]
    assert getattr(pkg.load(), "orbx_%s_device" % name)(*args) == 0
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    return d_out.cpu().numpy()


def references(pkg, oracle, name, inputs):
    """[(what, expected)]: what the device build of `name` has to equal on `inputs`."""
    L, O = pkg.load(), oracle.lib()
    if name == "fast_atan2":
        return [("the oracle's orc_fast_atan2", oracle.apply_binary(O.orc_fast_atan2, *inputs))]
    apply = oracle.apply_unary if len(inputs) == 1 else oracle.apply_binary
    return [("the host build orbx_ref_" + name, apply(getattr(L, "orbx_ref_" + name), *inputs)), ("glibc " + name, apply(getattr(O, "orc_libm_" + name), *inputs))]


def check(pkg, oracle, name, inputs, got):
    assert len(got) == len(inputs[0]) and not np.any(got == SENT), "%s: %d of %d outputs were never written" % (name, np.count_nonzero(got == SENT), len(got))
    msgs = [D.mismatch(name, inputs, got, want, ("device", what)) for what, want in references(pkg, oracle, name, inputs)]
    assert not any(msgs), "\n".join(m for m in msgs if m)


def test_cosf_device_equals_host_and_glibc(pkg, oracle):
    x = D.sincos()
    check(pkg, oracle, "cosf", (x,), device(pkg, "cosf", (x,)))


def test_sinf_device_equals_host_and_glibc(pkg, oracle):
    x = D.sincos()
    check(pkg, oracle, "sinf", (x,), device(pkg, "sinf", (x,)))


def test_atanf_device_equals_host_and_glibc(pkg, oracle):
    x = D.atanf()
    check(pkg, oracle, "atanf", (x,), device(pkg, "atanf", (x,)))


def test_atan2f_device_equals_host_and_glibc(pkg, oracle):
    yx = D.atan2f()
    check(pkg, oracle, "atan2f", yx, device(pkg, "atan2f", yx))


def test_fast_atan2_device_equals_oracle(pkg, oracle):
    yx = D.fast_atan2()
    check(pkg, oracle, "fast_atan2", yx, device(pkg, "fast_atan2", yx))


def small(name, n):
    """n inputs of the set of `name`: its head (the special values and the smallest pairs come first) and a strided pick of the rest."""
    s = {"cosf": D.sincos, "sinf": D.sincos, "atanf": D.atanf, "atan2f": D.atan2f, "fast_atan2": D.fast_atan2}[name]()
    s = s if isinstance(s, tuple) else (s,)
    idx = np.concatenate([np.arange(n // 2), np.arange(n // 2, len(s[0]), (len(s[0]) - n // 2) // (n - n // 2))[:n - n // 2]])
    assert len(idx) == n
    return tuple(a[idx] for a in s)


@pytest.mark.parametrize("name", ENTRIES)
def test_length_off_the_block_size_leaves_the_padding(pkg, oracle, name):
    """1001 elements = three blocks of 256 and 233 lanes of a fourth: the 23 idle lanes and the block that would follow write nothing."""
    inputs = small(name, 1001)
    out = device(pkg, name, inputs, pad=600)
    assert np.all(out[1001:] == SENT), "%s wrote past n: %d of 600 padding elements changed" % (name, np.count_nonzero(out[1001:] != SENT))
    check(pkg, oracle, name, inputs, out[:1001])


@pytest.mark.parametrize("name", ENTRIES)
def test_on_a_stream_of_its_own(pkg, oracle, name):
    import torch
    inputs = small(name, 70_001)
    stream = torch.cuda.Stream()
    check(pkg, oracle, name, inputs, device(pkg, name, inputs, stream=stream))
