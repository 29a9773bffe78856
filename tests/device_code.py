"""The library's device code, compiled once per test session with the build's own flags (no GPU): the assembly, and per kernel the
static LDS the compiler's metadata states."""
import importlib
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import PKG

_asm = None


def device_asm():
    """Lines of the gfx950 assembly of orbhip.hip; skips the calling test where there is no hipcc."""
    global _asm
    if _asm is None:
        build = importlib.import_module(PKG + ".build")
        if not os.path.exists(build.HIPCC):
            pytest.skip("no hipcc")
        tmp = tempfile.mkdtemp(prefix="orbhip_asm_")
        try:
            out = os.path.join(tmp, "orbhip.s")
            flags = [f for f in build.FLAGS if f != "-shared"]
            subprocess.check_call([build.HIPCC] + flags + ["--offload-device-only", "-S", os.path.join(build.CSRC, "orbhip.hip"), "-o", out],
                                  stderr=subprocess.DEVNULL)
            with open(out) as f:
                _asm = f.read().splitlines()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return _asm


def static_lds():
    """{mangled kernel name: bytes of static LDS} from the amdhsa.kernels metadata (a kernel's keys come in alphabetical order)."""
    sizes, last = {}, None
    for line in device_asm():
        m = re.match(r"\s+(?:- )?\.group_segment_fixed_size:\s+(\d+)", line)
        if m:
            last = int(m.group(1))
        m = re.match(r"\s+(?:- )?\.name:\s+(\S+)", line)
        if m and last is not None:
            sizes[m.group(1)] = last
            last = None
    return sizes
