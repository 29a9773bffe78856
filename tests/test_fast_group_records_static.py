"""k_fast's memory round trips, read off the compiled device code (no GPU): the group record is fetched by scalar loads in front of
the tile DMA, and nothing is loaded from memory between the workgroup barrier and the detection loop."""
import re

import pytest

from device_code import device_asm

LOAD = re.compile(r"^\s*(global_load|flat_load|buffer_load|scratch_load|s_load|s_buffer_load)\w*\s")


@pytest.fixture(scope="module")
def k_fast_asm():
    lines = device_asm()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z6k_fast\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return [l.split(";")[0].rstrip() for l in lines[start + 1:end]]


def test_no_load_between_barrier_and_detection_loop(k_fast_asm):
    barriers = [i for i, l in enumerate(k_fast_asm) if re.match(r"^\s*s_barrier\b", l)]
    assert len(barriers) == 1, "k_fast has one workgroup barrier"
    first_read = next(i for i in range(barriers[0], len(k_fast_asm)) if re.match(r"^\s*ds_read_u8\b", k_fast_asm[i]))
    between = [l.strip() for l in k_fast_asm[barriers[0]:first_read] if LOAD.match(l)]
    assert not between, between


def test_one_record_round_trip_before_the_dma(k_fast_asm):
    """In front of the first LDS-DMA the scalar loads are kernel arguments (the base of the kernel's first load) or the record's: the
    latter share one base and are issued together, with no wait between them."""
    dma = next(i for i, l in enumerate(k_fast_asm) if re.match(r"^\s*global_load_lds_dwordx4\b", l))
    loads = [(i, re.match(r"^\s*s_load_dword\w*\s+\S+\s+(s\[\d+:\d+\])", l)) for i, l in enumerate(k_fast_asm[:dma]) if re.match(r"^\s*s_load", l)]
    assert loads and all(m for _, m in loads)
    kernarg = loads[0][1].group(1)
    rec = [(i, m.group(1)) for i, m in loads if m.group(1) != kernarg]
    assert 1 <= len(rec) <= 2 and len({b for _, b in rec}) == 1, rec
    assert not [l for l in k_fast_asm[rec[0][0]:rec[-1][0]] if re.match(r"^\s*s_waitcnt", l)]
