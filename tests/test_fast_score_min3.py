"""fast_score_S (csrc/orb_fast_score.h) regrouped over a three-input minimum / maximum: 8 + 8 minima, 8 maxima, 8 min3, 3 max3 and
one maximum (36 packed operations), every value carried with a bias of 2048 that comes off at the end.  The header is compiled for the
host into the stand-alone program of test_fast_score_network.py (there the three-input primitive is the integer one; the device's is
the packed f16 form, which tests/test_gpu_fast_score_min3.py runs) and compared with the definition, arc by arc: rings at the ends
of the value range, where the biased halves reach 2048 - 255 and 2048 + 255, staircases at every rotation, whose arcs' minima all
differ so that each of the eight min3 and each input of the max3 tree decides the score in turn, and 10^6 random rings."""
import numpy as np
import pytest

from test_fast_score_network import build_program, definition, run_program


def extreme_flat_rings():
    """All-0 and all-255 rings at centres 0 and 255: margins 0, +255 (all of the ring brighter) and -255 in every half."""
    return np.array([[c] + [v] * 16 for c in (0, 255) for v in (0, 255)], np.uint8)


def staircase_rings():
    """ring[k] = lo + step * ((k + rot) % 16) for every rotation, ascending and descending, at steps that keep the ring inside
    [0, 255], with the centre below, inside and above the staircase."""
    rings = []
    for step in (1, 2, 7, 16, 17):
        span = 15 * step
        for lo in sorted({0, (255 - span) // 2, 255 - span}):
            for rot in range(16):
                for sgn in (1, -1):
                    ring = [lo + step * ((sgn * k + rot) % 16) for k in range(16)]
                    for centre in sorted({0, lo, lo + span // 2, lo + span, 255}):
                        rings.append([centre] + ring)
    return np.array(rings, np.uint8)


def random_rings():
    rng = np.random.default_rng(20261019)
    return rng.integers(0, 256, (1000000, 17), dtype=np.uint8)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("fast_score_min3")
    return build_program(d, "fast_score", ["-O2"]), d


@pytest.mark.parametrize("family", [extreme_flat_rings, staircase_rings, random_rings])
def test_min3_network_equals_definition(program, family):
    exe, d = program
    rings = family()
    ref = definition(rings)
    S = run_program(exe, d, rings)
    bad = np.flatnonzero(S != ref)
    assert len(bad) == 0, (len(bad), rings[bad[:4]], S[bad[:4]], ref[bad[:4]])


def test_families_reach_what_they_claim():
    ref = definition(extreme_flat_rings())
    assert ref.tolist() == [0, 255, 255, 0]          # (centre 0, ring 255) and (centre 255, ring 0): the +-255 extremes
    st = definition(staircase_rings())
    assert st.min() == 0 and st.max() > 200 and len(np.unique(st)) > 10
    assert (definition(random_rings()[:100000]) > 0).sum() > 1000
