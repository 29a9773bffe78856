"""fast_score_S (csrc/orb_fast_score.h), the one host/device statement of k_fast's 16-pixel score, compiled for the host into a
stand-alone program and compared with the definition: the maximum over the 16 arcs of 9 contiguous circle pixels of the minimum
over the arc, for both polarities, clamped to [0, 255].  Every ring must agree.  The structured families are also checked against
the oracle's cornerScore (orc_fast_corner_score at threshold 0 returns S - 1).  The program is built a second time with
-fsanitize=address,undefined and run on the structured rings; it has its own main, so nothing is preloaded."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3_orb_slam3_selfnote_amd", "csrc")
# (dy, dx) of ring pixel k, the order of ORB_RING in orb_fast_score.h
CIRCLE = [(3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1),
          (-3, 0), (-3, -1), (-2, -2), (-1, -3), (0, -3), (1, -3), (2, -2), (3, -1)]

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "orb_fast_score.h"
// argv[1]: 32 bytes (dy, dx) of the 16 ring pixels as int8, then records of 17 bytes: centre, ring[0..15].  argv[2]: one byte S per record.
int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
  if (!f || !g) return 3;
  int8_t pos[32];
  if (fread(pos, 1, 32, f) != 32) return 4;
  uint8_t *patch = (uint8_t *)malloc(7 * FAST_TILE_PITCH);   // exactly the 7 rows the score may read
  uint8_t *ctr = patch + 3 * FAST_TILE_PITCH + 3;
  memset(patch, 0, 7 * FAST_TILE_PITCH);
  enum { CH = 65536 };
  uint8_t *rec = (uint8_t *)malloc(17 * CH), *out = (uint8_t *)malloc(CH);
  size_t n;
  while ((n = fread(rec, 17, CH, f)) > 0) {
    for (size_t i = 0; i < n; i++) {
      const uint8_t *r = rec + 17 * i;
      ctr[0] = r[0];
      for (int k = 0; k < 16; k++) ctr[pos[2 * k] * FAST_TILE_PITCH + pos[2 * k + 1]] = r[1 + k];
      const int S = fast_score_S(ctr);
      if (S < 0 || S > 255) return 5;
      out[i] = (uint8_t)S;
    }
    if (fwrite(out, 1, n, g) != n) return 6;
  }
  free(rec); free(out); free(patch);
  fclose(f);
  return fclose(g) ? 7 : 0;
}
"""


def definition(rings):
    """rings: (N, 17) uint8, centre then ring.  S by the definition, arc by arc."""
    out = np.empty(len(rings), np.int16)
    for a in range(0, len(rings), 1 << 18):
        r = rings[a:a + (1 << 18)].astype(np.int16)
        d = r[:, :1] - r[:, 1:]
        best = np.full(len(r), -255, np.int16)
        for pol in (d, -d):
            w = pol.copy()
            for j in range(1, 9):
                w = np.minimum(w, np.roll(pol, -j, axis=1))   # w[:, k] = min pol[k .. k+8]
            best = np.maximum(best, w.max(axis=1))
        out[a:a + len(r)] = np.clip(best, 0, 255)
    return out


def flat(centre):
    r = np.full(17, centre, np.uint8)
    return r


def structured_rings():
    rings = []
    # one arc on a flat ring: every start x length 8, 9, 10, 16 x polarity x margin
    for s in range(16):
        for n in (8, 9, 10, 16):
            for m in (1, 7, 8, 20, 21, 254, 255):
                for centre, val in ((0, m), (255, 255 - m), (m // 2, m // 2 + m if m // 2 + m <= 255 else None)):
                    if val is None:
                        continue
                    r = flat(centre)
                    for j in range(n):
                        r[1 + (s + j) % 16] = val
                    rings.append(r)
    # the pair step: run d[k+1..k+8] at margin rr, the end pixels d[k] and d[k+9] decide.  Every k (even k are the pairs the
    # network forms, odd k straddle two of them), both polarities.
    for k in range(16):
        for sgn in (1, -1):
            for rr in (50, 9):
                for ek, ek9 in ((30, 10), (10, 30), (rr, rr), (30, 30), (rr, 10), (10, rr), (rr + 30, 10), (10, rr + 30),
                                (rr + 30, rr + 30), (rr - 1, rr + 1), (rr + 1, rr - 1), (0, 0), (-5, rr), (rr, -5), (-5, -7)):
                    for other in (0, -20, 3):
                        centre = 128
                        r = flat(centre)
                        margins = np.full(16, other)
                        for j in range(1, 9):
                            margins[(k + j) % 16] = rr
                        margins[k] = ek
                        margins[(k + 9) % 16] = ek9
                        r[1:] = (centre + sgn * margins).astype(np.uint8)
                        rings.append(r)
    # ties between arcs of opposite polarity: half the ring above the centre and half below by the same amount (both best arcs
    # have the same negative minimum), 9 against 7 with equal and with unequal magnitudes, and 8 against 8 around a neutral pixel
    for s in range(16):
        for m in (1, 7, 20, 21, 127):
            for nb in (7, 8, 9):
                for m2 in (m, m + 1, max(m - 1, 0)):
                    r = flat(128)
                    for j in range(16):
                        r[1 + (s + j) % 16] = 128 + m if j < nb else 128 - m2
                    rings.append(r)
    # all-equal rings: S = 0
    for v in range(256):
        rings.append(flat(v))
    return np.stack(rings)


def extreme_rings():
    """Every ring of {0, 255} pixels at centre 0 and at centre 255."""
    bits = ((np.arange(1 << 16)[:, None] >> np.arange(16)[None]) & 1).astype(np.uint8) * 255
    return np.concatenate([np.concatenate([np.full((1 << 16, 1), c, np.uint8), bits], axis=1) for c in (0, 255)])


def random_rings():
    rng = np.random.default_rng(20250917)
    uni = rng.integers(0, 256, (1 << 20, 17), dtype=np.uint8)
    centre = rng.integers(0, 256, (1 << 20, 1))
    span = rng.choice([2, 8, 22, 40], (1 << 20, 1))
    near = np.clip(centre + rng.integers(-64, 65, (1 << 20, 16)) * span // 64, 0, 255)
    return np.concatenate([uni, np.concatenate([centre, near], axis=1).astype(np.uint8)])


def compiler():
    for c in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"), shutil.which("amdclang++")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no ROCm clang++")


def build_program(tmp_path, name, extra):
    src = tmp_path / "fast_score_main.cc"
    src.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.check_call([compiler(), "-x", "hip", "--offload-host-only", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          [str(src), "-o", str(exe)])
    return exe


def run_program(exe, tmp_path, rings):
    fin, fout = tmp_path / "rings.bin", tmp_path / "scores.bin"
    with open(fin, "wb") as f:
        f.write(np.array(CIRCLE, np.int8).tobytes())
        f.write(np.ascontiguousarray(rings, np.uint8).tobytes())
    subprocess.check_call([str(exe), str(fin), str(fout)], timeout=120)
    S = np.fromfile(fout, np.uint8)
    assert len(S) == len(rings)
    return S.astype(np.int16)


def oracle_scores(oracle, rings):
    L = oracle.lib()
    patch = np.zeros((7, 7), np.uint8)
    out = np.empty(len(rings), np.int16)
    base = patch.ctypes.data + 3 * 7 + 3
    for i, r in enumerate(rings):
        patch[3, 3] = r[0]
        for k, (dy, dx) in enumerate(CIRCLE):
            patch[3 + dy, 3 + dx] = r[1 + k]
        out[i] = L.orc_fast_corner_score(base, C.c_size_t(7), 0) + 1   # cornerScore = S - 1, and -1 where nothing exceeds 0
    return out


@pytest.fixture(scope="module")
def structured():
    rings = structured_rings()
    return rings, definition(rings)


def test_definition_on_known_rings():
    """The numpy statement itself, on rings whose score is known by hand."""
    r = flat(100)
    r[1:10] = 130                              # 9 pixels brighter by 30
    assert definition(r[None])[0] == 30
    r[9] = 100                                 # 8 pixels: no arc
    assert definition(r[None])[0] == 0
    r = flat(100)
    r[1:] = [60, 70, 80, 90, 60, 60, 60, 60, 65, 100, 100, 100, 100, 100, 100, 100]   # darker by 40,30,20,10,40,40,40,40,35
    assert definition(r[None])[0] == 10


def test_structured_rings(tmp_path, oracle, structured):
    rings, ref = structured
    exe = build_program(tmp_path, "fast_score", ["-O2"])
    S = run_program(exe, tmp_path, rings)
    bad = np.flatnonzero(S != ref)
    assert len(bad) == 0, (len(bad), rings[bad[:4]], S[bad[:4]], ref[bad[:4]])
    assert np.array_equal(oracle_scores(oracle, rings), ref)
    # the families reach what they are meant to: scores at both clamps, arcs of 8 without a corner
    assert ref.min() == 0 and ref.max() == 255 and (ref == 0).sum() > 1000


def test_extreme_and_random_rings(tmp_path):
    exe = build_program(tmp_path, "fast_score", ["-O2"])
    for rings in (extreme_rings(), random_rings()):
        ref = definition(rings)
        S = run_program(exe, tmp_path, rings)
        bad = np.flatnonzero(S != ref)
        assert len(bad) == 0, (len(bad), rings[bad[:4]], S[bad[:4]], ref[bad[:4]])
        assert (ref > 0).sum() > 1000   # the inputs do contain corners


def test_extreme_rings_oracle(oracle):
    """cornerScore on a sample of the {0, 255} rings (every 16th and the first 4096) agrees with the definition as well."""
    rings = extreme_rings()
    rings = np.concatenate([rings[::16], rings[:4096]])
    assert np.array_equal(oracle_scores(oracle, rings), definition(rings))


def test_sanitized_build(tmp_path, structured):
    """Address and undefined-behaviour sanitizers on the host build: the score reads only the 7 rows of its patch (malloc'ed to
    that size) and its 16-bit arithmetic does not overflow."""
    rings, ref = structured
    exe = build_program(tmp_path, "fast_score_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    S = run_program(exe, tmp_path, np.concatenate([rings, extreme_rings()[::64]]))
    assert np.array_equal(S[:len(rings)], ref)
