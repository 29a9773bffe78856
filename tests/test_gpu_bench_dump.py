"""GPU: `bench.py --dump-outputs DIR` on a small EuRoC run.  The files hold what the last timed step's final batches handed back
(counts, nmatches, a sampled set of frames' keypoints, undistorted keypoints, descriptors and match indices), all float32, with
shapes that follow from the counts; one sampled frame's keypoints and descriptors are compared with the oracle's extraction of the
same synthetic input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import EUROC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S = 32, 2


def test_dump_outputs_match_the_oracle(tmp_path, synth, oracle):
    d = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", str(B),
           "--batches-per-step", "4", "--groups", "2", "--streams", str(S), "--dump-outputs", d]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["unit"] == "frames/s"
    assert "roofline" not in line and "cpu_baseline" not in line

    a = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert set(a) == {"counts", "nmatches", "frames", "keypoints", "keypoints_un", "descriptors", "matches"}
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    cnt = a["counts"].astype(np.int64)
    F = S * B
    assert cnt.shape == (F, 2) and a["nmatches"].shape == (F,) and (cnt[:, 0] > 100).all()
    sel = np.arange(F)           # fewer frames than the sample size: every frame is written, in batch order
    assert a["frames"].shape == (F, 2)
    nk = int(cnt[sel, 0].sum())
    nq = int(sum(cnt[(f // B) * B + (f % B - 1) % B, 0] for f in sel))     # match_of_query: one per keypoint of the frame before
    assert a["keypoints"].shape == (nk, 7) and a["keypoints_un"].shape == (nk, 7) and a["descriptors"].shape == (nk, 32)
    assert a["matches"].shape == (nq,) and a["matches"].min() >= -1 and (a["matches"] >= 0).any()

    g, t = (int(x) for x in a["frames"][0])
    frames, _ = synth.make_stream(1000 + g, B, 480, 752)
    mono, kps, desc = oracle.OracleExtractor(**EUROC).extract(frames[t], (0, 1000))
    n = int(cnt[0, 0])
    assert n == len(kps) and int(cnt[0, 1]) == mono
    ref = np.stack([kps[f].astype(np.float32) for f in ("x", "y", "size", "angle", "response", "octave", "class_id")], axis=1)
    assert np.array_equal(a["keypoints"][:n], ref)
    assert np.array_equal(a["descriptors"][:n], desc.astype(np.float32))
