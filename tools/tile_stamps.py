#!/usr/bin/env python3
"""Where k_resize's and k_blur's workgroups spend their cycles up to the tile (diagnostic builds -DTILE_STAMPS).  GPU box only.

    python tools/tile_stamps.py build/liborbhip_tile_parent.so build/liborbhip_tile.so

Per library (each in a child process of its own: a process loads one liborbhip) and per kernel and level: the median, over the
workgroups of one 256-frame EuRoC batch, of thread 0's cycles from kernel entry to "tile fetch issued", to "tile landed" (behind
the barrier) and to the end.  k_resize's one-pass form stages no tile and stamps the end only."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W = 256, 480, 752


def child():
    sys.path.insert(0, ROOT)
    import torch
    pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
    synth = importlib.import_module("3_orb_slam3_selfnote_amd.synth")
    frames, _ = synth.make_stream(1000, B)
    ex = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    cap = ex.configure(H, W, B)
    d_img = torch.from_numpy(frames).to("cuda")
    d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    L = pkg.load()
    # rows: k_blur's tiles (128 x 64 outputs), then k_resize's row tiles (16 output rows; EuRoC takes no 8-row level) of levels 1 .. 7
    shapes = [ex.level_shape(l) for l in range(8)]
    nblur = sum(-(-w // 128) * -(-h // 64) for h, w in shapes) * B
    nres = sum(-(-h // 16) for h, _ in shapes[1:]) * B
    buf = torch.zeros((nblur + nres + 1024, 8), dtype=torch.int32, device="cuda")   # (slack: the tail must stay untouched, checked below)
    L.orbx_debug_fast_stamps(C.c_void_p(buf.data_ptr()))
    for _ in range(3):
        buf.zero_()
        ex.extract_batch_device(d_img.data_ptr(), H, W, W, H * W, B, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), cap, (0, 1000), stream=0)
        torch.cuda.synchronize()
    v = buf.cpu().numpy().astype(np.int64)
    assert not v[nblur + nres:].any(), "stamps beyond the expected workgroups: the row count here disagrees with orbx_configure"
    for name, rows in (("k_blur", v[:nblur]), ("k_resize", v[nblur:nblur + nres])):
        assert (rows[:, 3] > 0).all(), "%s: %d workgroups left no stamp" % (name, int((rows[:, 3] == 0).sum()))
        for l in sorted(set(rows[:, 3] - 1)):
            r = rows[rows[:, 3] - 1 == l]
            m = np.median(r[:, :3], axis=0)
            print("%-8s level %d  %7d workgroups   fetch issued %6.0f   tile landed %6.0f   end %6.0f cycles (medians)" % (name, l, len(r), m[0], m[1], m[2]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
    else:
        for lib in sys.argv[1:] or [os.path.join(ROOT, "build", "liborbhip_tile.so")]:
            print("== %s" % lib, flush=True)
            env = dict(os.environ, ORBHIP_LIB=os.path.abspath(lib))
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env).returncode
            if rc != 0:
                sys.exit(rc)
