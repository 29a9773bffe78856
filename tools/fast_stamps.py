#!/usr/bin/env python3
"""Cycle shares of k_fast's sections (diagnostic build -DFAST_STAMPS, ORBHIP_LIB=build/liborbhip_fast.so).  GPU box only.
The stamps are thread 0's, so they time wavefront 0's cell of each group."""
import ctypes as C
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401

pkg = importlib.import_module("3_orb_slam3_selfnote_amd")
synth = importlib.import_module("3_orb_slam3_selfnote_amd.synth")
B, H, W = 256, 480, 752
frames, _ = synth.make_stream(1000, B)
ex = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
cap = ex.configure(H, W, B)
d_img = torch.from_numpy(frames).to("cuda")
d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
d_cnt = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
L = pkg.load()


def groups_per_frame():
    """k_fast's workgroups per frame: orbx_configure's groups of up to 2 x 2 cells (ORBextractor.cc:771-785 grid)."""
    n = 0
    for l in range(8):
        h, w = ex.level_shape(l)
        width, height = w - 32, h - 32
        nCols, nRows = width // 30, height // 30
        wCell, hCell = -(-width // nCols), -(-height // nRows)
        sx = 2 if 3 + 2 * wCell + 6 <= 80 else 1
        sy = 2 if 2 * hCell + 6 <= 76 else 1
        n += -(-nRows // sy) * -(-nCols // sx)
    return n


nwg = groups_per_frame() * B
buf = torch.zeros((nwg, 8), dtype=torch.int32, device="cuda")
L.orbx_debug_fast_stamps(C.c_void_p(buf.data_ptr()))
for it in range(3):
    buf.zero_()
    ex.extract_batch_device(d_img.data_ptr(), H, W, W, H * W, B, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), cap, (0, 1000), stream=0)
    torch.cuda.synchronize()
v = buf.cpu().numpy().astype(np.float64)
live = v[:, 0] > 0
# wavefront 0's cell (thread 0 stamps); a cell's second detection overwrites sections 1 and 2 with its own.  Slots in the order the
# kernel passes them; a cell outside the detection rectangle leaves after the barrier and stamps only the first two.
order = [3, 0, 4, 1, 2, 7]
names = {3: "arguments, group record, tile DMA issue", 0: "score plane clear + barrier (DMA wait)", 4: "barrier -> detection loop (cell record)",
         1: "pass1+2 compass+queue+score+list", 2: "pass3 NMS + emit", 7: "cell count"}
live = live & (v[:, 7] > 0)
m = v[live].mean(axis=0)
for i in order:
    print("%-40s %6.1f %%   %.0f cycles/workgroup" % (names[i], 100 * m[i] / m.sum(), m[i]))
print("prologue (first two sections) %.0f cycles/workgroup" % (m[3] + m[0]))
print("workgroups with work: %d of %d; total %.0f cycles/workgroup" % (live.sum(), nwg, m.sum()))
