#!/usr/bin/env python3
"""The rate probe's kernels at 1920 x 1088 with the built-in tables, for a profiler: bitrate mode, five-mode inter frames, a key
frame every fourth frame, 12 frames of a panning texture.  Run it under `rocprofv3 --kernel-trace --stats -- python
tools/enc_quant_probe_time.py` and read k_rate_dc<false> / k_rate_tok<false> (key frames) and k_rate_dc<true> / k_rate_tok<true>
(inter frames) from the kernel statistics; profiles/enc_quant_probe_times.txt holds such runs."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from theora_amd.encoder import Encoder   # noqa: E402

W, H, N = 1920, 1088, 12
rng = np.random.default_rng(1)
big = [rng.integers(0, 256, (H // d + 64, W // d + 64), dtype=np.uint8) for d in (1, 2, 2)]
y, x = np.mgrid[0:H + 64, 0:W + 64]
big[0] = ((big[0].astype(np.int64) // 4 + 96 + 64 * np.sin(x / 37.0) * np.cos(y / 23.0)).clip(0, 255)).astype(np.uint8)
e = Encoder(W, H, 0, 32, inter=True, keyframe_interval=4, bitrate=8000000)
e.header_packets()
total = 0
for f in range(N):
    dx, dy = 2 * f, f
    fr = [np.ascontiguousarray(big[0][dy:dy + H, dx:dx + W])] + \
         [np.ascontiguousarray(big[p][dy // 2:dy // 2 + H // 2, dx // 2:dx // 2 + W // 2]) for p in (1, 2)]
    e.encode(fr)
    total += len(e.packetout(f == N - 1)[0])
e.close()
print("frames", N, "bytes", total)
