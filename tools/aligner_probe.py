#!/usr/bin/env python3
"""Call time of Spatial_aligner (192 -> 192 channels, B = 1) at the three map sizes ELIC_master would run it for a 512x640
image: 64x80, 128x160, 256x320 (behind up1, up2, up3).  Device events around REPS calls in a row after WARM warm-up calls of
the shape (the third call of a shape on replays its captured graph); the median of ROUNDS windows.  DESIGN.md 5 quotes it."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rgbd_amd import Spatial_aligner  # noqa: E402

WARM, REPS, ROUNDS = 5, 50, 7
assert torch.cuda.is_available(), "aligner_probe needs a GPU"
sa = Spatial_aligner(in_channel=192, out_channel=192).to("cuda")
for H, W in ((64, 80), (128, 160), (256, 320)):
    g = torch.Generator().manual_seed(H)
    x, gd = torch.randn(1, 192, H, W, generator=g).cuda(), torch.randn(1, 192, H, W, generator=g).cuda()
    for _ in range(WARM):
        sa(x, gd)
    ms = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(REPS):
            sa(x, gd)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / REPS)
    tokens = (H // 2) * (W // 2)
    print(f"Spatial_aligner 1x192x{H}x{W} ({tokens} tokens, {tokens // 16 * 3} (window, head) pairs per block): "
          f"median {statistics.median(ms):.3f} ms per call (min {min(ms):.3f}, max {max(ms):.3f}; {ROUNDS} windows of {REPS} calls)")
