#!/usr/bin/env python3
"""Call time of SynthesisTransformPlus (N = 192, M = 320, B = 1) for the 512x640 decode: y_hat 32x40, guides of 64x80, 128x160
and 256x320, ch = 3 and ch = 192 (what ELIC_master builds).  Device events around REPS calls in a row after WARM warm-up calls
(the third call of a shape on replays its captured graph); the median of ROUNDS windows, as tools/aligner_probe.py does.  Beside
it the same handle's time with its three aligners switched off (rgbd_debug_synthesis_plus_guides: the walk of
SynthesisTransformEX on the same weights) and the three stand-alone Spatial_aligner figures of DESIGN.md 5.3.  DESIGN.md 5.7
quotes it; no threshold is set."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rgbd_amd import SynthesisTransformPlus, _lib  # noqa: E402

WARM, REPS, ROUNDS = 5, 50, 7
ALONE_MS = (0.233, 0.323, 0.789)  # Spatial_aligner alone at 64x80, 128x160, 256x320
h, w = 32, 40
assert torch.cuda.is_available(), "synplus_probe needs a GPU"


def timed(call):
    for _ in range(WARM):
        call()
    ms = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(REPS):
            call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / REPS)
    return statistics.median(ms), min(ms), max(ms)


g = torch.Generator().manual_seed(h)
y = (torch.randn(1, 320, h, w, generator=g) * 2.0).cuda()
ups = [torch.randn(1, 192, (2 * h) << k, (2 * w) << k, generator=g).cuda() for k in range(3)]
for ch in (3, 192):
    m = SynthesisTransformPlus(192, 320, ch=ch).to("cuda")
    on = timed(lambda: m(y, *ups))
    assert _lib.lib().rgbd_debug_synthesis_plus_guides(m._h, 0) == 0
    off = timed(lambda: m(y, *ups))
    assert _lib.lib().rgbd_debug_synthesis_plus_guides(m._h, 1) == 0
    print(f"SynthesisTransformPlus ch={ch}, y_hat 1x320x{h}x{w} -> 1x{ch}x{16 * h}x{16 * w}: median {on[0]:.3f} ms per call "
          f"(min {on[1]:.3f}, max {on[2]:.3f}); without the aligners {off[0]:.3f} ms (min {off[1]:.3f}, max {off[2]:.3f}); "
          f"difference {on[0] - off[0]:.3f} ms, the three aligners alone {sum(ALONE_MS):.3f} ms "
          f"({' + '.join(f'{v:.3f}' for v in ALONE_MS)}); {ROUNDS} windows of {REPS} calls")
    del m
