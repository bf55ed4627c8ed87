#!/usr/bin/env python3
"""Call times of MLIC++'s per-slice networks: EntropyParametersMLIC 960 -> 64 and 640 -> 64 as the fused launch
(csrc/pixel_mlp.hip) against the same handle with `fused = False` (four conv launches over the written-out concatenation), at
16x16 and 32x40 with B = 1 and at 32x40 with B = 4, with the fused-to-unfused ratio per size; and ChannelContext 288 -> 32 and
LatentResidualPrediction 640 -> 32 at 32x40.  Device events around REPS calls in a row after WARM warm-up calls (the third call
of a shape on replays its captured graph); the median of ROUNDS windows with the smallest and the largest, as
tools/synplus_probe.py does.  The engine is created first and everything runs on the stream the module submits to.

Without arguments every step runs in a child process of its own under a time limit, and the first step that fails or runs out
of time ends the probe; `--step NAME` is one step.  DESIGN.md 5.8 quotes the output; no threshold is set."""
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, REPS, ROUNDS = 5, 50, 7
STEP_SECONDS = 120
SEGMENTS = {960: [64, 64, 64, 128, 640], 640: [640]}
STEPS = [f"ep{d}_{b}x{h}x{w}" for d in (960, 640) for (b, h, w) in ((1, 16, 16), (1, 32, 40), (4, 32, 40))] + \
        ["cc288_1x32x40", "lrp640_1x32x40"]


def timed(torch, call):
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


def fmt(t):
    return f"median {1e3 * t[0]:.1f} us (min {1e3 * t[1]:.1f}, max {1e3 * t[2]:.1f})"


def step(name):
    import torch

    import rgbd_amd

    assert torch.cuda.is_available(), "mlic_slice_probe needs a GPU"
    kind, shape = name.split("_")
    B, H, W = (int(v) for v in shape.split("x"))
    g = torch.Generator().manual_seed(H)
    if kind.startswith("ep"):
        d = int(kind[2:])
        m = rgbd_amd.EntropyParametersMLIC(d, 64).to("cuda")  # the engine first
        xs = [torch.randn(B, c, H, W, generator=g).cuda() for c in SEGMENTS[d]]
        out = torch.empty(B, 64, H, W, device="cuda")
        fused = timed(torch, lambda: m.forward_segments(xs, out=out))
        m.fused = False
        unfused = timed(torch, lambda: m.forward_segments(xs, out=out))
        print(f"EntropyParametersMLIC {d} -> 64, {B}x{H}x{W}, {len(xs)} segment(s): fused {fmt(fused)}; four conv launches "
              f"{fmt(unfused)}; fused / unfused {fused[0] / unfused[0]:.2f}; {ROUNDS} windows of {REPS} calls", flush=True)
        return
    cls, d = (rgbd_amd.ChannelContext, 288) if kind.startswith("cc") else (rgbd_amd.LatentResidualPrediction, 640)
    m = cls(d, 32).to("cuda")
    x = torch.randn(B, d, H, W, generator=g).cuda()
    t = timed(torch, lambda: m(x))
    print(f"{cls.__name__} {d} -> 32, {B}x{H}x{W}: {fmt(t)}; {ROUNDS} windows of {REPS} calls", flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        return step(sys.argv[2])
    for name in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired:
            sys.exit(f"step {name} ran out of its {STEP_SECONDS} s: stopping here")
        if r.returncode:
            sys.exit(f"step {name} ended with status {r.returncode}: stopping here")


if __name__ == "__main__":
    main()
