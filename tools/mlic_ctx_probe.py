#!/usr/bin/env python3
"""Call time of MLIC++'s attention contexts at the latent size of a 512x640 image, [1, ., 32, 40]: LocalContext(32),
LinearGlobalIntraContext(32, 2 heads), LinearGlobalInterContext at dim 32, 160 and 288 (1, 5 and 9 heads of 32), and the
local-attention launch alone (rgbd_local_ckbd_attention on device buffers).  Device events around REPS calls in a row after
WARM warm-up calls of the shape (the third call of a shape on replays its captured graph); the median of ROUNDS windows.
DESIGN.md 5.4 quotes it."""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rgbd_amd import LinearGlobalInterContext, LinearGlobalIntraContext, LocalContext  # noqa: E402
from rgbd_amd._lib import check, lib  # noqa: E402

WARM, REPS, ROUNDS = 5, 50, 7
H, W = 32, 40
assert torch.cuda.is_available(), "mlic_ctx_probe needs a GPU"


def timed(what, call):
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
    print(f"{what}: median {statistics.median(ms) * 1e3:.1f} us per call (min {min(ms) * 1e3:.1f}, max {max(ms) * 1e3:.1f}; "
          f"{ROUNDS} windows of {REPS} calls)")


g = torch.Generator().manual_seed(0)
x = {d: torch.randn(1, d, H, W, generator=g).cuda() for d in (32, 160, 288)}
x2 = torch.randn(1, 32, H, W, generator=g).cuda()
lc = LocalContext(dim=32).to("cuda")
timed(f"LocalContext 1x32x{H}x{W}", lambda: lc(x[32]))
ia = LinearGlobalIntraContext(dim=32, num_heads=2).to("cuda")
timed(f"LinearGlobalIntraContext 1x32x{H}x{W}", lambda: ia(x[32], x2))
for d in (32, 160, 288):
    ie = LinearGlobalInterContext(dim=d, out_dim=64, num_heads=d // 32).to("cuda")
    timed(f"LinearGlobalInterContext 1x{d}x{H}x{W}, {d // 32} heads", lambda: ie(x[d]))

L = lib()
qkv = torch.randn(1, H, W, 96, generator=g).cuda()
table, fw, fb = torch.randn(81, 2, generator=g).cuda(), (torch.randn(64, 32, 5, 5, generator=g) / 28).cuda(), torch.zeros(64).cuda()
out = torch.empty(1, H, W, 64, device="cuda")
p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
timed(f"rgbd_local_ckbd_attention 1x{H}x{W}x96 alone ({(H // 2) * (W // 4)} workgroups)",
      lambda: check(L.rgbd_local_ckbd_attention(p(qkv), 96, 1, H, W, 32, 2, p(table), p(fw), p(fb), p(out), 64, stream), "local"))
