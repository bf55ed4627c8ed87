#!/usr/bin/env python3
"""Call times of the latent codec of ELIC_master (rgbd_amd.MasterLatentCodec, engine family 20) for B = 1 at 512 x 640: f
1x128x512x640, guides of 64x80, 128x160 and 256x320, f_hat 1x192x512x640.  compress, decompress and forward as whole calls
(host clock around synchronised calls: they end with the streams / f_hat on the host side of the call), and decompress split by
device events into what a call adds over its parts: the guided g_s alone is timed on a SynthesisTransformPlus(ch = 192) handle
of the same shapes (DESIGN.md 5.7's figure, measured again in this process), the entropy loop is the rest.  WARM warm-up calls
first (the third call of a shape on replays its captured graph), then the median of ROUNDS windows of REPS calls.

The engine is created BEFORE any other GPU work of the process (DESIGN.md 5.6 records what the other order did): no tensor is
moved to the device before MasterLatentCodec.to("cuda") has returned.  DESIGN.md 5.10 quotes the output; no threshold is set."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rgbd_amd import MasterLatentCodec, SynthesisTransformPlus, model_config, synth  # noqa: E402

WARM, REPS, ROUNDS = 4, 10, 5
H, W = 512, 640
assert torch.cuda.is_available(), "master_latent_probe needs a GPU"

cfg = model_config()
net = MasterLatentCodec(config=cfg).eval()
net.load_state_dict(synth.synthetic_state_dict(21, config=cfg, model="ELIC_master_latent"), strict=True)
net.update(force=True)
net = net.to("cuda")  # the engine exists before anything else touches the GPU

g = torch.Generator().manual_seed(7)
f_host = torch.randn(1, 128, H, W, generator=g)
ups_host = [torch.randn(1, 192, H >> (3 - k), W >> (3 - k), generator=g) for k in range(3)]
side = torch.cuda.Stream()  # (the NULL stream is not captured)


def timed(call):
    for _ in range(WARM):
        call()
    ms = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / REPS)
    return statistics.median(ms), min(ms), max(ms)


def timed_events(call):
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


def row(what, t):
    print(f"{what}: median {t[0]:.3f} ms per call (min {t[1]:.3f}, max {t[2]:.3f}); {ROUNDS} windows of {REPS} calls", flush=True)


with torch.cuda.stream(side):
    f, ups = f_host.cuda(), [u.cuda() for u in ups_host]
    out = net.compress(f)
    nbytes = len(out["strings"][0][0]) + sum(len(s) for s in out["strings"][1])
    print(f"MasterLatentCodec B=1 {H}x{W}: {nbytes} bytes, {nbytes * 8 / (H * W):.2f} bpp, workspace {net.workspace_bytes() / 2**20:.0f} MiB")
    row("compress (f -> streams)", timed(lambda: net.compress(f)))
    dec = timed(lambda: net.decompress(out["strings"], out["shape"], *ups))
    row("decompress (streams + guides -> f_hat)", dec)
    row("forward (f + guides -> f_hat, likelihoods)", timed_events(lambda: net.forward(f, *ups)))
    print(f"workspace after all three calls {net.workspace_bytes() / 2**20:.0f} MiB, cached graphs {net.graph_count()}")
    yhat = torch.from_numpy(net.debug_tensor("yhat")).cuda()
    gs = SynthesisTransformPlus(192, 320, ch=192)
    gs.load_state_dict({k[len("g_s."):]: v for k, v in net.state_dict().items() if k.startswith("g_s.")})
    gs = gs.to("cuda")
    t_gs = timed_events(lambda: gs(yhat, *ups))
    row("guided g_s alone (SynthesisTransformPlus ch=192 on the codec's y_hat and weights)", t_gs)
    print(f"decompress split: guided g_s {t_gs[0]:.3f} ms, entropy loop and the rest of the call {dec[0] - t_gs[0]:.3f} ms")
torch.cuda.synchronize()
