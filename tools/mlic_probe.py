#!/usr/bin/env python3
"""Timing probe for the MLIC++ codec (rgbd_amd.mlic) on one GPU.

    python tools/mlic_probe.py [--reps 10] [--out profiles/mlic_probe.txt]

For B = 1 at 128x128 and at 512x640 (the padded 480x640 of the testers), at the model's own widths (N 192, M 320, ten slices):

1. wall time of encode and decode as the product runs them: replayed HIP graphs, a host clock around `reps` calls that end in a
   device synchronise, after the eager and the capturing call of the shape;
2. one eager call per direction with event pairs around its phases (rgbd_elic_set_profile(m, 3), graphs off): transforms (g_a,
   h_a, h_s / h_s, g_s), contexts (local, intra, inter, channel), parameter networks (the fused 1x1 stack), LRPs (four 3x3 layers
   and the in-place update), coder (the checkerboard parts, rANS).  The rest of the eager call -- layout conversion, the z
   stage, stream transfer -- is its wall time minus the phases.  Eager launches wait for the host between small kernels, so
   the phase times add up to more than a replayed call takes: they say where the time goes, the wall times say how much.

Every figure is measured on the GPU this runs on; nothing is printed without one.
"""
import argparse
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("transforms", "contexts", "params", "lrp", "coder")


def timed(fn, reps):
    fn()
    fn()  # eager, then the capturing call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def phases(net, fn):
    from rgbd_amd._lib import check, lib

    check(lib().rgbd_elic_set_profile(net._h, 3), "set_profile")
    try:
        fn()  # (the first eager call of a profile also sizes the event pool)
        check(lib().rgbd_elic_set_profile(net._h, 3), "set_profile")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        with tempfile.NamedTemporaryFile("r", suffix=".csv") as f:
            check(lib().rgbd_elic_profile_dump(net._h, f.name.encode()), "profile_dump")
            rows = {r[0]: (int(r[1]), float(r[2])) for r in (ln.strip().split(",") for ln in f.read().splitlines()[1:])}
    finally:
        check(lib().rgbd_elic_set_profile(net._h, 0), "set_profile")
    out = {p: rows.get("phase." + p, (0, 0.0)) for p in PHASES}
    out["eager_wall_ms"] = wall
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "mlic_probe.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlic_probe needs a GPU: nothing here is measured without one")
    import rgbd_amd
    from rgbd_amd import synth

    net = rgbd_amd.MLICPlusPlus().eval()
    net.load_state_dict(synth.synthetic_state_dict(0, model="MLIC"))
    net.update(force=True)
    net = net.to("cuda")
    lines = [f"MLIC++ (N 192, M 320, 10 slices), B = 1, synthetic stress weights; measured on {torch.cuda.get_device_name(0)}",
             f"wall: ms per call over {args.reps} replayed calls (HIP graphs); phases: one eager call, event pairs per phase "
             "(number of pairs, ms); rest = eager wall - phases"]
    with torch.cuda.stream(torch.cuda.Stream()):
        for H, W in ((128, 128), (512, 640)):
            x = torch.from_numpy(synth.synthetic_batch(1, H, W, config_id=84, smooth=True)[0]).cuda()
            out = net.compress(x)
            enc = timed(lambda: net.compress(x), args.reps)
            dec = timed(lambda: net.decompress(out["strings"], out["shape"]), args.reps)
            nbytes = sum(len(s) for lst in out["strings"] for s in lst)
            lines.append(f"{H}x{W}: {nbytes} bytes ({8 * nbytes / (H * W):.2f} bpp); encode {enc:.3f} ms, decode {dec:.3f} ms")
            for what, fn in (("encode", lambda: net.compress(x)), ("decode", lambda: net.decompress(out["strings"], out["shape"]))):
                ph = phases(net, fn)
                tot = sum(ph[p][1] for p in PHASES)
                lines.append(f"   {what} phases: " + ", ".join(f"{p} {ph[p][0]} x / {ph[p][1]:.3f} ms" for p in PHASES) +
                             f"; eager wall {ph['eager_wall_ms']:.3f} ms, rest {ph['eager_wall_ms'] - tot:.3f} ms")
    torch.cuda.synchronize()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
