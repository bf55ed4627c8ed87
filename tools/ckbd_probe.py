#!/usr/bin/env python3
"""Timing probe for the checkerboard Cheng2020 model (rgbd_amd.ckbd) and its fused GDN launch on one GPU.

    python tools/ckbd_probe.py [--reps 20] [--iters 200] [--json out.json]

1. Encode and decode Mpx/s at 480x640 (padded to 512x640 as the testers do: dataset/utils.py:58-67) for B = 1 and B = 4
   (per-image streams): wall time of replayed calls (HIP graphs, the product path) -- a host clock around `reps` calls that
   end in a device synchronise, after the eager and the capturing call of the shape.  Mpx/s counts the 480x640 pixels of the
   images, not the padding.  One profiled call per shape (event pairs around every conv and GDN launch, graphs off) gives the
   GDN share of the transform time.
2. The GDN launch alone (rgbd_gdn_bench: device events around `iters` launches on NHWC scratch buffers, after a warm-up
   launch) at (4, 192, 240, 320) and (4, 192, 30, 40), GDN and IGDN, with the residual operand, each next to its yardstick on
   the same build: rgbd_conv_bench on the 1x1 convolution of the same shape (n, 192, h, w, 192, k = 1, with the residual
   operand).  Reported: both times, their ratio, and the GDN launch's achieved FLOP/s (2 C^2 per pixel) and bytes/s (x, the
   residual and the output, once each) against the MI355X's fp32-matrix and HBM peaks.
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MATRIX = 157.3e12  # FLOP/s, MI355X fp32 MFMA
PEAK_HBM = 8.0e12           # bytes/s


def timed(fn, reps):
    fn()
    fn()  # eager, then the capturing call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def profiled(net, fn):
    from rgbd_amd._lib import check, lib

    net.set_profile(True)
    try:
        fn()
        torch.cuda.synchronize()
        with tempfile.NamedTemporaryFile("r", suffix=".csv") as f:
            check(lib().rgbd_elic_profile_dump(net._h, f.name.encode()), "profile_dump")
            rows = [ln.strip().split(",") for ln in f.read().splitlines()[1:]]
    finally:
        net.set_profile(False)
    gdn = sum(float(r[2]) for r in rows if r[0].endswith("gdn"))
    return {"gdn_ms": gdn, "conv_ms": sum(float(r[2]) for r in rows) - gdn}


def gdn_alone(L, n, c, h, w, iters):
    from rgbd_amd._lib import check

    out = []
    for inverse in (0, 1):
        ms_g, ms_c = ctypes.c_float(0), ctypes.c_float(0)
        check(L.rgbd_gdn_bench(n, c, h, w, inverse, 1, iters, ctypes.byref(ms_g)), "gdn_bench")
        check(L.rgbd_conv_bench(n, c, h, w, c, 1, 1, 0, 0, 1, iters, ctypes.byref(ms_c)), "conv_bench")
        px = n * h * w
        flops, nbytes = 2.0 * c * c * px, 3.0 * 4 * c * px
        out.append({"shape": [n, c, h, w], "inverse": inverse, "gdn_ms": ms_g.value, "conv1x1_ms": ms_c.value,
                    "ratio": ms_g.value / ms_c.value, "tflops": flops / ms_g.value / 1e9, "tbytes_s": nbytes / ms_g.value / 1e9,
                    "share_of_peak": max(flops / PEAK_F32_MATRIX, nbytes / PEAK_HBM) / (ms_g.value * 1e-3),
                    "bound": "fp32 matrix" if flops / PEAK_F32_MATRIX > nbytes / PEAK_HBM else "HBM"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ckbd_probe needs a GPU: nothing here is measured without one")
    import rgbd_amd
    from rgbd_amd import synth
    from rgbd_amd._lib import lib

    net = rgbd_amd.modelZoo["ckbd"](N=192, channel=3).eval()
    net.load_state_dict(synth.synthetic_state_dict(0, model="ckbd"))
    net.update(force=True)
    net = net.to("cuda")
    res = {"codec": [], "gdn": []}
    with torch.cuda.stream(torch.cuda.Stream()):
        for B in (1, 4):
            x = torch.from_numpy(synth.synthetic_batch(B, 480, 640, config_id=74, smooth=True)[0]).cuda()
            x = F.pad(x, (0, 0, 0, 32), mode="replicate")  # 480 -> 512 rows
            net.per_image_streams = B > 1
            out = net.compress(x)
            enc = timed(lambda: net.compress(x), args.reps)
            dec = timed(lambda: net.decompress(out["strings"], out["shape"]), args.reps)
            mpx = B * 480 * 640 / 1e6
            row = {"B": B, "H": 480, "W": 640, "bytes": sum(len(s) for lst in out["strings"] for s in lst), "compress_ms": enc,
                   "decompress_ms": dec, "encode_mpx_s": mpx / (enc * 1e-3), "decode_mpx_s": mpx / (dec * 1e-3),
                   "compress_profile": profiled(net, lambda: net.compress(x)),
                   "decompress_profile": profiled(net, lambda: net.decompress(out["strings"], out["shape"]))}
            res["codec"].append(row)
            print(json.dumps(row))
    net.per_image_streams = False
    torch.cuda.synchronize()
    for shape in ((4, 192, 240, 320), (4, 192, 30, 40)):
        for row in gdn_alone(lib(), *shape, args.iters):
            res["gdn"].append(row)
            print(json.dumps(row))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
