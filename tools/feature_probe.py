#!/usr/bin/env python3
"""Timing probe for the thin 3x3 layers of Feature_encoder / Feature_decoder (csrc/thin_conv.hip) on one GPU.

    python tools/feature_probe.py [--iters 50] [--json out.json]

1. Each thin operator alone -- rgbd_conv3x3_thin_in (3 | 1 -> 64) and rgbd_conv3x3_thin_out (64 -> 3 | 1) -- at 480x640 and
   256x256 with B = 1 and B = 4: device events around `iters` launches after a warm-up launch.  Reported with it: the bytes the
   operator must move (the image planes and the 64-channel map, once each) over that time, as a share of the MI355X's HBM peak.
   (A working set that fits the 256 MiB Infinity Cache is re-used from there between launches: such a row is no HBM figure and
   says so.)
2. Beside it the same layer on the route the library had: rgbd_conv2d_nchw (the exported operator: weight packing, the layout
   passes to and from a 16-channel padded NHWC buffer, the MFMA convolution; device events around `iters / 5` calls), and the
   MFMA convolution of that route alone (rgbd_conv_bench: kernel-only time on padded NHWC scratch).

No engine handle is created here (DESIGN.md 5.6 says why the two networks are not in the tree).
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_HBM = 8.0e12  # bytes/s
L3_BYTES = 256 * 2 ** 20
WIDE = 64
SIZES = [(B, H, W) for (H, W) in ((480, 640), (256, 256)) for B in (1, 4)]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def event_ms(fn, iters, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _host(t):
    return t.numpy().ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def thin_row(L, op, B, H, W, thin, iters):
    from rgbd_amd._lib import check

    g = torch.Generator().manual_seed(1)
    if op == "thin_in":
        x = torch.randn(B, thin, H, W, generator=g).cuda()
        w, b = torch.randn(WIDE, thin, 3, 3, generator=g) / 5, torch.randn(WIDE, generator=g)
        wd, bd, y = w.cuda(), b.cuda(), torch.empty(B, H, W, WIDE, device="cuda")
        ms = event_ms(lambda: check(L.rgbd_conv3x3_thin_in(_p(x), B, thin, H, W, _p(wd), _p(bd), WIDE, _p(y), WIDE, _stream()), op), iters)
        y2 = torch.empty(B, WIDE, H, W, device="cuda")
        route = event_ms(lambda: check(L.rgbd_conv2d_nchw(_p(x), B, thin, H, W, _host(w), _host(b), WIDE, 3, 1, 1, 0, 0, None, _p(y2),
                                                          _stream()), "conv2d_nchw"), max(1, iters // 5))
        bench = (B, thin, H, W, WIDE, 3, 1, 1, 0, 0)
    else:
        x = torch.randn(B, H, W, WIDE, generator=g).cuda()
        t, b = torch.randn(WIDE, thin, 3, 3, generator=g) / 24, torch.randn(thin, generator=g)  # ConvTranspose2d layout
        wd, bd = t.transpose(0, 1).flip(2, 3).contiguous().cuda(), b.cuda()
        y = torch.empty(B, thin, H, W, device="cuda")
        ms = event_ms(lambda: check(L.rgbd_conv3x3_thin_out(_p(x), WIDE, B, H, W, WIDE, _p(wd), _p(bd), thin, _p(y), _stream()), op), iters)
        xn = torch.randn(B, WIDE, H, W, device="cuda")
        wh = wd.cpu()  # (the route runs the layer as the convolution it is: the weight in convolution orientation)
        route = event_ms(lambda: check(L.rgbd_conv2d_nchw(_p(xn), B, WIDE, H, W, _host(wh), _host(b), thin, 3, 1, 1, 0, 0, None, _p(y),
                                                          _stream()), "conv2d_nchw"), max(1, iters // 5))
        bench = (B, WIDE, H, W, thin, 3, 1, 1, 0, 0)
    ms_c = ctypes.c_float(0)
    check(L.rgbd_conv_bench(*bench, iters, ctypes.byref(ms_c)), "conv_bench")
    nbytes = 4.0 * B * H * W * (WIDE + thin)
    return {"op": op, "B": B, "H": H, "W": W, "thin_channels": thin, "ms": ms, "conv2d_nchw_ms": route, "conv_mfma_kernel_ms": ms_c.value,
            "route_over_thin": route / ms, "mfma_kernel_over_thin": ms_c.value / ms, "bytes": nbytes, "gbytes_s": nbytes / ms / 1e6,
            "share_of_hbm_peak": nbytes / ms / 1e-3 / PEAK_HBM, "fits_l3": nbytes <= L3_BYTES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_probe needs a GPU: nothing here is measured without one")
    from rgbd_amd._lib import lib

    res = {"operators": []}
    with torch.cuda.stream(torch.cuda.Stream()):
        for op, thin in (("thin_in", 3), ("thin_in", 1), ("thin_out", 3), ("thin_out", 1)):
            for B, H, W in SIZES:
                row = thin_row(lib(), op, B, H, W, thin, args.iters)
                res["operators"].append(row)
                print(json.dumps(row), flush=True)
    torch.cuda.synchronize()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
