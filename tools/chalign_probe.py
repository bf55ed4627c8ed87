#!/usr/bin/env python3
"""Timing probe for the pooled 3x3 head of Channel_aligner (csrc/pooled_head.hip) on one GPU.

    python tools/chalign_probe.py [--iters 50] [--json out.json]

1. The pooled head alone (rgbd_pooled_conv3x3, Cin 256 -> Cout 64) at 480x640 and 256x256 with B = 1 and B = 4: device events
   around `iters` launches on an NHWC map, after a warm-up launch.  Reported with it: the bytes of the map over that time --
   the head's achieved read rate -- as a share of the MI355X's HBM peak.  (A map that fits the 256 MiB Infinity Cache, 67 MB
   at 256x256 with B = 1, is re-read from there between launches: that row is no HBM figure and says so.)
2. Beside it the unfused form of the same shape, from launches the library already exports: the 256 -> 64 3x3 convolution
   (rgbd_conv_bench, kernel-only time on NHWC scratch) plus the channel mean of its 64-channel output
   (rgbd_pw_channel_mean, device events).
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
CIN, COUT = 256, 64


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def event_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def head_row(L, B, H, W, iters):
    from rgbd_amd._lib import check

    x = torch.randn(B, H, W, CIN, device="cuda")
    w, b = torch.randn(COUT, CIN, 3, 3, device="cuda") / 48, torch.randn(COUT, device="cuda")
    n = L.rgbd_pooled_conv3x3_ws_floats(B, H, W, CIN)
    ws, out = torch.empty(n, device="cuda"), torch.empty(B, COUT, device="cuda")
    head = event_ms(lambda: check(L.rgbd_pooled_conv3x3(_p(x), CIN, B, H, W, CIN, _p(w), _p(b), COUT, _p(out), _p(ws), _stream()),
                                  "pooled_conv3x3"), iters)
    ms_c = ctypes.c_float(0)
    check(L.rgbd_conv_bench(B, CIN, H, W, COUT, 3, 1, 1, 0, 0, iters, ctypes.byref(ms_c)), "conv_bench")
    y, mean = torch.randn(B, H, W, COUT, device="cuda"), torch.empty(B, COUT, device="cuda")
    pool = event_ms(lambda: check(L.rgbd_pw_channel_mean(_p(y), B, H * W, COUT, COUT, _p(mean), COUT, _stream()), "channel_mean"),
                    iters)
    nbytes = 4.0 * B * H * W * CIN
    return {"B": B, "H": H, "W": W, "head_ms": head, "conv3x3_ms": ms_c.value, "channel_mean_ms": pool,
            "unfused_ms": ms_c.value + pool, "unfused_over_head": (ms_c.value + pool) / head, "map_bytes": nbytes,
            "head_tbytes_s": nbytes / head / 1e9, "share_of_hbm_peak": nbytes / head / 1e-3 / PEAK_HBM,
            "map_fits_l3": nbytes <= L3_BYTES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chalign_probe needs a GPU: nothing here is measured without one")
    from rgbd_amd._lib import lib

    res = {"head": []}
    with torch.cuda.stream(torch.cuda.Stream()):
        for B, H, W in [(B, H, W) for (H, W) in ((480, 640), (256, 256)) for B in (1, 4)]:
            row = head_row(lib(), B, H, W, args.iters)
            res["head"].append(row)
            print(json.dumps(row), flush=True)
    torch.cuda.synchronize()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
