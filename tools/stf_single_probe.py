#!/usr/bin/env python3
"""Timing probe for the single-modal STF (rgbd_amd.stf) on one GPU: ms per compress() / decompress() call at B = 1,
512x512 and 512x640, and at B = 4 with per-image streams, with the convolution time split by layer family.

    python tools/stf_single_probe.py [--reps 10] [--json out.json]

Two measurements per call shape: wall time of replayed calls (HIP graphs, the product path: events around `reps` calls
after the eager and the capturing call), and one profiled call (event pairs around every conv launch, graphs off), whose
conv milliseconds are summed per family: transforms (patch_embed / layers / syn_layers / end_conv), hyper nets (h_a,
h_mean_s, h_scale_s), slice loop (cc_mean / cc_scale / lrp transforms).  What a profiled call spends outside convolutions
(LayerNorm, window attention, the slice kernels and the rANS coder) is reported as `other_ms` = profiled wall - conv ms; for
the decoder that is dominated by the 12 resumable rANS launches.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FAMILIES = (("transforms", ("patch_embed", "layers.", "syn_layers.", "end_conv")),
            ("hyper_nets", ("h_a.", "h_mean_s.", "h_scale_s.")),
            ("slice_loop_convs", ("cc_mean_transforms.", "cc_scale_transforms.", "lrp_transforms.")))


def family_ms(net):
    from rgbd_amd._lib import check, lib

    with tempfile.NamedTemporaryFile("r", suffix=".csv") as f:
        check(lib().rgbd_elic_profile_dump(net._h, f.name.encode()), "profile_dump")
        rows = [ln.strip().split(",") for ln in f.read().splitlines()[1:]]
    out = {k: 0.0 for k, _ in FAMILIES}
    for r in rows:
        for k, pre in FAMILIES:
            if r[0].startswith(pre):
                out[k] += float(r[2])
    return out


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
    net.set_profile(True)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        fam = family_ms(net)
    finally:
        net.set_profile(False)
    fam["other_ms"] = wall - sum(fam.values())
    fam["profiled_wall_ms"] = wall
    return fam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json")
    args = ap.parse_args()
    import rgbd_amd
    from rgbd_amd import synth

    net = rgbd_amd.modelZoo["STF"]().eval()
    net.load_state_dict(synth.synthetic_state_dict(0, model="STF"))
    net.update(force=True)
    net = net.to("cuda")
    res = []
    with torch.cuda.stream(torch.cuda.Stream()):
        for B, H, W, per_image in ((1, 512, 512, False), (1, 512, 640, False), (4, 512, 640, True)):
            x = torch.from_numpy(synth.synthetic_batch(B, H, W, config_id=70)[0]).cuda()
            net.per_image_streams = per_image
            out = net.compress(x)
            row = {"B": B, "H": H, "W": W, "per_image_streams": per_image, "symbols": B * 384 * (H // 16) * (W // 16),
                   "bytes": sum(len(s) for lst in out["strings"] for s in lst),
                   "compress_ms": timed(lambda: net.compress(x), args.reps),
                   "decompress_ms": timed(lambda: net.decompress(out["strings"], out["shape"]), args.reps),
                   "compress_profile": profiled(net, lambda: net.compress(x)),
                   "decompress_profile": profiled(net, lambda: net.decompress(out["strings"], out["shape"]))}
            res.append(row)
            print(json.dumps(row))
    net.per_image_streams = False
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
