#!/usr/bin/env python3
"""Split-K tuner for the small-grid layers (latent grid: entropy-parameter nets, channel / local context, hyper synthesis,
M-channel attention units, h_a).  For every distinct conv shape of one compress()+decompress() whose per-image output grid
has at most --max-px pixels, times (kernel + reducer, rgbd_conv_bench) every split factor x tile x staging mode and
writes the winners:

    csrc/splitk_table.h   {OH*OW per image, cin_pad, cout_pad, ntaps, nphase} -> S   (a function of the LAYER and the
                          per-image grid only, never of the batch: the summation order of an output must be the same for
                          every batching of the same images -- conv_splitk_for)
    gpurun_out/tile_table_splitk.h   tile-table lines for the (shape, S) winners, to be merged into csrc/tile_table.h

A split changes the fp32 summation order of a layer (an equally valid draw): re-record tests/golden/parity_floors.json
after changing the table.

    python tools/tune_splitk.py [--max-px 2048] [--streams S] B,H,W [B,H,W ...]     (default 4,512,640)
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import rgbd_amd  # noqa: E402
from rgbd_amd import synth  # noqa: E402
from rgbd_amd._lib import lib  # noqa: E402

argv = sys.argv[1:]


def opt(name, default, cast=int):
    if name in argv:
        v = cast(argv[argv.index(name) + 1])
        del argv[argv.index(name):argv.index(name) + 2]
        return v
    return default


MAX_PX = opt("--max-px", 2048)
STREAMS = opt("--streams", 1)
MODEL = opt("--model", "ELIC_united", str)
WORKLOADS = [tuple(int(v) for v in a.split(",")) for a in argv if not a.startswith("--")] or [(4, 512, 640)]
L = lib()
L.rgbd_debug_bench_streams(STREAMS)
os.environ["RGBD_NO_TILE_TABLE"] = "1"

sd = synth.synthetic_state_dict(0, model=MODEL)
net = rgbd_amd.modelZoo[MODEL](config=rgbd_amd.model_config(), channel=4).eval()
net.load_state_dict(sd)
net.update(force=True)
net = net.to("cuda")
net.per_image_streams = True

TILES = ([(2, m, 8) for m in (3, 2, 1)] + [(2, m, n) for n in (4, 2, 1) for m in (5, 4, 3, 2, 1)] +
         [(1, m, n) for n in (4, 2, 1) for m in (3, 2, 1)])
MODES = ((16, 1), (16, 2), (16, 3), (16, 0), (64, 0), (16, 4), (16, 5))  # 4 / 5: ring of 4 / 3 DMA stages (single-tap layers)
SPLITS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16)


def shapes(B, H, W):
    r, d = synth.synthetic_batch(B, H, W, config_id=2)
    rgb, depth = torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda()
    out = net.compress(rgb, depth)
    L.rgbd_debug_conv_log(1)
    out = net.compress(rgb, depth)
    net.decompress(out["r_strings"], out["d_strings"], out["shape"])
    L.rgbd_debug_conv_log(0)
    n = L.rgbd_debug_conv_log_read(None, 0)
    buf = ctypes.create_string_buffer(n)
    L.rgbd_debug_conv_log_read(buf, n)
    return [tuple(int(v) for v in ln.split(",")) for ln in buf.value.decode().strip().split("\n")[1:]]


def bench(key, iters):
    N, H, W, cin, cout, ntaps, stride, nphase, _ = key
    k = int(round(ntaps ** 0.5))
    ms = ctypes.c_float(0)
    L.rgbd_debug_force_ckbd(nphase // 10)
    nphase %= 10
    rc = L.rgbd_conv_bench(N, cin, H, W, cout, k, stride, k // 2, 1 if nphase > 1 else 0, 0, iters, ctypes.byref(ms))
    return ms.value if rc == 0 else float("inf")


split_of, tile_of = {}, {}
tot_now = tot_best = 0.0
for B, H, W in WORKLOADS:
    for row in shapes(B, H, W):
        key, cnt = row[:9], row[9]
        N, h, w, cin, cout, ntaps, stride, nphase, s_now = key
        oh, ow = (h * stride, w * stride) if nphase % 10 > 1 else (h // stride, w // stride)
        if oh * ow > MAX_PX or cin < 32:
            continue
        L.rgbd_debug_force_tile(b"")
        L.rgbd_debug_force_splitk(s_now)
        now = min(bench(key, 4), bench(key, 4))
        # phase 1: every split with the cost model's pick and a few representative tiles; phase 2: every tile at the best three
        coarse = {}
        for S in SPLITS:
            if S > cin // 16:
                continue
            L.rgbd_debug_force_splitk(S)
            L.rgbd_debug_force_tile(b"")
            t = bench(key, 3)
            for cfg in (b"2,2,4,16,1", b"2,4,4,16,1", b"2,3,2,16,1", b"1,3,4,16,1", b"2,2,2,16,2", b"2,2,2,64,0", b"2,4,4,16,4", b"2,2,4,16,4",
                        b"2,4,2,16,4"):
                L.rgbd_debug_force_tile(cfg)
                t = min(t, bench(key, 3))
            coarse[S] = t
        res = []
        for S in sorted(coarse, key=coarse.get)[:3] + ([s_now] if s_now in coarse else []):
            L.rgbd_debug_force_splitk(S)
            for wm, mt, nt in TILES:
                for kc, dma in MODES:
                    L.rgbd_debug_force_tile(f"{wm},{mt},{nt},{kc},{dma}".encode())
                    res.append((bench(key, 3), S, wm, mt, nt, kc, dma))
        res.sort()
        top = []
        for t, S, wm, mt, nt, kc, dma in res[:4]:
            L.rgbd_debug_force_splitk(S)
            L.rgbd_debug_force_tile(f"{wm},{mt},{nt},{kc},{dma}".encode())
            top.append((min(bench(key, 8), bench(key, 8)), S, wm, mt, nt, kc, dma))
        top.sort()
        best = top[0]
        # best with the CURRENT split (what a pure tile re-tune would give), for the record
        same = min((r for r in res if r[1] == s_now), default=(float("inf"),))
        tot_now += now * cnt
        tot_best += min(best[0], now) * cnt
        gkey = (oh * ow, cin, cout, ntaps, nphase % 10)
        if best[0] < now * 0.97:
            # one S per layer shape: the checkerboard and the full form of a layer, and every batch size, share it
            prev = split_of.get(gkey)
            if prev is None or best[0] * cnt > prev[1]:
                split_of[gkey] = (best[1], best[0] * cnt)
            tile_of[key[:8] + (best[1],)] = best[2:]
        print(f"{key} x{cnt:3d} now {now*1e3:8.1f} us (S={s_now}; best tile at that S {same[0]*1e3:8.1f}) -> {best[0]*1e3:8.1f} us "
              f"S={best[1]} tile {best[2:]}", flush=True)
L.rgbd_debug_force_tile(b"")
L.rgbd_debug_force_splitk(0)
L.rgbd_debug_force_ckbd(0)
print(f"total {tot_now:.3f} ms -> {tot_best:.3f} ms per enc+dec over the tuned shapes")
os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
with open(os.path.join(ROOT, "gpurun_out", "splitk_table.h"), "w") as f:
    f.write("// generated by tools/tune_splitk.py on MI355X -- measured split-K factors (conv_splitk_for)\n"
            "// out_px_per_image, cin_pad, cout_pad, ntaps, nphase,   S\n")
    for k, (S, _) in sorted(split_of.items()):
        f.write("{" + ", ".join(str(v) for v in k) + f",   {S}" + "},\n")
with open(os.path.join(ROOT, "gpurun_out", "tile_table_splitk.h"), "w") as f:
    for k, b in sorted(tile_of.items()):
        f.write("{" + ", ".join(str(v) for v in k) + ",   " + ", ".join(str(v) for v in b) + "},\n")
print("wrote gpurun_out/splitk_table.h, gpurun_out/tile_table_splitk.h")
