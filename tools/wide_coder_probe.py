#!/usr/bin/env python3
"""Wide rANS against the serial coder, in one process on one GPU.

Part 1: ns/symbol of the four kernels (serial / wide encode and decode, wide at L = 16 and L = 64) on the probe classes of
tools/coder_probe.py, one stream of N symbols resident in HBM, device events around REPS launches after a warm-up.
Part 2: B = 1 compress() / decompress() of a 512x640 pair with the stress and the trained-like weights (tools/latency_b1.py's
calling pattern), the coders alternating in blocks.
Usage: python3 tools/wide_coder_probe.py [N] [out.txt]"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import rgbd_amd  # noqa: E402
from rgbd_amd import ELIC_united, ans, synth  # noqa: E402
from rgbd_amd._lib import check, lib  # noqa: E402
from rgbd_amd.entropy_models import GaussianConditional, get_scale_table  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
OUT = sys.argv[2] if len(sys.argv) > 2 else None
WARM, REPS = 2, 5
LINES = []


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    LINES.append(line)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def timed(fn):
    """ms per call: device events around REPS calls after WARM."""
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def kernels():
    L = lib()
    gc = GaussianConditional()
    gc.update_scale_table(get_scale_table(), force=True)
    cdf, sizes, offsets = gc.numpy_tables()
    t = ans.Tables(cdf, sizes, offsets)
    rng = np.random.default_rng(0)
    scales = np.exp(np.linspace(np.log(0.11), np.log(256), 64))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dev(np.zeros(1, np.int64))
    err = torch.zeros(64, dtype=torch.int32, device="cuda")
    say(f"# kernels: one stream of N = {N} symbols, ns/symbol (ms per launch * 1e6 / N), {REPS} launches after {WARM}")
    say("class            rows      serial_enc serial_dec | wide16_enc wide16_dec | wide64_enc wide64_dec | bytes serial/w16/w64")
    for name, lo, hi, gain in (("idx0-7", 0, 8, 1.0), ("idx16-23", 16, 24, 1.0), ("idx32-39", 32, 40, 1.0), ("idx48-55", 48, 56, 1.0),
                               ("idx0-63", 0, 64, 1.0), ("stress-like", 0, 40, 3.0), ("zeros", 0, 4, 0.0)):
        idx = rng.integers(lo, hi, N).astype(np.int32)
        sym = np.rint(rng.normal(0.0, 1.0, N) * scales[idx] * gain).astype(np.int32)
        d_sym, d_idx = dev(np.concatenate([sym, [0]]).astype(np.int32)), dev(np.concatenate([idx, [0]]).astype(np.int32))
        out_sym = torch.zeros(N, dtype=torch.int32, device="cuda")
        cnt = dev(np.array([N], np.int64))
        ow = torch.zeros(1, dtype=torch.int64, device="cuda")
        res, nbytes = [], []
        # serial
        cap = int(L.rgbd_rans_max_bytes(N)) // 4
        words = torch.zeros(cap, dtype=torch.int32, device="cuda")
        res.append(timed(lambda: check(L.rgbd_rans_encode_batch_dev(t.handle, d_sym.data_ptr(), d_idx.data_ptr(), base.data_ptr(),
                                                                    cnt.data_ptr(), 1, words.data_ptr(), cap, ow.data_ptr(),
                                                                    err.data_ptr(), stream), "enc")))
        nw = int(ow.item())
        off, ln = dev(np.array([cap - nw], np.int64)), dev(np.array([nw], np.int64))
        state = torch.zeros(2, dtype=torch.int64, device="cuda")
        res.append(timed(lambda: check(L.rgbd_rans_decode_batch_dev(t.handle, words.data_ptr(), off.data_ptr(), ln.data_ptr(), 1,
                                                                    state.data_ptr(), 1, d_idx.data_ptr(), out_sym.data_ptr(),
                                                                    base.data_ptr(), 0, N, stream), "dec")))
        assert np.array_equal(out_sym.cpu().numpy(), sym), name
        nbytes.append(4 * nw)
        for lanes in (16, 64):
            capw = int(L.rgbd_rans_wide_max_bytes(N, lanes)) // 4
            wwords = torch.zeros(capw, dtype=torch.int32, device="cuda")
            seg = (ctypes.c_int64 * 1)(N)
            res.append(timed(lambda: check(L.rgbd_rans_wide_encode_batch_dev(t.handle, t.handle, 1, d_sym.data_ptr(), d_idx.data_ptr(),
                                                                             base.data_ptr(), 1, lanes, seg, 1, wwords.data_ptr(), capw,
                                                                             ow.data_ptr(), err.data_ptr(), stream), "wenc")))
            nw = int(ow.item())
            off, ln = dev(np.array([capw - nw], np.int64)), dev(np.array([nw], np.int64))
            wstate = torch.zeros(lanes + 1, dtype=torch.int64, device="cuda")
            out_sym.zero_()
            res.append(timed(lambda: check(L.rgbd_rans_wide_decode_batch_dev(t.handle, wwords.data_ptr(), off.data_ptr(), ln.data_ptr(),
                                                                             1, lanes, wstate.data_ptr(), 1, d_idx.data_ptr(),
                                                                             out_sym.data_ptr(), base.data_ptr(), 0, N, err.data_ptr(),
                                                                             stream), "wdec")))
            assert np.array_equal(out_sym.cpu().numpy(), sym), (name, lanes)
            nbytes.append(4 * nw)
        assert int(err.sum().item()) == 0
        ns = [v * 1e6 / N for v in res]
        say(f"{name:<16} {sizes[lo:hi].min():>4}-{sizes[lo:hi].max():<4} {ns[0]:>10.2f} {ns[1]:>10.2f} | {ns[2]:>10.2f} {ns[3]:>10.2f} |"
            f" {ns[4]:>10.2f} {ns[5]:>10.2f} | {nbytes[0]}/{nbytes[1]}/{nbytes[2]}")


def latency(recipe, H=512, W=640):
    net = ELIC_united(config=rgbd_amd.model_config(), channel=4).eval()
    net.load_state_dict(synth.synthetic_state_dict(0, recipe=recipe))
    net.update(force=True)
    net = net.to("cuda")
    r, d = synth.synthetic_batch(1, H, W, config_id=2)
    rgb, depth = torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda()
    coders = (("reference", 64), ("wide", 64), ("wide", 16))
    enc, dec, size = {c: [] for c in coders}, {c: [] for c in coders}, {}
    for block in range(2):
        for c in coders:
            net.set_coder(*c)
            for _ in range(3):  # eager, captured, replayed
                out = net.compress(rgb, depth)
                net.decompress(out["r_strings"], out["d_strings"], out["shape"])
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = net.compress(rgb, depth)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                net.decompress(out["r_strings"], out["d_strings"], out["shape"])
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                enc[c].append((t1 - t0) * 1e3)
                dec[c].append((t2 - t1) * 1e3)
            size[c] = len(out["r_strings"][0][0]) + len(out["d_strings"][0][0])
    for c in coders:
        say(f"B=1 {H}x{W} {recipe:<12} {c[0]:>9} L={c[1]:<2}: enc median {np.median(enc[c]):7.2f} ms (min {min(enc[c]):7.2f})  "
            f"dec median {np.median(dec[c]):7.2f} ms (min {min(dec[c]):7.2f})  y bytes {size[c]}")


if __name__ == "__main__":
    kernels()
    say(f"# B = 1 latency, coders alternating in two blocks of 5 timed calls each (after 3 warm-up calls per block)")
    for recipe in ("stress", "trained_like"):
        latency(recipe)
    if OUT:
        with open(OUT, "w") as f:
            f.write("\n".join(LINES) + "\n")
