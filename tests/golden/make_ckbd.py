#!/usr/bin/env python3
"""Generate the checkerboard Cheng2020 ("ckbd") fixtures by RUNNING THE UNMODIFIED REFERENCE
(models/Cheng2020withCKBD.py: Cheng2020AnchorwithCheckerboard).

    make -C oracle ref && python tests/golden/make_ckbd.py

Writes tests/golden/ckbd_*.npz (data only: streams, the reference's symbols / indexes in stream order, per symbol its
y - mean and scale as float32, the z symbols, a sub-sample and the sha of the latents, sha / PSNR of decompress()'s x_hat --
and the tensor itself when it is at most 64x128x3 --, summed -log2 likelihoods of forward() and the sha of its x_hat) and
tests/golden/ckbd_keys.json (the reference's state_dict names, shapes and parameter count).  Weights and images are
regenerated from rgbd_amd.synth, never stored.

The reference is observed, not changed: the symbols it hands its encoder are recorded by a delegating stand-in for
BufferedRansEncoder, the floats behind them by delegating wrappers around its GaussianConditional's quantize() /
build_indexes(), tensors by forward hooks.  The generator ASSERTS the fixture conditions on the reference alone: each
checkerboard half has >= 50 % non-zero symbols and >= 8 distinct scale indexes; >= 0.1 % escape symbols; >= 50 % non-zero z
symbols; in every GDN / IGDN layer max (norm - beta) / beta >= 1; at most 0.5 % of the decisions lie inside the
near-boundary windows of make_margins.py (ROUND_WINDOW = SCALE_WINDOW = 2e-4).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import _reference_loader as rl  # noqa: E402

ROUND_WINDOW = 2e-4  # make_margins.py: |distance to .5| <= ROUND_WINDOW * max(1, |y - mean|)
SCALE_WINDOW = 2e-4  # |scale / table_entry - 1| <= SCALE_WINDOW

# name -> (N, channel, B, H, W, image config id, weight seed)
CASES = {"a_64x128": (192, 3, 1, 64, 128, 71, 0), "b_b2_128x64_d": (192, 1, 2, 128, 64, 72, 5),
         "c_128x192_n128": (128, 3, 1, 128, 192, 73, 7)}


def sha_f32(t) -> str:
    return hashlib.sha256(np.ascontiguousarray(np.asarray(t, np.float32)).tobytes()).hexdigest()[:16]


def y_sub(y):  # every 12th channel, every other row and column
    return y[:, ::12, ::2, ::2]


def near_boundary(x, s, table):
    m_round = 0.5 - np.abs(x - np.rint(x))
    rel = np.abs(s[:, None] / table[None, :-1] - 1.0).min(axis=1)
    return (m_round <= ROUND_WINDOW * np.maximum(1.0, np.abs(x))) | (rel <= SCALE_WINDOW)


class _Recorder:
    """Stands in for compressai.ans.BufferedRansEncoder inside models/Cheng2020withCKBD.py: records, then delegates."""
    calls = []
    real = None

    def __init__(self):
        self._e = _Recorder.real()

    def encode_with_indexes(self, symbols, indexes, *tables):
        _Recorder.calls.append((np.asarray(symbols, np.int32), np.asarray(indexes, np.int32)))
        return self._e.encode_with_indexes(symbols, indexes, *tables)

    def flush(self):
        return self._e.flush()


def case(mod, synth, name, N, channel, B, H, W, config_id, seed):
    net = mod.Cheng2020AnchorwithCheckerboard(N=N, channel=channel).eval()
    net.load_state_dict(synth.synthetic_state_dict(seed, model="ckbd", N=N, channel=channel))
    assert net.update(force=True)
    r, d = synth.synthetic_batch(B, H, W, config_id=config_id)
    x = torch.from_numpy(r if channel == 3 else d)
    seen, gdn_ratio, floats = {}, {}, {"x": [], "s": []}
    hooks = [net.h_a.register_forward_hook(lambda m, i, o: seen.update(y=i[0].detach().clone(), z=o.detach().clone()))]

    def gdn_hook(label):
        def fn(m, i, o):
            xin = i[0].detach()
            C = xin.shape[1]
            beta, gamma = m.beta_reparam(m.beta).detach(), m.gamma_reparam(m.gamma).detach()
            norm = F.conv2d(xin ** 2, gamma.reshape(C, C, 1, 1), beta)
            ratio = float(((norm - beta.view(1, -1, 1, 1)) / beta.view(1, -1, 1, 1)).max())
            gdn_ratio[label] = max(gdn_ratio.get(label, 0.0), ratio)
        return fn

    for label, m in net.named_modules():
        if type(m).__name__ == "GDN":
            hooks.append(m.register_forward_hook(gdn_hook(label)))
    gc = net.gaussian_conditional
    q_real, b_real = gc.quantize, gc.build_indexes

    def quantize(inputs, mode, means=None):  # observes the encoder's (inputs - means), delegates
        if mode == "symbols":
            floats["x"].append((inputs - means).detach().reshape(-1).numpy().copy())
        return q_real(inputs, mode, means)

    def build_indexes(scales):
        floats["s"].append(scales.detach().reshape(-1).numpy().copy())
        return b_real(scales)

    _Recorder.calls = []
    gc.quantize, gc.build_indexes = quantize, build_indexes
    with torch.no_grad():
        out = net.compress(x)
    del gc.quantize, gc.build_indexes  # (instance attributes: the class's methods are back)
    assert len(_Recorder.calls) == 1 and len(out["strings"][0]) == 1 and len(out["strings"][1]) == B
    sym, idx = _Recorder.calls[0]
    xs, ss = np.concatenate(floats["x"]).astype(np.float32), np.concatenate(floats["s"]).astype(np.float32)
    h, w = H // 16, W // 16
    assert sym.size == B * N * h * w == xs.size == ss.size
    assert np.array_equal(np.rint(xs).astype(np.int32), sym)
    with torch.no_grad():
        fw = net(x)
        dec = net.decompress(out["strings"], out["shape"])
    for hk in hooks:
        hk.remove()
    # ---- fixture conditions
    lens, offs = gc._cdf_length.numpy(), gc._offset.numpy()
    v = sym - offs[idx]
    esc = float(np.mean((v < 0) | (v >= lens[idx] - 2)))
    half = sym.size // 2
    stats = []
    for i in range(2):
        s, k = sym[i * half:(i + 1) * half], idx[i * half:(i + 1) * half]
        stats.append((float(np.mean(s != 0)), int(np.abs(s).max()), int(np.unique(k).size)))
    med = net.entropy_bottleneck._get_medians().detach()
    zsym = torch.round(seen["z"] - med).to(torch.int32)
    znz = float((zsym != 0).float().mean())
    table = gc.scale_table.numpy().astype(np.float32)
    near = float(near_boundary(xs, ss, table).mean())
    nbytes = len(out["strings"][0][0]) + sum(len(s) for s in out["strings"][1])
    print(f"ckbd {name}: y {len(out['strings'][0][0])} B, z {[len(s) for s in out['strings'][1]]} B, {nbytes * 8 / (B * H * W):.2f} bpp, "
          f"escapes {100 * esc:.2f} %, z non-zero {100 * znz:.0f} %, near-boundary {100 * near:.3f} %")
    for i, st in enumerate(stats):
        print(f"   {'anchor' if i == 0 else 'non-anchor'}: non-zero {100 * st[0]:.0f} %, max |s| {st[1]}, scale indexes {st[2]}")
    print("   GDN max (norm - beta) / beta:", {k: round(v, 2) for k, v in gdn_ratio.items()})
    for i, st in enumerate(stats):
        assert st[0] >= 0.5 and st[2] >= 8, (name, i, st)
    assert znz >= 0.5, (name, znz)
    assert esc >= 0.001, (name, esc)
    assert len(gdn_ratio) == 6 and min(gdn_ratio.values()) >= 1.0, (name, gdn_ratio)
    assert near <= 0.005, (name, near)
    assert np.abs(sym).max() < 32768 and idx.max() < 128 and int(zsym.abs().max()) < 32768
    psnr = -10 * np.log10(torch.mean((dec["x_hat"] - x) ** 2).item())
    g = {"N": N, "channel": channel, "B": B, "H": H, "W": W, "config_id": config_id, "seed": seed,
         "shape": np.array(tuple(out["shape"]), np.int32), "y_stream": np.frombuffer(out["strings"][0][0], np.uint8),
         "symbols": sym.astype(np.int16), "indexes": idx.astype(np.int8), "x": xs, "sigma": ss,
         "z_symbols": zsym.numpy().astype(np.int16), "y_sub": y_sub(seen["y"]).numpy(), "y_sha": sha_f32(seen["y"]),
         "xhat_sha": sha_f32(dec["x_hat"]), "psnr": np.float64(psnr),
         "lik_y_bits": np.float64(-torch.log2(fw["likelihoods"]["y"].double()).sum().item()),
         "lik_z_bits": np.float64(-torch.log2(fw["likelihoods"]["z"].double()).sum().item()),
         "fw_xhat_sha": sha_f32(fw["x_hat"])}
    for i, s in enumerate(out["strings"][1]):
        g[f"z{i}"] = np.frombuffer(s, np.uint8)
    if dec["x_hat"].numel() <= 64 * 128 * 3:
        g["xhat"] = dec["x_hat"].numpy()
    np.savez_compressed(os.path.join(HERE, f"ckbd_{name}.npz"), **g)
    return net


def main():
    rl.load_reference()
    import models.Cheng2020withCKBD as mod

    import rgbd_amd.synth as synth

    torch.manual_seed(0)
    _Recorder.real = mod.BufferedRansEncoder
    mod.BufferedRansEncoder = _Recorder
    only = sys.argv[1:] or list(CASES)
    for name in only:
        case(mod, synth, name, *CASES[name])
    if len(only) == len(CASES):
        net = mod.Cheng2020AnchorwithCheckerboard(N=192, channel=3)
        keys = {k: list(v.shape) for k, v in net.state_dict().items()}
        with open(os.path.join(HERE, "ckbd_keys.json"), "w") as f:
            json.dump({"N": 192, "channel": 3, "n_tensors": len(keys),
                       "n_parameters": int(sum(p.numel() for p in net.parameters())), "keys": keys}, f, indent=0, sort_keys=False)
            f.write("\n")
        print("state_dict tensors:", len(keys))


if __name__ == "__main__":
    main()
