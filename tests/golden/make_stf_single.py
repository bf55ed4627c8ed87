#!/usr/bin/env python3
"""Generate the single-modal STF fixtures by RUNNING THE UNMODIFIED REFERENCE (models/stf.py: SymmetricalTransFormer).

    make -C oracle ref && python tests/golden/make_stf_single.py

Writes tests/golden/stf1_*.npz (data only: streams, the reference's symbols / indexes in stream order, a sub-sample and the
sha of the latents, sha and PSNR of x_hat, summed -log2 likelihoods of forward()) and tests/golden/stf1_keys.json (the
reference's state_dict names and shapes).  Weights and images are regenerated from rgbd_amd.synth, never stored.

The reference is observed, not changed: the symbols it hands its encoder are recorded by a delegating stand-in for
BufferedRansEncoder, tensors by forward hooks.  The generator ASSERTS the fixture conditions (every slice of every fixture:
>= 50 % non-zero symbols, >= 8 distinct scale indexes, max |0.5 tanh(lrp)| >= 0.1; >= 50 % non-zero z symbols; >= 0.1 %
escape symbols; decompress(compress(x)) == forward(x).x_hat.clamp(0, 1)).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import _reference_loader as rl  # noqa: E402

# name -> (B, H, W, image config id, weight seed)
CASES = {"a_128x192": (1, 128, 192, 61, 0), "b_256x256": (1, 256, 256, 62, 5), "c_b2_192x128": (2, 192, 128, 63, 0)}


def sha_f32(t) -> str:
    return hashlib.sha256(np.ascontiguousarray(np.asarray(t, np.float32)).tobytes()).hexdigest()[:16]


def y_sub(y):  # as the held-out STF_united goldens: every 24th channel, every other row and column
    return y[:, ::24, ::2, ::2]


class _Recorder:
    """Stands in for compressai.ans.BufferedRansEncoder inside models/stf.py: records what it is given, delegates."""
    calls = []
    real = None

    def __init__(self):
        self._e = _Recorder.real()

    def encode_with_indexes(self, symbols, indexes, *tables):
        _Recorder.calls.append((np.asarray(symbols, np.int32), np.asarray(indexes, np.int32)))
        return self._e.encode_with_indexes(symbols, indexes, *tables)

    def flush(self):
        return self._e.flush()


def case(stf_mod, synth, name, B, H, W, config_id, seed):
    net = stf_mod.SymmetricalTransFormer().eval()
    net.load_state_dict(synth.synthetic_state_dict(seed, model="STF"))
    assert net.update(force=True)
    r, _ = synth.synthetic_batch(B, H, W, config_id=config_id)
    x = torch.from_numpy(r)
    seen = {"lrp": []}
    hooks = [net.h_a.register_forward_hook(lambda m, i, o: seen.update(y=i[0].detach().clone(), z=o.detach().clone()))]
    for t in net.lrp_transforms:
        hooks.append(t.register_forward_hook(lambda m, i, o: seen["lrp"].append(float((0.5 * torch.tanh(o)).abs().max()))))
    _Recorder.calls = []
    with torch.no_grad():
        out = net.compress(x)
    for h in hooks:
        h.remove()
    assert len(_Recorder.calls) == 1 and len(out["strings"][0]) == 1 and len(out["strings"][1]) == B
    sym, idx = _Recorder.calls[0]
    h, w = H // 16, W // 16
    assert sym.size == B * 384 * h * w
    with torch.no_grad():
        fw = net(x)
        dec = net.decompress(out["strings"], out["shape"]) if B == 1 else None
    # ---- fixture conditions
    gc = net.gaussian_conditional
    lens, offs = gc._cdf_length.numpy(), gc._offset.numpy()
    v = sym - offs[idx]
    esc = float(np.mean((v < 0) | (v >= lens[idx] - 2)))
    per = sym.size // 12
    stats = []
    for i in range(12):
        s, k = sym[i * per:(i + 1) * per], idx[i * per:(i + 1) * per]
        stats.append((float(np.mean(s != 0)), int(np.abs(s).max()), int(np.unique(k).size), seen["lrp"][i]))
        assert stats[-1][0] >= 0.5 and stats[-1][2] >= 8 and stats[-1][3] >= 0.1, (name, i, stats[-1])
    med = net.entropy_bottleneck._get_medians().detach()
    zsym = torch.round(seen["z"] - med)
    znz = float((zsym != 0).float().mean())
    assert znz >= 0.5, (name, znz)
    assert esc >= 0.001, (name, esc)
    if dec is not None:
        diff = float((dec["x_hat"] - fw["x_hat"].clamp(0, 1)).abs().max())
        assert diff == 0.0, (name, diff)
    nbytes = len(out["strings"][0][0]) + sum(len(s) for s in out["strings"][1])
    print(f"stf1 {name}: y {len(out['strings'][0][0])} B, z {[len(s) for s in out['strings'][1]]} B, {nbytes * 8 / (B * H * W):.2f} bpp, "
          f"escapes {100 * esc:.2f} %, z non-zero {100 * znz:.0f} %")
    for i, st in enumerate(stats):
        print(f"   slice {i:2d}: non-zero {100 * st[0]:.0f} %, max |s| {st[1]}, scale indexes {st[2]}, max lrp {st[3]:.3f}")
    assert np.abs(sym).max() < 32768 and idx.max() < 128
    g = {"B": B, "H": H, "W": W, "config_id": config_id, "seed": seed, "shape": np.array(tuple(out["shape"]), np.int32),
         "y_stream": np.frombuffer(out["strings"][0][0], np.uint8), "symbols": sym.astype(np.int16), "indexes": idx.astype(np.int8),
         "y_sub": y_sub(seen["y"]).numpy(), "y_sha": sha_f32(seen["y"]),
         "lik_y_bits": np.float64(-torch.log2(fw["likelihoods"]["y"].double()).sum().item()),
         "lik_z_bits": np.float64(-torch.log2(fw["likelihoods"]["z"].double()).sum().item()),
         "fw_xhat_sha": sha_f32(fw["x_hat"])}
    for i, s in enumerate(out["strings"][1]):
        g[f"z{i}"] = np.frombuffer(s, np.uint8)
    if dec is not None:
        g["xhat_sha"] = sha_f32(dec["x_hat"])
        g["psnr"] = np.float64(-10 * np.log10(torch.mean((dec["x_hat"] - x) ** 2).item()))
    else:  # the reference cannot decompress a batch (stf.py:799): PSNR of the clamped forward() reconstruction
        g["psnr"] = np.float64(-10 * np.log10(torch.mean((fw["x_hat"].clamp(0, 1) - x) ** 2).item()))
    np.savez_compressed(os.path.join(HERE, f"stf1_{name}.npz"), **g)
    return net


def main():
    rl.load_reference()
    import models.stf as stf_mod

    import rgbd_amd.synth as synth

    torch.manual_seed(0)
    _Recorder.real = stf_mod.BufferedRansEncoder
    stf_mod.BufferedRansEncoder = _Recorder
    net = None
    only = sys.argv[1:] or list(CASES)
    for name in only:
        net = case(stf_mod, synth, name, *CASES[name])
    sd = net.state_dict()
    keys = {k: list(v.shape) for k, v in sd.items()}
    if len(only) == len(CASES):
        with open(os.path.join(HERE, "stf1_keys.json"), "w") as f:
            json.dump({"n_tensors": len(keys), "n_parameters": int(sum(p.numel() for p in net.parameters())), "keys": keys}, f,
                      indent=0, sort_keys=False)
            f.write("\n")
    print("state_dict tensors:", len(keys))


if __name__ == "__main__":
    main()
