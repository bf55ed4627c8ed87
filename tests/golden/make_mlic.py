#!/usr/bin/env python3
"""Generate the MLIC++ ("MLIC") fixtures by RUNNING THE UNMODIFIED REFERENCE (models/mlicpp.py: MLICPlusPlus) on the CPU.

    make -C oracle ref && python tests/golden/make_mlic.py [case ...]

Writes tests/golden/mlic_<case>.npz (read by tests/test_mlic_cpu.py and tests/test_gpu_mlic.py, as is tests/golden/mlic_floors.json,
which a recording run of the latter on the GPU writes: RGBD_RECORD_MLIC_FLOORS=<path>; data only: streams, the reference's symbols / indexes in stream order, per symbol its
y - mean and scale as float32, the z symbols, a sub-sample and the sha of y and of y_hat, sha / PSNR of decompress()'s x_hat,
summed -log2 likelihoods of forward()) and tests/golden/mlic_keys.json (the reference's state_dict names, shapes and parameter
count at the model's own widths).  Weights and images are regenerated from rgbd_amd.synth, never stored.

Next to the reference's own numbers each file holds what the fp64 restatement (tests/mlic_ref.py, dtype float64) gives under the
reference's symbols (teacher forcing, so that both see the same contexts): per symbol y - mean and scale (`x64`, `sigma64`: the
census' distances to the rounding and scale-bin boundaries), the sub-samples of y and y_hat, `e_ref_y` / `e_ref_yhat` /
`e_ref_x` / `e_ref_sigma` = max |reference fp32 - fp64| / max |fp64| of those tensors (the unit of the GPU tests' float bound),
the fp64 likelihood sums (`lik_y_bits64`, `lik_z_bits64`) and `lik_y_gap` / `lik_z_gap` = sum |bits fp32 - bits fp64| over the
elements / sum of the fp64 bits: the reference's own fp32 - fp64 gap in forward(), element by element (a signed difference of
the sums would measure cancellation), which is the unit of the GPU tests' forward tolerance.

The reference is observed, not changed: the symbols it hands its encoder are recorded by a delegating stand-in for
BufferedRansEncoder, the floats behind them by delegating wrappers around its GaussianConditional's quantize() /
build_indexes(), tensors by forward hooks.  The generator ASSERTS the fixture conditions on the reference alone: every part
(slice x checkerboard half) has >= 30 % non-zero symbols and >= 4 distinct scale indexes; >= 0.1 % escape symbols over the
stream; >= 50 % non-zero z symbols; in every GDN / IGDN layer max (norm - beta) / beta >= 1; every LRP's tanh sees a largest
|x| in 0.8 ... 3.2; every GELU sees arguments below -1 and above +1; at most 0.5 % of the decisions lie inside the
near-boundary windows of make_margins.py (ROUND_WINDOW = SCALE_WINDOW = 2e-4).

The two cases of LRP_BULK (s2_448x192, s2_b2_192x128: the weights of s2_128x128 on a 28x12 and a 2 x 12x8 latent grid) replace
the LRP condition, and only that one.  The band on the largest |x| is tuned to the 8x8 map, most of which is border: with the
seed-3 weights the largest |x| per LRP is 1.67 ... 2.10 at 128x128, 2.61 ... 3.54 at 2x192x128 and 5.39 ... 9.62 at 448x192, so no
weight set meets the band at both 128x128 and 448x192, and the three s2 cases have to share one weight set (one model across
shapes).  What the band is there for -- the tanh neither linear nor saturated over what it sees -- is asked of the bulk of the
values instead: in every LRP at least 85 % of the pre-tanh values have |x| <= 3.2 and at least 10 % have |x| >= 0.8 (the hook
keeps the values, not only their maximum; the shares are printed for every case).  The three older cases keep the maximum band.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _reference_loader as rl  # noqa: E402

ROUND_WINDOW = 2e-4  # make_margins.py: |distance to .5| <= ROUND_WINDOW * max(1, |y - mean|)
SCALE_WINDOW = 2e-4  # |scale / table_entry - 1| <= SCALE_WINDOW

# name -> (N, M, slice_num, B, H, W, image config id, weight seed)
CASES = {"s2_128x128": (64, 64, 2, 1, 128, 128, 81, 3), "s3_b2_128x192": (64, 96, 3, 2, 128, 192, 82, 4),
         "full_128x128": (192, 320, 10, 1, 128, 128, 83, 5),
         # the weights of s2_128x128 at two more shapes (tests/test_gpu_mlic.py runs one model across the three)
         "s2_448x192": (64, 64, 2, 1, 448, 192, 84, 3), "s2_b2_192x128": (64, 64, 2, 2, 192, 128, 85, 3)}
LRP_BULK = {"s2_448x192", "s2_b2_192x128"}  # the LRP condition on the share of the values, not on the largest (docstring)
LRP_BULK_BELOW, LRP_BULK_ABOVE = 0.85, 0.10  # share of the pre-tanh values with |x| <= 3.2, with |x| >= 0.8


def sha_f32(t) -> str:
    return hashlib.sha256(np.ascontiguousarray(np.asarray(t, np.float32)).tobytes()).hexdigest()[:16]


def y_sub(y):  # every 8th channel (four per slice), every other row and column
    return y[:, ::8, ::2, ::2]


def near_boundary(x, s, table):
    m_round = 0.5 - np.abs(x - np.rint(x))
    rel = np.abs(s[:, None] / table[None, :-1] - 1.0).min(axis=1)
    return (m_round <= ROUND_WINDOW * np.maximum(1.0, np.abs(x))) | (rel <= SCALE_WINDOW)


def rel_err(a, ref64):
    a, ref64 = np.asarray(a, np.float64), np.asarray(ref64, np.float64)
    return float(np.abs(a - ref64).max() / np.abs(ref64).max())


class _Recorder:
    """Stands in for compressai.ans.BufferedRansEncoder inside models/mlicpp.py: records, then delegates."""
    calls = []
    real = None

    def __init__(self):
        self._e = _Recorder.real()

    def encode_with_indexes(self, symbols, indexes, *tables):
        _Recorder.calls.append((np.asarray(symbols, np.int32), np.asarray(indexes, np.int32)))
        return self._e.encode_with_indexes(symbols, indexes, *tables)

    def flush(self):
        return self._e.flush()


def reference_net(mod, N, M, slice_num, channel=3):
    from utils.IOutils import Config

    return mod.MLICPlusPlus(Config({"N": N, "M": M, "slice_num": slice_num, "context_window": 5}), channel=channel).eval()


def case(mod, synth, name, N, M, S, B, H, W, config_id, seed):
    import mlic_ref

    net = reference_net(mod, N, M, S)
    sd = synth.synthetic_state_dict(seed, model="MLIC", N=N, M=M)
    net.load_state_dict(sd)
    assert net.update(force=True)
    r, _ = synth.synthetic_batch(B, H, W, config_id=config_id)
    x = torch.from_numpy(r)
    seen, gdn_ratio, gelu_range, pretanh, pretanh_all, floats = {}, {}, {}, {}, {}, {"x": [], "s": []}
    hooks = [net.h_a.register_forward_hook(lambda m, i, o: seen.update(y=i[0].detach().clone(), z=o.detach().clone())),
             net.g_s.register_forward_hook(lambda m, i, o: seen.update(yhat=i[0].detach().clone()))]

    def gdn_hook(label):
        def fn(m, i, o):
            xin = i[0].detach()
            n = xin.shape[1]
            beta, gamma = m.beta_reparam(m.beta).detach(), m.gamma_reparam(m.gamma).detach()
            norm = F.conv2d(xin ** 2, gamma.reshape(n, n, 1, 1), beta)
            ratio = float(((norm - beta.view(1, -1, 1, 1)) / beta.view(1, -1, 1, 1)).max())
            gdn_ratio[label] = max(gdn_ratio.get(label, 0.0), ratio)
        return fn

    def gelu_hook(label):
        def fn(m, i):
            lo, hi = gelu_range.get(label, (0.0, 0.0))
            gelu_range[label] = (min(lo, float(i[0].min())), max(hi, float(i[0].max())))
        return fn

    def lrp_hook(label):
        def fn(m, i, o):
            pretanh[label] = max(pretanh.get(label, 0.0), float(o.detach().abs().max()))
            pretanh_all.setdefault(label, []).append(o.detach().abs().reshape(-1).numpy().copy())
        return fn

    for label, m in net.named_modules():
        if type(m).__name__ == "GDN":
            hooks.append(m.register_forward_hook(gdn_hook(label)))
        elif isinstance(m, torch.nn.GELU):
            hooks.append(m.register_forward_pre_hook(gelu_hook(label)))
        elif label.endswith(".lrp_transform"):
            hooks.append(m.register_forward_hook(lrp_hook(label)))
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
    assert "cost_time" in out
    sym, idx = _Recorder.calls[0]
    xs, ss = np.concatenate(floats["x"]).astype(np.float32), np.concatenate(floats["s"]).astype(np.float32)
    h, w = H // 16, W // 16
    assert sym.size == B * M * h * w == xs.size == ss.size
    assert np.array_equal(np.rint(xs).astype(np.int32), sym)
    with torch.no_grad():
        dec = net.decompress(out["strings"], out["shape"])
        yhat = seen["yhat"].clone()
        fw = net(x)
    for hk in hooks:
        hk.remove()
    # ---- fixture conditions, on the reference alone
    lens, offs = gc._cdf_length.numpy(), gc._offset.numpy()
    v = sym - offs[idx]
    esc = float(np.mean((v < 0) | (v >= lens[idx] - 2)))
    part = B * 32 * h * (w // 2)
    stats = []
    for i in range(2 * S):
        s, k = sym[i * part:(i + 1) * part], idx[i * part:(i + 1) * part]
        stats.append((float(np.mean(s != 0)), int(np.abs(s).max()), int(np.unique(k).size)))
    med = net.entropy_bottleneck._get_medians().detach()
    zsym = torch.round(seen["z"] - med).to(torch.int32)
    znz = float((zsym != 0).float().mean())
    table = gc.scale_table.numpy().astype(np.float32)
    near = float(near_boundary(xs, ss, table).mean())
    nbytes = len(out["strings"][0][0]) + sum(len(s) for s in out["strings"][1])
    print(f"MLIC {name}: y {len(out['strings'][0][0])} B, z {[len(s) for s in out['strings'][1]]} B, {nbytes * 8 / (B * H * W):.2f} bpp, "
          f"escapes {100 * esc:.2f} %, z non-zero {100 * znz:.0f} %, near-boundary {100 * near:.3f} %", flush=True)
    print("   parts (non-zero %, max |s|, scale indexes):", [(round(100 * a), b, c) for a, b, c in stats])
    print("   GDN max (norm - beta) / beta:", {k.split("transform.")[1]: round(v, 2) for k, v in gdn_ratio.items()})
    print("   LRP max |x| in front of tanh:", {k[:-len(".lrp_transform")]: round(v, 2) for k, v in pretanh.items()})
    lrp_share = {k: (float(np.mean(np.concatenate(v) <= 3.2)), float(np.mean(np.concatenate(v) >= 0.8))) for k, v in pretanh_all.items()}
    print("   LRP share of the pre-tanh values with |x| <= 3.2, |x| >= 0.8 (%):",
          {k[:-len(".lrp_transform")]: (round(100 * lo, 2), round(100 * hi, 2)) for k, (lo, hi) in lrp_share.items()})
    g_lo, g_hi = max(lo for lo, hi in gelu_range.values()), min(hi for lo, hi in gelu_range.values())
    print(f"   GELU arguments over {len(gelu_range)} modules: every minimum <= {g_lo:.2f}, every maximum >= {g_hi:.2f}", flush=True)
    for i, st in enumerate(stats):
        assert st[0] >= 0.3 and st[2] >= 4, (name, i, st)
    assert esc >= 0.001, (name, esc)
    assert znz >= 0.5, (name, znz)
    assert len(gdn_ratio) == 6 and min(gdn_ratio.values()) >= 1.0, (name, gdn_ratio)
    if name in LRP_BULK:
        assert len(lrp_share) == 2 * S, (name, lrp_share)
        assert all(lo >= LRP_BULK_BELOW and hi >= LRP_BULK_ABOVE for lo, hi in lrp_share.values()), (name, lrp_share)
    else:
        assert len(pretanh) == 2 * S and all(0.8 <= t <= 3.2 for t in pretanh.values()), (name, pretanh)
    assert g_lo < -1.0 and g_hi > 1.0, (name, {k: v for k, v in gelu_range.items() if v[0] >= -1.0 or v[1] <= 1.0})
    assert near <= 0.005, (name, near)
    assert np.abs(sym).max() < 32768 and idx.max() < 128 and int(zsym.abs().max()) < 32768
    # ---- the fp64 restatement under the reference's symbols
    ref64 = mlic_ref.MlicRef(sd, dtype=torch.float64)
    ref64.update()
    ref64.trace = {}
    ref64.compress(x, forced_y=sym, forced_z=zsym.numpy().reshape(-1))
    t64, ref64.trace = ref64.trace, None  # (forward() would write its own, free-running y_hat into the trace)
    fw64 = ref64.forward(x)
    e = {"y": rel_err(seen["y"], t64["y"]), "yhat": rel_err(yhat, t64["yhat"]), "x": rel_err(xs, t64["x"]),
         "sigma": rel_err(ss, t64["sigma"])}
    print("   reference fp32 against the fp64 restatement (max |d| / max |ref|):", {k: f"{v:.2e}" for k, v in e.items()}, flush=True)
    assert all(v < 1e-3 for v in e.values()), (name, e)  # the restatement restates this model
    psnr = -10 * np.log10(torch.mean((dec["x_hat"] - x) ** 2).item())
    bits = lambda t: np.float64(-torch.log2(t.double()).sum().item())  # noqa: E731

    def gap(k):
        a, b = -torch.log2(fw["likelihoods"][k].double()), -torch.log2(fw64["likelihoods"][k].double())
        return np.float64(((a - b).abs().sum() / b.sum()).item())

    print(f"   forward(): fp32 - fp64 gap of the likelihood bits, y {gap('y_likelihoods'):.2e}, z {gap('z_likelihoods'):.2e}", flush=True)
    g = {"N": N, "M": M, "slice_num": S, "B": B, "H": H, "W": W, "config_id": config_id, "seed": seed,
         "shape": np.array(tuple(out["shape"]), np.int32), "y_stream": np.frombuffer(out["strings"][0][0], np.uint8),
         "symbols": sym.astype(np.int16), "indexes": idx.astype(np.int8), "x": xs, "sigma": ss,
         "x64": t64["x"].astype(np.float64), "sigma64": t64["sigma"].astype(np.float64),
         "z_symbols": zsym.numpy().astype(np.int16), "y_sub": y_sub(seen["y"]).numpy(), "y_sha": sha_f32(seen["y"]),
         "yhat_sub": y_sub(yhat).numpy(), "yhat_sha": sha_f32(yhat),
         "y_sub64": y_sub(t64["y"]).numpy(), "yhat_sub64": y_sub(t64["yhat"]).numpy(),
         "e_ref_y": np.float64(e["y"]), "e_ref_yhat": np.float64(e["yhat"]), "e_ref_x": np.float64(e["x"]),
         "e_ref_sigma": np.float64(e["sigma"]),
         "xhat_sha": sha_f32(dec["x_hat"]), "psnr": np.float64(psnr),
         "lik_y_bits": bits(fw["likelihoods"]["y_likelihoods"]), "lik_z_bits": bits(fw["likelihoods"]["z_likelihoods"]),
         "lik_y_bits64": bits(fw64["likelihoods"]["y_likelihoods"]), "lik_z_bits64": bits(fw64["likelihoods"]["z_likelihoods"]),
         "lik_y_gap": gap("y_likelihoods"), "lik_z_gap": gap("z_likelihoods"), "fw_xhat_sha": sha_f32(fw["x_hat"])}
    for i, s in enumerate(out["strings"][1]):
        g[f"z{i}"] = np.frombuffer(s, np.uint8)
    path = os.path.join(HERE, f"mlic_{name}.npz")
    np.savez_compressed(path, **g)
    print(f"   {os.path.basename(path)}: {os.path.getsize(path)} bytes", flush=True)
    assert os.path.getsize(path) <= 1 << 20


def main():
    rl.load_reference()
    import models.mlicpp as mod

    import rgbd_amd.synth as synth

    torch.manual_seed(0)
    _Recorder.real = mod.BufferedRansEncoder
    mod.BufferedRansEncoder = _Recorder
    only = sys.argv[1:] or list(CASES)
    for name in only:
        case(mod, synth, name, *CASES[name])
    if len(only) == len(CASES):
        net = reference_net(mod, 192, 320, 10)
        keys = {k: list(v.shape) for k, v in net.state_dict().items()}
        with open(os.path.join(HERE, "mlic_keys.json"), "w") as f:
            json.dump({"N": 192, "M": 320, "slice_num": 10, "channel": 3, "n_tensors": len(keys),
                       "n_parameters": int(sum(p.numel() for p in net.parameters())), "keys": keys}, f, indent=0, sort_keys=False)
            f.write("\n")
        print("state_dict tensors:", len(keys))


if __name__ == "__main__":
    main()
