#!/usr/bin/env python3
"""Generate the fixtures of the latent codec of ELIC_master by RUNNING THE UNMODIFIED REFERENCE CLASS
(models/elic_master.py: ELIC_master) on the CPU, in fp32 and again in `.double()`.

    make -C oracle ref && python tests/golden/make_master_latent.py [case ...]

Writes tests/golden/master_latent_<case>.npz (read by tests/test_master_latent_cpu.py and tests/test_gpu_master_latent.py; cases,
seeded inputs and weights: tests/master_latent_cases.py) and tests/golden/master_state_dict.json ([name, shape] of the
reference's ELIC_master(config, channel = 3) and channel = 1, in its order).  tests/golden/master_latent_floors.json is written by
a recording run of the GPU test (RGBD_RECORD_MASTER_FLOORS=<path>), not here.  Data only; weights and inputs are regenerated
from seeds, never stored.

compress(), decompress() and forward() are called as they are.  The four outer blocks of the instance (aux_encoder,
master_encoder, channel_aligner, master_decoder) are replaced by pass-through callables, so that cat([fv, fv_bar]) is the seeded
f [B,128,H,W] and master_decoder returns the g_s half of cat([fv_bar, g_s(...)]) (:217-218, 379-380): what is recorded is
everything between those blocks.  The symbols the reference hands its encoder are recorded by a delegating stand-in for
BufferedRansEncoder, the floats behind them by delegating wrappers around its GaussianConditional's quantize() / build_indexes(),
tensors by forward hooks.

The fp64 run is the same class after .double(), with torch's default dtype set to float64 for its duration (utils/ckbd.py builds
its squeezed tensors with torch.zeros / torch.Tensor of the default dtype).  Its compress() runs under the fp32 run's symbols: the
quantize() wrapper records the fp64 y - mean and returns the fp32 run's symbols for that part (teacher forcing), so that both runs
see the same contexts and `x64`, `sigma64`, y_hat and f_hat are the fp64 values of the SAME decisions.  forward() runs free.

Per fixture: the y stream and z streams; `symbols`, `indexes`, `z_symbols`; `x64`, `sigma64` (stream order); y and y_hat of the
fp64 run at master_latent_cases.y_sub with their maxima; e_ref_y / e_ref_yhat / e_ref_x / e_ref_sigma / e_ref_fhat = max |fp32 -
fp64| / max |fp64| of those tensors (whole tensors); f_hat of the fp64 decompress() at master_latent_cases.fhat_positions with
`ref64_max`; the -log2 likelihood sums of forward() from both runs and their element-wise gap.

Conditions ASSERTED here, on the reference alone: 4 <= max |y| <= 64; at least 25 % of the y symbols non-zero; every slice has a
non-zero symbol in both checkerboard parts; the scale indexes use at least 16 table rows; the fp32 and fp64 runs give the same
z symbols; at most 1 % of the decisions lie within the float bound of a rounding boundary, and at most 1 % within that of a
scale-table entry (master_latent_cases.decision_bounds / boundary_distances), and none within the reference's own fp32 error
(an eighth of that bound) of either; and the restatement of master_latent_cases.py, in
float64 under the same symbols, reproduces the fp64 run to 1e-9.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _reference_loader as rl  # noqa: E402


class _Recorder:
    """Stands in for compressai.ans.BufferedRansEncoder inside models/elic_master.py: records, then delegates."""
    calls = []
    real = None

    def __init__(self):
        self._e = _Recorder.real()

    def encode_with_indexes(self, symbols, indexes, *tables):
        _Recorder.calls.append((np.asarray(symbols, np.int32), np.asarray(indexes, np.int32)))
        return self._e.encode_with_indexes(symbols, indexes, *tables)

    def flush(self):
        return self._e.flush()


def reference_net(mod, cfg, sd_full, f_holder):
    """The reference's ELIC_master with the full synthetic state dict, its outer blocks replaced by pass-through callables."""
    net = mod.ELIC_master(cfg, channel=3).eval()
    net.load_state_dict(sd_full)
    assert net.update(force=True)
    for name in ("aux_encoder", "master_encoder", "master_decoder", "channel_aligner"):
        delattr(net, name)
    net.aux_encoder = lambda aux: torch.zeros_like(f_holder["f"][:, 64:])
    net.master_encoder = lambda x: x[:, :64]
    net.channel_aligner = lambda fv, aux_f: (f_holder["f"][:, 64:], 0.0, 0.0)
    net.master_decoder = lambda t: t[:, 64:]
    return net


def run(net, f, ups, forced=None):
    """compress / decompress / forward of one net; forced: the symbols quantize() returns instead of its own (per call, in order)."""
    seen, floats = {}, {"x": [], "s": []}
    hooks = [net.h_a.register_forward_hook(lambda m, i, o: seen.update(y=i[0].detach().clone(), z=o.detach().clone())),
             net.g_s.register_forward_hook(lambda m, i, o: seen.update(yhat=i[0].detach().clone(), fhat=o.detach().clone()))]
    gc = net.gaussian_conditional
    q_real, b_real = gc.quantize, gc.build_indexes
    pos = [0]

    def quantize(inputs, mode, means=None):
        if mode != "symbols":
            return q_real(inputs, mode, means)
        floats["x"].append((inputs - means).detach().reshape(-1).numpy().copy())
        if forced is None:
            return q_real(inputs, mode, means)
        n = inputs.numel()
        out = torch.from_numpy(forced[pos[0]:pos[0] + n].copy()).reshape(inputs.shape).int()
        pos[0] += n
        return out

    def build_indexes(scales):
        floats["s"].append(scales.detach().reshape(-1).numpy().copy())
        return b_real(scales)

    aux_out = {"up1": ups[0], "up2": ups[1], "up3": ups[2]}
    _Recorder.calls = []
    gc.quantize, gc.build_indexes = quantize, build_indexes
    with torch.no_grad():
        out = net.compress(f, aux=None, aux_out=aux_out)
    del gc.quantize
    nsym = sum(a.size for a in floats["x"])
    assert len(_Recorder.calls) == 1 and len(out["strings"][0]) == 1 and len(out["strings"][1]) == f.shape[0]
    sym, idx = _Recorder.calls[0]
    with torch.no_grad():
        y, z, yhat_enc = seen["y"], seen["z"], None
        dec = net.decompress(out["strings"], out["shape"], 0.0, 0.0, None, aux_out)
        yhat_dec, fhat = seen["yhat"].clone(), seen["fhat"].clone()
        assert torch.equal(dec["x_hat"], fhat)  # (master_decoder's stand-in returns the g_s half)
        fw = net(f, aux=None, aux_out=aux_out)
    del gc.build_indexes
    for h in hooks:
        h.remove()
    xs, ss = np.concatenate(floats["x"]), np.concatenate(floats["s"])[:nsym]  # (decompress() builds indexes again: compress's come first)
    del yhat_enc
    return dict(out=out, sym=sym, idx=idx, x=xs, s=ss, y=y, z=z, yhat=yhat_dec, fhat=fhat, fw=fw)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def case(mod, mc, name):
    B, H, W, _, wseed = mc.CASES[name]
    cfg = mc.config()
    f, *ups = mc.inputs(name)
    sd_full, sd = mc.weights(name, full=True), mc.weights(name)
    assert all(torch.equal(sd_full[k], v) for k, v in sd.items()) and set(sd_full) - set(sd) == {k for k in sd_full if k.startswith(mc.OUTER)}
    holder = {"f": f}
    r32 = run(reference_net(mod, cfg, sd_full, holder), f, ups)
    net64 = reference_net(mod, cfg, sd_full, holder).double()
    torch.set_default_dtype(torch.float64)
    try:
        holder["f"] = f.double()
        r64 = run(net64, f.double(), [u.double() for u in ups], forced=r32["sym"])
    finally:
        torch.set_default_dtype(torch.float32)
        holder["f"] = f
    sym, idx = r32["sym"], r32["idx"]
    h, w = H // 16, W // 16
    assert sym.size == B * mc.M * h * w == r32["x"].size == r32["s"].size == r64["x"].size == r64["s"].size
    assert np.array_equal(np.rint(r32["x"]).astype(np.int32), sym) and np.array_equal(r64["sym"], sym)
    med = net64.entropy_bottleneck._get_medians().detach()
    zsym = torch.round(r32["z"].double() - med).to(torch.int32)
    assert torch.equal(zsym, torch.round(r64["z"] - med).to(torch.int32)), "fp32 and fp64 z symbols differ"
    assert r32["out"]["strings"][1] == r64["out"]["strings"][1]
    # ---- fixture conditions, on the reference alone
    ymax = float(r32["y"].abs().max())
    nz = float(np.mean(sym != 0))
    parts, o = [], 0
    for C in cfg["slice_ch"]:
        for _ in range(2):
            n = B * C * h * (w // 2)
            parts.append(int((sym[o:o + n] != 0).sum()))
            o += n
    rows = int(np.unique(idx).size)
    e = {"y": rel(r32["y"], r64["y"]), "yhat": rel(r32["yhat"], r64["yhat"]), "x": rel(r32["x"], r64["x"]), "sigma": rel(r32["s"], r64["s"]),
         "fhat": rel(r32["fhat"], r64["fhat"])}
    fx = {"x64": r64["x"].astype(np.float64), "sigma64": r64["s"].astype(np.float64), "e_ref_x": e["x"], "e_ref_sigma": e["sigma"]}
    bx, bs = mc.decision_bounds(fx)
    d_round, d_scale = mc.boundary_distances(fx)
    near_r, near_s = float(np.mean(d_round < bx)), float(np.mean(d_scale < bs))
    nbytes = len(r32["out"]["strings"][0][0]) + sum(len(s) for s in r32["out"]["strings"][1])
    print(f"master_latent {name}: y {len(r32['out']['strings'][0][0])} B, z {[len(s) for s in r32['out']['strings'][1]]} B, "
          f"{nbytes * 8 / (B * H * W):.2f} bpp; max |y| {ymax:.1f}, non-zero symbols {100 * nz:.0f} %, per part {parts}, scale rows {rows}, "
          f"max |sigma| {np.abs(r64['s']).max():.1f}", flush=True)
    print("   reference fp32 against its fp64 run (max |d| / max |ref|):", {k: f"{v:.2e}" for k, v in e.items()})
    print(f"   decisions within the float bound of a boundary: rounding {100 * near_r:.3f} % (bound {bx:.2e}), scale index {100 * near_s:.3f} % (bound {bs:.2e})",
          flush=True)
    assert 4.0 <= ymax <= 64.0, ymax
    assert nz >= 0.25, nz
    assert min(parts) > 0, parts
    assert rows >= 16, rows
    assert near_r <= 0.01 and near_s <= 0.01, (near_r, near_s)
    # ... and none within the reference's OWN fp32 error of one (FACTOR = 1): there the reference's fp32 run does not take the
    # decision reliably itself, and everything that compares free-running results with it (streams, forward()'s bit sums)
    # would hang on a coin toss.  Seeds are tuned until this holds (3 to 9 decisions per case remain inside the 8-fold bound).
    own_r, own_s = float(d_round.min()) / (bx / mc.FACTOR), float(d_scale.min()) / (bs / mc.FACTOR)
    print(f"   closest decision to a boundary, in units of the reference's own error: rounding {own_r:.2f}, scale index {own_s:.2f}", flush=True)
    assert own_r > 1.0 and own_s > 1.0, (own_r, own_s)
    assert np.abs(sym).max() < 32768 and idx.max() < 128 and int(zsym.abs().max()) < 32768
    # ---- the restatement of master_latent_cases.py restates this model
    rs = mc.Restated(sd)
    with torch.no_grad():
        y_rs = rs.g_a(f)
        yhat_rs, x_rs, s_rs, _ = rs.latent(y_rs, zsym.numpy(), sym)
        fhat_rs = rs.g_s(yhat_rs, *ups)
    e_rs = {"y": rel(y_rs, r64["y"]), "yhat": rel(yhat_rs, r64["yhat"]), "x": rel(x_rs, r64["x"]), "sigma": rel(s_rs, r64["s"]), "fhat": rel(fhat_rs, r64["fhat"])}
    print("   the float64 restatement against the fp64 run:", {k: f"{v:.1e}" for k, v in e_rs.items()}, flush=True)
    assert all(v < 1e-9 for v in e_rs.values()), e_rs

    bits = lambda t: np.float64(-torch.log2(t.double()).sum().item())  # noqa: E731

    def gap(k):
        a, b = -torch.log2(r32["fw"]["likelihoods"][k].double()), -torch.log2(r64["fw"]["likelihoods"][k].double())
        return np.float64(((a - b).abs().sum() / b.sum()).item())

    pos = mc.fhat_positions(name)
    fh64 = r64["fhat"].reshape(-1)
    g = {"B": B, "H": H, "W": W, "seed": mc.CASES[name][3], "wseed": wseed, "shape": np.array(tuple(r32["out"]["shape"]), np.int32),
         "y_stream": np.frombuffer(r32["out"]["strings"][0][0], np.uint8), "symbols": sym.astype(np.int16), "indexes": idx.astype(np.int8),
         "z_symbols": zsym.numpy().astype(np.int16), "x64": fx["x64"], "sigma64": fx["sigma64"],
         "y_sub64": mc.y_sub(r64["y"].numpy()), "yhat_sub64": mc.y_sub(r64["yhat"].numpy()),
         "y64_max": np.float64(r64["y"].abs().max()), "yhat64_max": np.float64(r64["yhat"].abs().max()),
         "e_ref_y": np.float64(e["y"]), "e_ref_yhat": np.float64(e["yhat"]), "e_ref_x": np.float64(e["x"]), "e_ref_sigma": np.float64(e["sigma"]),
         "e_ref_fhat": np.float64(e["fhat"]), "fhat64": (fh64 if pos is None else fh64[torch.from_numpy(pos)]).numpy(),
         "ref64_max": np.float64(r64["fhat"].abs().max()),
         "lik_y_bits": bits(r32["fw"]["likelihoods"]["y_likelihoods"]), "lik_z_bits": bits(r32["fw"]["likelihoods"]["z_likelihoods"]),
         "lik_y_bits64": bits(r64["fw"]["likelihoods"]["y_likelihoods"]), "lik_z_bits64": bits(r64["fw"]["likelihoods"]["z_likelihoods"]),
         "lik_y_gap": gap("y_likelihoods"), "lik_z_gap": gap("z_likelihoods")}
    for i, s in enumerate(r32["out"]["strings"][1]):
        g[f"z{i}"] = np.frombuffer(s, np.uint8)
    print(f"   forward(): fp32 - fp64 gap of the likelihood bits, y {g['lik_y_gap']:.2e}, z {g['lik_z_gap']:.2e}")
    path = os.path.join(HERE, f"master_latent_{name}.npz")
    np.savez_compressed(path, **g)
    print(f"   {os.path.basename(path)}: {os.path.getsize(path)} bytes", flush=True)
    assert os.path.getsize(path) <= 1 << 20


def main():
    rl.load_reference()
    import models.elic_master as mod

    import master_latent_cases as mc

    torch.manual_seed(0)
    _Recorder.real = mod.BufferedRansEncoder
    mod.BufferedRansEncoder = _Recorder
    only = sys.argv[1:] or list(mc.CASES)
    for name in only:
        case(mod, mc, name)
    if len(only) == len(mc.CASES):
        from config.config import model_config

        doc = {f"channel{ch}": [[k, list(v.shape)] for k, v in mod.ELIC_master(model_config(), channel=ch).state_dict().items()] for ch in (3, 1)}
        with open(os.path.join(HERE, "master_state_dict.json"), "w") as fjs:
            json.dump(doc, fjs, indent=0)
            fjs.write("\n")
        print("state_dict tensors:", {k: len(v) for k, v in doc.items()})


if __name__ == "__main__":
    main()
