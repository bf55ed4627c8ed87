"""Spatial_aligner (rgbd_amd.Spatial_aligner; reference modules/transform/spatialAligner.py:341-390): the cases of the
fixtures tests/golden/aligner_<case>.npz (written by tests/golden/make_aligner.py from the unmodified reference), their
inputs and weights, the acceptance bound, and a torch restatement of the block with deliberate mistakes selectable --
shared by test_aligner_cases.py (CPU) and test_gpu_aligner.py.

Bound: e = max |out - ref64| / max |ref64| <= 8 * e_ref, e_ref = the reference's own fp32 error against its float64 run
(aligner_floors.json).  The factor covers another summation order (MFMA chains, blocked sums) and the device's expf / erff /
rsqrtf against the CPU's."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import guided_attention_cases as gc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTOR = 8.0
EMBED, HEADS = 96, 3
# name: (B, in_channel, out_channel, H, W, input seed, weight seed): one window per block (the shifted frame wraps onto
# itself); two images, non-square; the other orientation; in_channel != out_channel
CASES = {"a_1x192_8x8": (1, 192, 192, 8, 8, 101, 1), "b_2x192_16x24": (2, 192, 192, 16, 24, 102, 2),
         "c_1x192_24x16": (1, 192, 192, 24, 16, 103, 3), "d_1x64to96_16x8": (1, 64, 96, 16, 8, 104, 4)}
MUTATIONS = ["noshift", "guided_norm2", "eg_updated", "recovery_dydx", "xg_swapped"]


def case_inputs(name):
    B, cin, _, H, W, seed, _ = CASES[name]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, cin, H, W, generator=g), torch.randn(B, cin, H, W, generator=g)


def case_weights(name):
    from rgbd_amd import synth

    _, cin, cout, _, _, _, wseed = CASES[name]
    return synth.synthetic_state_dict(wseed, model="Spatial_aligner", in_channel=cin, out_channel=cout)


def load_fixture(name):
    g = dict(np.load(os.path.join(GOLDEN, f"aligner_{name}.npz")))
    with open(os.path.join(GOLDEN, "aligner_floors.json")) as f:
        g["e_ref"] = float(json.load(f)[name]["e_ref"])
    return g


def rel_err(out, ref64):
    out, ref64 = torch.as_tensor(out).double(), torch.as_tensor(ref64).double()
    return float((out - ref64).abs().max() / ref64.abs().max())


def aligner(sd, x, guided, mut=None, dtype=torch.float64):
    """The block restated: patch embeddings, two Swin blocks with the guided attention of guided_attention_cases.gwa (shift 0,
    then 2; norm1 on both streams; the guided stream is never updated), the transposed convolution.  mut: "noshift" the second
    block's shift dropped, "guided_norm2" guided normalised with norm2, "eg_updated" the guided stream replaced by the first
    block's output, "recovery_dydx" the taps of recovery transposed, "xg_swapped" x and guided exchanged."""
    w = lambda n: sd[n].to(dtype)  # noqa: E731
    x, guided = x.to(dtype), guided.to(dtype)
    if mut == "xg_swapped":
        x, guided = guided, x
    ex = F.conv2d(x, w("patch_embeding1.weight"), w("patch_embeding1.bias"), stride=2).permute(0, 2, 3, 1)
    eg = F.conv2d(guided, w("patch_embeding2.weight"), w("patch_embeding2.bias"), stride=2).permute(0, 2, 3, 1)
    for k in range(2):
        p = f"blocks.{k}"
        shift = 2 if (k == 1 and mut != "noshift") else 0
        ln = lambda t, n: F.layer_norm(t, (EMBED,), w(f"{p}.{n}.weight"), w(f"{p}.{n}.bias"), 1e-5)  # noqa: E731
        lin = lambda t, n: F.linear(t, w(f"{p}.{n}.weight"), w(f"{p}.{n}.bias"))  # noqa: E731
        q = lin(ln(ex, "norm1"), "attn.qkv1")
        kv = lin(ln(eg, "norm2" if mut == "guided_norm2" else "norm1"), "attn.qkv2")
        a = gc.gwa(q, kv, w(f"{p}.attn.relative_position_bias_table"), HEADS, shift, dtype=dtype)
        x1 = ex + lin(a, "attn.proj")
        ex = x1 + lin(F.gelu(lin(ln(x1, "norm2"), "mlp.fc1")), "mlp.fc2")
        if mut == "eg_updated" and k == 0:
            eg = ex
    rw = w("recovery.weight")
    if mut == "recovery_dydx":
        rw = rw.transpose(2, 3)
    return F.conv_transpose2d(ex.permute(0, 3, 1, 2), rw, w("recovery.bias"), stride=2)
