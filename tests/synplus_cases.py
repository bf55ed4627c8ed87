"""SynthesisTransformPlus (rgbd_amd.SynthesisTransformPlus; reference modules/transform/synthesis.py:74-110): the cases of the
fixtures tests/golden/synplus_<case>.npz (written by tests/golden/make_synplus.py from the unmodified reference), their inputs
and weights, the acceptance bound, and a torch restatement of the module with deliberate mistakes selectable -- shared by
test_synplus_cases.py (CPU) and test_gpu_synplus.py.

Bound: e = max |out - ref64| / max |ref64| <= 8 * e_ref, e_ref = the reference's own fp32 error against its float64 run over
the whole tensors (synplus_floors.json): the project's bound for module-level float contracts (aligner_cases.py,
features_cases.py).  Where ref64 in full would not fit a fixture (case c), out is compared at the fixture's positions (every
channel, every border pixel, seeded interior pixels) and normalised by the stored max |ref64| of the whole tensor."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import aligner_cases as ac

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTOR = 8.0
N, M = 192, 320
# name: (B, ch, h, w, input seed, weight seed) at N = 192, M = 320, the smallest maps the walk takes (h, w multiples of 4): one
# window per aligner block at sp1; two images, non-square; ch = N as ELIC_master builds it; the other orientation
CASES = {"a": (1, 3, 4, 4, 201, 11), "b": (2, 1, 4, 8, 202, 12), "c": (1, 192, 4, 4, 203, 13), "d": (1, 3, 8, 4, 204, 14)}
MUTATIONS = ["sp23_swapped", "sp1_xg_swapped", "residual", "no_sp3", "sp2_after_attn", "sp1_after_rbs"]
YHAT_SCALE = 2.0  # latents of a few units
SAMPLE_LIMIT = 200_000  # floats of ref64 a fixture holds in full
SAMPLE_INTERIOR = 160   # seeded interior pixels per channel of a sampled fixture (plus every border pixel)


def inputs(B, h, w, seed):
    """y_hat [B,M,h,w] and up1..up3 [B,N,2h << k,2w << k], seeded."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, M, h, w, generator=g) * YHAT_SCALE
    return (y,) + tuple(torch.randn(B, N, (2 * h) << k, (2 * w) << k, generator=g) for k in range(3))


def case_inputs(name):
    B, _, h, w, seed, _ = CASES[name]
    return inputs(B, h, w, seed)


def case_weights(name):
    from rgbd_amd import synth

    _, ch, _, _, _, wseed = CASES[name]
    return synth.synthetic_state_dict(wseed, model="SynthesisTransformPlus", N=N, M=M, channel=ch)


def sample_positions(shape, seed):
    """Flat positions into a [B,C,H,W] tensor: per (image, channel) every border pixel and SAMPLE_INTERIOR seeded interior ones."""
    B, C, H, W = shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    border = ((yy == 0) | (yy == H - 1) | (xx == 0) | (xx == W - 1)).reshape(-1)
    bpos, ipos = np.nonzero(border)[0], np.nonzero(~border)[0]
    rng = np.random.Generator(np.random.Philox(key=seed))
    out = []
    for p in range(B * C):
        pick = np.sort(rng.choice(ipos, size=min(SAMPLE_INTERIOR, ipos.size), replace=False))
        out.append(p * H * W + np.concatenate([bpos, pick]))
    return np.concatenate(out).astype(np.int64)


def load_fixture(name):
    g = dict(np.load(os.path.join(GOLDEN, f"synplus_{name}.npz")))
    with open(os.path.join(GOLDEN, "synplus_floors.json")) as f:
        g["e_ref"] = float(json.load(f)[name]["e_ref"])
    return g


def compared(out, fx):
    """The values of `out` the fixture holds, flat: the whole tensor, or its sampled positions."""
    flat = torch.as_tensor(out).reshape(-1)
    return flat[torch.from_numpy(fx["idx"])] if "idx" in fx else flat


def rel_err(out, fx):
    """max |out - ref64| / max |ref64| against a fixture."""
    d = (compared(out, fx).double() - torch.from_numpy(fx["ref64"]).reshape(-1).double()).abs().max()
    return float(d / float(fx["ref64_max"]))


def rel_err_t(out, ref):
    out, ref = torch.as_tensor(out).double(), torch.as_tensor(ref).double()
    return float((out - ref).abs().max() / ref.abs().max())


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def synthesis_plus(sd, x, up1, up2, up3, mut=None, dtype=torch.float64):
    """The module restated: AttentionBlock, deconv, 3 bottlenecks, deconv, AttentionBlock, 3 bottlenecks, deconv, 3 bottlenecks,
    deconv; behind the first three deconvs x = sp_k(x, up_k) (aligner_cases.aligner).  mut: "sp23_swapped" the weights of sp2
    and sp3 exchanged, "sp1_xg_swapped" x and guided exchanged in sp1, "residual" x + sp(x, up) instead of the replacement,
    "no_sp3" the third aligner skipped, "sp2_after_attn" the aligner of stage 5 applied behind the AttentionBlock of stage 6,
    "sp1_after_rbs" the aligner of stage 1 applied behind the bottlenecks of stages 2-4 (in front of stage 5)."""
    p = "synthesis_transform."
    w = lambda n: sd[p + n].to(dtype)  # noqa: E731
    conv = lambda t, n, pad=0: F.conv2d(t, w(n + ".weight"), w(n + ".bias"), padding=pad)  # noqa: E731

    def res_unit(t, n):  # compressai/layers/layers.py:177-196
        u = torch.relu(conv(t, n + ".conv.0"))
        u = torch.relu(conv(u, n + ".conv.2", 1))
        return torch.relu(conv(u, n + ".conv.4") + t)

    def attention(t, n):  # layers.py:198-213
        a = b = t
        for u in range(3):
            a = res_unit(a, f"{n}.conv_a.{u}")
            b = res_unit(b, f"{n}.conv_b.{u}")
        return a * torch.sigmoid(conv(b, n + ".conv_b.3")) + t

    def bottleneck(t, n):  # modules/layers/res_blk.py:7-27
        u = torch.relu(conv(t, n + ".branch.0"))
        u = torch.relu(conv(u, n + ".branch.2", 1))
        return conv(u, n + ".branch.4") + t

    def deconv(t, n):  # modules/layers/conv.py:16-24
        return F.conv_transpose2d(t, w(n + ".weight"), w(n + ".bias"), stride=2, padding=2, output_padding=1)

    ups = [up1, up2, up3]
    sps = ["sp1.", "sp2.", "sp3."]
    if mut == "sp23_swapped":
        sps = ["sp1.", "sp3.", "sp2."]

    def align(t, k):
        if mut == "no_sp3" and k == 2:
            return t
        o = ac.aligner(_sub(sd, sps[k]), t, ups[k], "xg_swapped" if (mut == "sp1_xg_swapped" and k == 0) else None, dtype)
        return t + o if mut == "residual" else o

    late = {"sp1_after_rbs": (0, 4), "sp2_after_attn": (1, 6)}.get(mut)  # (aligner, the stage it is applied behind instead)
    x = x.to(dtype)
    kinds = ["attn", "deconv", "rb", "rb", "rb", "deconv", "attn", "rb", "rb", "rb", "deconv", "rb", "rb", "rb", "deconv"]
    num = 0
    for i, kind in enumerate(kinds):
        x = attention(x, str(i)) if kind == "attn" else (bottleneck(x, str(i)) if kind == "rb" else deconv(x, str(i)))
        if kind == "deconv":
            if num < 3 and not (late and late[0] == num):
                x = align(x, num)
            num += 1
        if late and late[1] == i:
            x = align(x, late[0])
    return x
