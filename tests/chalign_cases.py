"""Channel_aligner (reference modules/transform/channelAligner.py) and its pooled head (rgbd_pooled_conv3x3 of
csrc/pooled_head.hip): the cases of the fixtures tests/golden/chalign_<case>.npz (written by tests/golden/make_chalign.py from
the unmodified reference), their inputs and weights, fp64 statements of the pooled head and of the module with deliberate
mistakes selectable, and the acceptance bound -- shared by test_chalign_cases.py (CPU) and test_gpu_chalign.py (the head alone;
the module's statement and fixtures are what an engine path for the whole block will be held to).

The pooled head: AdaptiveAvgPool2d(1) of a zero-padded 3x3 convolution is linear in the input.  Summed over all output
positions, tap (di, dj) sees the channel's total minus the border row it never reaches (di = 0: the last row, 1: none, 2: the
first), minus the border column (the same in dj), plus the corner both took out.  Nine numbers per (image, channel) and a
Cout x (Cin * 9) product give the pooled value exactly, H = 1 and W = 1 included.

Bound: e = max |out - ref64| / max |ref64| <= 8 * e_ref, e_ref floored at 2^-23 (a pooled value averages rounding errors away,
and no fp32 result can be asked to beat one ulp of the largest value).  Module level: e_ref = the reference's own fp32 error
against its float64 run on the same images (chalign_floors.json, per output and batch prefix).  Kernel level: the error of
the statement below evaluated in fp32 against itself in fp64.  The factor covers another summation order.

Every operation here works image by image, so the first b images of a case are the case at B = b."""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTOR = 8.0
FLOOR = 2.0 ** -23
WEIGHT_SEED = 31
# (B, H, W): degenerate maps (a border is the whole map), the smallest with an interior, odd sizes, and one with several
# workgroups and a ragged last chunk per image (67 * 129 = 135 * 64 + 3 pixels)
SIZES = [(1, 2, 2), (1, 1, 5), (1, 5, 1), (2, 3, 3), (1, 13, 7), (2, 24, 40), (2, 67, 129)]
LARGEST = "67x129"


def _module_cases():
    return {f"{h}x{w}": (b, h, w, 300 + i) for i, (b, h, w) in enumerate(SIZES)}


def _kernel_cases():
    out = {f"k256_{h}x{w}": (2, h, w, 256, 64, 400 + i) for i, (_, h, w) in enumerate(SIZES)}
    out["k16_1x1"] = (2, 1, 1, 16, 8, 420)
    out["k16_2x2"] = (2, 2, 2, 16, 8, 421)
    return out


CASES = _module_cases()          # name: (B, H, W, input seed)
KERNEL_CASES = _kernel_cases()   # name: (B, H, W, Cin, Cout, seed); every one at B = 2 (an image alone vs in the batch)
PADS = (0, 16)                   # channel stride = Cin + pad, NaN in the padding

# wrong restatements of the head, and where each can show at all (H, W of the map)
HEAD_MUTATIONS = {
    "no_border": lambda H, W: True,            # the total used for all nine taps
    "rows_swapped": lambda H, W: H >= 2,       # first and last row exchanged (one row: they are the same row)
    "cols_swapped": lambda H, W: W >= 2,
    "corner_dropped": lambda H, W: True,
    "corner_sign": lambda H, W: True,          # the corner subtracted
    "taps_transposed": lambda H, W: H * W > 1,  # (one pixel: only the centre tap sees anything)
    "taps_flipped": lambda H, W: H * W > 1,    # by 180 degrees
    "padded_area": lambda H, W: True,          # division by (H + 2)(W + 2)
}
MODULE_MUTATIONS = ["heads_exchanged", "halves_exchanged", "identity_f1"]  # conv2 <-> conv3; beta from feature2's trunk, gamma
#                                                                           from feature1's; out = gamma * feature1 + beta


def accept(e, e_ref):
    return e <= FACTOR * max(e_ref, FLOOR)


def rel_err(out, ref64):
    out, ref64 = torch.as_tensor(out).double(), torch.as_tensor(ref64).double()
    return float((out - ref64).abs().max() / ref64.abs().max())


# ---- the pooled head, stated on NHWC tensors ----------------------------------------------------------------------------------
def border_sums(x):
    """x [B,H,W,C] -> [B,9,C]: total, first row, last row, first column, last column, corners (0,0) (0,W-1) (H-1,0) (H-1,W-1)."""
    return torch.stack([x.sum((1, 2)), x[:, 0].sum(1), x[:, -1].sum(1), x[:, :, 0].sum(1), x[:, :, -1].sum(1),
                        x[:, 0, 0], x[:, 0, -1], x[:, -1, 0], x[:, -1, -1]], dim=1)


def pooled_head(x, w, b, mut=None, dtype=torch.float64):
    """rgbd_pooled_conv3x3: x [B,H,W,C], w [O,C,3,3], b [O] -> [B,O].  mut: one of HEAD_MUTATIONS."""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    B, H, W, C = x.shape
    s = border_sums(x)
    T = s[:, 0]
    zero = torch.zeros_like(T)
    first_r, last_r, first_c, last_c = s[:, 1], s[:, 2], s[:, 3], s[:, 4]
    if mut == "rows_swapped":
        first_r, last_r = last_r, first_r
    if mut == "cols_swapped":
        first_c, last_c = last_c, first_c
    R = [last_r, zero, first_r]  # what tap row 0 / 1 / 2 never reaches
    L = [last_c, zero, first_c]
    K = [[s[:, 8], zero, s[:, 7]], [zero, zero, zero], [s[:, 6], zero, s[:, 5]]]
    if mut == "rows_swapped":
        K = [K[2], K[1], K[0]]
    if mut == "cols_swapped":
        K = [[r[2], r[1], r[0]] for r in K]
    if mut == "taps_transposed":
        w = w.transpose(2, 3)
    if mut == "taps_flipped":
        w = w.flip(2, 3)
    acc = torch.zeros(B, w.shape[0], dtype=dtype)
    for di in range(3):
        for dj in range(3):
            if mut == "no_border":
                S = T
            else:
                corner = {"corner_dropped": 0.0, "corner_sign": -1.0}.get(mut, 1.0) * K[di][dj]
                S = T - R[di] - L[dj] + corner
            acc = acc + S @ w[:, :, di, dj].t()
    area = (H + 2) * (W + 2) if mut == "padded_area" else H * W
    return b + acc / area


def conv_mean(x, w, b, dtype=torch.float64):
    """What the head replaces: AdaptiveAvgPool2d(1)(conv3x3(x)) (channelAligner.py:30-31), x [B,H,W,C] -> [B,O]."""
    return F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype), b.to(dtype), padding=1).mean((2, 3))


def kernel_inputs(name):
    """The kind of map the trunk produces -- LeakyReLU of a shifted normal, mean well away from zero -- with the first and last
    rows and columns scaled by distinct factors, so that every border term and every corner carries weight of its own."""
    B, H, W, C, O, seed = KERNEL_CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = F.leaky_relu(torch.randn(B, H, W, C, generator=g) + 0.5)
    x[:, 0] *= 3.0
    x[:, -1] *= 5.0
    x[:, :, 0] *= 7.0
    x[:, :, -1] *= 9.0
    w = (torch.rand(O, C, 3, 3, generator=g) * 2 - 1) / (9 * C) ** 0.5
    b = (torch.rand(O, generator=g) * 2 - 1) / (9 * C) ** 0.5
    return x, w, b


def kernel_e_ref(name):
    x, w, b = kernel_inputs(name)
    return rel_err(pooled_head(x, w, b, dtype=torch.float32), pooled_head(x, w, b))


# ---- the module ----------------------------------------------------------------------------------------------------------------
def case_inputs(name):
    """feature1, feature2 [B,64,H,W]; feature2 with a scale and mean of its own."""
    B, H, W, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    f1 = torch.randn(B, 64, H, W, generator=g)
    f2 = torch.randn(B, 64, H, W, generator=g) * 1.5 + 0.25
    return f1, f2


@functools.lru_cache(maxsize=None)
def module_weights():
    from rgbd_amd import synth

    return synth.synthetic_state_dict(WEIGHT_SEED, model="Channel_aligner")


@functools.lru_cache(maxsize=None)
def _trunks(name):
    """conv1 on feature1 and on feature2 in fp64, NHWC (shared by every statement of a case; never modified)."""
    sd = module_weights()
    out = []
    for t in case_inputs(name):
        t = t.double()
        for i in (0, 2, 4, 6):
            t = F.leaky_relu(F.conv2d(t, sd[f"conv1.{i}.weight"].double(), sd[f"conv1.{i}.bias"].double(), padding=1))
        out.append(t.permute(0, 2, 3, 1).contiguous())
    return tuple(out)


def module_statement(name, mut=None):
    """The fp64 statement of case `name`: (out, beta, gamma) with beta, gamma [B,64].  mut: a HEAD or MODULE mutation."""
    sd = module_weights()
    f1, f2 = case_inputs(name)
    t1, t2 = _trunks(name)
    if mut == "halves_exchanged":
        t1, t2 = t2, t1
    hb, hg = ("conv3", "conv2") if mut == "heads_exchanged" else ("conv2", "conv3")
    hm = mut if mut in HEAD_MUTATIONS else None
    beta = pooled_head(t1, sd[f"{hb}.weight"], sd[f"{hb}.bias"], hm)
    gamma = pooled_head(t2, sd[f"{hg}.weight"], sd[f"{hg}.bias"], hm)
    ident = (f1 if mut == "identity_f1" else f2).double()
    return gamma[:, :, None, None] * ident + beta[:, :, None, None], beta, gamma


def load_fixture(name):
    g = dict(np.load(os.path.join(GOLDEN, f"chalign_{name}.npz")))
    with open(os.path.join(GOLDEN, "chalign_floors.json")) as f:
        g["floors"] = json.load(f)[name]
    return g


def fixture_refs(name, fx):
    """(out64, beta64, gamma64) of the fixture as fp64 tensors; out rebuilt from feature2 and the stored beta64 / gamma64."""
    beta, gamma = torch.from_numpy(fx["beta64"]).double(), torch.from_numpy(fx["gamma64"]).double()
    f2 = case_inputs(name)[1].double()
    return gamma[:, :, None, None] * f2 + beta[:, :, None, None], beta, gamma


def module_errors(name, fx, got, b):
    """{"out" | "beta" | "gamma": (e, e_ref)} of `got` = (out, beta, gamma) on the first b images against the fixture."""
    res = {}
    for key, g, r in zip(("out", "beta", "gamma"), got, fixture_refs(name, fx)):
        g = torch.as_tensor(g).double()
        g = g.reshape(g.shape[0], *r.shape[1:])[:b]  # (beta, gamma as [B,64] or [B,64,1,1])
        res[key] = (rel_err(g, r[:b]), float(fx["floors"][key][str(b)]))
    return res


def module_accepts(name, fx, got, b):
    return all(accept(e, er) for e, er in module_errors(name, fx, got, b).values())
