"""Feature_encoder / Feature_decoder (reference models/elic_master.py:15-53) and their two image-facing layers
(rgbd_conv3x3_thin_in / rgbd_conv3x3_thin_out of csrc/thin_conv.hip): the cases of the fixtures
tests/golden/features_<case>.npz (written by tests/golden/make_features.py from the unmodified reference), their inputs and
weights, fp64 statements of both operators and of both modules with deliberate mistakes selectable, and the acceptance bound
-- shared by test_features_cases.py (CPU) and test_gpu_thin_conv.py (the operators alone; the modules' statement and fixtures
are what an engine path for the two networks will be held to).

Bound: e = max |out - ref64| / max |ref64| <= 8 * max(e_ref, 2^-23).  Kernel level: e_ref = the statement below evaluated in
fp32 (torch's convolution) against itself in fp64.  Module level: e_ref = the unmodified reference's fp32 run against its own
float64 run on the same inputs (features_floors.json).  The factor covers another summation order; no fp32 result can be asked
to beat one ulp of the largest value.

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
WEIGHT_SEED = 47
FULL_UP_TO = 13 * 7   # maps up to this many pixels are stored in full, larger ones at NPOS positions
NPOS = 2048

# ---- the operators ------------------------------------------------------------------------------------------------------------
# degenerate maps (every tap but the centre meets padding somewhere), the smallest with an interior, odd sizes, a map of
# several workgroups in both kernels' tilings with ragged right and bottom tiles (67 = 16 * 4 + 3 = 8 * 8 + 3, 129 = 2 * 64 + 1)
KERNEL_MAPS = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (13, 7), (24, 40), (67, 129)]
KERNEL_B = 2                     # every case at B = 2 (an image alone vs in the batch)
THIN_IN_CH = [(1, 64), (3, 64), (4, 16)]    # (Cin, Cout)
THIN_OUT_CH = [(64, 1), (64, 3), (16, 4)]
PADS = (0, 16)                   # channel stride of the NHWC side = its channels + pad


def _kernel_cases(chs, seed0):
    out = {}
    for i, (ci, co) in enumerate(chs):
        for j, (h, w) in enumerate(KERNEL_MAPS):
            out[f"{ci}to{co}_{h}x{w}"] = (KERNEL_B, h, w, ci, co, seed0 + 16 * i + j)
    return out


THIN_IN_CASES = _kernel_cases(THIN_IN_CH, 500)    # name: (B, H, W, Cin, Cout, seed)
THIN_OUT_CASES = _kernel_cases(THIN_OUT_CH, 600)
KERNEL_MUTATIONS = ["taps_transposed", "taps_flipped", "bias_dropped"]


def accept(e, e_ref):
    return e <= FACTOR * max(e_ref, FLOOR)


def rel_err(out, ref64):
    out, ref64 = torch.as_tensor(out).double(), torch.as_tensor(ref64).double()
    return float((out - ref64).abs().max() / ref64.abs().max())


def _mutate_taps(w, mut):
    if mut == "taps_transposed":
        return w.transpose(2, 3)
    if mut == "taps_flipped":
        return w.flip(2, 3)
    return w


def thin_in(x, w, b, mut=None, dtype=torch.float64):
    """rgbd_conv3x3_thin_in: x [B,Cin,H,W], w [Cout,Cin,3,3], b [Cout] or None -> NHWC [B,H,W,Cout]."""
    b = None if (b is None or mut == "bias_dropped") else b.to(dtype)
    return F.conv2d(x.to(dtype), _mutate_taps(w.to(dtype), mut), b, padding=1).permute(0, 2, 3, 1).contiguous()


def thin_out(x, w, b, mut=None, dtype=torch.float64):
    """rgbd_conv3x3_thin_out: x NHWC [B,H,W,Cin], w [Cout,Cin,3,3] in convolution orientation, b [Cout] or None -> [B,Cout,H,W]."""
    b = None if (b is None or mut == "bias_dropped") else b.to(dtype)
    return F.conv2d(x.to(dtype).permute(0, 3, 1, 2), _mutate_taps(w.to(dtype), mut), b, padding=1).contiguous()


def deconv_as_conv(t, mut=None):
    """A ConvTranspose2d(Cin, Cout, 3, 1, 1) weight t [Cin,Cout,3,3] in the orientation thin_out takes: channel axes exchanged,
    taps turned by 180 degrees.  mut: "taps_not_flipped", "axes_not_exchanged" (the buffer read as [Cout][Cin] as it lies)."""
    w = t.reshape(t.shape[1], t.shape[0], 3, 3) if mut == "axes_not_exchanged" else t.transpose(0, 1)
    return (w if mut == "taps_not_flipped" else w.flip(2, 3)).contiguous()


@functools.lru_cache(maxsize=None)
def kernel_inputs(op, name):
    """(x, w, b) of a kernel case: x in the operator's input layout (thin_in: planes, thin_out: NHWC)."""
    B, H, W, ci, co, seed = (THIN_IN_CASES if op == "thin_in" else THIN_OUT_CASES)[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, ci, H, W) if op == "thin_in" else (B, H, W, ci), generator=g)
    w = (torch.rand(co, ci, 3, 3, generator=g) * 2 - 1) / (9 * ci) ** 0.5
    b = (torch.rand(co, generator=g) * 2 - 1) * 0.5
    return x, w, b


@functools.lru_cache(maxsize=None)
def kernel_refs(op, name):
    """(ref64, e_ref) of a kernel case; shared, never modified."""
    f = thin_in if op == "thin_in" else thin_out
    x, w, b = kernel_inputs(op, name)
    ref = f(x, w, b)
    return ref, rel_err(f(x, w, b, dtype=torch.float32), ref)


# ---- the modules ----------------------------------------------------------------------------------------------------------------
MODULE_SIZES = [(1, 2, 2), (2, 3, 3), (1, 13, 7), (2, 24, 40), (1, 67, 129)]
NETS = {"enc1": ("Feature_encoder", 1, 64), "enc3": ("Feature_encoder", 3, 64), "dec256to3": ("Feature_decoder", 256, 3),
        "dec256to1": ("Feature_decoder", 256, 1), "dec192to3": ("Feature_decoder", 192, 3)}   # net: (model, in_ch, out_ch)
LARGEST = "67x129"


def _module_cases():
    out = {}
    for i, net in enumerate(NETS):
        for j, (b, h, w) in enumerate(MODULE_SIZES):
            out[f"{net}_{h}x{w}"] = (net, b, h, w, 700 + 8 * i + j)
    return out


CASES = _module_cases()   # name: (net, B, H, W, input seed)
# wrong restatements, and the nets each can show on
MODULE_MUTATIONS = {
    "leaky_relu": ("enc", "dec"),             # the name the reference gives its nn.ReLU
    "add_before_relu": ("enc", "dec"),        # relu(conv2(t) + identity)
    "no_outer_shortcut": ("enc", "dec"),
    "skip_conv_exchanged": ("dec",),          # resblock1.skip <-> conv
    "taps_not_flipped": ("dec",),             # deconv1 read as a convolution without the 180 degree turn
    "axes_not_exchanged": ("dec",),           # deconv1's [64][out] buffer read as [out][64]
    "taps_transposed": ("enc", "dec"),        # the image-facing layer
    "bias_dropped": ("enc", "dec"),           # the image-facing layer
}


def mutations_of(net):
    """(one output channel: deconv1's [64][1] buffer IS [1][64], the axes cannot be confused)"""
    return [m for m, kinds in MODULE_MUTATIONS.items() if net[:3] in kinds and not (m == "axes_not_exchanged" and NETS[net][2] == 1)]


@functools.lru_cache(maxsize=None)
def net_weights(net):
    from rgbd_amd import synth

    model, ci, co = NETS[net]
    return synth.synthetic_state_dict(WEIGHT_SEED, model=model, in_channel=ci, out_channel=co)


def case_inputs(name):
    net, B, H, W, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, NETS[net][1], H, W, generator=g)


def _conv(sd, n, x, dtype):
    w = sd[f"{n}.weight"].to(dtype)
    return F.conv2d(x, w, sd[f"{n}.bias"].to(dtype), padding=w.shape[2] // 2)


def _res_block(sd, p, x, mut, dtype):
    """modules/layers/res_blk.py:48-57."""
    act = F.leaky_relu if mut == "leaky_relu" else F.relu
    skip = "conv" if (mut == "skip_conv_exchanged" and p == "resblock1") else f"{p}.skip"
    ident = _conv(sd, skip, x, dtype) if f"{p}.skip.weight" in sd else x
    t = _conv(sd, f"{p}.conv2", act(_conv(sd, f"{p}.conv1", x, dtype)), dtype)
    return act(t + ident) if mut == "add_before_relu" else act(t) + ident


def _blocks(sd, x, mut, dtype):
    for p in ("resblock1", "resblock2", "resblock3"):
        x = _res_block(sd, p, x, mut, dtype)
    return x


def module_statement(name, mut=None, dtype=torch.float64):
    """The statement of case `name`, [B,64 | out_ch,H,W].  mut: one of MODULE_MUTATIONS."""
    net = CASES[name][0]
    sd = net_weights(net)
    x = case_inputs(name).to(dtype)
    km = mut if mut in ("taps_transposed", "bias_dropped") else None
    if net.startswith("enc"):   # elic_master.py:23-31
        s = thin_in(x, sd["conv1.weight"], sd["conv1.bias"], km, dtype).permute(0, 3, 1, 2)
        out = _blocks(sd, s, mut, dtype)
        return (out if mut == "no_outer_shortcut" else out + s).contiguous()
    out = _blocks(sd, x, mut, dtype)   # elic_master.py:44-53
    if mut != "no_outer_shortcut":
        out = out + _conv(sd, "resblock1.skip" if mut == "skip_conv_exchanged" else "conv", x, dtype)
    w = deconv_as_conv(sd["deconv1.weight"], mut)
    return thin_out(out.permute(0, 2, 3, 1), w, sd["deconv1.bias"], km, dtype)


def positions(name, numel):
    """Where a fixture holds its output: everything up to FULL_UP_TO pixels, else NPOS flat indexes from the case seed."""
    net, B, H, W, seed = CASES[name]
    if H * W <= FULL_UP_TO:
        return torch.arange(numel)
    return torch.randint(0, numel, (NPOS,), generator=torch.Generator().manual_seed(seed + 100000))


def load_fixture(name):
    g = dict(np.load(os.path.join(GOLDEN, f"features_{name}.npz")))
    with open(os.path.join(GOLDEN, "features_floors.json")) as f:
        g["e_ref"] = float(json.load(f)[name])
    return g
