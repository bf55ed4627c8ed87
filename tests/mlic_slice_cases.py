"""The per-slice networks of MLIC++ (rgbd_amd.EntropyParametersMLIC / ChannelContext / LatentResidualPrediction and the fused
kernel of csrc/pixel_mlp.hip; reference modules/transform/entropy.py:31-53, context.py:140-160, LRP.py:9-26): the cases of the
fixtures tests/golden/mlicslice_<case>.npz (written by tests/golden/make_mlic_slice.py from the unmodified reference), their
inputs and weights, fp64 statements of the three modules with deliberate mistakes selectable, and the acceptance bound -- shared
by test_mlic_slice_cases.py (CPU) and test_gpu_mlic_slice.py.

Bound: e = max |out - ref64| / max |ref64| <= 8 * e_ref, e_ref = the reference's own fp32 error against its float64 run on the
same images (mlicslice_floors.json, per batch prefix).  The factor covers another summation order (single chains in increasing
k against oneDNN's blocked sums) and the device's erff / tanhf against the CPU's.

A fixture holds a batch of three images; every operation here works image by image, so the first b images are the case at
B = b.  The configurations are those of the model at M = 320 with ten slices of 32 channels (models/mlicpp.py:40-75).

Checked on the CPU before the fixtures were committed (test_mlic_slice_cases.py repeats it): the statements in fp32 stay
within the bound on every case and batch prefix, the largest at 0.23 of it (asserted below MARGIN_FP32), and the closest a
deliberate mistake comes to the bound is 59 bounds (the tanh form of GELU on cc32_8x12; asserted above MARGIN_MISTAKE)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTOR = 8.0
SIZES = [(4, 4), (8, 12), (12, 8), (4, 20)]  # one pixel tile; non-square, several tiles; the other way; wide, a partial tile
BATCHES = (1, 2, 3)
SWEEP = (32, 40)  # the latent grid of a 512 x 640 image, at B = 2
# module configuration: (class name, constructor arguments, weight seed)
MODULES = {
    "ep640": ("EntropyParametersMLIC", {"in_dim": 640, "out_dim": 64}, 21),   # anchor half of slice 0: hyper alone
    "ep704": ("EntropyParametersMLIC", {"in_dim": 704, "out_dim": 64}, 22),   # non-anchor half of slice 0
    "ep832": ("EntropyParametersMLIC", {"in_dim": 832, "out_dim": 64}, 23),   # anchor half of the later slices
    "ep960": ("EntropyParametersMLIC", {"in_dim": 960, "out_dim": 64}, 24),   # non-anchor half of the later slices
    "cc32": ("ChannelContext", {"in_dim": 32, "out_dim": 32}, 25),
    "cc96": ("ChannelContext", {"in_dim": 96, "out_dim": 32}, 26),
    "cc288": ("ChannelContext", {"in_dim": 288, "out_dim": 32}, 27),
    "lrp352": ("LatentResidualPrediction", {"in_dim": 352, "out_dim": 32}, 28),
    "lrp384": ("LatentResidualPrediction", {"in_dim": 384, "out_dim": 32}, 29),   # widths 296 / 208 / 120: no multiples of 16
    "lrp640": ("LatentResidualPrediction", {"in_dim": 640, "out_dim": 32}, 30),
}
SWEEP_MODULES = ("ep960",)
# the codec's torch.cat order in front of the parameter networks (mlicpp.py:122, 147, 163): local, intra, inter, channel, hyper
SEGMENTS = {"ep640": [640], "ep704": [64, 640], "ep832": [64, 128, 640], "ep960": [64, 64, 64, 128, 640]}
# a shape list only (no fixture): the one configuration here whose |out - in| is no multiple of 4, where diff * 3 // 4 and
# 3 * (diff // 4) differ; the model's own configurations cannot tell them apart
SHAPE_ONLY = {"lrp350": ("LatentResidualPrediction", {"in_dim": 350, "out_dim": 32})}


def _cases():
    out, seed = {}, 400
    for mod in MODULES:
        for (h, w) in SIZES:
            out[f"{mod}_{h}x{w}"] = (mod, 3, h, w, seed)
            seed += 1
    for mod in SWEEP_MODULES:
        out[f"{mod}_{SWEEP[0]}x{SWEEP[1]}"] = (mod, 2, SWEEP[0], SWEEP[1], seed)
        seed += 1
    return out


CASES = _cases()  # name: (module key, images in the fixture, H, W, input seed)
# what the weight recipe (synth._apply_stress_mlic_slice) is built for, asserted on every fixture: each GELU of the reference
# saw arguments below -GELU_SIDE and above +GELU_SIDE and none beyond GELU_MAX; the largest |x| in front of the LRP's tanh lies
# in TANH_BAND (tanh(0.8) = 0.66, 17 % off the line; tanh(3.2) = 0.997)
GELU_SIDE, GELU_MAX = 1.0, 12.0
TANH_BAND = (0.8, 3.2)
MARGIN_FP32 = 0.5      # the fp32 statement must leave half of the bound free on every case (measured: at most 0.23 of it)
MARGIN_MISTAKE = 10.0   # every mistake must land at least this many bounds away: a result within one bound of ref64 cannot hide it

EP_MUTATIONS = ["gelu_tanh", "gelu_after_last", "bias_dropped"]
SEGMENT_MUTATIONS = ["segments_exchanged"]
CONV3_MUTATIONS = ["gelu_tanh", "gelu_after_last", "bias_dropped", "taps_transposed"]
LRP_MUTATIONS = CONV3_MUTATIONS + ["half_dropped", "tanh_dropped"]


def case_batches(name):
    return BATCHES if CASES[name][1] == 3 else (CASES[name][1],)


def case_inputs(name):
    """[x], or for EntropyParametersMLIC the segments of its input in the codec's order (torch.cat(segments, 1) is x)."""
    mod, n, H, W, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, MODULES[mod][1]["in_dim"], H, W, generator=g)
    return list(torch.split(x, SEGMENTS[mod], dim=1)) if mod in SEGMENTS else [x]


def module_weights(mod):
    from rgbd_amd import synth

    cls, kw, wseed = MODULES[mod]
    return synth.synthetic_state_dict(wseed, model=cls, **kw)


def load_fixture(name):
    g = dict(np.load(os.path.join(GOLDEN, f"mlicslice_{name}.npz")))
    with open(os.path.join(GOLDEN, "mlicslice_floors.json")) as f:
        g["floors"] = json.load(f)[name]
    return g


def e_ref(fx, b):
    return float(fx["floors"]["e_ref"][str(b)])


def rel_err(out, ref64):
    out, ref64 = torch.as_tensor(out).double(), torch.as_tensor(ref64).double()
    return float((out - ref64).abs().max() / ref64.abs().max())


def anchor_map(H, W):
    """True where (row + col) is odd: the positions coded first (utils/ckbd.py:6-20)."""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return ((y + x) % 2) == 1


# ---- the three modules, stated in fp64 ------------------------------------------------------------------------------------
def _gelu(x, mut):
    return F.gelu(x, approximate="tanh") if mut == "gelu_tanh" else F.gelu(x)


def _stack(sd, prefix, n, x, pad, mut, dtype, seen=None):
    """n convolutions `prefix.{0,2,...}` with GELU between them; seen: collects (min, max) of every GELU's argument."""
    for i in range(n):
        w, b = sd[f"{prefix}.{2 * i}.weight"].to(dtype), sd[f"{prefix}.{2 * i}.bias"].to(dtype)
        if mut == "taps_transposed" and i == 1:
            w = w.transpose(2, 3)
        if mut == "bias_dropped" and i == n - 2:
            b = None
        x = F.conv2d(x, w, b, padding=pad)
        if i < n - 1 or mut == "gelu_after_last":
            if seen is not None and i < n - 1:
                seen.append((float(x.min()), float(x.max())))
            x = _gelu(x, mut)
    return x


def entropy_params(sd, segments, mut=None, dtype=torch.float64, seen=None):
    segments = list(segments)
    if mut == "segments_exchanged":
        segments[0], segments[1] = segments[1], segments[0]
    return _stack(sd, "fusion", 4, torch.cat(segments, dim=1).to(dtype), 0, mut, dtype, seen)


def channel_context(sd, x, mut=None, dtype=torch.float64, seen=None):
    return _stack(sd, "fushion", 3, x.to(dtype), 1, mut, dtype, seen)


def lrp(sd, x, mut=None, dtype=torch.float64, seen=None, pretanh=None):
    t = _stack(sd, "lrp_transform", 4, x.to(dtype), 1, mut, dtype, seen)
    if pretanh is not None:
        pretanh.append(float(t.abs().max()))
    if mut != "tanh_dropped":
        t = torch.tanh(t)
    return t if mut == "half_dropped" else 0.5 * t


def lrp_widths_mistaken(in_dim, out_dim):
    """The widths with 3 * (diff // 4) for diff * 3 // 4."""
    diff = abs(out_dim - in_dim)
    return [in_dim, in_dim - diff // 4, in_dim - diff // 2, in_dim - 3 * (diff // 4), out_dim]


def module_statement(name, b, mut=None, dtype=torch.float64, seen=None, pretanh=None):
    """The fp64 statement of case `name` on its first b images."""
    mod = CASES[name][0]
    sd = module_weights(mod)
    xs = [t[:b] for t in case_inputs(name)]
    cls = MODULES[mod][0]
    if cls == "EntropyParametersMLIC":
        return entropy_params(sd, xs, mut, dtype, seen)
    if cls == "ChannelContext":
        return channel_context(sd, xs[0], mut, dtype, seen)
    return lrp(sd, xs[0], mut, dtype, seen, pretanh)


def mutations_of(mod):
    cls = MODULES[mod][0]
    if cls == "EntropyParametersMLIC":
        return EP_MUTATIONS + (SEGMENT_MUTATIONS if len(SEGMENTS[mod]) > 1 else [])
    return CONV3_MUTATIONS if cls == "ChannelContext" else LRP_MUTATIONS


def pack_fragments(w):
    """rgbd_pixel_mlp4_pack, restated: w [cout][cin] -> [cout / 16][cin / 16][64 lanes][4]; lane (g = lane // 16, i = lane % 16),
    element j holds w[16 t + i][16 c + 4 j + g]."""
    cout, cin = w.shape
    v = w.reshape(cout // 16, 16, cin // 16, 4, 4)  # [t][i][c][j][g]
    return v.permute(0, 2, 4, 1, 3).contiguous().reshape(-1)  # [t][c][g][i][j]
