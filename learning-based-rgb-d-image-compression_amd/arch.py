"""Parameter inventory of the ELIC_united hot path.

The reference checkpoint format is the interface: this module enumerates every
state_dict entry of `ELIC_united` (reference: models/elic_united.py:14-86) by name, shape and role, so
that (a) checkpoints written by the reference load here, (b) synthetic weights can be produced for any
entry, and (c) the device-side weight packer knows what each tensor is.

Nothing here is executable network code; it is a table.
"""
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

# config/config.py:5-10 of the reference
DEFAULT_CONFIG = {
    "N": 192,
    "M": 320,
    "slice_num": 5,
    "context_window": 5,
    "slice_ch": [16, 16, 32, 64, 192],
    "quant": "ste",
}


class Config(dict):
    """Attribute dict with the same access pattern as the reference's utils/IOutils.py:14-23."""

    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def model_config() -> Config:
    return Config({k: (list(v) if isinstance(v, list) else v) for k, v in DEFAULT_CONFIG.items()})


@dataclass(frozen=True)
class Entry:
    shape: Tuple[int, ...]
    kind: str  # conv_w | deconv_w | bias | linear_w | eb_matrix | eb_bias | eb_factor | eb_quantiles | buffer
    dtype: str = "float32"
    fan_in: int = 0
    is_param: bool = True


class _Builder:
    def __init__(self):
        self.entries: "OrderedDict[str, Entry]" = OrderedDict()

    def conv(self, name: str, cin: int, cout: int, k: int):
        self.entries[f"{name}.weight"] = Entry((cout, cin, k, k), "conv_w", fan_in=cin * k * k)
        self.entries[f"{name}.bias"] = Entry((cout,), "bias", fan_in=cin * k * k)

    def deconv(self, name: str, cin: int, cout: int, k: int):
        # ConvTranspose2d weight is (Cin, Cout, kH, kW); torch's fan_in for it is size(1)*k*k
        self.entries[f"{name}.weight"] = Entry((cin, cout, k, k), "deconv_w", fan_in=cout * k * k)
        self.entries[f"{name}.bias"] = Entry((cout,), "bias", fan_in=cout * k * k)

    def linear_nobias(self, name: str, cin: int, cout: int):
        self.entries[f"{name}.weight"] = Entry((cout, cin), "linear_w", fan_in=cin)

    # modules/layers/res_blk.py:7-27
    def bottleneck(self, name: str, n: int, out: Optional[int] = None):
        out = n if out is None else out
        self.conv(f"{name}.branch.0", n, n // 2, 1)
        self.conv(f"{name}.branch.2", n // 2, n // 2, 3)
        self.conv(f"{name}.branch.4", n // 2, out, 1)
        if out != n:
            self.conv(f"{name}.skip", n, out, 1)

    # CompressAI/compressai/layers/layers.py:162-213
    def attention(self, name: str, n: int):
        for br in ("conv_a", "conv_b"):
            for u in range(3):
                self.conv(f"{name}.{br}.{u}.conv.0", n, n // 2, 1)
                self.conv(f"{name}.{br}.{u}.conv.2", n // 2, n // 2, 3)
                self.conv(f"{name}.{br}.{u}.conv.4", n // 2, n, 1)
        self.conv(f"{name}.conv_b.3", n, n, 1)

    # modules/transform/attention.py:70-83
    def esa(self, name: str, n: int):
        f = n // 4
        self.conv(f"{name}.conv1", n, f, 1)
        self.conv(f"{name}.conv_f", f, f, 1)
        self.conv(f"{name}.conv_max", f, f, 3)
        self.conv(f"{name}.conv2", f, f, 3)
        self.conv(f"{name}.conv3", f, f, 3)
        self.conv(f"{name}.conv3_", f, f, 3)
        self.conv(f"{name}.conv4", f, n, 1)

    # modules/transform/attention.py:14-48
    def bi_spf(self, name: str, n: int):
        self.conv(f"{name}.r_ext", n, n // 2, 3)
        self.conv(f"{name}.d_ext", n, n // 2, 3)
        self.esa(f"{name}.d_esa", n)
        self.esa(f"{name}.r_esa", n)

    # modules/transform/attention.py:52-61
    def se(self, name: str, c: int, reduction: int = 16):
        self.linear_nobias(f"{name}.fc.0", c, c // reduction)
        self.linear_nobias(f"{name}.fc.2", c // reduction, c)

    # modules/transform/entropy.py:56-67
    def entropy_params(self, name: str, in_dim: int, out_dim: int):
        self.conv(f"{name}.fusion.0", in_dim, in_dim // 6, 1)
        self.conv(f"{name}.fusion.2", in_dim // 6, out_dim * 4 // 3, 3)
        self.conv(f"{name}.fusion.4", out_dim * 4 // 3, out_dim, 5)
        self.se(f"{name}.se", in_dim)

    # modules/transform/context.py:10-19 (attribute really is spelled "fushion")
    def channel_context(self, name: str, in_dim: int, out_dim: int):
        self.conv(f"{name}.fushion.0", in_dim, 224, 5)
        self.conv(f"{name}.fushion.2", 224, 128, 5)
        self.conv(f"{name}.fushion.4", 128, out_dim, 5)

    # CompressAI/compressai/entropy_models/entropy_models.py:282-314
    def entropy_bottleneck(self, name: str, channels: int, filters=(3, 3, 3, 3)):
        f = (1,) + tuple(filters) + (1,)
        for i in range(len(filters) + 1):
            self.entries[f"{name}._matrix{i}"] = Entry((channels, f[i + 1], f[i]), "eb_matrix")
            self.entries[f"{name}._bias{i}"] = Entry((channels, f[i + 1], 1), "eb_bias")
            if i < len(filters):
                self.entries[f"{name}._factor{i}"] = Entry((channels, f[i + 1], 1), "eb_factor")
        self.entries[f"{name}.quantiles"] = Entry((channels, 1, 3), "eb_quantiles")
        self.buffer(f"{name}._offset", (0,), "int32")
        self.buffer(f"{name}._quantized_cdf", (0,), "int32")
        self.buffer(f"{name}._cdf_length", (0,), "int32")
        self.buffer(f"{name}.target", (3,))
        self.buffer(f"{name}.likelihood_lower_bound.bound", (1,))

    # entropy_models.py:462-485
    def gaussian_conditional(self, name: str):
        self.buffer(f"{name}._offset", (0,), "int32")
        self.buffer(f"{name}._quantized_cdf", (0,), "int32")
        self.buffer(f"{name}._cdf_length", (0,), "int32")
        self.buffer(f"{name}.scale_table", (0,))
        self.buffer(f"{name}.scale_bound", (1,))
        self.buffer(f"{name}.likelihood_lower_bound.bound", (1,))
        self.buffer(f"{name}.lower_bound_scale.bound", (1,))

    # nn.Linear / nn.LayerNorm / Swin pieces of models/stf_united.py
    def linear(self, name: str, cin: int, cout: int, bias: bool = True):
        self.entries[f"{name}.weight"] = Entry((cout, cin), "linear_w", fan_in=cin)
        if bias:
            self.entries[f"{name}.bias"] = Entry((cout,), "bias", fan_in=cin)

    def layernorm(self, name: str, c: int):
        self.entries[f"{name}.weight"] = Entry((c,), "ln_w")
        self.entries[f"{name}.bias"] = Entry((c,), "ln_b")

    # stf_united.py:118-214 (window 4x4: 49 relative offsets; relative_position_index is a registered buffer)
    def swin_block(self, name: str, dim: int, heads: int, window: int = 4, mlp_ratio: int = 4):
        self.layernorm(f"{name}.norm1", dim)
        self.entries[f"{name}.attn.relative_position_bias_table"] = Entry(((2 * window - 1) ** 2, heads), "rpb_table")
        self.buffer(f"{name}.attn.relative_position_index", (window * window, window * window), "int64")
        self.linear(f"{name}.attn.qkv", dim, 3 * dim)
        self.linear(f"{name}.attn.proj", dim, dim)
        self.layernorm(f"{name}.norm2", dim)
        self.linear(f"{name}.mlp.fc1", dim, mlp_ratio * dim)
        self.linear(f"{name}.mlp.fc2", mlp_ratio * dim, dim)

    def buffer(self, name: str, shape, dtype: str = "float32"):
        self.entries[name] = Entry(tuple(shape), "buffer", dtype=dtype, is_param=False)


def slice_offsets(slice_ch: List[int]) -> List[int]:
    out, acc = [], 0
    for c in slice_ch:
        out.append(acc)
        acc += c
    return out


def entropy_param_in_dims(M: int, slice_ch: List[int], i: int) -> Dict[str, int]:
    """Input widths of the four EntropyParametersEX nets of slice i (models/elic_united.py:53-78)."""
    c = slice_ch[i]
    base = 4 * M
    if i == 0:
        return {"rgb_anchor": base, "depth_anchor": base + 2 * c, "rgb_nonanchor": base + 4 * c,
                "depth_nonanchor": base + 4 * c}
    return {"rgb_anchor": base + 4 * c, "depth_anchor": base + 6 * c, "rgb_nonanchor": base + 8 * c,
            "depth_nonanchor": base + 8 * c}


def elic_united_entries(config=None) -> "OrderedDict[str, Entry]":
    """Every state_dict entry of ELIC_united, in a stable order."""
    cfg = model_config() if config is None else config
    N, M = int(cfg["N"]), int(cfg["M"])
    slice_ch = list(cfg["slice_ch"])
    b = _Builder()

    # g_a: modules/transform/analysis.py:116-159
    for mod, cin in (("rgb", 3), ("depth", 1)):
        p = f"g_a.{mod}_analysis_transform"
        b.conv(f"{p}.0", cin, N, 5)
        for j in (1, 2, 3):
            b.bottleneck(f"{p}.{j}", N)
        if mod == "rgb":
            b.bi_spf(f"{p}.4", N)
        b.conv(f"{p}.5", 2 * N, N, 5)
        for j in (6, 7, 8):
            b.bottleneck(f"{p}.{j}", N)
        b.attention(f"{p}.9", N)
        if mod == "rgb":
            b.bi_spf(f"{p}.10", N)
        b.conv(f"{p}.11", 2 * N, N, 5)
        for j in (12, 13, 14):
            b.bottleneck(f"{p}.{j}", N)
        if mod == "rgb":
            b.bi_spf(f"{p}.15", N)
        b.conv(f"{p}.16", 2 * N, M, 5)
        b.attention(f"{p}.17", M)

    # g_s: modules/transform/synthesis.py:126-169
    for mod, cout in (("rgb", 3), ("depth", 1)):
        p = f"g_s.{mod}_synthesis_transform"
        b.attention(f"{p}.0", M)
        b.deconv(f"{p}.1", M, N, 5)
        if mod == "rgb":
            b.bi_spf(f"{p}.2", N)
        b.bottleneck(f"{p}.3", 2 * N, N)
        b.bottleneck(f"{p}.4", N)
        b.bottleneck(f"{p}.5", N)
        b.deconv(f"{p}.6", N, N, 5)
        b.attention(f"{p}.7", N)
        if mod == "rgb":
            b.bi_spf(f"{p}.8", N)
        b.bottleneck(f"{p}.9", 2 * N, N)
        b.bottleneck(f"{p}.10", N)
        b.bottleneck(f"{p}.11", N)
        b.deconv(f"{p}.12", N, N, 5)
        if mod == "rgb":
            b.bi_spf(f"{p}.13", N)
        b.bottleneck(f"{p}.14", 2 * N, N)
        b.bottleneck(f"{p}.15", N)
        b.bottleneck(f"{p}.16", N)
        b.deconv(f"{p}.17", N, cout, 5)

    # h_a: analysis.py:231-237
    for mod in ("rgb", "depth"):
        p = f"h_a.{mod}_reduction"
        b.conv(f"{p}.0", M, N, 3)
        b.conv(f"{p}.2", N, N, 5)
        b.conv(f"{p}.4", N, N, 5)

    # h_s: synthesis.py:305-314, 345-354
    for m in ("r", "d"):
        for idx, (cin, cout, k) in enumerate(((2 * N, M, 5), (2 * M, M * 3 // 2, 5), (3 * M, 2 * M, 3)), 1):
            p = f"h_s.{m}_h_s{idx}"
            b.se(f"{p}.se", cin)
            b.deconv(f"{p}.deconv", cin, cout, k)

    # Bi-CEE nets: models/elic_united.py:30-78
    for fam in ("rgb_local_context", "rgb_local_context_anchor_with_nonanchor", "depth_local_context"):
        for i, c in enumerate(slice_ch):
            b.conv(f"{fam}.{i}", c, 2 * c, 5)
    for fam in ("rgb_channel_context", "depth_channel_context"):
        for i in range(1, len(slice_ch)):
            b.channel_context(f"{fam}.{i}", sum(slice_ch[:i]), 2 * slice_ch[i])
    for i, c in enumerate(slice_ch):
        dims = entropy_param_in_dims(M, slice_ch, i)
        b.entropy_params(f"rgb_entropy_parameters_anchor.{i}", dims["rgb_anchor"], 2 * c)
    for i, c in enumerate(slice_ch):
        dims = entropy_param_in_dims(M, slice_ch, i)
        b.entropy_params(f"depth_entropy_parameters_anchor.{i}", dims["depth_anchor"], 2 * c)
    for i, c in enumerate(slice_ch):
        dims = entropy_param_in_dims(M, slice_ch, i)
        b.entropy_params(f"rgb_entropy_parameters_nonanchor.{i}", dims["rgb_nonanchor"], 2 * c)
    for i, c in enumerate(slice_ch):
        dims = entropy_param_in_dims(M, slice_ch, i)
        b.entropy_params(f"depth_entropy_parameters_nonanchor.{i}", dims["depth_nonanchor"], 2 * c)

    b.entropy_bottleneck("rgb_entropy_bottleneck", N)
    b.entropy_bottleneck("depth_entropy_bottleneck", N)
    b.gaussian_conditional("rgb_gaussian_conditional")
    b.gaussian_conditional("depth_gaussian_conditional")
    return b.entries


def elic_entries(config=None, channel: int = 3) -> "OrderedDict[str, Entry]":
    """Every state_dict entry of the single-modal ELIC (reference: models/elic.py:15-57; 409 tensors, 36,932,427
    parameters for channel=3) -- BASELINE config 1 / SURVEY §8f rank 4."""
    cfg = model_config() if config is None else config
    N, M = int(cfg["N"]), int(cfg["M"])
    slice_ch = list(cfg["slice_ch"])
    b = _Builder()
    # modules/transform/analysis.py:29-52
    p = "g_a.analysis_transform"
    b.conv(f"{p}.0", channel, N, 5)
    for j in (1, 2, 3, 5, 6, 7, 10, 11, 12):
        b.bottleneck(f"{p}.{j}", N)
    b.conv(f"{p}.4", N, N, 5)
    b.attention(f"{p}.8", N)
    b.conv(f"{p}.9", N, N, 5)
    b.conv(f"{p}.13", N, M, 5)
    b.attention(f"{p}.14", M)
    # modules/transform/synthesis.py:32-51
    p = "g_s.synthesis_transform"
    b.attention(f"{p}.0", M)
    b.deconv(f"{p}.1", M, N, 5)
    for j in (2, 3, 4, 7, 8, 9, 11, 12, 13):
        b.bottleneck(f"{p}.{j}", N)
    b.deconv(f"{p}.5", N, N, 5)
    b.attention(f"{p}.6", N)
    b.deconv(f"{p}.10", N, N, 5)
    b.deconv(f"{p}.14", N, channel, 5)
    # analysis.py:207-216, synthesis.py:276-285
    b.conv("h_a.reduction.0", M, N, 3)
    b.conv("h_a.reduction.2", N, N, 5)
    b.conv("h_a.reduction.4", N, N, 5)
    b.deconv("h_s.increase.0", N, M, 5)
    b.deconv("h_s.increase.2", M, M * 3 // 2, 5)
    b.deconv("h_s.increase.4", M * 3 // 2, 2 * M, 3)
    # models/elic.py:32-53; EntropyParameters (entropy.py:7-17) is three 1x1 convolutions
    for i, c in enumerate(slice_ch):
        b.conv(f"local_context.{i}", c, 2 * c, 5)
    for i in range(1, len(slice_ch)):
        b.channel_context(f"channel_context.{i}", sum(slice_ch[:i]), 2 * slice_ch[i])
    for fam, extra in (("entropy_parameters_anchor", 0), ("entropy_parameters_nonanchor", 2)):
        for i, c in enumerate(slice_ch):
            in_dim, out = 2 * M + (extra + (2 if i else 0)) * c, 2 * c
            b.conv(f"{fam}.{i}.fusion.0", in_dim, out * 5 // 3, 1)
            b.conv(f"{fam}.{i}.fusion.2", out * 5 // 3, out * 4 // 3, 1)
            b.conv(f"{fam}.{i}.fusion.4", out * 4 // 3, out, 1)
    b.entropy_bottleneck("entropy_bottleneck", N)
    b.gaussian_conditional("gaussian_conditional")
    return b.entries


def r2d_entropy_param_in_dims(M: int, slice_ch: List[int], i: int) -> Dict[str, int]:
    """models/elic_united_R2D.py:47-71: the RGB nets see RGB context only, the depth nets see both."""
    c = slice_ch[i]
    if i == 0:
        return {"rgb_anchor": 2 * M, "depth_anchor": 4 * M + 2 * c, "rgb_nonanchor": 2 * M + 2 * c,
                "depth_nonanchor": 4 * M + 4 * c}
    return {"rgb_anchor": 2 * M + 2 * c, "depth_anchor": 4 * M + 6 * c, "rgb_nonanchor": 2 * M + 4 * c,
            "depth_nonanchor": 4 * M + 8 * c}


def elic_united_r2d_entries(config=None) -> "OrderedDict[str, Entry]":
    """Every state_dict entry of ELIC_united_R2D (reference: models/elic_united_R2D.py:9-71): the one-directional variant
    (RGB is coded on its own, depth is conditioned on RGB) -- SURVEY 8f rank 4."""
    cfg = model_config() if config is None else config
    N, M = int(cfg["N"]), int(cfg["M"])
    slice_ch = list(cfg["slice_ch"])
    b = _Builder()

    def spf_single(name, n):  # modules/transform/attention.py:14-32
        b.conv(f"{name}.r_ext", n, n // 2, 3)
        b.conv(f"{name}.d_ext", n, n // 2, 3)
        b.esa(f"{name}.d_esa", n)

    # analysis.py:56-112: the RGB stream never takes depth features; the depth stream concatenates the fused ones
    for mod, cin, k in (("rgb", 3, 1), ("depth", 1, 2)):
        p = f"g_a.{mod}_analysis_transform"
        b.conv(f"{p}.0", cin, N, 5)
        for j in (1, 2, 3, 6, 7, 8, 12, 13, 14):
            b.bottleneck(f"{p}.{j}", N)
        for j in (4, 10, 15):
            if mod == "rgb":
                spf_single(f"{p}.{j}", N)
        b.conv(f"{p}.5", k * N, N, 5)
        b.attention(f"{p}.9", N)
        b.conv(f"{p}.11", k * N, N, 5)
        b.conv(f"{p}.16", k * N, M, 5)
        b.attention(f"{p}.17", M)
    # synthesis.py:186-242
    for mod, cout, k in (("rgb", 3, 1), ("depth", 1, 2)):
        p = f"g_s.{mod}_synthesis_transform"
        b.attention(f"{p}.0", M)
        b.deconv(f"{p}.1", M, N, 5)
        for j in (2, 8, 13):
            if mod == "rgb":
                spf_single(f"{p}.{j}", N)
        for j in (3, 9, 14):
            b.bottleneck(f"{p}.{j}", k * N, N)
        for j in (4, 5, 10, 11, 15, 16):
            b.bottleneck(f"{p}.{j}", N)
        b.deconv(f"{p}.6", N, N, 5)
        b.attention(f"{p}.7", N)
        b.deconv(f"{p}.12", N, N, 5)
        b.deconv(f"{p}.17", N, cout, 5)
    for mod in ("rgb", "depth"):  # analysis.py:231-237 (HyperAnalysisEXcross, as in ELIC_united)
        p = f"h_a.{mod}_reduction"
        b.conv(f"{p}.0", M, N, 3)
        b.conv(f"{p}.2", N, N, 5)
        b.conv(f"{p}.4", N, N, 5)
    # synthesis.py:325-380: RGB hyper synthesis on its own, depth on (depth, rgb)
    for m, mult in (("r", 1), ("d", 2)):
        for idx, (cin, cout, k) in enumerate(((N, M, 5), (M, M * 3 // 2, 5), (M * 3 // 2, 2 * M, 3)), 1):
            p = f"h_s.{m}_h_s{idx}"
            b.se(f"{p}.se", mult * cin)
            b.deconv(f"{p}.deconv", mult * cin, cout, k)
    for fam in ("rgb_local_context", "rgb_local_context_anchor_with_nonanchor", "depth_local_context"):
        for i, c in enumerate(slice_ch):
            b.conv(f"{fam}.{i}", c, 2 * c, 5)
    for fam in ("rgb_channel_context", "depth_channel_context"):
        for i in range(1, len(slice_ch)):
            b.channel_context(f"{fam}.{i}", sum(slice_ch[:i]), 2 * slice_ch[i])
    for fam, key in (("rgb_entropy_parameters_anchor", "rgb_anchor"), ("depth_entropy_parameters_anchor", "depth_anchor"),
                     ("rgb_entropy_parameters_nonanchor", "rgb_nonanchor"),
                     ("depth_entropy_parameters_nonanchor", "depth_nonanchor")):
        for i, c in enumerate(slice_ch):
            b.entropy_params(f"{fam}.{i}", r2d_entropy_param_in_dims(M, slice_ch, i)[key], 2 * c)
    b.entropy_bottleneck("rgb_entropy_bottleneck", N)
    b.entropy_bottleneck("depth_entropy_bottleneck", N)
    b.gaussian_conditional("rgb_gaussian_conditional")
    b.gaussian_conditional("depth_gaussian_conditional")
    return b.entries


STF_DEPTHS = (2, 2, 6, 2)
STF_HEADS = (3, 6, 12, 24)
STF_EMBED = 48


def stf_config() -> Config:
    """models/stf_united.py:638-640: the Swin variant overrides N, M and the slice widths."""
    cfg = model_config()
    cfg["N"], cfg["M"], cfg["slice_ch"] = 192, 384, [24, 24, 48, 96, 192]
    return cfg


def stf_united_entries(config=None) -> "OrderedDict[str, Entry]":
    """Every state_dict entry of STF_united (reference: models/stf_united.py:403-678; 1440 tensors): the Swin analysis /
    synthesis transforms plus ELIC_united's hyper and entropy nets at N=192, M=384, slices [24,24,48,96,192]."""
    cfg = stf_config()
    base = elic_united_entries(cfg)
    b = _Builder()
    E, depths, heads = STF_EMBED, STF_DEPTHS, STF_HEADS
    # analysis: stf_united.py:403-502
    for mod, cin in (("rgb", 3), ("depth", 1)):
        b.conv(f"g_a.{mod}_patch_embed.proj", cin, E, 2)
        b.layernorm(f"g_a.{mod}_patch_embed.norm", E)
    for mod in ("rgb", "depth"):
        dim, li = E, 0
        for i in range(4):
            p = f"g_a.{mod}_ana_layers.{li}"
            for k in range(depths[i]):
                b.swin_block(f"{p}.blocks.{k}", dim, heads[i])
            if i < 3:
                b.linear(f"{p}.downsample.reduction", 4 * dim, 2 * dim, bias=False)
                b.layernorm(f"{p}.downsample.norm", 4 * dim)
            dim *= 2
            li += 1
            if i < 3:
                if mod == "rgb":
                    b.bi_spf(f"g_a.rgb_ana_layers.{li}", dim)
                li += 1
    # synthesis: stf_united.py:505-602
    for mod, cout in (("rgb", 3), ("depth", 1)):
        dim, li = 8 * E, 0
        for i in range(4):
            p = f"g_s.{mod}_syn_layers.{li}"
            for k in range(depths[3 - i]):
                b.swin_block(f"{p}.blocks.{k}", dim, heads[3 - i])
            if i < 3:
                b.linear(f"{p}.downsample.reduction", dim, 2 * dim, bias=False)
                b.layernorm(f"{p}.downsample.norm", dim)
            dim //= 2
            li += 1
            if i < 3:
                if mod == "rgb":
                    b.bi_spf(f"g_s.rgb_syn_layers.{li}", dim)
                li += 1
        b.conv(f"g_s.{mod}_end_conv.0", E, 4 * E, 5)
        b.conv(f"g_s.{mod}_end_conv.2", E, cout, 3)
    out = OrderedDict(b.entries)
    for k, v in base.items():
        if not k.startswith(("g_a.", "g_s.")):
            out[k] = v
    return out


STF_SLICES = 12        # models/stf.py:418 (num_slices); 384 / 12 = 32 channels per slice
STF_SUPPORT_SLICES = 6  # stf.py:439 (max_support_slices = num_slices // 2)


def stf_single_config() -> Config:
    """The fixed widths of the single-modal STF (models/stf.py:431, 630): N = 192 hyper channels, M = 384 latent channels
    in 12 raster slices of 32."""
    cfg = model_config()
    cfg["N"], cfg["M"] = 4 * STF_EMBED, 8 * STF_EMBED
    cfg["slice_num"], cfg["slice_ch"] = STF_SLICES, [8 * STF_EMBED // STF_SLICES] * STF_SLICES
    return cfg


def stf_entries(channel: int = 3) -> "OrderedDict[str, Entry]":
    """Every state_dict entry of the single-modal STF (reference: models/stf.py:408-585, SymmetricalTransFormer; 779 tensors,
    99,855,639 parameters for channel=3): Swin analysis / synthesis transforms, a hyper analysis of five 3x3 convolutions,
    two hyper-synthesis nets, and per slice two parameter nets plus the latent-residual-prediction net."""
    b = _Builder()
    E, depths, heads = STF_EMBED, STF_DEPTHS, STF_HEADS
    M, C = 8 * E, 8 * E // STF_SLICES
    b.conv("patch_embed.proj", channel, E, 2)
    b.layernorm("patch_embed.norm", E)
    dim = E
    for i in range(4):  # stf.py:454-472
        for k in range(depths[i]):
            b.swin_block(f"layers.{i}.blocks.{k}", dim, heads[i])
        if i < 3:
            b.linear(f"layers.{i}.downsample.reduction", 4 * dim, 2 * dim, bias=False)
            b.layernorm(f"layers.{i}.downsample.norm", 4 * dim)
            dim *= 2
    for i in range(4):  # stf.py:474-494
        for k in range(depths[3 - i]):
            b.swin_block(f"syn_layers.{i}.blocks.{k}", dim, heads[3 - i])
        if i < 3:
            b.linear(f"syn_layers.{i}.downsample.reduction", dim, 2 * dim, bias=False)
            b.layernorm(f"syn_layers.{i}.downsample.norm", dim)
            dim //= 2
    b.conv("end_conv.0", E, 4 * E, 5)  # stf.py:496-500
    b.conv("end_conv.2", E, channel, 3)
    for j, (cin, cout) in enumerate(((384, 384), (384, 336), (336, 288), (288, 240), (240, 192))):  # stf.py:507-517
        b.conv(f"h_a.{2 * j}", cin, cout, 3)
    for fam in ("h_mean_s", "h_scale_s"):  # stf.py:519-540; subpel_conv3x3 = Sequential(conv to 4 C channels, PixelShuffle)
        b.conv(f"{fam}.0", 192, 240, 3)
        b.conv(f"{fam}.2.0", 240, 288 * 4, 3)
        b.conv(f"{fam}.4", 288, 336, 3)
        b.conv(f"{fam}.6.0", 336, 384 * 4, 3)
        b.conv(f"{fam}.8", 384, 384, 3)
    for fam, extra in (("cc_mean_transforms", 0), ("cc_scale_transforms", 0), ("lrp_transforms", 1)):  # stf.py:541-582
        for i in range(STF_SLICES):
            cin = M + C * min(i + extra, STF_SUPPORT_SLICES + extra)
            for j, (a, o) in enumerate(((cin, 224), (224, 176), (176, 128), (128, 64), (64, C))):
                b.conv(f"{fam}.{i}.{2 * j}", a, o, 3)
    b.entropy_bottleneck("entropy_bottleneck", 4 * E)
    b.gaussian_conditional("gaussian_conditional")
    return b.entries


ALIGNER_EMBED, ALIGNER_HEADS = 96, 3  # modules/transform/spatialAligner.py:344-348 (window 4, patch 2)


def spatial_aligner_entries(in_ch: int = 192, out_ch: int = 192, prefix: str = "") -> "OrderedDict[str, Entry]":
    """Every state_dict entry of Spatial_aligner (reference: modules/transform/spatialAligner.py:341-374), in the reference's
    order: two 2x2 stride-2 patch embeddings, two Swin blocks with a cross attention (qkv1 for the query, qkv2 for key and
    value, :130-132) and the 2x2 stride-2 transposed convolution `recovery`.  prefix: "" or the block's name inside a model
    (e.g. "g_s.sp1")."""
    b = _Builder()
    p = f"{prefix}." if prefix else ""
    E = ALIGNER_EMBED
    b.conv(f"{p}patch_embeding1", in_ch, E, 2)
    b.conv(f"{p}patch_embeding2", in_ch, E, 2)
    for k in range(2):
        n = f"{p}blocks.{k}"
        b.layernorm(f"{n}.norm1", E)
        b.entries[f"{n}.attn.relative_position_bias_table"] = Entry((49, ALIGNER_HEADS), "rpb_table")
        b.buffer(f"{n}.attn.relative_position_index", (16, 16), "int64")
        b.linear(f"{n}.attn.qkv1", E, E)
        b.linear(f"{n}.attn.qkv2", E, 2 * E)
        b.linear(f"{n}.attn.proj", E, E)
        b.layernorm(f"{n}.norm2", E)
        b.linear(f"{n}.mlp.fc1", E, 4 * E)
        b.linear(f"{n}.mlp.fc2", 4 * E, E)
    b.deconv(f"{p}recovery", E, out_ch, 2)
    return b.entries


def synthesis_plus_entries(N: int = 192, M: int = 320, ch: int = 3) -> "OrderedDict[str, Entry]":
    """Every state_dict entry of SynthesisTransformPlus (reference: modules/transform/synthesis.py:74-96), in the reference's
    order: the g_s rows of elic_entries under `synthesis_transform.` (the last transposed convolution to `ch` channels), then
    sp1, sp2, sp3 -- Spatial_aligner() with its default 192 channels whatever N is, so only N = 192 gives a module that runs."""
    cfg = model_config()
    cfg["N"], cfg["M"] = int(N), int(M)
    p = "g_s.synthesis_transform."
    rows = [(name, e) for name, e in elic_entries(cfg, channel=int(ch)).items() if name.startswith(p)]
    rows.sort(key=lambda r: int(r[0][len(p):].split(".")[0]))  # (stable: stage by stage, each stage in its own order)
    out: "OrderedDict[str, Entry]" = OrderedDict((name[len("g_s."):], e) for name, e in rows)
    for k in (1, 2, 3):
        out.update(spatial_aligner_entries(prefix=f"sp{k}"))
    return out


def local_context_entries(dim: int = 32, window_size: int = 5, mlp_ratio: float = 2.0, num_heads: int = 2,
                          qkv_bias: bool = True) -> "OrderedDict[str, Entry]":
    """Every state_dict entry of MLIC++'s LocalContext (reference: modules/transform/context.py:33-56), in the reference's
    order: the module's own table and index buffer, then qkv_proj, proj, mlp, the two LayerNorms and the window-sized `fusion`."""
    b = _Builder()
    b.entries["relative_position_table"] = Entry(((2 * window_size - 1) ** 2, num_heads), "rpb_table")
    b.buffer("relative_position_index", (window_size ** 2, window_size ** 2), "int64")
    b.linear("qkv_proj", dim, 3 * dim, qkv_bias)
    b.linear("proj", 2 * dim, 2 * dim)
    b.linear("mlp.fc1", 2 * dim, int(2 * dim * mlp_ratio))
    b.linear("mlp.fc2", int(2 * dim * mlp_ratio), 2 * dim)
    b.layernorm("norm1", dim)
    b.layernorm("norm2", 2 * dim)
    b.conv("fusion", dim, 2 * dim, window_size)
    return b.entries


def _linear_context_entries(dim: int, mid: int, hidden: int, out: int, skip: bool) -> "OrderedDict[str, Entry]":
    b = _Builder()

    def dw(name, c):  # nn.Conv2d(c, c, 3, 1, 1, groups=c): weight [c][1][3][3]
        b.conv(name, 1, c, 3)

    for n in ("keys", "queries", "values"):
        b.conv(f"{n}.0", dim, dim, 1)
        dw(f"{n}.1", dim)
    b.conv("reprojection", dim, mid, 5)
    b.conv("mlp.0", mid, hidden, 1)
    dw("mlp.2", hidden)
    b.conv("mlp.4", hidden, out, 1)
    if skip:
        b.conv("skip", mid, out, 1)
    return b.entries


def linear_global_intra_entries(dim: int = 32) -> "OrderedDict[str, Entry]":
    """LinearGlobalIntraContext (context.py:163-187): keys / queries / values = 1x1 + depthwise 3x3, a 5x5 reprojection to
    2 dim and the 1x1 / depthwise / 1x1 mlp."""
    return _linear_context_entries(dim, 2 * dim, 4 * dim, 2 * dim, False)


def linear_global_inter_entries(dim: int = 32, out_dim: int = 64) -> "OrderedDict[str, Entry]":
    """LinearGlobalInterContext (context.py:216-241): as the intra context with a reprojection to 3/2 out_dim, an mlp over
    2 out_dim and the 1x1 `skip`."""
    return _linear_context_entries(dim, out_dim * 3 // 2, 2 * out_dim, out_dim, True)


MLIC_PARAM_HIDDEN = (320, 256, 128)  # modules/transform/entropy.py:35-41
MLIC_CHANNEL_HIDDEN = (192, 128)     # modules/transform/context.py:144-148


def entropy_params_mlic_entries(in_dim: int = 640, out_dim: int = 64) -> "OrderedDict[str, Entry]":
    """EntropyParametersMLIC (reference: modules/transform/entropy.py:31-41): four 1x1 convolutions, `fusion.{0,2,4,6}`."""
    b = _Builder()
    widths = (in_dim,) + MLIC_PARAM_HIDDEN + (out_dim,)
    for i in range(4):
        b.conv(f"fusion.{2 * i}", widths[i], widths[i + 1], 1)
    return b.entries


def channel_context_entries(in_dim: int = 32, out_dim: int = 32) -> "OrderedDict[str, Entry]":
    """MLIC++'s ChannelContext (context.py:140-150): three 3x3 convolutions to 4 out_dim channels, `fushion.{0,2,4}` (the
    reference's spelling)."""
    b = _Builder()
    widths = (in_dim,) + MLIC_CHANNEL_HIDDEN + (4 * out_dim,)
    for i in range(3):
        b.conv(f"fushion.{2 * i}", widths[i], widths[i + 1], 3)
    return b.entries


def lrp_widths(in_dim: int, out_dim: int) -> List[int]:
    """Channel counts of LatentResidualPrediction (modules/transform/LRP.py:12-21), input first: the reference's integer
    divisions as it writes them (diff * 3 // 4, not 3 * (diff // 4))."""
    diff = abs(out_dim - in_dim)
    return [in_dim, in_dim - diff // 4, in_dim - diff // 2, in_dim - diff * 3 // 4, out_dim]


def lrp_entries(in_dim: int = 352, out_dim: int = 32) -> "OrderedDict[str, Entry]":
    """LatentResidualPrediction (LRP.py:9-21): four 3x3 convolutions, `lrp_transform.{0,2,4,6}`."""
    b = _Builder()
    widths = lrp_widths(in_dim, out_dim)
    for i in range(4):
        b.conv(f"lrp_transform.{2 * i}", widths[i], widths[i + 1], 3)
    return b.entries


CHALIGN_IN, CHALIGN_MID, CHALIGN_OUT = 64, 256, 64  # modules/transform/channelAligner.py:9-20: constants of the reference


def channel_aligner_entries() -> "OrderedDict[str, Entry]":
    """Every state_dict entry of Channel_aligner (reference: modules/transform/channelAligner.py:5-22), in the reference's
    order: the trunk conv1 (four 3x3 convolutions 64 -> 256 -> 256 -> 256 -> 256 at indexes 0, 2, 4, 6 of a Sequential, a
    LeakyReLU behind each) and the two 3x3 heads conv2 (beta) and conv3 (gamma), 256 -> 64.  The pools have no state."""
    b = _Builder()
    for i, cin in zip((0, 2, 4, 6), (CHALIGN_IN, CHALIGN_MID, CHALIGN_MID, CHALIGN_MID)):
        b.conv(f"conv1.{i}", cin, CHALIGN_MID, 3)
    b.conv("conv2", CHALIGN_MID, CHALIGN_OUT, 3)
    b.conv("conv3", CHALIGN_MID, CHALIGN_OUT, 3)
    return b.entries


FEATURE_CH = 64  # the width Feature_encoder / Feature_decoder hard-code inside (models/elic_master.py:19-21, 38-41)


def _feature_resblocks(b: "_Builder", in_ch: int):
    for i, cin in zip((1, 2, 3), (in_ch, FEATURE_CH, FEATURE_CH)):
        b.conv(f"resblock{i}.conv1", cin, FEATURE_CH, 3)
        b.conv(f"resblock{i}.conv2", FEATURE_CH, FEATURE_CH, 3)
        if cin != FEATURE_CH:  # ResidualBlock.skip exists only where the widths differ (modules/layers/res_blk.py:43-46)
            b.conv(f"resblock{i}.skip", cin, FEATURE_CH, 1)


def feature_encoder_entries(in_ch: int = 3) -> "OrderedDict[str, Entry]":
    """Every state_dict entry of Feature_encoder (reference: models/elic_master.py:15-21), in the reference's order: conv1
    (3x3, in_ch -> 64) and three ResidualBlock(64, 64)."""
    b = _Builder()
    b.conv("conv1", in_ch, FEATURE_CH, 3)
    _feature_resblocks(b, FEATURE_CH)
    return b.entries


def feature_decoder_entries(in_ch: int = 64, out_ch: int = 3) -> "OrderedDict[str, Entry]":
    """Every state_dict entry of Feature_decoder (reference: models/elic_master.py:34-42), in the reference's order:
    ResidualBlock(in_ch, 64) -- with its 1x1 `skip` unless in_ch is 64 --, two ResidualBlock(64, 64), deconv1
    (ConvTranspose2d(64, out_ch, 3, 1, 1)) and the 1x1 shortcut `conv` (in_ch -> 64)."""
    b = _Builder()
    _feature_resblocks(b, in_ch)
    b.deconv("deconv1", FEATURE_CH, out_ch, 3)
    b.conv("conv", in_ch, FEATURE_CH, 1)
    return b.entries


MASTER_OUTER_PREFIXES = ("aux_encoder.", "master_encoder.", "master_decoder.", "channel_aligner.")  # models/elic_master.py:104-107


def elic_master_entries(config=None, channel: int = 3) -> "OrderedDict[str, Entry]":
    """Every state_dict entry of ELIC_master (reference: models/elic_master.py:56-107), in the reference's order: the entropy
    bottleneck (CompressionModel registers it first), g_a = AnalysisTransformEX(N, M, ch = 128), g_s = SynthesisTransformPlus(N,
    M, ch = N), ELIC's h_a / h_s, local and channel contexts, the EntropyParametersEX nets (widths 2M + 2c / 2M + 4c, without
    the channel context for slice 0), the Gaussian conditional, and the four outer blocks: aux_encoder (1 channel for a
    3-channel master image and the other way round), master_encoder, master_decoder (N + 64 -> channel) and channel_aligner."""
    if channel not in (1, 3):
        raise ValueError(f"channel must be 3 or 1 (models/elic_master.py:100-103), got {channel}")
    cfg = model_config() if config is None else config
    N, M = int(cfg["N"]), int(cfg["M"])
    slice_ch = list(cfg["slice_ch"])
    elic = elic_entries(cfg, channel=2 * FEATURE_CH)  # (cat([fv, fv_bar]), :67, 113)
    b = _Builder()
    b.entropy_bottleneck("entropy_bottleneck", N)
    p = "g_a.analysis_transform."
    rows = [(name, e) for name, e in elic.items() if name.startswith(p)]
    rows.sort(key=lambda r: int(r[0][len(p):].split(".")[0]))  # (stable: stage by stage, each stage in its own order)
    b.entries.update(rows)
    _prefixed(b, "g_s.", synthesis_plus_entries(N, M, ch=N))
    b.entries.update((name, e) for name, e in elic.items() if name.startswith(("h_a.", "h_s.", "local_context.", "channel_context.")))
    for fam, extra in (("entropy_parameters_anchor", 0), ("entropy_parameters_nonanchor", 2)):
        for i, c in enumerate(slice_ch):
            b.entropy_params(f"{fam}.{i}", 2 * M + (extra + (2 if i else 0)) * c, 2 * c)
    b.gaussian_conditional("gaussian_conditional")
    _prefixed(b, "aux_encoder.", feature_encoder_entries(1 if channel == 3 else 3))
    _prefixed(b, "master_encoder.", feature_encoder_entries(channel))
    _prefixed(b, "master_decoder.", feature_decoder_entries(N + FEATURE_CH, channel))
    _prefixed(b, "channel_aligner.", channel_aligner_entries())
    return b.entries


def elic_master_latent_entries(config=None) -> "OrderedDict[str, Entry]":
    """elic_master_entries without the outer blocks: what rgbd_amd.MasterLatentCodec holds (the image's channel count only
    shapes the outer blocks)."""
    return OrderedDict((name, e) for name, e in elic_master_entries(config, 3).items() if not name.startswith(MASTER_OUTER_PREFIXES))


def ckbd_config(N: int = 192) -> Config:
    """Cheng2020 anchor model with the checkerboard context (models/Cheng2020withCKBD.py:46-50): M = N, one slice."""
    cfg = model_config()
    cfg["N"], cfg["M"], cfg["slice_num"], cfg["slice_ch"] = int(N), int(N), 1, [int(N)]
    return cfg


def ckbd_entries(N: int = 192, channel: int = 3) -> "OrderedDict[str, Entry]":
    """Every state_dict entry of Cheng2020AnchorwithCheckerboard (reference: models/Cheng2020withCKBD.py:40-50 on
    CompressAI/compressai/models/waseda.py:22-81; 160 tensors, 26,598,956 parameters for N=192, channel=3): residual blocks
    of 3x3 / 1x1 convolutions with GDN / IGDN, sub-pixel up-sampling, three 1x1 entropy-parameter layers and the 5x5
    checkerboard context convolution (its mask is a buffer; the state_dict holds the unmasked weight)."""
    b = _Builder()
    b.entropy_bottleneck("entropy_bottleneck", N)

    def gdn(name):  # layers/gdn.py:35-50, ops/parametrizers.py:28-37
        b.entries[f"{name}.beta"] = Entry((N,), "gdn_beta")
        b.entries[f"{name}.gamma"] = Entry((N, N), "gdn_gamma")
        for r in ("beta_reparam", "gamma_reparam"):
            b.buffer(f"{name}.{r}.pedestal", (1,))
            b.buffer(f"{name}.{r}.lower_bound.bound", (1,))

    def res_block(name):  # layers.py:129-159
        b.conv(f"{name}.conv1", N, N, 3)
        b.conv(f"{name}.conv2", N, N, 3)

    for i in range(3):  # waseda.py:38-46
        cin = channel if i == 0 else N
        p = f"g_a.{2 * i}"  # ResidualBlockWithStride, layers.py:67-98
        b.conv(f"{p}.conv1", cin, N, 3)
        b.conv(f"{p}.conv2", N, N, 3)
        gdn(f"{p}.gdn")
        b.conv(f"{p}.skip", cin, N, 1)
        res_block(f"g_a.{2 * i + 1}")
    b.conv("g_a.6", N, N, 3)
    for i in range(3):  # waseda.py:72-81
        res_block(f"g_s.{2 * i}")
        p = f"g_s.{2 * i + 1}"  # ResidualBlockUpsample, layers.py:101-126
        b.conv(f"{p}.subpel_conv.0", N, 4 * N, 3)
        b.conv(f"{p}.conv", N, N, 3)
        gdn(f"{p}.igdn")
        b.conv(f"{p}.upsample.0", N, 4 * N, 3)
    res_block("g_s.6")
    b.conv("g_s.7.0", N, 4 * channel, 3)
    for k in range(5):  # waseda.py:48-58
        b.conv(f"h_a.{2 * k}", N, N, 3)
    b.conv("h_s.0", N, N, 3)  # waseda.py:60-70
    b.conv("h_s.2.0", N, 4 * N, 3)
    b.conv("h_s.4", N, N * 3 // 2, 3)
    b.conv("h_s.6.0", N * 3 // 2, 4 * (N * 3 // 2), 3)
    b.conv("h_s.8", N * 3 // 2, 2 * N, 3)
    b.gaussian_conditional("gaussian_conditional")
    M = N
    b.conv("entropy_parameters.0", M * 12 // 3, M * 10 // 3, 1)  # priors.py:403-409
    b.conv("entropy_parameters.2", M * 10 // 3, M * 8 // 3, 1)
    b.conv("entropy_parameters.4", M * 8 // 3, M * 6 // 3, 1)
    b.conv("context_prediction", M, 2 * M, 5)  # Cheng2020withCKBD.py:48-50
    b.buffer("context_prediction.mask", (2 * M, M, 5, 5))
    return b.entries


MLIC_SLICE_CH = 32  # LocalContext's kernel and the head counts slice_ch * i / 32 of the inter contexts (models/mlicpp.py:40-51)


def mlic_config(N: int = 192, M: int = 320, slice_num: int = 10) -> Config:
    """MLIC++ (config/config.py: N 192, M 320, ten slices of 32 channels, context window 5)."""
    if int(M) != MLIC_SLICE_CH * int(slice_num) or not 2 <= int(slice_num) <= 10 or int(N) % 16:
        raise ValueError(f"MLIC: M must be 32 * slice_num with 2 ... 10 slices and N a multiple of 16, got N={N}, M={M}, slice_num={slice_num}")
    cfg = model_config()
    cfg["N"], cfg["M"], cfg["slice_num"], cfg["slice_ch"] = int(N), int(M), int(slice_num), [MLIC_SLICE_CH] * int(slice_num)
    cfg["context_window"] = 5
    return cfg


def _prefixed(b: "_Builder", prefix: str, entries):
    for name, e in entries.items():
        b.entries[prefix + name] = e


def mlic_entries(N: int = 192, M: int = 320, slice_num: int = 10, channel: int = 3) -> "OrderedDict[str, Entry]":
    """Every state_dict entry of MLICPlusPlus (reference: models/mlicpp.py:15-75), in the reference's order: the entropy
    bottleneck, g_a / g_s (residual blocks with GDN / IGDN, modules/layers/res_blk.py:30-119), h_a / h_s, the Gaussian
    conditional, then per network kind the modules of slices 0 ... slice_num - 1 -- assembled from the per-module entry functions
    under the reference's prefixes.  channel_context, global_inter_context and global_intra_context hold None at i = 0."""
    C = M // slice_num
    b = _Builder()
    b.entropy_bottleneck("entropy_bottleneck", N)

    def gdn(name, c):  # layers/gdn.py:35-50, ops/parametrizers.py:28-37
        b.entries[f"{name}.beta"] = Entry((c,), "gdn_beta")
        b.entries[f"{name}.gamma"] = Entry((c, c), "gdn_gamma")
        for r in ("beta_reparam", "gamma_reparam"):
            b.buffer(f"{name}.{r}.pedestal", (1,))
            b.buffer(f"{name}.{r}.lower_bound.bound", (1,))

    def res_block(name, cin, cout):  # res_blk.py:30-58
        b.conv(f"{name}.conv1", cin, cout, 3)
        b.conv(f"{name}.conv2", cout, cout, 3)
        if cin != cout:
            b.conv(f"{name}.skip", cin, cout, 1)

    root = "g_a.analysis_transform"  # modules/transform/analysis.py:11-26
    for i in range(3):
        cin = channel if i == 0 else N
        p = f"{root}.{2 * i}"  # ResidualBlockWithStride, res_blk.py:61-91
        b.conv(f"{p}.conv1", cin, N, 3)
        b.conv(f"{p}.conv2", N, N, 3)
        gdn(f"{p}.gdn", N)
        b.conv(f"{p}.skip", cin, N, 1)
        res_block(f"{root}.{2 * i + 1}", N, N)
    b.conv(f"{root}.6", N, M, 3)
    root = "g_s.synthesis_transform"  # modules/transform/synthesis.py:12-29
    for i in range(3):
        res_block(f"{root}.{2 * i}", M if i == 0 else N, N)
        p = f"{root}.{2 * i + 1}"  # ResidualBlockUpsample, res_blk.py:94-119
        b.conv(f"{p}.subpel_conv.0", N, 4 * N, 3)
        b.conv(f"{p}.conv", N, N, 3)
        gdn(f"{p}.igdn", N)
        b.conv(f"{p}.upsample.0", N, 4 * N, 3)
    res_block(f"{root}.6", N, N)
    b.conv(f"{root}.7.0", N, 4 * channel, 3)
    for k, cin in zip(range(5), (M, N, N, N, N)):  # analysis.py:180-204
        b.conv(f"h_a.reduction.{2 * k}", cin, N, 3)
    M32 = M * 3 // 2
    b.conv("h_s.increase.0", N, M, 3)  # synthesis.py:248-273
    b.conv("h_s.increase.2.0", M, 4 * M, 3)
    b.conv("h_s.increase.4", M, M32, 3)
    b.conv("h_s.increase.6.0", M32, 4 * M32, 3)
    b.conv("h_s.increase.8", M32, 2 * M, 3)
    b.gaussian_conditional("gaussian_conditional")
    for i in range(slice_num):
        _prefixed(b, f"local_context.{i}.", local_context_entries(C))
    for i in range(1, slice_num):
        _prefixed(b, f"channel_context.{i}.", channel_context_entries(C * i, C))
    for i in range(1, slice_num):
        _prefixed(b, f"global_inter_context.{i}.", linear_global_inter_entries(C * i, 2 * C))
    for i in range(1, slice_num):
        _prefixed(b, f"global_intra_context.{i}.", linear_global_intra_entries(C))
    for i in range(slice_num):
        _prefixed(b, f"entropy_parameters_anchor.{i}.", entropy_params_mlic_entries(2 * M + (6 * C if i else 0), 2 * C))
    for i in range(slice_num):
        _prefixed(b, f"entropy_parameters_nonanchor.{i}.", entropy_params_mlic_entries(2 * M + (10 * C if i else 2 * C), 2 * C))
    for kind in ("lrp_anchor", "lrp_nonanchor"):
        for i in range(slice_num):
            _prefixed(b, f"{kind}.{i}.", lrp_entries(M + (i + 1) * C, C))
    return b.entries


def count_parameters(entries) -> int:
    n = 0
    for e in entries.values():
        if e.is_param:
            k = 1
            for s in e.shape:
                k *= s
            n += k
    return n
