"""Deterministic synthetic weights and images (no checkpoint ships with the reference).

Values come from numpy's Philox counter generator through integer arithmetic only, so the same
(name, seed) gives the same float32 tensor on any machine / numpy / torch version:
    raw 64-bit word -> four 16-bit fields -> their integer sum (Irwin-Hall, ~Gaussian) -> scale -> float32.

The "stress" recipe multiplies a few tensors so that the latents leave the dead zone
and the rANS coder sees a non-trivial symbol distribution (dozens of scale bins, escape symbols).
"""
import hashlib
import math
from collections import OrderedDict

import numpy as np

from .arch import (STF_SLICES, Entry, channel_aligner_entries, channel_context_entries, entropy_params_mlic_entries, lrp_entries, feature_decoder_entries, feature_encoder_entries, linear_global_inter_entries, linear_global_intra_entries, local_context_entries,
                   spatial_aligner_entries, synthesis_plus_entries, ckbd_config, ckbd_entries, elic_entries, elic_united_entries, elic_united_r2d_entries, model_config, stf_config,
                   stf_entries, stf_single_config, stf_united_entries, MLIC_SLICE_CH, mlic_config, mlic_entries, elic_master_entries,
                   elic_master_latent_entries)

_IH_STD = math.sqrt(4.0 * (65536.0**2 - 1.0) / 12.0)  # std of the sum of four uniform 16-bit ints
_IH_MEAN = 2.0 * 65535.0


def _key(name: str, seed: int) -> int:
    h = hashlib.sha256(f"{seed}:{name}".encode()).digest()
    return int.from_bytes(h[:8], "little")


def _raw(name: str, seed: int, n: int) -> np.ndarray:
    return np.random.Philox(key=_key(name, seed)).random_raw(n)


def normal_like(name: str, seed: int, shape, std: float) -> np.ndarray:
    n = int(np.prod(shape)) if len(shape) else 1
    w = _raw(name, seed, n)
    s = (w & 0xFFFF) + ((w >> 16) & 0xFFFF) + ((w >> 32) & 0xFFFF) + (w >> 48)
    v = (s.astype(np.float64) - _IH_MEAN) * (std / _IH_STD)
    return v.astype(np.float32).reshape(shape)


def uniform_like(name: str, seed: int, shape, lo: float, hi: float) -> np.ndarray:
    n = int(np.prod(shape)) if len(shape) else 1
    w = _raw(name, seed, n)
    u = (w >> 11).astype(np.float64) * (1.0 / 9007199254740992.0)  # 53-bit mantissa, [0,1)
    return (lo + (hi - lo) * u).astype(np.float32).reshape(shape)


def _eb_matrix_init(shape, index: int, filters=(3, 3, 3, 3), init_scale=10.0) -> np.ndarray:
    # entropy_models.py:291-299: log(expm1(1 / scale / filters[i+1]))
    f = (1,) + tuple(filters) + (1,)
    scale = init_scale ** (1.0 / (len(filters) + 1))
    init = math.log(math.expm1(1.0 / scale / f[index + 1]))
    return np.full(shape, init, dtype=np.float32)


GDN_PEDESTAL = np.float32((2.0 ** -18) ** 2)  # NonNegativeParametrizer: reparam_offset ** 2


def make_tensor(name: str, e: Entry, seed: int) -> np.ndarray:
    if e.kind in ("conv_w", "deconv_w", "bias"):
        # torch's default Conv2d/ConvTranspose2d init, U(-1/sqrt(fan_in), 1/sqrt(fan_in)); the reference's
        # kaiming pass (priors.py:63-68) runs before its conv layers exist, so this is what it starts from
        b = 1.0 / math.sqrt(e.fan_in)
        return uniform_like(name, seed, e.shape, -b, b)
    if e.kind == "linear_w":
        b = 1.0 / math.sqrt(e.fan_in)
        return uniform_like(name, seed, e.shape, -b, b)
    if e.kind == "ln_w":  # nn.LayerNorm starts at (1, 0); perturbed so that the affine part is exercised
        return (1.0 + uniform_like(name, seed, e.shape, -0.1, 0.1)).astype(np.float32)
    if e.kind == "ln_b":
        return uniform_like(name, seed, e.shape, -0.1, 0.1)
    if e.kind == "rpb_table":  # trunc_normal_(std=0.02) in the reference; wider here so the bias matters
        return normal_like(name, seed, e.shape, 0.3)
    if e.kind == "gdn_beta":  # layers/gdn.py:43-45: NonNegativeParametrizer(minimum=1e-6).init(ones)
        return np.sqrt(np.maximum(np.ones(e.shape, np.float32) + GDN_PEDESTAL, GDN_PEDESTAL)).astype(np.float32)
    if e.kind == "gdn_gamma":  # gdn.py:48-50: init(0.1 * eye)
        g = np.float32(0.1) * np.eye(e.shape[0], dtype=np.float32)
        return np.sqrt(np.maximum(g + GDN_PEDESTAL, GDN_PEDESTAL)).astype(np.float32)
    if e.kind == "eb_matrix":
        idx = int(name[-1])
        return _eb_matrix_init(e.shape, idx) + normal_like(name, seed, e.shape, 0.05)
    if e.kind == "eb_bias":
        return uniform_like(name, seed, e.shape, -0.5, 0.5)
    if e.kind == "eb_factor":
        return normal_like(name, seed, e.shape, 0.1)
    if e.kind == "eb_quantiles":
        c = e.shape[0]
        med = uniform_like(name + "#med", seed, (c,), -0.4, 0.4)
        lo = uniform_like(name + "#lo", seed, (c,), 7.0, 12.0)
        hi = uniform_like(name + "#hi", seed, (c,), 7.0, 12.0)
        q = np.stack([med - lo, med, med + hi], axis=1).astype(np.float32)
        return q.reshape(e.shape)
    if e.kind == "buffer":
        if e.dtype == "int32":
            return np.zeros(e.shape, dtype=np.int32)
        if e.dtype == "int64":  # relative_position_index of a Swin window (stf_united.py:62-72)
            ws = int(round(math.sqrt(e.shape[0])))
            c = np.stack(np.meshgrid(np.arange(ws), np.arange(ws), indexing="ij")).reshape(2, -1)
            rel = (c[:, :, None] - c[:, None, :]).transpose(1, 2, 0) + (ws - 1)
            return (rel[:, :, 0] * (2 * ws - 1) + rel[:, :, 1]).astype(np.int64)
        if name.endswith(".pedestal"):  # ops/parametrizers.py:34-37
            return np.array([GDN_PEDESTAL], dtype=np.float32)
        if name.endswith("_reparam.lower_bound.bound"):
            minimum = 1e-6 if ".beta_reparam." in name else 0.0
            return np.array([(minimum + (2.0 ** -18) ** 2) ** 0.5], dtype=np.float32)
        if name.endswith("context_prediction.mask"):  # Cheng2020withCKBD.py:28-31
            m = np.zeros(e.shape, dtype=np.float32)
            m[:, :, 0::2, 1::2] = 1
            m[:, :, 1::2, 0::2] = 1
            return m
        if name.endswith(".target"):
            t = math.log(2.0 / 1e-9 - 1.0)  # entropy_models.py:309-310
            return np.array([-t, 0.0, t], dtype=np.float32)
        if name.endswith("likelihood_lower_bound.bound"):
            return np.array([1e-9], dtype=np.float32)
        if name.endswith("lower_bound_scale.bound") or name.endswith("scale_bound"):
            return np.array([0.11], dtype=np.float32)
        return np.zeros(e.shape, dtype=np.float32)
    raise ValueError(f"unknown entry kind {e.kind} for {name}")


def synthetic_state_dict(seed: int = 0, config=None, stress: bool = True, as_torch: bool = True,
                         model: str = "ELIC_united", channel: int = 3, recipe: str = None, N: int = 192,
                         in_channel: int = 192, out_channel: int = 192, dim: int = 32, out_dim: int = 64, num_heads: int = 2,
                         M: int = 320, in_dim: int = 640):
    """Full state_dict (parameters + buffers) of ELIC_united (default), ELIC_united_R2D, STF_united, the single-modal STF
    (model="STF": recipes "stress" and "plain"), the checkerboard Cheng2020 model (model="ckbd", width N, the same two recipes)
    or the single-modal ELIC with deterministic synthetic values.  `recipe`: "stress" (= stress=True, the default: ~22 bpp, wide CDF rows, 17 % escapes -- the worst
    case for the entropy coder), "trained_like" (ELIC_united only: latents mostly inside the dead zone, scales near the
    bottom of the scale table, ~1 bpp per modality like a trained q=2_2 model -- the coder's realistic operating point),
    "high_rate" (ELIC_united only: latents of tens to hundreds, predicted scales of 10 ... 100 -- scale-table rows of 300 ...
    3000 entries, what a high-quality checkpoint makes the decoder search) or "plain" (default initialisation, everything
    quantises to zero).  model="Spatial_aligner" (in_channel, out_channel): the guided-attention block alone, always with its
    stress recipe (_apply_stress_aligner).  model="LocalContext" (dim, num_heads), "LinearGlobalIntraContext" (dim) or
    "LinearGlobalInterContext" (dim, out_dim): an attention context of MLIC++ alone, always with _apply_stress_context.
    model="Channel_aligner": the block alone (the reference's constant widths), always with _apply_stress_chalign.
    model="Feature_encoder" (in_channel) or "Feature_decoder" (in_channel, out_channel): a feature network of ELIC_master alone,
    always with _apply_stress_feature.  model="SynthesisTransformPlus" (N, M, channel = its `ch`): the guided synthesis transform
    alone, always with _apply_stress_synplus.  model="EntropyParametersMLIC", "ChannelContext" or "LatentResidualPrediction"
    (in_dim, out_dim): a per-slice network of MLIC++ alone, always with _apply_stress_mlic_slice.  model="MLIC" (N, M with
    M / 32 slices, channel): the MLIC++ codec, recipes "stress" (_apply_stress_mlic) and "plain".  model="ELIC_master_latent"
    (config): the latent codec of ELIC_master, recipes "stress" (_apply_stress_master) and "plain"; model="ELIC_master" (config,
    channel): the same values with the four outer blocks of the full model added (_apply_stress_feature, _apply_stress_chalign)."""
    if model in ("EntropyParametersMLIC", "ChannelContext", "LatentResidualPrediction"):
        entries = {"EntropyParametersMLIC": entropy_params_mlic_entries, "ChannelContext": channel_context_entries,
                   "LatentResidualPrediction": lrp_entries}[model](in_dim, out_dim)
        sd = OrderedDict((name, make_tensor(name, e, seed)) for name, e in entries.items())
        _apply_stress_mlic_slice(sd, model)
        if as_torch:
            import torch

            return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items())
        return sd
    if model in ("Feature_encoder", "Feature_decoder"):
        entries = feature_encoder_entries(in_channel) if model == "Feature_encoder" else feature_decoder_entries(in_channel, out_channel)
        sd = OrderedDict((name, make_tensor(name, e, seed)) for name, e in entries.items())
        _apply_stress_feature(sd)
        if as_torch:
            import torch

            return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items())
        return sd
    if model == "Channel_aligner":
        sd = OrderedDict((name, make_tensor(name, e, seed)) for name, e in channel_aligner_entries().items())
        _apply_stress_chalign(sd)
        if as_torch:
            import torch

            return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items())
        return sd
    if model in ("LocalContext", "LinearGlobalIntraContext", "LinearGlobalInterContext"):
        entries = (local_context_entries(dim, num_heads=num_heads) if model == "LocalContext" else
                   linear_global_intra_entries(dim) if model == "LinearGlobalIntraContext" else linear_global_inter_entries(dim, out_dim))
        sd = OrderedDict((name, make_tensor(name, e, seed)) for name, e in entries.items())
        _apply_stress_context(sd, seed)
        if as_torch:
            import torch

            return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items())
        return sd
    if model == "SynthesisTransformPlus":
        entries = synthesis_plus_entries(N, M, channel)
        sd = OrderedDict((name, make_tensor(name, e, seed)) for name, e in entries.items())
        _apply_stress_synplus(sd, seed)
        if as_torch:
            import torch

            return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items())
        return sd
    if model == "Spatial_aligner":
        sd = OrderedDict()
        for name, e in spatial_aligner_entries(in_channel, out_channel).items():
            sd[name] = make_tensor(name, e, seed)
        _apply_stress_aligner(sd, seed)
        if as_torch:
            import torch

            return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items())
        return sd
    if recipe is not None:
        if recipe not in ("stress", "trained_like", "high_rate", "plain"):
            raise ValueError(f"unknown recipe {recipe}")
        stress = recipe == "stress"
    if model == "STF_united":
        cfg = stf_config()
        entries = stf_united_entries()
    elif model == "STF":
        cfg = stf_single_config()
        entries = stf_entries(channel)
    elif model == "ckbd":
        cfg = ckbd_config(N)
        entries = ckbd_entries(N, channel)
    elif model == "MLIC":
        cfg = mlic_config(N, M, M // MLIC_SLICE_CH)
        entries = mlic_entries(N, M, M // MLIC_SLICE_CH, channel)
    elif model in ("ELIC_master", "ELIC_master_latent"):
        cfg = model_config() if config is None else config
        entries = elic_master_entries(cfg, channel) if model == "ELIC_master" else elic_master_latent_entries(cfg)
    else:
        cfg = model_config() if config is None else config
        entries = {"ELIC_united": elic_united_entries, "ELIC_united_R2D": elic_united_r2d_entries}.get(model)
        entries = entries(cfg) if entries else elic_entries(cfg, channel)
    sd = OrderedDict()
    for name, e in entries.items():
        sd[name] = make_tensor(name, e, seed)
    if stress and model in ("ELIC_united", "ELIC_united_R2D"):
        _apply_stress(sd, cfg)
    elif stress and model == "STF_united":
        _apply_stress(sd, cfg, transforms=False)
        for mod in ("rgb", "depth"):  # latents of a few units: the last patch-merging projection feeds the final stage
            sd[f"g_a.{mod}_ana_layers.4.downsample.reduction.weight"] *= np.float32(STF_Y_GAIN)
    elif stress and model == "STF":
        _apply_stress_stf(sd)
    elif stress and model == "ckbd":
        _apply_stress_ckbd(sd, seed, N)
    elif stress and model == "MLIC":
        _apply_stress_mlic(sd, seed, M // MLIC_SLICE_CH)
    elif stress and model in ("ELIC_master", "ELIC_master_latent"):
        _apply_stress_master(sd, cfg, seed, outer=model == "ELIC_master")
    elif stress:
        _apply_stress_single(sd, cfg)
    if recipe == "trained_like":
        if model != "ELIC_united":
            raise ValueError("the trained_like recipe is defined for ELIC_united")
        _apply_trained_like(sd, cfg)
    if recipe == "high_rate":
        if model != "ELIC_united":
            raise ValueError("the high_rate recipe is defined for ELIC_united")
        _apply_high_rate(sd, cfg)
    if as_torch:
        import torch

        return OrderedDict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in sd.items())
    return sd


STF_Y_GAIN = 12.0
ALIGNER_QK_GAIN = 3.5


def _apply_stress_aligner(sd, seed, prefix=""):
    """Spatial_aligner: what makes a wrong attention visible.  Relative position biases of order 1 (std 1), LayerNorm weights
    in [0.5, 1.5], and the query and key projections scaled so that the scores (std ~0.3 with the default initialisation on
    normalised tokens) reach |S| >= 10: a softmax that is far from uniform, so shift, mask, bias and the q / k / v roles
    all move the output.  prefix: "" or the block's name inside a model with its dot ("sp1.")."""
    for k in range(2):
        p = f"{prefix}blocks.{k}"
        sd[f"{p}.attn.relative_position_bias_table"] = (sd[f"{p}.attn.relative_position_bias_table"] / np.float32(0.3)).astype(np.float32)
        for n in ("norm1", "norm2"):
            name = f"{p}.{n}.weight"
            sd[name] = (1.0 + uniform_like(name + "#stress", seed, sd[name].shape, -0.5, 0.5)).astype(np.float32)
        g = np.float32(ALIGNER_QK_GAIN)
        sd[f"{p}.attn.qkv1.weight"] = sd[f"{p}.attn.qkv1.weight"] * g
        sd[f"{p}.attn.qkv1.bias"] = sd[f"{p}.attn.qkv1.bias"] * g
        E = sd[f"{p}.attn.qkv1.weight"].shape[0]
        sd[f"{p}.attn.qkv2.weight"][:E] *= g  # the key half; the value half keeps its scale
        sd[f"{p}.attn.qkv2.bias"][:E] *= g


SYNPLUS_DECONV_GAIN = math.sqrt(12.0)
SYNPLUS_RECOVERY_GAIN = 8.0


def _apply_stress_synplus(sd, seed, prefix=""):
    """SynthesisTransformPlus (prefix: "" or the module's name inside a model with its dot, "g_s."): the single-modal g_s recipe (which leaves g_s at its default initialisation) plus
    _apply_stress_aligner on sp1, sp2 and sp3, and two gains that keep the signal alive through three replacements.  A 5x5
    stride-2 transposed convolution at the default initialisation (variance 1 / (3 * 25 cout), 25 / 4 taps of cin channels per
    output) shrinks a map by sqrt(12): its weights are scaled back by that.  A Spatial_aligner returns about a tenth of its
    input's scale (recovery: 96 terms of variance 1 / (3 * 4 * 192)), so that behind the second one the biases of the patch
    embeddings would outweigh x and an aligner in the wrong place, or fed the wrong x, would barely move the output: the
    recovery weights are scaled by 8."""
    for i in (1, 5, 10, 14):
        sd[f"{prefix}synthesis_transform.{i}.weight"] = sd[f"{prefix}synthesis_transform.{i}.weight"] * np.float32(SYNPLUS_DECONV_GAIN)
    for k in (1, 2, 3):
        _apply_stress_aligner(sd, seed, prefix=f"{prefix}sp{k}.")
        sd[f"{prefix}sp{k}.recovery.weight"] = sd[f"{prefix}sp{k}.recovery.weight"] * np.float32(SYNPLUS_RECOVERY_GAIN)


LOCAL_QK_GAIN = 3.5
LINEAR_QK_GAIN = 8.0


def _apply_stress_context(sd, seed, prefix=""):
    """The attention contexts of MLIC++: what makes a wrong attention visible.  LocalContext: relative position biases of
    order 1, LayerNorm weights in [0.5, 1.5], the query and key rows of qkv_proj scaled so that the scores (std ~0.3 with the
    default initialisation) reach |S| of 10 to 40 -- far from a uniform softmax, and still well below the mask's 100.  The
    linear contexts: the depthwise layers behind keys and queries scaled so that both softmaxes (over tokens, over channels)
    see arguments of order 10.  prefix: "" or the module's name inside a model with its dot ("local_context.3.")."""
    p = prefix
    if p + "relative_position_table" in sd:
        sd[p + "relative_position_table"] = (sd[p + "relative_position_table"] / np.float32(0.3)).astype(np.float32)
        for n in ("norm1", "norm2"):
            name = f"{p}{n}.weight"
            sd[name] = (1.0 + uniform_like(name + "#stress", seed, sd[name].shape, -0.5, 0.5)).astype(np.float32)
        C = sd[p + "qkv_proj.weight"].shape[1]
        sd[p + "qkv_proj.weight"][:2 * C] *= np.float32(LOCAL_QK_GAIN)  # the query and key rows; the value rows keep their scale
        if p + "qkv_proj.bias" in sd:
            sd[p + "qkv_proj.bias"][:2 * C] *= np.float32(LOCAL_QK_GAIN)
    else:
        for n in ("keys.1", "queries.1"):
            sd[f"{p}{n}.weight"] = sd[f"{p}{n}.weight"] * np.float32(LINEAR_QK_GAIN)
            sd[f"{p}{n}.bias"] = sd[f"{p}{n}.bias"] * np.float32(LINEAR_QK_GAIN)


MLIC_SLICE_FIRST_GAIN = math.sqrt(3.0)
MLIC_SLICE_GELU_GAIN = math.sqrt(3.0 / 0.425)
MLIC_SLICE_LRP_OUT = 0.7


def _apply_stress_mlic_slice(sd, model, prefix=""):
    """EntropyParametersMLIC, ChannelContext, LatentResidualPrediction: pre-activations of order 1 at every layer, for inputs of
    unit variance.  The default initialisation (variance 1 / (3 fan_in)) shrinks a map by 0.58 per layer and a GELU by another
    0.65 (E gelu(x)^2 = 0.425 for a standard normal x), so that the third GELU would see arguments of a few hundredths, where
    it is the line x / 2 and its erf and tanh forms agree to 1e-7.  The first layer's weights are scaled by sqrt(3) and those
    behind a GELU by sqrt(3 / 0.425): every GELU sees both signs out to |x| of 3 to 5.  The last layer of the LRP is scaled by a
    further 0.7, so that the largest |x| in front of tanh is 1 to 3: past the linear part, short of saturation.  Biases keep
    their initialisation (a few hundredths, 1e4 times the tests' bound).  prefix: "" or the module's name inside a model with its dot."""
    names = [k for k in sd if k.endswith(".weight") and k.startswith(prefix)]
    for i, name in enumerate(names):
        g = MLIC_SLICE_FIRST_GAIN if i == 0 else MLIC_SLICE_GELU_GAIN
        if model == "LatentResidualPrediction" and i == len(names) - 1:
            g *= MLIC_SLICE_LRP_OUT
        sd[name] = sd[name] * np.float32(g)


CHALIGN_TRUNK_GAIN = math.sqrt(6.0)
CHALIGN_HEAD_GAIN = 4.0


def _apply_stress_chalign(sd):
    """Channel_aligner: beta and gamma that are not their heads' biases.  The default initialisation (U(+-1 / sqrt(fan_in)),
    variance 1 / (3 fan_in)) shrinks a map by about 0.4 per 3x3 + LeakyReLU layer, so that behind four of them the pooled
    product would be a few per cent of the heads' biases (+-1/48).  The trunk weights are therefore scaled by sqrt(6) -- He's
    gain for a rectifier, variance 2 / fan_in: the maps keep the scale of the input through the trunk -- and the weights of
    conv2 / conv3 by 4, their biases left alone: the mean of a LeakyReLU map (about 0.4 of its spread) times the 2304 head
    weights of an output gives max |beta|, |gamma| of 0.2 ... 5.7 on the fixtures' maps, ten to a few hundred times the bias."""
    for i in (0, 2, 4, 6):
        sd[f"conv1.{i}.weight"] = sd[f"conv1.{i}.weight"] * np.float32(CHALIGN_TRUNK_GAIN)
    for n in ("conv2", "conv3"):
        sd[f"{n}.weight"] = sd[f"{n}.weight"] * np.float32(CHALIGN_HEAD_GAIN)


FEATURE_RELU_GAIN = math.sqrt(6.0)
FEATURE_LINEAR_GAIN = math.sqrt(3.0)


def _apply_stress_feature(sd):
    """Feature_encoder / Feature_decoder: three residual branches and a shortcut of comparable size.  The default
    initialisation (variance 1 / (3 fan_in)) shrinks a map by about 0.4 per 3x3 + ReLU layer, so that a block's branch
    relu(conv2(relu(conv1 x))) would be a sixth of its identity and the sum of the three a fraction of the outer shortcut:
    a wrong branch would hide behind the shortcut.  The 3x3 weights of the blocks are scaled by sqrt(6) (He's gain for a
    rectifier: a branch keeps the scale of its input), and the layers without an activation -- the encoder's conv1, the
    decoder's resblock1.skip and `conv` -- by sqrt(3) (variance 1 / fan_in).  Biases and deconv1 keep theirs (torch's fan_in of
    a transposed convolution is out_channels * 9, so its default weights are already of order 1 / sqrt(27))."""
    for name in sd:
        if not name.endswith(".weight") or name == "deconv1.weight":
            continue
        relu = name.startswith("resblock") and ".skip." not in name
        sd[name] = sd[name] * np.float32(FEATURE_RELU_GAIN if relu else FEATURE_LINEAR_GAIN)


def _apply_stress(sd, cfg, transforms=True):
    slice_ch = list(cfg["slice_ch"])
    for mod in ("rgb", "depth"):
        if transforms:
            sd[f"g_a.{mod}_analysis_transform.16.weight"] *= np.float32(48.0)
    for mod in ("rgb", "depth"):
        sd[f"h_a.{mod}_reduction.4.weight"] *= np.float32(24.0)  # |z| of a few units: exercises the z coder
    for m in ("r", "d"):
        sd[f"h_s.{m}_h_s3.deconv.weight"] *= np.float32(40.0)
    for fam in ("rgb_entropy_parameters_anchor", "depth_entropy_parameters_anchor",
                "rgb_entropy_parameters_nonanchor", "depth_entropy_parameters_nonanchor"):
        for i, c in enumerate(slice_ch):
            sd[f"{fam}.{i}.fusion.4.weight"] *= np.float32(6.0)
            sd[f"{fam}.{i}.fusion.4.bias"][:c] = np.float32(1.0)  # scale half


def _apply_trained_like(sd, cfg):
    """Rates of a trained low-rate model instead of the stress recipe's: |y| of a few tenths (most symbols round to zero,
    some to +-1/+-2), predicted scales around 0.2-0.4 (scale-table rows of 7-9 entries), small |z|."""
    slice_ch = list(cfg["slice_ch"])
    for mod in ("rgb", "depth"):
        sd[f"g_a.{mod}_analysis_transform.16.weight"] *= np.float32(6.0)
        sd[f"h_a.{mod}_reduction.4.weight"] *= np.float32(6.0)
    for m in ("r", "d"):
        sd[f"h_s.{m}_h_s3.deconv.weight"] *= np.float32(8.0)
    for fam in ("rgb_entropy_parameters_anchor", "depth_entropy_parameters_anchor",
                "rgb_entropy_parameters_nonanchor", "depth_entropy_parameters_nonanchor"):
        for i, c in enumerate(slice_ch):
            sd[f"{fam}.{i}.fusion.4.weight"] *= np.float32(2.0)
            sd[f"{fam}.{i}.fusion.4.bias"][:c] = np.float32(0.25)  # scale half


HIGH_RATE_GAINS = (240.0, 24.0, 40.0, 12.0, 40.0)  # y, z, h_s, scale-head weight, scale-head bias


def _apply_high_rate(sd, cfg):
    """Wide scale-table rows: |y| of tens to hundreds and predicted scales of 10 ... 100 (sigma-index 37 ... 56 of 64, CDF rows
    of 300 ... 3000 entries) -- the rows a high-quality checkpoint codes on, which neither other recipe reaches
    (sigma-index <= 33).  Applied to the plain initialisation."""
    gy, gz, gh, gw, gb = (np.float32(v) for v in HIGH_RATE_GAINS)
    slice_ch = list(cfg["slice_ch"])
    for mod in ("rgb", "depth"):
        sd[f"g_a.{mod}_analysis_transform.16.weight"] *= gy
        sd[f"h_a.{mod}_reduction.4.weight"] *= gz
    for m in ("r", "d"):
        sd[f"h_s.{m}_h_s3.deconv.weight"] *= gh
    for fam in ("rgb_entropy_parameters_anchor", "depth_entropy_parameters_anchor",
                "rgb_entropy_parameters_nonanchor", "depth_entropy_parameters_nonanchor"):
        for i, c in enumerate(slice_ch):
            sd[f"{fam}.{i}.fusion.4.weight"] *= gw
            sd[f"{fam}.{i}.fusion.4.bias"][:c] = gb  # scale half


def _apply_stress_single(sd, cfg):
    # same idea as _apply_stress for the single-modal ELIC (its entropy-parameter nets end in a 1x1 convolution)
    slice_ch = list(cfg["slice_ch"])
    sd["g_a.analysis_transform.13.weight"] *= np.float32(48.0)
    sd["h_a.reduction.4.weight"] *= np.float32(24.0)
    sd["h_s.increase.4.weight"] *= np.float32(40.0)
    for fam in ("entropy_parameters_anchor", "entropy_parameters_nonanchor"):
        for i, c in enumerate(slice_ch):
            sd[f"{fam}.{i}.fusion.4.weight"] *= np.float32(6.0)
            sd[f"{fam}.{i}.fusion.4.bias"][:c] = np.float32(1.0)  # scale half


MASTER_Y_GAIN = 24.0


def _apply_stress_master(sd, cfg, seed, outer=False):
    """ELIC_master and its latent codec, composed from the recipes of their parts: the single-modal recipe for the transforms, the
    hyper path and the heads of the parameter nets (_apply_stress_single: the EX nets end in the same `fusion.4` the united
    model's recipe scales, with the same gains), _apply_stress_synplus under `g_s.`, and for the full model
    _apply_stress_feature / _apply_stress_chalign on the outer blocks.  g_a's last convolution takes MASTER_Y_GAIN in place of the
    single-modal 48 so that the value can follow the 128-channel input of unit variance (tests/master_latent_cases.py) on its
    own."""
    _apply_stress_single(sd, cfg)
    sd["g_a.analysis_transform.13.weight"] *= np.float32(MASTER_Y_GAIN / 48.0)
    _apply_stress_synplus(sd, seed, prefix="g_s.")
    if not outer:
        return
    for p in ("aux_encoder.", "master_encoder.", "master_decoder."):
        sub = OrderedDict((k[len(p):], v) for k, v in sd.items() if k.startswith(p))
        _apply_stress_feature(sub)
        sd.update((p + k, v) for k, v in sub.items())
    sub = OrderedDict((k[len("channel_aligner."):], v) for k, v in sd.items() if k.startswith("channel_aligner."))
    _apply_stress_chalign(sub)
    sd.update(("channel_aligner." + k, v) for k, v in sub.items())


# single-modal STF: y, z, hyper means / scales, scale head (weight, bias), mean head, LRP head
STF1_GAINS = {"y": 4.0, "z": 200.0, "hyper": 30.0, "scale_w": 40.0, "scale_b": 1.0, "mean_w": 10.0, "lrp_w": 30.0}


def _apply_stress_stf(sd):
    """At the default initialisation the single-modal STF is degenerate (every z symbol and scale index 0, LRP of a few
    hundredths).  These gains give latents of a few units, a busy z stream, a dozen or more scale-table rows per slice, means
    that move the rounding, escape symbols, and an LRP correction of tenths that later slices depend on."""
    g = {k: np.float32(v) for k, v in STF1_GAINS.items()}
    sd["layers.2.downsample.reduction.weight"] *= g["y"]  # the last patch-merging projection feeds the final stage
    sd["h_a.8.weight"] *= g["z"]
    sd["h_mean_s.8.weight"] *= g["hyper"]
    sd["h_scale_s.8.weight"] *= g["hyper"]
    for i in range(STF_SLICES):
        sd[f"cc_scale_transforms.{i}.8.weight"] *= g["scale_w"]
        sd[f"cc_scale_transforms.{i}.8.bias"][:] = g["scale_b"]
        sd[f"cc_mean_transforms.{i}.8.weight"] *= g["mean_w"]
        sd[f"lrp_transforms.{i}.8.weight"] *= g["lrp_w"]


# checkerboard Cheng2020: y, z, hyper, scale head (weight, bias), mean head, context conv
CKBD_GAINS = {"gdn_in": 6.0, "igdn_in": 2.0, "y": 5.0, "z": 150.0, "hyper": 80.0, "scale_w": 10.0, "scale_b": 2.0, "mean_w": 3.0, "ctx": 4.0}


def _apply_stress_ckbd(sd, seed, N):
    """From the reference's initialisation (GDN: beta = 1, gamma = 0.1 on the diagonal) to a model whose every stage matters:
    GDN / IGDN with a beta per channel and a dense gamma with positive off-diagonal mass, part of it below the
    parametrizer's bound (raw values <= 2^-18 clamp to gamma = 0), so that the gamma term exceeds beta somewhere in every
    layer; latents of a few units, a busy z stream, a dozen or more scale-table rows in each checkerboard half, escape
    symbols, and a context convolution whose MASKED taps are as large as the others in the state_dict (the reference masks the
    weight at every call), so that a missing or reversed mask shows."""
    g = {k: np.float32(v) for k, v in CKBD_GAINS.items()}
    for name in [k for k in sd if k.endswith(".beta")]:
        sd[name] = np.sqrt(uniform_like(name, seed, sd[name].shape, 0.5, 2.0) + GDN_PEDESTAL).astype(np.float32)
    for name in [k for k in sd if k.endswith(".gamma")]:
        c = sd[name].shape[0]
        dense = uniform_like(name, seed, (c, c), -0.02, 0.08)  # a fifth of the raw values below the bound; gamma <= 0.0064
        sd[name] = (sd[name] + dense).astype(np.float32)
    for i in (0, 2, 4):  # activations of a few units in front of the analysis GDNs
        sd[f"g_a.{i}.conv2.weight"] *= g["gdn_in"]
    for i in (1, 3, 5):  # ... and in front of the synthesis IGDNs
        sd[f"g_s.{i}.conv.weight"] *= g["igdn_in"]
    sd["g_a.6.weight"] *= g["y"]
    sd["h_a.8.weight"] *= g["z"]
    sd["h_s.8.weight"] *= g["hyper"]
    sd["entropy_parameters.4.weight"][:N] *= g["scale_w"]
    sd["entropy_parameters.4.bias"][:N] = g["scale_b"]  # chunk(2, 1): scales first
    sd["entropy_parameters.4.weight"][N:] *= g["mean_w"]
    sd["context_prediction.weight"] *= g["ctx"]


# MLIC++: conv in front of a GDN / an IGDN, y, z, hyper, scale head (weight, bias), mean head, the LRPs' last layer, and the
# linear contexts' reprojection and depthwise mlp layer
MLIC_GAINS = {"gdn_in": 6.0, "igdn_in": 3.5, "y": 5.0, "z": 8.0, "hyper": 4.0, "scale_w": 2.0, "scale_b": 0.7, "mean_w": 1.0,
              "lrp_out": 0.45, "inter_reproj": 4.0, "intra_reproj": 10.0, "ctx_dw": 2.0}


def _apply_stress_mlic(sd, seed, slice_num):
    """MLIC++, composed from the recipes of its parts: GDN / IGDN, latents, z and hyper parameters in the manner of
    _apply_stress_ckbd (a beta per channel, a dense gamma partly below the parametrizer's bound, activations of a few units in
    front of every GDN), _apply_stress_context on the thirty attention contexts and _apply_stress_mlic_slice on the channel
    contexts, parameter networks and LRPs.  The parameter networks end in (scales | means): the scale half gets a positive bias
    and a gain, so that every coding part sees a handful of scale-table rows and some escapes.  Every GELU is to see arguments
    on both sides of +-1: the hyper transforms' inner layers take the gain that undoes a default layer and a GELU
    (MLIC_SLICE_GELU_GAIN; z and hyper gains are the smaller for it), the linear contexts' reprojection and depthwise mlp layer
    gains of their own, and the LRPs' last layer is scaled down until tanh sees a largest |x| of 1 to 3 on latents of several
    units."""
    g = {k: np.float32(v) for k, v in MLIC_GAINS.items()}
    for name in ("h_a.reduction.2", "h_a.reduction.4", "h_a.reduction.6", "h_s.increase.2.0", "h_s.increase.4", "h_s.increase.6.0"):
        sd[name + ".weight"] *= np.float32(MLIC_SLICE_GELU_GAIN)
    for name in [k for k in sd if k.endswith(".beta")]:
        sd[name] = np.sqrt(uniform_like(name, seed, sd[name].shape, 0.5, 2.0) + GDN_PEDESTAL).astype(np.float32)
    for name in [k for k in sd if k.endswith(".gamma")]:
        c = sd[name].shape[0]
        dense = uniform_like(name, seed, (c, c), -0.02, 0.08)  # a fifth of the raw values below the bound; gamma <= 0.0064
        sd[name] = (sd[name] + dense).astype(np.float32)
    for i in (0, 2, 4):
        sd[f"g_a.analysis_transform.{i}.conv2.weight"] *= g["gdn_in"]
    for i in (1, 3, 5):
        sd[f"g_s.synthesis_transform.{i}.conv.weight"] *= g["igdn_in"]
    sd["g_a.analysis_transform.6.weight"] *= g["y"]
    sd["h_a.reduction.8.weight"] *= g["z"]
    sd["h_s.increase.8.weight"] *= g["hyper"]
    for i in range(slice_num):
        _apply_stress_context(sd, seed, f"local_context.{i}.")
        for kind in ("entropy_parameters_anchor", "entropy_parameters_nonanchor"):
            p = f"{kind}.{i}."
            _apply_stress_mlic_slice(sd, "EntropyParametersMLIC", p)
            half = sd[p + "fusion.6.bias"].shape[0] // 2
            sd[p + "fusion.6.weight"][:half] *= g["scale_w"]
            sd[p + "fusion.6.bias"][:half] = g["scale_b"]  # chunk(2, 1): scales first
            sd[p + "fusion.6.weight"][half:] *= g["mean_w"]
        for kind in ("lrp_anchor", "lrp_nonanchor"):
            _apply_stress_mlic_slice(sd, "LatentResidualPrediction", f"{kind}.{i}.")
            sd[f"{kind}.{i}.lrp_transform.6.weight"] *= g["lrp_out"]
        if i:
            _apply_stress_context(sd, seed, f"global_inter_context.{i}.")
            _apply_stress_context(sd, seed, f"global_intra_context.{i}.")
            for kind in ("global_inter_context", "global_intra_context"):
                sd[f"{kind}.{i}.reprojection.weight"] *= g["inter_reproj" if kind == "global_inter_context" else "intra_reproj"]
                sd[f"{kind}.{i}.mlp.2.weight"] *= g["ctx_dw"]
            _apply_stress_mlic_slice(sd, "ChannelContext", f"channel_context.{i}.")


def synthetic_pair(index: int, H: int, W: int, config_id: int = 0, smooth: bool = False):
    """One RGB-D pair in [0,1): rgb [3,H,W], depth [1,H,W] float32 (seed = 1000*config + index)."""
    seed = 1000 * config_id + index
    if not smooth:
        rgb = uniform_like("rgb", seed, (3, H, W), 0.0, 1.0)
        depth = uniform_like("depth", seed, (1, H, W), 0.0, 1.0)
        return rgb, depth
    # spatially correlated variant: bilinear-interpolated 8x8 noise (pure float64 arithmetic)
    def up(name, ch):
        g = uniform_like(name, seed, (ch, 9, 9), 0.0, 1.0).astype(np.float64)
        ys = np.linspace(0.0, 8.0, H, endpoint=False)
        xs = np.linspace(0.0, 8.0, W, endpoint=False)
        y0 = np.floor(ys).astype(int)
        x0 = np.floor(xs).astype(int)
        fy = (ys - y0)[None, :, None]
        fx = (xs - x0)[None, None, :]
        a = g[:, y0][:, :, x0]
        b = g[:, y0][:, :, x0 + 1]
        c = g[:, y0 + 1][:, :, x0]
        d = g[:, y0 + 1][:, :, x0 + 1]
        return ((a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy).astype(np.float32)

    return up("rgb_s", 3), up("depth_s", 1)


def synthetic_batch(B: int, H: int, W: int, config_id: int = 0, start: int = 0, smooth: bool = False):
    rs, ds = [], []
    for i in range(B):
        r, d = synthetic_pair(start + i, H, W, config_id, smooth)
        rs.append(r)
        ds.append(d)
    return np.stack(rs), np.stack(ds)


def synthetic_latents(B: int, h: int, w: int, M: int = 320, seed: int = 0):
    """Inputs of the Bi-CEE stage in isolation (BASELINE config 4, SURVEY §8d "C4"): y ~ N(0, 4^2) [B,M,h,w] and hyper
    parameters ~ N(0, 1) [B,2M,h,w] per modality.  Returns (rgb_y, rgb_hyper, depth_y, depth_hyper) as float32."""
    return (normal_like(f"c4.rgb_y.{B}x{h}x{w}", seed, (B, M, h, w), 4.0),
            normal_like(f"c4.rgb_hyper.{B}x{h}x{w}", seed, (B, 2 * M, h, w), 1.0),
            normal_like(f"c4.depth_y.{B}x{h}x{w}", seed, (B, M, h, w), 4.0),
            normal_like(f"c4.depth_hyper.{B}x{h}x{w}", seed, (B, 2 * M, h, w), 1.0))
