"""What rgbd_elic_finalize takes every state-dict entry for (csrc/engine_abi.hip: tensor_kind, through the host-only hook
rgbd_debug_tensor_kind): the classification is a chain of tests on family, name and shape whose ORDER matters -- the 2x2
`recovery.weight` and the contexts' dense 4-D weights are four-dimensional `.weight` tensors like every conv layer.  No GPU.

The names and shapes are those of the synthetic state dicts (synth.synthetic_state_dict builds them from these entry lists),
in the smallest configuration each recipe accepts, as the engine receives them: parameters only, an nn.Linear of a Swin block
as the 1x1 convolution EngineModule._upload makes of it.  The expected kinds are written out below from the chain, per entry
kind of arch.py, with the exceptions by name."""
import collections
import ctypes

import pytest

from rgbd_amd import arch
from rgbd_amd._lib import lib

IGNORED, RECOVERY, DENSE, CONV, DECONV, GDN, LINEAR, ARRAY, QUANTILES = range(9)  # RGBD_KIND_* of include/rgbd_amd.h

FAMILIES = {
    0: arch.elic_united_entries, 1: lambda: arch.elic_entries(None, 1), 2: arch.stf_united_entries,
    3: arch.elic_united_r2d_entries, 4: lambda: arch.stf_entries(1), 5: lambda: arch.ckbd_entries(128, 1),
    6: lambda: arch.spatial_aligner_entries(16, 16), 7: lambda: arch.local_context_entries(32),
    8: lambda: arch.linear_global_inter_entries(32, 32), 9: lambda: arch.linear_global_intra_entries(32),
}

# entry kind (arch.Entry.kind) -> what finalize does with it
BY_ENTRY_KIND = {
    "bias": IGNORED, "eb_bias": IGNORED, "eb_factor": IGNORED, "eb_matrix": IGNORED, "gdn_beta": IGNORED,  # read with their weight
    "conv_w": CONV, "deconv_w": DECONV, "gdn_gamma": GDN, "ln_w": ARRAY, "ln_b": ARRAY, "rpb_table": ARRAY,
    "eb_quantiles": QUANTILES,
}

# how many tensors of each kind a family's state dict holds (kinds with none are left out)
COUNTS = {
    0: {IGNORED: 517, CONV: 475, DECONV: 14, LINEAR: 52, QUANTILES: 2},
    1: {IGNORED: 205, CONV: 184, DECONV: 7, QUANTILES: 1},
    2: {IGNORED: 433, CONV: 411, DECONV: 6, LINEAR: 52, ARRAY: 268, QUANTILES: 2},
    3: {IGNORED: 472, CONV: 430, DECONV: 14, LINEAR: 52, QUANTILES: 2},
    4: {IGNORED: 308, CONV: 300, ARRAY: 134, QUANTILES: 1},
    5: {IGNORED: 68, CONV: 48, GDN: 6, QUANTILES: 1},
    6: {IGNORED: 13, RECOVERY: 1, CONV: 12, ARRAY: 10},
    7: {IGNORED: 5, DENSE: 1, CONV: 4, ARRAY: 5},
    8: {IGNORED: 11, DENSE: 4, CONV: 7},
    9: {IGNORED: 10, DENSE: 4, CONV: 6},
}


def kind(family, name, shape):
    return lib().rgbd_debug_tensor_kind(family, name.encode(), (ctypes.c_int64 * len(shape))(*shape), len(shape))


def uploaded(family):
    """(name, entry, shape) of what EngineModule._upload hands to rgbd_elic_set_tensor."""
    for name, e in FAMILIES[family]().items():
        if e.is_param:
            shape = tuple(e.shape)
            if e.kind == "linear_w" and ".fc." not in name:
                shape = (shape[0], shape[1], 1, 1)
            yield name, e, shape


def expected(family, name, e, shape):
    if e.kind == "linear_w":
        return LINEAR if len(shape) == 2 else CONV
    if name.endswith("recovery.weight") and shape[2:] == (2, 2):
        return RECOVERY  # before the conv layers, on every family
    if family >= 7 and e.kind == "conv_w" and (name == "fusion.weight" or shape[1:] == (1, 3, 3)):
        return DENSE  # before the conv layers, on the contexts only
    return BY_ENTRY_KIND[e.kind]


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_entry_of_the_family(family):
    got = collections.Counter()
    for name, e, shape in uploaded(family):
        k = kind(family, name, shape)
        assert k == expected(family, name, e, shape), (family, name, shape, k)
        got[k] += 1
    assert dict(got) == COUNTS[family]


def test_recovery_deconv_before_the_conv_layers():
    assert kind(6, "recovery.weight", (96, 16, 2, 2)) == RECOVERY
    assert kind(0, "g_s.sp1.recovery.weight", (96, 192, 2, 2)) == RECOVERY  # the block inside a model: by name and taps alone
    assert kind(6, "recovery.weight", (96, 16, 3, 3)) == CONV               # not the 2x2 form: a conv layer like any other
    assert kind(6, "patch_embeding1.weight", (96, 16, 2, 2)) == CONV        # a generic 4-D weight with 2x2 taps
    assert kind(6, "recovery.bias", (16,)) == IGNORED


@pytest.mark.parametrize("name, shape", [("fusion.weight", (64, 32, 5, 5)), ("keys.1.weight", (32, 1, 3, 3))])
def test_context_dense_on_the_contexts_only(name, shape):
    for family in range(10):
        assert kind(family, name, shape) == (DENSE if family >= 7 else CONV), family
    assert kind(7, name, shape[:3]) == IGNORED  # four dimensions or nothing


def test_transposed_layers_by_name():
    w = (192, 192, 5, 5)
    for mod in ("rgb", "depth"):
        for stage in (1, 5, 6, 10, 12, 14, 17):
            assert kind(0, f"g_s.{mod}_transform.{stage}.weight", w) == DECONV
        for stage in (0, 2, 3, 4, 7, 11, 13, 16):
            assert kind(0, f"g_s.{mod}_transform.{stage}.weight", w) == CONV
        assert kind(0, f"g_s.{mod}_transform.1.conv1.weight", w) == CONV  # a block with sub-names is not the bare stage
        assert kind(0, f"g_a.{mod}_transform.1.weight", w) == CONV        # the analysis side has no transposed layer
    assert kind(1, "g_s.synthesis_transform.14.weight", w) == DECONV
    for i in (0, 2, 4):
        assert kind(1, f"h_s.increase.{i}.weight", (640, 480, 3, 3)) == DECONV
    assert kind(1, "x.h_s.increase.0.weight", w) == CONV  # a prefix, not a substring
    assert kind(0, "h_s.d_h_s3.deconv.weight", (960, 640, 3, 3)) == DECONV


def test_norms_and_position_tables():
    for family in range(10):
        local = family == 7
        assert kind(family, "blocks.1.norm2.weight", (96,)) == ARRAY
        assert kind(family, "blocks.0.attn.relative_position_bias_table", (49, 3)) == ARRAY
        assert kind(family, "norm1.weight", (64,)) == (ARRAY if local else IGNORED)
        assert kind(family, "norm2.bias", (64,)) == (ARRAY if local else IGNORED)
        assert kind(family, "relative_position_table", (81, 2)) == (ARRAY if local else IGNORED)
    assert kind(2, "blocks.1.norm2.bias", (96, 1)) == IGNORED  # a `.norm` of two dimensions is nobody's
    assert kind(2, "blocks.1.norm2.weight", (96, 1)) == LINEAR  # ... unless it is a 2-D weight, which comes first


def test_quantiles_gamma_and_linear():
    assert kind(0, "rgb_entropy_bottleneck.quantiles", (192, 1, 3)) == QUANTILES
    assert kind(1, "entropy_bottleneck.quantiles", (192, 1, 3)) == QUANTILES
    assert kind(1, "entropy_bottleneck._matrix0", (192, 3, 1)) == IGNORED
    assert kind(5, "g_a.1.gdn.gamma", (128, 128)) == GDN
    assert kind(5, "g_a.1.gdn.gamma", (128, 64)) == IGNORED  # not square
    assert kind(5, "g_a.1.gdn.gamma", (128,)) == IGNORED
    assert kind(5, "g_a.1.gdn.beta", (128,)) == IGNORED
    assert kind(0, "rgb_entropy_parameters_anchor.0.se.fc.0.weight", (11, 176)) == LINEAR
    assert kind(0, "some.weight", (11, 176, 3)) == IGNORED  # a weight of three dimensions


def test_bad_arguments():
    L = lib()
    shape = (ctypes.c_int64 * 4)(8, 8, 3, 3)
    for family in (-1, 10, 1 << 20):
        assert L.rgbd_debug_tensor_kind(family, b"a.weight", shape, 4) == -22
    for ndim in (-1, 0, 5):
        assert L.rgbd_debug_tensor_kind(0, b"a.weight", shape, ndim) == -22
    assert L.rgbd_debug_tensor_kind(0, None, shape, 4) == -22
    assert L.rgbd_debug_tensor_kind(0, b"a.weight", None, 4) == -22
    assert L.rgbd_debug_tensor_kind(0, b"a.weight", (ctypes.c_int64 * 4)(8, 0, 3, 3), 4) == -22
    assert L.rgbd_debug_tensor_kind(0, b"a.weight", shape, 4) == CONV
