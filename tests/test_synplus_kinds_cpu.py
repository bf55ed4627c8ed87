"""What rgbd_elic_finalize takes the state-dict entries of SynthesisTransformPlus for (family 13 of csrc/engine_abi.hip's
tensor_kind, through the host-only hook rgbd_debug_tensor_kind): its transposed layers are named without the "g_s." the codecs'
rule looks for, its three aligners carry a block name in front, and the family numbers 10 to 12 stay reserved.  No GPU."""
import collections
import ctypes

import pytest

from rgbd_amd import arch
from rgbd_amd._lib import lib

IGNORED, RECOVERY, DENSE, CONV, DECONV, GDN, LINEAR, ARRAY, QUANTILES = range(9)  # RGBD_KIND_* of include/rgbd_amd.h
FAMILY = 13


def kind(family, name, shape):
    return lib().rgbd_debug_tensor_kind(family, name.encode(), (ctypes.c_int64 * len(shape))(*shape), len(shape))


def test_transposed_layers_of_the_walk():
    for stage, shape in ((1, (320, 192, 5, 5)), (5, (192, 192, 5, 5)), (10, (192, 192, 5, 5)), (14, (192, 3, 5, 5))):
        assert kind(FAMILY, f"synthesis_transform.{stage}.weight", shape) == DECONV
        assert kind(FAMILY, f"synthesis_transform.{stage}.bias", shape[1:2]) == IGNORED
    for name in ("synthesis_transform.0.conv_a.0.conv.0.weight", "synthesis_transform.0.conv_b.3.weight",
                 "synthesis_transform.2.branch.2.weight", "synthesis_transform.6.conv_a.1.conv.2.weight",
                 "synthesis_transform.13.branch.4.weight"):
        assert kind(FAMILY, name, (96, 96, 3, 3)) == CONV
    # the bare stage name only, and only in this family (ELIC's rule asks for "g_s." in front)
    assert kind(FAMILY, "synthesis_transform.1.conv.weight", (192, 192, 5, 5)) == CONV
    assert kind(FAMILY, "x.synthesis_transform.1.weight", (192, 192, 5, 5)) == CONV
    assert kind(1, "synthesis_transform.1.weight", (320, 192, 5, 5)) == CONV
    assert kind(6, "synthesis_transform.1.weight", (320, 192, 5, 5)) == CONV


def test_aligner_blocks_inside_the_module():
    assert kind(FAMILY, "sp2.recovery.weight", (96, 192, 2, 2)) == RECOVERY
    assert kind(FAMILY, "sp2.recovery.bias", (192,)) == IGNORED
    assert kind(FAMILY, "sp3.patch_embeding2.weight", (96, 192, 2, 2)) == CONV
    assert kind(FAMILY, "sp1.blocks.0.norm1.weight", (96,)) == ARRAY
    assert kind(FAMILY, "sp1.blocks.1.norm2.bias", (96,)) == ARRAY
    for k in (1, 2, 3):
        for b in (0, 1):
            assert kind(FAMILY, f"sp{k}.blocks.{b}.attn.relative_position_bias_table", (49, 3)) == ARRAY
    assert kind(FAMILY, "sp1.blocks.0.attn.qkv2.weight", (192, 96, 1, 1)) == CONV  # a Linear as the upload sends it


def test_every_entry_as_uploaded():
    got = collections.Counter()
    for ch in (1, 3, 192):
        for name, e in arch.synthesis_plus_entries(192, 320, ch).items():
            if not e.is_param:
                continue
            shape = tuple(e.shape)
            if e.kind == "linear_w":
                shape = (shape[0], shape[1], 1, 1)
            want = {"conv_w": CONV, "linear_w": CONV, "deconv_w": DECONV, "bias": IGNORED, "ln_w": ARRAY, "ln_b": ARRAY,
                    "rpb_table": ARRAY}[e.kind]
            if name.endswith("recovery.weight"):
                want = RECOVERY
            assert kind(FAMILY, name, shape) == want, (name, shape)
            if ch == 3:
                got[want] += 1
    # 2 AttentionBlocks of 19 convs, 9 bottlenecks of 3, 4 deconvs; per aligner 2 embeddings + 2 * 5 Linears, 1 recovery,
    # 2 * (2 norms * 2 + 1 table) arrays; a bias for every conv, deconv, Linear and recovery
    assert dict(got) == {CONV: 65 + 36, DECONV: 4, RECOVERY: 3, ARRAY: 30, IGNORED: 65 + 4 + 36 + 3}


@pytest.mark.parametrize("family", [10, 11, 12, 14])
def test_reserved_numbers_are_refused(family):
    assert kind(family, "synthesis_transform.1.weight", (320, 192, 5, 5)) == -22
    assert kind(family, "a.weight", (8, 8, 3, 3)) == -22
