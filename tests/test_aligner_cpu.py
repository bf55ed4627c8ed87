"""What Spatial_aligner and ELIC(return_mid=True) promise without a GPU: construction, the reference's state-dict names and
shapes (recorded from the reference module by tests/golden/make_aligner.py), strict loading, the exported symbols."""
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_elic_return_mid_constructs():
    import rgbd_amd

    net = rgbd_amd.ELIC(config=rgbd_amd.model_config(), channel=3, return_mid=True).eval()
    assert net.return_mid is True
    assert rgbd_amd.ELIC(config=rgbd_amd.model_config(), channel=3).return_mid is False
    for other in ("STF", "ckbd"):  # the attribute is ELIC's alone: the other single-modal classes have no *_mid path to select
        assert not hasattr(rgbd_amd.modelZoo[other](), "return_mid")


def test_state_dict_names_and_shapes_are_the_references():
    from rgbd_amd import Spatial_aligner, arch

    with open(os.path.join(ROOT, "tests", "golden", "aligner_state_dict.json")) as f:
        ref = [(n, tuple(s)) for n, s in json.load(f)]
    sa = Spatial_aligner(in_channel=192, out_channel=192)
    assert [(n, tuple(t.shape)) for n, t in sa.state_dict().items()] == ref
    e = arch.spatial_aligner_entries(64, 96, prefix="g_s.sp1")
    assert list(e) == ["g_s.sp1." + n for n, _ in ref]
    assert e["g_s.sp1.patch_embeding2.weight"].shape == (96, 64, 2, 2) and e["g_s.sp1.recovery.weight"].shape == (96, 96, 2, 2)
    assert e["g_s.sp1.blocks.1.attn.qkv2.weight"].shape == (192, 96)


def test_strict_loading():
    from rgbd_amd import Spatial_aligner, synth

    sd = synth.synthetic_state_dict(3, model="Spatial_aligner", in_channel=64, out_channel=96)
    sa = Spatial_aligner(in_channel=64, out_channel=96)
    sa.load_state_dict(sd, strict=True)
    assert all(torch.equal(sa.state_dict()[k], v) for k, v in sd.items())
    less = {k: v for k, v in sd.items() if k != "blocks.1.attn.qkv2.bias"}
    with pytest.raises(RuntimeError):
        sa.load_state_dict(less, strict=True)
    with pytest.raises(RuntimeError):
        sa.load_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)
    with pytest.raises(RuntimeError):
        Spatial_aligner(in_channel=192, out_channel=96).load_state_dict(sd, strict=True)  # size mismatch
    sa.load_state_dict({k: v for k, v in sd.items() if not k.endswith("relative_position_index")}, strict=False)


def test_synthetic_weights_leave_the_other_models_alone():
    from rgbd_amd import synth

    a = synth.synthetic_state_dict(5, model="Spatial_aligner")
    assert float(a["blocks.0.attn.relative_position_bias_table"].abs().max()) > 1.0
    assert float((a["blocks.1.norm1.weight"] - 1).abs().max()) > 0.3
    b = synth.synthetic_state_dict(5, model="STF", stress=False)
    assert abs(float(b["layers.0.blocks.0.attn.relative_position_bias_table"].std()) - 0.3) < 0.05


def test_new_symbols_are_exported_and_declared():
    from rgbd_amd import _lib

    with open(os.path.join(ROOT, "include", "rgbd_amd.h")) as f:
        hdr = f.read()
    for sym in ("rgbd_guided_window_attention", "rgbd_aligner_create", "rgbd_aligner_forward", "rgbd_elic_decompress_single_mid",
                "rgbd_elic_forward_single_mid"):
        assert sym in _lib.EXPORTS
        assert re.search(r"\bint " + sym + r"\(", hdr), sym
