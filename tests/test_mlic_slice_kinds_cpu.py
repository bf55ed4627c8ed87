"""What rgbd_elic_finalize takes the state-dict entries of MLIC++'s per-slice networks for (families 15 to 17 of
csrc/engine_abi.hip's tensor_kind, through the host-only hook rgbd_debug_tensor_kind), over the names arch gives them, and the
arch shape lists against the reference's (tests/golden/mlicslice_state_dict.json).  No GPU."""
import ctypes
import json
import os

import pytest

import mlic_slice_cases as mc
from rgbd_amd import arch
from rgbd_amd._lib import lib

IGNORED, RECOVERY, DENSE, CONV, DECONV, GDN, LINEAR, ARRAY, QUANTILES, PIXEL_MLP = range(10)  # RGBD_KIND_* of include/rgbd_amd.h
FAMILY = {"EntropyParametersMLIC": 15, "ChannelContext": 16, "LatentResidualPrediction": 17}
ENTRIES = {"EntropyParametersMLIC": arch.entropy_params_mlic_entries, "ChannelContext": arch.channel_context_entries,
           "LatentResidualPrediction": arch.lrp_entries}


def kind(family, name, shape):
    return lib().rgbd_debug_tensor_kind(family, name.encode(), (ctypes.c_int64 * len(shape))(*shape), len(shape))


@pytest.mark.parametrize("mod", list(mc.MODULES))
def test_every_entry_as_uploaded(mod):
    cls, kw, _ = mc.MODULES[mod]
    entries = ENTRIES[cls](**kw)
    prefix = {"EntropyParametersMLIC": "fusion.", "ChannelContext": "fushion.", "LatentResidualPrediction": "lrp_transform."}[cls]
    layers = (0, 2, 4) if cls == "ChannelContext" else (0, 2, 4, 6)
    assert list(entries) == [f"{prefix}{i}.{p}" for i in layers for p in ("weight", "bias")]
    for name, e in entries.items():
        want = IGNORED if e.kind == "bias" else (PIXEL_MLP if cls == "EntropyParametersMLIC" else CONV)
        assert kind(FAMILY[cls], name, tuple(e.shape)) == want, (name, e.shape)


def test_the_fragment_kind_is_this_family_and_this_name_only():
    assert kind(15, "fusion.0.weight", (320, 640, 1, 1)) == PIXEL_MLP
    assert kind(15, "fusion.0.weight", (320, 640, 3, 3)) == CONV
    assert kind(15, "other.0.weight", (320, 640, 1, 1)) == CONV
    for family in (1, 7, 16, 17):
        assert kind(family, "fusion.0.weight", (320, 640, 1, 1)) == CONV
    assert kind(16, "fushion.2.weight", (128, 192, 3, 3)) == CONV
    assert kind(17, "lrp_transform.4.weight", (120, 208, 3, 3)) == CONV


def test_family_14_stays_a_hole():
    assert kind(14, "fusion.0.weight", (320, 640, 1, 1)) == -22
    assert kind(18, "fusion.0.weight", (320, 640, 1, 1)) == -22


@pytest.mark.parametrize("mod", list(mc.MODULES) + list(mc.SHAPE_ONLY))
def test_arch_shape_lists_equal_the_reference(mod):
    with open(os.path.join(mc.GOLDEN, "mlicslice_state_dict.json")) as f:
        want = json.load(f)[mod]
    cls, kw = (mc.MODULES.get(mod) or mc.SHAPE_ONLY[mod])[:2]
    assert [[k, list(e.shape)] for k, e in ENTRIES[cls](**kw).items()] == want


def test_host_refusals_need_no_gpu():
    L = lib()
    h = ctypes.c_void_p()
    for fn, args in (("rgbd_entropy_params_mlic_create", (650, 64)), ("rgbd_entropy_params_mlic_create", (976, 64)),
                     ("rgbd_entropy_params_mlic_create", (640, 144)), ("rgbd_entropy_params_mlic_create", (640, 40)),
                     ("rgbd_channel_context_create", (0, 32)), ("rgbd_lrp_create", (32, 640)), ("rgbd_lrp_create", (0, 32))):
        assert getattr(L, fn)(*args, ctypes.byref(h)) == -22 and not h.value, (fn, args)
    assert L.rgbd_entropy_params_mlic_create(640, 64, None) == -22
    assert L.rgbd_entropy_params_mlic_set_fused(None, 1) == -22
    assert L.rgbd_channel_context_forward(None, None, 1, 4, 4, None, None) == -22
    assert L.rgbd_lrp_forward(None, None, 1, 4, 4, None, None) == -22
    assert L.rgbd_entropy_params_mlic_forward(None, None, None, 1, 1, 4, 4, -1, None, None) == -22
    assert L.rgbd_pixel_mlp4(None, None, None, 1, None, None, 64, 1, 4, 4, -1, None, 64, None) == -22
