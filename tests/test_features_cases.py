"""tests/features_cases.py against the fixtures of the unmodified reference (tests/golden/features_*.npz), on the CPU:

  * the fp64 statement of either module reproduces every fixture's fp32 output within the fixture's own e_ref (the
    reference's fp32 run against its float64 run), and the fp32 statement is accepted;
  * the operators' statements: the deconvolution handed over in convolution orientation is torch's conv_transpose2d, and
    every wrong reading of the taps or the bias is rejected;
  * the acceptance function rejects each deliberate mistake of the modules -- for every mistake on a case with an interior and
    on the largest map;
  * the state-dict entries of the package are those of the reference (names, order, shapes), and the new symbols are declared
    and exported."""
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

import features_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(fc.CASES))
def test_module_statement_reproduces_reference(name):
    fx = fc.load_fixture(name)
    assert int(fx["input_seed"]) == fc.CASES[name][4] and int(fx["weight_seed"]) == fc.WEIGHT_SEED
    ref = fc.module_statement(name)
    pos = fc.positions(name, ref.numel())
    ref32 = torch.from_numpy(fx["ref32"])
    assert ref32.shape == pos.shape
    e = fc.rel_err(ref32, ref.reshape(-1)[pos])
    print(f"{name}: fixture fp32 vs fp64 statement {e:.3e} at {len(pos)} positions, e_ref {fx['e_ref']:.3e}")
    assert 5e-8 < fx["e_ref"] < 5e-6  # an fp32 run's error, not an accident
    # (at the stored positions the error is at most the one over the whole output; their largest value may be smaller.  1e-13:
    # the statement and the reference's float64 run add in different orders, a few hundred ulps of 1.1e-16 at most)
    assert e <= fx["e_ref"] * float(ref.abs().max() / ref.reshape(-1)[pos].abs().max()) + 1e-13
    assert fc.accept(fc.rel_err(fc.module_statement(name, dtype=torch.float32), ref), fx["e_ref"])


MUTATION_SIZES = ("3x3", "13x7", fc.LARGEST)  # the smallest map with an interior, an odd one, the largest


@pytest.mark.parametrize("net", list(fc.NETS))
def test_module_mistakes_are_rejected(net):
    for size in MUTATION_SIZES:
        name = f"{net}_{size}"
        e_ref = fc.load_fixture(name)["e_ref"]
        ref = fc.module_statement(name)
        for mut in fc.mutations_of(net):
            e = fc.rel_err(fc.module_statement(name, mut), ref)
            print(f"{name} {mut}: {e:.3e} vs bound {fc.FACTOR * max(e_ref, fc.FLOOR):.3e}")
            assert not fc.accept(e, e_ref), (name, mut)
            # no near miss either (the smallest margin is one output channel's deconv1 bias, 3e-4 of the largest output)
            assert e > 10 * fc.FACTOR * max(e_ref, fc.FLOOR), (name, mut)


def test_every_mistake_is_tried_on_an_interior_and_on_the_largest():
    assert fc.LARGEST in MUTATION_SIZES and all(f"{net}_{s}" in fc.CASES for net in fc.NETS for s in MUTATION_SIZES)
    assert fc.CASES[f"enc3_{fc.LARGEST}"][2:4] == (67, 129)
    for mut in fc.MODULE_MUTATIONS:
        assert any(mut in fc.mutations_of(net) for net in fc.NETS), mut


@pytest.mark.parametrize("co", [1, 3])
def test_deconv_in_convolution_orientation_is_conv_transpose(co):
    g = torch.Generator().manual_seed(co)
    x = torch.randn(2, 64, 5, 6, generator=g, dtype=torch.float64)
    t = torch.randn(64, co, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(co, generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(x, t, b, stride=1, padding=1)
    got = fc.thin_out(x.permute(0, 2, 3, 1), fc.deconv_as_conv(t), b)
    assert fc.rel_err(got, want) <= 1e-14
    for mut in ("taps_not_flipped", "axes_not_exchanged")[:2 if co > 1 else 1]:  # (one channel: [64][1] is [1][64] as it lies)
        assert fc.rel_err(fc.thin_out(x.permute(0, 2, 3, 1), fc.deconv_as_conv(t, mut), b), want) > 0.1, mut


@pytest.mark.parametrize("op", ["thin_in", "thin_out"])
def test_kernel_mistakes_are_rejected(op):
    cases = fc.THIN_IN_CASES if op == "thin_in" else fc.THIN_OUT_CASES
    f = fc.thin_in if op == "thin_in" else fc.thin_out
    for name, (B, H, W, ci, co, _) in cases.items():
        x, w, b = fc.kernel_inputs(op, name)
        ref, e_ref = fc.kernel_refs(op, name)
        assert ref.shape == ((B, H, W, co) if op == "thin_in" else (B, co, H, W))
        assert e_ref < 5e-6
        for mut in fc.KERNEL_MUTATIONS:
            if H * W == 1 and mut != "bias_dropped":
                continue  # (one pixel: only the centre tap sees anything)
            e = fc.rel_err(f(x, w, b, mut), ref)
            assert e > 100 * fc.FACTOR * max(e_ref, fc.FLOOR), (name, mut, e)


def test_entries_are_the_reference_state_dict():
    from rgbd_amd import arch

    with open(os.path.join(fc.GOLDEN, "features_state_dict.json")) as f:
        want = json.load(f)
    for net, (model, ci, co) in fc.NETS.items():
        entries = arch.feature_encoder_entries(ci) if model == "Feature_encoder" else arch.feature_decoder_entries(ci, co)
        assert [[k, list(e.shape)] for k, e in entries.items()] == want[net], net
        assert [[k, list(v.shape)] for k, v in fc.net_weights(net).items()] == want[net], net
    # in_channel 64: the first block has no `skip` (res_blk.py:43-46)
    assert "resblock1.skip.weight" not in arch.feature_decoder_entries(64, 3)


NEW_SYMBOLS = ["rgbd_conv3x3_thin_in", "rgbd_conv3x3_thin_out"]


def test_new_symbols_are_declared_and_exported():
    from rgbd_amd import _lib

    with open(os.path.join(ROOT, "include", "rgbd_amd.h")) as f:
        hdr = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s
        assert s in _lib.EXPORTS, s
    assert "thin_conv.hip" in _lib._SRCS
