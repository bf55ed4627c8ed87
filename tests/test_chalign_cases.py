"""tests/chalign_cases.py against torch's convolution and the fixtures of the unmodified reference (tests/golden/chalign_*.npz),
on the CPU:

  * the fp64 statement of the pooled head (nine border sums and a product) is F.conv2d(...).mean((2, 3)) in fp64 on every
    kernel case, degenerate maps included;
  * the fp64 statement of the module reproduces every fixture's beta64 and gamma64;
  * the acceptance function rejects each deliberate mistake on every case where it can show at all -- for every mistake that
    includes a case of at least 3x3 and the largest one;
  * the state-dict entries of the package are those of the reference (names, order, shapes), and the new symbols are
    declared and exported."""
import json
import os
import re

import pytest
import torch

import chalign_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(cc.KERNEL_CASES))
def test_head_statement_is_conv_then_mean(name):
    x, w, b = cc.kernel_inputs(name)
    e = cc.rel_err(cc.pooled_head(x, w, b), cc.conv_mean(x, w, b))
    print(f"{name}: border-sum form vs conv2d().mean() in fp64 {e:.3e}; fp32 statement e_ref {cc.kernel_e_ref(name):.3e}")
    assert e <= 1e-14


@pytest.mark.parametrize("name", list(cc.KERNEL_CASES))
def test_head_mistakes_are_rejected(name):
    B, H, W = cc.KERNEL_CASES[name][:3]
    x, w, b = cc.kernel_inputs(name)
    ref, e_ref = cc.pooled_head(x, w, b), cc.kernel_e_ref(name)
    assert cc.accept(cc.rel_err(cc.pooled_head(x, w, b, dtype=torch.float32), ref), e_ref)
    for mut, shows in cc.HEAD_MUTATIONS.items():
        e = cc.rel_err(cc.pooled_head(x, w, b, mut), ref)
        print(f"{name} {mut}: {e:.3e} vs bound {cc.FACTOR * max(e_ref, cc.FLOOR):.3e}")
        if shows(H, W):
            assert not cc.accept(e, e_ref), mut
            assert e > 100 * cc.FACTOR * max(e_ref, cc.FLOOR), mut  # orders of magnitude out, not a near miss


def test_every_mistake_shows_on_a_3x3_and_on_the_largest():
    for mut, shows in cc.HEAD_MUTATIONS.items():
        assert any(shows(h, w) and h >= 3 and w >= 3 for _, h, w in cc.SIZES) and shows(67, 129), mut
    assert cc.LARGEST in cc.CASES and cc.CASES[cc.LARGEST][1:3] == (67, 129)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_module_statement_reproduces_reference(name):
    fx = cc.load_fixture(name)
    B = cc.CASES[name][0]
    assert int(fx["input_seed"]) == cc.CASES[name][3] and int(fx["weight_seed"]) == cc.WEIGHT_SEED
    got = cc.module_statement(name)
    for b in range(1, B + 1):
        for key, (e, e_ref) in cc.module_errors(name, fx, got, b).items():
            print(f"{name} B={b} {key}: statement vs fixture {e:.3e}, e_ref {e_ref:.3e}")
            assert 1e-8 < e_ref < 5e-6  # an fp32 run's error, not an accident
            assert e <= 1.2e-7  # beta64 / gamma64 are stored rounded to fp32: 6e-8 of their own
        assert cc.module_accepts(name, fx, got, b)
    # the fp32 results are the same run the floors were taken from
    for key in ("beta", "gamma"):
        assert cc.rel_err(fx[f"{key}32"], fx[f"{key}64"]) <= float(fx["floors"][key][str(B)]) + 1.2e-7


@pytest.mark.parametrize("name", list(cc.CASES))
def test_module_mistakes_are_rejected(name):
    fx = cc.load_fixture(name)
    B, H, W = cc.CASES[name][:3]
    for mut in list(cc.HEAD_MUTATIONS) + cc.MODULE_MUTATIONS:
        if mut in cc.HEAD_MUTATIONS and not cc.HEAD_MUTATIONS[mut](H, W):
            continue
        got = cc.module_statement(name, mut)
        errs = cc.module_errors(name, fx, got, B)
        print(f"{name} {mut}: " + ", ".join(f"{k} {e:.3e} (e_ref {r:.3e})" for k, (e, r) in errs.items()))
        assert not cc.module_accepts(name, fx, got, B), mut
        # (no near miss either; the smallest is the corner term on the largest map, four pixels of 8643 with plain borders)
        assert max(e / (cc.FACTOR * max(r, cc.FLOOR)) for e, r in errs.values()) > 10, mut


def test_entries_are_the_reference_state_dict():
    from rgbd_amd import arch

    with open(os.path.join(cc.GOLDEN, "chalign_state_dict.json")) as f:
        want = json.load(f)
    assert [[k, list(e.shape)] for k, e in arch.channel_aligner_entries().items()] == want
    assert [[k, list(v.shape)] for k, v in cc.module_weights().items()] == want


NEW_SYMBOLS = ["rgbd_pooled_conv3x3_ws_floats", "rgbd_pooled_conv3x3"]


def test_new_symbols_are_declared_and_exported():
    from rgbd_amd import _lib

    with open(os.path.join(ROOT, "include", "rgbd_amd.h")) as f:
        hdr = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s
        assert s in _lib.EXPORTS, s
    assert "pooled_head.hip" in _lib._SRCS
