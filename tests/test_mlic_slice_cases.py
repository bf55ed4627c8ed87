"""tests/mlic_slice_cases.py against the fixtures of the unmodified reference (tests/golden/mlicslice_*.npz), on the CPU:

  * the fp64 statements of the three modules reproduce every fixture's ref64 far inside the acceptance bound, at every batch
    size of the case, and evaluated in fp32 they stay within MARGIN_FP32 of the bound;
  * every GELU of the reference saw both signs beyond GELU_SIDE, and the LRP's tanh arguments in TANH_BAND: the bands the weight
    recipe is built for, on the fixtures and on the statements;
  * each deliberate mistake -- tanh-GELU, a GELU behind the last layer, a dropped bias, exchanged input segments, transposed
    3x3 taps, the dropped 0.5, the dropped tanh -- lands MARGIN_MISTAKE bounds away, on non-square maps;
  * the LRP widths with 3 * (diff // 4) are not the reference's shape list, where the two differ;
  * the state-dict entries of the package are those of the reference (names, order, shapes);
  * the host-side packer of rgbd_pixel_mlp4 orders a weight as the kernel's lanes read it."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mlic_slice_cases as mc


@pytest.mark.parametrize("name", list(mc.CASES))
def test_statement_reproduces_reference(name):
    fx = mc.load_fixture(name)
    ref64 = torch.from_numpy(fx["ref64"])
    mod = mc.CASES[name][0]
    assert int(fx["input_seed"]) == mc.CASES[name][4] and int(fx["weight_seed"]) == mc.MODULES[mod][2]
    for b in mc.case_batches(name):
        e = mc.rel_err(mc.module_statement(name, b), ref64[:b])
        e32 = mc.rel_err(mc.module_statement(name, b, dtype=torch.float32), ref64[:b])
        print(f"{name} B={b}: statement vs ref64 {e:.3e}, in fp32 {e32:.3e}, e_ref {mc.e_ref(fx, b):.3e}, "
              f"fp32 / bound {e32 / (mc.FACTOR * mc.e_ref(fx, b)):.3f}")
        assert 1e-8 < mc.e_ref(fx, b) < 5e-6  # an fp32 run's error, not an accident
        assert e <= 0.5 * mc.e_ref(fx, b)  # ref64 is stored rounded to fp32: 6e-8 of its own
        assert e32 <= mc.MARGIN_FP32 * mc.FACTOR * mc.e_ref(fx, b)
    # the strided fp32 output is the same run the floor was taken from
    s = int(fx["ref32_stride"])
    assert mc.rel_err(fx["ref32"], ref64[:, ::s]) <= mc.e_ref(fx, mc.case_batches(name)[-1]) + 1.2e-7  # (ref64's own rounding)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_activation_arguments_in_band(name):
    fx = mc.load_fixture(name)
    cls = mc.MODULES[mc.CASES[name][0]][0]
    seen, pretanh = [], []
    mc.module_statement(name, mc.CASES[name][1], seen=seen, pretanh=pretanh)
    assert len(fx["gelu_min"]) == len(seen) == (2 if cls == "ChannelContext" else 3)
    for (lo, hi), flo, fhi in zip(seen, fx["gelu_min"], fx["gelu_max"]):
        assert abs(lo - flo) <= 1e-6 * abs(flo) and abs(hi - fhi) <= 1e-6 * abs(fhi)  # the statement sees what the reference saw
        assert flo <= -mc.GELU_SIDE and fhi >= mc.GELU_SIDE and max(-flo, fhi) <= mc.GELU_MAX, (flo, fhi)
    assert list(fx["floors"]["gelu_min"]) == list(fx["gelu_min"])
    if cls == "LatentResidualPrediction":
        assert abs(pretanh[0] - float(fx["max_pretanh"])) <= 1e-6 * pretanh[0]
        assert mc.TANH_BAND[0] <= float(fx["max_pretanh"]) <= mc.TANH_BAND[1]
    else:
        assert "max_pretanh" not in fx


MISTAKE_CASES = [(f"{mod}_{size}", mut) for mod in mc.MODULES for size in ("8x12", "12x8") for mut in mc.mutations_of(mod)]


@pytest.mark.parametrize("name,mut", MISTAKE_CASES)
def test_mistakes_land_outside(name, mut):
    fx = mc.load_fixture(name)
    b = mc.case_batches(name)[-1]
    e = mc.rel_err(mc.module_statement(name, b, mut), torch.from_numpy(fx["ref64"])[:b])
    bound = mc.FACTOR * mc.e_ref(fx, b)
    print(f"{name} {mut}: {e:.3e} vs bound {bound:.3e}: {e / bound:.0f} bounds")
    assert e > mc.MARGIN_MISTAKE * bound


def test_lrp_widths_are_the_reference_integer_divisions():
    from rgbd_amd import arch

    with open(os.path.join(mc.GOLDEN, "mlicslice_state_dict.json")) as f:
        want = json.load(f)
    for mod, (cls, kw, *_) in list(mc.MODULES.items()) + list(mc.SHAPE_ONLY.items()):
        if cls != "LatentResidualPrediction":
            continue
        widths = [want[mod][0][1][1]] + [shape[0] for k, shape in want[mod] if k.endswith(".weight")]
        assert arch.lrp_widths(**kw) == widths
    kw = mc.SHAPE_ONLY["lrp350"][1]
    assert mc.lrp_widths_mistaken(**kw) != arch.lrp_widths(**kw)  # 3 * (318 // 4) = 237, 318 * 3 // 4 = 238
    assert arch.lrp_widths(384, 32) == [384, 296, 208, 120, 32]


@pytest.mark.parametrize("mod", list(mc.MODULES) + list(mc.SHAPE_ONLY))
def test_entries_are_the_reference_state_dict(mod):
    from rgbd_amd import arch, synth

    with open(os.path.join(mc.GOLDEN, "mlicslice_state_dict.json")) as f:
        want = json.load(f)[mod]
    cls, kw = (mc.MODULES.get(mod) or mc.SHAPE_ONLY[mod])[:2]
    ent = {"EntropyParametersMLIC": arch.entropy_params_mlic_entries, "ChannelContext": arch.channel_context_entries,
           "LatentResidualPrediction": arch.lrp_entries}[cls](**kw)
    assert [[k, list(e.shape)] for k, e in ent.items()] == want
    sd = synth.synthetic_state_dict(1, model=cls, **kw)
    assert [[k, list(v.shape)] for k, v in sd.items()] == want


def test_fragment_packer_matches_its_statement():
    from rgbd_amd._lib import lib

    L = lib()
    f32p = ctypes.POINTER(ctypes.c_float)
    for cout, cin in ((16, 16), (64, 128), (320, 704)):
        w = np.arange(cout * cin, dtype=np.float32).reshape(cout, cin)
        out = np.full(cout * cin, -1.0, dtype=np.float32)
        assert L.rgbd_pixel_mlp4_pack(w.ctypes.data_as(f32p), cout, cin, out.ctypes.data_as(f32p)) == 0
        assert np.array_equal(out, mc.pack_fragments(torch.from_numpy(w)).numpy())
    w = np.zeros((24, 16), dtype=np.float32)
    assert L.rgbd_pixel_mlp4_pack(w.ctypes.data_as(f32p), 24, 16, w.ctypes.data_as(f32p)) == -22
    assert L.rgbd_pixel_mlp4_pack(None, 16, 16, w.ctypes.data_as(f32p)) == -22
