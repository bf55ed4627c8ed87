"""MLIC++ (rgbd_amd.mlic, reference models/mlicpp.py) without a GPU: the parameter inventory against the reference's state_dict
(tests/golden/mlic_keys.json), the restatement (tests/mlic_ref.py) against what the unmodified reference produced
(tests/golden/mlic_*.npz, written by tests/golden/make_mlic.py) -- in fp32 symbols, indexes and the y stream exactly, in fp64
outside the near-boundary set --, every deliberate mistake of the restatement changing the symbols of every fixture, what
finalize takes each tensor of family 19 for, and the model lookup by name."""
import collections
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mlic_ref
from rgbd_amd import MLICPlusPlus, arch, synth  # (the feature: without it this import fails)
from rgbd_amd._lib import lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["s2_128x128", "s3_b2_128x192", "full_128x128", "s2_448x192", "s2_b2_192x128"]
ROUND_WINDOW = SCALE_WINDOW = 2e-4  # tests/golden/make_margins.py
FAMILY = 19
IGNORED, RECOVERY, DENSE, CONV, DECONV, GDN, LINEAR, ARRAY, QUANTILES, PIXEL_MLP = range(10)  # RGBD_KIND_* of include/rgbd_amd.h


def fixture_of(name):
    return dict(np.load(os.path.join(GOLDEN, f"mlic_{name}.npz")))


def image_of(g):
    r, _ = synth.synthetic_batch(int(g["B"]), int(g["H"]), int(g["W"]), config_id=int(g["config_id"]))
    return torch.from_numpy(r)


_SD, _RUNS = {}, {}


def weights_of(g):
    key = (int(g["seed"]), int(g["N"]), int(g["M"]))
    if key not in _SD:
        _SD[key] = synth.synthetic_state_dict(key[0], model="MLIC", N=key[1], M=key[2])
    return _SD[key]


def run(name, dtype=torch.float32, mistake=None, forced=False):
    """(compress() output, trace) of the restatement on a fixture's weights and image, computed once."""
    key = (name, dtype, mistake, forced)
    if key not in _RUNS:
        g = fixture_of(name)
        r = mlic_ref.MlicRef(weights_of(g), dtype=dtype, mistake=mistake)
        assert r.update()
        r.trace = {}
        kw = {"forced_y": g["symbols"].astype(np.int32), "forced_z": g["z_symbols"].astype(np.int32).reshape(-1)} if forced else {}
        _RUNS[key] = (r.compress(image_of(g), **kw), r.trace)
    return _RUNS[key]


def near_boundary(x, s, table):
    x, s = np.asarray(x, np.float64), np.asarray(s, np.float64)
    m_round = 0.5 - np.abs(x - np.rint(x))
    rel = np.abs(s[:, None] / table[None, :-1] - 1.0).min(axis=1)
    return (m_round <= ROUND_WINDOW * np.maximum(1.0, np.abs(x))) | (rel <= SCALE_WINDOW)


def test_entries_match_the_reference_state_dict():
    with open(os.path.join(GOLDEN, "mlic_keys.json")) as f:
        keys = json.load(f)
    entries = arch.mlic_entries(keys["N"], keys["M"], keys["slice_num"], keys["channel"])
    assert list(entries) == list(keys["keys"])  # names in the reference's order, its None slots at i = 0 included
    for name, e in entries.items():
        want = keys["keys"][name]
        if e.kind == "buffer" and not all(e.shape):  # tables that update() sizes
            continue
        assert list(e.shape) == want, name
    assert len(entries) == keys["n_tensors"]
    assert arch.count_parameters(entries) == keys["n_parameters"]
    for i in range(keys["slice_num"]):
        for kind in ("channel_context", "global_inter_context", "global_intra_context"):
            assert any(k.startswith(f"{kind}.{i}.") for k in entries) == (i > 0)
    cfg = arch.mlic_config()
    assert (cfg["N"], cfg["M"], cfg["slice_num"], cfg["slice_ch"]) == (192, 320, 10, [32] * 10)
    net = MLICPlusPlus(N=64, M=64, slice_num=2)
    assert (net.N, net.M, net.slice_num, net.channel) == (64, 64, 2, 3) and list(net.state_dict()) == list(arch.mlic_entries(64, 64, 2, 3))
    for bad in ({"M": 300}, {"slice_num": 1, "M": 32}, {"slice_num": 11, "M": 352}):
        with pytest.raises((ValueError, NotImplementedError)):
            MLICPlusPlus(**{"N": 192, "M": 320, "slice_num": 10, **bad})


def test_reference_order_attention_is_the_einsum_statement():
    """mlic_ref states the two attention cores in the reference's operation order; tests/mlic_context_cases.py states them as
    einsums (the yardstick of families 7-9).  In fp64 they are the same function to rounding."""
    import mlic_context_cases as cc

    gen = torch.Generator().manual_seed(1)
    for model, kw, heads in (("LocalContext", {"dim": 32}, 2), ("LinearGlobalInterContext", {"dim": 96, "out_dim": 64}, 3),
                             ("LinearGlobalIntraContext", {"dim": 32}, 2)):
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in synth.synthetic_state_dict(7, model=model, **kw).items()}
        x = torch.randn(2, kw["dim"], 6, 8, generator=gen, dtype=torch.float64) * 3
        x2 = torch.randn(2, kw["dim"], 6, 8, generator=gen, dtype=torch.float64)
        if model == "LocalContext":
            a, b = mlic_ref.local_context(sd, x), cc.local_context(sd, x)
        else:
            second = x2 if model == "LinearGlobalIntraContext" else None
            a, b = mlic_ref.linear_context(sd, x, second, heads), cc.linear_context(sd, x, second, heads)
        assert float((a - b).abs().max() / b.abs().max()) < 1e-13, model


@pytest.mark.parametrize("name", CASES)
def test_fp32_restatement_reproduces_the_reference(name):
    g = fixture_of(name)
    out, tr = run(name)
    assert np.array_equal(tr["symbols"], g["symbols"].astype(np.int32))
    assert np.array_equal(tr["indexes"], g["indexes"].astype(np.int32))
    assert out["strings"][0][0] == g["y_stream"].tobytes()
    assert [bytes(s) for s in out["strings"][1]] == [g[f"z{i}"].tobytes() for i in range(int(g["B"]))]
    assert np.array_equal(tr["z_symbols"].numpy().astype(np.int16), g["z_symbols"])
    assert tuple(out["shape"]) == tuple(g["shape"])
    # the same arithmetic on the same CPU: what the reference rounded and indexed, bit for bit
    assert np.array_equal(tr["x"].astype(np.float32), g["x"]) and np.array_equal(tr["sigma"].astype(np.float32), g["sigma"])


@pytest.mark.parametrize("name", CASES)
def test_fp64_restatement_agrees_outside_the_near_boundary_set(name):
    """Under the reference's symbols (so that every part sees the reference's context) the fp64 decisions are the reference's
    wherever the reference's own floats are not inside a near-boundary window."""
    g = fixture_of(name)
    _, tr = run(name, torch.float64, forced=True)
    table = mlic_ref.eo.scale_table().numpy().astype(np.float64)
    near = near_boundary(g["x"], g["sigma"], table.astype(np.float32))
    assert near.mean() <= 0.005
    sym64 = np.rint(tr["x"]).astype(np.int32)
    idx64 = np.searchsorted(table[:-1], np.maximum(tr["sigma"], float(np.float32(0.11))), side="left")  # (the bound is the fp32 buffer 0.11f = table[0]).astype(np.int32)
    differ = (sym64 != g["symbols"]) | (idx64 != g["indexes"])
    assert not (differ & ~near).any(), int((differ & ~near).sum())
    # the recorded fp64 floats are this restatement's
    assert np.array_equal(tr["x"], g["x64"]) and np.array_equal(tr["sigma"], g["sigma64"])
    assert np.abs(tr["x"] - g["x"]).max() / np.abs(tr["x"]).max() == pytest.approx(float(g["e_ref_x"]), rel=1e-6)


@pytest.mark.parametrize("mistake", mlic_ref.MISTAKES)
@pytest.mark.parametrize("name", CASES)
def test_every_mistake_changes_the_symbols(name, mistake):
    g = fixture_of(name)
    _, tr = run(name, mistake=mistake)
    changed = (tr["symbols"] != g["symbols"]) | (tr["indexes"] != g["indexes"])
    if mistake == "intra_first_slice" and int(g["slice_num"]) == 2:
        # with two slices y_hat_slices[0] IS y_hat_slices[-1] when the only intra context runs: the one pair where the
        # mistake is no mistake (the three-slice fixture is there to tell them apart)
        assert not changed.any()
    else:
        assert changed.mean() > 0.001, (mistake, int(changed.sum()))
    _RUNS.pop((name, torch.float32, mistake, False))  # (nothing else reads it)


def kind(name, shape):
    arr = (ctypes.c_int64 * len(shape))(*shape)
    return lib().rgbd_debug_tensor_kind(FAMILY, name.encode(), arr, len(shape))


@pytest.mark.parametrize("channel", [3, 1])
def test_finalize_kinds_of_the_mlic_family(channel):
    """Parameters as the engine receives them (an nn.Linear of LocalContext as the 1x1 convolution EngineModule._upload makes of
    it): the kinds follow the prefixed names."""
    by_entry = {"bias": IGNORED, "eb_bias": IGNORED, "eb_factor": IGNORED, "eb_matrix": IGNORED, "gdn_beta": IGNORED, "conv_w": CONV,
                "linear_w": CONV, "gdn_gamma": GDN, "ln_w": ARRAY, "ln_b": ARRAY, "rpb_table": ARRAY, "eb_quantiles": QUANTILES}
    got = collections.Counter()
    S = 3
    for name, e in arch.mlic_entries(64, 32 * S, S, channel).items():
        if not e.is_param:
            continue
        shape = e.shape + (1, 1) if e.kind == "linear_w" else e.shape
        want = by_entry[e.kind]
        ctx = name.startswith(("local_context.", "global_inter_context.", "global_intra_context."))
        if e.kind == "conv_w" and ctx and (shape[1:] == (1, 3, 3) or name.endswith(".fusion.weight")):
            want = DENSE  # depthwise layers of the contexts and LocalContext.fusion
        if e.kind == "conv_w" and name.startswith("entropy_parameters_") and ".fusion." in name:
            want = PIXEL_MLP
        assert kind(name, shape) == want, (name, shape)
        got[want] += 1
    # the first analysis conv of a one-channel model is [N][1][3][3] like a depthwise layer: it stays a convolution
    assert kind("g_a.analysis_transform.0.conv1.weight", (64, 1, 3, 3)) == CONV
    # no transposed convolution in this family, whatever the other families take the name for
    assert kind("h_s.increase.0.weight", (96, 64, 3, 3)) == CONV and kind("h_s.increase.8.weight", (192, 144, 3, 3)) == CONV
    assert got[PIXEL_MLP] == 2 * S * 4 and got[DENSE] == S + 2 * (S - 1) * 4 and got[GDN] == 6 and got[QUANTILES] == 1
    assert got[ARRAY] == S * 5 and DECONV not in got and LINEAR not in got


def test_model_lookup_by_name():
    """The testers take the first table name that is a substring of the model name (tester.py get_net -> rgbd_amd.zoo_lookup):
    modelZoo as it was, then the younger entries."""
    import rgbd_amd

    assert rgbd_amd.zoo_lookup("MLIC") is MLICPlusPlus and rgbd_amd.zoo_lookup("MLIC_q3") is MLICPlusPlus
    assert rgbd_amd.modelZooExtra["MLIC"] is MLICPlusPlus and "MLIC" not in rgbd_amd.modelZoo
    assert MLICPlusPlus._MODEL == "MLIC" and len(MLICPlusPlus._MODALITIES) == 1

    def before(model_name):  # the lookup as the testers did it until now
        for name, cls in rgbd_amd.modelZoo.items():
            if model_name.find(name) != -1:
                return cls
        return None

    for model_name in ("ELIC_united_R2D", "ELIC_united", "ELIC", "STF_united", "STF", "ckbd", "ELIC_united_R2D_q2", "ELIC_master",
                       "nyuv2_rgb_STF_2_2", "cheng", ""):
        assert rgbd_amd.zoo_lookup(model_name) is before(model_name), model_name
    assert before("ELIC_united_R2D") is rgbd_amd.ELIC_united_R2D and before("ckbd") is rgbd_amd.Cheng2020AnchorwithCheckerboard
    assert before("cheng") is None and before("MLIC") is None
    # the single-image tester builds it with MLIC's own configuration
    import types

    from rgbd_amd import tester

    class T(tester.TesterSingle):
        def get_net(self, cfg, model_name, ckpt):
            self.seen = (cfg, rgbd_amd.zoo_lookup(model_name))
            return 0

    t = T(types.SimpleNamespace(channel=3, debug=False, experiment="x", model="MLIC", quality="2_2", checkpoint=None, dataset=None))
    assert t.seen[1] is MLICPlusPlus and (t.seen[0]["M"], t.seen[0]["slice_num"]) == (320, 10)
    assert MLICPlusPlus(config=t.seen[0], channel=3).slice_ch == [32] * 10


@pytest.mark.parametrize("tester_name", ["TesterSingle", "TesterUnited"])
def test_tester_takes_the_configuration_by_model_name(tester_name):
    """playground/test.py:29-32: without a configuration of the caller's, a model name with "MLIC" in it selects MLIC's own and
    every other name the common one (tester.py; no model is built: the tester is handed a stand-in net)."""
    import types

    import rgbd_amd

    cls = getattr(rgbd_amd, tester_name)
    for model, want in (("MLIC", arch.mlic_config()), ("MLIC_q3", arch.mlic_config()), ("nyuv2_rgb_MLIC_1", arch.mlic_config()),
                        ("ELIC", arch.model_config()), ("STF", arch.model_config()), ("ckbd", arch.model_config()),
                        ("ELIC_united", arch.model_config()), ("mlic", arch.model_config())):
        args = types.SimpleNamespace(channel=3, debug=False, experiment="x", dataset=None, model=model, quality="1", checkpoint=None)
        stand_in = object()
        t = cls(args, None, net=stand_in)
        assert t.model_config == want and t.net is stand_in and t.epoch == 0, model
        assert (t.model_config == arch.mlic_config()) == ("MLIC" in model), model  # (the two configurations differ)
    own = arch.mlic_config(64, 64, 2)
    args = types.SimpleNamespace(channel=3, debug=False, experiment="x", dataset=None, model="MLIC", quality="1", checkpoint=None)
    assert rgbd_amd.TesterSingle(args, own, net=object()).model_config is own  # the caller's configuration wins


def test_host_side_refusals():
    net = MLICPlusPlus(N=64, M=64, slice_num=2).eval()
    with pytest.raises(rgbd_amd_error()):
        net.to("cpu")
    net._ready = lambda: None
    net._device = torch.device("cpu")
    for H, W in ((64, 128), (128, 64), (100, 128), (128, 192 + 32)):
        with pytest.raises(ValueError):
            net.compress(torch.zeros(1, 3, H, W))
        with pytest.raises(ValueError):
            net.forward(torch.zeros(1, 3, H, W))
    with pytest.raises(ValueError):
        net.decompress([[b""], [b""]], (1, 2))
    with pytest.raises(ValueError):
        net.compress(torch.zeros(1, 1, 128, 128))
    # the C ABI refuses what the model does not have before it creates anything
    h = ctypes.c_void_p()
    for N, M, S, ch in ((64, 64, 1, 3), (64, 352, 11, 3), (64, 96, 2, 3), (60, 64, 2, 3), (64, 64, 2, 0), (0, 64, 2, 3)):
        assert lib().rgbd_elic_create_mlic(N, M, S, ch, ctypes.byref(h)) == -22 and not h.value
    assert lib().rgbd_elic_create_mlic(64, 64, 2, 3, None) == -22
    # the two slot kernels refuse bad arguments before any launch (no GPU is touched)
    for args in ((None, 32, 32, 1, 2, 2, 0), (64, 32, 16, 1, 2, 2, 0), (64, 30, 32, 1, 2, 2, 0), (64, 32, 32, 1, 0, 2, 0),
                 (64, 32, 32, 1, 2, 0, 0), (68, 32, 32, 1, 2, 2, 0), (64, 32, 32, 1, 2, 2, 2), (64, 16, 32, 1, 2, 2, 0)):
        p, cs, ch, B, hh, ww, par = args
        assert lib().rgbd_mlic_slot_clear(p, cs, ch, B, hh, ww, par, None) == -22, args
        assert lib().rgbd_mlic_lrp_apply(p, cs, 128, 32, ch, B, hh, ww, par, None) == -22, args
    assert lib().rgbd_mlic_lrp_apply(64, 32, 64, 32, 32, 1, 2, 2, 0, None) == -22  # r is the slot


def rgbd_amd_error():
    import rgbd_amd

    return rgbd_amd.RgbdError
