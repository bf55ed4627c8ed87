"""The latent codec of ELIC_master without a GPU: the parameter inventory against the reference's recorded state dict, what
finalize takes its entries for (family 20 of rgbd_debug_tensor_kind), the host side of rgbd_amd.MasterLatentCodec, and the
acceptance functions of master_latent_cases.py on the fixtures -- the float64 restatement is accepted, four wrong restatements are
not."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import master_latent_cases as mc
import rgbd_amd
from rgbd_amd import MasterLatentCodec, arch, synth  # (the feature: without it this import fails)
from rgbd_amd._lib import lib

IGNORED, RECOVERY, DENSE, CONV, DECONV, GDN, LINEAR, ARRAY, QUANTILES = range(9)  # RGBD_KIND_* of include/rgbd_amd.h
FAMILY = 20


def kind(family, name, shape):
    return lib().rgbd_debug_tensor_kind(family, name.encode(), (ctypes.c_int64 * len(shape))(*shape), len(shape))


# ---- the inventory ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channel", [3, 1])
def test_entries_are_the_references_state_dict(channel):
    with open(os.path.join(mc.GOLDEN, "master_state_dict.json")) as f:
        want = [(k, tuple(s)) for k, s in json.load(f)[f"channel{channel}"]]
    got = [(k, tuple(e.shape)) for k, e in arch.elic_master_entries(mc.config(), channel).items()]
    assert got == want  # names, shapes and order
    latent = [(k, tuple(e.shape)) for k, e in arch.elic_master_latent_entries(mc.config()).items()]
    assert latent == [(k, s) for k, s in want if not k.startswith(mc.OUTER)]
    assert len(latent) < len(want) and {k.split(".")[0] + "." for k, _ in want if k.startswith(mc.OUTER)} == set(mc.OUTER)


def test_synthetic_weights_compose_the_recipes_of_the_parts():
    cfg = mc.config()
    sd, full = synth.synthetic_state_dict(21, config=cfg, model="ELIC_master_latent"), synth.synthetic_state_dict(21, config=cfg, model="ELIC_master")
    assert list(sd) == list(arch.elic_master_latent_entries(cfg)) and list(full) == list(arch.elic_master_entries(cfg, 3))
    assert all(torch.equal(full[k], v) for k, v in sd.items())
    plain = synth.synthetic_state_dict(21, config=cfg, model="ELIC_master_latent", stress=False)
    single = synth.synthetic_state_dict(21, config=cfg, model="ELIC", channel=3)
    for k in ("h_a.reduction.4.weight", "h_s.increase.4.weight"):  # the single-modal recipe on the hyper path
        assert torch.equal(sd[k], single[k]) and not torch.equal(sd[k], plain[k])
    k = "entropy_parameters_nonanchor.3.fusion.4"  # the EX-net recipe of the united model: head weight x 6, scale-half bias 1
    assert torch.equal(sd[k + ".weight"], plain[k + ".weight"] * np.float32(6.0)) and bool((sd[k + ".bias"][:64] == 1).all())
    # _apply_stress_synplus under g_s. (values are drawn per name, so the gains are checked, not a SynthesisTransformPlus state dict)
    for k, g in (("g_s.synthesis_transform.5.weight", synth.SYNPLUS_DECONV_GAIN), ("g_s.sp2.recovery.weight", synth.SYNPLUS_RECOVERY_GAIN),
                 ("g_s.sp3.blocks.1.attn.qkv1.weight", synth.ALIGNER_QK_GAIN)):
        assert torch.equal(sd[k], plain[k] * np.float32(g)), k
    assert not torch.equal(sd["g_s.sp1.blocks.0.norm1.weight"], plain["g_s.sp1.blocks.0.norm1.weight"])
    assert torch.equal(sd["g_a.analysis_transform.13.weight"], plain["g_a.analysis_transform.13.weight"] * np.float32(synth.MASTER_Y_GAIN))


# ---- tensor kinds -----------------------------------------------------------------------------------------------------------------
def test_every_latent_entry_as_uploaded():
    for name, e in arch.elic_master_latent_entries(mc.config()).items():
        if not e.is_param:
            continue
        shape = tuple(e.shape)
        if e.kind == "linear_w" and ".fc." not in name:  # nn.Linear of the Swin blocks -> 1x1 convolution (engine_module._upload)
            shape = (shape[0], shape[1], 1, 1)
        want = {"conv_w": CONV, "deconv_w": DECONV, "bias": IGNORED, "ln_w": ARRAY, "ln_b": ARRAY, "rpb_table": ARRAY,
                "linear_w": LINEAR if ".fc." in name else CONV, "eb_matrix": IGNORED, "eb_bias": IGNORED, "eb_factor": IGNORED,
                "eb_quantiles": QUANTILES}[e.kind]
        if name.endswith("recovery.weight"):
            want = RECOVERY
        assert kind(FAMILY, name, shape) == want, (name, shape)


def test_kinds_under_g_s_and_of_the_outer_blocks():
    for stage, shape in ((1, (320, 192, 5, 5)), (5, (192, 192, 5, 5)), (10, (192, 192, 5, 5)), (14, (192, 192, 5, 5))):
        assert kind(FAMILY, f"g_s.synthesis_transform.{stage}.weight", shape) == DECONV
    assert kind(FAMILY, "g_s.synthesis_transform.2.branch.2.weight", (96, 96, 3, 3)) == CONV
    for k in (1, 2, 3):
        assert kind(FAMILY, f"g_s.sp{k}.recovery.weight", (96, 192, 2, 2)) == RECOVERY
        for b in (0, 1):
            assert kind(FAMILY, f"g_s.sp{k}.blocks.{b}.norm1.weight", (96,)) == ARRAY
            assert kind(FAMILY, f"g_s.sp{k}.blocks.{b}.norm2.bias", (96,)) == ARRAY
            assert kind(FAMILY, f"g_s.sp{k}.blocks.{b}.attn.relative_position_bias_table", (49, 3)) == ARRAY
    assert kind(FAMILY, "g_a.analysis_transform.0.weight", (192, 128, 5, 5)) == CONV  # 128 channels in: no K-packed first layer
    assert kind(FAMILY, "h_s.increase.4.weight", (480, 640, 3, 3)) == DECONV
    assert kind(FAMILY, "entropy_parameters_anchor.2.se.fc.0.weight", (44, 704)) == LINEAR
    # the outer blocks are not this family's: IGNORED whatever their shape (in family 1 the same names are convolutions)
    for name, e in arch.elic_master_entries(mc.config(), 3).items():
        if name.startswith(mc.OUTER) and e.is_param:
            assert kind(FAMILY, name, tuple(e.shape)) == IGNORED, name
    assert kind(1, "master_encoder.conv1.weight", (64, 3, 3, 3)) == CONV
    # reserved and unclaimed numbers stay refused
    for fam in (10, 11, 12, 14, 18, 21):
        assert kind(fam, "g_a.analysis_transform.0.weight", (192, 128, 5, 5)) == -22


# ---- the class, host side -------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_and_checkpoints_of_the_full_model():
    net = MasterLatentCodec(config=mc.config()).eval()
    assert (net.channel, net.N, net.M, net.slice_ch) == (128, 192, 320, [16, 16, 32, 64, 192])
    sd = mc.weights("a")
    res = net.load_state_dict(sd, strict=True)
    assert res.missing_keys == [] and res.unexpected_keys == []
    assert net.update(force=True)
    back = net.state_dict()
    assert list(back) == list(sd)
    assert all(torch.equal(back[k], sd[k]) for k in sd if not k.endswith(("_offset", "_quantized_cdf", "_cdf_length", "scale_table")))
    assert back["gaussian_conditional._quantized_cdf"].numel() > 0
    other = MasterLatentCodec(config=mc.config())
    other.load_state_dict(back, strict=True)
    assert all(torch.equal(other.state_dict()[k], back[k]) for k in back)
    # a full ELIC_master checkpoint: the latent part loads, the outer blocks are reported
    full = mc.weights("a", full=True)
    res = other.load_state_dict(full, strict=False)
    assert res.missing_keys == [] and res.unexpected_keys == [k for k in full if k.startswith(mc.OUTER)] and len(res.unexpected_keys) > 0
    assert all(torch.equal(other.state_dict()[k], sd[k]) for k in sd if sd[k].is_floating_point() and sd[k].numel())
    with pytest.raises(RuntimeError) as ei:
        other.load_state_dict(full, strict=True)
    assert all(p in str(ei.value) for p in mc.OUTER)
    with pytest.raises(RuntimeError):  # a checkpoint that holds none of its parameters
        other.load_state_dict({k: v for k, v in full.items() if k.startswith(mc.OUTER)}, strict=False)


def test_shape_errors_are_raised_on_the_host():
    net = MasterLatentCodec()
    f, up1, up2, up3 = (torch.zeros(s) for s in ((1, 128, 64, 128), (1, 192, 8, 16), (1, 192, 16, 32), (1, 192, 32, 64)))
    with pytest.raises(ValueError):
        net.compress(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError):
        net.compress(torch.zeros(1, 128, 64, 100))
    with pytest.raises(ValueError):
        net.forward(torch.zeros(1, 128, 96, 64), up1, up2, up3)
    for bad in ((None, up2, up3), (up1, up3, up2), (up1, up2, torch.zeros(2, 192, 32, 64)), (up1, torch.zeros(1, 96, 16, 32), up3)):
        with pytest.raises(ValueError):
            net.forward(f, *bad)
        with pytest.raises(ValueError):
            net.decompress([[b""], [b""]], (1, 2), *bad)
    with pytest.raises(ValueError):
        net.decompress([[b"", b"", b""], [b"", b""]], (1, 2), up1, up2, up3)
    with pytest.raises(ValueError):
        net.decompress([[b""], [b""]], (0, 2), up1, up2, up3)
    with pytest.raises(NotImplementedError):
        net.set_coder("wide", 8)
    assert net.coder == "reference"
    with pytest.raises(NotImplementedError):
        MasterLatentCodec(config=arch.Config({**mc.config(), "N": 128}))


def test_the_class_is_in_neither_zoo_table():
    assert MasterLatentCodec not in rgbd_amd.modelZoo.values() and MasterLatentCodec not in rgbd_amd.modelZooExtra.values()
    assert rgbd_amd.zoo_lookup("ELIC_master") is rgbd_amd.ELIC and rgbd_amd.zoo_lookup("ELIC_master_latent") is rgbd_amd.ELIC
    assert MasterLatentCodec._MODEL == "ELIC_master_latent" and len(MasterLatentCodec._MODALITIES) == 1


# ---- the acceptance functions on the fixtures ------------------------------------------------------------------------------------------
_RUNS = {}


def _restated(name, mut):
    """y, y_hat and the decisions of the restatement under the fixture's symbols, and f_hat, in float64."""
    if (name, mut) not in _RUNS:
        fx = mc.load_fixture(name)
        f, *ups = mc.inputs(name)
        rs = mc.Restated(mc.weights(name), mut)
        with torch.no_grad():
            y = rs.g_a(f)
            yhat, x, s, _ = rs.latent(y, fx["z_symbols"], fx["symbols"].astype(np.int32))
            base = _RUNS.get((name, None))
            # (g_s only where its input or the mutation differs from the unmutated run's)
            fhat = rs.g_s(yhat, *ups) if base is None or mut == "up23_exchanged" else None
        tab = mc.scale_table()
        idx = (len(tab) - 1 - (np.maximum(s, tab[0])[:, None] <= tab[None, :-1]).sum(axis=1)).astype(np.int32)  # (build_indexes: the bound is table[0])
        _RUNS[(name, mut)] = dict(fx=fx, y=y.numpy(), yhat=yhat.numpy(), x=x, s=s, sym=np.rint(x).astype(np.int32), idx=idx, fhat=fhat)
    return _RUNS[(name, mut)]


@pytest.mark.parametrize("name", ["a", "d"])
def test_the_float64_restatement_is_accepted(name):
    r = _restated(name, None)
    fx = r["fx"]
    assert mc.y_err(r["y"], fx) <= mc.y_bound(fx) and mc.yhat_err(r["yhat"], fx) <= mc.yhat_bound(fx)
    assert mc.fhat_err(name, r["fhat"], fx) <= mc.fhat_bound(fx)
    assert mc.census(fx, r["sym"], r["idx"], r["x"], r["s"]) == []
    assert np.array_equal(r["sym"], fx["symbols"]) and np.array_equal(r["idx"], fx["indexes"])
    # the cap that keeps the census from excusing everything (asserted by the generator, held here)
    (bx, bs), (d_round, d_scale) = mc.decision_bounds(fx), mc.boundary_distances(fx)
    assert np.mean(d_round < bx) <= 0.01 and np.mean(d_scale < bs) <= 0.01


@pytest.mark.parametrize("mut", mc.MUTATIONS)
def test_wrong_restatements_land_outside_the_bound(mut):
    base, r = _restated("a", None), _restated("a", mut)
    fx = r["fx"]
    if mut == "up23_exchanged":  # the latent path is untouched; f_hat is not ELIC_master's
        assert np.array_equal(r["yhat"], base["yhat"])
        e = mc.fhat_err("a", r["fhat"], fx)
        print(f"{mut}: f_hat {e:.2e} against the bound {mc.fhat_bound(fx):.2e}")
        assert e > mc.fhat_bound(fx)
        return
    e = mc.yhat_err(r["yhat"], fx)
    print(f"{mut}: y_hat under the reference's symbols {e:.2e} against the bound {mc.yhat_bound(fx):.2e}; census: {mc.census(fx, r['sym'], r['idx'], r['x'], r['s'])}")
    assert e > mc.yhat_bound(fx)
    assert mc.census(fx, r["sym"], r["idx"], r["x"], r["s"]) != []
