"""The single-modal STF (rgbd_amd.stf, reference models/stf.py) without a GPU: parameter inventory against the reference's
state_dict (tests/golden/stf1_keys.json), synthetic weights, zoo order and tester name resolution, host-side errors, and the
CPU restatement (tests/stf_single_ref.py) against what the unmodified reference produced (tests/golden/stf1_*.npz, written
by tests/golden/make_stf_single.py).

The integer stage of every fixture is machine independent and always checked: the restatement's tables and coder turn the
reference's symbols / indexes into the reference's y stream, and its decoder gets them back.  The float stage reproduces the
fixture bit for bit where torch's CPU kernels are the build that generated it (the sha of the latents tells); on another
CPU it is held to 1e-5 relative against the stored sub-sample instead."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import stf_single_ref as ref
from oracle import coder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["a_128x192", "b_256x256", "c_b2_192x128"]


def _sha_f32(t):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(t, np.float32)).tobytes()).hexdigest()[:16]


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(GOLDEN, "stf1_keys.json")) as f:
        return json.load(f)


_REFS = {}


def _ref_for(seed):
    if seed not in _REFS:
        from rgbd_amd import synth

        r = ref.StfSingleRef(synth.synthetic_state_dict(seed, model="STF"))
        assert r.update()
        _REFS[seed] = r
    return _REFS[seed]


def test_entries_match_the_reference_state_dict(keys):
    from rgbd_amd import arch

    e = arch.stf_entries()
    assert keys["n_tensors"] == 779 and len(e) == 779
    assert set(e) == set(keys["keys"])
    for name, shape in keys["keys"].items():
        if e[name].kind == "buffer" and e[name].shape == (0,):
            continue  # tables built by update(): empty at construction here, sized by the reference's update()
        assert tuple(e[name].shape) == tuple(shape), (name, e[name].shape, shape)
    assert arch.count_parameters(e) == 99855639 == keys["n_parameters"]
    e1 = arch.stf_entries(channel=1)
    assert e1["patch_embed.proj.weight"].shape == (48, 1, 2, 2) and e1["end_conv.2.weight"].shape == (1, 48, 3, 3)


def test_synthetic_weights_load_strict_and_are_deterministic():
    import rgbd_amd
    from rgbd_amd import synth

    sd = synth.synthetic_state_dict(3, model="STF")
    sd2 = synth.synthetic_state_dict(3, model="STF")
    other = synth.synthetic_state_dict(4, model="STF")
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert not torch.equal(sd["h_a.0.weight"], other["h_a.0.weight"])
    plain = synth.synthetic_state_dict(3, model="STF", recipe="plain")
    assert torch.equal(plain["h_a.0.weight"], sd["h_a.0.weight"])
    assert torch.equal(plain["h_a.8.weight"] * np.float32(synth.STF1_GAINS["z"]), sd["h_a.8.weight"])
    m = rgbd_amd.SymmetricalTransFormer(pretrain_img_size=256, embed_dim=48, num_slices=12).eval()
    m.load_state_dict(sd, strict=True)
    assert m.update(force=True)
    assert m.count_parameters() == 99855639
    assert rgbd_amd.STF is rgbd_amd.SymmetricalTransFormer
    back = m.state_dict()
    assert set(back) == set(sd) and torch.equal(back["lrp_transforms.11.8.weight"], sd["lrp_transforms.11.8.weight"])
    m2 = rgbd_amd.SymmetricalTransFormer.from_state_dict(sd)
    assert torch.equal(m2.state_dict()["h_mean_s.6.0.weight"], sd["h_mean_s.6.0.weight"])
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if not k.startswith("lrp_transforms.3.")}, strict=True)


def test_zoo_order_and_tester_name_resolution(tmp_path):
    import rgbd_amd
    from rgbd_amd.tester import TesterSingle

    names = list(rgbd_amd.modelZoo)
    assert names[:2] == ["ELIC_united_R2D", "ELIC_united"]
    assert names.index("STF") > names.index("STF_united")
    assert rgbd_amd.modelZoo["STF"] is rgbd_amd.SymmetricalTransFormer

    def resolve(model_name):  # TesterSingle.get_net's match: the first zoo name that is a substring of the model name
        for name, model in rgbd_amd.modelZoo.items():
            if model_name.find(name) != -1:
                return model
        return None

    assert resolve("STF") is rgbd_amd.SymmetricalTransFormer
    assert resolve("STF_united") is rgbd_amd.SymmetricalTransFormerUnited
    assert resolve("ELIC") is rgbd_amd.ELIC
    # and through the tester itself (no GPU: the model is built and its checkpoint loaded, nothing is uploaded)
    t = TesterSingle.__new__(TesterSingle)
    t.channel = 3
    t.device = "cuda"
    t.ckpt_dir_path = str(tmp_path)
    from rgbd_amd import synth

    ck = tmp_path / "ck.pth.tar"
    torch.save({"epoch": 7, "state_dict": synth.synthetic_state_dict(0, model="STF")}, ck)
    try:
        t.get_net(rgbd_amd.model_config(), "STF", str(ck))
    except rgbd_amd.RgbdError:
        pass  # (.to("cuda") without a GPU)
    assert isinstance(t.net, rgbd_amd.SymmetricalTransFormer)


@pytest.mark.parametrize("name", CASES)
def test_integer_stage_from_the_reference_symbols(name):
    """Machine independent: tables + coder of the restatement on the reference's own symbols / indexes."""
    g = np.load(os.path.join(GOLDEN, f"stf1_{name}.npz"))
    r = _ref_for(int(g["seed"]))
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    sym, idx = g["symbols"].astype(np.int32), g["indexes"].astype(np.int32)
    assert sym.shape[0] == B * 384 * (H // 16) * (W // 16) == idx.shape[0]
    assert coder.rans_encode(sym, idx, r.gc) == g["y_stream"].tobytes()
    assert np.array_equal(coder.rans_decode(g["y_stream"].tobytes(), idx, r.gc), sym)
    per = sym.shape[0] // 12
    for i in range(12):  # the fixture conditions the generator asserted
        s, k = sym[i * per:(i + 1) * per], idx[i * per:(i + 1) * per]
        assert np.mean(s != 0) >= 0.5 and np.unique(k).size >= 8, (name, i)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    from rgbd_amd import synth

    g = np.load(os.path.join(GOLDEN, f"stf1_{name}.npz"))
    r = _ref_for(int(g["seed"]))
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    x = torch.from_numpy(synth.synthetic_batch(B, H, W, config_id=int(g["config_id"]))[0])
    r.trace = {}
    out = r.compress(x)
    tr, r.trace = r.trace, None
    assert tuple(out["shape"]) == tuple(g["shape"]) == (H // 64, W // 64)
    assert _rel(tr["y"].numpy()[:, ::24, ::2, ::2], g["y_sub"]) < 1e-5
    assert len(tr["slices"]) == 12 and all(float(s["lrp"].abs().max()) >= 0.1 for s in tr["slices"])
    same_build = _sha_f32(tr["y"]) == str(g["y_sha"])
    print(f"{name}: latents bit-identical to the fixture: {same_build}")
    if same_build:  # the generating build: everything bit for bit
        for i in range(B):
            assert out["strings"][1][i] == g[f"z{i}"].tobytes(), (name, i)
        assert np.array_equal(tr["symbols"], g["symbols"].astype(np.int32))
        assert np.array_equal(tr["indexes"], g["indexes"].astype(np.int32))
        assert out["strings"][0][0] == g["y_stream"].tobytes()
    else:  # another CPU: sizes stay close; the integer stage is covered by test_integer_stage_from_the_reference_symbols
        assert abs(len(out["strings"][0][0]) - g["y_stream"].shape[0]) <= 0.02 * g["y_stream"].shape[0]
    fw = r.forward(x)
    bits = float(-torch.log2(fw["likelihoods"]["y"].double()).sum()), float(-torch.log2(fw["likelihoods"]["z"].double()).sum())
    assert abs(bits[0] - float(g["lik_y_bits"])) <= 1e-4 * float(g["lik_y_bits"])
    assert abs(bits[1] - float(g["lik_z_bits"])) <= 1e-4 * float(g["lik_z_bits"])
    if B == 1:
        dec = r.decompress(out["strings"], out["shape"])
        assert torch.equal(dec["x_hat"], fw["x_hat"].clamp(0, 1))  # the reference's own identity (measured difference 0.0)
        psnr = -10 * np.log10(torch.mean((dec["x_hat"] - x) ** 2).item())
        assert abs(psnr - float(g["psnr"])) < (1e-9 if same_build else 1e-3)
        if same_build:
            assert _sha_f32(dec["x_hat"]) == str(g["xhat_sha"])
            assert _sha_f32(fw["x_hat"]) == str(g["fw_xhat_sha"])
