"""The checkerboard Cheng2020 model (rgbd_amd.ckbd, reference models/Cheng2020withCKBD.py) without a GPU: parameter inventory
against the reference's state_dict (tests/golden/ckbd_keys.json), synthetic weights, zoo resolution through
TesterSingle.get_net, strict loading, host-side errors, the host parametrizer map of the GDN layers against torch's bit for
bit, and the CPU restatement (tests/ckbd_ref.py) against what the unmodified reference produced (tests/golden/ckbd_*.npz,
written by tests/golden/make_ckbd.py): symbols, indexes and streams exactly, x_hat within 1e-6."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import ckbd_ref as ref
from oracle import coder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["a_64x128", "b_b2_128x64_d", "c_128x192_n128"]


def _sha_f32(t):
    return hashlib.sha256(np.ascontiguousarray(np.asarray(t, np.float32)).tobytes()).hexdigest()[:16]


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(GOLDEN, "ckbd_keys.json")) as f:
        return json.load(f)


_REFS = {}


def ref_for(g):
    """The restatement on the synthetic weights of a fixture (built once per (seed, N, channel))."""
    key = (int(g["seed"]), int(g["N"]), int(g["channel"]))
    if key not in _REFS:
        from rgbd_amd import synth

        r = ref.CkbdRef(synth.synthetic_state_dict(key[0], model="ckbd", N=key[1], channel=key[2]))
        assert r.update()
        _REFS[key] = r
    return _REFS[key]


def image_for(g):
    from rgbd_amd import synth

    r, d = synth.synthetic_batch(int(g["B"]), int(g["H"]), int(g["W"]), config_id=int(g["config_id"]))
    return torch.from_numpy(r if int(g["channel"]) == 3 else d)


def test_entries_match_the_reference_state_dict(keys):
    from rgbd_amd import arch

    e = arch.ckbd_entries(192, 3)
    assert keys["n_tensors"] == 160 and len(e) == 160
    assert list(e) == list(keys["keys"])
    for name, shape in keys["keys"].items():
        if e[name].kind == "buffer" and e[name].shape == (0,):
            continue  # tables built by update(): empty at construction
        assert tuple(e[name].shape) == tuple(shape), (name, e[name].shape, shape)
    assert arch.count_parameters(e) == 26598956 == keys["n_parameters"]
    for need in ("g_a.0.gdn.beta", "g_a.0.gdn.gamma", "g_s.5.igdn.gamma_reparam.pedestal", "g_s.1.igdn.beta_reparam.lower_bound.bound",
                 "context_prediction.mask"):
        assert need in e
    e1 = arch.ckbd_entries(128, 1)
    assert e1["g_a.0.conv1.weight"].shape == (128, 1, 3, 3) and e1["g_s.7.0.weight"].shape == (4, 128, 3, 3)
    assert e1["entropy_parameters.0.weight"].shape == (128 * 10 // 3, 128 * 4, 1, 1) and e1["g_a.2.gdn.gamma"].shape == (128, 128)


def test_synthetic_weights_load_strict_and_meet_the_recipe():
    import rgbd_amd
    from rgbd_amd import synth

    sd = synth.synthetic_state_dict(3, model="ckbd", N=128, channel=1)
    sd2 = synth.synthetic_state_dict(3, model="ckbd", N=128, channel=1)
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    plain = synth.synthetic_state_dict(3, model="ckbd", N=128, channel=1, recipe="plain")
    assert torch.equal(plain["g_a.2.gdn.beta"], torch.sqrt(torch.ones(128) + 2.0 ** -36))  # the reference's init
    assert torch.equal(plain["h_a.8.weight"] * np.float32(synth.CKBD_GAINS["z"]), sd["h_a.8.weight"])
    # the stress recipe: a beta per channel, a dense gamma with part of the raw values below the bound 2^-18, and masked
    # context taps that are NOT zero in the state_dict
    for p in ("g_a.0.gdn", "g_s.3.igdn"):
        raw = sd[p + ".gamma"]
        off = raw[~torch.eye(128, dtype=torch.bool)]
        assert 0.05 < float((off < 2.0 ** -18).float().mean()) < 0.5 and float(ref.parametrize(off, 0.0).sum()) > 1.0
        assert sd[p + ".beta"].unique().numel() > 100
        assert float(sd[p + ".gamma_reparam.lower_bound.bound"]) == 2.0 ** -18 and float(sd[p + ".beta_reparam.pedestal"]) == 2.0 ** -36
    w, mask = sd["context_prediction.weight"], sd["context_prediction.mask"]
    assert torch.equal(mask, ref.context_mask(w)) and int(mask[0, 0].sum()) == 12
    assert float(w[mask == 0].abs().mean()) > 0.5 * float(w[mask == 1].abs().mean())
    m = rgbd_amd.Cheng2020AnchorwithCheckerboard(N=128, channel=1, config=rgbd_amd.model_config()).eval()
    m.load_state_dict(sd, strict=True)
    assert m.update(force=True)
    from rgbd_amd import arch

    assert m.count_parameters() == arch.count_parameters(arch.ckbd_entries(128, 1))
    back = m.state_dict()
    assert list(back) == list(sd) and torch.equal(back["g_s.5.igdn.gamma"], sd["g_s.5.igdn.gamma"])
    m2 = rgbd_amd.Cheng2020AnchorwithCheckerboard.from_state_dict(sd)
    assert m2.N == 128 and m2.channel == 1
    for missing in ("g_a.4.gdn.gamma", "g_s.1.igdn.beta"):  # strict loading rejects a missing GDN tensor
        with pytest.raises(RuntimeError):
            m.load_state_dict({k: v for k, v in sd.items() if k != missing}, strict=True)
    with pytest.raises(ValueError):
        rgbd_amd.Cheng2020AnchorwithCheckerboard(N=160)


def test_zoo_resolution_through_the_tester(tmp_path):
    import rgbd_amd
    from rgbd_amd import synth
    from rgbd_amd.tester import TesterSingle

    names = list(rgbd_amd.modelZoo)
    assert names[:2] == ["ELIC_united_R2D", "ELIC_united"] and names[-1] == "ckbd"
    assert rgbd_amd.modelZoo["ckbd"] is rgbd_amd.Cheng2020AnchorwithCheckerboard
    assert not any("ckbd" in n or n in "ckbd" for n in names[:-1])
    t = TesterSingle.__new__(TesterSingle)
    t.channel = 3
    t.device = "cuda"
    t.ckpt_dir_path = str(tmp_path)
    ck = tmp_path / "ck.pth.tar"
    torch.save({"epoch": 7, "state_dict": synth.synthetic_state_dict(0, model="ckbd")}, ck)
    try:
        t.get_net(rgbd_amd.model_config(), "ckbd", str(ck))
    except rgbd_amd.RgbdError:
        pass  # (.to("cuda") without a GPU)
    assert isinstance(t.net, rgbd_amd.Cheng2020AnchorwithCheckerboard) and t.net.N == 192 and t.net.channel == 3


@pytest.mark.parametrize("is_beta", [1, 0])
def test_host_parametrizer_equals_torch_bit_for_bit(is_beta):
    """rgbd_gdn_parametrize (what packs beta / gamma for the kernel) against NonNegativeParametrizer.forward in torch fp32."""
    from rgbd_amd import _lib

    L = _lib.lib()
    minimum = 1e-6 if is_beta else 0.0
    bound = torch.tensor([(minimum + (2.0 ** -18) ** 2) ** 0.5], dtype=torch.float32)
    g = torch.Generator().manual_seed(11 + is_beta)
    raw = torch.cat([torch.randn(50000, generator=g), 1e-3 * torch.randn(50000, generator=g), 2e-5 * torch.rand(20000, generator=g),
                     torch.tensor([0.0, -0.0, -1.0, 1.0, 2.0 ** -18, 1e-3, 0.31622776]), bound, bound * 0.5,
                     torch.nextafter(bound, torch.tensor([0.0])), torch.nextafter(bound, torch.tensor([1.0]))]).float()
    assert (raw < bound).any() and (raw == bound).any() and (raw == 0).any() and (raw > bound).any()
    want = ref.parametrize(raw, minimum)
    src = raw.numpy()
    out = np.full(src.shape, np.nan, dtype=np.float32)
    f32p = ctypes.POINTER(ctypes.c_float)
    assert L.rgbd_gdn_parametrize(src.ctypes.data_as(f32p), src.size, is_beta, out.ctypes.data_as(f32p)) == 0
    assert np.array_equal(out.view(np.uint32), want.numpy().view(np.uint32))
    assert L.rgbd_gdn_parametrize(None, 4, is_beta, out.ctypes.data_as(f32p)) == -22
    assert L.rgbd_gdn_parametrize(src.ctypes.data_as(f32p), 4, 2, out.ctypes.data_as(f32p)) == -22


@pytest.mark.parametrize("name", CASES)
def test_integer_stage_from_the_reference_symbols(name):
    """Tables + coder of the restatement on the reference's own symbols / indexes, and the fixture conditions."""
    g = np.load(os.path.join(GOLDEN, f"ckbd_{name}.npz"))
    r = ref_for(g)
    B, N, H, W = int(g["B"]), int(g["N"]), int(g["H"]), int(g["W"])
    sym, idx = g["symbols"].astype(np.int32), g["indexes"].astype(np.int32)
    assert sym.shape[0] == B * N * (H // 16) * (W // 16) == idx.shape[0] == g["x"].shape[0] == g["sigma"].shape[0]
    assert coder.rans_encode(sym, idx, r.gc) == g["y_stream"].tobytes()
    assert np.array_equal(coder.rans_decode(g["y_stream"].tobytes(), idx, r.gc), sym)
    assert np.array_equal(np.rint(g["x"]).astype(np.int32), sym)
    half = sym.shape[0] // 2
    for i in range(2):
        s, k = sym[i * half:(i + 1) * half], idx[i * half:(i + 1) * half]
        assert np.mean(s != 0) >= 0.5 and np.unique(k).size >= 8, (name, i)
    assert np.mean(g["z_symbols"] != 0) >= 0.5


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    g = np.load(os.path.join(GOLDEN, f"ckbd_{name}.npz"))
    r = ref_for(g)
    B, H, W = int(g["B"]), int(g["H"]), int(g["W"])
    x = image_for(g)
    r.trace = {}
    out = r.compress(x)
    tr, r.trace = r.trace, None
    assert tuple(out["shape"]) == tuple(g["shape"]) == (H // 64, W // 64)
    assert _rel(tr["y"].numpy()[:, ::12, ::2, ::2], g["y_sub"]) < 1e-5
    print(f"{name}: latents bit-identical to the fixture: {_sha_f32(tr['y']) == str(g['y_sha'])}")
    for i in range(B):
        assert out["strings"][1][i] == g[f"z{i}"].tobytes(), (name, i)
    assert np.array_equal(tr["z_symbols"].numpy().astype(np.int32), g["z_symbols"].astype(np.int32))
    assert np.array_equal(tr["symbols"], g["symbols"].astype(np.int32))
    assert np.array_equal(tr["indexes"], g["indexes"].astype(np.int32))
    assert out["strings"][0][0] == g["y_stream"].tobytes()
    assert np.abs(tr["x"] - g["x"]).max() <= 1e-5 * max(1.0, float(np.abs(g["x"]).max()))
    assert np.abs(tr["sigma"] - g["sigma"]).max() <= 1e-5 * max(1.0, float(np.abs(g["sigma"]).max()))
    dec = r.decompress(out["strings"], out["shape"])
    if "xhat" in g:
        assert float((dec["x_hat"] - torch.from_numpy(g["xhat"])).abs().max()) <= 1e-6
    psnr = -10 * np.log10(torch.mean((dec["x_hat"] - x) ** 2).item())
    assert abs(psnr - float(g["psnr"])) < 1e-5
    # forced symbols that equal the coded ones change nothing
    r.trace = {}
    again = r.compress(x, forced_y=tr["symbols"], forced_z=tr["z_symbols"].numpy().reshape(-1))
    tr2, r.trace = r.trace, None
    assert again["strings"][0][0] == out["strings"][0][0] and torch.equal(tr2["yhat"], tr["yhat"])
    fw = r.forward(x)
    bits = float(-torch.log2(fw["likelihoods"]["y"].double()).sum()), float(-torch.log2(fw["likelihoods"]["z"].double()).sum())
    assert abs(bits[0] - float(g["lik_y_bits"])) <= 1e-5 * float(g["lik_y_bits"])
    assert abs(bits[1] - float(g["lik_z_bits"])) <= 1e-5 * float(g["lik_z_bits"])
    print(f"{name}: x_hat sha equal: {_sha_f32(dec['x_hat']) == str(g['xhat_sha'])}, forward x_hat sha equal: "
          f"{_sha_f32(fw['x_hat']) == str(g['fw_xhat_sha'])}, max |x_hat| {float(dec['x_hat'].abs().max()):.3f}, PSNR {psnr:.3f} dB")
