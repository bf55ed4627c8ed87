"""ELIC_united_R2D (reference models/elic_united_R2D.py) on the GPU vs the CPU oracle and the reference
golden.  Same layered contract as tests/test_gpu_model.py."""
import os

import numpy as np
import pytest
import torch

from gpu_utils import require_gpu
from oracle import coder
from oracle import elic_oracle as eo
from test_gpu_model import _rel, _walk_parts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sd_r2d():
    from rgbd_amd import synth

    return synth.synthetic_state_dict(0, model="ELIC_united_R2D")


@pytest.fixture(scope="module")
def net_r2d(sd_r2d):
    require_gpu()
    import rgbd_amd

    assert list(rgbd_amd.modelZoo)[:2] == ["ELIC_united_R2D", "ELIC_united"]  # substring matching order of the harness
    m = rgbd_amd.modelZoo["ELIC_united_R2D"](config=rgbd_amd.model_config(), channel=4).eval()
    m.load_state_dict(sd_r2d, strict=True)
    assert m.update(force=True)
    assert m.count_parameters() == 127005454
    return m.to("cuda")


def test_r2d_128x192(net_r2d, sd_r2d):
    from rgbd_amd import synth

    orc = eo.oracle_r2d(sd_r2d)
    orc.update()
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "r2d_128x192.npz"))
    r, d = synth.synthetic_batch(1, 128, 192, config_id=4)
    r, d = torch.from_numpy(r), torch.from_numpy(d)
    out = net_r2d.compress(r.cuda(), d.cuda())
    assert tuple(out["shape"]) == (2, 3)
    orc.trace = {}
    ref = orc.compress(r, d)
    tr, orc.trace = orc.trace, None
    for name in ("y_r", "y_d", "z_r", "z_d"):
        got = net_r2d.debug_tensor(name)
        assert _rel(got, tr[name].numpy()) < 1e-5, name
    assert _rel(net_r2d.debug_tensor("y_r"), g["y_r"]) < 1e-5 and _rel(net_r2d.debug_tensor("y_d"), g["y_d"]) < 1e-5
    for mod, key, zname in (("rgb", "r_strings", "z_r"), ("depth", "d_strings", "z_d")):
        strings, _ = orc._z_compress(mod, torch.from_numpy(net_r2d.debug_tensor(zname)))
        assert strings == out[key][1]
    zh = [torch.from_numpy(net_r2d.debug_tensor(n)) for n in ("zhat_r", "zhat_d")]
    ohr, ohd = eo.h_s_r2d(orc.sd, zh[0], zh[1])
    assert _rel(net_r2d.debug_tensor("hyper_r"), ohr.numpy()) < 2e-5 and _rel(net_r2d.debug_tensor("hyper_d"), ohd.numpy()) < 2e-5
    gsym, gidx = {}, {}
    for mod, key in ((0, "r_strings"), (1, "d_strings")):
        gsym[mod], gidx[mod] = net_r2d.debug_symbols(mod)
        assert coder.rans_encode(gsym[mod], gidx[mod], orc.gc) == out[key][0][0]
    # Bi-CEE (R2D wiring) against the oracle on the GPU's own latents and hyper parameters
    gy = [torch.from_numpy(net_r2d.debug_tensor(n)) for n in ("y_r", "y_d")]
    gh = [torch.from_numpy(net_r2d.debug_tensor(n)) for n in ("hyper_r", "hyper_d")]
    orc.trace = {}
    osr, osd = orc.compress_united(gy[0], gh[0], gy[1], gh[1])
    tr2, orc.trace = orc.trace, None
    clean = _walk_parts(tr2, gsym, gidx, orc, {0: gy[0], 1: gy[1]})
    print(f"ELIC_united_R2D: parts identical before the first boundary flip: {clean} of {len(tr2['parts'])};",
          "streams identical to the oracle end to end:", out["r_strings"] == ref["r_strings"] and out["d_strings"] == ref["d_strings"],
          "| to the reference golden:", out["r_strings"][0][0] == g["r_y"].tobytes() and out["d_strings"][0][0] == g["d_y"].tobytes())
    assert clean >= 1
    yhat_enc = [net_r2d.debug_tensor("yhat_r").copy(), net_r2d.debug_tensor("yhat_d").copy()]
    rec = net_r2d.decompress(out["r_strings"], out["d_strings"], out["shape"])
    assert np.array_equal(net_r2d.debug_tensor("yhat_r"), yhat_enc[0]) and np.array_equal(net_r2d.debug_tensor("yhat_d"), yhat_enc[1])
    xr, xd = rec["x_hat"]["r"].cpu(), rec["x_hat"]["d"].cpu()
    oxr, oxd = eo.g_s_r2d(orc.sd, torch.from_numpy(yhat_enc[0]), torch.from_numpy(yhat_enc[1]))
    oxr, oxd = oxr.clamp(0, 1), oxd.clamp(0, 1)
    assert (xr - oxr).abs().max() < 1e-4 and (xd - oxd).abs().max() < 1e-4
    assert abs(eo.psnr(xr, r) - eo.psnr(oxr, r)) < 1e-4 and abs(eo.psnr(xd, d) - eo.psnr(oxd, d)) < 1e-4
    # the RGB stream does not depend on the depth image at all (that is the point of the variant)
    d2 = torch.from_numpy(synth.synthetic_batch(1, 128, 192, config_id=44)[1])
    out2 = net_r2d.compress(r.cuda(), d2.cuda())
    assert out2["r_strings"] == out["r_strings"] and out2["d_strings"] != out["d_strings"]


def test_r2d_forward_and_stage_entry_points(net_r2d, sd_r2d):
    """models/elic_united_R2D.py inherits forward() / compress_united() / decompress_united() from ELIC_united; here they
    run on the R2D engine variant and are checked against the reference's golden outputs."""
    from rgbd_amd import synth

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "r2d_128x192.npz"))
    r, d = synth.synthetic_batch(1, 128, 192, config_id=4)
    r, d = torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda()
    fw = net_r2d(r, d)
    out = net_r2d.compress(r, d)
    rec = net_r2d.decompress(out["r_strings"], out["d_strings"], out["shape"])
    # eval forward == decompress(compress()) bit for bit (before the clamp), and both match the reference
    assert torch.equal(fw["x_hat"]["r"].clamp(0, 1), rec["x_hat"]["r"]) and torch.equal(fw["x_hat"]["d"].clamp(0, 1), rec["x_hat"]["d"])
    assert (fw["x_hat"]["r"].cpu()[:, :, ::4, ::4] - torch.from_numpy(g["fw_xhat_r_sub"])).abs().max() < 1e-4
    assert (fw["x_hat"]["d"].cpu()[:, :, ::4, ::4] - torch.from_numpy(g["fw_xhat_d_sub"])).abs().max() < 1e-4
    for mod in ("r", "d"):
        np.testing.assert_allclose(fw[f"{mod}_likelihoods"]["z"].cpu().numpy(), g[f"lik_z_{mod}"], rtol=2e-4, atol=1e-7)
        np.testing.assert_allclose(fw[f"{mod}_likelihoods"]["y"].cpu().numpy(), g[f"lik_y_{mod}"], rtol=2e-3, atol=1e-6)
    # the Bi-CEE stage alone on given latents: streams identical to the reference's, y_hat within the float tolerance
    lat = [torch.from_numpy(a).cuda() for a in synth.synthetic_latents(1, 8, 12, 320, int(g["cu_seed"]))]
    sr, sdp = net_r2d.compress_united(lat[0], lat[1], lat[2], lat[3])
    assert sr[0] == g["cu_r_y"].tobytes() and sdp[0] == g["cu_d_y"].tobytes()
    yh_r, yh_d = net_r2d.decompress_united(sr[0], lat[1], sdp[0], lat[3])
    assert _rel(yh_r.cpu().numpy(), g["cu_yhat_r"]) < 2e-5 and _rel(yh_d.cpu().numpy(), g["cu_yhat_d"]) < 2e-5
    # the RGB stream of the stage does not depend on the depth latents
    lat2 = [torch.from_numpy(a).cuda() for a in synth.synthetic_latents(1, 8, 12, 320, 77)]
    sr2, _ = net_r2d.compress_united(lat[0], lat[1], lat2[2], lat2[3])
    assert sr2[0] == sr[0]


def test_r2d_eager_capture_replay_agree(net_r2d):
    """compress() -> decompress() -> forward() of one shape four times on a torch side stream: eager, captured, replayed, and
    replayed on another input.  What a replayed graph hands back -- streams, x_hat, the forward outputs -- is what the eager
    call gave, bit for bit.  B = 2 at 128 x 128, the smallest size the codec takes: the ESA block of the third fusion stage
    pools 7 x 7 windows of the stride-2 map of its H/8 x W/8 grid (8 -> 3 at 64 pixels), so a 64-pixel side is refused with
    RGBD_EINVAL."""
    from rgbd_amd import synth

    def one_round(r, d):
        out = net_r2d.compress(r, d)
        rec = net_r2d.decompress(out["r_strings"], out["d_strings"], out["shape"])
        fw = net_r2d(r, d)
        tensors = [rec["x_hat"]["r"], rec["x_hat"]["d"], fw["x_hat"]["r"], fw["x_hat"]["d"]]
        tensors += [fw[f"{mod}_likelihoods"][k] for mod in ("r", "d") for k in ("y", "z")]
        return (out["r_strings"], out["d_strings"]), [t.clone() for t in tensors]

    def same(p, q):
        return p[0] == q[0] and all(torch.equal(s, t) for s, t in zip(p[1], q[1]))

    g0 = net_r2d.graph_count()
    with torch.cuda.stream(torch.cuda.Stream()):  # (the NULL stream cannot be captured)
        a = [torch.from_numpy(t).cuda() for t in synth.synthetic_batch(2, 128, 128, config_id=51)]
        b = [torch.from_numpy(t).cuda() for t in synth.synthetic_batch(2, 128, 128, config_id=52)]
        eager_a = one_round(*a)
        cap_a = one_round(*a)
        rep_a = one_round(*a)
        assert net_r2d.graph_count() >= g0 + 3  # compress, decompress and forward of this shape are cached graphs now
        rep_b = one_round(*b)
    torch.cuda.synchronize()
    assert same(cap_a, eager_a) and same(rep_a, eager_a)
    assert rep_b[0] != eager_a[0]  # a replayed graph reads the NEW inputs ...
    assert same(rep_b, one_round(*b))  # ... and gives what the eager call (the NULL stream never captures) gives for them
