"""ELIC(return_mid=True) on the GPU (models/elic.py:159-170, 318-329): up1..up3, the outputs of the first three transposed
convolutions of g_s, against the reference's (tests/golden/elic_mid_c1_256x256.npz, tests/golden/make_aligner.py) within
1e-4 * max(1, max|ref|) -- the measure test_gpu_elic_single.py applies to x_hat -- and the flag changing nothing else."""
import os

import numpy as np
import pytest
import torch

from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UPS = ("up1", "up2", "up3")


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def pair():
    """(return_mid=False, return_mid=True) on the same weights (seed 0)."""
    require_gpu()
    import rgbd_amd
    from rgbd_amd import synth

    sd = synth.synthetic_state_dict(0, model="ELIC")
    nets = []
    for mid in (False, True):
        m = rgbd_amd.ELIC(config=rgbd_amd.model_config(), channel=3, return_mid=mid).eval()
        m.load_state_dict(sd, strict=True)
        assert m.update(force=True)
        nets.append(m.to("cuda"))
    return nets


@pytest.fixture(scope="module")
def ref_streams():
    g = np.load(os.path.join(GOLDEN, "elic_c1_256x256.npz"))
    return [[g["y_stream"].tobytes()], [g["z0"].tobytes()]], tuple(int(v) for v in g["shape"])


def test_decompress_returns_the_references_mids(pair, ref_streams):
    plain, mid = pair
    strings, shape = ref_streams
    fx = np.load(os.path.join(GOLDEN, "elic_mid_c1_256x256.npz"))
    rec = mid.decompress(strings, shape)
    assert set(rec) == {"x_hat", "cost_time", "up1", "up2", "up3"}
    for k in UPS:
        up = rec[k].cpu()
        assert tuple(up.shape) == tuple(int(v) for v in fx[k + "_shape"])
        ref = torch.from_numpy(fx[k])
        err = float((up[:, ::8, ::4, ::4] - ref).abs().max())
        tol = 1e-4 * max(1.0, float(fx[k + "_max"]))
        print(f"elic mid {k}: max |gpu - ref| {err:.3e} (tolerance {tol:.3e}, max|ref| {float(fx[k + '_max']):.3f})")
        assert err <= tol, (k, err, tol)
    base = plain.decompress(strings, shape)
    assert set(base) == {"x_hat", "cost_time"}
    assert torch.equal(_bits(rec["x_hat"]), _bits(base["x_hat"]))
    # a second decompress into fresh tensors (the call shape's graph is captured / replayed by now): the first result's
    # tensors stay as they are and the new ones hold the same bits
    keep = {k: rec[k].clone() for k in UPS + ("x_hat",)}
    for _ in range(2):
        rec2 = mid.decompress(strings, shape)
        for k in UPS + ("x_hat",):
            assert rec2[k].data_ptr() != rec[k].data_ptr()
            assert torch.equal(_bits(rec[k]), _bits(keep[k])) and torch.equal(_bits(rec2[k]), _bits(keep[k])), k
    # a replay must not write into the tensors of an earlier call: scribble over them, decompress again
    for k in UPS:
        rec[k].fill_(-7.0)
    rec3 = mid.decompress(strings, shape)
    for k in UPS:
        assert (rec[k] == -7.0).all() and torch.equal(_bits(rec3[k]), _bits(keep[k])), k


def test_forward_and_compress_with_the_flag(pair):
    from rgbd_amd import synth

    plain, mid = pair
    r, _ = synth.synthetic_batch(1, 256, 256, config_id=1)
    x = torch.from_numpy(r).cuda()
    out_p, out_m = plain.compress(x), mid.compress(x)
    assert out_p["strings"] == out_m["strings"] and tuple(out_p["shape"]) == tuple(out_m["shape"])
    rec = mid.decompress(out_m["strings"], out_m["shape"])
    fw = mid(x)
    assert set(fw) == {"x_hat", "likelihoods", "up1", "up2", "up3"}
    fw_p = plain(x)
    assert set(fw_p) == {"x_hat", "likelihoods"}
    assert torch.equal(_bits(fw["x_hat"]), _bits(fw_p["x_hat"]))
    for k in ("y_likelihoods", "z_likelihoods"):
        assert torch.equal(_bits(fw["likelihoods"][k]), _bits(fw_p["likelihoods"][k]))
    for k in UPS:
        assert fw[k].shape == rec[k].shape
        assert torch.equal(_bits(fw[k]), _bits(rec[k])), k


def test_batch_of_two(pair):
    """B = 2 at 64x128 with one stream per image: shapes, and image 0 of the batch equals the B = 1 call bit for bit (what
    test_gpu_elic_single.py::test_batch_and_errors asserts for x_hat)."""
    from rgbd_amd import synth

    _, mid = pair
    r, _ = synth.synthetic_batch(2, 64, 128, config_id=3)
    x = torch.from_numpy(r).cuda()
    mid.per_image_streams = True
    try:
        out = mid.compress(x)
        rec = mid.decompress(out["strings"], out["shape"])
        N = mid.N
        assert rec["up1"].shape == (2, N, 8, 16) and rec["up2"].shape == (2, N, 16, 32) and rec["up3"].shape == (2, N, 32, 64)
        one = mid.compress(x[:1])
        assert one["strings"][0][0] == out["strings"][0][0]
        rec1 = mid.decompress(one["strings"], one["shape"])
        assert torch.equal(_bits(rec1["x_hat"][0]), _bits(rec["x_hat"][0]))
        for k in UPS:
            assert torch.equal(_bits(rec1[k][0]), _bits(rec[k][0])), k
    finally:
        mid.per_image_streams = False
