"""Last-bit pins of the small float kernels whose rounding is partly the COMPILER's choice (hipcc's default -ffp-contract=fast:
`a * b + c * d` has more than one legal contraction, and __fmul_rn / __fadd_rn are plain operators in this toolchain, so they
do not fence it -- DESIGN.md section 8).  Round 4 found a LayerNorm rewrite that silently took another contraction and moved an
STF_united stream by a few bytes; these hashes make such a change -- by an edit or by a compiler upgrade -- fail HERE, by
name, instead of surfacing as a golden that moved.  The values are not 'right' in themselves: re-record them
(RGBD_RECORD_PINS=1, on the GPU box) together with tests/golden/parity_floors.json when a change is deliberate."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointwise_pins.json")


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def _cases():
    from test_gpu_pointwise import _run

    g = torch.Generator().manual_seed(7)
    out = {}
    x = torch.randn(2, 48, 20, 27, generator=g)
    out["bilinear_48x20x27_to_61x83"] = _sha(_run(1, x, oh=61, ow=83))
    x = torch.randn(2, 192, 16, 24, generator=g)
    w0, w1 = torch.randn(12, 192, generator=g) * 0.05, torch.randn(192, 12, generator=g) * 0.2
    out["se_scale_192"] = _sha(_run(2, x, w0=w0, w1=w1))
    out["se_residual_192"] = _sha(_run(3, x, w0=w0, w1=w1))
    from rgbd_amd._lib import lib

    for C in (48, 192, 768):
        xt = (torch.randn(515, C, generator=g) * 3 + torch.randn(515, 1, generator=g) * 5).cuda()
        w, b = torch.randn(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
        y = torch.empty_like(xt)
        assert lib().rgbd_layernorm(xt.data_ptr(), 515, C, C, w.data_ptr(), b.data_ptr(), y.data_ptr(), C,
                                    torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        out[f"layernorm_{C}"] = _sha(y)
    # the two window-attention ops (csrc/swin.hip), whose op tests are tolerance tests: (B, H, W, heads, shift), padded
    # strides at B == 2.  All nine mask regions with a partly filled last workgroup, the C = 384 stage, an odd shift, and a
    # paired launch (both sets' outputs); guided: the same, and one window row with one head.
    import guided_attention_cases as gc
    from test_gpu_guided_attention import _gpu as _gwa_gpu
    from test_gpu_swin import _wa_gpu, _wa_inputs

    L = lib()
    for n, (B, H, W, heads, shift) in enumerate([(2, 8, 12, 3, 2), (1, 12, 8, 24, 0), (1, 8, 12, 3, 3)]):
        qkv, rpb, _, ocs = _wa_inputs(B, H, W, heads, 2.6, B == 2, seed=9100 + n)
        out[f"window_attention_{B}x{H}x{W}_h{heads}_s{shift}"] = _sha(_wa_gpu(L, qkv, rpb, heads, shift, ocs))
    qa, ra, _, ocs = _wa_inputs(2, 12, 8, 3, 2.6, True, seed=9110)
    qb, rb, _, _ = _wa_inputs(2, 12, 8, 3, 2.6, True, seed=9111)
    pa, pb = _wa_gpu(L, qa, ra, 3, 2, ocs, pair=(qb, rb))
    out["window_attention_pair_2x12x8_h3_s2_set0"], out["window_attention_pair_2x12x8_h3_s2_set1"] = _sha(pa), _sha(pb)
    for n, (B, H, W, heads, shift) in enumerate([(2, 8, 12, 3, 2), (1, 12, 8, 3, 0), (1, 4, 20, 1, 2), (1, 8, 12, 3, 3)]):
        q, kv, rpb, _, _, ocs = gc.inputs(B, H, W, heads, B == 2, 9200 + n)
        out[f"guided_attention_{B}x{H}x{W}_h{heads}_s{shift}"] = _sha(_gwa_gpu(L, q, kv, rpb, heads, shift, ocs))
    # round-4 review, item 3: the kernels behind a decision or a reported number that are not convolutions -- the factorised
    # prior (eb_forward, entropy_models.py:391-428), the Gaussian likelihoods of the checkerboard parts (ckbd_estimate,
    # entropy_models.py:534-558; its quantiser is ckbd_part's), x_hat of the eval forward, and the metric kernel
    import rgbd_amd
    from rgbd_amd import ELIC_united, metrics, synth

    net = ELIC_united(config=rgbd_amd.model_config(), channel=4).eval()
    net.load_state_dict(synth.synthetic_state_dict(0))
    net.update(force=True)
    net = net.to("cuda")
    r, d = synth.synthetic_batch(1, 128, 128, config_id=3)
    rgb, depth = torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda()
    fw = net(rgb, depth)
    for m in ("r", "d"):
        out[f"forward_lik_y_{m}"] = _sha(fw[f"{m}_likelihoods"]["y"])
        out[f"forward_lik_z_{m}"] = _sha(fw[f"{m}_likelihoods"]["z"])
        out[f"forward_xhat_{m}"] = _sha(fw["x_hat"][m])
    out["msssim_kernel_2x3x192x176"] = _sha(metrics.ms_ssim_gpu(torch.rand(2, 3, 192, 176, generator=g).cuda(),
                                                                 torch.rand(2, 3, 192, 176, generator=g).cuda()))
    return out


def test_small_kernels_keep_their_last_bits():
    require_gpu()
    got = _cases()
    if os.environ.get("RGBD_RECORD_PINS"):
        path = os.environ.get("RGBD_RECORD_PINS_TO", PINS)
        with open(path, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
        pytest.skip(f"recorded {path}")
    want = json.load(open(PINS))
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
