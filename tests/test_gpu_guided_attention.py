"""The guided window attention kernel (csrc/swin.hip: window_attention_kernel<32>) alone, through its C entry
rgbd_guided_window_attention, against the float64 statement of tests/guided_attention_cases.py (which
tests/test_guided_attention_cases.py pins to the reference's way of computing it).

Bound: max |gpu - f64| <= WA_TOL * max(1, max|S| / 30) * max|v|, WA_TOL = 2e-5 (tests/test_gpu_swin.py's), inputs with
15 < max|S| < 80.  Observed on MI355X: worst 1.11e-6 over the 31 cases (max |S| 19.5 ... 30.9), 5.5 % of the bound; every
mistake of the sensitivity check lands 1.7e4 ... 1.1e5 x the bound away."""
import pytest
import torch

import guided_attention_cases as gc
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

EINVAL = -22
SENTINEL = 12345.0


def _lib():
    require_gpu()
    from rgbd_amd import _lib as lib

    return lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gpu(L, q, kv, rpb, heads, shift, ocs):
    B, H, W, qcs = q.shape
    kvcs = kv.shape[-1]
    qd, kd, rd = q.cuda(), kv.cuda(), rpb.cuda()
    out = torch.full((B, H, W, ocs), SENTINEL, device="cuda")
    rc = L.rgbd_guided_window_attention(qd.data_ptr(), qcs, kd.data_ptr(), kvcs, B, H, W, gc.HEAD_DIM * heads, heads, shift,
                                        rd.data_ptr(), out.data_ptr(), ocs, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu()


def _check(L, B, H, W, heads, shift, pad):
    q, kv, rpb, qcs, kvcs, ocs = gc.inputs(B, H, W, heads, pad, gc.case_seed(B, H, W, heads, shift))
    C = gc.HEAD_DIM * heads
    smax = gc.scores_max(q, kv, rpb, heads)
    assert 15 < smax < 80, smax
    out = _gpu(L, q, kv, rpb, heads, shift, ocs)
    ref = gc.gwa(q, kv, rpb, heads, shift)
    vmax = float(kv[..., C:2 * C].abs().max())
    ok, err = gc.accept(out[..., :C], ref, vmax, smax)
    print(f"guided attention {B}x{H}x{W} heads {heads} shift {shift}: max|S| {smax:.1f}, err / max|v| {err:.2e} "
          f"(bound {gc.tolerance(1.0, smax):.2e})")
    assert ok, (err, gc.tolerance(1.0, smax))
    if ocs > C:
        assert (out[..., C:] == SENTINEL).all()


@pytest.mark.parametrize("B", gc.BATCHES)
@pytest.mark.parametrize("H,W,heads,shift", gc.CASES)
def test_guided_attention_vs_f64(H, W, heads, shift, B):
    """At B == 2 q, kv and out have padded channel strides: NaN in the pads of the inputs (a read of them poisons the
    result), a sentinel in out's that must survive."""
    _check(_lib(), B, H, W, heads, shift, pad=(B == 2))


def test_guided_attention_more_pairs_than_one_sweep():
    """1920 (window, head) pairs: every wavefront walks all of its pairs, 120 workgroups."""
    B, H, W, heads, shift = gc.SWEEP_CASE
    assert B * (H // 4) * (W // 4) * heads > 4 * 4 * 16
    _check(_lib(), B, H, W, heads, shift, pad=False)


@pytest.mark.parametrize("B,H,W,heads,shift", gc.SENSITIVITY_CASES)
def test_guided_attention_tolerance_is_sensitive(B, H, W, heads, shift):
    """Each mistake, applied to the float64 statement, lands at least 100x the bound away from the GPU's result."""
    L = _lib()
    q, kv, rpb, qcs, kvcs, ocs = gc.inputs(B, H, W, heads, False, gc.case_seed(B, H, W, heads, shift))
    C = gc.HEAD_DIM * heads
    out = _gpu(L, q, kv, rpb, heads, shift, ocs).double()
    tol = gc.tolerance(float(kv[..., C:2 * C].abs().max()), gc.scores_max(q, kv, rpb, heads))
    assert float((out - gc.gwa(q, kv, rpb, heads, shift)).abs().max()) <= tol
    margins = {m: float((out - gc.gwa(q, kv, rpb, heads, shift, m)).abs().max()) / tol for m in gc.MUTATIONS}
    print(f"sensitivity {B}x{H}x{W} heads {heads} shift {shift}:", {m: round(v) for m, v in margins.items()})
    assert min(margins.values()) >= 100, margins


def test_guided_attention_rejects_bad_arguments():
    """Every refusal of the boundary returns RGBD_EINVAL and writes nothing; a good call then succeeds."""
    L = _lib()
    heads, C, H, W = 3, 96, 8, 12
    q = torch.randn(1, H, W, C + 16, device="cuda")
    kv = torch.randn(1, H, W, 2 * C + 16, device="cuda")
    rpb = torch.randn(49, heads, device="cuda")
    out = torch.full((1, H, W, C + 16), SENTINEL, device="cuda")
    Q, KV, R, O = "q", "kv", "r", "o"

    def call(B=1, H_=H, W_=W, C_=C, heads_=heads, shift=2, qcs=C + 16, kvcs=2 * C + 16, ocs=C + 16, ptr=None):
        p = {Q: q.data_ptr(), KV: kv.data_ptr(), R: rpb.data_ptr(), O: out.data_ptr()}
        p.update(ptr or {})
        return L.rgbd_guided_window_attention(p[Q], qcs, p[KV], kvcs, B, H_, W_, C_, heads_, shift, p[R], p[O], ocs, _stream())

    bad = [dict(H_=6), dict(W_=10), dict(C_=48), dict(heads_=2), dict(heads_=6), dict(shift=-1), dict(shift=4), dict(qcs=C - 4),
           dict(kvcs=2 * C - 4), dict(ocs=C - 1), dict(qcs=C + 2), dict(kvcs=2 * C + 2), dict(ptr={Q: q.data_ptr() + 4}),
           dict(ptr={KV: kv.data_ptr() + 4}), dict(ptr={Q: None}), dict(ptr={KV: None}), dict(ptr={R: None}), dict(ptr={O: None}),
           dict(B=0), dict(B=-1),
           # pair counts above 0x7fffffff (refused before anything is touched): 2^31 windows of one head; 2^29 windows of 4
           dict(H_=4 * 65536, W_=4 * 32768, C_=32, heads_=1), dict(B=512, H_=4 * 1024, W_=4 * 1024, C_=128, heads_=4,
                                                                  qcs=128, kvcs=256, ocs=128)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (out[..., :C] == SENTINEL).any() and (out[..., C:] == SENTINEL).all()
