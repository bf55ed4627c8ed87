"""rgbd_pooled_conv3x3 (csrc/pooled_head.hip), the pooled 3x3 head of Channel_aligner, alone on the GPU (cases, statement and
bound: tests/chalign_cases.py; test_chalign_cases.py shows on the CPU that the statement is torch's conv + mean and that every
classic mistake is rejected).

Against its fp64 statement within 8x the error of that statement in fp32 (floored at 2^-23), for every case and both channel
strides; the same bits from two calls; image b of a batch as the image alone; NaN in the padding channels never reaches the
output; nothing written behind `out` or behind the declared scratch; refusals that write nothing.  The figures are printed and
recorded in DESIGN.md 5.5.  Observed on MI355X: 0.09 ... 0.39 x the bound's e_ref (e_gpu <= 1.04e-7)."""
import ctypes

import pytest
import torch

import chalign_cases as cc
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

EINVAL = -22
SENTINEL = 12345.0


def _lib():
    require_gpu()
    from rgbd_amd import _lib as lib

    return lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the pooled head alone ----------------------------------------------------------------------------------------------------
def _head_gpu(L, x, w, b, pad=0):
    B, H, W, C = x.shape
    O = w.shape[0]
    xd = torch.full((B, H, W, C + pad), float("nan"), device="cuda")  # a read of the pad poisons the result
    xd[..., :C] = x.cuda()
    wd, bd = w.cuda().contiguous(), b.cuda()  # (held until the call has run)
    n = L.rgbd_pooled_conv3x3_ws_floats(B, H, W, C)
    assert n > 0
    ws = torch.full((n + 64,), SENTINEL, device="cuda")
    out = torch.full((B * O + 64,), SENTINEL, device="cuda")
    assert L.rgbd_pooled_conv3x3(_p(xd), C + pad, B, H, W, C, _p(wd), _p(bd), O, _p(out), _p(ws), _stream()) == 0
    torch.cuda.synchronize()
    assert (ws[n:] == SENTINEL).all() and (out[B * O:] == SENTINEL).all()
    return out[:B * O].reshape(B, O).cpu()


@pytest.mark.parametrize("pad", cc.PADS)
@pytest.mark.parametrize("name", list(cc.KERNEL_CASES))
def test_pooled_head_kernel(name, pad):
    L = _lib()
    B = cc.KERNEL_CASES[name][0]
    x, w, b = cc.kernel_inputs(name)
    ref, e_ref = cc.pooled_head(x, w, b), cc.kernel_e_ref(name)
    out = _head_gpu(L, x, w, b, pad)
    assert torch.isfinite(out).all()
    e = cc.rel_err(out, ref)
    print(f"pooled head {name} cs = Cin + {pad}: e_gpu {e:.3e}, e_ref {e_ref:.3e} (floor {cc.FLOOR:.3e}), "
          f"ratio {e / max(e_ref, cc.FLOOR):.3f}")
    assert cc.accept(e, e_ref), (e, e_ref)
    assert _bits(_head_gpu(L, x, w, b, pad), out)
    for i in range(B):
        assert _bits(_head_gpu(L, x[i:i + 1], w, b, pad), out[i:i + 1])
    assert _bits(_head_gpu(L, x, w, b, 16 - pad), out)  # the stride changes no bit either


def test_pooled_head_rejects_bad_arguments():
    L = _lib()
    B, H, W, C, O = 2, 5, 6, 16, 8
    x = torch.randn(B, H, W, C + 16, device="cuda")
    w, b = torch.randn(O, C, 3, 3, device="cuda"), torch.randn(O, device="cuda")
    n = L.rgbd_pooled_conv3x3_ws_floats(B, H, W, C)
    assert n > 0
    ws = torch.full((n + 4,), SENTINEL, device="cuda")
    out = torch.full((B * O,), SENTINEL, device="cuda")
    X, WT, BS, OUT, WS = "x", "w", "b", "out", "ws"

    def call(B_=B, H_=H, W_=W, C_=C, O_=O, cs=C + 16, ptr=None):
        p = {X: x.data_ptr(), WT: w.data_ptr(), BS: b.data_ptr(), OUT: out.data_ptr(), WS: ws.data_ptr()}
        p.update(ptr or {})
        return L.rgbd_pooled_conv3x3(p[X], cs, B_, H_, W_, C_, p[WT], p[BS], O_, p[OUT], p[WS], _stream())

    bad = [dict(B_=0), dict(B_=-1), dict(H_=0), dict(W_=0), dict(C_=0), dict(O_=0), dict(cs=C - 4), dict(cs=C + 2), dict(C_=2, cs=4),
           dict(C_=6, cs=8), dict(C_=1028, cs=1028), dict(O_=65536), dict(B_=65536), dict(H_=65536, W_=65536),
           dict(ptr={X: x.data_ptr() + 4}), dict(ptr={WS: ws.data_ptr() + 4}), dict(ptr={X: None}), dict(ptr={WT: None}),
           dict(ptr={BS: None}), dict(ptr={OUT: None}), dict(ptr={WS: None})]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    for args in ((0, H, W, C), (B, 0, W, C), (B, H, 0, C), (B, H, W, 0), (B, H, W, 6), (B, H, W, 1028), (65536, H, W, C),
                 (B, 65536, 65536, C)):
        assert L.rgbd_pooled_conv3x3_ws_floats(*args) == EINVAL, args
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (ws == SENTINEL).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (out == SENTINEL).any() and (ws[n:] == SENTINEL).all()
