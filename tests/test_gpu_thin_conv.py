"""rgbd_conv3x3_thin_in / rgbd_conv3x3_thin_out (csrc/thin_conv.hip), the image-facing 3x3 layers of Feature_encoder /
Feature_decoder, alone on the GPU (cases, statements and bound: tests/features_cases.py; test_features_cases.py shows on the
CPU that every wrong reading of taps and bias is rejected).

Per case and channel stride: against the fp64 statement within 8x the error of torch's fp32 convolution (floored at 2^-23);
the same bits from two calls; image 0 of the batch as the image alone; NaN in the input's padding channels never reaches the
output; a sentinel in the output's padding channels and behind the output survives; refusals that write nothing.  The figures
are printed and recorded in DESIGN.md 5.6."""
import ctypes

import pytest
import torch

import features_cases as fc
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


def _thin_in_gpu(L, x, w, b, pad):
    B, ci, H, W = x.shape
    co = w.shape[0]
    xd, wd, bd = x.cuda().contiguous(), w.cuda().contiguous(), b.cuda()  # (held until the call has run)
    y = torch.full((B * H * W * (co + pad) + 64,), SENTINEL, device="cuda")
    assert L.rgbd_conv3x3_thin_in(_p(xd), B, ci, H, W, _p(wd), _p(bd), co, _p(y), co + pad, _stream()) == 0
    torch.cuda.synchronize()
    body = y[:B * H * W * (co + pad)].reshape(B, H, W, co + pad)
    assert (y[B * H * W * (co + pad):] == SENTINEL).all() and (body[..., co:] == SENTINEL).all()
    return body[..., :co].cpu()


def _thin_out_gpu(L, x, w, b, pad):
    B, H, W, ci = x.shape
    co = w.shape[0]
    xd = torch.full((B, H, W, ci + pad), float("nan"), device="cuda")  # a read of the pad poisons the result
    xd[..., :ci] = x.cuda()
    wd, bd = w.cuda().contiguous(), b.cuda()
    y = torch.full((B * co * H * W + 64,), SENTINEL, device="cuda")
    assert L.rgbd_conv3x3_thin_out(_p(xd), ci + pad, B, H, W, ci, _p(wd), _p(bd), co, _p(y), _stream()) == 0
    torch.cuda.synchronize()
    assert (y[B * co * H * W:] == SENTINEL).all()
    return y[:B * co * H * W].reshape(B, co, H, W).cpu()


def _check(op, run, name, pad):
    L = _lib()
    x, w, b = fc.kernel_inputs(op, name)
    ref, e_ref = fc.kernel_refs(op, name)
    out = run(L, x, w, b, pad)
    assert out.shape == ref.shape and torch.isfinite(out).all()
    e = fc.rel_err(out, ref)
    print(f"{op} {name} stride = channels + {pad}: e_gpu {e:.3e}, e_ref {e_ref:.3e} (floor {fc.FLOOR:.3e}), "
          f"ratio {e / max(e_ref, fc.FLOOR):.3f}")
    assert fc.accept(e, e_ref), (e, e_ref)
    assert _bits(run(L, x, w, b, pad), out)
    assert _bits(run(L, x[:1], w, b, pad), out[:1])  # image 0 alone
    assert _bits(run(L, x, w, b, 16 - pad), out)     # the stride changes no bit either


@pytest.mark.parametrize("pad", fc.PADS)
@pytest.mark.parametrize("name", list(fc.THIN_IN_CASES))
def test_thin_in_kernel(name, pad):
    _check("thin_in", _thin_in_gpu, name, pad)


@pytest.mark.parametrize("pad", fc.PADS)
@pytest.mark.parametrize("name", list(fc.THIN_OUT_CASES))
def test_thin_out_kernel(name, pad):
    _check("thin_out", _thin_out_gpu, name, pad)


def test_a_missing_bias_is_a_zero_bias():
    L = _lib()
    for op, run, name in (("thin_in", _thin_in_gpu, "3to64_13x7"), ("thin_out", _thin_out_gpu, "64to3_13x7")):
        x, w, b = fc.kernel_inputs(op, name)
        B, H, W = fc.KERNEL_B, 13, 7
        want = run(L, x, w, torch.zeros_like(b), 0)
        xd, wd = x.cuda().contiguous(), w.cuda().contiguous()
        y = torch.full(want.shape, SENTINEL, device="cuda")
        if op == "thin_in":
            assert L.rgbd_conv3x3_thin_in(_p(xd), B, 3, H, W, _p(wd), None, 64, _p(y), 64, _stream()) == 0
        else:
            assert L.rgbd_conv3x3_thin_out(_p(xd), 64, B, H, W, 64, _p(wd), None, 3, _p(y), _stream()) == 0
        torch.cuda.synchronize()
        assert _bits(y.cpu(), want)


def test_thin_in_rejects_bad_arguments():
    L = _lib()
    B, ci, H, W, co, cs = 2, 3, 5, 6, 16, 32
    x = torch.randn(B, ci + 2, H, W, device="cuda")
    w, b = torch.randn(64, ci + 2, 3, 3, device="cuda"), torch.randn(64, device="cuda")
    y = torch.full((B * H * W * 80 + 4,), SENTINEL, device="cuda")
    X, WT, Y = "x", "w", "y"

    def call(B_=B, ci_=ci, H_=H, W_=W, co_=co, cs_=cs, ptr=None):
        p = {X: x.data_ptr(), WT: w.data_ptr(), Y: y.data_ptr()}
        p.update(ptr or {})
        return L.rgbd_conv3x3_thin_in(p[X], B_, ci_, H_, W_, p[WT], _p(b), co_, p[Y], cs_, _stream())

    bad = [dict(ptr={X: None}), dict(ptr={WT: None}), dict(ptr={Y: None}), dict(ptr={Y: y.data_ptr() + 4}), dict(ci_=5), dict(ci_=0),
           dict(co_=0), dict(co_=65, cs_=80), dict(co_=68, cs_=80), dict(co_=6, cs_=8), dict(cs_=co - 4), dict(cs_=co + 2), dict(B_=0),
           dict(H_=0), dict(W_=0), dict(B_=-1), dict(B_=65536), dict(H_=65536, W_=65536)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (y[:co] == SENTINEL).any() and (y[co:cs] == SENTINEL).all()


def test_thin_out_rejects_bad_arguments():
    L = _lib()
    B, ci, H, W, co, cs = 2, 16, 5, 6, 3, 32
    x = torch.randn(B, H, W, 80, device="cuda")
    w, b = torch.randn(8, 68, 3, 3, device="cuda"), torch.randn(8, device="cuda")
    y = torch.full((B * 8 * H * W + 4,), SENTINEL, device="cuda")
    X, WT, Y = "x", "w", "y"

    def call(B_=B, ci_=ci, H_=H, W_=W, co_=co, cs_=cs, ptr=None):
        p = {X: x.data_ptr(), WT: w.data_ptr(), Y: y.data_ptr()}
        p.update(ptr or {})
        return L.rgbd_conv3x3_thin_out(p[X], cs_, B_, H_, W_, ci_, p[WT], _p(b), co_, p[Y], _stream())

    bad = [dict(ptr={X: None}), dict(ptr={WT: None}), dict(ptr={Y: None}), dict(ptr={X: x.data_ptr() + 4}), dict(ci_=5, cs_=8),
           dict(ci_=0), dict(ci_=68, cs_=80), dict(ci_=6, cs_=8), dict(co_=0), dict(co_=5), dict(co_=6), dict(co_=65), dict(cs_=ci - 4),
           dict(cs_=ci + 2), dict(B_=0), dict(H_=0), dict(W_=0), dict(B_=-1), dict(B_=65536), dict(H_=65536, W_=65536)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (y[:B * co * H * W] == SENTINEL).any() and (y[B * co * H * W:] == SENTINEL).all()
