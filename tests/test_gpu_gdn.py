"""The fused GDN / IGDN launch (csrc/gdn.hip) alone, behind rgbd_gdn_nchw (include/rgbd_amd.h), against the same formula in
float64 evaluated from the fp32 parametrized beta / gamma:

    out[n, i, p] = x[n, i, p] * f(beta'[i] + sum_j gamma'[i, j] * x[n, j, p]^2)  (+ res[n, i, p]),  f = 1 / sqrt or sqrt

Tolerance, per element (a bound from the arithmetic, not a measurement): the norm is a chain of c + 1 non-negative fp32 terms
(relative error <= (c + 1) * 2^-24 before, half of that after the square root), then come four single roundings (square of x,
sqrt, divide, multiply), then the residual add rounds the result once:

    |out - ref| <= ((c / 2 + 4) * |x * f(norm)| + |ref|) * 2^-24

The raw gamma is dense with values below the parametrizer's bound (the clamp acts), beta varies per channel, and the inputs
span 1e-3 ... 1e2 in magnitude with exact zeros."""
import ctypes

import numpy as np
import pytest
import torch

from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

EINVAL = -22
SENTINEL = 12345.0
GUARD = 4096
SHAPES = [(1, 16, 1, 1), (1, 20, 3, 5), (2, 192, 7, 9), (1, 128, 8, 8), (3, 192, 4, 4)]
ZERO_PIXEL_SHAPE = (2, 192, 7, 9)  # image 1, pixel (3, 4) is all zeros there: norm = beta


def _lib():
    require_gpu()
    from rgbd_amd import _lib as lib

    return lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _params(c, seed):
    """Raw beta [c] / gamma [c, c] as a state_dict holds them (before NonNegativeParametrizer.forward)."""
    g = torch.Generator().manual_seed(1000 + seed)
    beta = torch.sqrt(0.2 + 2.0 * torch.rand(c, generator=g))  # beta' in 0.2 ... 2.2, a different one per channel
    gamma = 0.08 * torch.rand(c, c, generator=g) - 0.015       # dense; about a fifth of it below the bound 2^-18
    gamma += torch.sqrt(torch.tensor(0.1)) * torch.eye(c)
    return beta.float().contiguous(), gamma.float().contiguous()


def _parametrized(raw, minimum):
    """NonNegativeParametrizer.forward (ops/parametrizers.py:21-45) as torch computes it in fp32."""
    pedestal = torch.tensor([(2.0 ** -18) ** 2], dtype=torch.float32)
    bound = torch.tensor([(minimum + (2.0 ** -18) ** 2) ** 0.5], dtype=torch.float32)
    return torch.max(raw, bound) ** 2 - pedestal


def _inputs(shape, seed):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (5.0 * torch.rand(shape, generator=g) - 3.0)  # 1e-3 ... 1e2
    x = mag * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    x = torch.where(torch.rand(shape, generator=g) < 0.1, torch.zeros(()), x).float()
    if shape == ZERO_PIXEL_SHAPE:
        x[1, :, 3, 4] = 0.0
    res = (3.0 * torch.randn(shape, generator=g)).float()
    return x.contiguous(), res.contiguous()


_CASES = {}


def _case(shape):
    """(x, res, raw beta, raw gamma, {(inverse, with_res): (float64 reference, tolerance)}): computed once per shape."""
    if shape not in _CASES:
        c = shape[1]
        x, res = _inputs(shape, 7 * c + shape[0])
        beta, gamma = _params(c, c)
        bp, gp = _parametrized(beta, 1e-6).double(), _parametrized(gamma, 0.0).double()
        assert (gamma < 2.0 ** -18).float().mean() > 0.05 and (gp > 0).float().mean() > 0.5
        xd = x.double()
        norm = bp[None, :, None, None] + torch.einsum("ij,njhw->nihw", gp, xd * xd)
        refs = {}
        for inverse in (0, 1):
            core = xd * (torch.sqrt(norm) if inverse else 1.0 / torch.sqrt(norm))
            for with_res in (0, 1):
                ref = core + res.double() if with_res else core
                tol = ((c / 2 + 4) * core.abs() + ref.abs()) * 2.0 ** -24
                refs[(inverse, with_res)] = (ref, tol)
        _CASES[shape] = (x, res, beta, gamma, refs)
    return _CASES[shape]


def _run(L, x, beta, gamma, inverse, res, expect=0):
    """One rgbd_gdn_nchw call on device copies; returns the destination (with its guard region) as a CPU tensor."""
    n, c, h, w = x.shape
    xd = x.cuda()
    rd = res.cuda() if res is not None else None
    y = torch.full((x.numel() + GUARD,), SENTINEL, device="cuda")
    b, g = beta.numpy(), gamma.numpy()
    rc = L.rgbd_gdn_nchw(xd.data_ptr(), n, c, h, w, _f32p(b), _f32p(g), inverse, rd.data_ptr() if rd is not None else None,
                         y.data_ptr(), _stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("with_res", [0, 1])
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gdn_vs_f64(shape, inverse, with_res):
    L = _lib()
    x, res, beta, gamma, refs = _case(shape)
    ref, tol = refs[(inverse, with_res)]
    y = _run(L, x, beta, gamma, inverse, res if with_res else None)
    out = y[:x.numel()].view(shape)
    assert torch.isfinite(out).all()
    err = (out.double() - ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"gdn {shape} inverse={inverse} res={with_res}: worst |err| / bound = {worst:.3f}")
    assert (err <= tol).all(), f"worst |err| / bound = {worst}"
    assert (y[x.numel():] == SENTINEL).all(), "the guard region behind the destination was written"
    # x = 0 gives exactly the residual (or 0); at the all-zero pixel the norm is beta itself
    zero = x == 0
    assert (out[zero] == (res[zero] if with_res else 0.0)).all()


def test_gdn_same_bits_across_calls_batches_and_tiles():
    """Equal bits for two calls, for B = 3 against three B = 1 calls, and for every pixel tile the launcher can be forced to."""
    L = _lib()
    try:
        for shape in ((3, 192, 4, 4), (2, 192, 7, 9), (1, 20, 3, 5)):
            x, res, beta, gamma, _ = _case(shape)
            for inverse in (0, 1):
                for r in (None, res):
                    assert L.rgbd_debug_force_gdn_tile(0) == 0
                    a = _run(L, x, beta, gamma, inverse, r)
                    assert torch.equal(a, _run(L, x, beta, gamma, inverse, r)), "two calls differ"
                    per = [_run(L, x[i:i + 1], beta, gamma, inverse, None if r is None else r[i:i + 1])[:x[0].numel()]
                           for i in range(shape[0])]
                    assert torch.equal(a[:x.numel()], torch.cat(per)), "the batch and its images one by one differ"
                    for tile in (16, 32, 64):
                        assert L.rgbd_debug_force_gdn_tile(tile) == 0
                        assert torch.equal(a, _run(L, x, beta, gamma, inverse, r)), f"tile {tile} differs from the automatic one"
        assert L.rgbd_debug_force_gdn_tile(48) == EINVAL
    finally:
        L.rgbd_debug_force_gdn_tile(0)


def test_gdn_bad_arguments_write_nothing():
    L = _lib()
    shape = (1, 20, 3, 5)
    x, res, beta, gamma, _ = _case(shape)
    n, c, h, w = shape
    xd, rd = x.cuda(), res.cuda()
    y = torch.full((x.numel() + GUARD,), SENTINEL, device="cuda")
    b, g = _f32p(beta.numpy()), _f32p(gamma.numpy())
    big = np.zeros(513 * 513, dtype=np.float32)
    bad = [
        (None, n, c, h, w, b, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, c, h, w, None, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, c, h, w, b, None, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, c, h, w, b, g, 0, rd.data_ptr(), None),
        (xd.data_ptr(), n, 0, h, w, b, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, -16, h, w, b, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, 513, 1, 1, _f32p(big), _f32p(big), 0, None, y.data_ptr()),
        (xd.data_ptr(), 0, c, h, w, b, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, c, 0, w, b, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, c, h, -1, b, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, c, h, w, b, g, 2, rd.data_ptr(), y.data_ptr()),
    ]
    for args in bad:
        assert L.rgbd_gdn_nchw(*args, _stream()) == EINVAL, args[1:5]
        torch.cuda.synchronize()
        assert (y == SENTINEL).all(), "a rejected call wrote to the destination"
    # ... and the same buffers are fine with good arguments
    assert L.rgbd_gdn_nchw(xd.data_ptr(), n, c, h, w, b, g, 0, rd.data_ptr(), y.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert (y[:x.numel()] != SENTINEL).all() and (y[x.numel():] == SENTINEL).all()
