"""SURVEY 8(a) row a6 in isolation: the pointwise operators of Bi-SPF / ESA / SE_Block (modules/transform/attention.py:35-97,
modules/transform/entropy.py:75) through the C ABI against torch's own CPU operators on the same inputs."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu


def _run(op, x, oh=0, ow=0, w0=None, w1=None):
    import rgbd_amd  # noqa: F401
    from rgbd_amd._lib import check, lib

    require_gpu()
    n, c, h, w = x.shape
    if op == 0:
        oh, ow = (h - 7) // 3 + 1, (w - 7) // 3 + 1
    elif op >= 2:
        oh, ow = h, w
    xd = x.cuda().contiguous()
    y = torch.empty((n, c, oh, ow), dtype=torch.float32, device="cuda")
    f32p = ctypes.POINTER(ctypes.c_float)
    p0 = w0.contiguous().numpy().ctypes.data_as(f32p) if w0 is not None else None
    p1 = w1.contiguous().numpy().ctypes.data_as(f32p) if w1 is not None else None
    check(lib().rgbd_pointwise_nchw(op, ctypes.c_void_p(xd.data_ptr()), n, c, h, w, oh, ow, p0, p1,
                                    ctypes.c_void_p(y.data_ptr()), None), "pointwise")
    return y.cpu()


@pytest.mark.parametrize("n,c,h,w", [(1, 48, 31, 47), (2, 48, 63, 79), (1, 24, 7, 7), (3, 16, 10, 22)])
def test_maxpool7s3_matches_torch(n, c, h, w):
    x = torch.randn(n, c, h, w)
    assert torch.equal(_run(0, x), F.max_pool2d(x, kernel_size=7, stride=3))  # a maximum is exact


@pytest.mark.parametrize("n,c,h,w,oh,ow", [(1, 48, 9, 14, 64, 96), (2, 48, 19, 25, 128, 160), (1, 16, 1, 1, 8, 8),
                                         (1, 32, 5, 7, 5, 7), (1, 48, 41, 53, 256, 320)])
def test_bilinear_matches_torch(n, c, h, w, oh, ow):
    x = torch.randn(n, c, h, w)
    ref = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False)
    got = _run(1, x, oh, ow)
    # the reference's CPU arithmetic: bit for bit the oracle's C restatement of ATen's two bilinear kernels ...
    import ctypes

    import numpy as np

    from oracle import cpu_arith as ca

    want = np.empty((n, c, oh, ow), np.float32)
    xn = np.ascontiguousarray(x.numpy())
    for i in range(n):
        ca.lib().orc_bilinear(xn[i].ctypes.data_as(ctypes.c_void_p), c, h, w, want[i].ctypes.data_as(ctypes.c_void_p), oh, ow)
    assert np.array_equal(got.numpy(), want)
    # ... and torch on this box's CPU to rounding (bit for bit where its kernels are the survey container's)
    assert float((got - ref).abs().max()) <= 2e-6 * float(ref.abs().max())


@pytest.mark.parametrize("n,c,h,w,op", [(1, 192, 16, 24, 2), (2, 384, 8, 10, 2), (4, 1280, 32, 40, 3), (1, 2432, 8, 12, 3),
                                        (1, 192, 96, 96, 2)])  # (96 x 96: the mean's cascade reaches its level 2)
def test_se_block_matches_torch(n, c, h, w, op):
    g = torch.Generator().manual_seed(c + h)
    x = torch.randn(n, c, h, w, generator=g)
    w0 = torch.randn(c // 16, c, generator=g) * 0.05
    w1 = torch.randn(c, c // 16, generator=g) * 0.2
    gate = torch.sigmoid(F.linear(torch.relu(F.linear(x.mean(dim=(2, 3)), w0)), w1)).view(n, c, 1, 1)
    ref = x * gate if op == 2 else x + x * gate
    got = _run(op, x, w0=w0, w1=w1)
    # ATen's cascade-sum mean, MKL's main dot-product order, Sleef's sigmoid; rows that MKL's row partition gives
    # another order are not modelled by this entry point (the codec takes them from the measured tables): 1e-6-level
    assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
    assert torch.equal(got, _run(op, x, w0=w0, w1=w1))  # and it is deterministic
    # ... and bit for bit the oracle's restatement of that arithmetic (every row of both Linear layers in the main order, which is
    # what this entry point runs): mean -> fc.0 -> ReLU -> fc.2 -> vector sigmoid, then x * g resp. x + x * g in two roundings
    from oracle import cpu_arith as ca

    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    xn, w0n, w1n = np.ascontiguousarray(x.numpy()), np.ascontiguousarray(w0.numpy()), np.ascontiguousarray(w1.numpy())
    gates = np.empty((n, c), np.float32)
    for i in range(n):
        mean, hid, lin = np.empty(c, np.float32), np.empty(c // 16, np.float32), np.empty(c, np.float32)
        ca.lib().orc_mean_rows(P(xn[i]), c, h * w, P(mean))
        ca.lib().orc_linear_b1(P(w0n), P(mean), c // 16, c, None, P(hid))
        hid = np.maximum(hid, np.float32(0))
        ca.lib().orc_linear_b1(P(w1n), P(hid), c, c // 16, None, P(lin))
        gates[i] = ca.sigmoid(lin)
    t = xn * gates[:, :, None, None]
    want = t if op == 2 else xn + t
    bad = np.flatnonzero(got.numpy().reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (f"{bad.size} of {want.size} elements differ from the oracle; first at flat index {int(bad[0])}: "
                           f"got {got.numpy().reshape(-1)[bad[0]]!r}, want {want.reshape(-1)[bad[0]]!r}")
