"""The reference-arithmetic pointwise kernels of csrc/pointwise.hip ALONE (channel_mean_ref_kernel, se_linear_ref_kernel,
sigmoid_gate_ref_kernel, small_conv_ref_kernel and the stride-2 deconv recipe route), through the C ABI's rgbd_ref_* hooks,
against oracle/cpu_arith.c -- BIT FOR BIT (np.array_equal on the fp32 outputs), at the cases of tests/refpointwise_cases.py.

tests/test_refpointwise_cases.py shows (without a GPU) that every case tells the oracle's summation structure from its
neighbours; oracle/cpu_arith.c itself is pinned to torch CPU and to frozen hashes in tests/test_oracle_arith.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gridcap_cases as gc
import refpointwise_cases as rc
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

f32p = ctypes.POINTER(ctypes.c_float)
i32p = ctypes.POINTER(ctypes.c_int32)
EINVAL = -22


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).contiguous()


def _ptr(t, offset_floats=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * offset_floats)


def _host(a, typ=f32p):
    return None if a is None else a.ctypes.data_as(typ)


def _report(got, want):
    """number of differing elements, the first differing index and both values"""
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(-1) & ~(np.isnan(got) & np.isnan(want)).reshape(-1))
    if bad.size == 0:
        return "equal"
    i = np.unravel_index(bad[0], got.shape)
    return f"{bad.size} of {got.size} elements differ; first at {tuple(int(v) for v in i)}: got {got[i]!r}, want {want[i]!r}"


def _check(rv, what):
    from rgbd_amd._lib import check

    check(rv, what)


# ------------------------------------------------------------------------------------------------ hooks
def gpu_mean(x, dev, out=None, offset=0, mstride=None):
    from rgbd_amd._lib import lib

    n, c, h, w = x.shape
    mstride = c if mstride is None else mstride
    xd = _dev(x, dev)
    out = torch.empty((n, mstride), device=dev) if out is None else out
    _check(lib().rgbd_ref_channel_mean(_ptr(xd), n, c, h, w, _ptr(out, offset), mstride, None), "ref_channel_mean")
    return out


def gpu_linear(W, x, cls, form, act, stage, dev):
    from rgbd_amd._lib import lib

    n, K = x.shape
    J = W.shape[0]
    xd = _dev(x, dev)
    yd = torch.empty((n, J), device=dev)
    Wc = np.ascontiguousarray(W, np.float32)
    cl = None if cls is None else np.ascontiguousarray(cls, np.int32)
    _check(lib().rgbd_ref_linear(_host(Wc), _ptr(xd), n, K, J, _host(cl, i32p), form, act, stage, _ptr(yd), None), "ref_linear")
    return yd.cpu().numpy()


def gpu_sigmoid_gate(t, mul, res, per_image, threads, dev):
    from rgbd_amd._lib import lib

    n, c, h, w = t.shape
    td, md, rd = _dev(t, dev), _dev(mul, dev), _dev(res, dev)
    yd = torch.full(t.shape, 7.0, device=dev)
    _check(lib().rgbd_ref_sigmoid_gate(_ptr(td), _ptr(md), _ptr(rd), n, c, h, w, per_image, threads, _ptr(yd), None), "ref_sigmoid_gate")
    return yd.cpu().numpy()


def gpu_small_conv(c, x, wt, b, extra, dev, kblocks="case"):
    from rgbd_amd._lib import lib

    kb = c["kblocks"] if kblocks == "case" else kblocks
    kbn = None if kb is None else np.ascontiguousarray(kb, np.int32)
    oh, ow = (c["h"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1, (c["w"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1
    xd, r1, m, r2 = _dev(x, dev), _dev(extra["res1"], dev), _dev(extra["mul"], dev), _dev(extra["res2"], dev)
    yd = torch.full((c["n"], c["cout"], oh, ow), 7.0, device=dev)
    y2 = torch.full_like(yd, 9.0) if c["y2"] else None
    _check(lib().rgbd_ref_small_conv_nchw(_ptr(xd), c["n"], c["cin"], c["h"], c["w"], _host(wt), _host(b), c["cout"], c["k"], c["stride"],
                                          c["pad"], c["act"], c["ckbd"], _host(kbn, i32p), 0 if kbn is None else len(kbn), _ptr(r1),
                                          _ptr(m), _ptr(r2), _ptr(yd), _ptr(y2), None), "ref_small_conv")
    return yd.cpu().numpy(), (None if y2 is None else y2.cpu().numpy())


def gpu_deconv(c, x, wt, b, dev):
    from rgbd_amd._lib import lib

    rec = np.ascontiguousarray(c["recipe"], np.int32)
    xd = _dev(x, dev)
    yd = torch.full((c["B"], c["cout"], 2 * c["h"], 2 * c["w"]), 7.0, device=dev)
    _check(lib().rgbd_ref_deconv_s2_nchw(_ptr(xd), c["B"], c["cin"], c["h"], c["w"], _host(wt), _host(b), c["cout"], c["act"],
                                         _host(rec, i32p), len(rec), _ptr(yd), None), "ref_deconv_s2")
    return yd.cpu().numpy()


# ------------------------------------------------------------------------------------------------ mean
@pytest.mark.parametrize("shape", rc.MEAN_SHAPES, ids=str)
def test_channel_mean_bit_exact(shape):
    dev = require_gpu()
    x = rc.mean_input(shape)
    want = rc.mean_expected(x)
    got = gpu_mean(x, dev).cpu().numpy()
    assert np.array_equal(got, want), _report(got, want)
    assert np.array_equal(gpu_mean(x, dev).cpu().numpy(), got)  # twice the same bits
    if shape[0] > 1:  # image 1 of the batch == that image alone
        assert np.array_equal(gpu_mean(x[1:2], dev).cpu().numpy()[0], got[1])


def test_channel_means_of_two_tensors_side_by_side():
    """the hyper-synthesis "cat(own, other)" use: both tensors' means into one [n][c1 + c2 (+ slack)] buffer through mstride"""
    dev = require_gpu()
    sa, sb = rc.MEAN_CAT
    xa, xb = rc.mean_input(sa), rc.mean_input(sb)
    n, ca_, cb_ = sa[0], sa[1], sb[1]
    stride = ca_ + cb_ + 5
    buf = torch.full((n, stride), -123.25, device=dev)
    gpu_mean(xa, dev, out=buf, offset=0, mstride=stride)
    gpu_mean(xb, dev, out=buf, offset=ca_, mstride=stride)
    got = buf.cpu().numpy()
    want = np.full((n, stride), -123.25, np.float32)
    want[:, :ca_] = rc.mean_expected(xa)
    want[:, ca_:ca_ + cb_] = rc.mean_expected(xb)
    assert np.array_equal(got, want), _report(got, want)


# ------------------------------------------------------------------------------------------------ Linear
@pytest.mark.parametrize("case", rc.LINEAR_CASES, ids=rc.case_id)
def test_linear_bit_exact(case):
    dev = require_gpu()
    W, x, cls = rc.linear_inputs(case)
    want = rc.linear_expected(case, W, x, cls)
    got = gpu_linear(W, x, cls, case["form"], case["act"], case["stage"], dev)
    assert np.array_equal(got, want), _report(got, want)
    if case["group"] == "d":
        assert np.array_equal(gpu_linear(W, x, cls, case["form"], case["act"], case["stage"], dev), got)  # twice the same bits
        if case["n"] > 1:  # row 1 of the batch == that row alone
            assert np.array_equal(gpu_linear(W, x[1:2], cls, case["form"], case["act"], case["stage"], dev)[0], got[1])


def test_linear_null_classes_are_the_main_order():
    dev = require_gpu()
    case = next(c for c in rc.LINEAR_CASES if c["id"] == "b-K176-J48-n1-all0-act0-fc2")
    W, x, cls = rc.linear_inputs(case)
    got = gpu_linear(W, x, None, -1, 0, 1, dev)
    want = rc.linear_expected(case, W, x, cls)
    assert np.array_equal(got, want), _report(got, want)


# ------------------------------------------------------------------------------------------------ sigmoid gate
@pytest.mark.parametrize("case", rc.SIGMOID_CASES, ids=rc.case_id)
def test_sigmoid_gate_bit_exact(case):
    """Planted inputs: every tail position and >= 1000 body positions hold an argument on which the vector and the scalar sigmoid
    differ, so a wrong tail MAP fails here; the "specials" cases add +-0, denormals, the cut-offs of both expf restatements,
    +-inf and nan.  (+-inf / nan: the oracle leans on a float -> int conversion C leaves undefined; it gives torch's 1, 0, nan on
    the CPUs this was run on -- tests/test_oracle_arith.py pins it to torch.)"""
    dev = require_gpu()
    t, mul, res, tail, planted, special = rc.sigmoid_inputs(case)
    want = rc.sigmoid_expected(case, t, mul, res)
    got = gpu_sigmoid_gate(t, mul, res, case["per_image"], case["threads"], dev)
    assert np.array_equal(got, want, equal_nan=True), _report(got, want)
    assert rc.bits_equal(got, want), "sign of a zero / a denormal differs: " + _report(got, want)
    if case["threads"] == 8:
        again = gpu_sigmoid_gate(t, mul, res, case["per_image"], case["threads"], dev)
        assert rc.bits_equal(again, got)  # twice the same bits
        if case["per_image"] and t.shape[0] > 1:  # image 1 of the batch == that image alone
            alone = gpu_sigmoid_gate(t[1:2], None if mul is None else mul[1:2], None if res is None else res[1:2], 1, 8, dev)
            assert rc.bits_equal(alone[0], got[1])


# ------------------------------------------------------------------------------------------------ small conv
def _torch_bound(got, ref):
    """tests/test_gpu_conv.py's bound against torch: 2e-5 * (max|ref| + 1e-3)"""
    err = float(np.abs(got - ref).max())
    tol = 2e-5 * (float(np.abs(ref).max()) + 1e-3)
    assert err <= tol, f"max |gpu - torch| = {err:.3e} > {tol:.3e}"


@pytest.mark.parametrize("case", rc.SMALL_CONV_CASES, ids=rc.case_id)
def test_small_conv_bit_exact(case):
    dev = require_gpu()
    x, wt, b, extra = rc.small_conv_inputs(case)
    want = rc.small_conv_expected(case, x, wt, b, extra)
    got, got2 = gpu_small_conv(case, x, wt, b, extra, dev)
    assert np.array_equal(got, want), _report(got, want)
    if case["y2"]:
        assert np.array_equal(got2, want), "second destination: " + _report(got2, want)
    if len(case["kblocks"]) == 1:  # no table = one block
        alone, _ = gpu_small_conv(case, x, wt, b, extra, dev, kblocks=None)
        assert np.array_equal(alone, got)
    if case["id"].startswith("syn"):
        assert np.array_equal(gpu_small_conv(case, x, wt, b, extra, dev)[0], got)  # twice the same bits
    if case["act"] == 0 and not case["mul"] and not case["ckbd"]:  # oracle and kernel are not wrong together
        ref = F.conv2d(torch.from_numpy(x), torch.from_numpy(wt), torch.from_numpy(b), stride=case["stride"], padding=case["pad"]).numpy()
        for key in ("res1", "res2"):
            if extra[key] is not None:
                ref = ref + extra[key]
        _torch_bound(got, ref)


# ------------------------------------------------------------------------------------------------ stride-2 deconv
@pytest.mark.parametrize("case", rc.DECONV_CASES, ids=rc.case_id)
def test_deconv_s2_recipe_bit_exact(case):
    dev = require_gpu()
    x, wt, b = rc.deconv_inputs(case)
    want = rc.deconv_expected(case, x, wt, b)
    got = gpu_deconv(case, x, wt, b, dev)
    assert np.array_equal(got, want), _report(got, want)
    if case["id"].startswith("syn"):
        assert np.array_equal(gpu_deconv(case, x, wt, b, dev), got)  # twice the same bits
    # every recipe covers all taps: within the conv bound of torch's conv_transpose2d
    ref = F.conv_transpose2d(torch.from_numpy(x), torch.from_numpy(wt), torch.from_numpy(b), stride=2, padding=2, output_padding=1)
    if case["act"] == rc.ACT_LEAKY:
        ref = F.leaky_relu(ref, 0.01)
    _torch_bound(got, ref.numpy())


# ------------------------------------------------------------------------------------------------ past the grid caps
# tests/gridcap_cases.py: sigmoid_gate_ref_kernel past 8192 x 256, small_conv_ref_kernel and the deconv route's gather / scatter
# kernels past 2048 x 256 (two sweeps, the last one ragged; the 9- and 6-tap gathers three and two; the weight gather in a case
# of its own).  Same oracle, same bit-for-bit
# rule as the tests above, over the whole pre-filled output; twice the same bits.
def test_sigmoid_gate_past_the_grid_cap():
    dev = require_gpu()
    bc = gc.build_sigmoid(rc)
    c = bc["case"]
    outs = [gpu_sigmoid_gate(bc["t"], bc["mul"], bc["res"], c["per_image"], c["threads"], dev) for _ in range(2)]
    assert bc["stages"]["sigmoid"]["accept"]({"y": outs[0]}) == []
    assert rc.bits_equal(outs[1], outs[0])


def test_small_conv_past_the_grid_cap():
    dev = require_gpu()
    bc = gc.build_small_conv(rc)
    outs = [gpu_small_conv(bc["case"], bc["x"], bc["wt"], bc["b"], bc["extra"], dev)[0] for _ in range(2)]
    assert bc["stages"]["small_conv"]["accept"]({"y": outs[0]}) == []
    assert np.array_equal(outs[1], outs[0])


def test_deconv_s2_past_the_grid_cap():
    dev = require_gpu()
    bc = gc.build_deconv(rc)
    outs = [gpu_deconv(bc["case"], bc["x"], bc["wt"], bc["b"], dev) for _ in range(2)]
    for name, stage in bc["stages"].items():
        assert stage["accept"]({"y": outs[0]}) == [], name
    assert np.array_equal(outs[1], outs[0])
    ref = F.leaky_relu(F.conv_transpose2d(torch.from_numpy(bc["x"]), torch.from_numpy(bc["wt"]), torch.from_numpy(bc["b"]), stride=2, padding=2,
                                          output_padding=1), 0.01)
    _torch_bound(outs[0], ref.numpy())


def test_deconv_s2_wide_layer_past_the_grid_cap():
    """gather_wslabs_kernel past 2048 x 256: its work is the layer's (cout_pad x taps x cin_pad / 4 float4s), so a 496 -> 496 layer
    on 2 x 4 pixels crosses at the 9-tap phase.  test_deconv_s2_recipe_bit_exact's rule."""
    dev = require_gpu()
    bc = gc.build_deconv_wide(rc)
    outs = [gpu_deconv(bc["case"], bc["x"], bc["wt"], bc["b"], dev) for _ in range(2)]
    assert bc["stages"]["wslabs_ph0"]["accept"]({"y": outs[0]}) == []
    assert np.array_equal(outs[1], outs[0])
    ref = F.leaky_relu(F.conv_transpose2d(torch.from_numpy(bc["x"]), torch.from_numpy(bc["wt"]), torch.from_numpy(bc["b"]), stride=2, padding=2,
                                          output_padding=1), 0.01)
    _torch_bound(outs[0], ref.numpy())


# ------------------------------------------------------------------------------------------------ refusals
def test_malformed_arguments_are_refused_on_the_host():
    """every refusal returns -22 before anything is allocated or launched: the device pointers below are never touched"""
    dev = require_gpu()
    from rgbd_amd._lib import lib

    L = lib()
    buf = torch.zeros(4096, device=dev)
    p, null = _ptr(buf), None
    # mean: null pointers, non-positive sizes, c % 16, mstride < c
    for args in [(null, 1, 16, 2, 2, p, 16), (p, 1, 16, 2, 2, null, 16), (p, 0, 16, 2, 2, p, 16), (p, 1, 16, 0, 2, p, 16), (p, 1, 16, 2, -1, p, 16),
                 (p, 1, 24, 2, 2, p, 24), (p, 1, 0, 2, 2, p, 16), (p, 1, 32, 2, 2, p, 16)]:
        assert L.rgbd_ref_channel_mean(*args, None) == EINVAL, args
    # Linear
    W = np.zeros((48, 32), np.float32)
    ok_cls = np.zeros(48, np.int32)
    bad_cls, neg_cls = ok_cls.copy(), ok_cls.copy()
    bad_cls[47], neg_cls[0] = 3, -1
    lin = lambda **kw: L.rgbd_ref_linear(*[{**dict(W=_host(W), x=p, n=1, K=32, J=48, cls=_host(ok_cls, i32p), form=-1, act=0, stage=1, y=p),  # noqa: E731
                                           **kw}[k] for k in ("W", "x", "n", "K", "J", "cls", "form", "act", "stage", "y")], None)
    for kw in [dict(W=None), dict(x=None), dict(y=None), dict(n=0), dict(K=0), dict(J=-3), dict(cls=_host(bad_cls, i32p)),
               dict(cls=_host(neg_cls, i32p)), dict(form=0), dict(form=2), dict(form=4), dict(act=2), dict(act=5), dict(stage=2), dict(stage=-1),
               dict(J=40), dict(stage=0, K=24)]:
        assert lin(**kw) == EINVAL, kw
    # sigmoid gate
    for args in [(null, null, null, 1, 16, 2, 2, 1, 8, p), (p, null, null, 1, 16, 2, 2, 1, 8, null), (p, null, null, 0, 16, 2, 2, 1, 8, p),
                 (p, null, null, 1, 0, 2, 2, 1, 8, p), (p, null, null, 1, 16, 2, 0, 1, 8, p), (p, null, null, 1, 16, 2, 2, 1, 0, p),
                 (p, null, null, 1, 16, 2, 2, 2, 8, p)]:
        assert L.rgbd_ref_sigmoid_gate(*args, None) == EINVAL, args
    # small conv: K blocks that do not sum to cin * k * k, more than 16 of them, a zero block, k > 3, bad stride / act / checkerboard
    wt, b = np.zeros((16, 4, 3, 3), np.float32), np.zeros(16, np.float32)

    def sc(kb, **kw):
        a = {**dict(x=p, n=1, cin=4, h=5, w=5, wt=_host(wt), b=_host(b), cout=16, k=3, stride=1, pad=1, act=0, ckbd=0, y=p), **kw}
        kbn = None if kb is None else np.asarray(kb, np.int32)
        return L.rgbd_ref_small_conv_nchw(a["x"], a["n"], a["cin"], a["h"], a["w"], a["wt"], a["b"], a["cout"], a["k"], a["stride"], a["pad"],
                                          a["act"], a["ckbd"], _host(kbn, i32p), 0 if kbn is None else len(kbn), None, None, None, a["y"],
                                          None, None)

    for kb in ([35], [37], [18, 17], [20, 17], [36, 0], [0, 36], [-1, 37], [2] * 17 + [2], [1] * 36):
        assert sc(kb) == EINVAL, kb
    for kw in [dict(k=4), dict(k=5), dict(k=0), dict(stride=3), dict(stride=0), dict(act=4), dict(act=-1), dict(ckbd=3), dict(ckbd=1, stride=2),
               dict(x=None), dict(wt=None), dict(y=None), dict(n=0), dict(cin=0), dict(cout=0), dict(h=0), dict(pad=-1), dict(h=1, w=1, pad=0)]:
        assert sc([36], **kw) == EINVAL, kw
    # deconv: recipes that do not parse to exactly 4 * w descriptors, too many taps / chains, taps off the kernel or of another phase
    case = next(c for c in rc.DECONV_CASES if c["id"] == "syn-1-32-48-3x5-drawn")
    wt5, b5 = np.zeros((32, 48, 5, 5), np.float32), np.zeros(48, np.float32)
    good = list(case["recipe"])

    def dc(rec, **kw):
        a = {**dict(x=p, n=1, cin=32, h=3, w=5, wt=_host(wt5), b=_host(b5), cout=48, act=0, y=p), **kw}
        r = None if rec is None else np.asarray(rec, np.int32)
        return L.rgbd_ref_deconv_s2_nchw(a["x"], a["n"], a["cin"], a["h"], a["w"], a["wt"], a["b"], a["cout"], a["act"], _host(r, i32p),
                                         0 if r is None else len(r), a["y"], None)

    last = len(good) - (1 + 3 * 4)  # the last descriptor: phase 3, 4 taps
    assert good[last] == 4
    seventeen = good[:last] + [17] + [1, 1, 1] * 17          # 17 taps (each its own chain)
    off_kernel = good[:last] + [4, 1, 5, 1] + good[last + 4:]  # kx = 5
    negative = good[:last] + [4, -1, 1, 1] + good[last + 4:]
    other_phase = good[:last] + [4, 0, 1, 1] + good[last + 4:]  # ky = 0 in phase py = 1
    bad_fresh = good[:last] + [4, 1, 1, 2] + good[last + 4:]
    for rec in (None, [], good[:-1], good + [0], good[:last], good + good[last:], seventeen, off_kernel, negative, other_phase, bad_fresh,
                [0] * 20, [-1] + good[1:], [2 ** 30] + good[1:]):
        assert dc(rec) == EINVAL, rec if rec is None else len(rec)
    for kw in [dict(x=None), dict(wt=None), dict(y=None), dict(n=0), dict(cin=0), dict(cout=0), dict(h=0), dict(w=0), dict(act=3), dict(act=-1),
               dict(w=4), dict(w=6)]:
        assert dc(good, **kw) == EINVAL, kw
    assert float(buf.abs().max()) == 0.0  # nothing was written
