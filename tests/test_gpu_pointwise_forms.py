"""The single-chain pointwise kernels and the two layout kernels of csrc/pointwise.hip alone, through the rgbd_pw_* hooks
(include/rgbd_amd.h), on the engine's own NHWC layout with the caller's strides: nothing is staged through the layout kernels,
so pads, neighbours and guard bands are this test's to fill and to inspect.  Cases, references and acceptance functions are
tests/pointwise_forms_cases.py's (checked on the CPU by tests/test_pointwise_forms_cases.py).

Every call is issued twice into fresh destinations and must give the same bits; every destination is followed by a guard band
of one row of a sentinel that must survive.

Largest share of the derived float64 bound used on MI355X (measured against the float64 statement; the bounds are meant to
have room, a share above 0.5 would be called out -- none is):
  channel mean   0.498 at HW = 3 (0.43 at HW = 4 / 5, 0.26 ... 0.14 at HW = 28 ... 65, 0.07 at HW = 259): where the bound
                 counts only 4 roundings the kernel's 2 ... 3 come close to half of it.  Bit for bit the float32 restatement
                 of the documented order on every case: the comment above channel_mean_kernel and the kernel agree.
  SE gate        0.182 (C = 16); 0.027 at C = 48, below 0.002 from C = 1280 on (the worst-case dot-product terms grow with C)
  bilinear       0.233 (1x9 -> 4x30); 0.11 ... 0.20 elsewhere, 0 for the identity
"""
import ctypes

import numpy as np
import pytest
import torch

import gridcap_cases as gc
import pointwise_forms_cases as pc
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

EINVAL = -22
F32P = ctypes.POINTER(ctypes.c_float)


def _lib():
    require_gpu()
    from rgbd_amd import _lib as lib

    return lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _host(a):
    a = np.ascontiguousarray(a, np.float32)
    return a, a.ctypes.data_as(F32P)


def _twice(n, guard, launch):
    """launch(dst_ptr) -> rc, into two fresh destinations of n floats, each followed by `guard` floats of the sentinel: both
    calls succeed, leave the guard alone and give the same bits.  -> the n floats."""
    outs = []
    for _ in range(2):
        dst = torch.full((n + guard,), pc.SENTINEL, device="cuda")
        assert launch(dst.data_ptr()) == 0
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        assert (got[n:] == pc.SENTINEL).all(), "the guard band behind the destination was written"
        outs.append(got[:n])
    assert pc.same_bits(outs[0], outs[1]), "two calls, different bits"
    return outs[0]


# ---- channel means ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", pc.MEAN_HW)
def test_channel_mean_order_and_bound(HW):
    """Bit for bit the float32 restatement of the documented order, and inside gamma(ceil(HW / 4) + 3) * sum|x| / HW of the
    float64 mean; the floats of the mean buffer outside [n * mstride, n * mstride + C) keep the pre-fill."""
    L = _lib()
    worst = 0.0
    for C in pc.MEAN_C:
        cs = pc.mean_cs(C)
        for N in pc.MEAN_N:
            x = pc.mean_input(N, HW, C, cs)
            xd = _dev(x)
            for ms in pc.mean_mstrides(C):
                buf = _twice(N * ms, ms, lambda p: L.rgbd_pw_channel_mean(xd.data_ptr(), N, HW, cs, C, p, ms, _stream()))
                ok, sh, bad = pc.accept_mean(buf, x, C, ms)
                worst = max(worst, sh)
                assert ok, (C, N, ms, sh, bad)
    print(f"channel mean HW {HW}: largest share of the float64 bound {worst:.3f}; float32 restatement: equal bits")


# ---- SE gate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perm", [0, 1])
@pytest.mark.parametrize("C,N,mstride", pc.SE_CASES)
def test_se_gate_vs_f64(C, N, mstride, perm):
    """sigmoid(W1 . relu(W0 . mean)) against float64 under the bound derived in pointwise_forms_cases.se_bound; NaN in the
    pads of the mean buffer (mstride > C)."""
    L = _lib()
    buf, w0, w1, m = pc.se_input(C, N, mstride, perm)
    pc.se_check_spread(C, N, m, w0, w1)
    md = _dev(buf)
    (k0, p0), (k1, p1) = _host(w0), _host(w1)
    vec = _twice(N * C, C, lambda p: L.rgbd_pw_se_gate(md.data_ptr(), N, C, p0, p1, mstride, perm, p, _stream())).reshape(N, C)
    ok, sh = pc.accept_se(vec, m, w0, w1, perm)
    print(f"se gate C {C} N {N} mstride {mstride} perm {perm}: share of the bound {sh:.3f}")
    assert ok, sh
    # each mistake of the CPU-side list, applied to the float64 statement, lands far from what the kernels returned
    for mut in pc.SE_MISTAKES:
        if (mut == "mstride_as_c" and (N == 1 or mstride == C)) or (mut == "perm_ignored" and not perm) or C < 48:
            continue
        wrong = pc.se_gate_vec(np.nan_to_num(buf, nan=7.0), C, w0, w1, perm, mut)
        assert pc.share(pc.se_logical(vec, perm), pc.se_logical(wrong, perm), pc.se_bound(m, w0, w1)) >= 100, mut


# ---- bilinear, single-chain ------------------------------------------------------------------------------------------------
def _bilinear(L, xd, N, h, w, cs, H, W, x1d=None, ref=0):
    n = N * H * W * cs
    if x1d is None:
        return _twice(n, W * cs, lambda p: L.rgbd_pw_bilinear(xd.data_ptr(), N, h, w, cs, p, H, W, None, None, ref, _stream()))
    # a pair: the second destination in the same allocation, behind the first one's guard band
    gap = n + W * cs

    def pair(p):
        return L.rgbd_pw_bilinear(xd.data_ptr(), N, h, w, cs, p, H, W, x1d.data_ptr(), p + 4 * gap, ref, _stream())

    both = _twice(gap + n, W * cs, pair)
    assert (both[n:gap] == pc.SENTINEL).all(), "the guard band between the two destinations was written"
    return both[:n], both[gap:]


@pytest.mark.parametrize("h,w,H,W", pc.BILINEAR_SHAPES)
def test_bilinear_single_chain_vs_f64(h, w, H, W):
    """ref_channels = 0 against the float64 formula under gamma(9) max|x| + gamma(3) (h Dy + w Dx)."""
    L = _lib()
    worst = 0.0
    for C, cs in pc.BILINEAR_C:
        for N in pc.BILINEAR_N:
            x = pc.bilinear_input(N, h, w, cs)
            out = _bilinear(L, _dev(x), N, h, w, cs, H, W).reshape(N, H, W, cs)
            ok, sh = pc.accept_bilinear(out, x)
            worst = max(worst, sh)
            assert ok, (C, N, sh)
            if (h, w) == (H, W):
                assert pc.same_bits(out, x)  # the identity is exact
            if (h, w, H, W) in pc.BILINEAR_SENSITIVITY:
                for mut in pc.BILINEAR_MISTAKES:
                    assert pc.share(out, pc.bilinear(x, H, W, mut=mut), pc.bilinear_bound(x)) >= 100, mut
    print(f"bilinear {h}x{w} -> {H}x{W}: largest share of the bound {worst:.3f}")


# ---- pair launches ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,C,cs", pc.PAIR_SHAPES)
def test_pair_launches_give_each_sets_own_bits(N, H, W, C, cs):
    """blockIdx.y == 1 of bilinear_kernel and maxpool7s3_kernel: each operand set of a pair launch carries the bits of its own
    single launch (the two inputs differ); max pool equals F.max_pool2d (restated in numpy, pinned to torch on the CPU)."""
    L = _lib()
    xa, xb = pc.bilinear_input(N, H, W, cs, key=1), pc.bilinear_input(N, H, W, cs, key=2)
    assert not np.array_equal(xa, xb)
    da, db = _dev(xa), _dev(xb)
    OH, OW = pc.pair_out_hw(H, W)
    sa, sb = _bilinear(L, da, N, H, W, cs, OH, OW), _bilinear(L, db, N, H, W, cs, OH, OW)
    pa, pb = _bilinear(L, da, N, H, W, cs, OH, OW, x1d=db)
    assert pc.same_bits(pa, sa) and pc.same_bits(pb, sb) and not pc.same_bits(sa, sb)
    for out, x in ((pa, xa), (pb, xb)):
        assert pc.accept_bilinear(out.reshape(N, OH, OW, cs), x)[0]

    PH, PW = (H - 7) // 3 + 1, (W - 7) // 3 + 1
    n = N * PH * PW * cs
    gap = n + PW * cs
    ma = _twice(n, PW * cs, lambda p: L.rgbd_pw_maxpool7s3(da.data_ptr(), N, H, W, cs, p, None, None, _stream()))
    mb = _twice(n, PW * cs, lambda p: L.rgbd_pw_maxpool7s3(db.data_ptr(), N, H, W, cs, p, None, None, _stream()))
    both = _twice(gap + n, PW * cs,
                  lambda p: L.rgbd_pw_maxpool7s3(da.data_ptr(), N, H, W, cs, p, db.data_ptr(), p + 4 * gap, _stream()))
    assert (both[n:gap] == pc.SENTINEL).all()
    assert pc.same_bits(both[:n], ma) and pc.same_bits(both[gap:], mb)
    assert pc.same_bits(ma.reshape(N, PH, PW, cs), pc.maxpool7s3(xa)) and pc.same_bits(mb.reshape(N, PH, PW, cs), pc.maxpool7s3(xb))


# ---- strided channel scale -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("HW", pc.CAT_HW)
def test_channel_scale_into_the_halves_of_a_wider_tensor(HW, mode):
    """The se_cat_to form: own (48 of 64) and other (32 of 32) into channels 0..47 / 48..79 of a destination of stride 96,
    under one gate vector of stride 80 per image -- the second launch with the gate pointer and the destination pointer offset
    by own's channels.  Exact; channels 80..95 and the guard keep the pre-fill; NaN in own's pads."""
    L = _lib()
    c = pc.CAT
    own, other, gate = pc.cat_input(HW)
    od, td, gd = _dev(own), _dev(other), _dev(gate)
    N, oc = c["N"], c["own_c"]

    def both(p):
        rc = L.rgbd_pw_channel_scale(od.data_ptr(), N, HW, c["own_cs"], oc, gd.data_ptr(), c["sstride"], mode, p, c["dst_cs"], _stream())
        return rc or L.rgbd_pw_channel_scale(td.data_ptr(), N, HW, c["other_cs"], c["other_c"], gd.data_ptr() + 4 * oc, c["sstride"],
                                             mode, p + 4 * oc, c["dst_cs"], _stream())

    dst = _twice(N * HW * c["dst_cs"], c["dst_cs"], both).reshape(N, HW, c["dst_cs"])
    want = pc.cat_ref(own, other, gate, mode)
    assert pc.exact(dst, want) == (True, 0)
    for mut in pc.SCALE_MISTAKES:
        if mut == "mode0_for_mode1" and mode == 0:
            continue
        assert not pc.exact(dst, pc.cat_ref(own, other, gate, mode, mut))[0], mut


@pytest.mark.parametrize("mode", [0, 1])
def test_channel_scale_plain_form(mode):
    """sstride == C, C = 20: a multiple of 4, not of 16."""
    L = _lib()
    p_ = pc.SCALE_PLAIN
    x, gate = pc.plain_scale_input()
    xd, gd = _dev(x), _dev(gate)
    dst = _twice(p_["N"] * p_["HW"] * p_["ycs"], p_["ycs"],
                 lambda p: L.rgbd_pw_channel_scale(xd.data_ptr(), p_["N"], p_["HW"], p_["xcs"], p_["C"], gd.data_ptr(), p_["C"], mode, p,
                                                   p_["ycs"], _stream()))
    assert pc.exact(dst.reshape(p_["N"], p_["HW"], p_["ycs"]), pc.plain_scale_ref(x, gate, mode)) == (True, 0)


# ---- copy_channels, fill_zero ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix,C,scs,dcs", pc.COPY_CASES)
def test_copy_channels_unequal_strides(npix, C, scs, dcs):
    L = _lib()
    src = pc.copy_input(npix, C, scs)
    sd = _dev(src)
    dst = _twice(npix * dcs, dcs, lambda p: L.rgbd_pw_copy_channels(sd.data_ptr(), scs, p, dcs, npix, C, _stream()))
    assert pc.same_bits(dst.reshape(npix, dcs), pc.copy_ref(src, C, dcs))  # the neighbours of the written channels included


@pytest.mark.parametrize("n", pc.FILL_N)
def test_fill_zero_inside_a_guarded_buffer(n):
    """n floats from an address that is 4-byte but not 16-byte aligned; the 3 floats in front and the guard behind survive."""
    L = _lib()
    lead = 3
    got = _twice(lead + n, 64, lambda p: L.rgbd_pw_fill_zero(p + 4 * lead, n, _stream()))
    assert (got[:lead] == pc.SENTINEL).all() and pc.same_bits(got[lead:], np.zeros(n, np.float32))


# ---- im2col5s2 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", pc.IM2COL_HW)
def test_im2col5s2_vs_gather(H, W):
    """Exact against the numpy gather written from the kernel's comment: taps outside the image and the padding terms are
    zeros over a non-zero pre-fill; NaN in the channels C .. cs - 1 of the image."""
    L = _lib()
    cs = pc.IM2COL_CS
    for C, KP in pc.IM2COL_CKP:
        for N in pc.IM2COL_N:
            x = pc.im2col_input(N, H, W, C)
            xd = _dev(x)
            OH, OW = (H + 1) // 2, (W + 1) // 2
            y = _twice(N * OH * OW * KP, OW * KP, lambda p: L.rgbd_pw_im2col5s2(xd.data_ptr(), N, H, W, cs, C, p, KP, _stream()))
            y = y.reshape(N, OH, OW, KP)
            assert pc.same_bits(y, pc.im2col5s2(x, C, KP)), (C, KP, N)
            if (H, W) != (1, 1):
                assert not pc.exact(y, pc.im2col5s2(x, C, KP, "kx_major"))[0]


def test_im2col5s2_refusals():
    L = _lib()
    x = _dev(pc.im2col_input(1, 9, 14, 3))
    y = torch.full((5 * 7 * 512 + 64,), pc.SENTINEL, device="cuda")
    for kw in pc.IM2COL_REFUSALS:
        a = dict(C=3, KP=80)
        a.update(kw)
        assert L.rgbd_pw_im2col5s2(x.data_ptr(), 1, 9, 14, pc.IM2COL_CS, a["C"], y.data_ptr(), a["KP"], _stream()) == EINVAL, kw
    torch.cuda.synchronize()
    assert (y == pc.SENTINEL).all()


# ---- layout kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perm", [0, 1])
@pytest.mark.parametrize("N,C,H,W,cs", pc.LAYOUT_CASES)
def test_layout_kernels_each_direction_alone(N, C, H, W, cs, perm):
    """nchw_to_nhwc16 and nhwc_to_nchw each against numpy -- a mistake that the pair undoes (a wrong permutation, a wrong pad
    handling) shows here -- and then as a pair on the device."""
    L = _lib()
    src = pc.layout_nchw_input(N, C, H, W)
    sd = _dev(src)
    npix = N * H * W
    nhwc = _twice(npix * cs, W * cs, lambda p: L.rgbd_pw_nchw_to_nhwc(sd.data_ptr(), N, C, H, W, p, cs, perm, _stream()))
    nhwc = nhwc.reshape(N, H, W, cs)
    assert pc.same_bits(nhwc, pc.to_nhwc(src, cs, perm))  # the positions that hold no channel: 0 over the non-zero pre-fill
    if perm and C > 1:
        assert not pc.exact(nhwc, pc.to_nhwc(src, cs, perm, "perm_ignored"))[0]
    for clamp01 in (0, 1):
        x = pc.layout_nhwc_input(N, C, H, W, cs, perm, clamp01)  # NaN where no channel sits
        xd = _dev(x)
        out = _twice(N * C * H * W, W, lambda p: L.rgbd_pw_nhwc_to_nchw(xd.data_ptr(), N, C, H, W, cs, p, clamp01, perm, _stream()))
        out = out.reshape(N, C, H, W)
        want = pc.to_nchw(x, C, perm, clamp01)
        assert pc.exact(out, want) == (True, 0)
        if not clamp01:
            assert pc.same_bits(out, want)
        if perm and C > 1:
            assert not pc.exact(out, pc.to_nchw(x, C, perm, clamp01, "perm_ignored"))[0]
    # the inverse pair round-trips on the device
    nd = _dev(nhwc)
    back = _twice(N * C * H * W, W, lambda p: L.rgbd_pw_nhwc_to_nchw(nd.data_ptr(), N, C, H, W, cs, p, 0, perm, _stream()))
    assert pc.same_bits(back.reshape(N, C, H, W), src)


# ---- past the grid cap -----------------------------------------------------------------------------------------------------
# grid_for() cuts every grid at 2048 blocks of 256: above 524 288 work items the kernels' grid-stride loops take a second sweep.
# Cases, owners and acceptance: tests/gridcap_cases.py (two sweeps, the second one ragged; copy and fill also three); the
# builders, references and rules are the ones of the tests above.  The whole allocation -- destination and guard band -- goes
# through the case's acceptance function; two calls must give the same bits.
def _whole_twice(n, launch):
    outs = []
    for _ in range(2):
        dst = torch.full((n,), pc.SENTINEL, device="cuda")
        assert launch(dst.data_ptr()) == 0
        torch.cuda.synchronize()
        outs.append(dst.cpu().numpy())
    assert pc.same_bits(outs[0], outs[1]), "two calls, different bits"
    return outs[0]


def _accepted(bc, got):
    for name, stage in bc["stages"].items():
        assert stage["accept"]({"dst": got}) == [], name


@pytest.mark.parametrize("case", gc.COPY_CASES, ids=lambda c: "%(npix)dx%(C)d" % c)
def test_copy_channels_past_the_grid_cap(case):
    L = _lib()
    bc = gc.build_copy(case)
    sd = _dev(bc["src"])
    npix, C, scs, dcs = (case[k] for k in ("npix", "C", "scs", "dcs"))
    _accepted(bc, _whole_twice(npix * dcs + bc["guard"], lambda p: L.rgbd_pw_copy_channels(sd.data_ptr(), scs, p, dcs, npix, C, _stream())))


@pytest.mark.parametrize("case", gc.FILL_CASES, ids=lambda c: "%(n)d" % c)
def test_fill_zero_past_the_grid_cap(case):
    L = _lib()
    n = case["n"]
    _accepted(gc.build_fill(case), _whole_twice(gc.FILL_LEAD + n + gc.FILL_GUARD, lambda p: L.rgbd_pw_fill_zero(p + 4 * gc.FILL_LEAD, n, _stream())))


@pytest.mark.parametrize("case", gc.SCALE_CASES, ids=lambda c: "hw%(HW)d-mode%(mode)d" % c)
def test_channel_scale_past_the_grid_cap(case):
    """the se_cat_to form of test_channel_scale_into_the_halves_of_a_wider_tensor: both launches cross the cap"""
    L = _lib()
    bc = gc.build_scale(case)
    c, HW, mode = pc.CAT, case["HW"], case["mode"]
    od, td, gd = _dev(bc["own"]), _dev(bc["other"]), _dev(bc["gate"])
    N, oc = c["N"], c["own_c"]

    def both(p):
        rc = L.rgbd_pw_channel_scale(od.data_ptr(), N, HW, c["own_cs"], oc, gd.data_ptr(), c["sstride"], mode, p, c["dst_cs"], _stream())
        return rc or L.rgbd_pw_channel_scale(td.data_ptr(), N, HW, c["other_cs"], c["other_c"], gd.data_ptr() + 4 * oc, c["sstride"],
                                             mode, p + 4 * oc, c["dst_cs"], _stream())

    _accepted(bc, _whole_twice(N * HW * c["dst_cs"] + bc["guard"], both))


@pytest.mark.parametrize("case", gc.BILINEAR_CASES, ids=lambda c: "%(h)dx%(w)d-%(H)dx%(W)d" % c)
def test_bilinear_past_the_grid_cap(case):
    L = _lib()
    bc = gc.build_bilinear(case)
    N, h, w, cs, H, W = (case[k] for k in ("N", "h", "w", "cs", "H", "W"))
    xd = _dev(bc["x"])
    _accepted(bc, _whole_twice(N * H * W * cs + bc["guard"],
                               lambda p: L.rgbd_pw_bilinear(xd.data_ptr(), N, h, w, cs, p, H, W, None, None, 0, _stream())))


@pytest.mark.parametrize("case", gc.MAXPOOL_CASES, ids=lambda c: "%(H)dx%(W)dx%(cs)d" % c)
def test_maxpool7s3_past_the_grid_cap(case):
    L = _lib()
    bc = gc.build_maxpool(case)
    N, H, W, cs = (case[k] for k in ("N", "H", "W", "cs"))
    xd = _dev(bc["x"])
    _accepted(bc, _whole_twice(bc["n"] + bc["guard"], lambda p: L.rgbd_pw_maxpool7s3(xd.data_ptr(), N, H, W, cs, p, None, None, _stream())))


@pytest.mark.parametrize("case", gc.IM2COL_CASES, ids=lambda c: "%(N)dx%(H)dx%(W)d-kp%(KP)d" % c)
def test_im2col5s2_past_the_grid_cap(case):
    L = _lib()
    bc = gc.build_im2col(case)
    N, H, W, C, KP = (case[k] for k in ("N", "H", "W", "C", "KP"))
    xd = _dev(bc["x"])
    _accepted(bc, _whole_twice(bc["n"] + bc["guard"], lambda p: L.rgbd_pw_im2col5s2(xd.data_ptr(), N, H, W, pc.IM2COL_CS, C, p, KP, _stream())))


@pytest.mark.parametrize("perm", [0, 1])
def test_layout_kernels_past_the_grid_cap(perm):
    """each direction at a shape of its own (the two work formulas differ), perm 0 and 1; clamp01 with perm 1"""
    L = _lib()
    case = gc.TO_NHWC_CASES[perm]
    bc = gc.build_to_nhwc(case)
    N, C, H, W, cs = (case[k] for k in ("N", "C", "H", "W", "cs"))
    sd = _dev(bc["src"])
    _accepted(bc, _whole_twice(bc["n"] + bc["guard"], lambda p: L.rgbd_pw_nchw_to_nhwc(sd.data_ptr(), N, C, H, W, p, cs, perm, _stream())))
    case = gc.TO_NCHW_CASES[perm]
    bc = gc.build_to_nchw(case)
    N, C, H, W, cs, clamp01 = (case[k] for k in ("N", "C", "H", "W", "cs", "clamp01"))
    xd = _dev(bc["x"])
    _accepted(bc, _whole_twice(bc["n"] + bc["guard"],
                               lambda p: L.rgbd_pw_nhwc_to_nchw(xd.data_ptr(), N, C, H, W, cs, p, clamp01, perm, _stream())))


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_hooks_reject_bad_arguments_and_write_nothing():
    """Every refusal of include/rgbd_amd.h returns -22 with real device buffers behind the pointers, and no destination is
    touched; a good call then succeeds."""
    L = _lib()
    n = 1 << 16
    x, x1 = torch.rand(n, device="cuda"), torch.rand(n, device="cuda")
    y, y1, v = (torch.full((n,), pc.SENTINEL, device="cuda") for _ in range(3))
    (k0, w0), (k1, w1) = _host(np.ones((3, 48))), _host(np.ones((48, 3)))
    got = pc.refusals(L, x.data_ptr(), y.data_ptr(), v.data_ptr(), x1.data_ptr(), y1.data_ptr(), w0, w1, _stream())
    assert [label for label, rc in got if rc != EINVAL] == []
    torch.cuda.synchronize()
    for t in (y, y1, v):
        assert (t == pc.SENTINEL).all()
    assert L.rgbd_pw_fill_zero(y.data_ptr(), 5, _stream()) == 0
    torch.cuda.synchronize()
    assert (y[:5] == 0).all() and (y[5:] == pc.SENTINEL).all()
