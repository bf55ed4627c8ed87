"""The references and acceptance functions of tests/pointwise_forms_cases.py, checked on the CPU: every float64 statement
equals torch's own operator in float64 where torch has one; a plain float32 evaluation passes each tolerance-based acceptance
function using at most a quarter of its bound (the channel mean's tight small-HW bounds excepted, see there); every deliberate mistake, applied to the reference, is rejected -- the
tolerance-based operators by a wide multiple of the bound, the exact ones in at least one element.

Multiples of the bound the mistakes reach (smallest over the cases each is run on):
  channel mean   drop_last 1.4e3 (HW 259) ... 1.0e6 (HW 5), div_hw1 9.5e2 ... 5.6e5; swap_chains stays inside the float64 bound
                 (0.06 ... 0.44 of it: another valid order) and is caught by the bit-exact part in 37 ... 62 of 240 elements;
                 mstride_as_c moves every element
  SE gate        perm_ignored 1.6e3 (C 2432) ... 2.2e5 (C 48), no_relu 1.4e3 ... 1.0e5, w1_not_transposed 1.7e3 ... 2.5e5,
                 mstride_as_c 2.5e5
  bilinear       align_corners 3.2e4, clamp_in_2 8.9e4
  exact operators (scale, copy, im2col5s2, layout): every mistake changes at least one element
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_forms_cases as pc

F64 = np.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- channel means ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", pc.MEAN_HW)
def test_mean_statement_restatement_and_bound(HW):
    for C in pc.MEAN_C:
        for N in pc.MEAN_N:
            x = pc.mean_input(N, HW, C, pc.mean_cs(C))
            ref = pc.mean_f64(x, C)
            assert np.abs(ref - _t(x[..., :C]).double().mean(dim=1).numpy()).max() <= 1e-14
            for ms in pc.mean_mstrides(C):
                ok, sh, bad = pc.accept_mean(pc.mean_place(pc.mean_f32_order(x, C), ms), x, C, ms)
                assert ok and bad == 0 and sh <= 1.0
            # a plain float32 evaluation (numpy's pairwise sum) passes.  It uses a quarter of the bound at most where the bound
            # counts many roundings (HW = 259: 68); at the smaller sizes the bound counts 4 ... 20, and the last few adds of any
            # summation work on sums of all-positive terms near their full size, each rounding up to its full half ulp: there
            # the evaluation reaches 0.3 ... 0.5 of the bound, and only the bound itself is asked for
            plain = (x[..., :C].sum(axis=1, dtype=np.float32) / np.float32(HW)).astype(np.float32)
            assert pc.share(plain, ref, pc.mean_bound(x, C)) <= (0.25 if HW >= 259 else 1.0)


@pytest.mark.parametrize("HW", [5, 33, 65, 259])
def test_mean_mistakes_fail(HW):
    C, N = 80, 3
    ms = C + 48
    x = pc.mean_input(N, HW, C, pc.mean_cs(C), pad=7.0)
    for mut in pc.MEAN_MISTAKES:
        vals = pc.mean_f32_order(x, C, None if mut == "mstride_as_c" else mut)
        ok, sh, bad = pc.accept_mean(pc.mean_place(vals, ms, mut), x, C, ms)
        assert not ok and bad >= 1, (mut, sh, bad)
        if mut in ("drop_last", "div_hw1"):
            assert sh >= 100, (mut, sh)
        print(f"mean HW {HW} {mut}: share {sh:.3g}, {bad} elements")
    assert not pc.accept_mean(np.full(N * ms, np.nan, np.float32), x, C, ms)[0]


# ---- SE gate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perm", [0, 1])
@pytest.mark.parametrize("C,N,mstride", pc.SE_CASES)
def test_se_statement_spread_and_fp32(C, N, mstride, perm):
    buf, w0, w1, m = pc.se_input(C, N, mstride, perm)
    pc.se_check_spread(C, N, m, w0, w1)
    ref = pc.se_f64(m, w0, w1)[0]
    tm, t0, t1 = _t(m).double(), _t(w0).double(), _t(w1).double()
    assert np.abs(ref - torch.sigmoid(F.linear(F.relu(F.linear(tm, t0)), t1)).numpy()).max() <= 1e-14
    # the vector by position is the statement put through the permutation rule, and back
    vec = pc.se_gate_vec(buf, C, w0, w1, perm)
    assert np.abs(pc.se_logical(vec, perm) - ref).max() <= 1e-14
    if perm:
        near = lambda a, b: abs(a - b) <= 1e-14  # noqa: E731
        assert near(vec[0, 4], ref[0, 1]) and near(vec[0, 1], ref[0, 4]) and (C < 32 or near(vec[0, 16 + 9], ref[0, 16 + 6]))
    ok, sh = pc.accept_se(pc.se_gate_vec(buf, C, w0, w1, perm, dtype=np.float32), m, w0, w1, perm)
    assert ok and sh <= 0.25, sh
    assert not pc.accept_se(np.full((N, C), np.nan, np.float32), m, w0, w1, perm)[0]


@pytest.mark.parametrize("C,N,mstride", [c for c in pc.SE_CASES if c[0] >= 48])
def test_se_mistakes_fail(C, N, mstride):
    buf, w0, w1, m = pc.se_input(C, N, mstride, 1, pad=7.0)
    for mut in pc.SE_MISTAKES:
        if mut == "mstride_as_c" and (N == 1 or mstride == C):
            continue  # (not a mistake on this case)
        ok, sh = pc.accept_se(pc.se_gate_vec(buf, C, w0, w1, 1, mut), m, w0, w1, 1)
        assert not ok and sh >= 100, (mut, sh)
        print(f"se C {C} {mut}: share {sh:.3g}")


# ---- bilinear --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,H,W", pc.BILINEAR_SHAPES)
def test_bilinear_statement_and_fp32(h, w, H, W):
    for C, cs in pc.BILINEAR_C:
        for N in pc.BILINEAR_N:
            x = pc.bilinear_input(N, h, w, cs)
            ref = pc.bilinear(x, H, W)
            tor = F.interpolate(_t(x).double().permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
            assert np.abs(ref - tor.permute(0, 2, 3, 1).numpy()).max() <= 1e-14
            ok, sh = pc.accept_bilinear(pc.bilinear(x, H, W, dtype=np.float32), x)
            assert ok and sh <= 0.25, sh
    if (h, w) == (H, W):
        assert np.array_equal(ref, x.astype(F64))  # the identity is exact


@pytest.mark.parametrize("h,w,H,W", pc.BILINEAR_SENSITIVITY)
def test_bilinear_mistakes_fail(h, w, H, W):
    x = pc.bilinear_input(2, h, w, 20)
    for mut in pc.BILINEAR_MISTAKES:
        ok, sh = pc.accept_bilinear(pc.bilinear(x, H, W, mut=mut), x)
        assert not ok and sh >= 100, (mut, sh)
        print(f"bilinear {h}x{w}->{H}x{W} {mut}: share {sh:.3g}")
    assert not pc.accept_bilinear(np.full((2, H, W, 20), np.nan, np.float32), x)[0]


# ---- max pool --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,C,cs", pc.PAIR_SHAPES)
def test_maxpool_equals_torch(N, H, W, C, cs):
    x = pc.bilinear_input(N, H, W, cs)
    tor = F.max_pool2d(_t(x).permute(0, 3, 1, 2), kernel_size=7, stride=3).permute(0, 2, 3, 1).numpy()
    assert pc.exact(pc.maxpool7s3(x), tor) == (True, 0)


# ---- strided channel scale, copy -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", pc.CAT_HW)
def test_scale_reference_and_mistakes(HW):
    own, other, gate = pc.cat_input(HW)
    oc, tc = pc.CAT["own_c"], pc.CAT["other_c"]
    for mode in (0, 1):
        ref = pc.cat_ref(own, other, gate, mode)
        cat = torch.cat([_t(own[..., :oc]), _t(other[..., :tc])], dim=-1)
        s = _t(gate)[:, None, :]
        tor = cat + cat * s if mode else cat * s  # (torch's CPU float32 ops round each step: two roundings in mode 1)
        assert pc.exact(ref[..., :oc + tc], tor.numpy()) == (True, 0)
        assert (ref[..., oc + tc:] == pc.SENTINEL).all()
        ok, bad = pc.exact(pc.cat_ref(own, other, gate, mode, "gate_offset_ignored"), ref)
        assert not ok and bad >= 1
    assert not pc.exact(pc.cat_ref(own, other, gate, 1, "mode0_for_mode1"), pc.cat_ref(own, other, gate, 1))[0]


def test_plain_scale_and_copy_references():
    x, gate = pc.plain_scale_input()
    C = pc.SCALE_PLAIN["C"]
    for mode in (0, 1):
        ref = pc.plain_scale_ref(x, gate, mode)
        tx, ts = _t(x[..., :C]), _t(gate)[:, None, :]
        assert pc.exact(ref[..., :C], (tx + tx * ts if mode else tx * ts).numpy()) == (True, 0)
        assert (ref[..., C:] == pc.SENTINEL).all()
    for npix, C, scs, dcs in pc.COPY_CASES:
        src = pc.copy_input(npix, C, scs)
        ref = pc.copy_ref(src, C, dcs)
        assert pc.same_bits(ref[:, :C], src[:, :C]) and (ref[:, C:] == pc.SENTINEL).all()


# ---- im2col5s2 -------------------------------------------------------------------------------------------------------------
def test_im2col_index_is_a_permutation_of_each_16():
    idx = [pc.im2col_index(t) for t in range(80)]
    assert sorted(idx) == list(range(80))
    assert idx[:8] == [0, 4, 8, 12, 1, 5, 9, 13]  # term = e * 4 + q -> q * 4 + e


@pytest.mark.parametrize("H,W", pc.IM2COL_HW)
def test_im2col_consequence_and_mistakes(H, W):
    """A float64 5x5 stride-2 pad-2 convolution of the image equals the float64 dot product of the gathered row with the
    weights in the same packed order."""
    for C, KP in pc.IM2COL_CKP:
        for N in pc.IM2COL_N:
            x = pc.im2col_input(N, H, W, C)
            rows = pc.im2col5s2(x, C, KP)
            assert rows.dtype == np.float32 and np.isfinite(rows).all()
            wt = pc.rng(10, C, KP).standard_normal((8, C, 5, 5))
            conv = F.conv2d(_t(x[..., :C]).double().permute(0, 3, 1, 2), _t(wt), stride=2, padding=2).permute(0, 2, 3, 1).numpy()
            dot = rows.astype(F64) @ pc.im2col_pack_weights(wt, KP).T
            assert conv.shape == dot.shape and np.abs(conv - dot).max() <= 1e-13
            assert (rows.reshape(-1, KP)[:, [pc.im2col_index(t) for t in range(25 * C, KP)]] == 0).all()
            for mut in pc.IM2COL_MISTAKES:
                ok, bad = pc.exact(pc.im2col5s2(x, C, KP, mut), rows)
                if mut == "kx_major" and H == 1 and W == 1:
                    continue  # (one pixel under the centre tap: both orders agree)
                if mut == "pad_not_zeroed" and 25 * C == KP:
                    continue
                assert not ok and bad >= 1, (mut, C, KP, N)


# ---- layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perm", [0, 1])
@pytest.mark.parametrize("N,C,H,W,cs", pc.LAYOUT_CASES)
def test_layout_references(N, C, H, W, cs, perm):
    src = pc.layout_nchw_input(N, C, H, W)
    nhwc = pc.to_nhwc(src, cs, perm)
    # written out with torch: pad the channel axis with zeros to cs, permute inside the groups of 16, channels last
    padded = F.pad(_t(src), (0, 0, 0, 0, 0, cs - C))
    if perm:
        padded = padded.view(N, cs // 16, 4, 4, H, W).transpose(2, 3).reshape(N, cs, H, W)
    assert pc.same_bits(nhwc, padded.permute(0, 2, 3, 1).numpy())
    assert pc.same_bits(pc.to_nchw(nhwc, C, perm, 0), src)  # the pair round-trips
    for mut in pc.LAYOUT_MISTAKES:
        if mut == "perm_ignored" and (not perm or C == 1):
            continue  # (channel 0 stays where it is)
        ok, bad = pc.exact(pc.to_nhwc(src, cs, perm, mut), nhwc)
        assert (not ok and bad >= 1) or (mut == "pad_not_zeroed" and cs == C), mut
    for clamp01 in (0, 1):
        x = pc.layout_nhwc_input(N, C, H, W, cs, perm, clamp01)
        out = pc.to_nchw(x, C, perm, clamp01)
        assert np.isfinite(out).all()
        body = _t(x).permute(0, 3, 1, 2)
        if perm:
            body = body.view(N, cs // 16, 4, 4, H, W).transpose(2, 3).reshape(N, cs, H, W)
        body = body[:, :C]
        assert pc.exact(out, (body.clamp(0, 1) if clamp01 else body).numpy()) == (True, 0)
        if clamp01:
            assert N * C * H * W < 8 or (out.min() == 0.0 and out.max() == 1.0 and ((out > 0) & (out < 1)).any())
        if perm and C > 1:
            assert not pc.exact(pc.to_nchw(x, C, perm, clamp01, "perm_ignored"), out)[0]


# ---- the hooks' refusals need no device --------------------------------------------------------------------------------------
def test_hooks_refuse_bad_arguments_before_any_device_call():
    import ctypes

    from rgbd_amd._lib import lib

    w = (ctypes.c_float * (48 * 3))()
    dev = 1 << 20  # (stands for 16-byte aligned device pointers: never dereferenced)
    got = pc.refusals(lib(), dev, 2 * dev, 3 * dev, 4 * dev, 5 * dev, w, w)
    assert len(got) > 100
    assert [label for label, rc in got if rc != -22] == []
