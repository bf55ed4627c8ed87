"""The Swin kernels of STF_united (csrc/swin.hip) one by one, each behind its operator boundary (include/rgbd_amd.h), against
a float64 statement of the published operation written out here:

  * WindowAttention with the cyclic shift (Swin Transformer, models/stf_united.py:48-114, 162-203): roll by -shift,
    4x4 windows, softmax((q * 16^-0.5) k^T + B[rel(i, j)] + mask) v with the -100 mask between the regions of the rolled
    frame, windows back, roll back;
  * PatchMerging's 2x2 gather and PixelShuffle(2): exact data movement;
  * LayerNorm at a token count above both grid caps (the grid-stride loops), single and paired launches.

The maps are non-square in both orientations, so H / W mix-ups that a square map hides show here; a sensitivity check
proves the attention tolerance cannot hide the usual mistakes."""
import pytest
import torch
import torch.nn.functional as F

from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

EINVAL = -22
SENTINEL = 12345.0
# max |gpu - f64| <= WA_TOL * max |v| at |S| ~ 30.  Observed on MI355X: worst 1.23e-6 over the 48 cases of
# test_window_attention_vs_f64 (max |S| 24 ... 43), 4.7e-6 at max |S| = 194; every mutation of the sensitivity check lands
# 2.2e4 ... 6.5e4 x WA_TOL away.
WA_TOL = 2e-5


def _lib():
    require_gpu()
    from rgbd_amd import _lib as lib

    return lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- float64 window attention ------------------------------------------------------------------------------------------
def _rel_index():
    """relative_position_index of a 4x4 window: [i, j] -> (dy + 3) * 7 + (dx + 3), d = coords(i) - coords(j)."""
    t = torch.arange(16)
    ty, tx = t // 4, t % 4
    return (ty[:, None] - ty[None, :] + 3) * 7 + (tx[:, None] - tx[None, :] + 3)


def _regions(n, lim, shift):
    """Region label along one axis of the rolled frame: [0, lim - 4), [lim - 4, lim - shift), [lim - shift, lim)."""
    c = torch.arange(n)
    return torch.where(c < lim - 4, 0, torch.where(c < lim - shift, 1, 2))


def wa_f64(qkv, rpb, heads, shift, mut=None):
    """qkv: [B, H, W, >= 3C] (channel which * C + head * 16 + d), rpb: [49, heads] -> out [B, H, W, C] in float64.
    mut: a deliberate mistake (the sensitivity check): "bias_t" transposed bias index, "mask_hw" H and W swapped in the mask
    regions, "nomask", "roll" roll direction reversed, "dim_major" channel d * heads + head, "scale" C^-0.5."""
    B, H, W, _ = qkv.shape
    C = 16 * heads
    x = qkv[..., :3 * C].double()
    s = shift if mut == "roll" else -shift
    if shift:
        x = torch.roll(x, (s, s), (1, 2))
    nwy, nwx = H // 4, W // 4
    win = x.reshape(B, nwy, 4, nwx, 4, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 16, 3 * C)
    if mut == "dim_major":
        t = win.reshape(-1, 16, 3, 16, heads).permute(2, 0, 4, 1, 3)
    else:
        t = win.reshape(-1, 16, 3, heads, 16).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]  # [windows, heads, token, d]
    scale = C ** -0.5 if mut == "scale" else 16 ** -0.5
    attn = (q * scale) @ k.transpose(-1, -2)
    idx = _rel_index()
    if mut == "bias_t":
        idx = idx.t()
    attn = attn + rpb.double()[idx].permute(2, 0, 1)
    if shift and mut != "nomask":
        hl, wl = (W, H) if mut == "mask_hw" else (H, W)
        lab = 3 * _regions(H, hl, shift)[:, None] + _regions(W, wl, shift)[None, :]
        mw = lab.reshape(nwy, 4, nwx, 4).permute(0, 2, 1, 3).reshape(-1, 16)
        mask = (mw[:, None, :] != mw[:, :, None]).double() * -100.0
        attn = (attn.view(B, nwy * nwx, heads, 16, 16) + mask[None, :, None]).view(-1, heads, 16, 16)
    o = torch.softmax(attn, -1) @ v  # [windows, heads, token, d]
    if mut == "dim_major":
        o = o.permute(0, 2, 3, 1)
    else:
        o = o.permute(0, 2, 1, 3)
    o = o.reshape(B, nwy, nwx, 4, 4, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    if shift:
        o = torch.roll(o, (-s, -s), (1, 2))
    return o


def _scores_max(qkv, rpb, heads):
    """max |(q * 0.25) k^T + bias| over the unshifted windows (how far the inputs drive the softmax)."""
    B, H, W, _ = qkv.shape
    C = 16 * heads
    win = qkv[..., :2 * C].double().reshape(B, H // 4, 4, W // 4, 4, 2 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 16, 2, heads, 16)
    q, k = win[:, :, 0].transpose(1, 2), win[:, :, 1].transpose(1, 2)
    return float(((q * 0.25) @ k.transpose(-1, -2) + rpb.double()[_rel_index()].permute(2, 0, 1)).abs().max())


def _wa_inputs(B, H, W, heads, qk_sigma, pad, seed):
    C = 16 * heads
    qcs, ocs = 3 * C + (16 if pad else 0), C + (16 if pad else 0)
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, H, W, qcs, generator=g)
    qkv[..., :2 * C] *= qk_sigma
    qkv[..., 3 * C:] = float("nan")  # a kernel that reads the pad channels turns its output into NaN
    rpb = torch.randn(49, heads, generator=g) * 2.0
    return qkv, rpb, qcs, ocs


def _wa_gpu(L, qkv, rpb, heads, shift, ocs, pair=None):
    B, H, W, qcs = qkv.shape
    C = 16 * heads
    q_d, r_d = qkv.cuda(), rpb.cuda()
    out = torch.full((B, H, W, ocs), SENTINEL, device="cuda")
    if pair is None:
        rc = L.rgbd_window_attention(q_d.data_ptr(), B, H, W, C, qcs, heads, shift, r_d.data_ptr(), out.data_ptr(), ocs,
                                     None, None, None, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        return out.cpu()
    q1, r1 = pair[0].cuda(), pair[1].cuda()
    out1 = torch.full((B, H, W, ocs), SENTINEL, device="cuda")
    rc = L.rgbd_window_attention(q_d.data_ptr(), B, H, W, C, qcs, heads, shift, r_d.data_ptr(), out.data_ptr(), ocs,
                                 q1.data_ptr(), r1.data_ptr(), out1.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu(), out1.cpu()


# (H, W, heads, shift): one window; non-square both ways; one window row / column; the deep stage (C = 384); shifts 1 and 3
WA_CASES = [(4, 4, 2, 0), (4, 4, 2, 2), (8, 12, 2, 0), (8, 12, 2, 2), (12, 8, 2, 0), (12, 8, 2, 2), (16, 20, 3, 0),
            (16, 20, 3, 2), (4, 36, 2, 0), (4, 36, 2, 2), (36, 4, 2, 0), (36, 4, 2, 2), (8, 12, 24, 0), (12, 8, 24, 2),
            (12, 8, 2, 1), (8, 12, 3, 3)]


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("H,W,heads,shift", WA_CASES)
def test_window_attention_vs_f64(H, W, heads, shift, B):
    """Scores up to |S| ~ 30 (the softmax far from uniform); at B == 2 with padded qkv / out channel strides whose pads hold
    a sentinel (NaN in qkv: a read of them would poison the result; out's must survive: attention leaves them untouched)."""
    L = _lib()
    pad = B == 2
    qkv, rpb, qcs, ocs = _wa_inputs(B, H, W, heads, 2.6, pad, seed=1000 * H + 10 * W + heads + 7 * shift + 100000 * B)
    smax = _scores_max(qkv, rpb, heads)
    assert 15 < smax < 80, smax
    out = _wa_gpu(L, qkv, rpb, heads, shift, ocs)
    C = 16 * heads
    ref = wa_f64(qkv, rpb, heads, shift)
    vmax = float(qkv[..., 2 * C:3 * C].abs().max())
    err = float((out[..., :C].double() - ref).abs().max())
    print(f"window attention {B}x{H}x{W} heads {heads} shift {shift}: max|S| {smax:.1f}, err / max|v| {err / vmax:.2e}")
    assert err <= WA_TOL * vmax, (err / vmax, WA_TOL)
    if ocs > C:
        assert (out[..., C:] == SENTINEL).all()


def test_window_attention_large_scores_and_grid():
    """|S| > 100, where the -100 mask no longer dominates (the reference adds -100 too: the results must still agree), on a
    map of 23 040 (window, head) pairs (1 440 workgroups)."""
    L = _lib()
    B, H, W, heads, shift = 3, 64, 80, 24, 2
    qkv, rpb, qcs, ocs = _wa_inputs(B, H, W, heads, 5.5, False, seed=77)
    assert B * (H // 4) * (W // 4) * heads >= 20000
    smax = _scores_max(qkv, rpb, heads)
    assert smax > 100, smax
    out = _wa_gpu(L, qkv, rpb, heads, shift, ocs)
    C = 16 * heads
    ref = wa_f64(qkv, rpb, heads, shift)
    vmax = float(qkv[..., 2 * C:].abs().max())
    err = float((out.double() - ref).abs().max())
    # fp32 scores carry an absolute error of a few ulp(|S|): the bound scales with max|S| / 30 past the |S| ~ 30 cases
    tol = WA_TOL * max(1.0, smax / 30.0)
    print(f"window attention large: max|S| {smax:.1f}, err / max|v| {err / vmax:.2e} (tolerance {tol:.2e})")
    assert err <= tol * vmax, (err / vmax, tol)


MUTATIONS = ["bias_t", "mask_hw", "nomask", "roll", "dim_major", "scale"]


@pytest.mark.parametrize("B,H,W,heads,shift", [(2, 12, 8, 3, 2), (1, 8, 20, 2, 1)])
def test_window_attention_tolerance_is_sensitive(B, H, W, heads, shift):
    """Each classic mistake, applied to the float64 statement, lands at least 100x the tolerance away from the GPU's result
    on the same inputs: the tolerance cannot hide any of them."""
    L = _lib()
    qkv, rpb, qcs, ocs = _wa_inputs(B, H, W, heads, 2.6, False, seed=4242 + H)
    out = _wa_gpu(L, qkv, rpb, heads, shift, ocs).double()
    C = 16 * heads
    tol = WA_TOL * float(qkv[..., 2 * C:].abs().max())
    assert float((out - wa_f64(qkv, rpb, heads, shift)).abs().max()) <= tol
    margins = {m: float((out - wa_f64(qkv, rpb, heads, shift, m)).abs().max()) / tol for m in MUTATIONS}
    print(f"sensitivity {B}x{H}x{W} heads {heads} shift {shift}:", {m: round(v) for m, v in margins.items()})
    assert min(margins.values()) >= 100, margins


@pytest.mark.parametrize("B,H,W,heads,shift", [(2, 12, 8, 3, 2), (1, 16, 20, 2, 0), (3, 8, 12, 24, 2)])
def test_window_attention_pair_launch_same_bits(B, H, W, heads, shift):
    """The paired launch (blockIdx.y == 1: the other modality, its own qkv and bias table) gives, for each set, the bits of a
    single launch of that set."""
    L = _lib()
    qa, ra, qcs, ocs = _wa_inputs(B, H, W, heads, 2.6, True, seed=11)
    qb, rb, _, _ = _wa_inputs(B, H, W, heads, 2.6, True, seed=12)
    pa, pb = _wa_gpu(L, qa, ra, heads, shift, ocs, pair=(qb, rb))
    sa, sb = _wa_gpu(L, qa, ra, heads, shift, ocs), _wa_gpu(L, qb, rb, heads, shift, ocs)
    assert torch.equal(pa.view(torch.int32), sa.view(torch.int32)) and torch.equal(pb.view(torch.int32), sb.view(torch.int32))
    assert not torch.equal(pa, pb)


def test_window_attention_rejects_bad_arguments():
    """Every assumption of the kernel is checked at the boundary: RGBD_EINVAL and nothing written."""
    L = _lib()
    heads, C = 2, 32
    q = torch.randn(1, 8, 12, 3 * C + 16, device="cuda")
    rpb = torch.randn(49, heads, device="cuda")
    out = torch.full((1, 8, 12, C + 16), SENTINEL, device="cuda")

    def call(H=8, W=12, C_=C, qcs=3 * C + 16, heads_=heads, shift=2, ocs=C + 16, qptr=None, pair=(None, None, None)):
        return L.rgbd_window_attention(q.data_ptr() if qptr is None else qptr, 1, H, W, C_, qcs, heads_, shift, rpb.data_ptr(),
                                       out.data_ptr(), ocs, *pair, _stream())

    bad = [dict(H=6), dict(W=10), dict(C_=48), dict(heads_=3), dict(shift=-1), dict(shift=4), dict(qcs=3 * C - 4),
           dict(qcs=3 * C + 2), dict(ocs=C - 1), dict(qptr=q.data_ptr() + 4), dict(pair=(q.data_ptr() + 4, rpb.data_ptr(), out.data_ptr())),
           dict(pair=(q.data_ptr(), None, out.data_ptr()))]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (out[..., :C] == SENTINEL).any()


# ---- patch merging / pixel shuffle: exact -------------------------------------------------------------------------------
def _padded(B, H, W, C, cs, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, cs, generator=g)
    x[..., C:] = float("nan")
    return x


@pytest.mark.parametrize("B,H,W,C,xcs,ycs", [(2, 12, 20, 48, 64, 208), (2, 20, 12, 96, 96, 384), (1, 2, 2, 4, 4, 16),
                                             (2, 160, 192, 192, 192, 784)])
def test_patch_merge_gather_exact(B, H, W, C, xcs, ycs):
    """PatchMerging's gather == cat(x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2]) on the channels, bit for bit;
    the last case moves 2.9 M float4s, past the 8192 x 256 grid cap (the grid-stride loop).  y's pad channels are left as
    they were."""
    L = _lib()
    x = _padded(B, H, W, C, xcs, seed=H * W + C)
    xd = x.cuda()
    y = torch.full((B, H // 2, W // 2, ycs), SENTINEL, device="cuda")
    assert L.rgbd_patch_merge_gather(xd.data_ptr(), B, H, W, C, xcs, y.data_ptr(), ycs, _stream()) == 0
    torch.cuda.synchronize()
    y = y.cpu()
    xc = x[..., :C]
    ref = torch.cat([xc[:, 0::2, 0::2], xc[:, 1::2, 0::2], xc[:, 0::2, 1::2], xc[:, 1::2, 1::2]], -1)
    assert torch.equal(y[..., :4 * C], ref)
    assert (y[..., 4 * C:] == SENTINEL).all()


@pytest.mark.parametrize("B,H,W,Co,xcs,ycs", [(2, 6, 10, 48, 192, 64), (2, 10, 6, 3, 16, 16), (1, 1, 1, 1, 4, 4),
                                              (2, 64, 96, 48, 208, 64)])
def test_pixel_shuffle2_exact(B, H, W, Co, xcs, ycs):
    """== F.pixel_shuffle(x, 2) (NCHW) bit for bit; pad channels Co .. ycs - 1 of y zeroed; the last case writes 3.1 M
    elements, past the 8192 x 256 grid cap."""
    L = _lib()
    x = _padded(B, H, W, 4 * Co, xcs, seed=H * W + Co)
    xd = x.cuda()
    y = torch.full((B, 2 * H, 2 * W, ycs), SENTINEL, device="cuda")
    assert L.rgbd_pixel_shuffle2(xd.data_ptr(), B, H, W, Co, xcs, y.data_ptr(), ycs, _stream()) == 0
    torch.cuda.synchronize()
    y = y.cpu()
    ref = F.pixel_shuffle(x[..., :4 * Co].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(y[..., :Co], ref)
    assert (y[..., Co:] == 0).all()


def test_gather_and_shuffle_reject_bad_arguments():
    L = _lib()
    x = torch.randn(2, 8, 12, 64, device="cuda")
    y = torch.full((2 * 8 * 12 * 64 * 4,), SENTINEL, device="cuda")
    s = _stream()
    pm = L.rgbd_patch_merge_gather
    for args in [(x.data_ptr(), 2, 7, 12, 16, 64, y.data_ptr(), 64), (x.data_ptr(), 2, 8, 11, 16, 64, y.data_ptr(), 64),
                 (x.data_ptr(), 2, 8, 12, 18, 64, y.data_ptr(), 72), (x.data_ptr(), 2, 8, 12, 16, 64, y.data_ptr(), 60),
                 (x.data_ptr(), 2, 8, 12, 16, 62, y.data_ptr(), 64), (x.data_ptr() + 4, 2, 8, 12, 16, 64, y.data_ptr(), 64),
                 (x.data_ptr(), 2, 8, 12, 16, 64, y.data_ptr() + 4, 64), (x.data_ptr(), 2, 8, 12, 16, 12, y.data_ptr(), 64)]:
        assert pm(*args, s) == EINVAL, args
    ps = L.rgbd_pixel_shuffle2
    for args in [(x.data_ptr(), 2, 8, 12, 16, 60, y.data_ptr(), 16), (x.data_ptr(), 2, 8, 12, 16, 64, y.data_ptr(), 15),
                 (x.data_ptr(), 0, 8, 12, 16, 64, y.data_ptr(), 16), (None, 2, 8, 12, 16, 64, y.data_ptr(), 16)]:
        assert ps(*args, s) == EINVAL, args
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()


# ---- LayerNorm above the grid caps --------------------------------------------------------------------------------------
def _ln_inputs(ntok, C, xcs, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(ntok, xcs, generator=g) * 3 + torch.randn(ntok, 1, generator=g) * 5
    return x, torch.randn(C, generator=g), torch.randn(C, generator=g)


@pytest.mark.parametrize("C,xcs,ycs", [(48, 64, 64), (192, 192, 192)])
def test_layernorm_grid_stride_forms_and_pair(C, xcs, ycs):
    """300 001 tokens: more than one sweep of both grids (4096 x 4 tokens one wave per token, 8192 x 16 sixteen lanes per
    token), single and paired (blockIdx.y == 1) launches.  Both forms and both entries give the same bits; within the
    float64 bound of test_gpu_stf.py::test_layernorm_forms_same_bits; pad channels zeroed."""
    L = _lib()
    ntok = 300001
    assert ntok > 4096 * 4 and ntok > 8192 * 16
    sets = [_ln_inputs(ntok, C, xcs, seed) for seed in (C, C + 1)]
    dev = [(x.cuda(), w.cuda(), b.cuda()) for x, w, b in sets]
    base = None  # form 0, single launches: every other form / entry must give these bits
    try:
        for form in (0, 1):
            L.rgbd_debug_force_layernorm_form(form)
            ys = []
            for xd, wd, bd in dev:
                y = torch.full((ntok, ycs), SENTINEL, device="cuda")
                assert L.rgbd_layernorm(xd.data_ptr(), ntok, C, xcs, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), ycs, _stream()) == 0
                ys.append(y)
            pair = [torch.full((ntok, ycs), SENTINEL, device="cuda") for _ in range(2)]
            (x0, w0, b0), (x1, w1, b1) = dev
            assert L.rgbd_layernorm2(x0.data_ptr(), ntok, C, xcs, w0.data_ptr(), b0.data_ptr(), pair[0].data_ptr(), ycs,
                                     x1.data_ptr(), w1.data_ptr(), b1.data_ptr(), pair[1].data_ptr(), _stream()) == 0
            torch.cuda.synchronize()
            if base is None:
                base = ys
            for k in range(2):
                assert torch.equal(ys[k].view(torch.int32), base[k].view(torch.int32)), (form, "single", k)
                assert torch.equal(pair[k].view(torch.int32), base[k].view(torch.int32)), (form, "pair", k)
    finally:
        L.rgbd_debug_force_layernorm_form(-1)
    for k, (x, w, b) in enumerate(sets):
        y = base[k].cpu()
        assert (y[:, C:] == 0).all()
        ref = F.layer_norm(x[:, :C].double(), (C,), w.double(), b.double(), 1e-5)
        err = float((y[:, :C].double() - ref).abs().max())
        print(f"layernorm C {C} set {k}: err / max|ref| {err / float(ref.abs().max()):.2e}")
        assert err <= 2e-5 * float(ref.abs().max())


def test_layernorm2_rejects_bad_arguments():
    L = _lib()
    x = torch.randn(64, 48, device="cuda")
    w, b = torch.randn(48, device="cuda"), torch.randn(48, device="cuda")
    y = torch.full((64, 48), SENTINEL, device="cuda")
    p = (x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr())
    ln2 = L.rgbd_layernorm2
    assert ln2(p[0], 64, 48, 48, p[1], p[2], p[3], 48, None, p[1], p[2], p[3], _stream()) == EINVAL
    assert ln2(p[0], 64, 48, 40, p[1], p[2], p[3], 48, p[0], p[1], p[2], p[3], _stream()) == EINVAL
    assert ln2(p[0], 0, 48, 48, p[1], p[2], p[3], 48, p[0], p[1], p[2], p[3], _stream()) == EINVAL
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()
