"""Guided (cross) window attention of Spatial_aligner (csrc/swin.hip: window_attention_kernel<32>): the cases, a float64
statement of the published operation written out here, and the acceptance function -- shared by the CPU test of this file's
own logic (test_guided_attention_cases.py) and the GPU test of the kernel (test_gpu_guided_attention.py).

The operation (Swin Transformer's shifted-window attention with the query from one map and key / value from another;
modules/transform/spatialAligner.py:138-170, 249-331): roll both maps by -shift, 4x4 windows, per head of 32 channels
softmax((q * 32^-0.5) k^T + B[rel(i, j)] + mask) v with the -100 mask between the regions of the rolled frame, windows back,
roll back.  q: [B, H, W, >= C], channel head * 32 + d; kv: [B, H, W, >= 2C], channel which * C + head * 32 + d (0 = k, 1 = v).
"""
import torch

HEAD_DIM = 32
WA_TOL = 2e-5  # max |out - f64| <= WA_TOL * max(1, max|S| / 30) * max|v|: the bound and scaling of tests/test_gpu_swin.py
QK_SIGMA = 2.4  # scores ~ N(0, QK_SIGMA^4): 15 < max |S| < 80 on every case (asserted)

# (H, W, heads, shift) of the token grid, each at B = 1, 2, 3: one window (the shifted frame wraps onto itself); non-square
# both ways; one window row / column with one head; the other shifts
CASES = [(4, 4, 3, 0), (4, 4, 3, 2), (8, 12, 3, 0), (8, 12, 3, 2), (12, 8, 3, 0), (12, 8, 3, 2), (4, 20, 1, 2), (20, 4, 1, 2),
         (12, 8, 3, 1), (8, 12, 3, 3)]
BATCHES = [1, 2, 3]
# a wavefront of the kernel walks several (window, head) pairs: 1920 pairs, 120 workgroups
SWEEP_CASE = (2, 64, 80, 3, 2)  # B, H, W, heads, shift
# B, H, W, heads, shift: non-square (a square map hides "mask_hw"), several heads (one head hides "dim_major")
SENSITIVITY_CASES = [(2, 12, 8, 3, 2), (1, 8, 20, 3, 1)]
MUTATIONS = ["bias_t", "mask_hw", "nomask", "roll", "dim_major", "scale16", "kv_swapped", "self_attn"]


def rel_index():
    """relative_position_index of a 4x4 window: [i, j] -> (dy + 3) * 7 + (dx + 3), d = coords(i) - coords(j)."""
    t = torch.arange(16)
    ty, tx = t // 4, t % 4
    return (ty[:, None] - ty[None, :] + 3) * 7 + (tx[:, None] - tx[None, :] + 3)


def regions(n, lim, shift):
    """Region label along one axis of the rolled frame: [0, lim - 4), [lim - 4, lim - shift), [lim - shift, lim)."""
    c = torch.arange(n)
    return torch.where(c < lim - 4, 0, torch.where(c < lim - shift, 1, 2))


def _windows(x, heads, dim_major):
    """[B, H, W, heads * 32] -> [windows, heads, token, d]"""
    B, H, W, C = x.shape
    win = x.reshape(B, H // 4, 4, W // 4, 4, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 16, C)
    if dim_major:
        return win.reshape(-1, 16, HEAD_DIM, heads).permute(0, 3, 1, 2)
    return win.reshape(-1, 16, heads, HEAD_DIM).permute(0, 2, 1, 3)


def gwa(q, kv, rpb, heads, shift, mut=None, dtype=torch.float64):
    """out [B, H, W, C] in `dtype`.  mut: a deliberate mistake (the sensitivity checks): "bias_t" transposed bias index,
    "mask_hw" H and W swapped in the mask regions, "nomask", "roll" roll direction reversed, "dim_major" channel
    d * heads + head, "scale16" 0.25 instead of 32^-0.5, "kv_swapped" the k and v halves exchanged, "self_attn" the query
    taken from the guided tensor (its k half)."""
    B, H, W, _ = q.shape
    C = HEAD_DIM * heads
    qq, kk, vv = q[..., :C].to(dtype), kv[..., :C].to(dtype), kv[..., C:2 * C].to(dtype)
    if mut == "kv_swapped":
        kk, vv = vv, kk
    if mut == "self_attn":
        qq = kk
    s = shift if mut == "roll" else -shift
    if shift:
        qq, kk, vv = (torch.roll(t, (s, s), (1, 2)) for t in (qq, kk, vv))
    dm = mut == "dim_major"
    qw, kw, vw = _windows(qq, heads, dm), _windows(kk, heads, dm), _windows(vv, heads, dm)
    scale = 0.25 if mut == "scale16" else HEAD_DIM ** -0.5
    attn = (qw * scale) @ kw.transpose(-1, -2)
    idx = rel_index()
    if mut == "bias_t":
        idx = idx.t()
    attn = attn + rpb.to(dtype)[idx].permute(2, 0, 1)
    nwy, nwx = H // 4, W // 4
    if shift and mut != "nomask":
        hl, wl = (W, H) if mut == "mask_hw" else (H, W)
        lab = 3 * regions(H, hl, shift)[:, None] + regions(W, wl, shift)[None, :]
        mw = lab.reshape(nwy, 4, nwx, 4).permute(0, 2, 1, 3).reshape(-1, 16)
        mask = (mw[:, None, :] != mw[:, :, None]).to(dtype) * -100.0
        attn = (attn.view(B, nwy * nwx, heads, 16, 16) + mask[None, :, None]).view(-1, heads, 16, 16)
    o = torch.softmax(attn, -1) @ vw  # [windows, heads, token, d]
    o = o.permute(0, 2, 3, 1) if dm else o.permute(0, 2, 1, 3)
    o = o.reshape(B, nwy, nwx, 4, 4, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)
    if shift:
        o = torch.roll(o, (-s, -s), (1, 2))
    return o


def scores_max(q, kv, rpb, heads):
    """max |(q * 32^-0.5) k^T + bias| over the unshifted windows (how far the inputs drive the softmax)."""
    C = HEAD_DIM * heads
    qw, kw = _windows(q[..., :C].double(), heads, False), _windows(kv[..., :C].double(), heads, False)
    return float(((qw * HEAD_DIM ** -0.5) @ kw.transpose(-1, -2) + rpb.double()[rel_index()].permute(2, 0, 1)).abs().max())


def case_seed(B, H, W, heads, shift):
    return 1000 * H + 10 * W + heads + 7 * shift + 100000 * B


def inputs(B, H, W, heads, pad, seed):
    """q [B,H,W,qcs], kv [B,H,W,kvcs], rpb [49,heads] and the three channel strides.  pad: 16 more channels per stride; the
    pads of q and kv hold NaN (a kernel that reads them poisons its result)."""
    C = HEAD_DIM * heads
    extra = 16 if pad else 0
    qcs, kvcs, ocs = C + extra, 2 * C + extra, C + extra
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, W, qcs, generator=g)
    kv = torch.randn(B, H, W, kvcs, generator=g)
    q[..., :C] *= QK_SIGMA
    kv[..., :C] *= QK_SIGMA
    q[..., C:] = float("nan")
    kv[..., 2 * C:] = float("nan")
    rpb = torch.randn(49, heads, generator=g) * 2.0
    return q, kv, rpb, qcs, kvcs, ocs


def tolerance(vmax, smax):
    """fp32 scores carry an absolute error of a few ulp(|S|): the bound scales with max|S| / 30 past |S| ~ 30."""
    return WA_TOL * max(1.0, smax / 30.0) * vmax


def accept(out, ref, vmax, smax):
    """(within the bound, max |out - ref| / max |v|)"""
    err = float((out.double() - ref.double()).abs().max())
    return (err == err) and err <= tolerance(vmax, smax), err / vmax
