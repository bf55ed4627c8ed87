"""The float64 statement and the acceptance function of tests/guided_attention_cases.py, checked on the CPU: the statement
equals the reference's WindowAttention with its window partition / roll / mask (modules/transform/spatialAligner.py:54-83,
138-170, 249-331), restated here in torch float64 the way the reference computes it (a mask image labelled by slices,
partitioned like the tokens; the bias gathered through a relative_position_index built from coordinate differences); a plain
fp32 evaluation passes the acceptance function on every case; every deliberate mistake fails it."""
import pytest
import torch

import guided_attention_cases as gc

ALL = [(B, *c) for c in gc.CASES for B in gc.BATCHES] + [gc.SWEEP_CASE]


def _partition(x, ws=4):
    B, H, W, C = x.shape
    return x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C)


def _reverse(windows, H, W, ws=4):
    B = int(windows.shape[0] / (H * W / ws / ws))
    return windows.view(B, H // ws, W // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


def _reference_style(q, kv, rpb, heads, shift):
    """q: [B,H,W,C], kv: [B,H,W,2C] (what qkv1 / qkv2 produce), float64."""
    ws = 4
    B, H, W, C = q.shape
    mask = None
    if shift > 0:
        img = torch.zeros((1, H, W, 1), dtype=torch.float64)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[:, hs, wsl, :] = cnt
                cnt += 1
        mwin = _partition(img).view(-1, ws * ws)
        mask = mwin.unsqueeze(1) - mwin.unsqueeze(2)
        mask = mask.masked_fill(mask != 0, -100.0).masked_fill(mask == 0, 0.0)
        q = torch.roll(q, shifts=(-shift, -shift), dims=(1, 2))
        kv = torch.roll(kv, shifts=(-shift, -shift), dims=(1, 2))
    qw = _partition(q).view(-1, ws * ws, C)
    kvw = _partition(kv).view(-1, ws * ws, 2 * C)
    B_, N, _ = qw.shape
    qh = qw.reshape(B_, N, 1, heads, C // heads).permute(2, 0, 3, 1, 4)[0]
    kvh = kvw.reshape(B_, N, 2, heads, C // heads).permute(2, 0, 3, 1, 4)
    k, v = kvh[0], kvh[1]
    attn = (qh * (C // heads) ** -0.5) @ k.transpose(-2, -1)
    coords = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    index = rel.sum(-1)
    bias = rpb[index.view(-1)].view(N, N, -1).permute(2, 0, 1).contiguous()
    attn = attn + bias.unsqueeze(0)
    if mask is not None:
        nW = mask.shape[0]
        attn = (attn.view(B_ // nW, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    attn = torch.softmax(attn, dim=-1)
    o = (attn @ v).transpose(1, 2).reshape(B_, N, C)
    o = _reverse(o.view(-1, ws, ws, C), H, W)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o


def _case(B, H, W, heads, shift, pad=False):
    q, kv, rpb, *_ = gc.inputs(B, H, W, heads, pad, gc.case_seed(B, H, W, heads, shift))
    C = gc.HEAD_DIM * heads
    return q, kv, rpb, C


@pytest.mark.parametrize("B,H,W,heads,shift", ALL)
def test_statement_equals_reference_style(B, H, W, heads, shift):
    q, kv, rpb, C = _case(B, H, W, heads, shift, pad=(B == 2))
    ours = gc.gwa(q, kv, rpb, heads, shift)
    ref = _reference_style(q[..., :C].double(), kv[..., :2 * C].double(), rpb.double(), heads, shift)
    assert ours.shape == ref.shape == (B, H, W, C)
    assert float((ours - ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("B,H,W,heads,shift", ALL)
def test_inputs_drive_the_softmax_and_fp32_passes(B, H, W, heads, shift):
    q, kv, rpb, C = _case(B, H, W, heads, shift, pad=(B == 2))
    smax = gc.scores_max(q, kv, rpb, heads)
    assert 15 < smax < 80, smax
    vmax = float(kv[..., C:2 * C].abs().max())
    ref = gc.gwa(q, kv, rpb, heads, shift)
    ok, err = gc.accept(gc.gwa(q, kv, rpb, heads, shift, dtype=torch.float32), ref, vmax, smax)
    assert ok, err
    assert err < 0.25 * gc.tolerance(1.0, smax)  # a plain fp32 evaluation uses a fraction of the bound


@pytest.mark.parametrize("B,H,W,heads,shift", gc.SENSITIVITY_CASES + [gc.SWEEP_CASE])
def test_every_mistake_fails(B, H, W, heads, shift):
    q, kv, rpb, C = _case(B, H, W, heads, shift)
    smax = gc.scores_max(q, kv, rpb, heads)
    vmax = float(kv[..., C:2 * C].abs().max())
    ref = gc.gwa(q, kv, rpb, heads, shift)
    for m in gc.MUTATIONS:
        ok, err = gc.accept(gc.gwa(q, kv, rpb, heads, shift, m), ref, vmax, smax)
        assert not ok and err >= 100 * gc.tolerance(1.0, smax), (m, err)
    assert not gc.accept(torch.full_like(ref, float("nan")), ref, vmax, smax)[0]
