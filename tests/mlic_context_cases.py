"""The attention contexts of MLIC++ (rgbd_amd.LocalContext / LinearGlobalIntraContext / LinearGlobalInterContext and the three
kernels of csrc/context_attn.hip; reference modules/transform/context.py): the cases of the fixtures
tests/golden/mlicctx_<case>.npz (written by tests/golden/make_mlic_context.py from the unmodified reference), their inputs and
weights, fp64 statements of the three operations and of the three modules with deliberate mistakes selectable, and the
acceptance bound -- shared by test_mlic_context_cases.py (CPU) and test_gpu_mlic_context.py.

Bound, module level: e = max |out - ref64| / max |ref64| <= 8 * e_ref, e_ref = the reference's own fp32 error against its
float64 run on the same images (mlicctx_floors.json, per batch prefix).  Kernel level: the same factor over the error of the
statement below evaluated in fp32 against itself in fp64.  The factor covers another summation order (single fma chains, the
chunked token sums) and the device's expf / erff against the CPU's.

A fixture holds a batch of three images; every operation here works image by image, so the first b images are the case at
B = b."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTOR = 8.0
SIZES = [(4, 4), (8, 12), (12, 8), (4, 20)]  # one tile and less; non-square, several tiles / W % 4 == 0; the other way; wide
BATCHES = (1, 2, 3)
SWEEP = (32, 40)  # the latent grid of a 512 x 640 image, at B = 2
# module configuration: (class name, constructor arguments, weight seed)
MODULES = {
    "local": ("LocalContext", {"dim": 32}, 11),
    "intra": ("LinearGlobalIntraContext", {"dim": 32, "num_heads": 2}, 12),
    "inter32": ("LinearGlobalInterContext", {"dim": 32, "out_dim": 64, "num_heads": 1}, 13),
    "inter96": ("LinearGlobalInterContext", {"dim": 96, "out_dim": 64, "num_heads": 3}, 14),
    "inter288": ("LinearGlobalInterContext", {"dim": 288, "out_dim": 64, "num_heads": 9}, 15),
}
SWEEP_MODULES = ("local", "intra", "inter96")


def _cases():
    out, seed = {}, 200
    for mod in MODULES:
        for (h, w) in SIZES:
            out[f"{mod}_{h}x{w}"] = (mod, 3, h, w, seed)
            seed += 1
    for mod in SWEEP_MODULES:
        out[f"{mod}_{SWEEP[0]}x{SWEEP[1]}"] = (mod, 2, SWEEP[0], SWEEP[1], seed)
        seed += 1
    return out


CASES = _cases()  # name: (module key, images in the fixture, H, W, input seed)
SCORE_BAND = (10.0, 50.0)  # LocalContext: max |score + bias| -- a softmax far from uniform, and far below the mask's 100

LOCAL_MUTATIONS = ["head_slow_in", "head_fast_out", "bias_transposed", "parity_flipped", "mask_dropped", "masked_rows_skipped",
                   "oob_left_out", "fusion_transposed"]
LINEAR_MUTATIONS = ["axes_exchanged", "ctx_transposed"]
INTRA_MUTATIONS = ["sets_exchanged"]


def case_batches(name):
    return BATCHES if CASES[name][1] == 3 else (CASES[name][1],)


def case_inputs(name):
    mod, n, H, W, seed = CASES[name]
    dim = MODULES[mod][1]["dim"]
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(n, dim, H, W, generator=g)]
    if mod == "intra":
        xs.append(torch.randn(n, dim, H, W, generator=g))
    return xs


def module_weights(mod):
    from rgbd_amd import synth

    cls, kw, wseed = MODULES[mod]
    return synth.synthetic_state_dict(wseed, model=cls, **kw)


def load_fixture(name):
    g = dict(np.load(os.path.join(GOLDEN, f"mlicctx_{name}.npz")))
    with open(os.path.join(GOLDEN, "mlicctx_floors.json")) as f:
        g["floors"] = json.load(f)[name]
    return g


def e_ref(fx, b):
    return float(fx["floors"]["e_ref"][str(b)])


def rel_err(out, ref64):
    out, ref64 = torch.as_tensor(out).double(), torch.as_tensor(ref64).double()
    return float((out - ref64).abs().max() / ref64.abs().max())


def anchor_map(H, W):
    """True where (row + col) is odd: the positions coded first (utils/ckbd.py:6-20)."""
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return ((y + x) % 2) == 1


# ---- the three operations, stated on NHWC tensors -------------------------------------------------------------------------
def _windows(t, H, W):
    """t [..., H, W] -> [..., H, W, 25]: the 5x5 neighbourhood of every position, zeros outside the map."""
    tp = F.pad(t, (2, 2, 2, 2))
    return torch.stack([tp[..., iy:iy + H, ix:ix + W] for iy in range(5) for ix in range(5)], dim=-1)


def local_attention(qkv, table, fw, fb, heads=2, mut=None, dtype=torch.float64, want_score=False):
    """rgbd_local_ckbd_attention: qkv [B,H,W,3C] (q | k | v, channel d * heads + h) -> [B,H,W,2C].  mut: one of LOCAL_MUTATIONS."""
    qkv, table, fw, fb = qkv.to(dtype), table.to(dtype), fw.to(dtype), fb.to(dtype)
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads

    def per_head(t):  # [B,H,W,C] -> [B,heads,hd,H,W]
        if mut == "head_slow_in":
            return t.reshape(B, H, W, heads, hd).permute(0, 3, 4, 1, 2)
        return t.reshape(B, H, W, hd, heads).permute(0, 4, 3, 1, 2)

    qw, kw, vw = (_windows(per_head(qkv[..., i * C:(i + 1) * C]), H, W) for i in range(3))  # [B,heads,hd,H,W,25]
    score = torch.einsum("bhdyxi,bhdyxj->bhyxij", qw * hd ** -0.5, kw)
    iy, ix = torch.arange(25) // 5, torch.arange(25) % 5
    rel = (iy[:, None] - iy[None, :] + 4) * 9 + (ix[:, None] - ix[None, :] + 4)  # [i][j]
    if mut == "bias_transposed":
        rel = rel.t()
    score = score + table[rel].permute(2, 0, 1)[None, :, None, None]
    smax = float(score.abs().max())
    am = anchor_map(H, W)
    if mut == "parity_flipped":
        am = ~am
    inside = _windows(torch.ones(H, W, dtype=dtype), H, W) > 0  # [H,W,25]
    aw = _windows(am.to(dtype), H, W) > 0  # inside the map and an anchor
    both = aw[:, :, :, None] & aw[:, :, None, :]
    mask = torch.where(both, 0.0, -100.0).to(dtype)
    if mut == "mask_dropped":
        mask = torch.zeros_like(mask)
    score = score + mask[None, None]
    if mut == "oob_left_out":
        score = score.masked_fill(~inside[None, None, :, :, None, :], float("-inf"))
    A = torch.softmax(score, dim=-1)
    o = torch.einsum("bhyxij,bhdyxj->bhdyxi", A, vw)  # [B,heads,hd,H,W,25]
    if mut == "masked_rows_skipped":
        o = o * aw.to(dtype)[None, None, None]
    if mut == "head_fast_out":
        o = o.permute(0, 2, 1, 3, 4, 5)  # channel d * heads + h
    xin = o.reshape(B, C, H, W, 25)
    w3 = (fw.transpose(2, 3) if mut == "fusion_transposed" else fw).reshape(2 * C, C, 25)
    out = torch.einsum("bcyxi,oci->byxo", xin, w3) + fb
    return (out, smax) if want_score else out


def linear_attention(k, q, v, heads, mode, mut=None, dtype=torch.float64):
    """rgbd_linear_attention: k, q, v [B,H,W,dim] -> [B,H,W,dim].  mut: LINEAR_MUTATIONS, INTRA_MUTATIONS or "no_max" (the
    key softmax as exp / sum of exp without the maximum taken off, in `dtype`)."""
    k, q, v = k.to(dtype), q.to(dtype), v.to(dtype)
    B, H, W, dim = k.shape
    hd = dim // heads
    flat = lambda t: t.reshape(B, H * W, heads, hd)  # noqa: E731
    am = anchor_map(H, W).reshape(-1)
    kv_idx = torch.nonzero(am).reshape(-1) if mode else torch.arange(H * W)
    q_idx = torch.nonzero(~am).reshape(-1) if mode else torch.arange(H * W)
    if mut == "sets_exchanged":
        kv_idx, q_idx = q_idx, kv_idx
    K, V, Q = flat(k)[:, kv_idx], flat(v)[:, kv_idx], flat(q)[:, q_idx]
    if mut == "no_max":
        e = torch.exp(K)
        Ks = e / e.sum(dim=1, keepdim=True)
    else:
        Ks = torch.softmax(K, dim=3 if mut == "axes_exchanged" else 1)
    Qs = torch.softmax(Q, dim=1 if mut == "axes_exchanged" else 3)
    ctx = torch.einsum("bnhd,bnhe->bhde", Ks, V)
    if mut == "ctx_transposed":
        ctx = ctx.transpose(2, 3)
    o = torch.einsum("bhde,bnhd->bnhe", ctx, Qs)
    out = torch.zeros(B, H * W, heads, hd, dtype=dtype)
    out[:, q_idx] = o
    return out.reshape(B, H, W, dim)


def dwconv3x3(x, w, b, gelu, dtype=torch.float64):
    """rgbd_dwconv3x3: x [B,H,W,C], w [C,1,3,3] -> [B,H,W,C]."""
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype), b.to(dtype), padding=1, groups=x.shape[3])
    return (F.gelu(y) if gelu else y).permute(0, 2, 3, 1)


# ---- the three modules ----------------------------------------------------------------------------------------------------
def local_context(sd, x, mut=None, dtype=torch.float64, want_score=False):
    w = lambda n: sd[n].to(dtype)  # noqa: E731
    lin = lambda t, n: F.linear(t, w(f"{n}.weight"), w(f"{n}.bias"))  # noqa: E731
    ln = lambda t, n: F.layer_norm(t, (t.shape[-1],), w(f"{n}.weight"), w(f"{n}.bias"), 1e-5)  # noqa: E731
    t = x.to(dtype).permute(0, 2, 3, 1)
    a, smax = local_attention(lin(ln(t, "norm1"), "qkv_proj"), w("relative_position_table"), w("fusion.weight"), w("fusion.bias"),
                              2, mut, dtype, want_score=True)
    x1 = lin(a, "proj")
    out = (x1 + lin(F.gelu(lin(ln(x1, "norm2"), "mlp.fc1")), "mlp.fc2")).permute(0, 3, 1, 2)
    return (out, smax) if want_score else out


def linear_context(sd, x1, x2, heads, mut=None, dtype=torch.float64):
    """x2 None: LinearGlobalInterContext; else LinearGlobalIntraContext."""
    w = lambda n: sd[n].to(dtype)  # noqa: E731
    cv = lambda t, n, **kw: F.conv2d(t, w(f"{n}.weight"), w(f"{n}.bias"), **kw)  # noqa: E731
    dw = lambda t, n: cv(t, n, padding=1, groups=t.shape[1])  # noqa: E731
    br = lambda t, n: dw(cv(t, f"{n}.0"), f"{n}.1").permute(0, 2, 3, 1)  # noqa: E731
    x1 = x1.to(dtype)
    if x2 is None:
        k, q, v = br(x1, "keys"), br(x1, "queries"), br(x1, "values")
    else:
        am = anchor_map(x1.shape[2], x1.shape[3]).to(dtype)
        k, q, v = br(x1 * am, "keys"), br(x1 * (1 - am), "queries"), br(x2.to(dtype), "values")
    a = linear_attention(k, q, v, heads, 0 if x2 is None else 1, mut, dtype).permute(0, 3, 1, 2)
    att = cv(a, "reprojection", padding=2)
    m = cv(F.gelu(dw(F.gelu(cv(att, "mlp.0")), "mlp.2")), "mlp.4")
    return (cv(att, "skip") if x2 is None else att) + m


def module_statement(name, b, mut=None, dtype=torch.float64):
    """The fp64 statement of case `name` on its first b images."""
    mod = CASES[name][0]
    sd = module_weights(mod)
    xs = [t[:b] for t in case_inputs(name)]
    if mod == "local":
        return local_context(sd, xs[0], mut, dtype)
    return linear_context(sd, xs[0], xs[1] if mod == "intra" else None, MODULES[mod][1]["num_heads"], mut, dtype)


# ---- kernel-level inputs ----------------------------------------------------------------------------------------------------
def local_kernel_inputs(B, H, W, seed, C=32, heads=2):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, H, W, 3 * C, generator=g)
    qkv[..., :2 * C] *= 2.0  # scores of std ~4
    table = torch.randn(81, heads, generator=g)
    fw = (torch.rand(2 * C, C, 5, 5, generator=g) * 2 - 1) / (25 * C) ** 0.5
    fb = torch.rand(2 * C, generator=g) - 0.5
    return qkv, table, fw, fb


def linear_kernel_inputs(B, H, W, heads, hd, seed, key_offset=0.0):
    g = torch.Generator().manual_seed(seed)
    k, q, v = (torch.randn(B, H, W, heads * hd, generator=g) * s for s in (3.0, 3.0, 1.0))
    return k + key_offset, q, v


def dwconv_inputs(B, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, H, W, C, generator=g), (torch.rand(C, 1, 3, 3, generator=g) * 2 - 1) / 3,
            (torch.rand(C, generator=g) * 2 - 1) / 3)
