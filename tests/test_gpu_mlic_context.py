"""rgbd_amd.LocalContext / LinearGlobalIntraContext / LinearGlobalInterContext and the three kernels of csrc/context_attn.hip
on the GPU (cases, statements and bounds: tests/mlic_context_cases.py; test_mlic_context_cases.py shows on the CPU that the
statements are the reference's and that every classic mistake lands 100x the bound away).

Module level: e_gpu = max |gpu - ref64| / max |ref64| <= 8 * e_ref per case and batch size, against the fixtures of the
unmodified reference; the state dict round trip.  Kernel level: each exported kernel alone against its fp64 statement, within
8x the error of that statement evaluated in fp32; the same bits from two calls; image b of a batch as the image alone; exact
zeros at the anchor positions in mode 1; channels beyond the logical ones untouched; refusals that write nothing.  The figures
are printed and recorded in DESIGN.md 5.4.  Observed on MI355X: modules 0.70 ... 2.45 x e_ref (bound 8 x), local attention
0.90 ... 1.62 x e32, linear attention 0.57 ... 2.08 x e32, depthwise convolution 0.44 ... 1.00 x e32."""
import ctypes
import json
import os

import pytest
import torch

import gridcap_cases as gc
import mlic_context_cases as mc
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
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- modules ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    require_gpu()
    import rgbd_amd

    out = {}
    for mod, (cls, kw, _) in mc.MODULES.items():
        m = getattr(rgbd_amd, cls)(**kw)
        m.load_state_dict(mc.module_weights(mod), strict=True)
        out[mod] = m.to("cuda")
    return out


@pytest.mark.parametrize("name", list(mc.CASES))
def test_module_vs_reference(nets, name):
    mod, _, H, W, _ = mc.CASES[name]
    fx = mc.load_fixture(name)
    ref64 = torch.from_numpy(fx["ref64"])
    xs = [t.cuda() for t in mc.case_inputs(name)]
    outs = {}
    for b in mc.case_batches(name):
        out = nets[mod](*[t[:b].contiguous() for t in xs])
        assert out.shape == ref64[:b].shape
        e_gpu = mc.rel_err(out.cpu(), ref64[:b])
        print(f"mlicctx {name} B={b}: e_gpu {e_gpu:.3e}, e_ref {mc.e_ref(fx, b):.3e}, ratio {e_gpu / mc.e_ref(fx, b):.2f}")
        assert e_gpu <= mc.FACTOR * mc.e_ref(fx, b), (e_gpu, mc.e_ref(fx, b))
        outs[b] = out
    b = mc.case_batches(name)[-1]
    # again (the captured graph of the call shape), into another tensor: the same bits; image 0 of the batch as alone
    again = nets[mod](*[t[:b].contiguous() for t in xs])
    assert again.data_ptr() != outs[b].data_ptr() and _bits(again, outs[b])
    alone = outs.get(1)
    if alone is None:
        alone = nets[mod](*[t[:1].contiguous() for t in xs])
    assert _bits(outs[b][:1], alone)
    assert _bits(outs[b][b - 1:], nets[mod](*[t[b - 1:b].contiguous() for t in xs]))


def test_state_dict_round_trip():
    require_gpu()
    import rgbd_amd

    with open(os.path.join(mc.GOLDEN, "mlicctx_state_dict.json")) as f:
        want = json.load(f)
    for mod, (cls, kw, _) in mc.MODULES.items():
        m = getattr(rgbd_amd, cls)(**kw)
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want[mod]
        sd = mc.module_weights(mod)
        m.load_state_dict(sd, strict=True)
        assert all(torch.equal(m.state_dict()[k].float(), sd[k].float()) for k in sd)
        first = want[mod][-1][0]
        with pytest.raises(RuntimeError):
            m.load_state_dict({k: v for k, v in sd.items() if k != first}, strict=True)
        with pytest.raises(RuntimeError):
            m.load_state_dict({**sd, "extra.weight": torch.zeros(1)}, strict=True)
        with pytest.raises(RuntimeError):
            m.load_state_dict({**sd, first: torch.zeros(tuple(sd[first].shape) + (1,))}, strict=True)
    lc = rgbd_amd.LocalContext(dim=32)
    assert lc.update_resolution(8, 12, "cuda") is True and lc.update_resolution(8, 12, "cuda") is False


def test_module_clone_and_handle_families(nets):
    L = _lib()
    name = "intra_8x12"
    x1, x2 = (t.cuda() for t in mc.case_inputs(name))
    clone = nets["intra"].clone_shared()
    assert _bits(clone(x1, x2), nets["intra"](x1, x2))
    out = torch.full((3, 64, 8, 12), 7.0, device="cuda")
    # a forward of another family, and a codec call, on a context handle
    assert L.rgbd_local_context_forward(nets["intra"]._h, _p(x1), 3, 8, 12, _p(out), _stream()) == EINVAL
    assert L.rgbd_linear_inter_forward(nets["local"]._h, _p(x1), 3, 8, 12, _p(out), _stream()) == EINVAL
    assert L.rgbd_linear_intra_forward(nets["inter32"]._h, _p(x1), _p(x2), 3, 8, 12, _p(out), _stream()) == EINVAL
    assert L.rgbd_aligner_forward(nets["local"]._h, _p(x1), _p(x2), 3, 8, 8, _p(out), _stream()) == EINVAL
    assert L.rgbd_elic_compress_single(nets["local"]._h, _p(x1), 1, 64, 64, 0, _stream()) == EINVAL
    assert L.rgbd_linear_intra_forward(nets["intra"]._h, _p(x1), _p(x2), 3, 8, 11, _p(out), _stream()) == EINVAL  # odd W
    assert L.rgbd_linear_intra_forward(nets["intra"]._h, _p(x1), None, 3, 8, 12, _p(out), _stream()) == EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    h = ctypes.c_void_p()
    assert L.rgbd_local_context_create(48, ctypes.byref(h)) == EINVAL
    assert L.rgbd_linear_inter_create(96, 64, 5, ctypes.byref(h)) == EINVAL
    assert L.rgbd_linear_intra_create(48, 1, ctypes.byref(h)) == EINVAL
    with pytest.raises(ValueError):
        nets["intra"](torch.zeros(1, 32, 4, 5), torch.zeros(1, 32, 4, 5))
    with pytest.raises(ValueError):
        nets["local"](torch.zeros(1, 16, 4, 4))


# ---- the local attention kernel --------------------------------------------------------------------------------------------
def _local_gpu(L, qkv, table, fw, fb, qpad=0, opad=0):
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    qd = torch.full((B, H, W, C3 + qpad), float("nan"), device="cuda")  # a read of the pad poisons the result
    qd[..., :C3] = qkv.cuda()
    out = torch.full((B, H, W, 2 * C + opad), SENTINEL, device="cuda")
    td, wd, bd = table.cuda(), fw.cuda().contiguous(), fb.cuda()  # (held until the call has run)
    rc = L.rgbd_local_ckbd_attention(_p(qd), C3 + qpad, B, H, W, C, 2, _p(td), _p(wd), _p(bd), _p(out), 2 * C + opad, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu()


# sizes: below one 2 x 4 tile; odd sizes that are no multiple of the tile; several tiles both ways; one wide row
LOCAL_SIZES = [(1, 1), (3, 5), (8, 12), (12, 8), (4, 20), (7, 9)]


@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("H,W", LOCAL_SIZES)
def test_local_attention_kernel(H, W, B):
    L = _lib()
    qkv, table, fw, fb = mc.local_kernel_inputs(B, H, W, 1000 + 100 * H + W)
    ref, smax = mc.local_attention(qkv, table, fw, fb, want_score=True)
    if H * W >= 15:
        assert mc.SCORE_BAND[0] <= smax <= mc.SCORE_BAND[1], smax
    e32 = mc.rel_err(mc.local_attention(qkv, table, fw, fb, dtype=torch.float32), ref)
    pad = 16 if B == 2 else 0
    out = _local_gpu(L, qkv, table, fw, fb, qpad=pad, opad=pad)
    e = mc.rel_err(out[..., :64], ref)
    print(f"local attention {B}x{H}x{W}: max|S| {smax:.1f}, e_gpu {e:.3e}, e32 {e32:.3e}, ratio {e / e32:.2f}")
    assert e <= mc.FACTOR * e32, (e, e32)
    assert (out[..., 64:] == SENTINEL).all()
    assert _bits(_local_gpu(L, qkv, table, fw, fb, qpad=pad, opad=pad), out)
    for b in range(B):
        assert _bits(_local_gpu(L, qkv[b:b + 1], table, fw, fb)[..., :64], out[b:b + 1, ..., :64])


def test_local_attention_rejects_bad_arguments():
    L = _lib()
    H, W, C = 6, 8, 32
    qkv, table, fw, fb = (t.cuda() for t in mc.local_kernel_inputs(1, H, W, 5))
    fw = fw.contiguous()
    out = torch.full((1, H, W, 2 * C + 16), SENTINEL, device="cuda")
    Q, T, FW, FB, O = "q", "t", "fw", "fb", "o"

    def call(B=1, H_=H, W_=W, C_=C, heads=2, qcs=3 * C, ocs=2 * C + 16, ptr=None):
        p = {Q: qkv.data_ptr(), T: table.data_ptr(), FW: fw.data_ptr(), FB: fb.data_ptr(), O: out.data_ptr()}
        p.update(ptr or {})
        return L.rgbd_local_ckbd_attention(p[Q], qcs, B, H_, W_, C_, heads, p[T], p[FW], p[FB], p[O], ocs, _stream())

    bad = [dict(B=0), dict(H_=0), dict(W_=-1), dict(C_=16), dict(C_=64), dict(heads=1), dict(heads=4), dict(qcs=3 * C - 4),
           dict(qcs=3 * C + 2), dict(ocs=2 * C - 1), dict(ptr={Q: qkv.data_ptr() + 4}), dict(ptr={FW: fw.data_ptr() + 4}),
           dict(ptr={Q: None}), dict(ptr={T: None}), dict(ptr={FW: None}), dict(ptr={FB: None}), dict(ptr={O: None}),
           dict(B=65536), dict(H_=65536, W_=65536)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (out[..., :2 * C] == SENTINEL).any() and (out[..., 2 * C:] == SENTINEL).all()


# ---- the linear attention kernel -------------------------------------------------------------------------------------------
def _linear_gpu(L, k, q, v, heads, hd, mode, pad=0):
    B, H, W, dim = k.shape

    def padded(t):
        d = torch.full((B, H, W, dim + pad), float("nan"), device="cuda")
        d[..., :dim] = t.cuda()
        return d

    kd, qd, vd = padded(k), padded(q), padded(v)
    out = torch.full((B, H, W, dim + pad), SENTINEL, device="cuda")
    n = L.rgbd_linear_attention_ws_floats(B, H, W, heads, hd, mode)
    assert n > 0
    ws = torch.full((n + 64,), SENTINEL, device="cuda")
    rc = L.rgbd_linear_attention(_p(kd), dim + pad, _p(qd), dim + pad, _p(vd), dim + pad, B, H, W, heads, hd, mode, _p(out),
                                 dim + pad, _p(ws), n, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert (ws[n:] == SENTINEL).all()
    return out.cpu()


# (H, W, heads, head_dim): one chunk of 128 tokens and less; exactly one chunk (16 x 8; 16 x 16 in mode 1); a chunk and a
# bit; several chunks; both head sizes; one head and several
LINEAR_CASES = [(1, 2, 1, 16), (4, 6, 2, 16), (16, 8, 1, 32), (16, 16, 2, 16), (10, 13 * 2, 3, 32), (24, 18, 2, 32), (5, 30, 9, 32)]


@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("H,W,heads,hd", LINEAR_CASES)
def test_linear_attention_kernel(H, W, heads, hd, mode, B):
    L = _lib()
    k, q, v = mc.linear_kernel_inputs(B, H, W, heads, hd, 2000 + 100 * H + W + mode)
    ref = mc.linear_attention(k, q, v, heads, mode)
    e32 = mc.rel_err(mc.linear_attention(k, q, v, heads, mode, dtype=torch.float32), ref)
    pad = 16 if B == 2 else 0
    out = _linear_gpu(L, k, q, v, heads, hd, mode, pad)
    dim = heads * hd
    e = mc.rel_err(out[..., :dim], ref)
    print(f"linear attention {B}x{H}x{W} heads {heads}x{hd} mode {mode}: e_gpu {e:.3e}, e32 {e32:.3e}, ratio {e / e32:.2f}")
    assert e <= mc.FACTOR * e32, (e, e32)
    assert (out[..., dim:] == SENTINEL).all()
    if mode:
        am = mc.anchor_map(H, W)
        assert (out[:, am][..., :dim].view(torch.int32) == 0).all()  # +0.0f, bit for bit
    assert _bits(_linear_gpu(L, k, q, v, heads, hd, mode, pad), out)
    for b in range(B):
        assert _bits(_linear_gpu(L, k[b:b + 1], q[b:b + 1], v[b:b + 1], heads, hd, mode)[..., :dim], out[b:b + 1, ..., :dim])


def test_linear_attention_keys_that_overflow_without_the_maximum():
    L = _lib()
    k, q, v = mc.linear_kernel_inputs(2, 12, 14, 2, 16, 7, key_offset=100.0)
    for mode in (0, 1):
        ref = mc.linear_attention(k, q, v, 2, mode)
        e32 = mc.rel_err(mc.linear_attention(k, q, v, 2, mode, dtype=torch.float32), ref)
        e = mc.rel_err(_linear_gpu(L, k, q, v, 2, 16, mode), ref)
        print(f"linear attention, keys + 100, mode {mode}: e_gpu {e:.3e}, e32 {e32:.3e}")
        assert e <= mc.FACTOR * e32


def test_linear_attention_rejects_bad_arguments():
    L = _lib()
    H, W, heads, hd = 6, 8, 2, 16
    dim = heads * hd
    k, q, v = (torch.randn(1, H, W, dim + 16, device="cuda") for _ in range(3))
    out = torch.full((1, H, W, dim + 16), SENTINEL, device="cuda")
    n = L.rgbd_linear_attention_ws_floats(1, H, W, heads, hd, 0)
    ws = torch.full((n,), SENTINEL, device="cuda")
    K, Q, V, O, WS = "k", "q", "v", "o", "ws"

    def call(B=1, H_=H, W_=W, heads_=heads, hd_=hd, mode=0, kcs=dim + 16, qcs=dim + 16, vcs=dim + 16, ocs=dim + 16, wsn=n, ptr=None):
        p = {K: k.data_ptr(), Q: q.data_ptr(), V: v.data_ptr(), O: out.data_ptr(), WS: ws.data_ptr()}
        p.update(ptr or {})
        return L.rgbd_linear_attention(p[K], kcs, p[Q], qcs, p[V], vcs, B, H_, W_, heads_, hd_, mode, p[O], ocs, p[WS], wsn, _stream())

    bad = [dict(B=0), dict(H_=0), dict(W_=0), dict(heads_=0), dict(hd_=8), dict(hd_=64), dict(mode=2), dict(mode=-1),
           dict(mode=1, W_=7), dict(kcs=dim - 4), dict(qcs=dim - 4), dict(vcs=dim - 4), dict(ocs=dim - 4), dict(kcs=dim + 2),
           dict(qcs=dim + 2), dict(vcs=dim + 2), dict(ocs=dim + 2), dict(wsn=n - 1), dict(ptr={K: k.data_ptr() + 4}),
           dict(ptr={Q: q.data_ptr() + 4}), dict(ptr={V: v.data_ptr() + 4}), dict(ptr={O: out.data_ptr() + 4}), dict(ptr={K: None}),
           dict(ptr={Q: None}), dict(ptr={V: None}), dict(ptr={O: None}), dict(ptr={WS: None}), dict(B=65536),
           dict(H_=65536, W_=65536)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    assert L.rgbd_linear_attention_ws_floats(1, H, 7, heads, hd, 1) == EINVAL
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (ws == SENTINEL).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (out[..., :dim] == SENTINEL).any() and (out[..., dim:] == SENTINEL).all()


# ---- the depthwise convolution ----------------------------------------------------------------------------------------------
def _dw_gpu(L, x, w, b, gelu, pad=0):
    B, H, W, C = x.shape
    xd = torch.full((B, H, W, C + pad), float("nan"), device="cuda")
    xd[..., :C] = x.cuda()
    y = torch.full((B, H, W, C + pad), SENTINEL, device="cuda")
    wd, bd = w.cuda().contiguous(), b.cuda()  # (held until the call has run)
    assert L.rgbd_dwconv3x3(_p(xd), B, H, W, C, C + pad, _p(wd), _p(bd), gelu, _p(y), C + pad, _stream()) == 0
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("gelu", [0, 1])
@pytest.mark.parametrize("H,W,C", [(1, 1, 32), (3, 5, 7), (8, 12, 96), (12, 8, 128), (5, 31, 288)])
def test_dwconv_kernel(H, W, C, gelu, B):
    L = _lib()
    x, w, b = mc.dwconv_inputs(B, H, W, C, 3000 + 100 * H + W)
    ref = mc.dwconv3x3(x, w, b, gelu)
    e32 = mc.rel_err(mc.dwconv3x3(x, w, b, gelu, dtype=torch.float32), ref)
    pad = 5 if B == 2 else 0
    out = _dw_gpu(L, x, w, b, gelu, pad)
    e = mc.rel_err(out[..., :C], ref)
    print(f"dwconv {B}x{H}x{W}x{C} gelu {gelu}: e_gpu {e:.3e}, e32 {e32:.3e}")
    assert e <= mc.FACTOR * e32, (e, e32)
    assert (out[..., C:] == SENTINEL).all()
    assert _bits(_dw_gpu(L, x, w, b, gelu, pad), out)
    for i in range(B):
        assert _bits(_dw_gpu(L, x[i:i + 1], w, b, gelu)[..., :C], out[i:i + 1, ..., :C])


@pytest.mark.parametrize("case", gc.DWCONV_CASES, ids=lambda c: "gelu%(gelu)d" % c)
def test_dwconv_kernel_past_the_grid_cap(case):
    """1 x 86 x 85 x 288 = 2 105 280 outputs against the 8192 x 256 grid cap (two sweeps, the second one ragged), under
    test_dwconv_kernel's reference and bound; the whole destination is compared, the channels behind C keep the sentinel, two
    calls give the same bits, and so does the call without pad channels."""
    L = _lib()
    bc = gc.build_dwconv(case, mc, SENTINEL)
    C = case["C"]
    outs = [_dw_gpu(L, bc["x"], bc["w"], bc["b"], case["gelu"], gc.DWCONV_PAD).numpy() for _ in range(2)]
    assert bc["stages"]["dwconv"]["accept"]({"y": outs[0]}) == []
    assert gc.same_bits(outs[0], outs[1])
    alone = _dw_gpu(L, bc["x"], bc["w"], bc["b"], case["gelu"]).numpy()
    assert gc.same_bits(alone, outs[0][..., :C])


def test_dwconv_rejects_bad_arguments():
    L = _lib()
    H, W, C = 4, 6, 32
    x, w, b = (t.cuda() for t in mc.dwconv_inputs(1, H, W, C, 9))
    y = torch.full((1, H, W, C + 8), SENTINEL, device="cuda")

    def call(B=1, H_=H, W_=W, C_=C, xcs=C, ycs=C + 8, gelu=1, xp=x.data_ptr(), wp=w.data_ptr(), bp=b.data_ptr(), yp=y.data_ptr()):
        return L.rgbd_dwconv3x3(xp, B, H_, W_, C_, xcs, wp, bp, gelu, yp, ycs, _stream())

    bad = [dict(B=0), dict(H_=0), dict(W_=0), dict(C_=0), dict(xcs=C - 1), dict(ycs=C - 1), dict(gelu=2), dict(gelu=-1), dict(xp=None),
           dict(wp=None), dict(bp=None), dict(yp=None), dict(yp=x.data_ptr(), ycs=C), dict(H_=65536, W_=65536)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (y[..., :C] == SENTINEL).any() and (y[..., C:] == SENTINEL).all()
