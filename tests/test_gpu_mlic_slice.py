"""rgbd_amd.EntropyParametersMLIC / ChannelContext / LatentResidualPrediction and the fused kernel of csrc/pixel_mlp.hip on the
GPU (cases, statements and bounds: tests/mlic_slice_cases.py; test_mlic_slice_cases.py shows on the CPU that the statements are
the reference's and that every classic mistake lands at least 10 bounds away).

Module level: e_gpu = max |gpu - ref64| / max |ref64| <= 8 * e_ref per case and batch size, against the fixtures of the
unmodified reference, for the fused launch and for the four conv launches behind `fused = False`; the same bits from three calls
in a row, from image b of a batch and the image alone, from a clone, and from one instance called at another size in between;
the state dict round trip; refusals that launch nothing.  Kernel level (rgbd_pixel_mlp4 through ctypes): the input cut into the
codec's segments gives the bits of the concatenated input; a parity call gives the full call's bits on its pixels and leaves
every other pixel of a sentinel-filled output alone; image b of a B = 3 call gives the bits of the B = 1 call on that image.
The figures are printed and recorded in DESIGN.md 5.8."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import mlic_slice_cases as mc
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

EINVAL = -22
SENTINEL = 12345.0
EP = [m for m in mc.MODULES if mc.MODULES[m][0] == "EntropyParametersMLIC"]


def _lib():
    require_gpu()
    from rgbd_amd import _lib as lib

    return lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


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


def _call(net, mod, xs):
    """The module on its case inputs: the parameter networks take their segments, the others their one tensor."""
    return net.forward_segments(xs) if mod in mc.SEGMENTS else net(xs[0])


@pytest.mark.parametrize("name", list(mc.CASES))
def test_module_vs_reference(nets, name):
    mod = mc.CASES[name][0]
    fx = mc.load_fixture(name)
    ref64 = torch.from_numpy(fx["ref64"])
    xs = [t.cuda() for t in mc.case_inputs(name)]
    outs = {}
    for b in mc.case_batches(name):
        out = _call(nets[mod], mod, [t[:b].contiguous() for t in xs])
        assert out.shape == ref64[:b].shape
        e_gpu = mc.rel_err(out.cpu(), ref64[:b])
        print(f"mlicslice {name} B={b}: e_gpu {e_gpu:.3e}, e_ref {mc.e_ref(fx, b):.3e}, ratio {e_gpu / mc.e_ref(fx, b):.2f}")
        assert e_gpu <= mc.FACTOR * mc.e_ref(fx, b), (e_gpu, mc.e_ref(fx, b))
        outs[b] = out
    b = mc.case_batches(name)[-1]
    # twice more (the captured graph of the call shape), into other tensors: the same bits; images of the batch as alone
    for _ in range(2):
        again = _call(nets[mod], mod, [t[:b].contiguous() for t in xs])
        assert again.data_ptr() != outs[b].data_ptr() and _bits(again, outs[b])
    alone = outs.get(1)
    if alone is None:
        alone = _call(nets[mod], mod, [t[:1].contiguous() for t in xs])
    assert _bits(outs[b][:1], alone)
    assert _bits(outs[b][b - 1:], _call(nets[mod], mod, [t[b - 1:b].contiguous() for t in xs]))
    if mod in mc.SEGMENTS:  # the reference's call: one concatenated tensor
        assert _bits(nets[mod](torch.cat(xs, dim=1)[:b].contiguous()), outs[b])


@pytest.mark.parametrize("name", [n for n in mc.CASES if mc.CASES[n][0] in EP])
def test_unfused_layers_vs_reference(nets, name):
    mod = mc.CASES[name][0]
    fx = mc.load_fixture(name)
    ref64 = torch.from_numpy(fx["ref64"])
    xs = [t.cuda() for t in mc.case_inputs(name)]
    net = nets[mod]
    assert net.fused is True
    net.fused = False
    try:
        for b in mc.case_batches(name):
            out = net.forward_segments([t[:b].contiguous() for t in xs])
            e_gpu = mc.rel_err(out.cpu(), ref64[:b])
            print(f"mlicslice {name} B={b} unfused: e_gpu {e_gpu:.3e}, e_ref {mc.e_ref(fx, b):.3e}, ratio {e_gpu / mc.e_ref(fx, b):.2f}")
            assert e_gpu <= mc.FACTOR * mc.e_ref(fx, b), (e_gpu, mc.e_ref(fx, b))
            assert _bits(net.forward_segments([t[:b].contiguous() for t in xs]), out)
    finally:
        net.fused = True


@pytest.mark.parametrize("fused", [True, False])
def test_module_parity_halves(nets, fused):
    name = "ep960_8x12"
    xs = [t.cuda() for t in mc.case_inputs(name)]
    net = nets["ep960"]
    net.fused = fused
    try:
        full = net.forward_segments(xs)
        am = mc.anchor_map(8, 12).cuda()
        for parity, sel in ((0, am), (1, ~am)):
            out = torch.full_like(full, SENTINEL)
            assert net.forward_segments(xs, parity=parity, out=out) is out
            assert _bits(out[:, :, sel], full[:, :, sel]) and (out[:, :, ~sel] == SENTINEL).all()
        with pytest.raises(ValueError):
            net.forward_segments(xs, parity=0)  # no out
        with pytest.raises(ValueError):
            net.forward_segments(xs, parity=2, out=out)
    finally:
        net.fused = True


def test_one_instance_across_sizes(nets):
    for mod in ("ep832", "cc96", "lrp384"):
        small = [t.cuda() for t in mc.case_inputs(f"{mod}_4x4")]
        other = [t.cuda() for t in mc.case_inputs(f"{mod}_12x8")]
        first = _call(nets[mod], mod, small)
        _call(nets[mod], mod, other)
        assert _bits(_call(nets[mod], mod, small), first)


def test_state_dict_round_trip():
    require_gpu()
    import rgbd_amd

    with open(os.path.join(mc.GOLDEN, "mlicslice_state_dict.json")) as f:
        want = json.load(f)
    for mod, (cls, kw, _) in mc.MODULES.items():
        m = getattr(rgbd_amd, cls)(**kw)
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want[mod]
        sd = mc.module_weights(mod)
        m.load_state_dict(sd, strict=True)
        assert all(torch.equal(m.state_dict()[k].float(), sd[k].float()) for k in sd)
        last = want[mod][-1][0]
        with pytest.raises(RuntimeError):
            m.load_state_dict({k: v for k, v in sd.items() if k != last}, strict=True)
        with pytest.raises(RuntimeError):
            m.load_state_dict({**sd, "extra.weight": torch.zeros(1)}, strict=True)
        with pytest.raises(RuntimeError):
            m.load_state_dict({**sd, last: torch.zeros(tuple(sd[last].shape) + (1,))}, strict=True)


def test_clones_give_the_same_bits(nets):
    for mod in ("ep960", "cc288", "lrp384"):
        xs = [t.cuda() for t in mc.case_inputs(f"{mod}_8x12")]
        clone = nets[mod].clone_shared()
        assert _bits(_call(clone, mod, xs), _call(nets[mod], mod, xs))


def test_refusals(nets):
    L = _lib()
    import rgbd_amd
    from torch import nn

    h = ctypes.c_void_p()
    assert L.rgbd_entropy_params_mlic_create(648, 64, ctypes.byref(h)) == EINVAL and not h.value  # in_dim % 16
    assert L.rgbd_entropy_params_mlic_create(640, 144, ctypes.byref(h)) == EINVAL and not h.value  # out_dim > 128
    with pytest.raises(NotImplementedError):
        rgbd_amd.EntropyParametersMLIC(648, 64)
    with pytest.raises(NotImplementedError):
        rgbd_amd.EntropyParametersMLIC(640, 64, act=nn.ReLU)
    with pytest.raises(NotImplementedError):
        rgbd_amd.LatentResidualPrediction(352, 32, act=nn.ReLU)
    ep, cc, lrp = nets["ep960"], nets["cc32"], nets["lrp352"]
    x = torch.randn(1, 960, 4, 4, device="cuda")
    out = torch.full((1, 128, 4, 4), SENTINEL, device="cuda")
    seven = [x[:, :128]] * 6 + [x[:, :192]]
    with pytest.raises(ValueError):
        ep.forward_segments(seven)  # more than 6 segments
    ptrs = (ctypes.c_void_p * 7)(*[x.data_ptr()] * 7)
    chans = (ctypes.c_int32 * 7)(128, 128, 128, 128, 128, 128, 192)
    fwd = L.rgbd_entropy_params_mlic_forward
    assert fwd(ep._h, ptrs, chans, 7, 1, 4, 4, -1, _p(out), _stream()) == EINVAL
    one = (ctypes.c_void_p * 1)(x.data_ptr())
    assert fwd(ep._h, one, (ctypes.c_int32 * 1)(944), 1, 1, 4, 4, -1, _p(out), _stream()) == EINVAL  # not the handle's in_dim
    assert fwd(ep._h, one, (ctypes.c_int32 * 1)(960), 1, 1, 4, 5, 0, _p(out), _stream()) == EINVAL  # a parity on an odd W
    assert fwd(cc._h, one, (ctypes.c_int32 * 1)(32), 1, 1, 4, 4, -1, _p(out), _stream()) == EINVAL  # a foreign handle
    with pytest.raises(ValueError):
        ep(torch.zeros(1, 944, 4, 4))
    with pytest.raises(ValueError):
        ep.forward_segments([x[:, :8], x[:, 8:]])  # a segment that is no multiple of 16
    # H = 1 or W = 1 on the 3x3 modules: refused on the host, nothing is launched
    x32 = torch.randn(1, 352, 1, 8, device="cuda")
    assert L.rgbd_channel_context_forward(cc._h, _p(x32), 1, 1, 8, _p(out), _stream()) == EINVAL
    assert L.rgbd_channel_context_forward(cc._h, _p(x32), 1, 8, 1, _p(out), _stream()) == EINVAL
    assert L.rgbd_lrp_forward(lrp._h, _p(x32), 1, 1, 8, _p(out), _stream()) == EINVAL
    assert L.rgbd_lrp_forward(lrp._h, _p(x32), 1, 8, 1, _p(out), _stream()) == EINVAL
    with pytest.raises(ValueError):
        cc(torch.zeros(1, 32, 1, 8))
    with pytest.raises(ValueError):
        lrp(torch.zeros(1, 352, 8, 1))
    # a forward of another family, the switch and the codec calls on these handles
    assert L.rgbd_lrp_forward(cc._h, _p(x32), 1, 4, 4, _p(out), _stream()) == EINVAL
    assert L.rgbd_channel_context_forward(ep._h, _p(x32), 1, 4, 4, _p(out), _stream()) == EINVAL
    assert L.rgbd_local_context_forward(lrp._h, _p(x32), 1, 4, 4, _p(out), _stream()) == EINVAL
    assert L.rgbd_entropy_params_mlic_set_fused(cc._h, 0) == EINVAL
    assert L.rgbd_entropy_params_mlic_set_fused(ep._h, 2) == EINVAL
    for m in (ep, cc, lrp):
        assert L.rgbd_elic_compress_single(m._h, _p(x), 1, 64, 64, 0, _stream()) == EINVAL
        assert L.rgbd_elic_set_coder(m._h, 1, 64) == EINVAL
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ---- the fused kernel alone ---------------------------------------------------------------------------------------------------
class Mlp:
    """The packed weights of one parameter network on the device, and rgbd_pixel_mlp4 over NHWC tensors."""

    def __init__(self, L, mod):
        self.L, sd = L, mc.module_weights(mod)
        f32p = ctypes.POINTER(ctypes.c_float)
        self.w, self.b = [], []
        for i in range(4):
            w = sd[f"fusion.{2 * i}.weight"].numpy().reshape(sd[f"fusion.{2 * i}.weight"].shape[:2]).copy()
            packed = np.empty(w.size, dtype=np.float32)
            assert L.rgbd_pixel_mlp4_pack(w.ctypes.data_as(f32p), w.shape[0], w.shape[1], packed.ctypes.data_as(f32p)) == 0
            self.w.append(torch.from_numpy(packed).cuda())
            self.b.append(sd[f"fusion.{2 * i}.bias"].cuda())
        self.out_dim = self.b[3].numel()

    def run(self, segs, parity=-1, out=None, opad=0, channels=None, strides=None):
        """segs: NHWC device tensors [B,H,W,cs_i]; returns the NHWC output (with opad sentinel channels behind it)."""
        B, H, W = segs[0].shape[:3]
        if out is None:
            out = torch.full((B, H, W, self.out_dim + opad), SENTINEL, device="cuda")
        n = len(segs)
        rc = self.L.rgbd_pixel_mlp4((ctypes.c_void_p * n)(*[t.data_ptr() for t in segs]),
                                    (ctypes.c_int32 * n)(*(channels or [t.shape[3] for t in segs])),
                                    (ctypes.c_int32 * n)(*(strides or [t.shape[3] for t in segs])), n,
                                    (ctypes.c_void_p * 4)(*[t.data_ptr() for t in self.w]),
                                    (ctypes.c_void_p * 4)(*[t.data_ptr() for t in self.b]), self.out_dim, B, H, W, parity,
                                    _p(out), out.shape[3], _stream())
        torch.cuda.synchronize()
        return rc, out


def _nhwc(name):
    return [t.permute(0, 2, 3, 1).contiguous().cuda() for t in mc.case_inputs(name)]


@pytest.mark.parametrize("mod", EP)
@pytest.mark.parametrize("size", ["4x4", "8x12", "4x20"])
def test_kernel_segments_batch_and_reference(mod, size):
    L = _lib()
    name = f"{mod}_{size}"
    mlp = Mlp(L, mod)
    segs = _nhwc(name)
    whole = torch.cat(segs, dim=3).contiguous()
    rc, full = mlp.run([whole])
    assert rc == 0
    fx = mc.load_fixture(name)
    e = mc.rel_err(full.permute(0, 3, 1, 2).cpu(), torch.from_numpy(fx["ref64"]))
    print(f"pixel_mlp4 {name}: e_gpu {e:.3e}, e_ref {mc.e_ref(fx, 3):.3e}, ratio {e / mc.e_ref(fx, 3):.2f}")
    assert e <= mc.FACTOR * mc.e_ref(fx, 3)
    # the codec's segments, each a tensor of its own; then as channel views of a wider buffer whose other channels are NaN
    rc, cut = mlp.run(segs, opad=16)
    assert rc == 0 and _bits(cut[..., :mlp.out_dim], full) and (cut[..., mlp.out_dim:] == SENTINEL).all()
    wide = [torch.full(t.shape[:3] + (t.shape[3] + 16,), float("nan"), device="cuda") for t in segs]
    for wd, t in zip(wide, segs):
        wd[..., :t.shape[3]] = t
    rc, strided = mlp.run(wide, channels=[t.shape[3] for t in segs])
    assert rc == 0 and _bits(strided, full)
    assert _bits(mlp.run([whole])[1], full)
    for b in range(3):
        assert _bits(mlp.run([t[b:b + 1].contiguous() for t in segs])[1], full[b:b + 1])


@pytest.mark.parametrize("size", ["4x4", "8x12", "12x8", "4x20"])
def test_kernel_parity_halves(size):
    L = _lib()
    name = f"ep960_{size}"
    mlp = Mlp(L, "ep960")
    segs = _nhwc(name)
    _, full = mlp.run(segs)
    H, W = full.shape[1:3]
    am = mc.anchor_map(H, W).cuda()
    for parity, sel in ((0, am), (1, ~am)):
        rc, half = mlp.run(segs, parity=parity, opad=16)
        assert rc == 0
        assert _bits(half[:, sel][..., :64], full[:, sel])
        assert (half[:, ~sel] == SENTINEL).all() and (half[..., 64:] == SENTINEL).all()
    # anchor half, then the other half into the same tensor: the full call
    _, both = mlp.run(segs, parity=0)
    assert mlp.run(segs, parity=1, out=both)[0] == 0 and _bits(both, full)


def test_kernel_sweep_size_and_small_widths():
    L = _lib()
    mlp = Mlp(L, "ep960")
    segs = _nhwc("ep960_32x40")
    fx = mc.load_fixture("ep960_32x40")
    rc, full = mlp.run(segs)
    assert rc == 0
    e = mc.rel_err(full.permute(0, 3, 1, 2).cpu(), torch.from_numpy(fx["ref64"]))
    print(f"pixel_mlp4 ep960_32x40: e_gpu {e:.3e}, e_ref {mc.e_ref(fx, 2):.3e}, ratio {e / mc.e_ref(fx, 2):.2f}")
    assert e <= mc.FACTOR * mc.e_ref(fx, 2)
    assert _bits(mlp.run([t[1:].contiguous() for t in segs])[1], full[1:])
    # the narrowest shapes the entry point takes: in_dim 16, out_dim 16 (one output tile: three of the four waves idle)
    g = torch.Generator().manual_seed(5)
    ws = [torch.randn(co, ci, generator=g) / ci ** 0.5 for ci, co in ((16, 320), (320, 256), (256, 128), (128, 16))]
    bs = [torch.randn(w.shape[0], generator=g) for w in ws]
    x = torch.randn(2, 3, 5, 16, generator=g)
    t = x.double()
    for i, (w, b) in enumerate(zip(ws, bs)):
        t = t @ w.double().t() + b.double()
        t = torch.nn.functional.gelu(t) if i < 3 else t
    f32p = ctypes.POINTER(ctypes.c_float)
    mlp.w, mlp.b, mlp.out_dim = [], [b.cuda() for b in bs], 16
    for w in ws:
        packed = np.empty(w.numel(), dtype=np.float32)
        wn = w.numpy().copy()
        assert L.rgbd_pixel_mlp4_pack(wn.ctypes.data_as(f32p), w.shape[0], w.shape[1], packed.ctypes.data_as(f32p)) == 0
        mlp.w.append(torch.from_numpy(packed).cuda())
    rc, out = mlp.run([x.cuda()])
    assert rc == 0
    t32 = x
    for i, (w, b) in enumerate(zip(ws, bs)):
        t32 = t32 @ w.t() + b
        t32 = torch.nn.functional.gelu(t32) if i < 3 else t32
    e, e32 = mc.rel_err(out.cpu(), t), mc.rel_err(t32, t)
    print(f"pixel_mlp4 16 -> 16 on 2x3x5: e_gpu {e:.3e}, e32 {e32:.3e}")
    assert e <= mc.FACTOR * e32


def test_kernel_rejects_bad_arguments():
    L = _lib()
    mlp = Mlp(L, "ep704")
    segs = _nhwc("ep704_4x4")
    out = torch.full((3, 4, 4, 80), SENTINEL, device="cuda")
    x = segs[1]
    bad = [dict(segs=[x[..., :16].contiguous()] * 7), dict(segs=segs, channels=[64, 632]), dict(segs=segs, channels=[64, 648]),
           dict(segs=segs, strides=[64, 642]), dict(segs=segs, parity=2), dict(segs=segs, parity=-2),
           dict(segs=[t[:, :, :3].contiguous() for t in segs], parity=0),  # odd W
           dict(segs=[torch.cat([x, x], dim=3)])]  # in_dim 1280
    for kw in bad:
        assert mlp.run(out=out, **kw)[0] == EINVAL, {k: v for k, v in kw.items() if k != "segs"}
    keep = mlp.out_dim
    for od in (0, 8, 144):
        mlp.out_dim = od
        assert mlp.run(segs, out=out)[0] == EINVAL
    mlp.out_dim = keep
    narrow = torch.full((3, 4, 4, 48), SENTINEL, device="cuda")
    assert mlp.run(segs, out=narrow)[0] == EINVAL  # out_stride < out_dim
    assert (out == SENTINEL).all() and (narrow == SENTINEL).all()
    rc, _ = mlp.run(segs, out=out)
    assert rc == 0 and not (out[..., :64] == SENTINEL).any() and (out[..., 64:] == SENTINEL).all()
