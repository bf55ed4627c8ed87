"""Torch-CPU functional restatement of MLIC++ (reference: models/mlicpp.py) over a plain state_dict, for the tests of
`rgbd_amd.mlic`: fp32 by default, fp64 with dtype=torch.float64.  The attention contexts and the per-slice networks are the
statements of tests/mlic_context_cases.py and tests/mlic_slice_cases.py under the codec's name prefixes; the factorised prior,
the Gaussian tables, the checkerboard packing and the rANS coder come from `oracle/`; GDN is tests/ckbd_ref.py's.  What is
stated here is what only this model has: its residual blocks (GELU / ReLU), the hyper transforms, and the slice loop.

The two attention cores are stated a second time here, operation by operation in the reference's order (unfold and batched
matrix products where tests/mlic_context_cases.py has einsums over gathered windows): in fp32 the sum order of a product decides
the last bit, and the fp32 run is to take the reference's decisions exactly.  The einsum statements remain the yardstick of the
two functions below (test_mlic_cpu.py holds them together in fp64).

`mistake` selects one deliberate error (MISTAKES): the tests require each of them to change the symbols of every fixture.
`trace` (a dict, when set) receives y, z, zhat, hyper, yhat, symbols / indexes / x (= y - mean) / sigma in stream order,
z_symbols, and pretanh: the largest |argument| of every LRP's tanh, in call order.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mlic_context_cases as cc  # noqa: E402
import mlic_slice_cases as sc  # noqa: E402
from ckbd_ref import PEDESTAL, anchor_mask  # noqa: E402
from oracle import coder  # noqa: E402
from oracle import elic_oracle as eo  # noqa: E402

MISTAKES = ("no_anchor_zeros",       # the anchor pass's LRP, local and intra contexts see the whole slice
            "lrp_both_parities",     # the LRP correction added at every pixel
            "lrp_uncorrected_anchor",  # the non-anchor LRP reads the anchors before their correction
            "inter_channel_exchanged",  # the two segments exchanged in front of the parameter networks
            "lrp_hyper_scales",      # hyper_scales instead of hyper_means in the LRP input
            "intra_first_slice",     # y_hat_slices[0] instead of [-1] for the intra context
            "stride_leaky")          # LeakyReLU instead of GELU in ResidualBlockWithStride
C = 32  # channels per slice


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def conv(sd, name, x, stride=1, pad=None):
    w = sd[name + ".weight"]
    return F.conv2d(x, w, sd[name + ".bias"], stride=stride, padding=w.shape[-1] // 2 if pad is None else pad)


def parametrize(raw, minimum):  # ops/parametrizers.py:21-45 (fp32 buffers; exact in fp64 as well)
    bound = torch.tensor([(minimum + PEDESTAL) ** 0.5], dtype=torch.float32).to(raw.dtype)
    return torch.max(raw, bound) ** 2 - torch.tensor([PEDESTAL], dtype=torch.float32).to(raw.dtype)


def gdn(sd, p, x, inverse=False):  # layers/gdn.py:52-67
    n = x.shape[1]
    beta, gamma = parametrize(sd[p + ".beta"], 1e-6), parametrize(sd[p + ".gamma"], 0.0)
    norm = F.conv2d(x ** 2, gamma.reshape(n, n, 1, 1), beta)
    return x * (torch.sqrt(norm) if inverse else torch.rsqrt(norm))


def res_block(sd, p, x):  # res_blk.py:30-58
    out = torch.relu(conv(sd, p + ".conv2", torch.relu(conv(sd, p + ".conv1", x))))
    return out + (conv(sd, p + ".skip", x) if p + ".skip.weight" in sd else x)


def res_block_stride(sd, p, x, mistake=None):  # res_blk.py:61-91
    act = F.leaky_relu if mistake == "stride_leaky" else F.gelu
    out = conv(sd, p + ".conv2", act(conv(sd, p + ".conv1", x, stride=2)))
    return gdn(sd, p + ".gdn", out) + conv(sd, p + ".skip", x, stride=2)


def res_block_up(sd, p, x):  # res_blk.py:94-119
    out = F.gelu(F.pixel_shuffle(conv(sd, p + ".subpel_conv.0", x), 2))
    out = gdn(sd, p + ".igdn", conv(sd, p + ".conv", out), inverse=True)
    return out + F.pixel_shuffle(conv(sd, p + ".upsample.0", x), 2)


def g_a(sd, x, mistake=None):  # analysis.py:11-26
    r = "g_a.analysis_transform."
    for i in range(3):
        x = res_block(sd, f"{r}{2 * i + 1}", res_block_stride(sd, f"{r}{2 * i}", x, mistake))
    return conv(sd, r + "6", x, stride=2)


def g_s(sd, y):  # synthesis.py:12-29
    r = "g_s.synthesis_transform."
    for i in range(3):
        y = res_block_up(sd, f"{r}{2 * i + 1}", res_block(sd, f"{r}{2 * i}", y))
    return F.pixel_shuffle(conv(sd, r + "7.0", res_block(sd, r + "6", y)), 2)


def h_a(sd, y):  # analysis.py:180-204
    t = y
    for k, stride in enumerate((1, 1, 2, 1, 2)):
        t = conv(sd, f"h_a.reduction.{2 * k}", t, stride=stride)
        if k < 4:
            t = F.gelu(t)
    return t


def h_s(sd, zhat):  # synthesis.py:248-273
    t = F.gelu(conv(sd, "h_s.increase.0", zhat))
    t = F.gelu(F.pixel_shuffle(conv(sd, "h_s.increase.2.0", t), 2))
    t = F.gelu(conv(sd, "h_s.increase.4", t))
    t = F.gelu(F.pixel_shuffle(conv(sd, "h_s.increase.6.0", t), 2))
    return conv(sd, "h_s.increase.8", t)


def local_context(sd, x):  # context.py:58-137
    B, n, H, W = x.shape
    L, ws, heads, hd, dt = H * W, 5, 2, n // 2, x.dtype
    lin = lambda t, p: F.linear(t, sd[p + ".weight"], sd[p + ".bias"])  # noqa: E731
    ln = lambda t, p: F.layer_norm(t, (t.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], 1e-5)  # noqa: E731
    unfold = lambda t: F.unfold(t, kernel_size=ws, stride=1, padding=2)  # noqa: E731
    ck = torch.zeros(1, 2, H, W, dtype=dt)  # :65-78: the mask lets a window's anchors see each other and nothing else
    ck[:, :, 0::2, 1::2] = 1
    ck[:, :, 1::2, 0::2] = 1
    qk = unfold(ck).permute(0, 2, 1).view(1, L, 2, 1, ws, ws).permute(2, 0, 1, 3, 4, 5)
    mq, mk = (t.reshape(1, L, 1, ws * ws).permute(0, 1, 3, 2) for t in (qk[0], qk[1]))
    mask = mq @ mk.transpose(-2, -1)
    mask = mask.masked_fill(mask == 0.0, -100.0).masked_fill(mask == 1, 0.0)[0]
    t = ln(x.reshape(B, n, L).permute(0, 2, 1), "norm1")
    qkv = lin(t, "qkv_proj").reshape(B, H, W, 3, n).permute(3, 0, 4, 1, 2)
    win = unfold(torch.cat([qkv[0], qkv[1], qkv[2]], dim=1)).permute(0, 2, 1).view(B, L, 3, n, ws, ws).permute(2, 0, 1, 3, 4, 5)
    q, k, v = (win[i].reshape(B, L, hd, heads, ws * ws).permute(0, 1, 3, 4, 2) for i in range(3))
    attn = (q * hd ** -0.5) @ k.transpose(-2, -1)
    bias = sd["relative_position_table"][sd["relative_position_index"].view(-1)].view(ws * ws, ws * ws, -1).permute(2, 0, 1).contiguous()
    attn = torch.softmax(attn + bias.unsqueeze(0).unsqueeze(1) + mask.unsqueeze(0).unsqueeze(2), dim=-1)
    o = (attn @ v).reshape(B, L, heads, ws, ws, hd).permute(0, 1, 3, 4, 2, 5).reshape(B * L, ws, ws, n).permute(0, 3, 1, 2)
    o = lin(F.conv2d(o, sd["fusion.weight"], sd["fusion.bias"]).reshape(B, L, 2 * n), "proj")
    o = o + lin(F.gelu(lin(ln(o, "norm2"), "mlp.fc1")), "mlp.fc2")
    return o.permute(0, 2, 1).reshape(B, 2 * n, H, W)


def linear_context(sd, x1, x2, heads):
    """x2 None: LinearGlobalInterContext.forward (context.py:243-262); else LinearGlobalIntraContext.forward (:189-213)."""
    B, n, H, W = x1.shape
    dt = x1.dtype
    cv = lambda t, p, **kw: F.conv2d(t, sd[p + ".weight"], sd[p + ".bias"], **kw)  # noqa: E731
    br = lambda t, p: cv(cv(t, p + ".0"), p + ".1", padding=1, groups=n)  # noqa: E731
    hd, outs = n // heads, []
    if x2 is None:
        queries, keys, values = (br(x1, p).reshape(B, n, H * W) for p in ("queries", "keys", "values"))
    else:
        am = anchor_mask(H, W)
        zero = torch.zeros((), dtype=dt)
        queries = eo.pack(br(torch.where(am, zero, x1), "queries"), False).reshape(B, n, H * W // 2)
        keys = eo.pack(br(torch.where(am, x1, zero), "keys"), True).reshape(B, n, H * W // 2)
        values = eo.pack(br(x2, "values"), True).reshape(B, n, H * W // 2)
    for i in range(heads):
        key = F.softmax(keys[:, i * hd:(i + 1) * hd, :], dim=2)
        query = F.softmax(queries[:, i * hd:(i + 1) * hd, :], dim=1)
        value = values[:, i * hd:(i + 1) * hd, :]
        if x2 is not None:  # back on the full grid, zeros at the other parity (:203-205)
            key = eo.unpack(key.reshape(B, hd, H, W // 2), True).reshape(B, hd, H * W)
            value = eo.unpack(value.reshape(B, hd, H, W // 2), True).reshape(B, hd, H * W)
            query = eo.unpack(query.reshape(B, hd, H, W // 2), False).reshape(B, hd, H * W)
        context = key @ value.transpose(1, 2)
        outs.append((context.transpose(1, 2) @ query).reshape(B, hd, H, W))
    att = cv(torch.cat(outs, dim=1), "reprojection", padding=2)
    m = cv(F.gelu(cv(F.gelu(cv(att, "mlp.0")), "mlp.2", padding=1, groups=sd["mlp.2.weight"].shape[0])), "mlp.4")
    return (cv(att, "skip") if x2 is None else att) + m


class MlicRef:
    def __init__(self, state_dict, dtype=torch.float32, mistake=None):
        assert mistake is None or mistake in MISTAKES, mistake
        self.dtype, self.mistake = dtype, mistake
        self.sd32 = {k: v.detach().to(torch.float32) if v.is_floating_point() else v for k, v in state_dict.items()}
        self.sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in self.sd32.items()}
        self.M = int(self.sd["g_a.analysis_transform.6.weight"].shape[0])
        self.S = self.M // C
        self.table = eo.scale_table()
        self.gc = self.eb = self.trace = None

    def update(self):
        self.gc = eo.gaussian_tables(self.table)
        self.eb = eo.bottleneck_tables(self.sd32, "entropy_bottleneck")
        return True

    def _median(self):
        return self.sd["entropy_bottleneck.quantiles"][:, :, 1:2].reshape(1, -1, 1, 1)

    def z_symbols(self, z):
        return torch.round(z - self._median()).int()

    def z_compress(self, z):  # entropy_models.py:195-224, 431-440
        sym = self.z_symbols(z)
        n = z.shape[1]
        idx = torch.arange(n, dtype=torch.int32).view(1, n, 1, 1).expand_as(sym)
        if self.trace is not None:
            self.trace["z_symbols"] = sym.clone()
        return [coder.rans_encode(sym[i].reshape(-1).numpy(), idx[i].reshape(-1).numpy(), self.eb) for i in range(z.shape[0])], sym

    def z_decompress(self, strings, shape):
        n = self.eb.cdf.shape[0]
        idx = torch.arange(n, dtype=torch.int32).view(n, 1, 1).expand(n, shape[0], shape[1]).reshape(-1).numpy()
        outs = [torch.from_numpy(coder.rans_decode(s, idx, self.eb).astype(np.float32)).reshape(n, shape[0], shape[1]) for s in strings]
        return torch.stack(outs).to(self.dtype) + self._median()

    # ---- the networks of slice i under their prefixes ---------------------------------------------------------------------
    def _net(self, kind, i):
        return sub(self.sd, f"{kind}.{i}.")

    def slice_loop(self, y, hyper, dec=None, forced=None, estimate=False):
        """mlicpp.py:220-303 (encode: y given), :331-404 (decode: dec = a RansDecoder on the y stream), :105-182 (estimate: the
        eval forward, returns likelihoods instead of symbols).  forced: symbols in stream order that y_hat is rebuilt from."""
        dt, mk, tr = self.dtype, self.mistake, self.trace
        B, _, h, w = hyper.shape
        hyper_scales, hyper_means = hyper.chunk(2, 1)
        am = anchor_mask(h, w)
        part_n = B * C * h * (w // 2)
        slices, syms, idxs, xs, sgs, liks, pretanh = [], [], [], [], [], [], []
        table = self.table.to(dt)
        pos = 0

        def code(y_slice, scales, means, anchor):
            """One part: returns the part's y_hat (zero off its parity), as compress_anchor / compress_nonanchor do."""
            nonlocal pos
            sq, mq = eo.pack(scales, anchor), eo.pack(means, anchor)
            if estimate:
                return torch.where(am if anchor else ~am, torch.round(y_slice - means) + means, torch.zeros((), dtype=dt))
            idx = torch.searchsorted(table[:-1].contiguous(), torch.clamp(sq, min=0.11).contiguous(), right=False).int()
            if y_slice is not None:
                yq = eo.pack(y_slice, anchor)
                sym = torch.round(yq - mq).int()
                xs.append((yq - mq).reshape(-1).numpy())
            else:
                sym = torch.from_numpy(dec.decode_stream(idx.reshape(-1).numpy(), self.gc)).reshape(idx.shape)
            syms.append(sym.reshape(-1).numpy().astype(np.int32))
            idxs.append(idx.reshape(-1).numpy().astype(np.int32))
            sgs.append(sq.reshape(-1).numpy())
            use = sym if forced is None else torch.from_numpy(np.asarray(forced[pos:pos + part_n], np.int32)).reshape(sym.shape)
            pos += part_n
            return eo.unpack(use.to(dt) + mq, anchor)

        def lrp(kind, i, cur):
            first = hyper_scales if mk == "lrp_hyper_scales" else hyper_means
            return sc.lrp(self._net(kind, i), torch.cat([first] + slices + [cur], dim=1), dtype=dt, pretanh=pretanh)

        for i in range(self.S):
            ys = None if y is None else y[:, C * i:C * (i + 1)]
            inter = chan = None
            if i:
                prev = torch.cat(slices, dim=1)
                inter = linear_context(self._net("global_inter_context", i), prev, None, i)
                chan = sc.channel_context(self._net("channel_context", i), prev, dtype=dt)
            segs = [inter, chan, hyper] if i else [hyper]
            if mk == "inter_channel_exchanged" and i:
                segs = [chan, inter, hyper]
            sa, ma = sc.entropy_params(self._net("entropy_parameters_anchor", i), segs, dtype=dt).chunk(2, 1)
            anchor = code(ys, sa, ma, True)
            seen = anchor
            if mk == "no_anchor_zeros" and ys is not None:  # the other half of the slice is there too, unquantised
                seen = anchor + torch.where(am, torch.zeros((), dtype=dt), ys)
            r = lrp("lrp_anchor", i, seen)
            before = anchor
            anchor = anchor + (r if mk == "lrp_both_parities" else torch.where(am, r, torch.zeros((), dtype=dt)))
            seen = seen + (anchor - before)
            intra = None
            if i:
                last = slices[0] if mk == "intra_first_slice" else slices[-1]
                intra = linear_context(self._net("global_intra_context", i), last, seen, 2)
            local = local_context(self._net("local_context", i), seen)
            segs = [local, intra, inter, chan, hyper] if i else [local, hyper]
            if mk == "inter_channel_exchanged" and i:
                segs = [local, intra, chan, inter, hyper]
            sn, mn = sc.entropy_params(self._net("entropy_parameters_nonanchor", i), segs, dtype=dt).chunk(2, 1)
            non = code(ys, sn, mn, False)
            r = lrp("lrp_nonanchor", i, non + (before if mk == "lrp_uncorrected_anchor" else anchor))
            non = non + (r if mk == "lrp_both_parities" else torch.where(am, torch.zeros((), dtype=dt), r))
            slices.append(non + anchor)
            if estimate:  # entropy_models.py:534-558 on the merged parameters
                scales, means = torch.where(am, sa, sn), torch.where(am, ma, mn)
                val = torch.abs(torch.round(ys - means) + means - means)
                s_ = torch.clamp(scales, min=0.11)
                cst = float(-(2 ** -0.5))
                lik = 0.5 * torch.erfc(cst * ((0.5 - val) / s_)) - 0.5 * torch.erfc(cst * ((-0.5 - val) / s_))
                liks.append(torch.clamp(lik, min=1e-9))
        yhat = torch.cat(slices, dim=1)
        if tr is not None:
            tr.update({"yhat": yhat, "pretanh": pretanh})
            if sgs:
                tr["sigma"] = np.concatenate(sgs)
            if xs:
                tr["x"] = np.concatenate(xs)
        if estimate:
            return yhat, torch.cat(liks, dim=1)
        return yhat, np.concatenate(syms), np.concatenate(idxs)

    @torch.no_grad()
    def compress(self, x, forced_y=None, forced_z=None):  # mlicpp.py:199-312
        x = x.to(self.dtype)
        y = g_a(self.sd, x, self.mistake)
        z = h_a(self.sd, y)
        zs, zsym = self.z_compress(z)
        if forced_z is not None:
            zsym = torch.from_numpy(np.asarray(forced_z, np.int32)).reshape(z.shape)
        zhat = zsym.to(self.dtype) + self._median()
        hyper = h_s(self.sd, zhat)
        yhat, sym, idx = self.slice_loop(y, hyper, forced=forced_y)
        ys = coder.rans_encode(sym, idx, self.gc)
        if self.trace is not None:
            self.trace.update({"y": y, "z": z, "zhat": zhat, "hyper": hyper, "symbols": sym, "indexes": idx})
        return {"strings": [[ys], zs], "shape": tuple(z.shape[-2:])}

    @torch.no_grad()
    def decompress(self, strings, shape):  # mlicpp.py:314-413 (x_hat is not clamped)
        zhat = self.z_decompress(strings[1], shape)
        hyper = h_s(self.sd, zhat)
        dec = coder.RansDecoder()
        dec.set_stream(strings[0][0])
        yhat, sym, idx = self.slice_loop(None, hyper, dec=dec)
        return {"x_hat": g_s(self.sd, yhat)}

    @torch.no_grad()
    def forward(self, x):  # mlicpp.py:77-188 (eval mode)
        sd = self.sd
        x = x.to(self.dtype)
        y = g_a(sd, x, self.mistake)
        z = h_a(sd, y)
        med = self._median()
        zhat = torch.round(z - med) + med
        B, n = z.shape[:2]  # entropy_models.py:369-428 on the quantised z
        v = zhat.permute(1, 0, 2, 3).reshape(n, 1, -1)
        lower, upper = eo._eb_logits(sd, "entropy_bottleneck", v - 0.5), eo._eb_logits(sd, "entropy_bottleneck", v + 0.5)
        sign = -torch.sign(lower + upper)
        zl = torch.abs(torch.sigmoid(sign * upper) - torch.sigmoid(sign * lower)).clamp(min=1e-9)
        zl = zl.reshape(n, B, *z.shape[2:]).permute(1, 0, 2, 3)
        yhat, lik = self.slice_loop(y, h_s(sd, zhat), estimate=True)
        if self.trace is not None:
            self.trace.update({"y": y, "z": z, "zhat": zhat})
        return {"x_hat": g_s(sd, yhat), "likelihoods": {"y_likelihoods": lik, "z_likelihoods": zl}}
