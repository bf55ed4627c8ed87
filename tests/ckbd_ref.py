"""Torch-CPU functional restatement of the checkerboard Cheng2020 model (reference: models/Cheng2020withCKBD.py:40-265 on
CompressAI/compressai/models/waseda.py:22-81) over a plain state_dict, for the tests of `rgbd_amd.ckbd`.  The factorised
prior, the Gaussian tables, the checkerboard packing and the rANS coder come from `oracle/` (elic_oracle.py, coder.py); what
is stated here is what only this model has: GDN / IGDN, its residual blocks, and the two-pass entropy model with the masked
5x5 context convolution.  Every function cites the reference lines it restates.

`trace` (a dict, when set) receives y, z, zhat, hyper, yhat, ctx (the context convolution's output: whole grid; meaningful at
non-anchor positions), means / scales (anchor pass at anchor positions, non-anchor pass elsewhere), symbols / indexes in
stream order, x (= y - mean per symbol) and sigma (the scale per symbol) in stream order, z_symbols.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from oracle import coder  # noqa: E402
from oracle import elic_oracle as eo  # noqa: E402

PEDESTAL = (2.0 ** -18) ** 2


def parametrize(raw, minimum):  # ops/parametrizers.py:21-45: lower bound, square, subtract the pedestal (fp32)
    bound = torch.tensor([(minimum + PEDESTAL) ** 0.5], dtype=torch.float32)
    return torch.max(raw, bound) ** 2 - torch.tensor([PEDESTAL], dtype=torch.float32)


def gdn(sd, p, x, inverse=False):  # layers/gdn.py:52-67
    C = x.shape[1]
    beta, gamma = parametrize(sd[p + ".beta"], 1e-6), parametrize(sd[p + ".gamma"], 0.0)
    norm = F.conv2d(x ** 2, gamma.reshape(C, C, 1, 1), beta)
    return x * (torch.sqrt(norm) if inverse else torch.rsqrt(norm))


def res_block(sd, p, x):  # layers.py:129-159
    out = F.leaky_relu(eo._conv(sd, p + ".conv1", x))
    return F.leaky_relu(eo._conv(sd, p + ".conv2", out)) + x


def res_block_stride(sd, p, x):  # layers.py:67-98
    out = eo._conv(sd, p + ".conv2", F.leaky_relu(eo._conv(sd, p + ".conv1", x, stride=2)))
    return gdn(sd, p + ".gdn", out) + eo._conv(sd, p + ".skip", x, stride=2)


def res_block_up(sd, p, x):  # layers.py:101-126
    out = F.leaky_relu(F.pixel_shuffle(eo._conv(sd, p + ".subpel_conv.0", x), 2))
    out = gdn(sd, p + ".igdn", eo._conv(sd, p + ".conv", out), inverse=True)
    return out + F.pixel_shuffle(eo._conv(sd, p + ".upsample.0", x), 2)


def g_a(sd, x):  # waseda.py:38-46
    for i in range(3):
        x = res_block(sd, f"g_a.{2 * i + 1}", res_block_stride(sd, f"g_a.{2 * i}", x))
    return eo._conv(sd, "g_a.6", x, stride=2)


def g_s(sd, y):  # waseda.py:72-81
    for i in range(3):
        y = res_block_up(sd, f"g_s.{2 * i + 1}", res_block(sd, f"g_s.{2 * i}", y))
    return F.pixel_shuffle(eo._conv(sd, "g_s.7.0", res_block(sd, "g_s.6", y)), 2)


def h_a(sd, y):  # waseda.py:48-58
    t = y
    for k, stride in enumerate((1, 1, 2, 1, 2)):
        t = eo._conv(sd, f"h_a.{2 * k}", t, stride=stride)
        if k < 4:
            t = F.leaky_relu(t)
    return t


def h_s(sd, zhat):  # waseda.py:60-70
    t = F.leaky_relu(eo._conv(sd, "h_s.0", zhat))
    t = F.leaky_relu(F.pixel_shuffle(eo._conv(sd, "h_s.2.0", t), 2))
    t = F.leaky_relu(eo._conv(sd, "h_s.4", t))
    t = F.leaky_relu(F.pixel_shuffle(eo._conv(sd, "h_s.6.0", t), 2))
    return eo._conv(sd, "h_s.8", t)


def context_mask(w):  # Cheng2020withCKBD.py:28-31: the taps with (ky + kx) odd survive
    m = torch.zeros_like(w)
    m[:, :, 0::2, 1::2] = 1
    m[:, :, 1::2, 0::2] = 1
    return m


def context(sd, yhat):  # Cheng2020withCKBD.py:33-37 (the reference masks the weight in place at every call)
    w = sd["context_prediction.weight"]
    return F.conv2d(yhat, w * context_mask(w), sd["context_prediction.bias"], padding=2)


def entropy_parameters(sd, x):  # priors.py:403-409
    t = F.leaky_relu(eo._conv(sd, "entropy_parameters.0", x))
    t = F.leaky_relu(eo._conv(sd, "entropy_parameters.2", t))
    return eo._conv(sd, "entropy_parameters.4", t)


def anchor_mask(h, w):  # [0::2, 1::2] and [1::2, 0::2]: (row + col) odd
    r, c = torch.arange(h)[:, None], torch.arange(w)[None, :]
    return ((r + c) % 2 == 1)


class CkbdRef:
    def __init__(self, state_dict):
        self.sd = {k: v.detach().to(torch.float32) if v.is_floating_point() else v for k, v in state_dict.items()}
        self.M = int(self.sd["g_a.6.weight"].shape[0])
        self.table = eo.scale_table()
        self.gc = None
        self.eb = None
        self.trace = None

    def update(self):  # Cheng2020withCKBD.py:260-265
        self.gc = eo.gaussian_tables(self.table)
        self.eb = eo.bottleneck_tables(self.sd, "entropy_bottleneck")
        return True

    def _median(self):
        return self.sd["entropy_bottleneck.quantiles"][:, :, 1:2].reshape(1, -1, 1, 1)

    def z_compress(self, z):  # entropy_models.py:195-224, 431-440: one stream per image, (c, row, col) order
        sym = torch.round(z - self._median()).int()
        c = z.shape[1]
        idx = torch.arange(c, dtype=torch.int32).view(1, c, 1, 1).expand_as(sym)
        if self.trace is not None:
            self.trace["z_symbols"] = sym.clone()
        return [coder.rans_encode(sym[i].reshape(-1).numpy(), idx[i].reshape(-1).numpy(), self.eb) for i in range(z.shape[0])]

    def z_decompress(self, strings, shape):  # entropy_models.py:226-266, 442-446
        c = self.eb.cdf.shape[0]
        idx = torch.arange(c, dtype=torch.int32).view(c, 1, 1).expand(c, shape[0], shape[1]).reshape(-1).numpy()
        outs = [torch.from_numpy(coder.rans_decode(s, idx, self.eb).astype(np.float32)).reshape(c, shape[0], shape[1])
                for s in strings]
        return torch.stack(outs) + self._median()

    def _params(self, ctx, hyper):  # :123-124 / :128-129: cat(ctx, hyper), chunk(2, 1) = (scales, means)
        return entropy_parameters(self.sd, torch.cat([ctx, hyper], dim=1)).chunk(2, 1)

    def two_pass(self, y, hyper, dec=None, forced=None):
        """Cheng2020withCKBD.py:121-130, 204-225 (encode: y given) and :154-167, 227-249 (decode: dec = a RansDecoder on the
        y stream).  forced: symbols in stream order that y_hat is rebuilt from (teacher forcing).  Returns (y_hat, symbols,
        indexes): both halves of the whole batch in stream order, anchor half first."""
        tr = self.trace
        B, _, h, w = hyper.shape
        half = B * self.M * h * (w // 2)
        yhat = torch.zeros(B, self.M, h, w)
        syms, idxs, xs, sgs = [], [], [], []
        ctx = torch.zeros(B, 2 * self.M, h, w)
        full_s, full_m = torch.zeros(B, self.M, h, w), torch.zeros(B, self.M, h, w)
        for part, anchor in enumerate((True, False)):
            if not anchor:
                ctx = context(self.sd, yhat)
            scales, means = self._params(ctx, hyper)
            sq, mq = eo.pack(scales, anchor), eo.pack(means, anchor)
            idx = eo.scale_indexes(sq, self.table)
            if y is not None:
                yq = eo.pack(y, anchor)
                sym = eo.quantize_symbols(yq, mq)
                xs.append((yq - mq).reshape(-1).numpy())
            else:
                sym = torch.from_numpy(dec.decode_stream(idx.reshape(-1).numpy(), self.gc)).reshape(idx.shape)
            syms.append(sym.reshape(-1).numpy().astype(np.int32))
            idxs.append(idx.reshape(-1).numpy().astype(np.int32))
            sgs.append(sq.reshape(-1).numpy())
            use = sym if forced is None else torch.from_numpy(np.asarray(forced[part * half:(part + 1) * half], np.int32)).reshape(sym.shape)
            yhat = yhat + eo.unpack(use.float() + mq, anchor)
            am = anchor_mask(h, w) if anchor else ~anchor_mask(h, w)
            full_s = torch.where(am, scales, full_s)
            full_m = torch.where(am, means, full_m)
        if tr is not None:
            tr.update({"ctx": ctx, "scales": full_s, "means": full_m, "yhat": yhat, "sigma": np.concatenate(sgs)})
            if xs:
                tr["x"] = np.concatenate(xs)
        return yhat, np.concatenate(syms), np.concatenate(idxs)

    @torch.no_grad()
    def compress(self, x, forced_y=None, forced_z=None):  # Cheng2020withCKBD.py:101-136
        y = g_a(self.sd, x)
        z = h_a(self.sd, y)
        zs = self.z_compress(z)
        zhat = self.z_decompress(zs, z.shape[-2:])
        if forced_z is not None:
            zhat = torch.from_numpy(np.asarray(forced_z, np.float32)).reshape(z.shape) + self._median()
        hyper = h_s(self.sd, zhat)
        yhat, sym, idx = self.two_pass(y, hyper, forced=forced_y)
        ys = coder.rans_encode(sym, idx, self.gc)
        if self.trace is not None:
            self.trace.update({"y": y, "z": z, "zhat": zhat, "hyper": hyper, "symbols": sym, "indexes": idx})
        return {"strings": [[ys], zs], "shape": tuple(z.shape[-2:])}

    @torch.no_grad()
    def decompress(self, strings, shape):  # Cheng2020withCKBD.py:138-174 (x_hat is not clamped)
        zhat = self.z_decompress(strings[1], shape)
        hyper = h_s(self.sd, zhat)
        dec = coder.RansDecoder()
        dec.set_stream(strings[0][0])
        yhat, sym, idx = self.two_pass(None, hyper, dec=dec)
        if self.trace is not None:
            self.trace.update({"zhat": zhat, "hyper": hyper})
        return {"x_hat": g_s(self.sd, yhat)}

    @torch.no_grad()
    def forward(self, x):  # Cheng2020withCKBD.py:52-71 (eval mode)
        sd = self.sd
        y = g_a(sd, x)
        z = h_a(sd, y)
        med = self._median()
        zhat = torch.round(z - med) + med
        B, C = z.shape[:2]  # entropy_models.py:369-428 on the quantised z
        v = zhat.permute(1, 0, 2, 3).reshape(C, 1, -1)
        lower, upper = eo._eb_logits(sd, "entropy_bottleneck", v - 0.5), eo._eb_logits(sd, "entropy_bottleneck", v + 0.5)
        sign = -torch.sign(lower + upper)
        zl = torch.abs(torch.sigmoid(sign * upper) - torch.sigmoid(sign * lower)).clamp(min=1e-9)
        zl = zl.reshape(C, B, *z.shape[2:]).permute(1, 0, 2, 3)
        yhat = torch.round(y)  # quantize(y, "dequantize") without means
        hyper = h_s(sd, zhat)
        ctx = context(sd, yhat)
        ctx = torch.where(anchor_mask(*y.shape[-2:]), torch.zeros(()), ctx)  # :64-66: anchor outputs zeroed
        scales, means = self._params(ctx, hyper)
        out = torch.round(y - means) + means  # entropy_models.py:534-558
        val = torch.abs(out - means)
        sc = torch.clamp(scales, min=0.11)
        cst = float(-(2 ** -0.5))
        lik = 0.5 * torch.erfc(cst * ((0.5 - val) / sc)) - 0.5 * torch.erfc(cst * ((-0.5 - val) / sc))
        if self.trace is not None:
            self.trace.update({"y": y, "z": z, "zhat": zhat, "hyper": hyper, "yhat": yhat, "ctx": ctx, "scales": scales,
                               "means": means})
        return {"x_hat": g_s(sd, yhat), "likelihoods": {"y": torch.clamp(lik, min=1e-9), "z": zl}}
