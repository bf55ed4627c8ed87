"""Torch-CPU functional restatement of the single-modal STF (reference: models/stf.py:408-816, SymmetricalTransFormer) over
a plain state_dict, for the tests of `rgbd_amd.stf`.  Swin blocks, the factorised prior, the Gaussian tables and the rANS
coder come from `oracle/` (elic_oracle.py, coder.py); what is stated here is what only this model has: its hyper nets and
the 12-slice entropy loop with latent residual prediction.  Every function cites the reference lines it restates.

`trace` (a dict, when set) receives y, z, zhat, latent_means, latent_scales, yhat and per slice mu, sigma, symbols,
indexes, lrp (= 0.5 * tanh of the LRP net) and the slice's final y_hat.
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

NUM_SLICES, SLICE_CH, MAX_SUPPORT, M = 12, 32, 6, 384  # stf.py:418, 439, 630


def g_a(sd, x):  # stf.py:704-713 (patch_embed :372-405, BasicLayer / PatchMerging as in stf_united.py)
    x = F.conv2d(x, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=2)
    Wh, Ww = x.shape[2], x.shape[3]
    x = eo._ln(sd, "patch_embed.norm", x.flatten(2).transpose(1, 2))
    for i in range(4):
        x, Wh, Ww = eo._basic_layer(sd, f"layers.{i}", x, Wh, Ww, eo.STF_DEPTHS[i], eo.STF_HEADS[i], "merge" if i < 3 else None)
    return x.view(-1, Wh, Ww, M).permute(0, 3, 1, 2).contiguous()


def g_s(sd, yhat):  # stf.py:809-815 without the clamp
    B, C, Wh, Ww = yhat.shape
    x = yhat.permute(0, 2, 3, 1).contiguous().view(-1, Wh * Ww, C)
    for i in range(4):
        x, Wh, Ww = eo._basic_layer(sd, f"syn_layers.{i}", x, Wh, Ww, eo.STF_DEPTHS[::-1][i], eo.STF_HEADS[::-1][i],
                                    "split" if i < 3 else None)
    x = x.view(-1, Wh, Ww, eo.STF_EMBED).permute(0, 3, 1, 2).contiguous()
    return eo._conv(sd, "end_conv.2", F.pixel_shuffle(eo._conv(sd, "end_conv.0", x), 2))  # stf.py:496-500


def h_a(sd, y):  # stf.py:507-517: conv3x3 (stride 1, 1, 2, 1, 2) with GELU between
    t = y
    for k, stride in enumerate((1, 1, 2, 1, 2)):
        t = eo._conv(sd, f"h_a.{2 * k}", t, stride=stride)
        if k < 4:
            t = F.gelu(t)
    return t


def h_s(sd, fam, zhat):  # stf.py:519-540 (fam: h_mean_s / h_scale_s); subpel_conv3x3 = conv + PixelShuffle(2)
    t = F.gelu(eo._conv(sd, f"{fam}.0", zhat))
    t = F.gelu(F.pixel_shuffle(eo._conv(sd, f"{fam}.2.0", t), 2))
    t = F.gelu(eo._conv(sd, f"{fam}.4", t))
    t = F.gelu(F.pixel_shuffle(eo._conv(sd, f"{fam}.6.0", t), 2))
    return eo._conv(sd, f"{fam}.8", t)


def net5(sd, p, x):  # stf.py:541-582: five 3x3 convolutions with GELU between them
    for k in range(5):
        x = eo._conv(sd, f"{p}.{2 * k}", x)
        if k < 4:
            x = F.gelu(x)
    return x


def gc_likelihood(y, scales, means):  # entropy_models.py:534-558 (eval mode: quantize "dequantize" with the means)
    out = torch.round(y - means) + means
    v = torch.abs(out - means)
    sc = torch.clamp(scales, min=0.11)
    cst = float(-(2 ** -0.5))
    lik = 0.5 * torch.erfc(cst * ((0.5 - v) / sc)) - 0.5 * torch.erfc(cst * ((-0.5 - v) / sc))
    return torch.clamp(lik, min=1e-9)


class StfSingleRef:
    def __init__(self, state_dict):
        self.sd = {k: v.detach().to(torch.float32) if v.is_floating_point() else v for k, v in state_dict.items()}
        self.table = eo.scale_table()
        self.gc = None
        self.eb = None
        self.trace = None

    def update(self):  # stf.py:680-685
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

    def slice_loop(self, y, latent_means, latent_scales, dec=None, lik=None):
        """stf.py:735-758 (encode: y given), :786-807 (decode: dec = a RansDecoder on the y stream; one image, or a batch in
        the encoder's order -- the package's extension) and :647-667 (lik: a list that receives the likelihoods).
        Returns (y_hat, symbols, indexes) with symbols / indexes concatenated in stream order."""
        sd, yhat, syms, idxs = self.sd, [], [], []
        tr = self.trace
        for i in range(NUM_SLICES):
            support = yhat[:MAX_SUPPORT]
            mean_support = torch.cat([latent_means] + support, dim=1)
            mu = net5(sd, f"cc_mean_transforms.{i}", mean_support)
            scale = net5(sd, f"cc_scale_transforms.{i}", torch.cat([latent_scales] + support, dim=1))
            idx = eo.scale_indexes(scale, self.table)  # build_indexes on the raw net output
            if y is not None:
                ys = y[:, i * SLICE_CH:(i + 1) * SLICE_CH]
                sym = eo.quantize_symbols(ys, mu)
                if lik is not None:
                    lik.append(gc_likelihood(ys, scale, mu))
            else:
                sym = torch.from_numpy(dec.decode_stream(idx.reshape(-1).numpy(), self.gc)).reshape(idx.shape)
            syms.append(sym.reshape(-1).numpy().astype(np.int32))
            idxs.append(idx.reshape(-1).numpy().astype(np.int32))
            pre = sym.float() + mu
            lrp = 0.5 * torch.tanh(net5(sd, f"lrp_transforms.{i}", torch.cat([mean_support, pre], dim=1)))
            yh = pre + lrp
            yhat.append(yh)
            if tr is not None:
                tr.setdefault("slices", []).append({"mu": mu.clone(), "sigma": scale.clone(), "symbols": sym.clone(),
                                                    "indexes": idx.clone(), "lrp": lrp.clone(), "yhat": yh.clone()})
        return torch.cat(yhat, dim=1), np.concatenate(syms), np.concatenate(idxs)

    @torch.no_grad()
    def compress(self, x):  # stf.py:703-764
        y = g_a(self.sd, x)
        z = h_a(self.sd, y)
        zs = self.z_compress(z)
        zhat = self.z_decompress(zs, z.shape[-2:])
        lm, ls = h_s(self.sd, "h_mean_s", zhat), h_s(self.sd, "h_scale_s", zhat)
        yhat, sym, idx = self.slice_loop(y, lm, ls)
        ys = coder.rans_encode(sym, idx, self.gc)
        if self.trace is not None:
            self.trace.update({"y": y, "z": z, "zhat": zhat, "latent_means": lm, "latent_scales": ls, "yhat": yhat,
                               "symbols": sym, "indexes": idx})
        return {"strings": [[ys], zs], "shape": tuple(z.shape[-2:])}

    @torch.no_grad()
    def decompress(self, strings, shape):  # stf.py:766-816
        zhat = self.z_decompress(strings[1], shape)
        lm, ls = h_s(self.sd, "h_mean_s", zhat), h_s(self.sd, "h_scale_s", zhat)
        dec = coder.RansDecoder()
        dec.set_stream(strings[0][0])
        yhat, sym, idx = self.slice_loop(None, lm, ls, dec=dec)
        if self.trace is not None:
            self.trace.update({"zhat": zhat, "latent_means": lm, "latent_scales": ls, "yhat": yhat})
        return {"x_hat": g_s(self.sd, yhat).clamp_(0, 1)}

    @torch.no_grad()
    def forward(self, x):  # stf.py:618-678 (eval mode)
        sd = self.sd
        y = g_a(sd, x)
        z = h_a(sd, y)
        med = self._median()
        zhat = torch.round(z - med) + med
        # entropy_models.py:369-428 on the quantised z
        B, C = z.shape[:2]
        v = zhat.permute(1, 0, 2, 3).reshape(C, 1, -1)
        lower, upper = eo._eb_logits(sd, "entropy_bottleneck", v - 0.5), eo._eb_logits(sd, "entropy_bottleneck", v + 0.5)
        sign = -torch.sign(lower + upper)
        zl = torch.abs(torch.sigmoid(sign * upper) - torch.sigmoid(sign * lower)).clamp(min=1e-9)
        zl = zl.reshape(C, B, *z.shape[2:]).permute(1, 0, 2, 3)
        lm, ls = h_s(sd, "h_mean_s", zhat), h_s(sd, "h_scale_s", zhat)
        lik = []
        yhat, _, _ = self.slice_loop(y, lm, ls, lik=lik)
        return {"x_hat": g_s(sd, yhat), "likelihoods": {"y": torch.cat(lik, dim=1), "z": zl}}
