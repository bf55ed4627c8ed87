"""The latent codec of ELIC_master (rgbd_amd.MasterLatentCodec; reference models/elic_master.py:109-220, 222-307, 309-387 without
the outer blocks): the cases of the fixtures tests/golden/master_latent_<case>.npz (written by tests/golden/make_master_latent.py
from the unmodified reference class), their seeded inputs and weights, the bounds and acceptance functions, and a torch
restatement of the codec with deliberate mistakes selectable -- shared by test_master_latent_cpu.py and
test_gpu_master_latent.py.

Bounds.  FACTOR = 8, the project's bound for float contracts, times the reference's own fp32-to-fp64 distance of the tensor in
question (recorded in the fixture): e = max |out - ref64| / max |ref64| <= 8 * e_ref for y, for y_hat under the reference's
symbols, and for f_hat (there 8 * max(e_ref_fhat, 2^-23): an fp32 result cannot be asked to stand closer to fp64 than its own
rounding).  A decision (symbol or scale index) may differ from the reference's only where the fp64 value lies within 8 * e_ref *
max |fp64| of a boundary: of a rounding boundary for y - mean, of a scale-table entry for the scale.

f_hat has 192 full-resolution channels; above synplus_cases.SAMPLE_LIMIT it is compared at synplus_cases.sample_positions (every
channel, every border pixel, seeded interior pixels), thinned to at most FHAT_SAMPLES positions by a fixed stride so that a
fixture stays below the size limit of a committed file, and normalised by the stored max |ref64| of the whole tensor.

The guides have three different shapes, so "two of them exchanged" goes through a resampling: exchanged_guides() hands up3's
every other pixel in as up2 and up2's pixels, each repeated 2 x 2, in as up3."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import synplus_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTOR = 8.0
N, M, F_CH = 192, 320, 128
# name: (B, H, W, input seed, weight seed).  a: y 4x4, z 1x1, one aligner window at sp1, the smallest map g_s takes; b: a batch (one
# y stream, two z streams), non-square; c: the other orientation; d: y 12x8, z 3x2, aligner maps that need window padding and the
# shifted mask, a second set of weights.  The input seeds are the first of 301 / 302 / 303 / 304 + 10 k for which the generator's
# conditions hold on the reference alone (make_master_latent.py: the last of them, no decision within the reference's own fp32
# error of a boundary, holds for about one seed in fifteen at d's 30,720 symbols)
CASES = {"a": (1, 64, 64, 301, 21), "b": (2, 64, 128, 332, 21), "c": (1, 128, 64, 343, 21), "d": (1, 192, 128, 584, 22)}
ONE_MODEL = ["a", "c", "b", "a"]  # the shapes one model sees in turn (one set of weights)
FHAT_SAMPLES = 40_000
MUTATIONS = ["up23_exchanged", "no_se", "parity_swapped", "segments_reordered"]
OUTER = ("aux_encoder.", "master_encoder.", "master_decoder.", "channel_aligner.")


def config():
    from rgbd_amd import model_config

    return model_config()  # (the reference's config/config.py: N 192, M 320, slices 16, 16, 32, 64, 192)


def inputs(name):
    """f [B,128,H,W] of unit variance, and up1..up3 as synplus_cases.inputs draws them for the case's latent grid."""
    B, H, W, seed, _ = CASES[name]
    f = torch.randn(B, F_CH, H, W, generator=torch.Generator().manual_seed(seed + 1000))
    return (f,) + tuple(sc.inputs(B, H // 16, W // 16, seed)[1:])


def exchanged_guides(up1, up2, up3):
    return up1, up3[:, :, ::2, ::2].contiguous(), up2.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3).contiguous()


def weights(name, full=False, channel=3):
    from rgbd_amd import synth

    return synth.synthetic_state_dict(CASES[name][4], config=config(), model="ELIC_master" if full else "ELIC_master_latent", channel=channel)


def fhat_positions(name):
    """None (the whole tensor) or the flat positions into f_hat [B,N,H,W] a fixture holds."""
    B, H, W, seed, _ = CASES[name]
    if B * N * H * W <= sc.SAMPLE_LIMIT:
        return None
    pos = sc.sample_positions((B, N, H, W), seed)
    return pos[::max(1, math.ceil(pos.size / FHAT_SAMPLES))]


def load_fixture(name):
    return dict(np.load(os.path.join(GOLDEN, f"master_latent_{name}.npz")))


def y_sub(t):
    """What a fixture keeps of y and y_hat: every fourth channel (four and more per slice), every pixel."""
    return np.asarray(t)[:, ::4]


def scale_table():
    from rgbd_amd.entropy_models import get_scale_table

    return np.asarray(get_scale_table(), np.float32).astype(np.float64)


# ---- bounds and acceptance ----------------------------------------------------------------------------------------------------------
def rel(a, ref64, ref_max=None):
    a, ref64 = np.asarray(a, np.float64).reshape(-1), np.asarray(ref64, np.float64).reshape(-1)
    return float(np.abs(a - ref64).max() / (np.abs(ref64).max() if ref_max is None else ref_max))


def y_err(y, fx):
    return rel(y_sub(y), fx["y_sub64"], float(fx["y64_max"]))


def yhat_err(yhat, fx):
    return rel(y_sub(yhat), fx["yhat_sub64"], float(fx["yhat64_max"]))


def fhat_err(name, fhat, fx):
    pos = fhat_positions(name)
    flat = torch.as_tensor(fhat).reshape(-1)
    got = flat if pos is None else flat[torch.from_numpy(pos)]
    return rel(got.numpy(), fx["fhat64"], float(fx["ref64_max"]))


def y_bound(fx):
    return FACTOR * float(fx["e_ref_y"])


def yhat_bound(fx):
    return FACTOR * float(fx["e_ref_yhat"])


def fhat_bound(fx):
    return FACTOR * max(float(fx["e_ref_fhat"]), 2.0 ** -23)


def decision_bounds(fx):
    """Absolute float bounds of the two tensors a decision reads: (of y - mean, of the scale)."""
    return (FACTOR * float(fx["e_ref_x"]) * np.abs(fx["x64"]).max(), FACTOR * float(fx["e_ref_sigma"]) * np.abs(fx["sigma64"]).max())


def boundary_distances(fx):
    """Per coded symbol, from the fp64 run: the distance of y - mean to the rounding boundary, and of the scale to the nearest
    scale-table entry (below table[0] = the bound 0.11 a scale indexes row 0 until it crosses that entry)."""
    x64, s64 = fx["x64"], fx["sigma64"]
    tab = scale_table()
    return 0.5 - np.abs(x64 - np.rint(x64)), np.abs(s64[:, None] - tab[None, :-1]).min(axis=1)


def census(fx, sym, idx, x=None, s=None):
    """The teacher-forced census: the list of what is not accepted (empty = accepted).  sym / idx: the decisions taken under the
    reference's symbols; x / s: the floats behind them (optional)."""
    bx, bs = decision_bounds(fx)
    d_round, d_scale = boundary_distances(fx)
    bad = []
    dsym, didx = np.asarray(sym) != fx["symbols"].astype(np.int32), np.asarray(idx) != fx["indexes"].astype(np.int32)
    if (dsym & ~(d_round < bx)).any():
        bad.append(f"{int((dsym & ~(d_round < bx)).sum())} symbols differ from the reference's away from a rounding boundary")
    if (didx & ~(d_scale < bs)).any():
        bad.append(f"{int((didx & ~(d_scale < bs)).sum())} scale indexes differ from the reference's away from a table entry")
    if x is not None and np.abs(np.asarray(x, np.float64) - fx["x64"]).max() > bx:
        bad.append(f"max |d(y - mean)| {np.abs(x - fx['x64']).max():.3e} > {bx:.3e}")
    if s is not None and np.abs(np.asarray(s, np.float64) - fx["sigma64"]).max() > bs:
        bad.append(f"max |d scale| {np.abs(s - fx['sigma64']).max():.3e} > {bs:.3e}")
    return bad


# ---- the codec restated (float64 by default) -----------------------------------------------------------------------------------------
class Restated:
    """models/elic_master.py without its outer blocks, on a state dict: g_a (analysis.py:29-52), h_a, h_s, the checkerboard slice
    loop (:248-300) and g_s (synplus_cases.synthesis_plus).  mut: None, or one of MUTATIONS -- "up23_exchanged" exchanged_guides() on
    the way into g_s; "no_se" the EX nets without `params + se(params)`; "parity_swapped" each net applied to the other's
    checkerboard half (the nets' widths differ, so it is the halves that change hands: the anchor net codes the pixels with
    (row + col) even first, from the hyper prior alone); "segments_reordered" the nets' inputs as hyper | channel | local."""

    def __init__(self, sd, mut=None, dtype=torch.float64):
        self.sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        self.mut, self.dtype = mut, dtype
        self.slice_ch = list(config()["slice_ch"])

    def conv(self, t, n, stride=1, pad=0):
        return F.conv2d(t, self.sd[n + ".weight"], self.sd[n + ".bias"], stride=stride, padding=pad)

    def deconv(self, t, n, stride=2):
        k = self.sd[n + ".weight"].shape[-1]
        return F.conv_transpose2d(t, self.sd[n + ".weight"], self.sd[n + ".bias"], stride=stride, padding=k // 2, output_padding=stride - 1)

    def g_a(self, f):
        p = "g_a.analysis_transform."

        def res_unit(t, n):
            u = torch.relu(self.conv(t, n + ".conv.0"))
            u = torch.relu(self.conv(u, n + ".conv.2", pad=1))
            return torch.relu(self.conv(u, n + ".conv.4") + t)

        x = f.to(self.dtype)
        for i, kind in enumerate(["conv", "rb", "rb", "rb", "conv", "rb", "rb", "rb", "attn", "conv", "rb", "rb", "rb", "conv", "attn"]):
            n = p + str(i)
            if kind == "conv":
                x = self.conv(x, n, 2, 2)
            elif kind == "rb":
                u = torch.relu(self.conv(x, n + ".branch.0"))
                u = torch.relu(self.conv(u, n + ".branch.2", pad=1))
                x = self.conv(u, n + ".branch.4") + x
            else:
                a = b = x
                for u in range(3):
                    a, b = res_unit(a, f"{n}.conv_a.{u}"), res_unit(b, f"{n}.conv_b.{u}")
                x = a * torch.sigmoid(self.conv(b, n + ".conv_b.3")) + x
        return x

    def h_a(self, y):
        t = torch.relu(self.conv(y, "h_a.reduction.0", 1, 1))
        t = torch.relu(self.conv(t, "h_a.reduction.2", 2, 2))
        return self.conv(t, "h_a.reduction.4", 2, 2)

    def h_s(self, zhat):
        t = torch.relu(self.deconv(zhat, "h_s.increase.0"))
        t = torch.relu(self.deconv(t, "h_s.increase.2"))
        return self.deconv(t, "h_s.increase.4", 1)

    def medians(self):
        return self.sd["entropy_bottleneck.quantiles"][:, 0, 1].reshape(1, -1, 1, 1)

    def params(self, n, t):
        if self.mut != "no_se":
            g = t.mean(dim=(2, 3))
            g = torch.sigmoid(F.linear(torch.relu(F.linear(g, self.sd[n + ".se.fc.0.weight"])), self.sd[n + ".se.fc.2.weight"]))
            t = t + t * g[:, :, None, None]
        t = torch.relu(self.conv(t, n + ".fusion.0"))
        t = torch.relu(self.conv(t, n + ".fusion.2", pad=1))
        return self.conv(t, n + ".fusion.4", pad=2)

    def latent(self, y, z_symbols=None, forced=None):
        """y -> (y_hat, x = y - mean per coded symbol in stream order, scale likewise, symbols); z_symbols / forced: the
        reference's symbols (teacher forcing) or None (its own roundings)."""
        z = self.h_a(y)
        zs = torch.round(z - self.medians()) if z_symbols is None else torch.as_tensor(np.asarray(z_symbols)).reshape(z.shape).to(self.dtype)
        hyper = self.h_s(zs + self.medians())
        B, _, h, w = y.shape
        rr, cc = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        anchor = ((rr + cc) % 2 == 1) != (self.mut == "parity_swapped")  # [h, w]
        cat = (lambda parts: torch.cat(parts[::-1], 1)) if self.mut == "segments_reordered" else (lambda parts: torch.cat(parts, 1))
        xs, ss, syms, slices, c0, pos = [], [], [], [], 0, 0
        for i, C in enumerate(self.slice_ch):
            ys = y[:, c0:c0 + C]
            ctx = [] if i == 0 else [self.channel_context(i, torch.cat(slices, 1))]
            yh = torch.zeros_like(ys)
            for part, mask in enumerate((anchor, ~anchor)):
                fam = "entropy_parameters_nonanchor." if part else "entropy_parameters_anchor."
                inp = ([self.conv(yh, f"local_context.{i}", pad=2)] if part else []) + ctx + [hyper]
                scales, means = self.params(fam + str(i), cat(inp)).chunk(2, 1)
                x = (ys - means)[:, :, mask]  # [B, C, h * w / 2]: row-major over the half's pixels = the squeezed (row, w / 2) order
                n = x.numel()
                s = torch.round(x) if forced is None else torch.as_tensor(np.asarray(forced[pos:pos + n])).reshape(x.shape).to(self.dtype)
                yh = yh.clone()
                yh[:, :, mask] = s + means[:, :, mask]
                xs.append(x.reshape(-1))
                ss.append(scales[:, :, mask].reshape(-1))
                syms.append(s.reshape(-1))
                pos += n
            slices.append(yh)
            c0 += C
        return torch.cat(slices, 1), torch.cat(xs).numpy(), torch.cat(ss).numpy(), torch.cat(syms).numpy().astype(np.int32)

    def channel_context(self, i, t):
        n = f"channel_context.{i}.fushion."
        t = torch.relu(self.conv(t, n + "0", pad=2))
        t = torch.relu(self.conv(t, n + "2", pad=2))
        return self.conv(t, n + "4", pad=2)

    def g_s(self, yhat, up1, up2, up3):
        ups = exchanged_guides(up1, up2, up3) if self.mut == "up23_exchanged" else (up1, up2, up3)
        sub = {k[len("g_s."):]: v for k, v in self.sd.items() if k.startswith("g_s.")}
        return sc.synthesis_plus(sub, yhat, *[u.to(self.dtype) for u in ups], None, self.dtype)
