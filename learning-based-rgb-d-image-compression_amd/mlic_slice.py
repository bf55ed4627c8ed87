"""The three networks MLIC++ runs inside its slice loop on MI355X: `EntropyParametersMLIC`, `ChannelContext` and
`LatentResidualPrediction` (reference modules/transform/entropy.py:31-53, context.py:140-160, LRP.py:9-26) over the HIP engine,
each a block of its own.

    ep = EntropyParametersMLIC(960, 64).to("cuda");    out = ep(params)          # [B,960,H,W] -> [B,64,H,W]
    out = ep.forward_segments([a, b, c, d, e])                                   # the same on torch.cat([...], 1), never formed
    ep.forward_segments([a, b, c, d, e], parity=0, out=out)                      # only the anchor pixels of `out` are rewritten
    cc = ChannelContext(96, 32).to("cuda");            out = cc(channel_params)  # [B,96,H,W] -> [B,128,H,W]
    lrp = LatentResidualPrediction(352, 32).to("cuda"); out = lrp(x)             # [B,352,H,W] -> [B,32,H,W], in (-0.5, 0.5)

MLICPlusPlus (models/mlicpp.py) builds them per 32-channel slice: two parameter networks and two residual predictions per
slice, one channel context from the second slice on.  Constructor arguments and state-dict names are the reference's (the
attribute of ChannelContext is spelled `fushion` there).  EntropyParametersMLIC is one fused launch (csrc/pixel_mlp.hip);
`.fused = False` runs the same layers as four convolution launches.  The model around them is not part of this package yet
(DESIGN.md 7).  No CPU path.
"""
import ctypes

import torch
from torch import nn

from ._lib import check, lib
from .arch import channel_context_entries, entropy_params_mlic_entries, lrp_entries
from .engine_module import EngineModule

MAX_SEGMENTS = 6


def _gelu_only(act, who):
    if act is not nn.GELU:
        raise NotImplementedError(f"{who}: the kernels compute nn.GELU (erf form) between the layers; act={act!r} is not built")


class _SliceNet(EngineModule):
    """x [B,in_dim,H,W] -> [B,_out_channels,H,W] through one engine call."""
    _FORWARD = ""
    _CREATE = ""

    def _synth_args(self):
        return {"in_dim": self.in_dim, "out_dim": self.out_dim}

    def _create_engine(self):
        return self._create(self._CREATE, self.in_dim, self.out_dim)

    def _checked(self, x):
        self._ready()
        if x.dim() != 4 or x.size(1) != self.in_dim:
            raise ValueError(f"expected a tensor of shape [B,{self.in_dim},H,W], got {tuple(x.shape)}")
        return x.to(self._device, torch.float32).contiguous()

    def forward(self, x):
        x = self._checked(x)
        B, _, H, W = x.shape
        if H < 2 or W < 2:
            raise ValueError(f"expected a tensor of shape [B,{self.in_dim},H,W] with H >= 2 and W >= 2, got {tuple(x.shape)}")
        out = torch.empty((B, self._out_channels, H, W), dtype=torch.float32, device=self._device)
        check(getattr(lib(), self._FORWARD)(self._h, self._ptr(x), B, H, W, self._ptr(out), self._stream_ptr()),
              self._FORWARD[len("rgbd_"):])
        return out

    __call__ = forward


class EntropyParametersMLIC(_SliceNet):
    _MODEL = "EntropyParametersMLIC"
    _CREATE = "rgbd_entropy_params_mlic_create"

    def __init__(self, in_dim, out_dim, act=nn.GELU, init_seed=0):
        _gelu_only(act, "EntropyParametersMLIC")
        self.in_dim, self.out_dim = int(in_dim), int(out_dim)
        if self.in_dim % 16 or not 16 <= self.in_dim <= 960 or self.out_dim % 16 or not 16 <= self.out_dim <= 128:
            raise NotImplementedError("EntropyParametersMLIC: the kernel is built for in_dim 16 ... 960 and out_dim 16 ... 128, "
                                      "multiples of 16")
        self._out_channels = self.out_dim
        self._fused = True
        super().__init__(entropy_params_mlic_entries(self.in_dim, self.out_dim), init_seed)

    @property
    def fused(self):
        """True (default): one fused launch; False: the four layers as four convolution launches (the yardstick)."""
        return self._fused

    @fused.setter
    def fused(self, on):
        self._fused = bool(on)
        if self._h is not None:
            check(lib().rgbd_entropy_params_mlic_set_fused(self._h, int(self._fused)), "entropy_params_mlic_set_fused")

    def _upload(self):
        super()._upload()
        check(lib().rgbd_entropy_params_mlic_set_fused(self._h, int(self._fused)), "entropy_params_mlic_set_fused")

    def forward_segments(self, tensors, parity=-1, out=None):
        """The module on torch.cat(tensors, dim=1) without forming it: a list of 1 ... 6 tensors [B,c_i,H,W], every c_i a
        multiple of 16, summing to in_dim.  parity -1: every pixel; 0: only the anchor pixels ((row + col) odd) are computed
        and written, 1: only the others -- the rest of `out` keeps what it held (`out` is required then, W must be even)."""
        self._ready()
        tensors = list(tensors)
        ok = 1 <= len(tensors) <= MAX_SEGMENTS and all(t.dim() == 4 for t in tensors)
        ok = ok and all(t.shape[0] == tensors[0].shape[0] and t.shape[2:] == tensors[0].shape[2:] for t in tensors)
        if not ok or any(t.size(1) % 16 or t.size(1) < 16 for t in tensors) or sum(t.size(1) for t in tensors) != self.in_dim:
            raise ValueError(f"expected 1 ... {MAX_SEGMENTS} tensors [B,c_i,H,W] of the same B, H, W, every c_i a multiple of 16, "
                             f"summing to {self.in_dim} channels; got {[tuple(t.shape) for t in tensors]}")
        if parity not in (-1, 0, 1):
            raise ValueError(f"parity must be -1 (all pixels), 0 (anchor) or 1 (non-anchor), got {parity!r}")
        B, _, H, W = tensors[0].shape
        if parity >= 0 and (out is None or W % 2):
            raise ValueError("a parity call rewrites one checkerboard half of `out`: pass out=, and W must be even")
        shape = (B, self.out_dim, H, W)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self._device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != self._device or not out.is_contiguous():
            raise ValueError(f"expected out to be a contiguous float32 tensor of shape {list(shape)} on {self._device}")
        xs = [t.to(self._device, torch.float32).contiguous() for t in tensors]
        ptrs = (ctypes.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
        chans = (ctypes.c_int32 * len(xs))(*[t.size(1) for t in xs])
        check(lib().rgbd_entropy_params_mlic_forward(self._h, ptrs, chans, len(xs), B, H, W, int(parity), self._ptr(out),
                                                     self._stream_ptr()), "entropy_params_mlic_forward")
        return out

    def forward(self, params):  # entropy.py:43-53
        return self.forward_segments([self._checked(params)])

    __call__ = forward


class ChannelContext(_SliceNet):
    _MODEL = "ChannelContext"
    _CREATE = "rgbd_channel_context_create"
    _FORWARD = "rgbd_channel_context_forward"

    def __init__(self, in_dim, out_dim, init_seed=0):
        self.in_dim, self.out_dim = int(in_dim), int(out_dim)
        self._out_channels = 4 * self.out_dim
        super().__init__(channel_context_entries(self.in_dim, self.out_dim), init_seed)


class LatentResidualPrediction(_SliceNet):
    _MODEL = "LatentResidualPrediction"
    _CREATE = "rgbd_lrp_create"
    _FORWARD = "rgbd_lrp_forward"

    def __init__(self, in_dim, out_dim, act=nn.GELU, init_seed=0):
        _gelu_only(act, "LatentResidualPrediction")
        self.in_dim, self.out_dim = int(in_dim), int(out_dim)
        self._out_channels = self.out_dim
        super().__init__(lrp_entries(self.in_dim, self.out_dim), init_seed)
