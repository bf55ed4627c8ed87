"""`Cheng2020AnchorwithCheckerboard` ("ckbd") on MI355X: the reference's single-image baseline
(models/Cheng2020withCKBD.py:40-265 on CompressAI's Cheng2020Anchor, compressai/models/waseda.py:22-81) over the HIP engine.

    net = Cheng2020AnchorwithCheckerboard(N=192, channel=3).eval()
    net.load_state_dict(checkpoint["state_dict"]); net.update(force=True); net = net.to("cuda")
    out = net.compress(x)                              -> {"strings": [[y], [z]*B], "shape": (H/64, W/64)}
    rec = net.decompress(out["strings"], out["shape"]) -> {"x_hat": [B,C,H,W] (not clamped, :167-174), "cost_time"}
    fwd = net(x)                                       -> {"x_hat", "likelihoods": {"y", "z"}}

Residual blocks of 3x3 / 1x1 convolutions with GDN / IGDN (one fused launch each, csrc/gdn.hip), sub-pixel up-sampling, and
a two-pass checkerboard entropy model: the anchor half of y is coded from the hyper prior alone, the other half with the
masked 5x5 context convolution over the decoded anchors; both halves of the whole batch go into ONE rANS stream (anchor
first), or into one stream per image with per_image_streams.  M = N.  validate() and training are not part of the inference
path.  No CPU path.
"""
import ctypes

import torch

from ._lib import check, lib
from .arch import ckbd_config, ckbd_entries
from .elic import ELIC
from .elic_united import _LazyStore
from .entropy_models import EntropyBottleneck, GaussianConditional


class Cheng2020AnchorwithCheckerboard(ELIC):
    _MODEL = "ckbd"

    def __init__(self, N=192, channel=3, init_seed=0, **kwargs):
        # (a config= keyword is accepted and ignored, as the reference's class swallows it in **kwargs)
        if int(N) not in (128, 192):
            raise ValueError(f"N must be 128 or 192 (the reference's quality levels), got {N}")
        if int(channel) not in (1, 3):
            raise ValueError(f"channel must be 3 or 1, got {channel}")
        self.config = ckbd_config(N)
        self.channel = int(channel)
        self.N = self.M = int(N)
        self.slice_ch = [self.M]
        self.slice_num = 1
        self.quant = "ste"
        self.training = False
        self.per_image_streams = False  # False = the reference's format: one y stream for the whole batch
        self._entries = ckbd_entries(self.N, self.channel)
        self._init_seed = init_seed
        self._params = None
        self.gaussian_conditional = GaussianConditional(None)
        self._store = _LazyStore(self)
        self.entropy_bottleneck = EntropyBottleneck(self._store, "entropy_bottleneck")
        self._h = None
        self._device = None
        self._dirty = True
        self._gen = 0
        self._parent = None

    @classmethod
    def from_state_dict(cls, state_dict):  # waseda.py:83-89
        w = state_dict["g_a.0.conv1.weight"]
        net = cls(N=int(w.shape[0]), channel=int(w.shape[1]))
        net.load_state_dict(state_dict)
        return net

    def _materialize(self):
        if self._params is None:
            from . import synth

            self._params = synth.synthetic_state_dict(self._init_seed, stress=False, model="ckbd", N=self.N, channel=self.channel)
        return self._params

    def _create_engine(self):
        h = ctypes.c_void_p()
        check(lib().rgbd_elic_create_ckbd(self.N, self.channel, ctypes.byref(h)), "elic_create_ckbd")
        return h

    def forward(self, x):  # Cheng2020withCKBD.py:52-71 (eval mode)
        """Eval-mode forward(): y_hat = round(y), one parameter pass over the context with its anchor outputs zeroed;
        {"x_hat", "likelihoods": {"y", "z"}} like the reference."""
        self._ready()
        if self.training:
            raise RuntimeError("forward() is built for eval mode (inference path); call .eval() first")
        if x.dim() != 4 or x.size(1) != self.channel:
            raise ValueError(f"expected x [B,{self.channel},H,W]")
        B, _, H, W = x.shape
        if H % 64 or W % 64:
            raise ValueError("H and W must be multiples of 64 (pad first: dataset/utils.py:58-67)")
        x = x.to(self._device, torch.float32).contiguous()
        xh = torch.empty((B, self.channel, H, W), dtype=torch.float32, device=self._device)
        ly = torch.empty((B, self.M, H // 16, W // 16), dtype=torch.float32, device=self._device)
        lz = torch.empty((B, self.N, H // 64, W // 64), dtype=torch.float32, device=self._device)
        check(lib().rgbd_elic_forward_single(self._h, ctypes.c_void_p(x.data_ptr()), B, H, W, ctypes.c_void_p(xh.data_ptr()),
                                             ctypes.c_void_p(ly.data_ptr()), ctypes.c_void_p(lz.data_ptr()),
                                             self._stream_ptr()), "forward")
        return {"x_hat": xh, "likelihoods": {"y": ly, "z": lz}}

    __call__ = forward

    def validate(self, x):
        raise NotImplementedError("validate() (training-time distortion estimate) is not part of the inference path")
