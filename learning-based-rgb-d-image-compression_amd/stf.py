"""Single-modal `STF` (SymmetricalTransFormer) on MI355X: the reference's single-image Swin codec (models/stf.py:408-816)
over the HIP engine.

    net = SymmetricalTransFormer(channel=3).eval()
    net.load_state_dict(checkpoint["state_dict"]); net.update(force=True); net = net.to("cuda")
    out = net.compress(x)                              -> {"strings": [[y], [z]*B], "shape": (H/64, W/64)}
    rec = net.decompress(out["strings"], out["shape"]) -> {"x_hat": [B,C,H,W] clamped to [0, 1] (stf.py:815), "cost_time"}
    fwd = net(x)                                       -> {"x_hat" (not clamped), "likelihoods": {"y", "z"}}

The transforms are the Swin stacks of STF_united without the cross-modal fusion; the entropy model is the channel-slice
model of stf.py:723-807: 12 raster slices of 32 channels in ONE rANS stream per call, two hyper-synthesis nets, two parameter
nets per slice and latent residual prediction.  N = 192, M = 384 and the slices are fixed by the model.  One defined
difference from the reference: its decompress() handles one image only (stf.py:799 reshapes the whole batch into one image);
here decompress() of a batch is the inverse of compress() of that batch.  No CPU path.
"""
import ctypes

import torch

from ._lib import check, lib
from .arch import stf_entries, stf_single_config
from .elic import ELIC
from .elic_united import _LazyStore
from .entropy_models import EntropyBottleneck, GaussianConditional


class SymmetricalTransFormer(ELIC):
    _MODEL = "STF"

    def __init__(self, config=None, channel=3, init_seed=0, **kwargs):
        # (config, and the reference's keyword arguments -- pretrain_img_size, embed_dim, depths, ... -- are accepted and
        #  ignored: the engine implements the reference's defaults, which is what its zoo and testers build)
        self.config = stf_single_config()
        self.channel = channel
        self.N, self.M = int(self.config["N"]), int(self.config["M"])
        self.slice_ch = list(self.config["slice_ch"])
        self.slice_num = self.num_slices = len(self.slice_ch)
        self.max_support_slices = self.num_slices // 2
        self.quant = "ste"
        self.training = False
        self.per_image_streams = False  # False = the reference's format: one y stream for the whole batch
        self._entries = stf_entries(channel)
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
    def from_state_dict(cls, state_dict):  # stf.py:696-701
        net = cls()
        net.load_state_dict(state_dict)
        return net

    def _materialize(self):
        if self._params is None:
            from . import synth

            self._params = synth.synthetic_state_dict(self._init_seed, stress=False, model="STF", channel=self.channel)
        return self._params

    def _create_engine(self):
        h = ctypes.c_void_p()
        check(lib().rgbd_elic_create_stf_single(int(self.channel), ctypes.byref(h)), "elic_create_stf_single")
        return h

    def forward(self, x):  # stf.py:618-678 (eval mode)
        """Eval-mode forward(): {"x_hat" (not clamped), "likelihoods": {"y", "z"}} like the reference."""
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


STF = SymmetricalTransFormer
