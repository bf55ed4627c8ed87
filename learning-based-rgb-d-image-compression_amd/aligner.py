"""`Spatial_aligner` on MI355X: the reference's guided window-attention block (modules/transform/spatialAligner.py:341-390)
over the HIP engine.

    sa = Spatial_aligner(in_channel=192, out_channel=192)
    sa.load_state_dict(state_dict); sa = sa.to("cuda")
    out = sa(x, guided)            # x, guided: [B,in_channel,H,W], H and W multiples of 8 -> [B,out_channel,H,W]

The block SynthesisTransformPlus inserts behind each of the first three transposed convolutions of g_s (synthesis.py:74-110):
two 2x2 stride-2 patch embeddings to 96 channels, two Swin blocks (4x4 windows, 3 heads of 32, shift 0 then 2) whose attention
takes the query from x and key / value from guided, and a 2x2 stride-2 transposed convolution.  State-dict names are the
reference's (patch_embeding1/2, blocks.K.{norm1,attn.{qkv1,qkv2,proj,relative_position_bias_table,relative_position_index},
norm2,mlp.{fc1,fc2}}, recovery); the index buffer is accepted and ignored.  No CPU path.
"""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from ._lib import RgbdError, check, lib
from .arch import spatial_aligner_entries


class Spatial_aligner:
    def __init__(self, in_channel=192, out_channel=192, input_resolution=(224, 224), init_seed=0):
        # (input_resolution only sizes a buffer the reference never reads: its forward() takes H and W from the input)
        self.in_channel, self.out_channel = int(in_channel), int(out_channel)
        self._entries = spatial_aligner_entries(self.in_channel, self.out_channel)
        self._init_seed = init_seed
        self._params = None
        self._h = None
        self._device = None
        self._dirty = True
        self._parent = None

    def _materialize(self):
        if self._params is None:
            from . import synth

            self._params = synth.synthetic_state_dict(self._init_seed, model="Spatial_aligner", in_channel=self.in_channel,
                                                      out_channel=self.out_channel)
        return self._params

    def eval(self):
        return self

    def state_dict(self):
        p = self._materialize()
        return OrderedDict((name, p[name]) for name in self._entries)

    def load_state_dict(self, state_dict, strict=True):
        if self._parent is not None:
            raise RgbdError("load_state_dict() on a shared-weight clone: call it on the parent")
        missing = [k for k, e in self._entries.items() if k not in state_dict and (e.is_param or strict)]
        unexpected = [k for k in state_dict if k not in self._entries]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for Spatial_aligner: missing {missing[:5]}, unexpected {unexpected[:5]}")
        params = OrderedDict(self._materialize()) if missing else OrderedDict()
        for name, e in self._entries.items():
            if name not in state_dict:
                continue
            v = state_dict[name]
            v = v.detach().cpu() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
            if tuple(v.shape) != tuple(e.shape):
                raise RuntimeError(f"size mismatch for {name}: checkpoint {tuple(v.shape)} vs model {tuple(e.shape)}")
            params[name] = v.float().contiguous().clone() if e.is_param else v.clone()
        self._params = params
        self._dirty = True

    def to(self, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RgbdError("Spatial_aligner (rgbd_amd) runs on the GPU only: use .to('cuda'); there is no CPU path")
        if not torch.cuda.is_available():
            raise RgbdError("no HIP device visible to torch")
        self._device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        self._upload()
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else f"cuda:{int(device)}")

    def _upload(self):
        L = lib()
        torch.cuda.set_device(self._device)
        if self._h is None:
            h = ctypes.c_void_p()
            check(L.rgbd_aligner_create(self.in_channel, self.out_channel, ctypes.byref(h)), "aligner_create")
            self._h = h
        p = self._materialize()
        for name, e in self._entries.items():
            if not e.is_param:
                continue
            a = p[name].detach().float().contiguous().numpy()
            if e.kind == "linear_w":  # nn.Linear -> 1x1 convolution
                a = a.reshape(a.shape[0], a.shape[1], 1, 1)
            shape = (ctypes.c_int64 * a.ndim)(*a.shape)
            check(L.rgbd_elic_set_tensor(self._h, name.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), shape, a.ndim),
                  f"set_tensor({name})")
        check(L.rgbd_elic_finalize(self._h), "finalize")
        self._dirty = False

    def clone_shared(self):
        """Another engine instance on the same GPU that borrows this one's device weights (own workspace)."""
        self._ready()
        other = type(self).__new__(type(self))
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k != "_h"})
        h = ctypes.c_void_p()
        check(lib().rgbd_elic_clone_shared(self._h, ctypes.byref(h)), "clone_shared")
        other._h = h
        other._parent = self
        return other

    def _ready(self):
        if self._h is None or self._device is None:
            raise RgbdError("call .to('cuda') before the forward pass")
        if self._dirty and self._parent is None:
            self._upload()
        torch.cuda.set_device(self._device)

    def forward(self, x, guided):  # spatialAligner.py:376-390
        self._ready()
        if x.dim() != 4 or x.size(1) != self.in_channel or guided.shape != x.shape:
            raise ValueError(f"expected x and guided of the same shape [B,{self.in_channel},H,W]")
        B, _, H, W = x.shape
        if H % 8 or W % 8:
            raise ValueError("H and W must be multiples of 8 (2x2 patches, 4x4 windows)")
        x = x.to(self._device, torch.float32).contiguous()
        guided = guided.to(self._device, torch.float32).contiguous()
        out = torch.empty((B, self.out_channel, H, W), dtype=torch.float32, device=self._device)
        check(lib().rgbd_aligner_forward(self._h, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(guided.data_ptr()), B, H, W,
                                         ctypes.c_void_p(out.data_ptr()),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "aligner_forward")
        return out

    __call__ = forward

    def __del__(self):
        try:
            if self._h is not None:
                lib().rgbd_elic_destroy(self._h)
                self._h = None
        except Exception:
            pass
