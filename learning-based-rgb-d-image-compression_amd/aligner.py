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
import torch

from ._lib import check, lib
from .arch import spatial_aligner_entries
from .engine_module import EngineModule


class Spatial_aligner(EngineModule):
    _MODEL = "Spatial_aligner"

    def __init__(self, in_channel=192, out_channel=192, input_resolution=(224, 224), init_seed=0):
        # (input_resolution only sizes a buffer the reference never reads: its forward() takes H and W from the input)
        self.in_channel, self.out_channel = int(in_channel), int(out_channel)
        super().__init__(spatial_aligner_entries(self.in_channel, self.out_channel), init_seed)

    def _synth_args(self):
        return {"in_channel": self.in_channel, "out_channel": self.out_channel}

    def _create_engine(self):
        return self._create("rgbd_aligner_create", self.in_channel, self.out_channel)

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
        check(lib().rgbd_aligner_forward(self._h, self._ptr(x), self._ptr(guided), B, H, W, self._ptr(out), self._stream_ptr()),
              "aligner_forward")
        return out

    __call__ = forward
