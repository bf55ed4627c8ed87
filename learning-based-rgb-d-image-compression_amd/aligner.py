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
from .arch import spatial_aligner_entries, synthesis_plus_entries
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


class SynthesisTransformPlus(EngineModule):
    """The guided synthesis transform of ELIC_master (modules/transform/synthesis.py:74-110): the 15 g_s stages of ELIC with
    x replaced by Spatial_aligner(x, up_k) behind each of the first three transposed convolutions.

        gs = SynthesisTransformPlus(N=192, M=320, ch=3)
        gs.load_state_dict(state_dict); gs = gs.to("cuda")
        x_hat = gs(y_hat, up1, up2, up3)   # [B,M,h,w], [B,N,2h,2w], [B,N,4h,4w], [B,N,8h,8w] -> [B,ch,16h,16w]

    up1..up3 are what ELIC(return_mid=True) returns for the aux image; tensors that already live on the module's device are
    read in place.  h and w are multiples of 4.  State-dict names are the reference's (synthesis_transform.K.*, sp1|sp2|sp3.*);
    N is 192, the width the reference builds sp1..sp3 with whatever N is.  Float arithmetic (single chain); no CPU path."""
    _MODEL = "SynthesisTransformPlus"

    def __init__(self, N, M, ch=3, act=None, init_seed=0):
        if not (act is None or act is torch.nn.ReLU or isinstance(act, torch.nn.ReLU)):
            raise NotImplementedError("SynthesisTransformPlus on MI355X fuses ReLU into its convolutions: act must be nn.ReLU")
        self.N, self.M, self.ch = int(N), int(M), int(ch)
        if self.N != 192:
            raise ValueError("N must be 192: sp1..sp3 are Spatial_aligner() with 192 channels (synthesis.py:94-96)")
        super().__init__(synthesis_plus_entries(self.N, self.M, self.ch), init_seed)

    def _synth_args(self):
        return {"N": self.N, "M": self.M, "channel": self.ch}

    def _create_engine(self):
        return self._create("rgbd_synthesis_plus_create", self.N, self.M, self.ch)

    def forward(self, x, up1, up2, up3):  # synthesis.py:98-110
        self._ready()
        if x.dim() != 4 or x.size(1) != self.M:
            raise ValueError(f"expected x of shape [B,{self.M},h,w]")
        B, _, h, w = x.shape
        if h % 4 or w % 4:
            raise ValueError("h and w must be multiples of 4 (the aligner behind up1 works on 8x8 blocks of the 2h x 2w map)")
        ups = []
        for k, u in enumerate((up1, up2, up3)):
            want = (B, self.N, (2 * h) << k, (2 * w) << k)
            if tuple(u.shape) != want:
                raise ValueError(f"expected up{k + 1} of shape {list(want)}, got {list(u.shape)}")
            ups.append(u.to(self._device, torch.float32).contiguous())
        x = x.to(self._device, torch.float32).contiguous()
        out = torch.empty((B, self.ch, 16 * h, 16 * w), dtype=torch.float32, device=self._device)
        check(lib().rgbd_synthesis_plus_forward(self._h, self._ptr(x), self._ptr(ups[0]), self._ptr(ups[1]), self._ptr(ups[2]),
                                                B, h, w, self._ptr(out), self._stream_ptr()), "synthesis_plus_forward")
        return out

    __call__ = forward
