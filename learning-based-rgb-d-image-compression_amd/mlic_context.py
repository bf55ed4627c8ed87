"""The attention contexts of MLIC++ on MI355X: `LocalContext`, `LinearGlobalIntraContext` and `LinearGlobalInterContext`
(reference modules/transform/context.py:33-137, 163-213, 216-262) over the HIP engine, each a block of its own.

    lc = LocalContext(dim=32).to("cuda");                          out = lc(x)        # [B,32,H,W] -> [B,64,H,W]
    ia = LinearGlobalIntraContext(dim=32, num_heads=2).to("cuda"); out = ia(x1, x2)   # [B,32,H,W] x 2 -> [B,64,H,W], W even
    ie = LinearGlobalInterContext(dim=96, out_dim=64, num_heads=3).to("cuda"); out = ie(x1)   # [B,96,H,W] -> [B,64,H,W]

MLICPlusPlus (models/mlicpp.py) builds them per 32-channel slice: the local context on the decoded anchor half of a slice, the
intra context between the halves of one slice, the inter context over all slices decoded so far.  Constructor arguments and
state-dict names are the reference's; `relative_position_index` is accepted and ignored (the kernel computes the offsets).
The model around them is not part of this package yet.  No CPU path.
"""
import torch

from ._lib import check, lib
from .arch import linear_global_inter_entries, linear_global_intra_entries, local_context_entries
from .engine_module import EngineModule


class _Context(EngineModule):
    """x (and x2) [B,dim,H,W] -> [B,out,H,W] through one engine call."""
    _FORWARD = ""

    def _run(self, out_ch, x, *more):
        self._ready()
        if x.dim() != 4 or x.size(1) != self.dim or any(t.shape != x.shape for t in more):
            raise ValueError(f"expected {1 + len(more)} tensor(s) of the same shape [B,{self.dim},H,W]")
        B, _, H, W = x.shape
        xs = [t.to(self._device, torch.float32).contiguous() for t in (x,) + more]
        out = torch.empty((B, out_ch, H, W), dtype=torch.float32, device=self._device)
        check(getattr(lib(), self._FORWARD)(self._h, *[self._ptr(t) for t in xs], B, H, W, self._ptr(out), self._stream_ptr()),
              self._FORWARD[len("rgbd_"):])
        return out


class LocalContext(_Context):
    _MODEL = "LocalContext"
    _FORWARD = "rgbd_local_context_forward"

    def __init__(self, dim=32, window_size=5, mlp_ratio=2.0, num_heads=2, qkv_bias=True, qk_scale=None, init_seed=0):
        if (dim, window_size, num_heads) != (32, 5, 2) or not qkv_bias or qk_scale is not None or int(2 * dim * mlp_ratio) % 16:
            raise NotImplementedError("LocalContext: the kernel is built for dim 32, window 5, 2 heads, the default scale "
                                      "(the form MLIC++ uses)")
        self.dim, self.num_heads, self.window_size, self.mlp_ratio = int(dim), int(num_heads), int(window_size), float(mlp_ratio)
        self.H = self.W = -1
        super().__init__(local_context_entries(self.dim, self.window_size, self.mlp_ratio, self.num_heads), init_seed)

    def _synth_args(self):
        return {"dim": self.dim, "num_heads": self.num_heads}

    def _create_engine(self):
        return self._create("rgbd_local_context_create", self.dim)

    def update_resolution(self, H, W, device=None, mask=None):
        """The reference builds its attention mask here (:58-80); the kernel derives it from the position.  Returns whether
        the size changed, as the reference does."""
        updated = (self.H, self.W) != (H, W)
        self.H, self.W = H, W
        return updated

    def forward(self, x):  # :82-137
        return self._run(2 * self.dim, x)

    __call__ = forward


class LinearGlobalIntraContext(_Context):
    _MODEL = "LinearGlobalIntraContext"
    _FORWARD = "rgbd_linear_intra_forward"

    def __init__(self, dim=32, num_heads=2, init_seed=0):
        self.dim, self.num_heads = int(dim), int(num_heads)
        super().__init__(linear_global_intra_entries(self.dim), init_seed)

    def _synth_args(self):
        return {"dim": self.dim}

    def _create_engine(self):
        return self._create("rgbd_linear_intra_create", self.dim, self.num_heads)

    def forward(self, x1, x2):  # :189-213
        if x1.dim() == 4 and x1.size(3) % 2:
            raise ValueError("W must be even (the checkerboard halves of a row have the same length)")
        return self._run(2 * self.dim, x1, x2)

    __call__ = forward


class LinearGlobalInterContext(_Context):
    _MODEL = "LinearGlobalInterContext"
    _FORWARD = "rgbd_linear_inter_forward"

    def __init__(self, dim=32, out_dim=64, num_heads=2, init_seed=0):
        self.dim, self.out_dim, self.num_heads = int(dim), int(out_dim), int(num_heads)
        super().__init__(linear_global_inter_entries(self.dim, self.out_dim), init_seed)

    def _synth_args(self):
        return {"dim": self.dim, "out_dim": self.out_dim}

    def _create_engine(self):
        return self._create("rgbd_linear_inter_create", self.dim, self.out_dim, self.num_heads)

    def forward(self, x1):  # :243-262
        return self._run(self.out_dim, x1)

    __call__ = forward
