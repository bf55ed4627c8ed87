"""Single-modal `ELIC` on MI355X: the reference's model API (models/elic.py) over the HIP engine -- and `SingleCodec`, the
base it shares with the other one-tensor models (stf.py, ckbd.py, mlic.py).

    net = ELIC(config=model_config(), channel=3).eval()
    net.load_state_dict(checkpoint["state_dict"]); net.update(force=True); net = net.to("cuda")
    out = net.compress(x)                              -> {"strings": [[y], [z]*B], "shape": (H/64, W/64)}
    rec = net.decompress(out["strings"], out["shape"]) -> {"x_hat": [B,C,H,W] (not clamped, as in the reference), "cost_time"}

ELIC(config, channel, return_mid=True) (the aux network of the reference's TesterMaster / trainer_master): decompress() and
forward() also return "up1", "up2", "up3", the outputs of the first three transposed convolutions of g_s
(modules/transform/synthesis.py:54-67): [B,N,H/8,W/8], [B,N,H/4,W/4], [B,N,H/2,W/2].

Same engine, kernels and rules as ELIC_united (no CPU path); only the layer graph differs (no cross-modal fusion, one
entropy bottleneck, EntropyParameters = three 1x1 convolutions).
"""
import time

import torch

from ._lib import check, lib
from .arch import elic_entries, model_config
from .elic_united import Codec


class SingleCodec(Codec):
    """One tensor per call: compress(x) / decompress(strings, shape) / forward(x) over the engine's *_single entry points."""
    _MODALITIES = (("", 0, 2),)
    _LIKELIHOOD_KEYS = ("y", "z")  # of forward()["likelihoods"]

    def _synth_args(self):
        return {**super()._synth_args(), "channel": self.channel}

    def _mid_tensors(self, B, H, W):
        """Tensors for what a call returns besides x_hat (none: the *_mid entry points belong to ELIC(return_mid=True))."""
        return []

    def _check_image(self, x):
        if x.dim() != 4 or x.size(1) != self.channel:
            raise ValueError(f"expected x [B,{self.channel},H,W]")
        if x.shape[2] % 64 or x.shape[3] % 64:
            raise ValueError("H and W must be multiples of 64 (pad first: dataset/utils.py:58-67)")
        return x.shape[0], x.shape[2], x.shape[3]

    def compress(self, x):  # models/elic.py:161-253
        self._ready()
        B, H, W = self._check_image(x)
        x = x.to(self._device, torch.float32).contiguous()
        check(lib().rgbd_elic_compress_single(self._h, self._ptr(x), B, H, W, 1 if self.per_image_streams else 0,
                                              self._stream_ptr()), "compress")
        return {"strings": [self._tag_y(self._fetch_streams(0, 0)), self._fetch_streams(0, 1)], "shape": torch.Size((H // 64, W // 64))}

    def decompress(self, strings, shape):  # models/elic.py:255-325
        self._ready()
        torch.cuda.current_stream().synchronize()
        t0 = time.process_time()
        ys, zs = self._untag_y(strings[0]), list(strings[1])
        B = len(zs)
        if len(ys) not in (1, B):
            raise ValueError("Invalid strings parameters")
        zh, zw = int(shape[0]), int(shape[1])
        out = torch.empty((B, self.channel, zh * 64, zw * 64), dtype=torch.float32, device=self._device)
        k1, py, ly = self._pack_strings(ys)
        k2, pz, lz = self._pack_strings(zs)
        ups = self._mid_tensors(B, zh * 64, zw * 64)  # models/elic.py:318-329
        fn = lib().rgbd_elic_decompress_single_mid if ups else lib().rgbd_elic_decompress_single
        check(fn(self._h, py, ly, len(ys), pz, lz, B, zh, zw, self._ptr(out), *map(self._ptr, ups), self._stream_ptr()),
              "decompress")
        torch.cuda.current_stream().synchronize()
        del k1, k2
        return {"x_hat": out, "cost_time": time.process_time() - t0, **dict(zip(("up1", "up2", "up3"), ups))}

    def forward(self, x):  # models/elic.py:60-161, stf.py:618-678, Cheng2020withCKBD.py:52-71 (eval mode, quant = "ste")
        """Eval-mode forward(): {"x_hat", "likelihoods": {y key, z key}} like the reference (x_hat is not clamped; Gaussian /
        factorised-prior likelihoods).  ELIC: y_hat = round(y - mean) + mean slice by slice, keys "y_likelihoods" /
        "z_likelihoods".  STF, ckbd: keys "y" / "z"; ckbd: y_hat = round(y), one parameter pass over the context with its
        anchor outputs zeroed."""
        self._ready()
        if self.training:
            raise RuntimeError("forward() is built for eval mode (inference path); call .eval() first")
        if self.quant != "ste":  # models/elic.py:84-99: any other setting rounds without the mean (and adds noise in training)
            raise NotImplementedError(f"forward() implements config quant = 'ste' (the reference's model_config); got {self.quant!r}")
        B, H, W = self._check_image(x)
        x = x.to(self._device, torch.float32).contiguous()
        xh = torch.empty((B, self.channel, H, W), dtype=torch.float32, device=self._device)
        ly = torch.empty((B, self.M, H // 16, W // 16), dtype=torch.float32, device=self._device)
        lz = torch.empty((B, self.N, H // 64, W // 64), dtype=torch.float32, device=self._device)
        ups = self._mid_tensors(B, H, W)  # models/elic.py:159-170
        fn = lib().rgbd_elic_forward_single_mid if ups else lib().rgbd_elic_forward_single
        check(fn(self._h, self._ptr(x), B, H, W, self._ptr(xh), self._ptr(ly), self._ptr(lz), *map(self._ptr, ups),
                 self._stream_ptr()), "forward")
        return {"x_hat": xh, "likelihoods": dict(zip(self._LIKELIHOOD_KEYS, (ly, lz))), **dict(zip(("up1", "up2", "up3"), ups))}

    __call__ = forward


class ELIC(SingleCodec):
    _MODEL = "ELIC"
    _LIKELIHOOD_KEYS = ("y_likelihoods", "z_likelihoods")

    def __init__(self, config=None, channel=3, return_mid=False, init_seed=0, **kwargs):
        config = model_config() if config is None else config
        super().__init__(elic_entries(config, channel), config, channel, init_seed)
        self.return_mid = bool(return_mid)  # models/elic.py:17,44

    def _create_engine(self):
        return self._create("rgbd_elic_create_single", self.N, self.M, self.slice_ch, self.channel)

    def _mid_tensors(self, B, H, W):
        if not self.return_mid:
            return []
        return [torch.empty((B, self.N, H >> k, W >> k), dtype=torch.float32, device=self._device) for k in (3, 2, 1)]
