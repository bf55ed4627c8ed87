"""`MasterLatentCodec` on MI355X: the latent codec of the reference's ELIC_master (models/elic_master.py) over the HIP engine --
everything between the model's outer blocks, which is its whole bitstream.

    net = MasterLatentCodec(config=model_config()).eval()
    net.load_state_dict(checkpoint["state_dict"], strict=False); net.update(force=True); net = net.to("cuda")
    out = net.compress(f)                                             -> {"strings": [[y], [z]*B], "shape": (H/64, W/64)}
    rec = net.decompress(out["strings"], out["shape"], up1, up2, up3) -> {"f_hat": [B,N,H,W]}
    fwd = net(f, up1, up2, up3)                                       -> {"f_hat", "likelihoods": {"y_likelihoods", "z_likelihoods"}}

f [B,128,H,W] is cat([fv, fv_bar]) (:113, 226): the master image's features and the aligned aux features.  up1..up3 are what
ELIC(return_mid=True) hands back for the decoded aux image: [B,N,H/8,W/8], [B,N,H/4,W/4], [B,N,H/2,W/2].  f_hat is g_s's output
(:216, 378), the tensor the reference concatenates with fv_bar and hands to master_decoder.  Inside: g_a = AnalysisTransformEX on
128 channels, ELIC's h_a / h_s, the checkerboard slice loop with EntropyParametersEX nets, g_s = SynthesisTransformPlus.
Feature_encoder, Feature_decoder and Channel_aligner are not part of this class; a full ELIC_master checkpoint
loads with strict=False, its entries under aux_encoder., master_encoder., master_decoder. and channel_aligner. reported as
unexpected.  H and W must be multiples of 64.  No CPU path.
"""
from collections import namedtuple

import torch

from ._lib import check, lib
from .arch import FEATURE_CH, MASTER_OUTER_PREFIXES, elic_master_latent_entries, model_config
from .elic import SingleCodec

IncompatibleKeys = namedtuple("IncompatibleKeys", ["missing_keys", "unexpected_keys"])


class MasterLatentCodec(SingleCodec):
    _MODEL = "ELIC_master_latent"
    _LIKELIHOOD_KEYS = ("y_likelihoods", "z_likelihoods")

    def __init__(self, config=None, init_seed=0, **kwargs):
        config = model_config() if config is None else config
        if int(config["N"]) != 192:
            raise NotImplementedError("ELIC_master_latent: g_s.sp1..sp3 are built with 192 channels whatever N is (synthesis.py:94-96)")
        super().__init__(elic_master_latent_entries(config), config, 2 * FEATURE_CH, init_seed)

    def _create_engine(self):
        return self._create("rgbd_master_latent_create", self.N, self.M, self.slice_ch)

    def set_coder(self, coder="reference", lanes=64):
        if coder == "wide":
            raise NotImplementedError("ELIC_master_latent codes the reference's stream format only (no wide path)")
        return super().set_coder(coder, lanes)

    def load_state_dict(self, state_dict, strict=False):
        """The latent part of a checkpoint.  strict=False: a full ELIC_master checkpoint loads, and its outer-block entries come
        back as `unexpected_keys`; strict=True refuses any key this class does not hold, naming the keys."""
        if state_dict and all(k.startswith("module.") for k in state_dict):
            state_dict = {k[len("module."):]: v for k, v in state_dict.items()}
        missing = [k for k in self._entries if k not in state_dict]
        unexpected = [k for k in state_dict if k not in self._entries]
        if strict and (missing or unexpected):
            outer = sorted({k.split(".")[0] + "." for k in unexpected if k.startswith(MASTER_OUTER_PREFIXES)})
            raise RuntimeError(f"Error(s) in loading state_dict for {self._MODEL}: {len(missing)} missing {missing[:5]}, "
                               f"{len(unexpected)} unexpected {unexpected[:5]}" +
                               (f"; the outer blocks of ELIC_master ({', '.join(outer)}) are not part of this class: "
                                f"load with strict=False" if outer else ""))
        super().load_state_dict(state_dict, strict=False)
        return IncompatibleKeys(missing, unexpected)

    def _check_guides(self, B, H, W, ups):
        """Host-side check of the guides of g_s (models/elic_master.py:213-216), before anything touches the GPU."""
        for k, u in enumerate(ups):
            want = [B, self.N, H >> (3 - k), W >> (3 - k)]
            if u is None or list(u.shape) != want:
                raise ValueError(f"expected up{k + 1} {want}, got {None if u is None else list(u.shape)}")

    def compress(self, f):  # models/elic_master.py:228-304
        self._check_image(f)
        return super().compress(f)

    def decompress(self, strings, shape, up1=None, up2=None, up3=None):  # models/elic_master.py:319-378
        ys, zs = list(strings[0]), list(strings[1])
        B = len(zs)
        if B < 1 or len(ys) not in (1, B):
            raise ValueError("Invalid strings parameters")
        zh, zw = int(shape[0]), int(shape[1])
        if zh < 1 or zw < 1:
            raise ValueError("shape must be at least (1, 1)")
        H, W = zh * 64, zw * 64
        self._check_guides(B, H, W, (up1, up2, up3))
        self._ready()
        ups = [u.to(self._device, torch.float32).contiguous() for u in (up1, up2, up3)]
        out = torch.empty((B, self.N, H, W), dtype=torch.float32, device=self._device)
        k1, py, ly = self._pack_strings(ys)
        k2, pz, lz = self._pack_strings(zs)
        check(lib().rgbd_master_latent_decompress(self._h, py, ly, len(ys), pz, lz, B, zh, zw, *map(self._ptr, ups), self._ptr(out),
                                                  self._stream_ptr()), "decompress")
        torch.cuda.current_stream().synchronize()
        del k1, k2
        return {"f_hat": out}

    def forward(self, f, up1=None, up2=None, up3=None):  # models/elic_master.py:115-216 (eval mode, quant = "ste")
        if self.training:
            raise RuntimeError("forward() is built for eval mode (inference path); call .eval() first")
        if self.quant != "ste":
            raise NotImplementedError(f"forward() implements config quant = 'ste' (the reference's model_config); got {self.quant!r}")
        B, H, W = self._check_image(f)
        self._check_guides(B, H, W, (up1, up2, up3))
        self._ready()
        ups = [u.to(self._device, torch.float32).contiguous() for u in (up1, up2, up3)]
        f = f.to(self._device, torch.float32).contiguous()
        fh = torch.empty((B, self.N, H, W), dtype=torch.float32, device=self._device)
        ly = torch.empty((B, self.M, H // 16, W // 16), dtype=torch.float32, device=self._device)
        lz = torch.empty((B, self.N, H // 64, W // 64), dtype=torch.float32, device=self._device)
        check(lib().rgbd_master_latent_forward(self._h, self._ptr(f), *map(self._ptr, ups), B, H, W, self._ptr(fh), self._ptr(ly),
                                               self._ptr(lz), self._stream_ptr()), "forward")
        return {"f_hat": fh, "likelihoods": dict(zip(self._LIKELIHOOD_KEYS, (ly, lz)))}

    __call__ = forward
    # compress(f) is SingleCodec's (rgbd_elic_compress_single on the 128-channel f: g_s does not run, no guides are taken).
