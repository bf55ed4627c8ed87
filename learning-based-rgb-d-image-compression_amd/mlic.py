"""`MLICPlusPlus` ("MLIC") on MI355X: the reference's single-image MLIC++ (models/mlicpp.py) over the HIP engine.

    net = MLICPlusPlus(N=192, M=320, slice_num=10, channel=3).eval()
    net.load_state_dict(checkpoint["state_dict"]); net.update(force=True); net = net.to("cuda")
    out = net.compress(x)                              -> {"strings": [[y], [z]*B], "shape": (H/64, W/64)}
    rec = net.decompress(out["strings"], out["shape"]) -> {"x_hat": [B,C,H,W] (not clamped, :406-413)}
    fwd = net(x)                                       -> {"x_hat", "likelihoods": {"y_likelihoods", "z_likelihoods"}}

Residual blocks of 3x3 / 1x1 convolutions with GDN / IGDN and GELU, sub-pixel up-sampling, and a channel-slice entropy model:
slice_num slices of 32 channels, each coded in two checkerboard parts.  The anchor part of slice i is predicted from the hyper
prior and, from the second slice on, the linear global inter context and the channel context over the decoded slices; the
other part also from the local (5x5 window attention) and the linear global intra context of the decoded anchors.  A latent
residual prediction corrects each part in place.  The per-slice modules are the ones of mlic_context.py and mlic_slice.py; the
engine runs them on channel views of one state buffer, so no concatenation is written.  All parts of all
images of a call go into ONE rANS stream, slice-major, anchor part first (per_image_streams: one stream per image).  H and W
must be multiples of 64 and at least 128.  No CPU path.
"""
from .arch import MLIC_SLICE_CH, mlic_config, mlic_entries
from .elic import SingleCodec


class MLICPlusPlus(SingleCodec):
    _MODEL = "MLIC"
    _LIKELIHOOD_KEYS = ("y_likelihoods", "z_likelihoods")

    def __init__(self, config=None, channel=3, N=None, M=None, slice_num=None, init_seed=0, **kwargs):
        # (the reference's signature is MLICPlusPlus(config, channel): N, M and slice_num come from the config there)
        def pick(v, key, default):
            return int(v) if v is not None else int(config[key]) if config is not None and key in config else default

        N, M, slice_num = pick(N, "N", 192), pick(M, "M", 320), pick(slice_num, "slice_num", 10)
        if not 1 <= int(channel) <= 16:
            raise ValueError(f"channel must be 1 ... 16, got {channel}")
        if config is not None and int(config.get("context_window", 5)) != 5:
            raise NotImplementedError("MLIC: the local-context kernel is built for context_window 5")
        if M != MLIC_SLICE_CH * slice_num:
            raise NotImplementedError(f"MLIC: slices of {MLIC_SLICE_CH} channels (M = 32 * slice_num), got M={M}, slice_num={slice_num}")
        super().__init__(mlic_entries(N, M, slice_num, int(channel)), mlic_config(N, M, slice_num), int(channel), init_seed)

    def _synth_args(self):
        return {**super()._synth_args(), "N": self.N, "M": self.M}

    def _create_engine(self):
        return self._create("rgbd_elic_create_mlic", self.N, self.M, self.slice_num, self.channel)

    def _check_image(self, x):
        B, H, W = super()._check_image(x)
        if H < 128 or W < 128:
            raise ValueError("H and W must be at least 128 (h_a and h_s run 3x3 layers on the H/64 x W/64 grid)")
        return B, H, W

    def decompress(self, strings, shape):  # models/mlicpp.py:314-413
        if int(shape[0]) < 2 or int(shape[1]) < 2:
            raise ValueError("shape must be at least (2, 2): H and W of at least 128")
        out = super().decompress(strings, shape)
        out.pop("cost_time", None)  # (the reference times itself with a host clock; callers time the call)
        return out

    def update_resolutions(self, H, W):
        """The reference builds the local contexts' attention masks here (:190-197); the kernel derives them from the position."""

    # compress(), decompress() and the eval-mode forward() (mlicpp.py:77-188) are SingleCodec's.
