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
from .arch import ckbd_config, ckbd_entries
from .elic import SingleCodec


class Cheng2020AnchorwithCheckerboard(SingleCodec):
    _MODEL = "ckbd"

    def __init__(self, N=192, channel=3, init_seed=0, **kwargs):
        # (a config= keyword is accepted and ignored, as the reference's class swallows it in **kwargs)
        if int(N) not in (128, 192):
            raise ValueError(f"N must be 128 or 192 (the reference's quality levels), got {N}")
        if int(channel) not in (1, 3):
            raise ValueError(f"channel must be 3 or 1, got {channel}")
        super().__init__(ckbd_entries(int(N), int(channel)), ckbd_config(N), int(channel), init_seed)

    @classmethod
    def from_state_dict(cls, state_dict):  # waseda.py:83-89
        w = state_dict["g_a.0.conv1.weight"]
        net = cls(N=int(w.shape[0]), channel=int(w.shape[1]))
        net.load_state_dict(state_dict)
        return net

    def _synth_args(self):
        return {**super()._synth_args(), "N": self.N}

    def _create_engine(self):
        return self._create("rgbd_elic_create_ckbd", self.N, self.channel)

    # compress(), decompress() and the eval-mode forward() (Cheng2020withCKBD.py:52-71: y_hat = round(y), one parameter pass
    # over the context with its anchor outputs zeroed; likelihoods "y" / "z") are SingleCodec's.

    def validate(self, x):
        raise NotImplementedError("validate() (training-time distortion estimate) is not part of the inference path")
