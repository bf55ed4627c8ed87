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
from .arch import stf_entries, stf_single_config
from .elic import SingleCodec


class SymmetricalTransFormer(SingleCodec):
    _MODEL = "STF"

    def __init__(self, config=None, channel=3, init_seed=0, **kwargs):
        # (config, and the reference's keyword arguments -- pretrain_img_size, embed_dim, depths, ... -- are accepted and
        #  ignored: the engine implements the reference's defaults, which is what its zoo and testers build)
        super().__init__(stf_entries(channel), stf_single_config(), channel, init_seed)
        self.num_slices = self.slice_num
        self.max_support_slices = self.num_slices // 2

    @classmethod
    def from_state_dict(cls, state_dict):  # stf.py:696-701
        net = cls()
        net.load_state_dict(state_dict)
        return net

    def _create_engine(self):
        return self._create("rgbd_elic_create_stf_single", self.channel)

    # compress(), decompress() and the eval-mode forward() (stf.py:618-678: x_hat not clamped, likelihoods "y" / "z") are
    # SingleCodec's: the engine created above runs the channel-slice entropy model behind the same entry points.


STF = SymmetricalTransFormer
