"""`ELIC_united_R2D` on MI355X: the reference's one-directional variant (models/elic_united_R2D.py) over the HIP engine --
RGB is coded without looking at depth, depth is conditioned on RGB.  Same API and return values as ELIC_united."""
from .arch import elic_united_r2d_entries
from .elic_united import ELIC_united


class ELIC_united_R2D(ELIC_united):
    _MODEL = "ELIC_united_R2D"
    _ENTRIES = staticmethod(elic_united_r2d_entries)

    def _create_engine(self):
        return self._create("rgbd_elic_create_r2d", self.N, self.M, self.slice_ch)

    # forward(), compress_united() and decompress_united() are inherited, exactly as in the reference
    # (models/elic_united_R2D.py overrides only the per-slice coders of models/elic_united.py): the engine created above
    # (variant "r2d") runs the one-directional slice coder and the single-input hyper synthesis behind them.
