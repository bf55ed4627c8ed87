"""`STF_united` (SymmetricalTransFormerUnited) on MI355X: the reference's Swin-transform variant of ELIC_united
(models/stf_united.py:605-678) over the HIP engine.  Same API and return values as ELIC_united; N=192, M=384 and the
slice widths [24,24,48,96,192] are fixed by the model (stf_united.py:638-640)."""
from .arch import stf_config, stf_united_entries
from .elic_united import ELIC_united


class SymmetricalTransFormerUnited(ELIC_united):
    _MODEL = "STF_united"
    _ENTRIES = staticmethod(stf_united_entries)

    def __init__(self, config=None, channel=4, init_seed=0, **kwargs):
        super().__init__(config=stf_config(), channel=channel, init_seed=init_seed)

    def _create_engine(self):
        return self._create("rgbd_elic_create_stf", self.N, self.M, self.slice_ch)


STF_united = SymmetricalTransFormerUnited
