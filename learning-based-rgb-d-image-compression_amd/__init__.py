"""MI355X-native ELIC_united encode/decode hot path.

The directory name is not a Python identifier; import it through the `rgbd_amd` alias package at the
repository root (`import rgbd_amd`), which resolves to this package.
"""
from . import arch, synth  # noqa: F401
from .arch import Config, model_config  # noqa: F401
from . import _lib, ans, distributed, entropy_models  # noqa: F401,E402
from ._lib import RgbdError  # noqa: F401,E402
from . import elic_united  # noqa: E402
from .elic_united import ELIC_united  # noqa: F401,E402
from .elic_united_r2d import ELIC_united_R2D  # noqa: F401,E402
from .elic import ELIC  # noqa: F401,E402
from .stf_united import STF_united, SymmetricalTransFormerUnited  # noqa: F401,E402
from .stf import STF, SymmetricalTransFormer  # noqa: F401,E402
from .ckbd import Cheng2020AnchorwithCheckerboard  # noqa: F401,E402
from .mlic import MLICPlusPlus  # noqa: F401,E402
from .master import MasterLatentCodec  # noqa: F401,E402  (in neither zoo table: DESIGN.md 7)

# models/__init__.py:11-20, "the complex ones first": the testers take the first zoo name that is a substring of the model
# name, so "ELIC_united_R2D" stands before "ELIC_united" before "ELIC", and "STF_united" before "STF"; "ckbd" comes last (no
# zoo name contains it and it contains none of them)
modelZoo = {"ELIC_united_R2D": ELIC_united_R2D, "ELIC_united": ELIC_united, "ELIC": ELIC,
            "STF_united": SymmetricalTransFormerUnited, "STF": SymmetricalTransFormer, "ckbd": Cheng2020AnchorwithCheckerboard}
elic_united.modelZoo = modelZoo  # (`from rgbd_amd.elic_united import modelZoo`, the name's first home, is this dict)
# Entries that came after tests/golden/model_surface_record.json was taken: `modelZoo` is held to that record's six names and
# their order (tests/test_model_surface.py), so younger classes stand here, and the testers look a name up in both (zoo_lookup).
# models/__init__.py:19: "MLIC" (no name of either table contains it and it contains none of them)
modelZooExtra = {"MLIC": MLICPlusPlus}
elic_united.modelZooExtra = modelZooExtra


def zoo_lookup(model_name):
    """The class of the first table name that is a substring of `model_name` (modelZoo first, in its order, then
    modelZooExtra), as the reference's testers pick a model (testing/tester.py:55-62); None when there is none."""
    for table in (modelZoo, modelZooExtra):
        for name, cls in table.items():
            if model_name.find(name) != -1:
                return cls
    return None


elic_united.zoo_lookup = zoo_lookup
from .aligner import Spatial_aligner, SynthesisTransformPlus  # noqa: F401,E402
from .mlic_context import LinearGlobalInterContext, LinearGlobalIntraContext, LocalContext  # noqa: F401,E402
from .mlic_slice import ChannelContext, EntropyParametersMLIC, LatentResidualPrediction  # noqa: F401,E402
from .pool import CodecPool  # noqa: F401,E402
from . import datautils, ioutils, metrics, tester  # noqa: F401,E402
from .tester import TesterSingle, TesterUnited  # noqa: F401,E402
