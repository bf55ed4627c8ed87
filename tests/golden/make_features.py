"""Fixtures of Feature_encoder / Feature_decoder from the UNMODIFIED reference modules (models/elic_master.py:15-53), run on
the CPU (python tests/golden/make_features.py; needs the reference and oracle/_ref, see _reference_loader.py):

  features_<case>.npz (the module cases of tests/features_cases.py): input_seed, weight_seed (weights and inputs are
      regenerated from them: synth.synthetic_state_dict(model="Feature_encoder" | "Feature_decoder"),
      features_cases.case_inputs), ref32 = the reference module's fp32 output on those inputs -- in full (flattened) for maps up
      to 13 x 7, else its values at the 2048 flat positions features_cases.positions() derives from the case seed;
  features_floors.json: per case, e_ref = max |ref32 - ref64| / max |ref64| over the whole output, ref64 = the same module in
      float64;
  features_state_dict.json: per net of features_cases.NETS, [name, shape] of the reference module's state_dict, in its order.

No program text of the reference goes into these files."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from _reference_loader import load_reference  # noqa: E402


def build(ref, fc, net):
    model, ci, co = fc.NETS[net]
    return ref[model](in_channel=ci, out_channel=co).eval()


def run_case(ref, fc, name):
    net, B, H, W, seed = fc.CASES[name]
    sd = fc.net_weights(net)
    x = fc.case_inputs(name)
    res = {}
    for dt in (torch.float32, torch.float64):
        m = build(ref, fc, net)
        m.load_state_dict(sd, strict=True)
        m = m.to(dt)
        with torch.no_grad():
            res[dt] = m(x.to(dt))
    r32, r64 = res[torch.float32], res[torch.float64]
    e_ref = float((r32.double() - r64).abs().max() / r64.abs().max())
    pos = fc.positions(name, r32.numel())
    np.savez_compressed(os.path.join(HERE, f"features_{name}.npz"), input_seed=seed, weight_seed=fc.WEIGHT_SEED,
                        ref32=r32.reshape(-1)[pos].numpy())
    print(f"features {name}: e_ref {e_ref:.3e}, max|out| {float(r64.abs().max()):.3f}, {len(pos)} values")
    return e_ref


def main():
    load_reference()
    from models.elic_master import Feature_decoder, Feature_encoder

    import features_cases as fc

    ref = {"Feature_encoder": Feature_encoder, "Feature_decoder": Feature_decoder}
    torch.manual_seed(0)
    floors = {name: run_case(ref, fc, name) for name in fc.CASES}
    with open(os.path.join(HERE, "features_floors.json"), "w") as f:
        json.dump(floors, f, indent=1)
    with open(os.path.join(HERE, "features_state_dict.json"), "w") as f:
        json.dump({net: [[k, list(v.shape)] for k, v in build(ref, fc, net).state_dict().items()] for net in fc.NETS}, f, indent=0)


if __name__ == "__main__":
    main()
