"""Fixtures of Channel_aligner from the UNMODIFIED reference module (modules/transform/channelAligner.py), run on the CPU
(python tests/golden/make_chalign.py; needs the reference and oracle/_ref, see _reference_loader.py):

  chalign_<case>.npz (the module cases of tests/chalign_cases.py): input_seed, weight_seed (weights and inputs are regenerated
      from them: synth.synthetic_state_dict(model="Channel_aligner"), chalign_cases.case_inputs), beta64 / gamma64 = the
      reference module's beta and gamma in float64 on the same inputs, rounded once to fp32, as [B,64]; beta32 / gamma32 = its
      fp32 results.  `out` is not stored: the tests rebuild it in fp64 from feature2, beta64 and gamma64;
  chalign_floors.json: per case and output ("out", "beta", "gamma"), e_ref[b] = max |ref32 - ref64| / max |ref64| over the
      first b images;
  chalign_state_dict.json: [name, shape] of the reference module's state_dict, in its order.

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


def run_case(ref_cls, cc, name):
    B, H, W, seed = cc.CASES[name]
    sd = cc.module_weights()
    f1, f2 = cc.case_inputs(name)
    res = {}
    for dt in (torch.float32, torch.float64):
        m = ref_cls().eval()
        m.load_state_dict(sd, strict=True)
        m = m.to(dt)
        with torch.no_grad():
            out, beta, gamma = m(f1.to(dt), f2.to(dt))
        res[dt] = {"out": out, "beta": beta.reshape(B, 64), "gamma": gamma.reshape(B, 64)}
    r32, r64 = res[torch.float32], res[torch.float64]
    floors = {k: {str(b): float((r32[k][:b].double() - r64[k][:b]).abs().max() / r64[k][:b].abs().max()) for b in range(1, B + 1)}
              for k in ("out", "beta", "gamma")}
    np.savez_compressed(os.path.join(HERE, f"chalign_{name}.npz"), input_seed=seed, weight_seed=cc.WEIGHT_SEED,
                        beta64=r64["beta"].float().numpy(), gamma64=r64["gamma"].float().numpy(),
                        beta32=r32["beta"].numpy(), gamma32=r32["gamma"].numpy())
    bias = max(float(sd[f"{n}.bias"].abs().max()) for n in ("conv2", "conv3"))
    print(f"chalign {name}: e_ref {floors}, max|beta| {float(r64['beta'].abs().max()):.3f}, max|gamma| "
          f"{float(r64['gamma'].abs().max()):.3f}, max|head bias| {bias:.3f}")
    return floors


def main():
    load_reference()
    from modules.transform.channelAligner import Channel_aligner

    import chalign_cases as cc

    torch.manual_seed(0)
    floors = {name: run_case(Channel_aligner, cc, name) for name in cc.CASES}
    with open(os.path.join(HERE, "chalign_floors.json"), "w") as f:
        json.dump(floors, f, indent=1)
    with open(os.path.join(HERE, "chalign_state_dict.json"), "w") as f:
        json.dump([[k, list(v.shape)] for k, v in Channel_aligner().state_dict().items()], f, indent=0)


if __name__ == "__main__":
    main()
