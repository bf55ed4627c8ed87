"""Fixtures of MLIC++'s per-slice networks from the UNMODIFIED reference modules (modules/transform/entropy.py
EntropyParametersMLIC, context.py ChannelContext, LRP.py LatentResidualPrediction), run on the CPU
(python tests/golden/make_mlic_slice.py; needs the reference and oracle/_ref, see _reference_loader.py):

  mlicslice_<case>.npz (the cases of tests/mlic_slice_cases.py): input_seed, weight_seed (weights and inputs are regenerated
      from them: synth.synthetic_state_dict(model=...), mlic_slice_cases.case_inputs), ref64 = the output of the reference
      module in float64 on the same inputs, rounded once to fp32; ref32 = its fp32 output, every ref32_stride-th channel (a
      fixed stride keeps each file below 1 MiB); gelu_min / gelu_max = the smallest and largest argument each nn.GELU of the
      module saw in the float64 run; for the LRP max_pretanh = the largest |x| that reached torch.tanh;
  mlicslice_floors.json: per case e_ref[b] = max |ref32 - ref64| / max |ref64| over the first b images, and the same extremes;
  mlicslice_state_dict.json: per module configuration, [name, shape] of the reference module's state_dict, in its order.

The reference itself is not touched (forward hooks read the extremes).  No program text of it goes into these files."""
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


def run_case(classes, mc, name):
    mod, n, H, W, seed = mc.CASES[name]
    cls, kw, wseed = mc.MODULES[mod]
    sd = mc.module_weights(mod)
    x = torch.cat(mc.case_inputs(name), dim=1)
    outs, gelu_seen, pretanh = {}, [], []
    for dt in (torch.float32, torch.float64):
        m = classes[cls](**kw).eval()
        m.load_state_dict(sd, strict=True)
        m = m.to(dt)
        if dt == torch.float64:
            for sub in m.modules():
                if isinstance(sub, torch.nn.GELU):
                    sub.register_forward_pre_hook(lambda _m, inp: gelu_seen.append((float(inp[0].min()), float(inp[0].max()))))
            if cls == "LatentResidualPrediction":
                m.lrp_transform.register_forward_hook(lambda _m, _i, out: pretanh.append(float(out.abs().max())))
        with torch.no_grad():
            outs[dt] = m(x.to(dt))
    ref64, ref32 = outs[torch.float64], outs[torch.float32]
    e_ref = {str(b): float((ref32[:b].double() - ref64[:b]).abs().max() / ref64[:b].abs().max()) for b in mc.case_batches(name)}
    stride = 1
    while (ref64.numel() + ref32[:, ::stride].numel()) * 4 > 900_000:
        stride *= 2
    gmin, gmax = [g[0] for g in gelu_seen], [g[1] for g in gelu_seen]
    extra = {"max_pretanh": np.float64(pretanh[0])} if pretanh else {}
    np.savez_compressed(os.path.join(HERE, f"mlicslice_{name}.npz"), input_seed=seed, weight_seed=wseed, ref64=ref64.float().numpy(),
                        ref32=ref32[:, ::stride].numpy(), ref32_stride=stride, gelu_min=np.float64(gmin), gelu_max=np.float64(gmax),
                        **extra)
    print(f"mlicslice {name}: e_ref {e_ref}, gelu args {[f'{a:.1f}..{b:.1f}' for a, b in gelu_seen]}, "
          f"max|pretanh| {pretanh[0] if pretanh else float('nan'):.2f}, max|out| {float(ref64.abs().max()):.3f}, ref32 stride {stride}")
    floors = {"e_ref": e_ref, "gelu_min": gmin, "gelu_max": gmax}
    if pretanh:
        floors["max_pretanh"] = pretanh[0]
    return floors


def main():
    load_reference()
    from modules.transform.context import ChannelContext
    from modules.transform.entropy import EntropyParametersMLIC
    from modules.transform.LRP import LatentResidualPrediction

    import mlic_slice_cases as mc

    classes = {"EntropyParametersMLIC": EntropyParametersMLIC, "ChannelContext": ChannelContext,
               "LatentResidualPrediction": LatentResidualPrediction}
    torch.manual_seed(0)
    floors = {name: run_case(classes, mc, name) for name in mc.CASES}
    with open(os.path.join(HERE, "mlicslice_floors.json"), "w") as f:
        json.dump(floors, f, indent=1)
    names = {mod: [[k, list(v.shape)] for k, v in classes[cls](**kw).state_dict().items()]
             for mod, (cls, kw, *_) in list(mc.MODULES.items()) + list(mc.SHAPE_ONLY.items())}
    with open(os.path.join(HERE, "mlicslice_state_dict.json"), "w") as f:
        json.dump(names, f, indent=0)


if __name__ == "__main__":
    main()
