"""Fixtures of MLIC++'s attention contexts from the UNMODIFIED reference modules (modules/transform/context.py), run on the CPU
(python tests/golden/make_mlic_context.py; needs the reference and oracle/_ref, see _reference_loader.py):

  mlicctx_<case>.npz (the cases of tests/mlic_context_cases.py): input_seed, weight_seed (weights and inputs are regenerated
      from them: synth.synthetic_state_dict(model=...), mlic_context_cases.case_inputs), ref64 = the output of the reference
      module in float64 on the same inputs, rounded once to fp32; ref32 = its fp32 output, every ref32_stride-th channel (a
      fixed stride keeps each file below 1 MiB); for LocalContext max_score = the largest |score + bias| (mask not added)
      its softmax saw;
  mlicctx_floors.json: per case e_ref[b] = max |ref32 - ref64| / max |ref64| over the first b images, and max_score;
  mlicctx_state_dict.json: per module configuration, [name, shape] of the reference module's state_dict, in its order.

The ckbd_*_sequeeze helpers of the reference allocate in the default dtype, so the float64 pass runs under
torch.set_default_dtype(torch.float64); the reference itself is not touched.  No program text of it goes into these files."""
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


def run_case(ctx, mc, name):
    mod, n, H, W, seed = mc.CASES[name]
    cls, kw, wseed = mc.MODULES[mod]
    sd = mc.module_weights(mod)
    xs = mc.case_inputs(name)
    outs, smax = {}, 0.0
    for dt in (torch.float32, torch.float64):
        torch.set_default_dtype(dt)
        try:
            m = getattr(ctx, cls)(**kw).eval()
            m.load_state_dict(sd, strict=True)
            m = m.to(dt)
            seen = []
            if mod == "local":
                def pre(module, inp):  # the softmax's input: score + bias + mask; the mask taken out again
                    a = inp[0] - m.attn_mask.unsqueeze(0).unsqueeze(2).to(inp[0].dtype)
                    seen.append(float(a.abs().max()))
                m.softmax.register_forward_pre_hook(pre)
            with torch.no_grad():
                outs[dt] = m(*[x.to(dt) for x in xs])
            if seen:
                smax = max(seen)
        finally:
            torch.set_default_dtype(torch.float32)
    ref64, ref32 = outs[torch.float64], outs[torch.float32]
    e_ref = {str(b): float((ref32[:b].double() - ref64[:b]).abs().max() / ref64[:b].abs().max()) for b in mc.case_batches(name)}
    stride = 1
    while (ref64.numel() + ref32[:, ::stride].numel()) * 4 > 900_000:
        stride *= 2
    np.savez_compressed(os.path.join(HERE, f"mlicctx_{name}.npz"), input_seed=seed, weight_seed=wseed, ref64=ref64.float().numpy(),
                        ref32=ref32[:, ::stride].numpy(), ref32_stride=stride, max_score=np.float64(smax))
    print(f"mlicctx {name}: e_ref {e_ref}, max|S| {smax:.1f}, max|out| {float(ref64.abs().max()):.3f}, ref32 stride {stride}")
    return {"e_ref": e_ref, "max_score": smax}


def main():
    load_reference()
    import modules.transform.context as ctx

    import mlic_context_cases as mc

    torch.manual_seed(0)
    floors = {name: run_case(ctx, mc, name) for name in mc.CASES}
    with open(os.path.join(HERE, "mlicctx_floors.json"), "w") as f:
        json.dump(floors, f, indent=1)
    names = {mod: [[k, list(v.shape)] for k, v in getattr(ctx, cls)(**kw).state_dict().items()]
             for mod, (cls, kw, _) in mc.MODULES.items()}
    with open(os.path.join(HERE, "mlicctx_state_dict.json"), "w") as f:
        json.dump(names, f, indent=0)


if __name__ == "__main__":
    main()
