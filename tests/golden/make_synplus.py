"""Fixtures of SynthesisTransformPlus from the UNMODIFIED reference, run on the CPU (python tests/golden/make_synplus.py; needs
the reference and oracle/_ref, see _reference_loader.py):

  synplus_<case>.npz (the cases of tests/synplus_cases.py): input_seed, weight_seed (weights and inputs are regenerated from
      them: synth.synthetic_state_dict(model="SynthesisTransformPlus"), synplus_cases.case_inputs); shape; ref64 = the output
      of the reference module in .double() on the same inputs, rounded once to fp32 -- the whole tensor, or (case c, whose
      tensor would exceed the size a fixture keeps) its values at idx = synplus_cases.sample_positions(shape, input_seed):
      every border pixel and 160 seeded interior pixels of every channel; ref64_max = max |ref64| over the whole tensor;
      ref32 = every ref32_stride-th of the same values from the fp32 run; max_scores = the largest |score| (bias added, mask
      not) each of the six attentions saw, in the order sp1.blocks.0, sp1.blocks.1, sp2.blocks.0, ...;
  synplus_floors.json: per case e_ref = max |ref32 - ref64| / max |ref64| over the whole tensors, and max_scores;
  synplus_state_dict.json: [name, shape] of the reference module's state_dict (N = 192, M = 320, ch = 3), in its order.

No program text of the reference goes into any of these."""
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

REF32_STRIDE = 4


def synplus_case(STP, sc, name):
    B, ch, h, w, seed, wseed = sc.CASES[name]
    sd = sc.case_weights(name)
    ins = sc.case_inputs(name)
    outs, scores = {}, None
    for dt in (torch.float32, torch.float64):
        m = STP(sc.N, sc.M, ch=ch).eval()
        m.load_state_dict(sd, strict=True)
        m = m.to(dt)
        seen = []

        def hook(blk):
            def pre(mod, inp):  # the softmax's input: scores + bias (+ mask, taken out again)
                a = inp[0]
                if blk.attn_mask is not None:
                    nW = blk.attn_mask.shape[0]
                    a = a.view(a.shape[0] // nW, nW, *a.shape[1:]) - blk.attn_mask.unsqueeze(1).unsqueeze(0).to(a.dtype)
                seen.append(float(a.abs().max()))
            return pre

        for sp in (m.sp1, m.sp2, m.sp3):
            for blk in sp.blocks:
                blk.attn.softmax.register_forward_pre_hook(hook(blk))
        with torch.no_grad():
            outs[dt] = m(*(t.to(dt) for t in ins))
        scores = seen
    ref64, ref32 = outs[torch.float64], outs[torch.float32]
    assert tuple(ref64.shape) == (B, ch, 16 * h, 16 * w) and len(scores) == 6
    ref_max = float(ref64.abs().max())
    e_ref = float((ref32.double() - ref64).abs().max() / ref_max)
    g = {"input_seed": seed, "weight_seed": wseed, "shape": np.array(ref64.shape, np.int32), "ref64_max": np.float64(ref_max),
         "ref32_stride": REF32_STRIDE, "max_scores": np.array(scores, np.float64)}
    if ref64.numel() > sc.SAMPLE_LIMIT:
        g["idx"] = sc.sample_positions(tuple(ref64.shape), seed)
        assert g["idx"].size >= 65536
    fx = {"idx": g["idx"]} if "idx" in g else {}
    g["ref64"] = sc.compared(ref64, fx).float().numpy()
    g["ref32"] = sc.compared(ref32, fx)[::REF32_STRIDE].numpy()
    np.savez_compressed(os.path.join(HERE, f"synplus_{name}.npz"), **g)
    print(f"synplus {name}: e_ref {e_ref:.3e}, max|S| {[round(s, 1) for s in scores]}, max|out| {ref_max:.3f}, "
          f"{g['ref64'].size} of {ref64.numel()} values, {os.path.getsize(os.path.join(HERE, f'synplus_{name}.npz'))} bytes")
    return {"e_ref": e_ref, "max_scores": scores}


def main():
    load_reference()
    from modules.transform.synthesis import SynthesisTransformPlus as STP

    import synplus_cases as sc

    torch.manual_seed(0)
    floors = {name: synplus_case(STP, sc, name) for name in sc.CASES}
    with open(os.path.join(HERE, "synplus_floors.json"), "w") as f:
        json.dump(floors, f, indent=1)
    names = [[k, list(v.shape)] for k, v in STP(sc.N, sc.M, ch=3).state_dict().items()]
    with open(os.path.join(HERE, "synplus_state_dict.json"), "w") as f:
        json.dump(names, f, indent=0)


if __name__ == "__main__":
    main()
