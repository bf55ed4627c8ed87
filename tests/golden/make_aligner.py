"""Fixtures of Spatial_aligner and of ELIC(return_mid=True) from the UNMODIFIED reference, run on the CPU
(python tests/golden/make_aligner.py; needs the reference and oracle/_ref, see _reference_loader.py):

  aligner_<case>.npz (the cases of tests/aligner_cases.py): input_seed, weight_seed (weights and inputs are regenerated from
      them: synth.synthetic_state_dict(model="Spatial_aligner"), aligner_cases.case_inputs), ref64 = the output of the
      reference module in .double() on the same inputs, rounded once to fp32; ref32 = its fp32 output, every
      ref32_stride-th channel (a fixed stride keeps each file below 1 MiB); max_score = the largest |score| (bias added,
      mask not) its two attentions saw;
  aligner_floors.json: per case e_ref = max |ref32 - ref64| / max |ref64| over the whole tensors, and max_score;
  aligner_state_dict.json: [name, shape] of the reference module's state_dict (in = out = 192), in its order;
  elic_mid_c1_256x256.npz: the reference ELIC(return_mid=True), weight seed 0, on the image of elic_c1_256x256.npz (the
      generator asserts that its streams equal that fixture's): up1..up3 as up[:, ::8, ::4, ::4] and each tensor's max |.|.

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


def aligner_case(SA, ac, name):
    B, cin, cout, H, W, seed, wseed = ac.CASES[name]
    sd = ac.case_weights(name)
    x, g = ac.case_inputs(name)
    outs, smax = {}, 0.0
    for dt in (torch.float32, torch.float64):
        m = SA(in_channel=cin, out_channel=cout).eval()
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

        for blk in m.blocks:
            blk.attn.softmax.register_forward_pre_hook(hook(blk))
        with torch.no_grad():
            outs[dt] = m(x.to(dt), g.to(dt))
        smax = max(seen)
    ref64 = outs[torch.float64]
    e_ref = float((outs[torch.float32].double() - ref64).abs().max() / ref64.abs().max())
    stride = 1
    while (ref64.numel() + ref64[:, ::stride].numel()) * 4 > 900_000:
        stride *= 2
    np.savez_compressed(os.path.join(HERE, f"aligner_{name}.npz"), input_seed=seed, weight_seed=wseed,
                        ref64=ref64.float().numpy(), ref32=outs[torch.float32][:, ::stride].numpy(), ref32_stride=stride,
                        max_score=np.float64(smax))
    print(f"aligner {name}: e_ref {e_ref:.3e}, max|S| {smax:.1f}, max|out| {float(ref64.abs().max()):.3f}, ref32 stride {stride}")
    return {"e_ref": e_ref, "max_score": smax}


def elic_mid(ext, model_config, synth):
    fx = np.load(os.path.join(HERE, "elic_c1_256x256.npz"))
    net = ext["ELIC"](config=model_config(), channel=3, return_mid=True).eval()
    net.load_state_dict(synth.synthetic_state_dict(0, model="ELIC"))
    assert net.update(force=True)
    r, _ = synth.synthetic_batch(1, 256, 256, config_id=int(fx["config_id"]))
    # (the reference's floats depend on how oneDNN splits a convolution over its threads: DESIGN.md 4a.  One thread is where
    # this run reproduces the streams of the fixture, which the assertion below holds it to.)
    torch.set_num_threads(1)
    with torch.no_grad():
        out = net.compress(torch.from_numpy(r))
        assert out["strings"][0][0] == fx["y_stream"].tobytes() and out["strings"][1][0] == fx["z0"].tobytes()
        dec = net.decompress(out["strings"], out["shape"])
    dx = float(np.abs(dec["x_hat"][:, :, ::4, ::4].numpy() - fx["xhat_sub"]).max())
    print("elic mid: max |x_hat - fixture's x_hat|", dx)
    assert dx < 1e-5  # the same decode (the synthesis transform's last bits move with the thread split)
    g = {}
    for k in ("up1", "up2", "up3"):
        g[k] = dec[k][:, ::8, ::4, ::4].numpy()
        g[k + "_shape"] = np.array(dec[k].shape, np.int32)
        g[k + "_max"] = np.float64(dec[k].abs().max())
        print("elic mid", k, tuple(dec[k].shape), float(g[k + "_max"]))
    np.savez_compressed(os.path.join(HERE, "elic_mid_c1_256x256.npz"), **g)


def main():
    _, model_config, ext = load_reference()
    from modules.transform.spatialAligner import Spatial_aligner as SA

    import aligner_cases as ac
    from rgbd_amd import synth

    torch.manual_seed(0)
    floors = {name: aligner_case(SA, ac, name) for name in ac.CASES}
    with open(os.path.join(HERE, "aligner_floors.json"), "w") as f:
        json.dump(floors, f, indent=1)
    names = [[k, list(v.shape)] for k, v in SA(in_channel=192, out_channel=192).state_dict().items()]
    with open(os.path.join(HERE, "aligner_state_dict.json"), "w") as f:
        json.dump(names, f, indent=0)
    if "--no-elic" not in sys.argv:
        elic_mid(ext, model_config, synth)


if __name__ == "__main__":
    main()
