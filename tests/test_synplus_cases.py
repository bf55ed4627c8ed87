"""tests/synplus_cases.py checked on the CPU against the fixtures of the unmodified reference: the float64 restatement of
SynthesisTransformPlus reproduces the reference's float64 output, its fp32 evaluation passes the bound of the GPU test, the
synthetic weights drive all six attentions well away from a uniform softmax, every deliberate mistake in the walk lands at
least 10x the bound away (shown on cases a and b), and arch.synthesis_plus_entries names what the reference's state_dict
names, in its order."""
import json
import os

import numpy as np
import pytest
import torch

import synplus_cases as sc

MISTAKE_CASES = ["a", "b"]


@pytest.fixture(scope="module", params=list(sc.CASES))
def case(request):
    name = request.param
    return name, sc.case_weights(name), sc.case_inputs(name), sc.load_fixture(name)


def test_fixture_and_restatement_agree(case):
    name, sd, ins, fx = case
    B, ch, h, w, seed, wseed = sc.CASES[name]
    assert int(fx["input_seed"]) == seed and int(fx["weight_seed"]) == wseed
    assert tuple(fx["shape"]) == (B, ch, 16 * h, 16 * w)
    n = B * ch * 256 * h * w
    if "idx" in fx:  # a sampled fixture: at least 65,536 values, every channel, the image borders
        assert fx["ref64"].size == fx["idx"].size >= 65536
        assert np.array_equal(fx["idx"], sc.sample_positions(tuple(fx["shape"]), seed))
        H, W = 16 * h, 16 * w
        plane, pix = fx["idx"] // (H * W), fx["idx"] % (H * W)
        assert np.array_equal(np.unique(plane), np.arange(B * ch))
        border = 2 * H + 2 * W - 4
        yy, xx = pix // W, pix % W
        assert int(((yy == 0) | (yy == H - 1) | (xx == 0) | (xx == W - 1)).sum()) == border * B * ch
    else:
        assert fx["ref64"].size == n
        assert float(np.abs(fx["ref64"]).max()) == pytest.approx(float(fx["ref64_max"]), rel=1e-6)
    scores = [float(s) for s in fx["max_scores"]]
    print(f"synplus {name}: max|S| of sp1.blocks.0 ... sp3.blocks.1 {[round(s, 1) for s in scores]}")
    assert len(scores) == 6 and min(scores) >= 10.0  # every attention is stressed ...
    assert all(15.0 <= max(scores[2 * k:2 * k + 2]) <= 26.0 for k in range(3))  # ... every aligner about as far as when it stands alone
    assert 0 < fx["e_ref"] < 1e-4
    out64 = sc.synthesis_plus(sd, *ins)
    assert tuple(out64.shape) == tuple(fx["shape"])
    e64 = sc.rel_err(out64, fx)
    assert e64 < 2e-7  # (the fixture's float64 output is rounded once to fp32)
    st = int(fx["ref32_stride"])
    # (e_ref was taken against the float64 tensor itself; the stored one is off by up to half an fp32 ulp, 2^-24 of its max)
    d32 = np.abs(fx["ref32"].astype(np.float64) - fx["ref64"].reshape(-1)[::st].astype(np.float64)).max() / float(fx["ref64_max"])
    assert d32 <= fx["e_ref"] + 2.0 ** -24
    e32 = sc.rel_err(sc.synthesis_plus(sd, *ins, dtype=torch.float32), fx)
    print(f"synplus {name}: e_ref {fx['e_ref']:.3e}, fp64 restatement {e64:.3e}, fp32 restatement {e32:.3e}, "
          f"bound {sc.FACTOR * fx['e_ref']:.3e}")
    assert e32 <= sc.FACTOR * fx["e_ref"]


@pytest.mark.parametrize("name", MISTAKE_CASES)
def test_every_mistake_is_far_from_the_bound(name):
    sd, ins, fx = sc.case_weights(name), sc.case_inputs(name), sc.load_fixture(name)
    bound = sc.FACTOR * fx["e_ref"]
    margins = {m: sc.rel_err(sc.synthesis_plus(sd, *ins, mut=m), fx) / bound for m in sc.MUTATIONS}
    print(f"synplus {name} sensitivity:", {m: round(v) for m, v in margins.items()})
    assert min(margins.values()) >= 10, margins


@pytest.mark.parametrize("ch", [3])
def test_entries_are_the_references_state_dict(ch):
    from rgbd_amd import arch

    with open(os.path.join(sc.GOLDEN, "synplus_state_dict.json")) as f:
        ref = [(k, tuple(s)) for k, s in json.load(f)]
    ours = [(k, tuple(e.shape)) for k, e in arch.synthesis_plus_entries(sc.N, sc.M, ch).items()]
    assert ours == ref


def test_entries_follow_ch_and_the_recipe_covers_them():
    from rgbd_amd import arch, synth

    for ch in (1, 192):
        e = arch.synthesis_plus_entries(sc.N, sc.M, ch)
        assert e["synthesis_transform.14.weight"].shape == (sc.N, ch, 5, 5) and e["synthesis_transform.14.bias"].shape == (ch,)
        assert e["sp3.recovery.weight"].shape == (96, 192, 2, 2)
    sd = synth.synthetic_state_dict(11, model="SynthesisTransformPlus", channel=3)
    assert list(sd) == list(arch.synthesis_plus_entries(sc.N, sc.M, 3))
    # the three aligners are stressed alike and do not share their values
    assert not torch.equal(sd["sp1.blocks.0.norm1.weight"], sd["sp2.blocks.0.norm1.weight"])
    assert float(sd["sp2.blocks.1.norm2.weight"].min()) < 0.7 and float(sd["sp3.blocks.0.attn.relative_position_bias_table"].std()) > 0.5
