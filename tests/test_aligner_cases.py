"""tests/aligner_cases.py checked on the CPU against the fixtures of the unmodified reference: the float64 restatement
reproduces the reference's float64 output, its fp32 evaluation passes the bound of the GPU test, the synthetic weights drive
the attention scores past |S| = 10, and every deliberate mistake lands at least 100x the bound away on every case."""
import pytest
import torch

import aligner_cases as ac


@pytest.fixture(scope="module", params=list(ac.CASES))
def case(request):
    name = request.param
    x, g = ac.case_inputs(name)
    return name, ac.case_weights(name), x, g, ac.load_fixture(name)


def test_fixture_and_restatement_agree(case):
    name, sd, x, g, fx = case
    B, cin, cout, H, W, seed, wseed = ac.CASES[name]
    assert int(fx["input_seed"]) == seed and int(fx["weight_seed"]) == wseed
    assert fx["ref64"].shape == (B, cout, H, W)
    assert float(fx["max_score"]) >= 10.0  # the weights stress the softmax
    assert 0 < fx["e_ref"] < 1e-4
    out64 = ac.aligner(sd, x, g)
    assert ac.rel_err(out64, fx["ref64"]) < 2e-7  # (the fixture's float64 output is rounded once to fp32)
    st = int(fx["ref32_stride"])
    # (e_ref was taken against the float64 tensor itself; the stored one is off by up to half an fp32 ulp, 2^-24 of its max)
    assert ac.rel_err(torch.from_numpy(fx["ref32"]), fx["ref64"][:, ::st]) <= fx["e_ref"] + 2.0 ** -24
    e32 = ac.rel_err(ac.aligner(sd, x, g, dtype=torch.float32), fx["ref64"])
    print(f"aligner {name}: e_ref {fx['e_ref']:.3e}, fp32 restatement {e32:.3e}, bound {ac.FACTOR * fx['e_ref']:.3e}")
    assert e32 <= ac.FACTOR * fx["e_ref"]


def test_every_mistake_is_far_from_the_bound(case):
    name, sd, x, g, fx = case
    bound = ac.FACTOR * fx["e_ref"]
    margins = {m: ac.rel_err(ac.aligner(sd, x, g, m), fx["ref64"]) / bound for m in ac.MUTATIONS}
    print(f"aligner {name} sensitivity:", {m: round(v) for m, v in margins.items()})
    assert min(margins.values()) >= 100, margins
