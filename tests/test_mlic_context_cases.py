"""tests/mlic_context_cases.py against the fixtures of the unmodified reference (tests/golden/mlicctx_*.npz), on the CPU:

  * the fp64 statements of the three modules reproduce every fixture's ref64 far inside the acceptance bound, at every batch
    size of the case, and LocalContext's scores sit in the band the cases are built for;
  * each deliberate mistake of the local attention, of the linear attention and of the checkerboard token sets lands outside
    the bound -- on non-square maps with more than one head, where none of them hides;
  * the key softmax without its maximum taken off fails on the case built to overflow fp32 without it;
  * the state-dict entries of the package are those of the reference (names, order, shapes)."""
import json
import os

import pytest
import torch

import mlic_context_cases as mc


@pytest.mark.parametrize("name", list(mc.CASES))
def test_statement_reproduces_reference(name):
    fx = mc.load_fixture(name)
    ref64 = torch.from_numpy(fx["ref64"])
    assert int(fx["input_seed"]) == mc.CASES[name][4] and int(fx["weight_seed"]) == mc.MODULES[mc.CASES[name][0]][2]
    for b in mc.case_batches(name):
        e = mc.rel_err(mc.module_statement(name, b), ref64[:b])
        print(f"{name} B={b}: statement vs ref64 {e:.3e}, e_ref {mc.e_ref(fx, b):.3e}")
        assert 1e-8 < mc.e_ref(fx, b) < 5e-6  # an fp32 run's error, not an accident
        assert e <= 0.5 * mc.e_ref(fx, b)  # ref64 is stored rounded to fp32: 6e-8 of its own
    # the strided fp32 output is the same run the floor was taken from
    s = int(fx["ref32_stride"])
    assert mc.rel_err(fx["ref32"], ref64[:, ::s]) <= mc.e_ref(fx, mc.case_batches(name)[-1]) + 1.2e-7  # (ref64's own rounding)


@pytest.mark.parametrize("name", [n for n in mc.CASES if mc.CASES[n][0] == "local"])
def test_local_scores_in_band(name):
    fx = mc.load_fixture(name)
    _, smax = mc.local_context(mc.module_weights("local"), mc.case_inputs(name)[0], want_score=True)
    assert abs(smax - float(fx["max_score"])) <= 1e-3 * smax
    assert mc.SCORE_BAND[0] <= float(fx["max_score"]) <= mc.SCORE_BAND[1]


def _outside(name, mut):
    fx = mc.load_fixture(name)
    b = mc.case_batches(name)[-1]
    e = mc.rel_err(mc.module_statement(name, b, mut), torch.from_numpy(fx["ref64"])[:b])
    print(f"{name} {mut}: {e:.3e} vs bound {mc.FACTOR * mc.e_ref(fx, b):.3e}")
    return e > 100 * mc.FACTOR * mc.e_ref(fx, b)


@pytest.mark.parametrize("mut", mc.LOCAL_MUTATIONS)
@pytest.mark.parametrize("name", ["local_8x12", "local_12x8"])
def test_local_mistakes_land_outside(name, mut):
    assert _outside(name, mut)


@pytest.mark.parametrize("mut", mc.LINEAR_MUTATIONS + mc.INTRA_MUTATIONS)
@pytest.mark.parametrize("name", ["intra_8x12", "intra_12x8"])
def test_intra_mistakes_land_outside(name, mut):
    assert _outside(name, mut)


@pytest.mark.parametrize("mut", mc.LINEAR_MUTATIONS)
@pytest.mark.parametrize("name", ["inter32_8x12", "inter96_12x8", "inter288_4x20"])
def test_inter_mistakes_land_outside(name, mut):
    assert _outside(name, mut)


def test_no_max_overflows_where_built_to():
    k, q, v = mc.linear_kernel_inputs(1, 4, 6, 2, 16, 7, key_offset=100.0)
    ref = mc.linear_attention(k, q, v, 2, 0)
    good = mc.linear_attention(k, q, v, 2, 0, dtype=torch.float32)
    bad = mc.linear_attention(k, q, v, 2, 0, mut="no_max", dtype=torch.float32)
    assert mc.rel_err(good, ref) < 1e-5
    assert not (mc.rel_err(bad, ref) < 1e-5)  # inf / inf: not a number, which no bound accepts


@pytest.mark.parametrize("mod", list(mc.MODULES))
def test_entries_are_the_reference_state_dict(mod):
    from rgbd_amd import arch

    with open(os.path.join(mc.GOLDEN, "mlicctx_state_dict.json")) as f:
        want = json.load(f)[mod]
    cls, kw, _ = mc.MODULES[mod]
    ent = {"LocalContext": lambda: arch.local_context_entries(kw["dim"]),
           "LinearGlobalIntraContext": lambda: arch.linear_global_intra_entries(kw["dim"]),
           "LinearGlobalInterContext": lambda: arch.linear_global_inter_entries(kw["dim"], kw.get("out_dim", 64))}[cls]()
    assert [[k, list(e.shape)] for k, e in ent.items()] == want
    sd = mc.module_weights(mod)
    assert [[k, list(v.shape)] for k, v in sd.items()] == want
