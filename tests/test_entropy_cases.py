"""Are the cases of tests/entropy_cases.py worth running on the GPU?  (CPU only.)

  * the fp32 CPU restatement of every kernel passes the acceptance function the GPU outputs go through;
  * every deliberately wrong restatement (MUTANTS) is rejected by that same function on at least one case;
  * the references agree with tests/ckbd_ref.py's and tests/stf_single_ref.py's likelihoods to fp32 rounding;
  * every likelihood case puts >= 10 % of its positions on the floor, >= 30 % above 1e-6 and <= 2 % in the undecided band,
    and the planted edges (special scales, exact ties, non-integer fp32(out - mean), pad positions) are really there.
"""
import numpy as np
import pytest
import torch

import entropy_cases as ec
import stf_single_ref

FAMILY_CASES = [(fam, cid) for fam, (ids, _, _, _) in ec.FAMILIES.items() for cid in ids]


@pytest.mark.parametrize("fam,cid", FAMILY_CASES, ids=[f"{f}-{c}" for f, c in FAMILY_CASES])
def test_restatement_is_accepted(fam, cid):
    _, build, emulate, accept = ec.FAMILIES[fam]
    c = build(cid)
    stats = {}
    fails = accept(c, emulate(c), stats)
    print(fam, cid, stats)
    assert not fails, fails
    if "k0" in stats:
        assert stats["k"] == stats["k0"] and 0.5 < stats["k0"] < 4.0, stats  # the restatement's own k: ~1.8 on such grids


@pytest.mark.parametrize("fam,mutant", [(f, m) for f, ms in ec.MUTANTS.items() for m in ms])
def test_mutant_is_rejected(fam, mutant):
    ids, build, emulate, accept = ec.FAMILIES[fam]
    small = [i for i in ids if i != "grid"]  # (the large cases add nothing here)
    rejected = [cid for cid in small if accept(build(cid), emulate(build(cid), mutant))]
    print(fam, mutant, "rejected on", rejected)
    assert rejected, f"{fam}: the wrong restatement '{mutant}' passes every case"
    if mutant in ("perm_in", "perm_out"):
        perm_cases = [cid for cid in small if build(cid)["perm"]]
        assert set(rejected) == set(perm_cases)  # on every permuted case, and of course on no other


@pytest.mark.parametrize("fam,cid", [fc for fc in FAMILY_CASES if fc[0] in ("ckbd_est", "slice_est", "eb")],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_likelihood_case_conditions(fam, cid):
    c = ec.FAMILIES[fam][1](cid)
    floor, undecided, above = ec.share(c["ref"])
    print(fam, cid, f"floor {floor:.3f} undecided {undecided:.4f} above 1e-6 {above:.3f} of {c['ref']['lik64'].size}")
    assert floor >= 0.10 and above >= 0.30 and undecided <= 0.02
    if fam == "eb":
        assert (c["C"] < c["zcs"]) == cid.startswith("c24")
        med = c["prm"]["medians"]
        assert (med != np.rint(med)).all()
        assert np.abs(c["z"] - med.reshape(1, -1, 1, 1)).max() > 55
        d = (c["z"] - med.reshape(1, -1, 1, 1)).astype(np.float32)
        assert (np.abs(d - np.trunc(d)) == 0.5).sum() >= 10  # exact ties
        assert any((c["prm"][f"_matrix{i}"] > 20).any() for i in range(5))
        return
    y, mean, scale = c["y"], c["mean"], c["scale"]
    for s in ec.SPECIAL_SCALES:
        assert (scale == s).sum() >= 8, s
    d = (y - mean).astype(np.float32)
    for t in (0.5, 1.5, 2.5):
        assert (d == t).any() and (d == -t).any(), t
    out, v, _ = ec.gauss_steps32(y, mean, scale)
    assert (v != np.rint(v)).sum() >= 16  # fp32(out - mean) is no integer there
    assert np.abs(mean).max() > 25 and (v == 0).any()


def test_undecided_share_on_a_large_grid():
    y, mean, scale = ec.gauss_inputs("share", (96000,))
    ref = ec.gauss_reference(y, mean, scale)
    floor, undecided, above = ec.share(ref)
    print(f"floor {floor:.3f} undecided {undecided:.4f} ({int(ref['undecided'].sum())} of 96000) above 1e-6 {above:.3f}")
    assert undecided <= 0.02 and floor >= 0.10 and above >= 0.30
    _, v, sc = ec.gauss_steps32(y, mean, scale)
    lik = ec.gauss_lik32(v, sc)
    k0 = ec.gauss_k(lik, ref)
    j = ref["judged"]
    rel = (np.abs(lik - ref["lik64"])[j] / ref["lik64"][j]).max()
    print(f"fp32 restatement: k0 = {k0:.3f}, worst relative error {rel:.3g}")
    assert 1.0 < k0 < 3.0


def test_references_agree_with_the_model_restatements():
    """gc_likelihood (stf_single_ref.py; ckbd_ref.py states the same lines inline) is the fp32 torch form the fp64 reference
    is measured with: identical to gauss_lik32 on the same fp32 steps, and within k0 E of the fp64 reference."""
    y, mean, scale = ec.gauss_inputs("agree", (2, 16, 3, 6))
    ref = ec.gauss_reference(y, mean, scale)
    got = stf_single_ref.gc_likelihood(torch.from_numpy(y), torch.from_numpy(scale), torch.from_numpy(mean)).numpy()
    _, v, sc = ec.gauss_steps32(y, mean, scale)
    assert ec.bits_equal(got, ec.gauss_lik32(v, sc))
    assert ec.bits_equal((torch.round(torch.from_numpy(y) - torch.from_numpy(mean)) + torch.from_numpy(mean)).numpy(), ref["out"])
    assert ec.gauss_k(got, ref) < 4.0
    assert (got[ref["floor"]] == ec.FLOOR).all()
    # the factorised prior: the oracle's _eb_logits (used by both model restatements) on the same parameters
    from oracle import elic_oracle as eo

    c = ec.eb_case("c24p")
    sd = {f"eb.{k}": torch.from_numpy(v) for k, v in c["prm"].items()}
    out = c["ref"]["out"]
    B, C, h, w = out.shape
    v = torch.from_numpy(np.ascontiguousarray(out.transpose(1, 0, 2, 3).reshape(C, 1, -1)))
    lo, up = eo._eb_logits(sd, "eb", v - 0.5), eo._eb_logits(sd, "eb", v + 0.5)
    s = -torch.sign(lo + up)
    lik = torch.abs(torch.sigmoid(s * up) - torch.sigmoid(s * lo)).reshape(C, B, h, w).permute(1, 0, 2, 3).numpy()
    assert ec.bits_equal(np.ascontiguousarray(lik), ec.eb_lik(c["prm"], out))
    worst = ec.eb_decade_worst(np.maximum(lik, ec.FLOOR), c["ref"])
    print("factorised prior, fp32 restatement, worst relative error per decade:", [f"{x:.2g}" for x in worst])
    assert max(worst) < 1e-3


def test_layout_helpers():
    p = ec.cperm(np.arange(64))
    assert sorted(p) == list(range(64)) and (ec.cperm(p) == np.arange(64)).all() and p[1] == 4 and p[4] == 1 and p[17] == 20
    x = np.arange(2 * 32 * 3 * 4, dtype=np.float32).reshape(2, 32, 3, 4)
    t = ec.to_nhwc(x, 40, 1)
    assert t[1, 2, 3, 4] == x[1, 1, 2, 3] and (t[..., 32:] == ec.SENT).all() and ec.bits_equal(ec.from_nhwc(t, 32, 1), x)
    z = ec.to_zbuf(x[:, :24], 32, 1, np.float32(0))
    pads = [pc for pc in range(32) if ec.cperm(pc) >= 24]
    assert len(pads) == 8 and pads != list(range(24, 32)) and (z[..., pads] == 0).all()
    assert ec.bits_equal(ec.from_zbuf(z, 24, 1), x[:, :24])
    m = ec.anchor_mask(3, 6, True)
    assert m[0, 1] and m[1, 0] and not m[0, 0] and ec.bits_equal(ec.pack(x, 1)[0, 0], np.array([[1, 3], [4, 6], [9, 11]], np.float32))
    pos = ec.part_positions(2, 16, 3, 3, 1, [7, 500], 10)
    assert pos[1, 2, 1, 2] == 500 + 10 + (2 * 3 + 1) * 3 + 2
    pos = ec.part_positions(2, 16, 3, 3, 0, [11], 10)
    assert pos[1, 2, 1, 2] == 11 + 10 * 2 + ((1 * 16 + 2) * 3 + 1) * 3 + 2
