"""Are the cases of tests/msssim_cases.py worth running on the GPU?  (CPU only.)

  * the fp32 CPU restatement of the kernels passes the acceptance function the GPU output goes through, at a ratio of at most 1;
  * every deliberately wrong restatement (MUTANTS) is rejected by that same function, the tile-edge ones on the cases whose
    scale-0 map ends on or one past a tile edge, the pooling ones on odd sides, `range` on family h, `c_swap` on family d;
  * the inputs are what the cases claim: a plane with CS < 0 and one with CS > 0.9 in every case, a luminance factor away from 1
    in family d, the chains of map sizes of the table, and no E32 anywhere near the cap;
  * stats64 folded by relu, weights, product and mean is oracle/msssim_ref.py's ms_ssim.
"""
import numpy as np
import pytest

import msssim_cases as mc
from oracle import msssim_ref


@pytest.mark.parametrize("cid", mc.IDS)
def test_restatement_is_accepted(cid):
    c = mc.build(cid)
    stats = {}
    fails = mc.accept(c, mc.emulate(c), stats)
    print(f"{cid}: E32 {stats['E32']:.3g}, ratio {stats['ratio']:.3f}; E32 per scale (ssim, cs): " +
          " ".join(f"{a:.2g},{b:.2g}" for a, b in c["E32"]))
    assert not fails, fails
    assert stats["ratio"] <= 1.0  # by construction: E32 is this very distance
    assert c["E32"].max() < mc.CAP  # a broken restatement cannot open the bound


@pytest.mark.parametrize("mutant", mc.MUTANTS)
def test_mutant_is_rejected(mutant):
    rejected = [cid for cid in mc.SMALL if mc.accept(mc.build(cid), mc.emulate(mc.build(cid), mutant))]  # (planes65 adds nothing here)
    print(mutant, "rejected on", rejected)
    assert rejected, f"the wrong restatement '{mutant}' passes every case"
    odd = [cid for cid in mc.SMALL if mc.build(cid)["H"] % 2 or mc.build(cid)["W"] % 2]
    must = {"drop_pixel": ["one_over", "exact_tiles"], "edge_row": ["one_over", "exact_tiles"], "edge_col": ["one_over", "exact_tiles"],
            "pool_divisor": odd, "pool_pad": odd, "range": ["range255", "range_half"],
            "c_swap": [cid for cid in mc.SMALL if "d" in mc.build(cid)["fam"]],
            "no_clamp": ["clamp1"], "clamp_pool_after": ["clamp1"], "clamp_pool_skip": ["clamp1"], "always_clamp": ["clamp0"]}
    if mutant in must:
        assert set(rejected) & set(must[mutant]), (mutant, rejected, must[mutant])
    if mutant == "range":
        assert set(rejected) == {"range255", "range_half"}  # (on every other case the mutant is the restatement)
    if mutant in ("drop_pixel", "edge_row", "edge_col"):
        assert {"one_over", "exact_tiles"} <= set(rejected)


def test_mutants_are_judged_per_plane_of_family_d():
    """c_swap must be caught ON a dark plane (not only somewhere in a case that has one)"""
    for cid in ("min_odd", "wide"):
        c = mc.build(cid)
        p = c["fam"].index("d")
        err = np.abs(mc.emulate(c, "c_swap")[p].astype(np.float64) - c["ref"][p])
        assert (err > 4 * c["unit"][p]).any(), cid


@pytest.mark.parametrize("cid", mc.IDS)
def test_case_conditions(cid):
    c = mc.build(cid)
    cs0 = c["ref"][:, 0, 1]
    print(cid, "fp64 CS at scale 0:", np.round(cs0[:8], 4), "families", "".join(c["fam"][:8]))
    assert (cs0 < 0).any() and (cs0 > 0.9).any()
    assert c["P"] >= 3 and len({a.tobytes() for a in c["x"][:3]}) == 3  # at least 3 planes of different content
    assert c["x"].dtype == np.float32 and c["x"].shape == (c["P"], c["H"], c["W"]) and np.isfinite(c["ref"]).all()
    d = [p for p, f in enumerate(c["fam"]) if f == "d"]
    if d:
        lum = mc.luminance64(c["x"][d], c["y"][d])
        print(cid, "family d: mean luminance factor at scale 0:", lum[:4])
        assert (np.abs(lum - 1.0) > 1e-2).all() and c["x"][d].max() <= 0.004 and c["y"][d].max() <= 0.004 and c["x"][d].min() >= 0
    for p, f in enumerate(c["fam"]):
        if f == "c" or f == "n":
            assert (c["ref"][p, :4, 1] < 0).all(), (cid, p)  # every CS term the wrapper uses is negative: the scalar is blind
        if f == "g":
            assert np.abs(c["ref"][p] - 1.0).max() < 1e-12
    if cid in ("clamp1", "clamp0"):
        assert c["x"].min() < -0.4 and c["x"].max() > 1.4 and c["y"].min() < -0.4 and c["y"].max() > 1.4
    if cid == "clamp0":  # the clamp matters: the same planes, clamped, have other statistics
        assert np.abs(c["ref"] - mc.build("clamp1")["ref"]).max() > 1e-2
        assert np.array_equal(c["x"], mc.build("clamp1")["x"])


def test_family_e_cancels_in_fp32():
    """the flat bright plane is where fp32 costs most: E[x^2] - mu^2 ~ 4e-6 from terms ~ 0.94, against c2 = 9e-4"""
    c = mc.build("min_odd")
    p = c["fam"].index("e")
    err = np.abs(c["emu"].astype(np.float64) - c["ref"])
    print("family e:", err[p].max(), "others:", np.delete(err, p, axis=0).max())
    assert err[p].max() > 8 * mc.EPS24 and err[p].max() == c["E32"].max()


def test_chains_of_map_sizes():
    assert mc.sides(161) == [161, 81, 41, 21, 11] and mc.sides(203) == [203, 102, 51, 26, 13] and mc.sides(162) == [162, 81, 41, 21, 11]
    assert mc.sides(170) == [170, 85, 43, 22, 11] and mc.sides(400) == [400, 200, 100, 50, 25]
    shapes = {c[0]: c[1:4] for c in mc.CASES}
    assert shapes["min_odd"] == (3, 161, 161) and shapes["exact_tiles"] == (3, 170, 202) and shapes["one_over"] == (3, 171, 203)
    assert shapes["wide"][1:] == (163, 400) and shapes["tall"][1:] == (400, 162) and shapes["planes65"] == (65, 161, 170)
    assert (170 - 10) % mc.TH == 0 and (202 - 10) % mc.TW == 0              # exactly 10 x 3 tiles
    assert (171 - 10) % mc.TH == 1 and (203 - 10) % mc.TW == 1              # a last tile of one row / of one column
    assert [s - 10 for s in mc.sides(161)][-1] == 1                          # scale 4's map is 1 x 1
    assert all(s % 2 for s in mc.sides(161)[:4])                             # every pool pads
    # the restatement's pool walks the same chain
    import torch

    x = torch.zeros(1, 171, 203)
    for h, w in zip(mc.sides(171)[1:], mc.sides(203)[1:]):
        x = mc._pool(x, None)
        assert tuple(x.shape[-2:]) == (h, w)


def test_restated_pool_and_filter_are_the_definition_s():
    """the restatement's own pieces against oracle/msssim_ref.py's, on an odd-sided plane (fp32 against fp64)"""
    import torch

    rng = np.random.RandomState(5)
    a = rng.uniform(0, 1, (2, 23, 31)).astype(np.float32)
    assert np.abs(mc._pool(torch.tensor(a), None).numpy() - msssim_ref._pool2(a.astype(np.float64))).max() < 4 * mc.EPS24
    taps = mc.taps32()
    got = mc._filter(mc._filter(torch.tensor(a), taps, 2), taps, 1).numpy()
    assert np.abs(got - msssim_ref._blur(a.astype(np.float64), msssim_ref._window())).max() < 16 * mc.EPS24
    assert np.abs(taps.astype(np.float64) - msssim_ref._window()).max() < mc.EPS24


@pytest.mark.parametrize("cid", ["one_over", "min_odd"])
def test_stats64_folds_into_the_reference_scalar(cid):
    c = mc.build(cid)
    x, y = np.clip(c["x"].astype(np.float64), 0, 1)[None], np.clip(c["y"].astype(np.float64), 0, 1)[None]  # one image of P channels
    st = c["ref"]
    terms = np.maximum(np.concatenate([st[:, :4, 1], st[:, 4:, 0]], axis=1), 0.0)
    val = np.prod(terms ** np.asarray(msssim_ref.WEIGHTS)[None], axis=1).mean()
    want = msssim_ref.ms_ssim(x, y, c["data_range"])
    print(cid, val, want)
    assert abs(val - want) < 1e-12
