"""CPU-side checks of tests/convforms_cases.py (no GPU): the derived fp64 bounds are ones a correct fp32 implementation meets,
the blocked reference of a fused chain is the chain of three stand-alone oracle convolutions, and the case list keeps the
coverage tests/test_gpu_convforms.py relies on -- so that a geometry or channel case cannot be dropped quietly."""
import numpy as np
import pytest
import torch

import convforms_cases as cc
from oracle import cpu_arith as ca

CASES = cc.CASES
GELU = [c for c in CASES if c["act"] == cc.ACT_GELU]


@pytest.mark.parametrize("c", CASES, ids=cc.case_id)
def test_torch_fp32_meets_the_derived_bound(c):
    for g in range(c["groups"]):
        d = cc.inputs(c, g)
        ref, got = cc.reference64(c, d), cc.torch32(c, d)
        for key in ("y", "u") if c["cout3"] else ("y",):
            err = float(np.abs(got[key].astype(np.float64) - ref[key]).max())
            bound = ref["bound_" + key]
            print(f"{c['id']} set {g} {key}: err {err:.3e} bound {bound:.3e}")
            assert 0.0 < bound < 1e-2 * (np.abs(ref[key]).max() + 1e-3)  # (a bound, not a licence)
            assert err <= bound, (key, err, bound)


@pytest.mark.parametrize("c", [c for c in CASES if c["blocked"] and c["cout2"]], ids=cc.case_id)
def test_blocked_reference_is_the_chain_of_stand_alone_convs(c):
    d = cc.inputs(c)
    got = cc.blocked_reference(c, d)
    x = cc.x_slice(c, d)
    if c["k"] > 1:
        t = ca.conv2d(x, d["w"], d["b"], 1, c["pad"], blocks=ca.direct_blocks(c["cin"]), bias_mode=1)
    else:
        t = ca.conv2d(x, d["w"], d["b"], 1, 0, blocks=[c["cin"]], bias_mode=2)
    if c["act_mid"]:
        t = np.maximum(t, np.float32(0))
    y = ca.conv2d(t, d["w2"], d["b2"], 1, 0, blocks=[c["cout"]], bias_mode=2)
    if c["res1"]:
        y = y + d["res1"]
    assert y.dtype == np.float32
    y = cc._act_np(y, c["act"])
    assert np.array_equal(got["y"], y)
    if c["cout3"]:
        u = np.maximum(ca.conv2d(y, d["w3"], d["b3"], 1, 0, blocks=[c["cout2"]], bias_mode=2), np.float32(0))
        assert np.array_equal(got["u"], u)
    # ... and it is not the single chain in disguise: within the fp64 bound of it, but not the same bits everywhere
    ref = cc.reference64(c, d)
    assert np.abs(got["y"].astype(np.float64) - ref["y"]).max() <= ref["bound_y"]


def test_inputs_are_deterministic_and_the_operand_sets_differ():
    for c in CASES:
        a, b = cc.inputs(c, 0), cc.inputs(c, 0)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
        if c["groups"] == 2:
            o = cc.inputs(c, 1)
            assert o.keys() == a.keys()
            for k in a:  # the two operand sets differ in every tensor
                assert a[k].shape == o[k].shape and not np.array_equal(a[k], o[k]), (c["id"], k)
        if c["mul"]:
            assert a["mul"].min() > 0 and a["mul"].max() < 1
        if c["x_total"] > c["cin"]:
            lo = cc.inputs(c, 0, cc.X_FILL[1])
            assert np.array_equal(cc.x_slice(c, a), cc.x_slice(c, lo)) and not np.array_equal(a["x"], lo["x"])


def _is_fused(c):
    return c["cout2"] > 0


def test_coverage_output_grids():
    grids = {cc.out_hw(c) for c in CASES}
    assert (1, 1) in grids and (3, 5) in grids
    assert any(h == 1 and w > 1 for h, w in grids) and any(w == 1 and h > 1 for h, w in grids)
    for width in (15, 16, 17, 33, 65, 129):
        assert any(w == width for _, w in grids), width
    assert {c["n"] for c in CASES} >= {1, 2, 3}
    # the fused forms run under every pixel-tile class (64 / 128 / 256 pixels): a partial last tile row for each of them, with
    # and without the lead layer (which has no 256-pixel form: the launcher gives it 128)
    for lead in (False, True):
        for tp in (64, 128, 256):
            rows = []
            for c in CASES:
                if _is_fused(c) and bool(c["cout3"]) == lead:
                    gh, gw = cc.out_hw(c)
                    t = 128 if lead and tp == 256 else tp
                    rows.append(gh % (t // cc.pick_tw(gw, gh, t)) != 0)
            assert any(rows) and not all(rows), (lead, tp)  # (and some whose tiles end with the map)
    # maps narrower than a tile and maps that need several tiles per row
    assert any(cc.out_hw(c)[1] < 4 for c in CASES if _is_fused(c)) and any(cc.out_hw(c)[1] > 64 for c in CASES if _is_fused(c))


def test_coverage_fused_shapes():
    fused = [c for c in CASES if _is_fused(c)]
    assert {c["k"] for c in fused} == {1, 3}
    assert {c["cin"] for c in fused} >= {16, 48, 96, 213}
    assert {c["cout"] for c in fused} == {81, 90, 96} and all(cc.round_up(c["cout"], 16) == 96 for c in fused)
    for c2 in (84, 96, 177, 192, 288):
        assert {c["res1"] for c in fused if c["cout2"] == c2} == {False, True}, c2
    assert {c["act"] for c in fused} == {0, 1, 2} and {c["act_mid"] for c in fused} == {0, 1}
    assert all(c["stride"] == 1 and not c["transposed"] and not c["mul"] and not c["res2"] and not c["y2"] and c["splitk"] == 1 and
               not c["ckbd"] for c in fused)
    lead = [c for c in CASES if c["cout3"]]
    assert all(c["family"] == "lead" for c in lead) and all(c["cout2"] for c in lead)
    assert {cc.round_up(c["cout2"], 16) for c in lead} == {96, 192, 288}
    assert {c["cout3"] for c in lead} == {90, 96}
    assert any(c["y3_total"] == c["cout3"] for c in lead) and any(c["y3_total"] > c["cout3"] and c["y3_off"] > 0 for c in lead)
    # single-chain and blocked, with and without the lead layer
    for lead_on in (False, True):
        assert {c["blocked"] for c in CASES if _is_fused(c) and bool(c["cout3"]) == lead_on} == {False, True}
    for c in CASES:
        if c["blocked"]:  # what the hook accepts in the permuted layout
            assert not c["transposed"] and c["act"] != cc.ACT_SIGMOID and c["splitk"] == 1
            assert c["y_off"] % 16 == 0 and c["x_off"] % 16 == 0 and cc.cout_store(c) == cc.round_up(cc.y_channels(c), 16)


def test_coverage_plain_operands():
    plain = [c for c in CASES if c["family"] == "plain" and not c["blocked"] and c["groups"] == 1 and not c["ckbd"]]
    for r1, m, r2 in ((False, False, False), (True, False, False), (False, True, False), (False, True, True)):  # what the engine issues
        sel = [c for c in plain if (c["res1"], c["mul"], c["res2"]) == (r1, m, r2)]
        assert any(c["y2"] for c in sel), (r1, m, r2)
        assert any(c["splitk"] == 1 and not c["y2"] for c in sel) and any(c["splitk"] == 4 and c["cin"] >= 64 for c in sel), (r1, m, r2)
    assert not any(c["y2"] and c["splitk"] > 1 for c in CASES)  # (refused by the launcher: test_refusals)
    assert {c["ckbd"] for c in CASES} == {0, 1, 2} and all(c["stride"] == 1 and not c["transposed"] for c in CASES if c["ckbd"])
    assert any(c["stride"] == 2 and not c["transposed"] for c in CASES) and any(c["stride"] == 2 and c["transposed"] for c in CASES)
    assert {c["k"] for c in CASES} >= {1, 3, 5}


def test_coverage_slices_and_placement():
    def narrow(c):  # an output slice narrower than its 16-padded width inside a wider buffer
        return c["y_total"] > cc.y_channels(c) and cc.cout_store(c) < cc.round_up(cc.y_channels(c), 16)

    for fused in (False, True):
        sel = [c for c in CASES if _is_fused(c) == fused and narrow(c)]
        assert any(c["y_off"] == 0 for c in sel) and any(c["y_off"] > 0 for c in sel), fused
        assert any(c["x_off"] > 0 for c in CASES if _is_fused(c) == fused)
    assert any((cc.y_channels(c), c["y_total"]) == (24, 48) for c in CASES)  # STF_united's 24-of-48 slice
    for c in CASES:  # what the hook accepts (include/rgbd_amd.h): nothing stored runs over a neighbouring slice
        assert c["x_off"] % 16 == 0 and c["x_off"] + c["cin"] <= c["x_total"]
        dsts = [(c["y_off"], cc.y_channels(c), c["y_total"], cc.cout_store(c))]
        if c["y2"]:
            dsts.append((c["y2_off"], cc.y_channels(c), c["y2_total"], cc.cout_store(c)))
        if c["cout3"]:
            dsts.append((c["y3_off"], c["cout3"], c["y3_total"], 96))
        for off, ch, total, store in dsts:
            assert off % 4 == 0 and off + ch <= total and (store == ch or off + ch == total) and off + store <= cc.round_up(total, 16)
        if c["x_total"] > c["cin"]:
            assert c["x_off"] + cc.round_up(c["cin"], 16) <= cc.round_up(c["x_total"], 16)


def test_coverage_grouped():
    for fam in cc.FAMILIES:
        assert any(c["groups"] == 2 for c in CASES if c["family"] == fam), fam
    for groups in (1, 2):  # the reducer's GELU over one plane and over several, each as a single and as a grouped launch
        sel = [c for c in GELU if c["groups"] == groups]
        assert any(c["splitk"] == 1 for c in sel) and any(c["splitk"] > 1 for c in sel), groups
    grouped = [c for c in CASES if c["groups"] == 2]
    assert any(c["splitk"] > 1 and c["res1"] for c in grouped) and any(c["ckbd"] for c in grouped) and any(c["y2"] for c in grouped)
    assert any(c["cout2"] and not c["cout3"] and c["res1"] for c in grouped) and any(c["cout3"] for c in grouped)
    assert any(c["blocked"] and c["cout2"] for c in grouped)
    assert any(c["mul"] and c["res2"] for c in grouped)
    assert all(c["groups"] in (1, 2) for c in CASES)


# ================================================================================================ GELU (the reducer's activation)
def _pre(c, d, dtype):
    return cc.torch_compose(c, d, dtype)["v"].numpy()


def test_gelu_family_is_what_the_engine_launches():
    assert [c["id"] for c in GELU] == ["gelu-k1", "gelu-k1-grouped", "gelu-k1-split3", "gelu-k3", "gelu-k3-s2", "gelu-k3-grouped-split2",
                                       "gelu-1x1grid"]
    for c in GELU:  # the plain form outside the reference's CPU arithmetic, one destination: where launch_conv accepts GELU
        assert c["family"] == "gelu" and not (c["cout2"] or c["blocked"] or c["y2"] or c["ckbd"] or c["transposed"])
        oh, ow = cc.out_hw(c)
        assert c["n"] * oh * ow <= 400
    assert all(c["act"] == cc.ACT_GELU for c in CASES if c["family"] == "gelu")
    split3 = next(c for c in GELU if c["splitk"] == 3)  # chunks of 3, 3 and 1 groups of 16 channels
    n16 = cc.round_up(split3["cin"], 16) // 16
    assert n16 == 7 and -(-n16 // 3) == 3
    assert {c["k"] for c in GELU} == {1, 3} and {c["stride"] for c in GELU} == {1, 2} and (1, 1) in {cc.out_hw(c) for c in GELU}
    assert any(c["cout"] % 16 and c["cin"] % 16 for c in GELU)  # pad channels on both sides


def test_gelu_constants():
    """GELU_SLOPE is sup |gelu'| (at v = sqrt 2, where gelu'' = phi(v) (2 - v^2) changes sign), rounded up; E_ERF is four times a
    measured figure, not a chosen one."""
    s = 2.0 ** 0.5
    Phi = 0.5 * (1.0 + torch.erf(torch.tensor(1.0, dtype=torch.float64)).item())
    phi = np.exp(-1.0) / (2.0 * np.pi) ** 0.5
    sup = Phi + s * phi
    print(f"sup |gelu'| = {sup:.5f}; torch CPU fp32 erf on the cases' arguments: {cc.E_ERF_CPU:.3f} ulp; E_ERF = {cc.E_ERF:.3f}")
    assert sup <= cc.GELU_SLOPE <= sup + 2e-4
    v = torch.linspace(-9, 9, 180001, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(torch.nn.functional.gelu(v).sum(), v)
    assert g.abs().max().item() <= sup + 1e-12
    # a faithfully rounded erf errs by less than 1 ulp, a correctly rounded one by up to 0.5: the device is granted 2 to 4
    assert cc.E_ERF == 4.0 * cc.E_ERF_CPU and 0.4 < cc.E_ERF_CPU <= 1.0


def test_gelu_device_formula_meets_the_activation_bound_with_one_ulp():
    """The reference alone passes: 0.5f * v * (1.0f + erff(v * c)) in torch-CPU fp32 stays within B_act with E_ERF = 1 (torch's
    erf is within 1 ulp), on 2.4 million values of -9 .. 9 and on every case's own pre-activations."""
    vs = [torch.linspace(-9, 9, 2400001, dtype=torch.float32).numpy()]
    vs += [_pre(c, cc.inputs(c, g), torch.float32).ravel() for c in GELU for g in range(c["groups"])]
    v = np.concatenate(vs)
    assert float(cc.erf32_ulps(v * cc.SQRT1_2).max()) <= 1.0
    ratio = np.abs(cc.gelu_device_formula(v).astype(np.float64) - cc.gelu64(v)) / cc.act_bound(v, 1.0)
    print(f"device formula in torch fp32: worst err / B_act(E_ERF = 1) = {ratio.max():.3f} over {v.size} values")
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("c", GELU, ids=cc.case_id)
def test_gelu_case_is_not_hollow(c):
    """Each operand set reaches the region where 1 + erf cancels, the linear region, and the neighbourhood of 0."""
    for g in range(c["groups"]):
        v = _pre(c, cc.inputs(c, g), torch.float32)
        lo, hi, mid = float((v < -3).mean()), float((v > 3).mean()), int((np.abs(v) < 0.1).sum())
        print(f"{c['id']} set {g}: v in [{v.min():.2f}, {v.max():.2f}], {100 * lo:.1f} % below -3, {100 * hi:.1f} % above 3, {mid} within 0.1 of 0")
        assert lo >= 0.01 and hi >= 0.01 and mid > 0


def _split_chunks(c):
    n16 = cc.round_up(c["cin"], 16) // 16
    per = -(-n16 // c["splitk"])  # (csrc/conv_mfma_body.h: per = ceil(n16 / splitk))
    return [(16 * s * per, min(c["cin"], 16 * min(n16, (s + 1) * per))) for s in range(c["splitk"])]


@pytest.mark.parametrize("c", GELU, ids=cc.case_id)
def test_gelu_mistakes_land_far_from_the_bounds(c):
    """Another GELU than the erf form, against the element-wise bound (b); GELU at the wrong place of the epilogue, against the
    operator bound (a): each at least 100 times its bound, on every case it applies to."""
    F = torch.nn.functional
    for g in range(c["groups"]):
        d = cc.inputs(c, g)
        ref = cc.reference64(c, d)
        v32 = _pre(c, d, torch.float32)
        want, bound = cc.gelu64(v32), cc.act_bound(v32)
        t = torch.from_numpy(v32).double()
        for name, wrong in (("tanh form", F.gelu(t, approximate="tanh")), ("v * sigmoid(1.702 v)", t * torch.sigmoid(1.702 * t))):
            ratio = float((np.abs(wrong.numpy() - want) / bound).max())
            print(f"{c['id']} set {g}: {name}: {ratio:.3g} x B_act")
            assert ratio >= 100.0, name
        T = lambda a: torch.from_numpy(a).double()
        x, w, b = T(cc.x_slice(c, d)), T(d["w"]), T(d["b"])
        wrongs = [("GELU before the bias", F.gelu(cc._conv_t(c, x, w, None)) + b.view(1, -1, 1, 1))]
        if c["splitk"] > 1:
            chunks = _split_chunks(c)
            assert len(chunks) == c["splitk"] and chunks[-1][1] == c["cin"] and all(lo < hi for lo, hi in chunks)
            parts = [cc._conv_t(c, x[:, lo:hi], w[:, lo:hi], b if i == 0 else None) for i, (lo, hi) in enumerate(chunks)]
            assert float((sum(parts) - T(ref["y"] * 0 + _pre(c, d, torch.float64))).abs().max()) < 1e-12  # (the chunks are the conv)
            wrongs.append(("GELU of each partial, then the sum", sum(F.gelu(p) for p in parts)))
        for name, wrong in wrongs:
            ratio = float(np.abs(wrong.numpy() - ref["y"]).max()) / ref["bound_y"]
            print(f"{c['id']} set {g}: {name}: {ratio:.3g} x bound")
            assert ratio >= 100.0, name
