"""Is the tile sweep of tests/test_gpu_conv_tiles.py worth running?  Everything here follows from convtiles_cases.fits() -- the
Python restatement of the launchers' host rules, which the GPU sweep holds to the launchers' own return codes -- and from the
library's list of instantiated forms (rgbd_debug_tile_list, a host-only call).  No GPU.

The conditions are per form, so that the sweep cannot hide "this form was compared with nothing that could show a fault" behind
a refusal.  Where the rules decide something for every layer shape, the condition says so instead of pretending a case could
change it (convtiles_cases.never_fits / single_tap_only / feasible; each is computed from fits() on probe layers, none is a list).
"""
import numpy as np
import pytest

import convforms_cases as cc
import convtiles_cases as ct

FAMILIES = (0, 1)


@pytest.fixture(scope="module")
def forms():
    return {b: ct.exported_forms(b) for b in FAMILIES}


def _good(f, b, F):
    """[(case, Fit)] of the family's cases form f fits"""
    r = [(c, ct.fits(f, c, F)) for c in ct.family(b)]
    return [(c, x) for c, x in r if x.rc == 0]


def test_export_is_what_the_dispatch_macros_instantiate(forms):
    """27 / 25 tiles; every tile with kc 64, kc 16 register-staged and three direct-to-LDS caps; the tiles with whole waves of patch
    slots also as rings of four and three: 179 / 165 forms.  The baseline tile is in both families."""
    for b, ntiles, nring in ((0, 27, 22), (1, 25, 20)):
        F = forms[b]
        tr = ct.triples(F)
        assert len(tr) == ntiles and len(F) == 5 * ntiles + 2 * nring
        for (wm, mt, nt), fs in tr.items():
            modes = [(kc, dm) for _, _, _, kc, dm in fs]
            ring = (16 * nt * (2 if wm == 2 else 4)) % 64 == 0
            assert modes == [(64, 0), (16, 0), (16, 1), (16, 2), (16, 3)] + ([(16, 4), (16, 5)] if ring else []), (wm, mt, nt, modes)
            assert not b or ct.conv_blk_tile_ok(wm, mt, nt)
        assert ct.BASELINE in F
    assert set(forms[1]) < set(forms[0])
    # a short buffer gets a terminated prefix and the same size back
    import ctypes

    from rgbd_amd._lib import lib

    buf = ctypes.create_string_buffer(b"\xff" * 16, 16)
    need = lib().rgbd_debug_tile_list(0, buf, 16)
    assert need == len("\n".join(ct.form_str(f) for f in forms[0])) + 2 and len(buf.value) == 15
    assert lib().rgbd_debug_tile_list(0, None, 0) == need


def test_baseline_fits_every_case(forms):
    for c in ct.CASES:
        assert ct.fits(ct.BASELINE, c, forms[c["tile_family"]]).rc == 0, c["id"]


def test_forms_no_launch_can_reach(forms):
    """The instantiations the rules refuse for every layer, by the arithmetic of the module docstring of convtiles_cases: kc 64
    with TM = 160 or 256-pixel tiles, and the 38 KiB cap on 256-pixel tiles of TM > 48."""
    for b in FAMILIES:
        dead = {f for f in forms[b] if ct.never_fits(f)}
        want = {f for f in forms[b]
                if (f[3] == 64 and (16 * f[1] * f[0] == 160 or f[2] * (2 if f[0] == 2 else 4) == 16))
                or (f[3:] == (16, 3) and f[2] * (2 if f[0] == 2 else 4) == 16 and 16 * f[1] * f[0] > 48)}
        assert dead == want, sorted(dead ^ want)
        print(f"family {b}: {len(dead)} of {len(forms[b])} forms can never be launched: {' '.join(ct.form_str(f) for f in sorted(dead))}")
        for f in dead:
            assert all(ct.fits(f, c, forms[b]).rc == ct.ENOSPC for c in ct.family(b)), f


def test_every_form_fits_at_least_three_cases(forms):
    for b in FAMILIES:
        for f in forms[b]:
            if not ct.never_fits(f):
                assert len(_good(f, b, forms[b])) >= 3, (f, [c["id"] for c, _ in _good(f, b, forms[b])])


def test_every_non_ring_form_runs_single_and_multi_tap(forms):
    for b in FAMILIES:
        one = ct.BY_ID["blk-one-tap" if b else "one-tap"]
        for f in forms[b]:
            if f[4] in (4, 5) or ct.never_fits(f):
                continue
            good = _good(f, b, forms[b])
            assert any(c is one for c, _ in good), f
            if not ct.single_tap_only(f):
                assert any(ct.geometry(c)["max_taps"] > 1 for c, _ in good), f


def test_every_form_meets_partial_tiles(forms):
    """a cout tile that hangs over cout_pad (impossible for TM = 16: cout_pad is a multiple of 16), and a tile grid that hangs over
    the map in both directions"""
    for b in FAMILIES:
        for f in forms[b]:
            if ct.never_fits(f):
                continue
            good = _good(f, b, forms[b])
            if 16 * f[1] * f[0] > 16:
                assert any(ct.geometry(c)["cout_pad"] % x.TM for c, x in good), f
            assert any(ct.geometry(c)["GW"] % (x.TW * (2 if c["ckbd"] else 1)) and ct.geometry(c)["GH"] % x.TH for c, x in good), f


def test_lds_caps_change_the_walk(forms):
    """Staging modes 2 and 3 differ from mode 1 only in the LDS cap, i.e. in how many taps go into a stage: each fits a case where
    that number differs from mode 1's -- unless the rules leave it single-tap layers only (one tap per stage under any cap)."""
    for b in FAMILIES:
        for t in ct.triples(forms[b]):
            for dm in (2, 3):
                f, m1 = t + (16, dm), t + (16, 1)
                if ct.never_fits(f) or ct.single_tap_only(f):
                    continue
                assert any(x.tps != ct.fits(m1, c, forms[b]).tps and ct.fits(m1, c, forms[b]).rc == 0 for c, x in _good(f, b, forms[b])), f


def test_ring_forms_wrap(forms):
    for b in FAMILIES:
        for f in forms[b]:
            if f[4] in (4, 5):
                need = 6 if f[4] == 4 else 5
                assert any(x.stages >= need and x.tps == 1 for _, x in _good(f, b, forms[b])), f


def test_every_case_fits_half_of_what_its_kind_of_layer_allows(forms):
    """A case that most forms refuse says little.  Counted against the forms that can run the case's KIND of layer on some map
    (convtiles_cases.feasible): ring forms cannot run a multi-tap layer, the strided 5x5 patch of 19 x 19 pixels and more leaves
    no room for most direct-to-LDS forms -- on any map, so no choice of case could let them in."""
    for b in FAMILIES:
        F = forms[b]
        for c in ct.family(b):
            able = [f for f in F if ct.feasible(f, c, F)]
            fit = [f for f in able if ct.fits(f, c, F).rc == 0]
            print(f"{c['id']}: fits {len(fit)} of the {len(able)} forms that can run this kind of layer ({len(F)} in the family)")
            assert 2 * len(fit) >= len(able), c["id"]
            assert 4 * len(able) >= len(F), c["id"]  # (and the kind itself is not a corner: a quarter of the family can run it)


def test_no_pair_is_an_argument_error(forms):
    n = {0: 0, ct.ENOSPC: 0}
    for b in FAMILIES:
        for f in forms[b]:
            for c in ct.family(b):
                rc = ct.fits(f, c, forms[b]).rc
                assert rc in (0, ct.ENOSPC), (f, c["id"], rc)
                n[rc] += 1
    print(f"(form, case) pairs: {n[0]} launched, {n[ct.ENOSPC]} refused")


def test_cases_stay_small_and_plain():
    for c in ct.CASES:
        oh, ow = cc.out_hw(c)
        assert max(c["h"] * c["w"], oh * ow) <= 400 and c["act"] in (cc.ACT_NONE, cc.ACT_RELU, cc.ACT_LEAKY)
        assert c["y_total"] == c["cout"] and c["x_total"] == c["cin"]
        if c["blocked"] and c["k"] == 1:
            assert len(c["blocks"]) > 1 and sum(c["blocks"]) == c["cin"] and all(v % 16 == 0 for v in c["blocks"][:-1])


# ---------------------------------------------------------------------------------------------- check() and bound()
def _outs(c, seed=0):
    oh, ow = cc.out_hw(c)
    r = np.random.RandomState(seed)
    outs = []
    for _ in range(c["groups"]):
        y = np.full((c["n"], c["y_total"], oh, ow), cc.FILL, np.float32)
        y[..., ct.computed_mask(c)] = r.standard_normal((c["n"], c["y_total"], int(ct.computed_mask(c).sum()))).astype(np.float32)
        outs.append({"y": y})
    return outs


@pytest.mark.parametrize("cid", ["one-tap", "ckbd1", "grouped", "blk-k3"])
def test_check_rejects_one_ulp_and_one_fill_element(cid):
    c = ct.BY_ID[cid]
    base = _outs(c)
    ct.check(_outs(c), base, c)  # equal tensors pass
    # one element of the last cout tile, last image, last pixel, off by one ulp
    got = _outs(c)
    y = got[-1]["y"]
    pos = tuple(int(v) for v in np.argwhere(ct.computed_mask(c))[-1])
    idx = (c["n"] - 1, c["cout"] - 1) + pos
    y[idx] = np.nextafter(y[idx], np.float32(np.inf))
    with pytest.raises(AssertionError, match=r"first at \(n, c, y, x\) = \(%d, %d, %d, %d\)" % idx):
        ct.check(got, base, c)
    if c["ckbd"]:  # one element the launch must leave alone, overwritten
        got = _outs(c)
        hole = tuple(int(v) for v in np.argwhere(~ct.computed_mask(c))[0])
        assert got[0]["y"][(0, 0) + hole].view(np.uint32) == cc.FILL_BITS
        got[0]["y"][(0, 0) + hole] = 0.0
        with pytest.raises(AssertionError, match="differ from the baseline"):
            ct.check(got, base, c)
    # +0 and -0, equal as numbers, are different bits
    got, zero = _outs(c), _outs(c)
    got[0]["y"][(0, 0) + pos], zero[0]["y"][(0, 0) + pos] = np.float32(0.0), np.float32(-0.0)
    with pytest.raises(AssertionError):
        ct.check(got, zero, c)


def test_check_rejects_a_fill_element_overwritten_with_fill_left_elsewhere():
    """a launch that leaves a computed element at FILL (nothing stored) differs from the baseline as well"""
    c = ct.BY_ID["k3"]
    base, got = _outs(c), _outs(c)
    got[1 - 1]["y"][0, 3, 2, 5] = cc.FILL
    with pytest.raises(AssertionError, match=r"\(0, 3, 2, 5\)"):
        ct.check(got, base, c)


@pytest.mark.parametrize("cid", ["k2", "deconv", "splitk3", "blk-one-tap"])
def test_bound_holds_for_torch_fp32_and_is_not_slack(cid):
    """The bound is arithmetic, not a measurement: torch's own fp32 convolution (another summation order of the same terms) lies
    inside it, and it is tight enough to notice one dropped term -- a result without its largest |w x| product lies outside."""
    c = ct.BY_ID[cid]
    d = cc.inputs(c, 0)
    ref, bnd = ct.bound(c, d)
    y32 = cc.torch32(c, d)["y"].astype(np.float64)
    assert ref.shape == bnd.shape == y32.shape and (bnd > 0).all()
    assert (np.abs(y32 - ref) <= bnd).all()
    K = ct.geometry(c)["cin_pad"] * ct.geometry(c)["max_taps"]
    assert bnd.max() < (K + 3 + 1 + c["splitk"]) * ct.U * 40.0  # (sum |w x| of these inputs stays far below 40)
    # dropping input channel 0 of the reduction moves the pre-activation result by far more than the bound somewhere
    d2 = dict(d, x=d["x"].copy())
    d2["x"][:, 0] = 0
    moved = np.abs(ct.bound(dict(c, act=cc.ACT_NONE), d2)[0] - ct.bound(dict(c, act=cc.ACT_NONE), d)[0])
    assert (moved > 100 * bnd).any()
