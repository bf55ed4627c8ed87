"""Are the cases of tests/gdn_cases.py worth running on the GPU?  (CPU only.)

  (a) the honest fp32 restatement of the launch stays within the derived bound at every case (the cap asserted on
      |err| / bound is 1.0: the bound itself, not a measured figure), at the automatic tile and, on the small cases, at every
      tile the launcher can be forced to;
  (b) every deliberately wrong restatement (gdn_cases.MUTANTS) is rejected by the same acceptance function on at least one
      named case and tile;
  (c) rgbd_gdn_pack -- what the engine's finalize uploads -- equals the fragment formula, with beta's pad 1 and gamma's pad 0;
  and gdn_tile_for's rule, restated, chooses the tiles the automatic-tile cases are there for.
"""
import ctypes

import numpy as np
import pytest

import gdn_cases as gc

F32P = ctypes.POINTER(ctypes.c_float)


@pytest.mark.parametrize("cid", [c["id"] for c in gc.CASES])
def test_restatement_is_within_the_bound(cid):
    k = gc.build(cid)
    tiles = (None,) if k["group"] == "auto" else (None,) + gc.TILES
    worst = 0.0
    for tile in tiles:
        for inverse, with_res in gc.COMBOS:
            stats = {}
            fails = gc.accept(k, gc.emulate(k, inverse, with_res, tile=tile), inverse, with_res, stats)
            assert not fails, (tile, inverse, with_res, fails)
            worst = max(worst, stats["worst"])
    print(f"gdn restatement {cid}: worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0


# where each mistake can show at all: (case, tile) -> bool
_NT = lambda k: k["cs"] // 16
_WHERE = {
    "no_second_pass": lambda k, t: t != 16 and _NT(k) > gc.IT,
    "second_pass_first_gamma": lambda k, t: t != 16 and _NT(k) > gc.IT,
    "drop_last_part": lambda k, t: t == 16 and _NT(k) % 4 != 0,
    "gamma_transposed": lambda k, t: True,
    "sqrt_swapped": lambda k, t: True,
    "res_xcs": lambda k, t: k["xcs"] != k["rcs"],
    "stage_xcs": lambda k, t: k["xcs"] > k["cs"],
    "write_ycs": lambda k, t: k["ycs"] > k["cs"],
    "partial_tile_unwritten": lambda k, t: k["npix"] % t != 0,
    "past_npix": lambda k, t: k["npix"] % t != 0,
}


@pytest.mark.parametrize("mutant", gc.MUTANTS)
def test_mutant_is_rejected(mutant):
    """(the three large cases add nothing here: the small ones hold every mechanism)"""
    rejected, missed = [], []
    for cid in gc.SMALL:
        k = gc.build(cid)
        for tile in gc.TILES:
            hit = [combo for combo in gc.COMBOS if gc.accept(k, gc.emulate(k, *combo, mutant=mutant, tile=tile), *combo)]
            name = f"{cid}@{tile}"
            if hit:
                rejected.append(name)
            can_show = _WHERE[mutant](k, tile)
            assert can_show or not hit, f"{mutant} cannot differ from the honest restatement on {name}, yet it is rejected"
            if can_show and not hit:
                missed.append(name)
    print(f"gdn mutant {mutant}: rejected on {len(rejected)} case@tile pairs, all that can show it: {' '.join(rejected[:4])} ...")
    assert rejected, f"the wrong restatement '{mutant}' passes every case"
    assert not missed, f"'{mutant}' passes on {missed}, where it changes what is computed"


def test_tile_rule_on_the_automatic_tile_cases():
    assert sorted(gc.AUTO_TILE) == sorted(c["id"] for c in gc.CASES if c["group"] == "auto")
    for cid, tile in gc.AUTO_TILE.items():
        k = gc.BY_ID[cid]
        assert gc.tile_for(k["npix"], k["cs"]) == tile, cid
        assert k["npix"] % 64 and k["npix"] % tile  # the last workgroup is a partial one
    # the thresholds themselves: 512 workgroups of the tile, and the 32-pixel cap above 256 channels
    assert [gc.tile_for(n, 16) for n in (16383, 16384, 32767, 32768)] == [16, 32, 32, 64]
    assert [gc.tile_for(n, 256) for n in (32768, 1 << 20)] == [64, 64] and [gc.tile_for(n, 272) for n in (16384, 32768, 1 << 20)] == [32] * 3
    for cid in gc.SMALL:
        assert gc.tile_for(gc.BY_ID[cid]["npix"], gc.BY_ID[cid]["cs"]) == 16


def test_cases_hold_what_they_are_there_for():
    ids = [c["id"] for c in gc.CASES]
    assert len(set(ids)) == len(ids)
    nts = {c["cs"] // 16 for c in gc.CASES}
    assert {1, 5, 7, 13, 17, 20, 24, 32} <= nts and max(c["cs"] for c in gc.CASES) == gc.MAX_C
    for c in gc.CASES:
        assert all(c[s] >= c["cs"] and c[s] % 4 == 0 for s in ("xcs", "ycs", "rcs"))
        assert gc.dense_id(c) in gc.BY_ID or c["group"] in ("pix", "auto")
    k = gc.build("stride-c500-n37-s16.4.36")
    c, cs, npix = k["c"], k["cs"], k["npix"]
    assert (cs, k["xcs"], k["ycs"], k["rcs"]) == (512, 528, 516, 548)
    assert (k["xbuf"][:npix, c:cs] == 0).all() and np.isnan(k["xbuf"][:npix, cs:]).all() and not np.isnan(k["xbuf"][:, :cs]).any()
    assert (k["rbuf"][:npix, c:cs] == 0).all() and np.isnan(k["rbuf"][:npix, cs:]).all() and (k["rbuf"][npix:] == 0).all()
    x = k["x"]
    assert (x[npix // 2] == 0).all() and 0.05 < (x == 0).mean() < 0.2 and not np.signbit(x[x == 0]).any()
    nz = np.abs(x[x != 0])
    assert nz.min() < 2e-3 and nz.max() > 50
    assert (k["gamma"] < 2.0 ** -18).mean() > 0.05 and len(set(k["bp"][:c].tolist())) == c
    d = gc.build(gc.dense_id(k))
    assert np.array_equal(d["x"], x) and np.array_equal(d["res"], k["res"]) and np.array_equal(d["gamma"], k["gamma"])
    # the acceptance function needs the whole buffer untouched outside [0, cs): an unwritten destination fails, too
    assert gc.accept(k, gc.new_y(k), 0, 1)


@pytest.mark.parametrize("c", [16, 20, 200, 500])
def test_pack_is_the_fragment_formula(c):
    from rgbd_amd import _lib

    L = _lib.lib()
    cs = gc.round_up(c, 16)
    beta, gamma = (t.numpy() for t in gc.params(c, c))
    bp, gp = np.empty(c, np.float32), np.empty((c, c), np.float32)
    assert L.rgbd_gdn_parametrize(beta.ctypes.data_as(F32P), c, 1, bp.ctypes.data_as(F32P)) == 0
    assert L.rgbd_gdn_parametrize(gamma.ctypes.data_as(F32P), c * c, 0, gp.ctypes.data_as(F32P)) == 0
    assert np.array_equal(bp, gc.parametrized(gc.params(c, c)[0], 1e-6).numpy())
    assert np.array_equal(gp, gc.parametrized(gc.params(c, c)[1], 0.0).numpy())
    bo, go = np.full(cs + 8, -7.0, np.float32), np.full(cs * cs + 8, -7.0, np.float32)
    assert L.rgbd_gdn_pack(beta.ctypes.data_as(F32P), gamma.ctypes.data_as(F32P), c, bo.ctypes.data_as(F32P), go.ctypes.data_as(F32P)) == 0
    assert (bo[cs:] == -7.0).all() and (go[cs * cs:] == -7.0).all(), "rgbd_gdn_pack wrote past cs / cs * cs floats"
    assert np.array_equal(bo[:c], bp) and (bo[c:cs] == 1.0).all()
    padded = np.zeros((cs, cs), np.float32)
    padded[:c, :c] = gp
    want = gc.fragments(padded)
    assert want.shape == (cs // 16, cs // 16, 64, 4)
    assert np.array_equal(go[:cs * cs].view(np.uint32), want.reshape(-1).view(np.uint32))
    # spelled out once: lane 37 = row 5 of the tile, k group 2
    assert want[cs // 16 - 1, 0, 37, 3] == padded[cs - 16 + 5, 11]
    if c < cs:
        assert (want[-1, :, c % 16:16, :] == 0).all() and (want[:, -1, 16 * (c % 16 // 4 + 1):, :] == 0).all()
    # refusals
    assert L.rgbd_gdn_pack(None, gamma.ctypes.data_as(F32P), c, bo.ctypes.data_as(F32P), go.ctypes.data_as(F32P)) == -22
    assert L.rgbd_gdn_pack(beta.ctypes.data_as(F32P), gamma.ctypes.data_as(F32P), 0, bo.ctypes.data_as(F32P), go.ctypes.data_as(F32P)) == -22
    assert L.rgbd_gdn_pack(beta.ctypes.data_as(F32P), gamma.ctypes.data_as(F32P), 513, bo.ctypes.data_as(F32P), go.ctypes.data_as(F32P)) == -22
    assert L.rgbd_gdn_pack(beta.ctypes.data_as(F32P), gamma.ctypes.data_as(F32P), c, None, go.ctypes.data_as(F32P)) == -22
