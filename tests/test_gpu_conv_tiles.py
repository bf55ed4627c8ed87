"""Every tile form the conv dispatch instantiates, forced on its own, against the bits of the baseline tile.

DESIGN.md 3.1: tile shape, stage depth and staging mode never change a bit of a result -- the tile tables, the cost model,
rgbd_debug_tile_override and RGBD_CONV_FORCE all rest on it.  tests/test_gpu_conv.py and tests/test_gpu_convforms.py hold 13
hand-written tile strings to that contract; the library instantiates 179 single-chain and 165 blocked forms
(rgbd_debug_tile_list, from the lists of csrc/conv_tiles.h that the dispatch itself expands).  Here each of them runs, through
rgbd_conv_forms_nchw with rgbd_debug_force_tile, on the cases of tests/convtiles_cases.py -- shapes of a few hundred pixels
chosen so that every form meets partial cout tiles, tile grids that hang over the map, taps split over stages, a ring that wraps
(tests/test_convtiles_cases.py shows that from the host rules alone):

  * the launcher's return code equals convtiles_cases.fits(form, case) -- a refusal is an asserted -28, never a skipped form,
    and leaves every destination untouched; the hook's guard-band report (-1) is a failure like any other mismatch;
  * where the form fits, every destination equals the baseline's (forced tile 2,2,2,16,0, register-staged, in both families)
    bit for bit over its whole extent, the checkerboard half no launch may write included.  A failure names the form, the case
    and the first differing (n, c, y, x).

The anchor: the baseline itself lies within convtiles_cases.bound of an fp64 reference, element by element (the bound is derived
from the chain length and sum |w x|, not measured), and in the blocked family equals the chain of oracle/cpu_arith.c bit for bit.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import convforms_cases as cc
import convtiles_cases as ct
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

f32p = ctypes.POINTER(ctypes.c_float)
i32p = ctypes.POINTER(ctypes.c_int32)

FORMS = {b: ct.exported_forms(b) for b in (0, 1)}
TRIPLES = [(b,) + t for b in (0, 1) for t in ct.triples(FORMS[b])]

_INPUTS, _BASE = {}, {}


def _sets(c):
    if c["id"] not in _INPUTS:
        _INPUTS[c["id"]] = [cc.inputs(c, g) for g in range(c["groups"])]
    return _INPUTS[c["id"]]


@contextlib.contextmanager
def switches(c, form):
    """the debug switches a launch runs under; all of them back to their defaults afterwards"""
    from rgbd_amd._lib import check, lib

    L = lib()
    try:
        check(L.rgbd_debug_force_splitk(c["splitk"] if c["splitk"] > 1 else 0), "force_splitk")
        check(L.rgbd_debug_force_ckbd(c["ckbd"]), "force_ckbd")
        check(L.rgbd_debug_force_fuse(-1), "force_fuse")
        check(L.rgbd_debug_force_tile(ct.form_str(form).encode()), "force_tile")
        yield
    finally:
        L.rgbd_debug_force_tile(b"")
        L.rgbd_debug_force_fuse(-1)
        L.rgbd_debug_force_ckbd(0)
        L.rgbd_debug_force_splitk(0)


def launch(c, form, dev):
    """case c under the forced tile `form` -> (rc, [{"y": wide NCHW array} per operand set]); destinations pre-filled with FILL"""
    from rgbd_amd._lib import ConvFormsDesc, lib

    oh, ow = cc.out_hw(c)
    d = ConvFormsDesc()
    for k in ("n", "cin", "h", "w", "cout", "k", "stride", "pad", "transposed", "act", "x_off", "x_total", "y_off", "y_total"):
        setattr(d, k, c[k])
    d.groups = c["groups"]
    keep = []
    if c["blocked"]:
        blocks, d.bias_mode = ct.blocks_of(c)
        d.refmode = 1
        if blocks is not None:
            bl = np.ascontiguousarray(blocks, np.int32)
            keep.append(bl)
            d.blocks, d.nblocks = bl.ctypes.data_as(i32p), len(bl)
    outs = []
    for g, ins in enumerate(_sets(c)):
        o = d.set[g]
        for key, field in (("w", "weight"), ("b", "bias")):
            a = np.ascontiguousarray(ins[key], np.float32)
            keep.append(a)
            setattr(o, field, a.ctypes.data_as(f32p))
        x = torch.from_numpy(ins["x"]).to(dev)
        y = torch.full((c["n"], c["y_total"], oh, ow), float(cc.FILL), dtype=torch.float32, device=dev)
        keep += [x, y]
        o.x_dev, o.y_dev = x.data_ptr(), y.data_ptr()
        outs.append(y)
    with switches(c, form):
        rc = lib().rgbd_conv_forms_nchw(ctypes.byref(d), None)
    return rc, [{"y": y.cpu().numpy()} for y in outs]


def baseline(c, dev):
    if c["id"] not in _BASE:
        rc, outs = launch(c, ct.BASELINE, dev)
        assert rc == 0, f"{c['id']}: the baseline tile {ct.form_str(ct.BASELINE)} returned {rc}"
        _BASE[c["id"]] = outs
    return _BASE[c["id"]]


@pytest.mark.parametrize("blocked,wm,mt,nt", TRIPLES, ids=lambda v: str(v))
def test_tile_form_never_changes_a_bit(blocked, wm, mt, nt):
    dev = require_gpu()
    F = FORMS[blocked]
    mine = [f for f in F if f[:3] == (wm, mt, nt)]
    assert len(mine) in (5, 7)
    launched = refused = 0
    for c in ct.family(blocked):
        base = baseline(c, dev)
        for f in mine:
            want = ct.fits(f, c, F)
            rc, outs = launch(c, f, dev)
            what = f"tile {ct.form_str(f)} ({'blocked' if blocked else 'single-chain'}) on {c['id']}"
            assert rc != -1, f"{what}: a store landed in the guard band behind a destination"
            assert rc == want.rc, f"{what}: the launcher returned {rc}, the host rules say {want.rc} ({want})"
            if rc:
                for o in outs:  # a refusal launches nothing
                    assert (o["y"].view(np.uint32) == cc.FILL_BITS).all(), f"{what}: refused with {rc}, yet a destination was written"
                refused += 1
                continue
            try:
                ct.check(outs, base, c)
            except AssertionError as e:
                raise AssertionError(f"{what} [tile {want.TM} couts x {want.TH} x {want.TW} pixels, {want.tps} taps per stage, "
                                     f"{want.stages} stages]: {e}") from None
            launched += 1
    print(f"{'blk' if blocked else 'main'} {wm},{mt},{nt}: {launched} (form, case) pairs launched and equal, {refused} refused as the rules say")
    assert launched >= 3 * (len(mine) - sum(ct.never_fits(f) for f in mine))


@pytest.mark.parametrize("c", ct.CASES, ids=cc.case_id)
def test_baseline_against_fp64(c):
    dev = require_gpu()
    outs = baseline(c, dev)
    mask = ct.computed_mask(c)
    worst = 0.0
    for g, (ins, out) in enumerate(zip(_sets(c), outs)):
        y = out["y"]
        b = y.view(np.uint32)
        assert (b[..., ~mask] == cc.FILL_BITS).all(), f"{c['id']} set {g}: the checkerboard half that is not computed was written"
        assert (b[..., mask] != cc.FILL_BITS).all(), f"{c['id']} set {g}: computed positions were left unwritten"
        ref, bnd = ct.bound(c, ins)
        err = np.abs(y.astype(np.float64) - ref)[..., mask]
        ratio = err / bnd[..., mask]
        worst = max(worst, float(ratio.max()))
        if not (ratio <= 1.0).all():
            i = tuple(int(v) for v in np.argwhere(~(np.abs(y.astype(np.float64) - ref) <= bnd) & mask)[0])
            raise AssertionError(f"{c['id']} set {g}: {int((ratio > 1).sum())} elements outside the bound; first at (n, c, y, x) = {i}: "
                                 f"got {y[i]!r}, fp64 {ref[i]!r}, bound {bnd[i]:.3e}")
        if c["blocked"]:
            want = ct.blocked_reference(c, ins)
            same = y.view(np.uint32)[..., mask] == want.view(np.uint32)[..., mask]
            if not same.all():
                i = tuple(int(v) for v in np.argwhere((y.view(np.uint32) != want.view(np.uint32)) & mask)[0])
                raise AssertionError(f"{c['id']} set {g}: {int((~same).sum())} elements differ from the oracle/cpu_arith chain; first at "
                                     f"(n, c, y, x) = {i}: got {y[i]!r}, want {want[i]!r}")
    print(f"{c['id']}: worst |err| / bound of the baseline tile = {worst:.4f}")
    if c["groups"] == 2:
        assert not np.array_equal(outs[0]["y"], outs[1]["y"])
