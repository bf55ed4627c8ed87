"""The conv launchers (csrc/conv_mfma.hip: launch_conv / launch_conv_fused, conv_mfma_body.h, conv_mfma_blk.hip) in the forms
that only whole-model runs used to reach -- fused tail, its lead layer, gate / skip operands, second destination, channel-slice
placement, grouped launch -- each ALONE, through the C ABI rgbd_conv_forms_nchw (include/rgbd_amd.h), on the cases of
tests/convforms_cases.py.

  * single-chain results lie within the case's derived bound of a torch-CPU fp64 reference (convforms_cases.py: the per-layer rule
    of test_gpu_conv.py, composed along the chain); results in the reference's CPU arithmetic ("blocked") equal the chain of
    oracle/cpu_arith.c bit for bit;
  * a fused launch equals the same layers issued as stand-alone launches bit for bit, for every pixel-tile class;
  * a grouped launch equals its two single launches bit for bit;
  * every destination is pre-filled with a bit pattern: the channels next to an output slice and the checkerboard half that is
    not computed come back untouched (the hook also keeps a guard band behind every destination and returns -1 if a launch
    wrote into it); the channels next to an input slice do not reach a single output bit;
  * the forced tiles of test_gpu_conv.py::test_tile_choice_never_changes_a_bit, a second run and batch[1:2] alone change no bit;
  * what the launchers refuse comes back as -22 from the host check, with nothing launched.

Placements are restricted to the ones the engine makes (csrc/engine_conv.hip, engine_elic.hip, engine_swin.hip):
  Engine::conv_plan        "a channel slice narrower than its 16-padded width inside a wider buffer (STF_united: 24 of 48): stop at
                           the slice end; a buffer of its own gets its pad channels zeroed as usual"
                           a.cout_store = (pcy->cout % 16 && y.cs != round_up(pcy->cout, 16)) ? round_up(pcy->cout, 4) : pcy->cout_pad;
  Engine::bi_spf           Act rf = view(rd, 0, half), df = view(rd, half, half);  const Act rf2 = view(dr, half, half), df2 = view(dr, 0, half);
                           er.dup = &rf2;  (y and y2: halves of two concat buffers)
  Engine::entropy stage    entropy_params(..., view(ctx, 4 * C, wide - 4 * C), ...), Act l1 = view(ctxm, 0, sup + C): the input a slice
                           at a 16-multiple offset whose last 16-channel group may hold a neighbour's channels (zero weights)
  Engine::bottleneck2 / res_unit2   lead_out[m] = alloc(...): y3 is a buffer of its own in the engine; the slice cases of y3 only
                           move the pointer and the stride, as conv_plan would for any destination.
Spot checks this file is meant to catch (each makes at least one test here fail; none moves today's other tests reliably):
  `gy < a.GH` -> `gy <= a.GH` in the fused epilogue's ok[u]   every test that launches a fused case with a partial last tile row: the hook
                                                               returns -1 (guard band); 25 cases of test_against_reference and of
                                                               test_fused_equals_unfused among them
  `g1 ? a.g1.res1 : a.res1` -> `a.res1`                        test_grouped_equals_single and test_against_reference on plain-grouped-r1,
                                                               fused-grouped, fused-blk-grouped, lead-grouped, lead-blk-grouped (the
                                                               reducer's copy of that line: plain-grouped-r1-split4)
  dropping `cb < a.cout_store`                                 the untouched-neighbour check of test_against_reference: fused-slice-o0
                                                               (fused epilogue), slice-out-o0 / -o24, slice-grouped (plain epilogue),
                                                               slice-in-out-split4 (reducer)
(tried on scratch builds of the kernels with each line changed: 74, 10 and 21 tests of this file fail.)

GELU (family "gelu") is the split-K reducer's activation (splitk_reduce_kernel): launch_conv refuses it without a partial plane, so
the hook books one even with a split factor of 1, as Engine::conv_plan does.  The cases stand for the engine's GELU launches (Swin
mlp.fc1 single and grouped, h_a_stf1 at stride 1 and 2, h_s_stf1 grouped with split-K).  test_against_reference holds them to the
fp64 operator under 1.129 * (the conv rule on the pre-activation) + max B_act, and -- element by element -- to gelu64 of the
launch's own fp32 pre-activation (the same launch with act = 0) under B_act (convforms_cases.act_bound), which a tanh-form GELU
misses by a factor of 1000.  Spot checks on scratch builds, as above (the tests named fail; the counts are of `-k gelu`):
  the ACT_GELU branch of splitk_reduce_kernel removed          test_against_reference on all 7 gelu cases (the element-wise bound)
  `g1 ? a.g1.bias : a.bias` -> `a.bias` in the reducer         test_against_reference and test_grouped_equals_single on gelu-k1-grouped and
                                                               gelu-k3-grouped-split2 (4 tests)
  the hook's partial plane one pixel row short                 the hook returns -1 (the guard band behind the planes) in every launch that
                                                               has a partial plane: 11 tests of the gelu cases, and every split-K case.
                                                               (Tried with the guard band moved one row forward inside an allocation of
                                                               the full size, so that no store left it.)
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import convforms_cases as cc
import gridcap_cases as gc
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

f32p = ctypes.POINTER(ctypes.c_float)
i32p = ctypes.POINTER(ctypes.c_int32)
CASES = cc.CASES
BY_ID = {c["id"]: c for c in CASES}
FUSED = [c for c in CASES if c["cout2"]]
GROUPED = [c for c in CASES if c["groups"] == 2]
CLASSES = (1, 2, 4)  # rgbd_debug_force_fuse: 64 / 128 / 256-pixel tiles


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _report(got, want, what):
    """count of differing elements, the first index and the two values (as tests/test_gpu_pointwise.py reports)"""
    bad = np.argwhere(_bits(got) != _bits(np.asarray(want, np.float32)))
    i = tuple(bad[0])
    return f"{what}: {len(bad)} of {got.size} elements differ; first at {i}: got {got[i]!r}, want {np.float32(want[i])!r}"


def _report_tol(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    bad = np.argwhere(~(err <= bound))
    i = tuple(bad[0])
    return f"{what}: {len(bad)} of {got.size} elements off by more than {bound:.3e} (max {err.max():.3e}); first at {i}: got {got[i]!r}, want {want[i]!r}"


@contextlib.contextmanager
def switches(c, cls=-1, tile=b""):
    """the debug switches a case runs under; all of them back to their defaults afterwards"""
    from rgbd_amd._lib import check, lib

    L = lib()
    try:
        check(L.rgbd_debug_force_splitk(c["splitk"] if c["splitk"] > 1 else 0), "force_splitk")
        check(L.rgbd_debug_force_ckbd(c["ckbd"]), "force_ckbd")
        check(L.rgbd_debug_force_fuse(cls), "force_fuse")
        check(L.rgbd_debug_force_tile(tile), "force_tile")
        yield
    finally:
        L.rgbd_debug_force_fuse(-1)
        L.rgbd_debug_force_tile(b"")
        L.rgbd_debug_force_ckbd(0)
        L.rgbd_debug_force_splitk(0)


def launch(c, sets, dev, mutate=None):
    """One call of the hook for case c on the operand sets `sets` (1 or 2 dicts of convforms_cases.inputs()).
    -> (rc, [{"y", "y2", "y3"} wide NCHW numpy arrays per set])."""
    from rgbd_amd._lib import ConvFormsDesc, lib

    oh, ow = cc.out_hw(c)
    d = ConvFormsDesc()
    for k in ("n", "cin", "h", "w", "cout", "k", "stride", "pad", "transposed", "act", "cout2", "act_mid", "cout3", "x_off", "x_total",
              "y_off", "y_total", "y2_off", "y2_total", "y3_off", "y3_total"):
        setattr(d, k, c[k])
    d.groups = len(sets)
    keep = []
    if c["blocked"]:
        blocks, bias_mode = cc.ref_layer1(c)
        d.refmode, d.bias_mode = 1, bias_mode
        if blocks is not None:
            bl = np.ascontiguousarray(blocks, np.int32)
            keep.append(bl)
            d.blocks, d.nblocks = bl.ctypes.data_as(i32p), len(bl)
    outs = []
    for g, ins in enumerate(sets):
        o = d.set[g]

        def host(a):
            a = np.ascontiguousarray(a, np.float32)
            keep.append(a)
            return a.ctypes.data_as(f32p)

        def device(a):
            t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
            keep.append(t)
            return t

        o.x_dev = device(ins["x"]).data_ptr()
        o.weight, o.bias = host(ins["w"]), host(ins["b"])
        if c["cout2"]:
            o.w2, o.bias2 = host(ins["w2"]), host(ins["b2"])
        if c["cout3"]:
            o.w3, o.bias3 = host(ins["w3"]), host(ins["b3"])
        for key in ("res1", "mul", "res2"):
            if c[key]:
                setattr(o, key + "_dev", device(ins[key]).data_ptr())
        out = {"y": device(np.full((c["n"], c["y_total"], oh, ow), cc.FILL, np.float32))}
        o.y_dev = out["y"].data_ptr()
        if c["y2"]:
            out["y2"] = device(np.full((c["n"], c["y2_total"], oh, ow), cc.FILL, np.float32))
            o.y2_dev = out["y2"].data_ptr()
        if c["cout3"]:
            out["y3"] = device(np.full((c["n"], c["y3_total"], oh, ow), cc.FILL, np.float32))
            o.y3_dev = out["y3"].data_ptr()
        outs.append(out)
    if mutate:
        mutate(d)
    rc = lib().rgbd_conv_forms_nchw(ctypes.byref(d), None)
    return rc, [{k: v.cpu().numpy() for k, v in out.items()} for out in outs]


def run(c, sets, dev, cls=None, tile=b""):
    from rgbd_amd._lib import check

    with switches(c, (cls or 1) if c["cout2"] else -1, tile):
        rc, outs = launch(c, sets, dev)
    check(rc, f"rgbd_conv_forms_nchw({c['id']})")
    return outs


def _sets(c, x_fill=cc.X_FILL[0]):
    return [cc.inputs(c, g, x_fill) for g in range(c["groups"])]


def _computed(c):
    """[OH, OW] mask of the positions a launch computes (checkerboard output: one half)"""
    oh, ow = cc.out_hw(c)
    yy, xx = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    if not c["ckbd"]:
        return np.ones((oh, ow), bool)
    return (yy + xx) % 2 == (1 if c["ckbd"] == 1 else 0)  # 1: the anchors, (row + col) odd


def check_untouched(c, out, what):
    """everything a launch must not write still holds the fill pattern"""
    cy, mask = cc.y_channels(c), _computed(c)
    for key, off, ch in (("y", c["y_off"], cy), ("y2", c["y2_off"], cy), ("y3", c["y3_off"], c["cout3"])):
        if key not in out:
            continue
        b = _bits(out[key])
        outside = np.ones(b.shape[1], bool)
        outside[off:off + ch] = False
        assert (b[:, outside] == cc.FILL_BITS).all(), f"{what} {key}: channels outside [{off}, {off + ch}) were written: " \
            f"{int((b[:, outside] != cc.FILL_BITS).sum())} elements, first at {tuple(np.argwhere(b[:, outside] != cc.FILL_BITS)[0])}"
        if key != "y3":
            assert (b[:, off:off + ch][..., ~mask] == cc.FILL_BITS).all(), f"{what} {key}: the other checkerboard half was written"
            assert (b[:, off:off + ch][..., mask] != cc.FILL_BITS).all(), f"{what} {key}: computed positions were left unwritten"
        else:
            assert (b[:, off:off + ch] != cc.FILL_BITS).all(), f"{what} {key}: positions were left unwritten"


def _slices(c, out):
    cy = cc.y_channels(c)
    r = {"y": out["y"][:, c["y_off"]:c["y_off"] + cy]}
    if "y3" in out:
        r["u"] = out["y3"][:, c["y3_off"]:c["y3_off"] + c["cout3"]]
    return r


def _check_gelu(c, got, v, what):
    """The reducer's GELU against the launch's own pre-activation v (the same launch with act = 0: one plane + bias are the two
    operands of the kernel's own epilogue add; several planes go through the same reducer), element by element:
    |got - gelu64(v)| <= B_act(v) (convforms_cases.act_bound).  Where v is a zero, so is the result."""
    want, bound = cc.gelu64(v), cc.act_bound(v)
    err = np.abs(got.astype(np.float64) - want)
    ratio = err / bound
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"{what}: gelu vs own pre-activation: worst err / B_act = {ratio[i]:.3f} at v = {v[i]!r} (E_ERF = {cc.E_ERF:.3f}; v in "
          f"[{v.min():.2f}, {v.max():.2f}])")
    assert (err <= bound).all(), f"{what}: {int((~(err <= bound)).sum())} of {got.size} elements off by more than B_act; worst at {i}: " \
        f"v {v[i]!r}, got {got[i]!r}, want {want[i]!r}, B_act {bound[i]:.3e}"
    assert (got[v == 0] == 0).all(), f"{what}: a zero pre-activation did not give a zero"


@pytest.mark.parametrize("c", CASES, ids=cc.case_id)
def test_against_reference(c):
    dev = require_gpu()
    mask = _computed(c)
    for cls in (CLASSES if c["cout2"] else (None,)):
        sets = _sets(c)
        outs = run(c, sets, dev, cls)
        # (GELU: the same launch without the activation, under the same switches, is its fp32 pre-activation)
        pre = run(dict(c, act=cc.ACT_NONE), sets, dev, cls) if c["act"] == cc.ACT_GELU else None
        for g, (ins, out) in enumerate(zip(sets, outs)):
            what = f"{c['id']} set {g} class {cls}"
            check_untouched(c, out, what)
            got = _slices(c, out)
            if c["y2"]:
                y2 = out["y2"][:, c["y2_off"]:c["y2_off"] + cc.y_channels(c)]
                assert _same_bits(y2[..., mask], got["y"][..., mask]), _report(y2[..., mask], got["y"][..., mask], what + " y2 vs y")
            if c["act"] == cc.ACT_GELU:
                _check_gelu(c, got["y"], pre[g]["y"][:, c["y_off"]:c["y_off"] + cc.y_channels(c)], what)
            if c["blocked"]:
                want = cc.blocked_reference(c, ins)
                for key in got:
                    assert _same_bits(got[key], want[key]), _report(got[key], want[key], what + " " + key)
            else:
                ref = cc.reference64(c, ins)
                for key in got:
                    err = np.abs(got[key].astype(np.float64) - ref[key])[..., mask]
                    print(f"{what} {key}: max err {err.max():.3e}, bound {ref['bound_' + key]:.3e}")
                    assert (err <= ref["bound_" + key]).all(), _report_tol(got[key][..., mask], ref[key][..., mask], ref["bound_" + key],
                                                                            what + " " + key)


def test_splitk_reducer_past_the_grid_cap():
    """splitk_reduce_kernel past its 2048 x 256 grid cap (tests/gridcap_cases.py: 181 x 243 pixels of 12 float4s, two partial
    planes, res1 and ReLU in the reducer; two sweeps, the second one ragged) under test_against_reference's rule: every computed
    position written, within the case's derived bound of the fp64 reference; a second run gives the same bits."""
    dev = require_gpu()
    bc = gc.build_splitk(cc)
    c = bc["case"]
    outs = [run(c, [bc["ins"]], dev)[0] for _ in range(2)]
    check_untouched(c, outs[0], c["id"])
    assert bc["stages"]["splitk"]["accept"]({"y": outs[0]["y"]}) == []
    assert _same_bits(outs[0]["y"], outs[1]["y"])


def _chain_cases(c, ins):
    """the layers of fused case c as stand-alone plain cases: [(case, inputs builder from the previous output)]"""
    oh, ow = cc.out_hw(c)
    base = dict(stride=1, transposed=0, blocked=c["blocked"])
    c1 = cc._case(c["id"] + "/1", "plain", c["n"], c["cin"], c["h"], c["w"], c["cout"], c["k"], pad=c["pad"], act=c["act_mid"],
                  x_off=c["x_off"], x_total=c["x_total"], **base)
    c2 = cc._case(c["id"] + "/2", "plain", c["n"], c["cout"], oh, ow, c["cout2"], 1, act=c["act"], res1=c["res1"], **base)
    chain = [(c1, lambda prev: {"x": ins["x"], "w": ins["w"], "b": ins["b"]}),
             (c2, lambda prev: dict({"x": prev, "w": ins["w2"], "b": ins["b2"]}, **({"res1": ins["res1"]} if c["res1"] else {})))]
    if c["cout3"]:
        c3 = cc._case(c["id"] + "/3", "plain", c["n"], c["cout2"], oh, ow, c["cout3"], 1, act=cc.ACT_RELU, **base)
        chain.append((c3, lambda prev: {"x": prev, "w": ins["w3"], "b": ins["b3"]}))
    return chain


@pytest.mark.parametrize("c", FUSED, ids=cc.case_id)
def test_fused_equals_unfused(c):
    """y and u of the fused launch == the same layers as stand-alone launches through the same hook, bit for bit, under every
    pixel-tile class, with and without the lead layer, single-chain and blocked (the case list has all four)."""
    dev = require_gpu()
    for g in range(c["groups"]):
        ins = cc.inputs(c, g)
        prev, steps = None, []
        for ci, build in _chain_cases(c, ins):
            prev = run(ci, [build(prev)], dev)[0]["y"]
            steps.append(prev)
        want = {"y": steps[1]}
        if c["cout3"]:
            want["u"] = steps[2]
        single = dict(c, groups=1)
        for cls in CLASSES:
            got = _slices(c, run(single, [ins], dev, cls)[0])
            for key in want:
                assert _same_bits(got[key], want[key]), _report(got[key], want[key], f"{c['id']} set {g} class {cls} {key}: fused vs stand-alone")


@pytest.mark.parametrize("c", GROUPED, ids=cc.case_id)
def test_grouped_equals_single(c):
    """one grouped launch == its two single launches, bit for bit (plain, split-K, checkerboard, second destination, slices, fused,
    fused + lead, single-chain and blocked: test_convforms_cases.py::test_coverage_grouped)"""
    dev = require_gpu()
    sets = _sets(c)
    single = dict(c, groups=1)
    for cls in (CLASSES if c["cout2"] else (None,)):
        both = run(c, sets, dev, cls)
        for g in range(2):
            alone = run(single, [sets[g]], dev, cls)[0]
            for key in alone:
                assert _same_bits(both[g][key], alone[key]), _report(both[g][key], alone[key], f"{c['id']} class {cls} set {g} {key}: grouped vs single")
        # (the two sets really are two results)
        assert not _same_bits(both[0]["y"], both[1]["y"])


@pytest.mark.parametrize("c", [c for c in CASES if c["x_total"] > c["cin"]], ids=cc.case_id)
def test_sliced_input_ignores_its_neighbours(c):
    dev = require_gpu()
    a = run(c, _sets(c, cc.X_FILL[0]), dev)
    b = run(c, _sets(c, cc.X_FILL[1]), dev)
    for g in range(c["groups"]):
        for key in a[g]:
            assert _same_bits(a[g][key], b[g][key]), _report(a[g][key], b[g][key], f"{c['id']} set {g} {key}: neighbour fill {cc.X_FILL}")


TILE_CASES = ["plain-r1", "plain-mr2-split4", "plain-none-y2", "plain-ckbd1", "plain-grouped-r1", "slice-in-out-split4", "slice-grouped",
              "fused-slice-o0", "lead-c96-own", "gelu-k1-grouped", "gelu-k3-grouped-split2"]
TILES = ["2,3,8,16,1", "2,2,8,16,0", "1,3,4,16,1", "2,5,4,16,0", "1,1,1,16,1", "2,3,4,64,0", "2,2,4,16,4", "2,3,4,16,4", "2,5,2,16,4",
         "1,3,2,16,4", "1,1,1,16,4", "2,2,8,16,5", "1,3,4,16,5"]  # (test_gpu_conv.py::test_tile_choice_never_changes_a_bit)


_TILE_BASE = {}


def test_tile_case_list_covers_every_family():
    assert {BY_ID[i]["family"] for i in TILE_CASES} == set(cc.FAMILIES)


@pytest.mark.parametrize("tile", TILES)
def test_tile_choice_never_changes_a_bit(tile):
    dev = require_gpu()
    from rgbd_amd._lib import check

    launched = 0
    for cid in TILE_CASES:
        c = BY_ID[cid]
        sets = _sets(c)
        if cid not in _TILE_BASE:  # the baseline: a register-staged tile, whatever the cost model would pick
            _TILE_BASE[cid] = run(c, sets, dev, tile=b"2,2,2,16,0")
        base = _TILE_BASE[cid]
        with switches(c, 1 if c["cout2"] else -1, tile.encode()):
            rc, outs = launch(c, sets, dev)
        if rc == -28:  # this tile cannot hold the layer's patch / taps: the launcher refuses it, nothing to compare
            continue
        check(rc, f"{cid} (forced tile {tile})")
        for g in range(c["groups"]):
            for key in base[g]:
                assert _same_bits(outs[g][key], base[g][key]), _report(outs[g][key], base[g][key], f"{cid} tile {tile} set {g} {key}")
        launched += 1
    assert launched >= 2  # (the fused forms have their own tiles: they run, and match, under every forced one)


DETERMINISM = ["plain-none", "plain-m-split4", "plain-ckbd1", "slice-out-o24", "fused-3x96x33x1-c90-k3-o177-r1-a2-m1", "fused-blk-k3",
               "lead-c192-own90", "lead-blk", "fused-grouped", "gelu-k1", "gelu-k3-s2"]


@pytest.mark.parametrize("cid", DETERMINISM)
def test_second_run_and_batch_slice_give_the_same_bits(cid):
    dev = require_gpu()
    c = BY_ID[cid]
    assert c["n"] >= 2
    sets = _sets(c)
    for cls in (CLASSES if c["cout2"] else (None,)):
        full = run(c, sets, dev, cls)
        again = run(c, sets, dev, cls)
        one = dict(c, n=1)
        part = run(one, [{k: (v[1:2] if v.shape[0] == c["n"] and k in ("x", "res1", "mul", "res2") else v) for k, v in s.items()} for s in sets],
                   dev, cls)
        for g in range(c["groups"]):
            for key in full[g]:
                assert _same_bits(full[g][key], again[g][key]), _report(again[g][key], full[g][key], f"{cid} class {cls} {key}: second run")
                assert _same_bits(full[g][key][1:2], part[g][key]), _report(part[g][key], full[g][key][1:2], f"{cid} class {cls} {key}: batch[1:2] alone")


def _refused(c, dev, cls=-1, mutate=None, splitk=None, ckbd=None):
    cc_ = dict(c, splitk=splitk if splitk is not None else c["splitk"], ckbd=ckbd if ckbd is not None else c["ckbd"])
    with switches(cc_, cls):
        rc, outs = launch(cc_, _sets(cc_), dev, mutate)
    assert rc == -22, (c["id"], rc)
    for out in outs:  # nothing was launched: every destination still holds the fill pattern
        for key, v in out.items():
            assert (_bits(v) == cc.FILL_BITS).all(), (c["id"], key)


def test_refusals():
    """Each of these is refused on the host (-22) by the launcher itself -- and by the hook's own check before anything is allocated
    or launched.  None of them reaches a kernel."""
    dev = require_gpu()
    fused, lead = BY_ID["fused-16x16"], BY_ID["lead-c96-own"]
    _refused(dict(fused, stride=2), dev, 1)                                   # fused with stride 2
    _refused(dict(fused, cout=64), dev, 1)                                    # fused with cout_pad != 96
    _refused(dict(fused, k=5, pad=2), dev, 1)                                 # fused with k = 5
    _refused(dict(fused, act=cc.ACT_SIGMOID), dev, 1)                         # fused with act = 3
    _refused(dict(fused, act_mid=2), dev, 1)
    # GELU is the reducer's: only the plain form outside the reference's CPU arithmetic, with one destination
    _refused(dict(fused, act=cc.ACT_GELU), dev, 1)
    _refused(dict(BY_ID["plain-blk-r1"], act=cc.ACT_GELU), dev)
    _refused(dict(BY_ID["plain-none-y2"], act=cc.ACT_GELU), dev)
    _refused(dict(BY_ID["plain-none"], act=5), dev)
    _refused(dict(lead, cout2=80, y_total=80), dev, 1)                        # lead with cout2_pad % 32 != 0
    _refused(dict(lead, cout3=64, y3_total=64), dev, 1)                       # (the lead layer's couts are the first layer's tile)
    _refused(BY_ID["plain-none-y2"], dev, splitk=4)                           # y2 together with split-K
    _refused(BY_ID["plain-s2-k5"], dev, ckbd=1)                               # checkerboard with stride 2
    _refused(BY_ID["plain-deconv-s2"], dev, ckbd=2)
    _refused(dict(fused, ckbd=1), dev, 1)
    grouped = BY_ID["plain-grouped-r1"]

    def drop(field):
        def f(d):
            setattr(d.set[1], field, None)
        return f

    _refused(grouped, dev, mutate=drop("res1_dev"))                           # a grouped call with one twin pointer missing
    _refused(grouped, dev, mutate=drop("x_dev"))
    _refused(grouped, dev, mutate=drop("bias"))
    _refused(BY_ID["lead-grouped"], dev, 1, mutate=drop("y3_dev"))
    _refused(BY_ID["fused-grouped"], dev, 1, mutate=drop("w2"))
    # the automatic plan returns 0 on maps this small: the fused forms then return -22, as launch_conv_fused does
    _refused(fused, dev, -1)
    _refused(fused, dev, 0)
    # placements the engine never makes: the stored channels would run over the neighbouring slice / the offsets are not aligned
    _refused(dict(BY_ID["slice-out-o0"], cout=22), dev)
    _refused(dict(BY_ID["slice-out-o24"], cout=20, y_off=26), dev)
    _refused(dict(BY_ID["slice-in-o32"], x_off=8), dev)
    _refused(BY_ID["slice-in-o32"], dev, mutate=lambda d: setattr(d, "x_off", 80))  # (past the end of the wide tensor)
    _refused(dict(lead, cout3=90, y3_total=160), dev, 1)
    _refused(dict(BY_ID["plain-blk-r1"], y_total=64, y_off=4), dev)
    _refused(BY_ID["plain-none"], dev, mutate=lambda d: setattr(d, "n", 0))
    _refused(BY_ID["plain-none"], dev, mutate=lambda d: setattr(d, "groups", 3))
