"""Are the cases of tests/refpointwise_cases.py worth running?  (No GPU.)

tests/test_gpu_refpointwise.py compares the reference-arithmetic pointwise kernels with oracle/cpu_arith.c bit for bit.  Such a
test only proves something if a neighbouring arithmetic would have produced other bits ON THAT INPUT: here, for the committed
seeds, every case is shown to tell the oracle's structure from the next-simpler one."""
import ctypes

import numpy as np
import pytest

import refpointwise_cases as rc
from oracle import cpu_arith as ca


# ------------------------------------------------------------------------------------------------ mean
@pytest.mark.parametrize("shape", rc.MEAN_SHAPES + list(rc.MEAN_CAT), ids=str)
def test_mean_cases_tell_the_cascade_levels_apart(shape):
    x = rc.mean_input(shape)
    n, c, h, w = shape
    hw = h * w
    want = rc.mean_expected(x).reshape(-1)
    rows = x.reshape(n * c, hw)
    assert np.array_equal(rc.cascade_mean(rows, 3), want)  # the numpy cascade IS the oracle's when no level is withheld
    assert (rc.sequential_mean(rows) != want).any(), "the plain sequential sum gives the same means"
    if hw >= 8192:
        d = int((rc.cascade_mean(rows, 1) != want).sum())
        assert d >= 1, "a cascade without level 2 gives the same means: the case does not reach level 2"
    if hw >= 131072:
        d = int((rc.cascade_mean(rows, 2) != want).sum())
        assert d >= 1, "a cascade without level 3 gives the same means: the case does not reach level 3"


def test_mean_cases_reach_level_2_and_3():
    hws = [s[2] * s[3] for s in rc.MEAN_SHAPES]
    assert sum(8192 <= v < 131072 for v in hws) >= 2 and sum(v >= 131072 for v in hws) >= 1
    assert max(s[0] * s[1] * s[2] * s[3] for s in rc.MEAN_SHAPES) == 16 * 512 * 640  # the largest tensor of the GPU module


# ------------------------------------------------------------------------------------------------ Linear
def test_linear_case_list_is_what_it_claims():
    groups = {g: [c for c in rc.LINEAR_CASES if c["group"] == g] for g in "abcd"}
    assert len(groups["a"]) == len(rc.TABLES["linear"]) == 46
    assert {(c["K"], c["stage"]) for c in groups["b"]} == {(k, 1) for k in rc.LIN_K} | {(k, 0) for k in (16, 32, 48, 64, 176, 2816)}
    assert {(c["K"], c["stage"]) for c in groups["c"]} == {(k, 1) for k in rc.LIN_K_FORM3} | {(k, 0) for k in (16, 48, 64, 176, 2816)}
    assert {(c["n"], c["act"], c["stage"]) for c in groups["d"]} == {(n, a, s) for n in (1, 2, 3) for a in (0, 1, 3) for s in (0, 1)}
    assert len({c["id"] for c in rc.LINEAR_CASES}) == len(rc.LINEAR_CASES)
    for c in groups["a"]:
        _, _, cls = rc.linear_inputs(c)
        assert len(cls) == c["J"] and (c["K"] if c["stage"] == 0 else c["J"]) % 16 == 0


@pytest.mark.parametrize("case", [c for c in rc.LINEAR_CASES if c["group"] in "bc"], ids=rc.case_id)
def test_linear_cases_tell_the_orders_apart(case):
    """the oracle under each OTHER class / form differs in at least one row (exempt: the pairs that are the same arithmetic by
    construction at this K, rc.linear_same_arithmetic)"""
    W, x, cls = rc.linear_inputs(case)
    K, J = case["K"], case["J"]
    want = rc.linear_raw(W, x, cls, case["form"])
    mine = np.full(J, 3, np.int32) if case["form"] == 3 else cls
    for other in (0, 1, 2, 3):
        alt = rc.linear_raw(W, x, None if other == 3 else np.full(J, other, np.int32), 3 if other == 3 else -1)
        rows = np.array([not rc.linear_same_arithmetic(K, int(m), other) for m in mine])  # rows on which `other` is another order
        if not rows.any():
            assert np.array_equal(alt, want), (K, other)  # ... and where it is the same one, it gives the same floats
            continue
        assert (alt[:, rows] != want[:, rows]).any(), f"K {K}: order {other} gives the same floats as {case['id']}"


# ------------------------------------------------------------------------------------------------ sigmoid gate
@pytest.mark.parametrize("case", rc.SIGMOID_CASES, ids=rc.case_id)
def test_sigmoid_cases_have_a_discriminating_argument_on_every_tail_position(case):
    t, mul, res, tail, planted, special = rc.sigmoid_inputs(case)
    # the numpy tail map is ATen's rule as the oracle states it
    n = t.shape[0]
    numel = t[0].size if case["per_image"] else t.size
    tm = tail.reshape(n, -1)[0] if case["per_image"] else tail.reshape(-1)
    probe = np.unique(np.concatenate([np.arange(0, numel, max(1, numel // 997)), np.flatnonzero(tm), np.flatnonzero(tm) - 1,
                                      [0, numel - 1]]))
    probe = probe[(probe >= 0) & (probe < numel)]
    for i in probe:
        assert bool(ca.lib().orc_aten_scalar_tail(ctypes.c_int64(int(i)), ctypes.c_int64(numel), case["threads"])) == bool(tm[i])
    vec, sca = ca.sigmoid(t).reshape(t.shape), rc.scalar_sigmoid(t).reshape(t.shape)
    differs = vec.view(np.uint32) != sca.view(np.uint32)
    assert differs[tail & ~special].all(), "a tail position holds an argument on which both sigmoid forms agree"
    # (1 x 16 x 5 x 7 has 560 elements in all: there every body position is planted)
    assert int((differs & ~tail).sum()) >= min(1000, int((~tail).sum()))
    assert np.array_equal(planted & ~special, planted) and differs[planted].all()
    if case["specials"]:
        for where in (tail, ~tail):  # every special value on a tail AND on a body position
            have = t[special & where]
            assert have.size == rc.SPECIALS.size
            assert np.array_equal(np.sort(have.view(np.uint32)), np.sort(rc.SPECIALS.view(np.uint32)))
        # the denormal range is really reached: sigmoid(-88) = 6.05e-39 in both forms
        want = rc.sigmoid_expected(dict(case, mul=False, res=False), t, None, None)
        den = want[(t == np.float32(-88.0))]
        assert den.size == 2 and (den > 0).all() and (den < np.finfo(np.float32).tiny).all()
    else:
        assert not special.any()


def test_sigmoid_case_list_is_what_it_claims():
    grid = {(c["shape"], c["threads"], c["per_image"]) for c in rc.SIGMOID_CASES if not c["specials"]}
    assert grid == {(s, t, p) for s in rc.SIG_SHAPES for t in rc.SIG_THREADS for p in (0, 1)}
    assert {(c["mul"], c["res"]) for c in rc.SIGMOID_CASES if c["shape"] == (1, 320, 16, 16) and c["specials"]} == \
        {(m, r) for m in (False, True) for r in (False, True)}
    tails = {c["id"]: int(rc.sigmoid_inputs(c)[3].sum()) for c in rc.SIGMOID_CASES if c["threads"] == 8 and not c["specials"]}
    assert tails["1x320x16x16-t8-pi0-mul0-res0"] == 32 and tails["2x320x8x8-t8-pi0-mul0-res0"] == 0


# ------------------------------------------------------------------------------------------------ small conv
@pytest.mark.parametrize("case", rc.SMALL_CONV_CASES, ids=rc.case_id)
def test_small_conv_cases_tell_the_k_blocks_apart(case):
    k, cin = case["k"], case["cin"]
    assert sum(case["kblocks"]) == cin * k * k and 1 <= len(case["kblocks"]) <= 16
    x, wt, b, extra = rc.small_conv_inputs(case)
    want = rc.small_conv_expected(case, x, wt, b, extra)
    if len(case["kblocks"]) > 1:
        assert (rc.small_conv_expected(case, x, wt, b, extra, kblocks=[cin * k * k]) != want).any(), "one K block gives the same floats"
    if case["ckbd"]:
        assert (want == 0).sum() >= want.size // 2 - want.shape[0] * want.shape[1] * want.shape[2]


def test_small_conv_case_list_is_what_it_claims():
    syn = [c for c in rc.SMALL_CONV_CASES if c["id"].startswith("syn")]
    assert len(rc.SMALL_CONV_CASES) - len(syn) == len(rc.TABLES["im2col"]) == 32
    assert {(c["k"], c["stride"], c["pad"]) for c in syn} >= {(k, s, p) for k in (1, 2, 3) for s in (1, 2) for p in (0, 1)}
    assert {len(c["kblocks"]) for c in syn} == {1, 2, 5, 16} and {c["cout"] for c in syn} == {32, 42}
    assert {len(c["kblocks"]) for c in syn if c["stride"] == 2 and c["pad"] == 1 and c["k"] == 3} >= {2, 5, 16}
    assert {c["act"] for c in syn if c["res1"] and c["mul"] and c["res2"]} == {0, 1, 2, 3}
    assert {c["ckbd"] for c in syn} == {0, 1, 2} and all(c["n"] == 2 for c in syn)
    for c in syn:  # a boundary inside a channel's taps
        if c["k"] > 1 and len(c["kblocks"]) > 1:
            assert any(v % (c["k"] * c["k"]) for v in np.cumsum(c["kblocks"])[:-1]), c["id"]


# ------------------------------------------------------------------------------------------------ stride-2 deconv
SYN_DECONV = [c for c in rc.DECONV_CASES if c["id"].startswith("syn")]


@pytest.mark.parametrize("case", SYN_DECONV, ids=rc.case_id)
def test_deconv_cases_tell_the_chains_apart(case):
    w = case["w"]
    off = rc.recipe_offsets(case["recipe"], w)
    flat = case["recipe"]
    for i, o in enumerate(off):  # every descriptor: the full tap set of its phase, first tap fresh
        ph = i // w
        taps = [(flat[o + 1 + 3 * t], flat[o + 2 + 3 * t]) for t in range(flat[o])]
        assert sorted(taps) == rc.phase_taps(ph >> 1, ph & 1) and flat[o + 3] == 1
        fresh = [flat[o + 3 + 3 * t] for t in range(flat[o])]
        assert case["variant"] != "one_chain" or sum(fresh) == 1
        assert case["variant"] != "all_fresh" or sum(fresh) == len(fresh)
    x, wt, b = rc.deconv_inputs(case)
    want = rc.deconv_expected(case, x, wt, b)
    if case["variant"] == "one_chain":
        return
    alt = rc.deconv_expected(case, x, wt, b, recipe=rc.one_chain(flat))
    if case["id"].startswith(rc.DECONV_SAME_AS_ONE_CHAIN):
        assert np.array_equal(alt, want)  # (exempt by name: one tap per output pixel)
    else:
        assert (alt != want).any(), "the one-chain recipe gives the same floats"


def test_deconv_case_list_is_what_it_claims():
    assert len(rc.DECONV_CASES) - len(SYN_DECONV) == len(rc.TABLES["deconv_s2"]) == 22
    assert {c["B"] for c in rc.DECONV_CASES if c["id"].startswith("table")} == {1, 2}
    assert {(c["B"], c["cin"], c["cout"], c["h"], c["w"]) for c in SYN_DECONV} == set(rc.DECONV_SYN_SHAPES)
    assert {c["act"] for c in SYN_DECONV} == {rc.ACT_NONE, rc.ACT_LEAKY}

    def widths(c):  # widths of the runs of equal descriptors, per phase
        off = list(rc.recipe_offsets(c["recipe"], c["w"])) + [len(c["recipe"])]
        d = [tuple(c["recipe"][off[i]:off[i + 1]]) for i in range(4 * c["w"])]
        out = []
        for ph in range(4):
            row, run = d[ph * c["w"]:(ph + 1) * c["w"]], 1
            for a, b in zip(row, row[1:]):
                if a == b:
                    run += 1
                else:
                    out.append(run)
                    run = 1
            out.append(run)
        return out

    drawn = {c["id"]: widths(c) for c in SYN_DECONV if c["variant"] == "drawn"}
    assert set(drawn["syn-2-48-32-4x4-drawn"]) == {1}              # a class change in every column
    assert set(drawn["syn-1-40-16-2x9-drawn"]) == {9}              # one class of width w
    assert 1 in drawn["syn-3-64-80-5x7-drawn"] and max(drawn["syn-3-64-80-5x7-drawn"]) > 1
