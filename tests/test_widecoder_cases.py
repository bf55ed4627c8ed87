"""The wide-rANS format model (tests/widecoder_cases.py) on the CPU: it is the reference's stream at one lane, it round-trips
segment by segment, and its case list tells the format apart from every near miss of it."""
import numpy as np
import pytest

import widecoder_cases as wc
from oracle import coder


@pytest.fixture(scope="module")
def tabs():
    cdf, sizes, offsets = wc.tables()
    return cdf, sizes, offsets, coder.Tables(cdf, sizes, offsets)


def test_case_list_covers_the_issue():
    cs = wc.cases()
    assert len({c[0] for c in cs}) == len(cs)
    for L in wc.LANES:
        mine = [c for c in cs if c[1] == L]
        assert {c[2] for c in mine} == {0, 1, L - 1, L, L + 1, 3 * L + 5, 4097}
        for n in (3 * L + 5, 4097):
            for segs in wc.segmentations(n):
                assert {c[4] for c in mine if c[2] == n and list(c[3]) == segs} == set(wc.MIXES)
    assert any(len(c[3]) == 5 for c in cs) and any(len(c[3]) == 2 for c in cs)
    slots = np.array(wc.SLOTS)
    assert (slots <= 64).any() and ((slots > 64) & (slots <= 128)).any() and {129, 1000, 4033} <= set(wc.SLOTS)


def test_escape_mix_spans_one_to_eight_nibbles():
    cdf, sizes, offsets = wc.tables()
    sym, idx = wc.symbols(4097, "escapes", 7)
    counts, sides = set(), set()
    for s, t in zip(sym.tolist(), idx.tolist()):
        it = wc.items_of(s, t, cdf, sizes, offsets)
        if len(it) > 1:
            counts.add(it[1][0])
            sides.add(s < offsets[t])
        assert abs(s - int(offsets[t])) < 1 << 30
    assert set(range(1, 9)) <= counts and sides == {True, False}


def test_one_lane_one_segment_is_the_reference_stream(tabs):
    cdf, sizes, offsets, ot = tabs
    seen = 0
    for cid, L, n, segs, mix, seed in wc.cases():
        sym, idx = wc.symbols(n, mix, seed)  # every (n, mix, seed) of the list, whatever its L and segmentation
        got = wc.encode(sym.tolist(), idx.tolist(), cdf, sizes, offsets, 1)
        assert got == coder.rans_encode(sym, idx, ot), cid
        seen += 1
    assert seen == len(wc.cases())


def test_every_case_round_trips_segment_by_segment():
    cdf, sizes, offsets = wc.tables()
    for c in wc.cases():
        L, segs, sym, idx, data = wc.case_data(c[0])
        assert len(data) % 4 == 0 and len(data) >= 8 * L
        d = wc.Decoder()
        d.set_stream(data, L)
        got, at = [], 0
        for cnt in segs:
            got += d.decode(idx[at:at + cnt].tolist(), cdf, sizes, offsets)
            at += cnt
        assert got == sym.tolist(), c[0]
        assert d.pos == len(data) // 4, c[0]  # every word is read, none twice


@pytest.mark.parametrize("wrong", wc.WRONG)
def test_cases_discriminate(wrong):
    """Each wrong restatement of the format changes the bytes of at least one case."""
    cdf, sizes, offsets = wc.tables()
    for c in wc.cases():
        L, segs, sym, idx, data = wc.case_data(c[0])
        if wc.encode(sym.tolist(), idx.tolist(), cdf, sizes, offsets, L, segs, wrong=wrong) != data:
            return
    pytest.fail(f"no case tells the format from `{wrong}`")
