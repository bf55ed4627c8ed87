"""The plain-C oracle coder against known answers produced by the reference's own C++ (tests/golden/coder_kat.npz,
tests/golden/coder_ref_cpp.npz), and against the reference C++ itself where oracle/_ref has been built.  All integer work:
bit-exact."""
import hashlib
import os

import numpy as np
import pytest

from coder_cases import (COARSE_EDGE_SLOTS, coarse_edge_cases, lane_edge_symbols, lane_edge_tables, reference_cpp_vectors,
                         seeded_case)
from conftest import GOLDEN
from oracle import coder


def _sha(b):
    return hashlib.sha256(b).hexdigest()[:16]


def _b2_inputs(table):
    rng = np.random.RandomState(1234)
    n = 49152
    idx = rng.randint(0, 64, n)
    sym = np.rint(rng.standard_normal(n) * table[idx]).astype(np.int64)
    sym[::97] *= 8
    sym[5::193] = -sym[5::193] - 3
    return sym.astype(np.int32), idx.astype(np.int32)


def test_tiny_kat(kat, gc_tables):
    s = coder.rans_encode(kat["tiny_sym"], kat["tiny_idx"], gc_tables)
    assert s == kat["tiny_stream"].tobytes()
    assert s.hex() == "3ec315415cc000009f056801115a315121ffff01f7ff2f4cffffd204"
    assert np.array_equal(coder.rans_decode(s, kat["tiny_idx"], gc_tables), kat["tiny_sym"])


def test_tiny_kat_split_decode(kat, gc_tables):
    d = coder.RansDecoder()
    d.set_stream(kat["tiny_stream"].tobytes())
    idx = kat["tiny_idx"]
    got = np.concatenate([d.decode_stream(idx[:4], gc_tables), d.decode_stream(idx[4:9], gc_tables),
                          d.decode_stream(idx[9:], gc_tables)])
    assert np.array_equal(got, kat["tiny_sym"])


def test_kat_b2(kat, gc_tables):
    sym, idx = _b2_inputs(kat["scale_table"])
    assert _sha(sym.tobytes()) == kat["b2_sym_sha"].tobytes().decode()
    assert _sha(idx.tobytes()) == kat["b2_idx_sha"].tobytes().decode()
    s = coder.rans_encode(sym, idx, gc_tables)
    assert len(s) == 28664 and _sha(s) == "e74a4ba73e7caf82"
    assert s == kat["b2_stream"].tobytes()
    assert np.array_equal(coder.rans_decode(s, idx, gc_tables), sym)


def test_escape_and_short(kat, gc_tables):
    s = coder.rans_encode(kat["esc_sym"], np.zeros_like(kat["esc_sym"]), gc_tables)
    assert s == kat["esc_stream"].tobytes()
    assert np.array_equal(coder.rans_decode(s, np.zeros_like(kat["esc_sym"]), gc_tables), kat["esc_sym"])
    assert coder.rans_encode([3, -2], [20, 7], gc_tables) == kat["two_stream"].tobytes()


def test_empty_and_single_defined(gc_tables):
    # The reference under-allocates for <2 symbols (UB, rans_interface.cpp:171); the build defines them.
    e = coder.rans_encode([], [], gc_tables)
    assert e == (1 << 31).to_bytes(8, "little")
    one = coder.rans_encode([3], [20], gc_tables)
    assert len(one) == 8 and coder.rans_decode(one, [20], gc_tables).tolist() == [3]


def test_pmf_to_quantized_cdf(kat):
    for k in range(4):
        got = coder.pmf_to_quantized_cdf(kat[f"pmf{k}"], 16)
        assert np.array_equal(got, kat[f"pmf{k}_cdf"]), k
    assert coder.pmf_to_quantized_cdf([0.1, 0.2, 0.7]).tolist() == [0, 6554, 19661, 65536]


def test_gaussian_table_facts(kat):
    assert _sha(kat["gc_cdf"].astype("<i4").tobytes()) == "482d4620b3eb5802"
    assert kat["gc_sizes"][:8].tolist() == [5, 5, 5, 5, 7, 7, 7, 7]
    assert kat["gc_sizes"][-3:].tolist() == [2449, 2769, 3133]
    assert kat["gc_offsets"][-3:].tolist() == [-1223, -1383, -1565]
    assert int(kat["gc_sizes"].sum()) == 27256
    assert kat["gc_cdf"][0, :5].tolist() == [0, 1, 65534, 65535, 65536]


def test_table_construction_matches_reference(kat):
    from oracle import elic_oracle as eo

    t = eo.gaussian_tables()
    assert np.array_equal(t.cdf, kat["gc_cdf"])
    assert np.array_equal(t.sizes, kat["gc_sizes"]) and np.array_equal(t.offsets, kat["gc_offsets"])
    assert np.array_equal(eo.scale_table().numpy(), kat["scale_table"])


@pytest.fixture(scope="module")
def ref_cpp(kat, gc_tables):
    """The reference C++ coder's answers on the inputs below (tests/golden/coder_ref_cpp.npz, tests/golden/make_coder_ref.py).
    Where oracle/_ref has been built, the stored answers are first recomputed with the reference itself and must be equal."""
    stored = dict(np.load(os.path.join(GOLDEN, "coder_ref_cpp.npz")))
    ref = coder.load_reference_coder()
    if ref is not None:
        live = reference_cpp_vectors(ref, kat["scale_table"], gc_tables)
        assert sorted(live) == sorted(stored)
        for k in live:
            assert np.array_equal(live[k], stored[k]), k
    return stored


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_against_reference_cpp(seed, kat, gc_tables, ref_cpp):
    sym, idx, pmfs = seeded_case(seed, kat["scale_table"])
    n = len(idx)
    want = ref_cpp[f"seeded{seed}_stream"].tobytes()
    assert coder.rans_encode(sym, idx, gc_tables) == want
    d = coder.RansDecoder()
    d.set_stream(want)
    cut = n // 3
    for h, (a, b) in enumerate(((0, cut), (cut, n))):
        assert d.decode_stream(idx[a:b], gc_tables).tolist() == ref_cpp[f"seeded{seed}_dec{h}"].tolist()
    for t, p in enumerate(pmfs):
        assert coder.pmf_to_quantized_cdf(p).tolist() == ref_cpp[f"seeded{seed}_pmf{t}"].tolist()


@pytest.mark.parametrize("seed", [0, 1])
def test_lane_edge_tables_against_reference_cpp(seed, ref_cpp):
    """The table family of tests/test_gpu_coder.py::test_rows_around_the_lane_count (rows of 2 ... 70 slots, frequency-1
    symbols, escapes on both sides) through the reference's own C++ coder: pins the oracle on exactly the inputs the GPU
    decoder's lane-count edges are tested with."""
    cdf, sizes, offsets, rng = lane_edge_tables(seed)
    ot = coder.Tables(cdf, sizes, offsets)
    for n in (1, 63, 64, 65, 4000):
        idx, sym = lane_edge_symbols(rng, n, sizes, offsets)
        if n < 2:  # (the reference's flush() under-allocates its output for fewer than two symbols: rans_interface.cpp:171)
            continue
        want = ref_cpp[f"lane{seed}_n{n}_stream"].tobytes()
        assert coder.rans_encode(sym, idx, ot) == want
        assert ref_cpp[f"lane{seed}_n{n}_dec"].tolist() == sym.tolist()
        assert coder.rans_decode(want, idx, ot).tolist() == sym.tolist()


def test_coarse_edge_tables_against_reference_cpp(ref_cpp):
    """The table family of tests/test_gpu_coder.py::test_rows_around_the_coarse_level (rows of 128 ... 4033 slots next to narrow
    ones, every slot, escapes on both sides) through the reference's own C++ coder: the oracle is pinned on exactly the inputs
    the GPU decoder's coarse first level is tested with."""
    cdf, sizes, offsets, rng = lane_edge_tables(0, COARSE_EDGE_SLOTS)
    ot = coder.Tables(cdf, sizes, offsets)
    for k, (n, rows) in enumerate(coarse_edge_cases()):
        idx, sym = lane_edge_symbols(rng, n, sizes, offsets, rows=rows)
        want = ref_cpp[f"coarse{k}_stream"].tobytes()
        assert coder.rans_encode(sym, idx, ot) == want
        assert ref_cpp[f"coarse{k}_dec"].tolist() == sym.tolist()
        assert coder.rans_decode(want, idx, ot).tolist() == sym.tolist()
