"""Input families shared by the CPU (oracle vs the reference's C++) and GPU (HIP coder vs oracle) coder tests."""
import numpy as np


def lane_edge_tables(seed, slots=(2, 3, 5, 17, 31, 32, 33, 62, 63, 64, 65, 66, 70)):
    """CDF rows of 2 ... 70 slots with random frequencies (many of them 1): the GPU decoder's first level holds 64 slots of a
    row in the 64 lanes, so 63 / 64 / 65 slots are its edges.  Returns (cdf [rows, stride], sizes, offsets, rng)."""
    rng = np.random.RandomState(100 + seed)
    slots = list(slots)
    stride = max(slots) + 1
    cdf = np.zeros((len(slots), stride), np.int32)
    for r, n in enumerate(slots):
        f = np.ones(n, np.int64)
        f += rng.multinomial(65536 - n, rng.dirichlet(np.full(n, 0.3)))
        cdf[r, : n + 1] = np.concatenate([[0], np.cumsum(f)])
        assert cdf[r, n] == 65536
    sizes = np.array([n + 1 for n in slots], np.int32)
    offsets = np.array([-(n // 2) for n in slots], np.int32)
    return cdf, sizes, offsets, rng


# rows around the decoder's coarse first level (129 ... 4032 slots: blocks of ceil(slots / 64) symbols), next to narrow rows and
# to wide rows that stay with the bucket table (65 ... 128 and > 4032 slots)
COARSE_EDGE_SLOTS = (5, 40, 64, 100, 128, 129, 130, 191, 192, 193, 1000, 4031, 4032, 4033)


def lane_edge_symbols(rng, n, sizes, offsets, rows=None):
    """n (index, symbol) pairs over those rows (or over `rows`, a sequence of row indices to draw from): every table slot, the
    first and the last one over-represented, and one in ten an escape on either side of the table."""
    idx = (rng.randint(0, len(sizes), n) if rows is None else np.asarray(rows)[rng.randint(0, len(rows), n)]).astype(np.int32)
    v = (rng.rand(n) * (sizes[idx] - 2)).astype(np.int64)      # a table slot (escape slot excluded) ...
    edge = rng.rand(n)
    v = np.where(edge < 0.15, 0, np.where(edge < 0.3, sizes[idx] - 3, v))
    sym = v + offsets[idx]
    esc = rng.rand(n) < 0.1                                     # ... or an escape on either side
    far = (2.0 ** rng.uniform(0, 20, n)).astype(np.int64)
    sym = np.where(esc, np.where(rng.rand(n) < 0.5, offsets[idx] - far, offsets[idx] + sizes[idx] - 2 + far), sym)
    return idx, sym.astype(np.int32)


def seeded_case(seed, scale_table):
    """test_oracle_coder.py::test_against_reference_cpp[seed]: n (symbol, index) pairs over the Gaussian table (2 % of them
    with four times the scale, 1 % far escapes) and 20 random pmfs of 2 ... 39 entries.  Returns (sym, idx, pmfs)."""
    rng = np.random.RandomState(seed)
    n = [17, 4096, 20000][seed]
    idx = rng.randint(0, 64, n).astype(np.int32)
    sym = np.rint(rng.standard_normal(n) * scale_table[idx] * (1 + 3 * (rng.rand(n) < 0.02))).astype(np.int32)
    sym[rng.rand(n) < 0.01] = rng.randint(-100000, 100000)
    pmfs = []
    for _ in range(20):
        m = rng.randint(2, 40)
        p = rng.rand(m).astype(np.float32) ** 4
        p /= p.sum()
        pmfs.append(p)
    return sym, idx, pmfs


def reference_cpp_vectors(ref, scale_table, gc_tables):
    """What the reference's own C++ coder (`oracle.coder.load_reference_coder()`) returns on every input of the
    *_against_reference_cpp tests: streams, decoded symbols and quantised CDFs, keyed by case.  Stored as
    tests/golden/coder_ref_cpp.npz (tests/golden/make_coder_ref.py), so that those tests run without the reference."""
    out = {}

    def encode(sym, idx, cdf_l, sz_l, off_l):
        return ref["ans"].RansEncoder().encode_with_indexes(sym.tolist(), idx.tolist(), cdf_l, sz_l, off_l)

    def decode(stream, parts, cdf_l, sz_l, off_l):
        d = ref["ans"].RansDecoder()
        d.set_stream(stream)
        return [np.array(d.decode_stream(p.tolist(), cdf_l, sz_l, off_l), np.int32) for p in parts]

    cdf_l, sz_l, off_l = gc_tables.cdf.tolist(), gc_tables.sizes.tolist(), gc_tables.offsets.tolist()
    for seed in range(3):
        sym, idx, pmfs = seeded_case(seed, scale_table)
        s = encode(sym, idx, cdf_l, sz_l, off_l)
        out[f"seeded{seed}_stream"] = np.frombuffer(s, np.uint8)
        cut = len(idx) // 3
        out[f"seeded{seed}_dec0"], out[f"seeded{seed}_dec1"] = decode(s, [idx[:cut], idx[cut:]], cdf_l, sz_l, off_l)
        for t, p in enumerate(pmfs):
            out[f"seeded{seed}_pmf{t}"] = np.array(ref["_CXX"].pmf_to_quantized_cdf([float(v) for v in p], 16), np.uint32)
    for seed in range(2):
        cdf, sizes, offsets, rng = lane_edge_tables(seed)
        tl = cdf.tolist(), sizes.tolist(), offsets.tolist()
        for n in (1, 63, 64, 65, 4000):
            idx, sym = lane_edge_symbols(rng, n, sizes, offsets)
            if n < 2:  # (the reference's flush() under-allocates its output for fewer than two symbols)
                continue
            s = encode(sym, idx, *tl)
            out[f"lane{seed}_n{n}_stream"] = np.frombuffer(s, np.uint8)
            out[f"lane{seed}_n{n}_dec"] = decode(s, [idx], *tl)[0]
    cdf, sizes, offsets, rng = lane_edge_tables(0, COARSE_EDGE_SLOTS)
    tl = cdf.tolist(), sizes.tolist(), offsets.tolist()
    for k, (n, rows) in enumerate(coarse_edge_cases()):
        idx, sym = lane_edge_symbols(rng, n, sizes, offsets, rows=rows)
        s = encode(sym, idx, *tl)
        out[f"coarse{k}_stream"] = np.frombuffer(s, np.uint8)
        out[f"coarse{k}_dec"] = decode(s, [idx], *tl)[0]
    return out


def coarse_edge_cases():
    """(n, rows) of test_oracle_coder.py::test_coarse_edge_tables_against_reference_cpp, in draw order."""
    coarse = [r for r, n in enumerate(COARSE_EDGE_SLOTS) if 128 < n <= 4032]
    return [(65, None), (3000, coarse), (3000, None)]
