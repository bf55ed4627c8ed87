"""Wide rANS, the lane-interleaved stream format (include/rgbd_amd.h): a plain-Python model of the format --
integer arithmetic only, nothing imported from the product -- and the case list the CPU test (the model against the oracle
coder and against wrong restatements of itself) and the GPU tests (the HIP kernels against the model) share.

The format, as its decoder reads it.  L Rans64 states x_0 ... x_(L-1); the stream is 32-bit little-endian words.
  start-up   x_l = w[2l] | w[2l+1] << 32, pos = 2L
  a call     decodes one SEGMENT of c symbols: symbol i belongs to lane i mod L and row i div L
  a symbol   is a list of items: the table symbol; for the escape slot one count nibble and that many payload nibbles
             (rans_interface.cpp:119-163 with the count below 15: an int32 symbol needs at most 8 nibbles)
  a row      runs rounds j = 0, 1, ...: every lane whose symbol has an item j decodes it on its own state (Rans64DecGet /
             Rans64DecAdvance / Rans64DecGetBits without their renormalisation), then the lanes whose state fell below 2^31
             take one word each from pos upward, in increasing lane order; the row ends when no lane has a further item
The encoder is the inverse: segments, rows and rounds backwards, the lanes of a round from the highest down, each writing its
renormalisation word in front of what is written already; at the end lanes L-1 ... 0 are flushed (Rans64EncFlush)."""
import bisect
import functools

import numpy as np

RANS_L = 1 << 31
MASK32 = 0xFFFFFFFF
MAX_NIB = 8

# the ways to get the format wrong that the case list must tell apart from the format (test_widecoder_cases.py)
WRONG = ("ascending_lanes", "rounds_forward", "rows_across_segments", "flush_reversed", "words_per_lane")


def items_of(sym, ti, cdf, sizes, offsets):
    """[(start, freq, nbits)]: nbits 16 for the table symbol, 4 for a bypass nibble (rans_interface.cpp:119-163)."""
    top = int(sizes[ti]) - 2
    v = int(sym) - int(offsets[ti])
    raw = 0
    if v < 0:
        raw, v = -2 * v - 1, top
    elif v >= top:
        raw, v = 2 * (v - top), top
    row = cdf[ti]
    out = [(int(row[v]), int(row[v + 1]) - int(row[v]), 16)]
    if v == top:
        nn = 0
        while raw >> (4 * nn):
            nn += 1
        assert nn <= MAX_NIB
        out.append((nn, 1, 4))
        for j in range(nn):
            out.append(((raw >> (4 * j)) & 15, 1, 4))
    return out


def _put(x, item, emit):
    start, freq, nbits = item
    if nbits == 4:
        freq = 1 << 12  # Rans64EncPutBits: a symbol of frequency 2^(16 - nbits)
    if x >= ((RANS_L >> 16) << 32) * freq:
        emit(x & MASK32)
        x >>= 32
    return (x << 4) | start if nbits == 4 else ((x // freq) << 16) + (x % freq) + start


def encode(sym, idx, cdf, sizes, offsets, lanes, segments=None, wrong=None):
    """The stream as bytes.  `wrong`: one of WRONG, a deliberate misstatement of the format."""
    n = len(sym)
    segs = [n] if segments is None else list(segments)
    assert sum(segs) == n and all(c >= 0 for c in segs) and 1 <= len(segs) <= 32
    if wrong == "rows_across_segments":
        segs = [n]
    L = lanes
    x = [RANS_L] * L
    back = []  # words in the order they are written: from the end of the stream towards its head
    lane_order = list(range(L)) if wrong == "ascending_lanes" else list(range(L - 1, -1, -1))
    off = n
    for c in reversed(segs):
        off -= c
        for r in range((c + L - 1) // L - 1, -1, -1):
            its = [items_of(sym[off + r * L + l], idx[off + r * L + l], cdf, sizes, offsets) for l in range(min(L, c - r * L))]
            deepest = max(len(i) for i in its)
            rounds = list(range(deepest)) if wrong == "rounds_forward" else list(range(deepest - 1, -1, -1))
            if wrong == "words_per_lane":  # every lane finishes its symbol before the next lane starts
                steps = [(j, l) for l in lane_order for j in rounds]
            else:
                steps = [(j, l) for j in rounds for l in lane_order]
            for j, l in steps:
                if l < len(its) and j < len(its[l]):
                    x[l] = _put(x[l], its[l][j], back.append)
    for l in (range(L) if wrong == "flush_reversed" else range(L - 1, -1, -1)):
        back.append(x[l] >> 32)
        back.append(x[l] & MASK32)
    return np.array(back[::-1], dtype="<u4").tobytes()


class Decoder:
    """Stateful: set_stream(), then one decode() per segment."""

    def set_stream(self, data, lanes):
        w = np.frombuffer(bytes(data), dtype="<u4")
        if len(w) < 2 * lanes:
            raise ValueError("stream shorter than its states")
        self.w = [int(v) for v in w]
        self.L = lanes
        self.x = [self.w[2 * l] | (self.w[2 * l + 1] << 32) for l in range(lanes)]
        self.pos = 2 * lanes

    def _renorm(self, lanes_in_order):
        for l in lanes_in_order:
            if self.x[l] < RANS_L:
                if self.pos >= len(self.w):
                    raise ValueError("read past the end of the stream")
                self.x[l] = (self.x[l] << 32) | self.w[self.pos]
                self.pos += 1

    def decode(self, idx, cdf, sizes, offsets):
        L, c, out = self.L, len(idx), []
        for r in range((c + L - 1) // L):
            m = min(L, c - r * L)
            ti = [int(idx[r * L + l]) for l in range(m)]
            val = [0] * m
            # round 0: the table symbol
            for l in range(m):
                row, last = cdf[ti[l]], int(sizes[ti[l]]) - 2
                cum = self.x[l] & 0xFFFF
                a = bisect.bisect_right(row, cum, 0, last + 2) - 1  # the slot with row[a] <= cum < row[a + 1]
                start, freq = int(row[a]), int(row[a + 1]) - int(row[a])
                self.x[l] = freq * (self.x[l] >> 16) + cum - start
                val[l] = a
            self._renorm(range(m))
            esc = [l for l in range(m) if val[l] == int(sizes[ti[l]]) - 2]
            # round 1: the count; rounds 2 ...: the payload, low nibble first
            left, raw = {}, {}
            for l in esc:
                left[l], raw[l] = self.x[l] & 15, 0
                self.x[l] >>= 4
                if left[l] > MAX_NIB:
                    raise ValueError("escape of more than 8 nibbles")
            self._renorm(esc)
            k = 0
            while True:
                act = [l for l in esc if k < left[l]]
                if not act:
                    break
                for l in act:
                    raw[l] |= (self.x[l] & 15) << (4 * k)
                    self.x[l] >>= 4
                self._renorm(act)
                k += 1
            for l in esc:
                last = int(sizes[ti[l]]) - 2
                val[l] = -(raw[l] >> 1) - 1 if raw[l] & 1 else (raw[l] >> 1) + last
            out += [val[l] + int(offsets[ti[l]]) for l in range(m)]
        return out


# ---- the case list ----------------------------------------------------------------------------------------------------------
LANES = (1, 2, 16, 64)
SLOTS = (2, 3, 17, 63, 64, 65, 100, 128, 129, 1000, 4033)  # rows of <= 64, 65 ... 128, and 129 / 1000 / 4033 slots
MIXES = {"narrow": [r for r, s in enumerate(SLOTS) if s <= 64], "mid": [r for r, s in enumerate(SLOTS) if 64 < s <= 128],
         "wide": [r for r, s in enumerate(SLOTS) if s > 128], "all": list(range(len(SLOTS))), "escapes": list(range(len(SLOTS)))}


@functools.lru_cache(maxsize=None)
def tables(second=False):
    """(cdf [rows, stride] int32, sizes, offsets): random frequencies, many of them 1.  second: another set over the same row
    sizes (the launches take two table sets, split at a stream index)."""
    rng = np.random.RandomState(977 if second else 4242)
    stride = max(SLOTS) + 1
    cdf = np.zeros((len(SLOTS), stride), np.int32)
    for r, n in enumerate(SLOTS):
        f = np.ones(n, np.int64) + rng.multinomial(65536 - n, rng.dirichlet(np.full(n, 0.3)))
        cdf[r, : n + 1] = np.concatenate([[0], np.cumsum(f)])
        assert cdf[r, n] == 65536
    sizes = np.array([n + 1 for n in SLOTS], np.int32)  # (the reference's cdf_length - 1 = slots, the last one the escape)
    offsets = np.array([-(n // 2) for n in SLOTS], np.int32)
    return cdf, sizes, offsets


def symbols(n, mix, seed):
    """n (symbol, index) pairs over the rows of `mix`.  Ordinary mixes: every slot, the first and the last over-represented,
    one in ten an escape; "escapes": seven in ten an escape, on both sides of the row, with payloads of 1 ... 8 nibbles and
    |symbol - offset| < 2^30."""
    _, sizes, offsets = tables()
    rng = np.random.RandomState(1000 + seed)
    rows = np.asarray(MIXES[mix])
    idx = rows[rng.randint(0, len(rows), n)].astype(np.int32)
    top = sizes[idx].astype(np.int64) - 2
    v = (rng.rand(n) * top).astype(np.int64)
    edge = rng.rand(n)
    v = np.where(edge < 0.15, 0, np.where(edge < 0.3, np.maximum(top - 1, 0), v))
    esc = rng.rand(n) < (0.7 if mix == "escapes" else 0.1)
    far = (2.0 ** rng.uniform(0, 29.9 if mix == "escapes" else 20, n)).astype(np.int64)  # raw = 2 far (- 1) < 2^31: <= 8 nibbles
    far = np.minimum(far, (1 << 30) - 5000)
    v = np.where(esc, np.where(rng.rand(n) < 0.5, -far, top + far - 1), v)
    return (v + offsets[idx]).astype(np.int32), idx


def segmentations(n):
    out = [[n]]
    if n >= 1:
        out.append([1, n - 1])
    if n >= 129:
        out.append([100, 28, 0, 1, n - 129])
    return out


def sizes_for(L):
    return sorted({0, 1, L - 1, L, L + 1, 3 * L + 5, 4097})


@functools.lru_cache(maxsize=None)
def cases():
    """[(id, lanes, n, segments, mix, seed)]: every (L, n, segmentation); every mix on the two largest sizes, one mix in turn on
    the small ones."""
    out, turn = [], 0
    names = list(MIXES)
    for L in LANES:
        for n in sizes_for(L):
            for segs in segmentations(n):
                if n >= 3 * L + 5:
                    mixes = names
                else:
                    mixes = [names[turn % len(names)]]
                    turn += 1
                for mix in mixes:
                    seed = len(out)
                    out.append((f"L{L}-n{n}-s{len(segs)}-{mix}", L, n, tuple(segs), mix, seed))
    return out


@functools.lru_cache(maxsize=None)
def case_data(case_id):
    """(lanes, segments, sym, idx, model bytes) of a case; computed once per process."""
    cid, L, n, segs, mix, seed = next(c for c in cases() if c[0] == case_id)
    cdf, sizes, offsets = tables()
    sym, idx = symbols(n, mix, seed)
    return L, list(segs), sym, idx, encode(sym.tolist(), idx.tolist(), cdf, sizes, offsets, L, list(segs))
