"""The wide-rANS kernels (csrc/rans_wide.hip) through the C ABI and rgbd_amd.ans, against the plain-Python model of the format
(tests/widecoder_cases.py): bytes, round trips segment by segment, the device-resident pair with several streams and two table
sets, slot bounds, and what the entry points refuse on the host."""
import ctypes

import numpy as np
import pytest

import widecoder_cases as wc
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC = -22, -28
SENTINEL = 0x5EA7BEEF
GUARD = 64  # sentinel words in front of the first slot and behind the last


@pytest.fixture(scope="module")
def tabs():
    require_gpu()
    from rgbd_amd import ans

    return [ans.Tables(*wc.tables(second)) for second in (False, True)]


def _by_lanes():
    return [[c[0] for c in wc.cases() if c[1] == L] for L in wc.LANES]


@pytest.mark.parametrize("ids", _by_lanes(), ids=[f"L{L}" for L in wc.LANES])
def test_encode_bytes_equal_the_model(ids, tabs):
    from rgbd_amd import ans

    cdf, sizes, offsets = wc.tables()
    for cid in ids:
        L, segs, sym, idx, want = wc.case_data(cid)
        got = ans.WideRansEncoder(L).encode_with_indexes(sym, idx, cdf, sizes, offsets, segments=segs)
        assert got == want, cid
        if L == 1 and len(segs) == 1:  # the anchor: one lane, one segment is the reference's stream
            assert got == ans._encode(tabs[0], sym, idx), cid


@pytest.mark.parametrize("ids", _by_lanes(), ids=[f"L{L}" for L in wc.LANES])
def test_decode_of_model_bytes_segment_by_segment(ids, tabs):
    from rgbd_amd import ans

    cdf, sizes, offsets = wc.tables()
    for cid in ids:
        L, segs, sym, idx, data = wc.case_data(cid)
        d = ans.WideRansDecoder(L)
        d.set_stream(data)
        got, at = [], 0
        for cnt in segs:  # one call per segment, the state carried across calls
            got += d.decode_stream(idx[at:at + cnt], cdf, sizes, offsets)
            at += cnt
        assert got == sym.tolist(), cid


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, copy=True)).cuda()


def _batch_inputs(L, n, nstreams, mix):
    syms, idxs = [], []
    for s in range(nstreams):
        sym, idx = wc.symbols(n, mix, 500 + 7 * s + L)
        syms.append(sym)
        idxs.append(idx)
    return syms, idxs


def _encode_batch(tabs, L, segs, syms, idxs, cap_words):
    """-> (rc, err, out_words [nstreams], buffer as uint32 numpy incl. guards)"""
    import torch

    from rgbd_amd._lib import lib

    ns, n = len(syms), len(syms[0])
    sym = _dev(np.concatenate(syms + [np.zeros(1, np.int32)]))
    idx = _dev(np.concatenate(idxs + [np.zeros(1, np.int32)]))
    base = _dev(np.arange(ns, dtype=np.int64) * n)
    buf = torch.full((2 * GUARD + ns * cap_words,), SENTINEL, dtype=torch.int32, device="cuda")
    ow = torch.full((ns,), -7, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    seg = (ctypes.c_int64 * len(segs))(*segs)
    rc = lib().rgbd_rans_wide_encode_batch_dev(tabs[0].handle, tabs[1].handle, min(2, ns), sym.data_ptr(), idx.data_ptr(),
                                               base.data_ptr(), ns, L, seg, len(segs), buf.data_ptr() + 4 * GUARD, cap_words,
                                               ow.data_ptr(), err.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, int(err.item()), ow.cpu().numpy(), buf.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("L", wc.LANES)
@pytest.mark.parametrize("nstreams", [1, 5])
def test_batch_dev_pair(L, nstreams, tabs):
    """nstreams streams (five: more than the four of one decoder workgroup), tables split at stream 2: bytes equal the model's,
    a second call gives the same bytes, sentinels around every slot survive, and the decoder returns the symbols."""
    import torch

    from rgbd_amd._lib import lib

    n = 3 * L + 5 + 256
    segs = [100, 28, 0, 1, n - 129]
    syms, idxs = _batch_inputs(L, n, nstreams, "all" if L != 2 else "escapes")
    t = [wc.tables(False), wc.tables(True)]
    want = [wc.encode(syms[s].tolist(), idxs[s].tolist(), *t[0 if s < 2 else 1], L, segs) for s in range(nstreams)]
    cap = int(lib().rgbd_rans_wide_max_bytes(n, L)) // 4
    runs = [_encode_batch(tabs, L, segs, syms, idxs, cap) for _ in range(2)]
    for rc, err, ow, buf in runs:
        assert rc == 0 and err == 0
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all()
        for s in range(nstreams):
            slot = buf[GUARD + s * cap: GUARD + (s + 1) * cap]
            nw = int(ow[s])
            assert slot[cap - nw:].tobytes() == want[s], (L, s)
            assert (slot[: cap - nw] == SENTINEL).all(), (L, s)  # nothing in front of the stream: both sides of every slot hold
    assert runs[0][3].tobytes() == runs[1][3].tobytes()

    # decode the model's bytes: one launch per segment and table set, state carried in HBM
    lens = np.array([len(w) // 4 for w in want], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    words = _dev(np.frombuffer(b"".join(want), np.uint32).view(np.int32))
    d_off, d_len = _dev(offs), _dev(lens)
    idx = _dev(np.concatenate(idxs))
    out = torch.full((nstreams * n,), -12345, dtype=torch.int32, device="cuda")
    base = _dev(np.arange(nstreams, dtype=np.int64) * n)
    state = torch.zeros(nstreams * (L + 1), dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    at = 0
    for k, cnt in enumerate(segs):
        for lo, hi, tb in ((0, min(2, nstreams), tabs[0]), (2, nstreams, tabs[1])):
            if hi <= lo:
                continue
            rc = lib().rgbd_rans_wide_decode_batch_dev(tb.handle, words.data_ptr(), d_off.data_ptr() + 8 * lo, d_len.data_ptr() + 8 * lo,
                                                       hi - lo, L, state.data_ptr() + 8 * lo * (L + 1), 1 if k == 0 else 0,
                                                       idx.data_ptr(), out.data_ptr(), base.data_ptr() + 8 * lo, at, cnt,
                                                       err.data_ptr(), None)
            assert rc == 0
        at += cnt
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    assert out.cpu().numpy().tolist() == np.concatenate(syms).tolist()
    pos = state.cpu().numpy().reshape(nstreams, L + 1)[:, L]
    assert pos.tolist() == lens.tolist()  # every stream read to its last word, no further


@pytest.mark.parametrize("L,nstreams", [(1, 1), (16, 1), (64, 1), (64, 5)])
def test_small_slot_sets_err_and_stays_inside(L, nstreams, tabs):
    n = 4097
    syms, idxs = _batch_inputs(L, n, nstreams, "escapes")
    cap = 2 * L + 37  # room for the flush and little else
    rc, err, ow, buf = _encode_batch(tabs, L, [n], syms, idxs, cap)
    assert rc == 0 and err != 0
    assert (ow == 0).all()
    assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all()


def test_refusals_on_the_host(tabs):
    """Every row is refused by the argument checks, which precede the first HIP call of the entry point."""
    from rgbd_amd._lib import lib

    L = lib()
    t = tabs[0].handle
    i32p, i64p, u8p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint8)
    n = 10
    sym, idx = (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)()
    cap = int(L.rgbd_rans_wide_max_bytes(n, 64))
    out, ln = (ctypes.c_uint8 * cap)(), ctypes.c_int64(-1)

    def enc(lanes=64, segs=(n,), nseg=None, cap_=cap, t_=t, sym_=sym, idx_=idx, out_=out, ln_=ctypes.byref(ln), null_segs=False):
        seg = (ctypes.c_int64 * max(1, len(segs)))(*segs)
        return L.rgbd_rans_wide_encode(t_, sym_, idx_, n, lanes, None if null_segs else seg, len(segs) if nseg is None else nseg,
                                       out_, cap_, ln_)

    for lanes in (0, -1, 3, 48, 65, 128):
        assert L.rgbd_rans_wide_max_bytes(n, lanes) == EINVAL
        assert enc(lanes=lanes) == EINVAL, lanes
    assert L.rgbd_rans_wide_max_bytes(-1, 64) == EINVAL
    assert enc(segs=(), nseg=0) == EINVAL
    assert enc(segs=(0,) * 32 + (n,), nseg=33) == EINVAL
    assert enc(segs=(n + 1, -1)) == EINVAL          # a negative count
    assert enc(segs=(4, 5)) == EINVAL               # sum below n
    assert enc(segs=(4, 7)) == EINVAL               # sum above n
    assert enc(cap_=cap - 4) == ENOSPC              # capacity below max_bytes
    assert enc(t_=None) == EINVAL and enc(sym_=None) == EINVAL and enc(idx_=None) == EINVAL
    assert enc(out_=None) == EINVAL and enc(ln_=None) == EINVAL and enc(null_segs=True) == EINVAL
    assert ln.value == -1 and bytes(out) == bytes(cap)  # nothing was written

    d = ctypes.c_void_p()
    assert L.rgbd_rans_wide_decoder_create(None) == EINVAL
    assert L.rgbd_rans_wide_decoder_create(ctypes.byref(d)) == 0
    data = (ctypes.c_uint8 * 512)()
    for lanes in (0, 3, 128):
        assert L.rgbd_rans_wide_decoder_set_stream(d, data, 512, lanes) == EINVAL
    assert L.rgbd_rans_wide_decoder_set_stream(d, data, 8 * 64 - 4, 64) == EINVAL  # shorter than 8 L bytes
    assert L.rgbd_rans_wide_decoder_set_stream(d, data, 8 * 16 - 4, 16) == EINVAL
    assert L.rgbd_rans_wide_decoder_set_stream(d, data, 130, 16) == EINVAL         # not whole words
    assert L.rgbd_rans_wide_decoder_set_stream(d, None, 512, 64) == EINVAL
    assert L.rgbd_rans_wide_decoder_set_stream(None, data, 512, 64) == EINVAL
    o = (ctypes.c_int32 * n)()
    assert L.rgbd_rans_wide_decoder_decode(d, t, idx, n, o) == EINVAL              # no stream set
    assert L.rgbd_rans_wide_decoder_decode(None, t, idx, n, o) == EINVAL
    L.rgbd_rans_wide_decoder_destroy(d)

    # the device-resident pair: the pointer values are never dereferenced by a refused call
    p = ctypes.c_void_p(4096)
    seg1 = (ctypes.c_int64 * 1)(n)

    def benc(t0=t, t1=t, split=1, sym_=p, idx_=p, base=p, ns=2, lanes=64, seg=seg1, nseg=1, out_=p, capw=cap // 4, ow=p, err=p):
        return L.rgbd_rans_wide_encode_batch_dev(t0, t1, split, sym_, idx_, base, ns, lanes, seg, nseg, out_, capw, ow, err, None)

    for kw in (dict(t0=None), dict(t1=None), dict(split=3), dict(split=-1), dict(sym_=None), dict(idx_=None), dict(base=None),
               dict(ns=-1), dict(lanes=0), dict(lanes=24), dict(seg=None), dict(nseg=0), dict(nseg=33), dict(out_=None),
               dict(capw=127), dict(capw=1 << 31), dict(ow=None), dict(err=None), dict(seg=(ctypes.c_int64 * 1)(-1))):
        assert benc(**kw) == EINVAL, kw

    def bdec(t_=t, w=p, off=p, ln_=p, ns=2, lanes=64, st=p, idx_=p, sym_=p, base=p, part=0, count=n, err=p):
        return L.rgbd_rans_wide_decode_batch_dev(t_, w, off, ln_, ns, lanes, st, 1, idx_, sym_, base, part, count, err, None)

    for kw in (dict(t_=None), dict(w=None), dict(off=None), dict(ln_=None), dict(ns=-1), dict(lanes=0), dict(lanes=5), dict(st=None),
               dict(idx_=None), dict(sym_=None), dict(base=None), dict(part=-1), dict(count=-1), dict(err=None)):
        assert bdec(**kw) == EINVAL, kw


def test_python_classes_refuse_bad_lanes():
    require_gpu()
    from rgbd_amd import ans

    for lanes in (0, 3, 128):
        with pytest.raises(ValueError):
            ans.WideRansEncoder(lanes)
        with pytest.raises(ValueError):
            ans.WideRansDecoder(lanes)
