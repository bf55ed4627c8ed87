"""The fused GDN / IGDN launch (csrc/gdn.hip) alone, behind rgbd_gdn_nchw (include/rgbd_amd.h), against the same formula in
float64 evaluated from the fp32 parametrized beta / gamma:

    out[n, i, p] = x[n, i, p] * f(beta'[i] + sum_j gamma'[i, j] * x[n, j, p]^2)  (+ res[n, i, p]),  f = 1 / sqrt or sqrt

Tolerance, per element (a bound from the arithmetic, not a measurement): the norm is a chain of c + 1 non-negative fp32 terms
(relative error <= (c + 1) * 2^-24 before, half of that after the square root), then come four single roundings (square of x,
sqrt, divide, multiply), then the residual add rounds the result once:

    |out - ref| <= ((c / 2 + 4) * |x * f(norm)| + |ref|) * 2^-24

The raw gamma is dense with values below the parametrizer's bound (the clamp acts), beta varies per channel, and the inputs
span 1e-3 ... 1e2 in magnitude with exact zeros.

The second half of the file runs the launch in the engine's own layout, through rgbd_gdn_pack + rgbd_gdn_nhwc (the boundary
Engine::gdn uses: a GdnArgs and launch_gdn, nothing else), on the cases of tests/gdn_cases.py: c up to 512 (one, two and
three passes of 12 output tiles; four-wave splits with a short or empty last part), pixel counts around every tile boundary,
each channel stride larger than cs on its own and all three different (NaN behind cs in x / res, a sentinel behind cs in y),
and maps large enough for the launcher to choose the 32- and 64-pixel tiles itself.  Same bound, through
gdn_cases.accept; tests/test_gdn_cases.py shows on the CPU that this function rejects ten kinds of wrong kernel.

One-line changes to csrc/gdn.hip tried on scratch builds on the MI355X, each alone ("before" = the 22 tests this file had
before the second half and the shapes c = 208 / 320 / 512 were added; 113 tests now):
  * `it0 += kGdnIT` -> the body runs once (`break`): before all pass; 22 fail now -- nhwc_vs_f64[auto-c272-n32773] (the one
    case whose automatic tile walks 17 output tiles in one wave), same_bits_for_every_tile on all 20 cases with cs > 192
    (tiles 32 / 64 differ from tile 16), dense_equals_the_public_operator[auto-c272-n32773].
  * `(part + 1) * per` -> `part * per + per - 1`: this one drops the last output tile of EVERY wave's part, also at
    NT = 12, so "before" already failed (21 of 22); 102 of 113 fail now.  The mistake of that kind which "before" does not
    see is `per` rounded down (`max(1, NT / WS)`: the tiles behind 4 * (NT / 4) are dropped): before all pass; 53 fail now --
    every case and shape with NT % 4 != 0 and NT > 4 (nhwc_vs_f64 17, same_bits 18, dense_equals 13, vs_f64[1x208x3x5] 4,
    nhwc_bad_arguments' final good call).
  * `a.res + gp * a.rcs` -> `a.res + gp * a.xcs`: before all pass; 11 fail now -- nhwc_vs_f64 and strided_equals_dense on the
    5 cases with xcs != rcs, and nhwc_bad_arguments' final good call.
  * `gp * a.ycs` -> `gp * a.cs`: before all pass; 9 fail now -- the same two tests on the 4 cases with ycs > cs, and
    nhwc_bad_arguments' final good call.
  * `gp < a.npix` dropped in the epilogue: run on the new nhwc tests only (their buffers are 64 pixels longer than npix, so
    the stray rows stay inside them; rgbd_gdn_nchw's internal buffers are not, which is why "before" was not run: from the
    code it cannot see the mistake, it reads back [0, npix) only): 55 of 59 fail -- every case but npix = 16 and 64 (guard
    band written; tiles 32 / 64 at npix = 16 are caught by same_bits).
"""
import ctypes

import numpy as np
import pytest
import torch

import gdn_cases as gc
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

EINVAL = -22
SENTINEL = 12345.0
GUARD = 4096
SHAPES = [(1, 16, 1, 1), (1, 20, 3, 5), (2, 192, 7, 9), (1, 128, 8, 8), (3, 192, 4, 4),
          (1, 208, 3, 5), (1, 320, 3, 5), (1, 512, 3, 5)]  # (the last three: the public operator's upper range, up to three passes)
ZERO_PIXEL_SHAPE = (2, 192, 7, 9)  # image 1, pixel (3, 4) is all zeros there: norm = beta


def _lib():
    require_gpu()
    from rgbd_amd import _lib as lib

    return lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _params(c, seed):
    """Raw beta [c] / gamma [c, c] as a state_dict holds them (before NonNegativeParametrizer.forward)."""
    g = torch.Generator().manual_seed(1000 + seed)
    beta = torch.sqrt(0.2 + 2.0 * torch.rand(c, generator=g))  # beta' in 0.2 ... 2.2, a different one per channel
    gamma = 0.08 * torch.rand(c, c, generator=g) - 0.015       # dense; about a fifth of it below the bound 2^-18
    gamma += torch.sqrt(torch.tensor(0.1)) * torch.eye(c)
    return beta.float().contiguous(), gamma.float().contiguous()


def _parametrized(raw, minimum):
    """NonNegativeParametrizer.forward (ops/parametrizers.py:21-45) as torch computes it in fp32."""
    pedestal = torch.tensor([(2.0 ** -18) ** 2], dtype=torch.float32)
    bound = torch.tensor([(minimum + (2.0 ** -18) ** 2) ** 0.5], dtype=torch.float32)
    return torch.max(raw, bound) ** 2 - pedestal


def _inputs(shape, seed):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (5.0 * torch.rand(shape, generator=g) - 3.0)  # 1e-3 ... 1e2
    x = mag * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    x = torch.where(torch.rand(shape, generator=g) < 0.1, torch.zeros(()), x).float()
    if shape == ZERO_PIXEL_SHAPE:
        x[1, :, 3, 4] = 0.0
    res = (3.0 * torch.randn(shape, generator=g)).float()
    return x.contiguous(), res.contiguous()


_CASES = {}


def _case(shape):
    """(x, res, raw beta, raw gamma, {(inverse, with_res): (float64 reference, tolerance)}): computed once per shape."""
    if shape not in _CASES:
        c = shape[1]
        x, res = _inputs(shape, 7 * c + shape[0])
        beta, gamma = _params(c, c)
        bp, gp = _parametrized(beta, 1e-6).double(), _parametrized(gamma, 0.0).double()
        assert (gamma < 2.0 ** -18).float().mean() > 0.05 and (gp > 0).float().mean() > 0.5
        xd = x.double()
        norm = bp[None, :, None, None] + torch.einsum("ij,njhw->nihw", gp, xd * xd)
        refs = {}
        for inverse in (0, 1):
            core = xd * (torch.sqrt(norm) if inverse else 1.0 / torch.sqrt(norm))
            for with_res in (0, 1):
                ref = core + res.double() if with_res else core
                tol = ((c / 2 + 4) * core.abs() + ref.abs()) * 2.0 ** -24
                refs[(inverse, with_res)] = (ref, tol)
        _CASES[shape] = (x, res, beta, gamma, refs)
    return _CASES[shape]


def _run(L, x, beta, gamma, inverse, res, expect=0):
    """One rgbd_gdn_nchw call on device copies; returns the destination (with its guard region) as a CPU tensor."""
    n, c, h, w = x.shape
    xd = x.cuda()
    rd = res.cuda() if res is not None else None
    y = torch.full((x.numel() + GUARD,), SENTINEL, device="cuda")
    b, g = beta.numpy(), gamma.numpy()
    rc = L.rgbd_gdn_nchw(xd.data_ptr(), n, c, h, w, _f32p(b), _f32p(g), inverse, rd.data_ptr() if rd is not None else None,
                         y.data_ptr(), _stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("with_res", [0, 1])
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gdn_vs_f64(shape, inverse, with_res):
    L = _lib()
    x, res, beta, gamma, refs = _case(shape)
    ref, tol = refs[(inverse, with_res)]
    y = _run(L, x, beta, gamma, inverse, res if with_res else None)
    out = y[:x.numel()].view(shape)
    assert torch.isfinite(out).all()
    err = (out.double() - ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"gdn {shape} inverse={inverse} res={with_res}: worst |err| / bound = {worst:.3f}")
    assert (err <= tol).all(), f"worst |err| / bound = {worst}"
    assert (y[x.numel():] == SENTINEL).all(), "the guard region behind the destination was written"
    # x = 0 gives exactly the residual (or 0); at the all-zero pixel the norm is beta itself
    zero = x == 0
    assert (out[zero] == (res[zero] if with_res else 0.0)).all()


def test_gdn_same_bits_across_calls_batches_and_tiles():
    """Equal bits for two calls, for B = 3 against three B = 1 calls, and for every pixel tile the launcher can be forced to."""
    L = _lib()
    try:
        for shape in ((3, 192, 4, 4), (2, 192, 7, 9), (1, 20, 3, 5)):
            x, res, beta, gamma, _ = _case(shape)
            for inverse in (0, 1):
                for r in (None, res):
                    assert L.rgbd_debug_force_gdn_tile(0) == 0
                    a = _run(L, x, beta, gamma, inverse, r)
                    assert torch.equal(a, _run(L, x, beta, gamma, inverse, r)), "two calls differ"
                    per = [_run(L, x[i:i + 1], beta, gamma, inverse, None if r is None else r[i:i + 1])[:x[0].numel()]
                           for i in range(shape[0])]
                    assert torch.equal(a[:x.numel()], torch.cat(per)), "the batch and its images one by one differ"
                    for tile in (16, 32, 64):
                        assert L.rgbd_debug_force_gdn_tile(tile) == 0
                        assert torch.equal(a, _run(L, x, beta, gamma, inverse, r)), f"tile {tile} differs from the automatic one"
        assert L.rgbd_debug_force_gdn_tile(48) == EINVAL
    finally:
        L.rgbd_debug_force_gdn_tile(0)


def test_gdn_bad_arguments_write_nothing():
    L = _lib()
    shape = (1, 20, 3, 5)
    x, res, beta, gamma, _ = _case(shape)
    n, c, h, w = shape
    xd, rd = x.cuda(), res.cuda()
    y = torch.full((x.numel() + GUARD,), SENTINEL, device="cuda")
    b, g = _f32p(beta.numpy()), _f32p(gamma.numpy())
    big = np.zeros(513 * 513, dtype=np.float32)
    bad = [
        (None, n, c, h, w, b, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, c, h, w, None, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, c, h, w, b, None, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, c, h, w, b, g, 0, rd.data_ptr(), None),
        (xd.data_ptr(), n, 0, h, w, b, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, -16, h, w, b, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, 513, 1, 1, _f32p(big), _f32p(big), 0, None, y.data_ptr()),
        (xd.data_ptr(), 0, c, h, w, b, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, c, 0, w, b, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, c, h, -1, b, g, 0, rd.data_ptr(), y.data_ptr()),
        (xd.data_ptr(), n, c, h, w, b, g, 2, rd.data_ptr(), y.data_ptr()),
    ]
    for args in bad:
        assert L.rgbd_gdn_nchw(*args, _stream()) == EINVAL, args[1:5]
        torch.cuda.synchronize()
        assert (y == SENTINEL).all(), "a rejected call wrote to the destination"
    # ... and the same buffers are fine with good arguments
    assert L.rgbd_gdn_nchw(xd.data_ptr(), n, c, h, w, b, g, 0, rd.data_ptr(), y.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert (y[:x.numel()] != SENTINEL).all() and (y[x.numel():] == SENTINEL).all()


# ================================================================================================ the engine's layout
_DEV = {}


def _dev(cid):
    """(case, device operands): x / res in their strided buffers, beta / gamma as rgbd_gdn_pack lays them out"""
    if cid not in _DEV:
        L = _lib()
        k = gc.build(cid)
        cs = k["cs"]
        hb, hg = np.empty(cs, np.float32), np.empty(cs * cs, np.float32)
        assert L.rgbd_gdn_pack(_f32p(k["beta"]), _f32p(k["gamma"]), k["c"], _f32p(hb), _f32p(hg)) == 0
        _DEV[cid] = (k, {"x": torch.tensor(k["xbuf"]).cuda(), "res": torch.tensor(k["rbuf"]).cuda(),
                         "beta": torch.from_numpy(hb).cuda(), "gamma": torch.from_numpy(hg).cuda()})
    return _DEV[cid]


def _new_y(k):
    return torch.full(((k["npix"] + gc.TAIL) * k["ycs"],), float(gc.SENTINEL), device="cuda")


def _nhwc(L, k, d, inverse, with_res):
    """One rgbd_gdn_nhwc call into a fresh destination (with its guard band); returns it, on the device."""
    y = _new_y(k)
    rc = L.rgbd_gdn_nhwc(d["x"].data_ptr(), k["xcs"], k["npix"], k["cs"], d["beta"].data_ptr(), d["gamma"].data_ptr(), inverse,
                         d["res"].data_ptr() if with_res else None, k["rcs"] if with_res else 0, y.data_ptr(), k["ycs"], _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return y


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


CASE_IDS = [c["id"] for c in gc.CASES]


@pytest.mark.parametrize("cid", CASE_IDS)
def test_gdn_nhwc_vs_f64(cid):
    """Every case, GDN / IGDN, with / without the residual, at the tile the launcher chooses: gdn_cases.accept."""
    L = _lib()
    k, d = _dev(cid)
    assert L.rgbd_debug_force_gdn_tile(0) == 0
    worst, fails = {}, {}
    for inverse, with_res in gc.COMBOS:
        stats = {}
        f = gc.accept(k, _nhwc(L, k, d, inverse, with_res).cpu().numpy(), inverse, with_res, stats)
        worst[(inverse, with_res)] = round(stats["worst"], 3)
        if f:
            fails[(inverse, with_res)] = f
    print(f"gdn nhwc {cid}: worst |err| / bound per (inverse, res) = {worst}")
    assert not fails, fails


@pytest.mark.parametrize("cid", CASE_IDS)
def test_gdn_nhwc_same_bits_for_every_tile(cid):
    """Base: the forced 16-pixel tile (four waves share the output tiles).  A second call, the forced 32- and 64-pixel tiles
    (one wave walks all output tiles, in passes of 12; 64 pixels at cs = 512 is the largest LDS the launch may ask for) and the
    automatic choice give the same bits over the whole buffer, sentinels included."""
    L = _lib()
    k, d = _dev(cid)
    try:
        for inverse, with_res in gc.COMBOS:
            assert L.rgbd_debug_force_gdn_tile(16) == 0
            base = _nhwc(L, k, d, inverse, with_res)
            assert _same_bits(base, _nhwc(L, k, d, inverse, with_res)), "two calls differ"
            for tile in (32, 64, 0):
                assert L.rgbd_debug_force_gdn_tile(tile) == 0
                assert _same_bits(base, _nhwc(L, k, d, inverse, with_res)), f"tile {tile} (0 = automatic) differs from tile 16"
    finally:
        L.rgbd_debug_force_gdn_tile(0)


@pytest.mark.parametrize("cid", [c["id"] for c in gc.CASES if c["group"] != "stride"])
def test_gdn_nhwc_dense_equals_the_public_operator(cid):
    """All three strides = cs: the same bits as rgbd_gdn_nchw on the same data (which packs, lays out and launches itself)."""
    L = _lib()
    k, d = _dev(cid)
    c, npix = k["c"], k["npix"]
    assert k["xcs"] == k["ycs"] == k["rcs"] == k["cs"]
    assert L.rgbd_debug_force_gdn_tile(0) == 0
    x = torch.tensor(k["x"]).t().contiguous().reshape(1, c, 1, npix)
    res = torch.tensor(k["res"]).t().contiguous().reshape(1, c, 1, npix)
    for inverse, with_res in gc.COMBOS:
        y = _nhwc(L, k, d, inverse, with_res).view(npix + gc.TAIL, k["ycs"])[:npix, :c]
        pub = _run(L, x, torch.tensor(k["beta"]), torch.tensor(k["gamma"]), inverse, res if with_res else None)
        assert (pub[c * npix:] == SENTINEL).all()
        assert _same_bits(y.cpu().t().contiguous(), pub[:c * npix].view(c, npix)), (inverse, with_res)


@pytest.mark.parametrize("cid", [c["id"] for c in gc.CASES if c["group"] == "stride"])
def test_gdn_nhwc_strided_equals_dense(cid):
    """A stride larger than cs moves the rows and nothing else: channels [0, cs) equal the dense form's, bit for bit."""
    L = _lib()
    k, d = _dev(cid)
    kd, dd = _dev(gc.dense_id(k))
    npix, cs = k["npix"], k["cs"]
    assert L.rgbd_debug_force_gdn_tile(0) == 0
    for inverse, with_res in gc.COMBOS:
        y = _nhwc(L, k, d, inverse, with_res).view(npix + gc.TAIL, k["ycs"])
        dense = _nhwc(L, kd, dd, inverse, with_res).view(npix + gc.TAIL, cs)
        assert _same_bits(y[:npix, :cs].contiguous(), dense[:npix].contiguous()), (inverse, with_res)
        assert (y[:npix, cs:] == float(gc.SENTINEL)).all() and (y[npix:] == float(gc.SENTINEL)).all()


def test_gdn_nhwc_bad_arguments_write_nothing():
    """launch_gdn's own check, reached through the hook: -22, nothing launched, and the same buffers work afterwards."""
    L = _lib()
    k, d = _dev("stride-c200-n37-s16.4.36")
    cs = k["cs"]
    y = _new_y(k)
    good = dict(x=d["x"].data_ptr(), xcs=k["xcs"], npix=k["npix"], cs=cs, beta=d["beta"].data_ptr(), gamma=d["gamma"].data_ptr(),
                inverse=0, res=d["res"].data_ptr(), rcs=k["rcs"], y=y.data_ptr(), ycs=k["ycs"])
    bad = [("cs % 16", dict(cs=cs - 8)), ("cs > 512", dict(cs=528, xcs=528, ycs=528, rcs=528)), ("cs = 0", dict(cs=0)),
           ("npix = 0", dict(npix=0)), ("npix < 0", dict(npix=-1))]
    for s in ("xcs", "ycs", "rcs"):
        bad += [(f"{s} < cs", {s: cs - 4}), (f"{s} % 4", {s: good[s] + 2})]
    for p in ("x", "y", "res", "beta", "gamma"):
        bad.append((f"{p} + 4 bytes", {p: good[p] + 4}))
    for p in ("x", "y", "beta", "gamma"):
        bad.append((f"{p} NULL", {p: None}))

    def call(a):
        return L.rgbd_gdn_nhwc(a["x"], a["xcs"], a["npix"], a["cs"], a["beta"], a["gamma"], a["inverse"], a["res"], a["rcs"], a["y"],
                               a["ycs"], _stream())

    for what, change in bad:
        assert call({**good, **change}) == EINVAL, what
        torch.cuda.synchronize()
        assert (y == float(gc.SENTINEL)).all(), f"the call refused for '{what}' wrote to the destination"
    # ... and the same buffers are fine with good arguments
    assert call(good) == 0
    torch.cuda.synchronize()
    assert not gc.accept(k, y.cpu().numpy(), 0, 1)
