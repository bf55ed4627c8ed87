"""The MS-SSIM kernels of csrc/metrics.hip ALONE -- msssim_scale_kernel, msssim_finish_kernel, avgpool2_kernel and the host walk
over the five scales -- through the C ABI's rgbd_msssim_stats, whose out[P][5][2] (mean SSIM and mean CS of every plane at every
scale) is judged statistic by statistic against the fp64 statement of the definition, at the cases of tests/msssim_cases.py and
through ITS acceptance function:

    |out - ref64| <= 4 * max(E32, 8 * 2^-24 * max(1, |ref64|))   per (case, scale, statistic); E32: the fp32 CPU restatement's
                                                                  own distance on the same inputs, fixed before any kernel runs

tests/test_msssim_cases.py shows (without a GPU) that this function rejects every wrong restatement listed there: a dropped
pixel at a tile corner, a tile's last row or column, the wrong count, divisor, pad, constants, range, clamp, plane, slot, scale.
Also here: the workspace promise and the guards round `out`, same bits (again, on a side stream, one plane alone), the Python
wrapper's layout handling and fold, and the refusals (host-side, before any launch).

Measured on an MI355X (gfx950): the table in tests/msssim_cases.py; the tests print every case's figures before they assert.
"""
import ctypes

import numpy as np
import pytest
import torch

import msssim_cases as mc
from gpu_utils import require_gpu
from oracle import msssim_ref

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC = -22, -28
GUARD = 4096            # bytes in front of and behind the workspace and `out`
WS_FILL = 0xA5
SENT = np.float32(-777.25)
f32p = ctypes.POINTER(ctypes.c_float)


def _lib():
    from rgbd_amd._lib import lib

    return lib()


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off)


class Guarded:
    """`out` [P][5][2] and a workspace of exactly the documented size, each with GUARD sentinel bytes on both sides"""

    def __init__(self, P, H, W, ws_bytes=None):
        self.P = P
        self.nbytes = int(_lib().rgbd_msssim_workspace_bytes(P, H, W)) if ws_bytes is None else ws_bytes
        self.ws = torch.full((self.nbytes + 2 * GUARD,), WS_FILL, dtype=torch.uint8).cuda()
        self.out = torch.full((P * 10 + 2 * (GUARD // 4),), float(SENT)).cuda()

    def ws_ptr(self):
        return _p(self.ws, GUARD)

    def out_ptr(self):
        return _p(self.out, GUARD)

    def guards_intact(self):
        ws, out = self.ws.cpu().numpy(), self.out.cpu().numpy()
        g = GUARD // 4
        return bool((ws[:GUARD] == WS_FILL).all() and (ws[GUARD + self.nbytes:] == WS_FILL).all() and
                    (out[:g] == SENT).all() and (out[g + self.P * 10:] == SENT).all())

    def untouched(self):
        return bool((self.ws.cpu().numpy() == WS_FILL).all() and (self.out.cpu().numpy() == SENT).all())

    def get(self):
        g = GUARD // 4
        return self.out.cpu().numpy()[g:g + self.P * 10].reshape(self.P, 5, 2).copy()


def run(c, planes=slice(None), stream=None):
    """rgbd_msssim_stats on the case's planes -> out [P][5][2] fp32 (numpy); the guards are checked on every call"""
    x, y = _dev(c["x"][planes]), _dev(c["y"][planes])
    P, H, W = x.shape
    buf = Guarded(P, H, W)
    assert buf.nbytes > 0
    taps = np.ascontiguousarray(c["taps"], np.float32)
    torch.cuda.synchronize()  # (the inputs are there, whichever stream runs the call)
    st = torch.cuda.current_stream() if stream is None else stream
    rv = _lib().rgbd_msssim_stats(_p(x), _p(y), P, H, W, taps.ctypes.data_as(f32p), float(c["data_range"]), int(c["clamp01"]),
                                  buf.out_ptr(), buf.ws_ptr(), buf.nbytes, ctypes.c_void_p(st.cuda_stream))
    assert rv == 0, rv
    st.synchronize()
    torch.cuda.synchronize()  # (raises if a kernel failed)
    assert buf.guards_intact(), "a kernel wrote outside the documented workspace or outside out[P][5][2]"
    return buf.get()


_FIRST = {}


def first(cid):
    """the case's first run, shared by the tests that compare against it"""
    if cid not in _FIRST:
        _FIRST[cid] = run(mc.build(cid))
    return _FIRST[cid]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ the statistics
@pytest.mark.parametrize("cid", mc.IDS)
def test_statistics_per_plane_and_scale(cid):
    require_gpu()
    c = mc.build(cid)
    got = first(cid)
    stats = {}
    fails = mc.accept(c, got, stats)
    print(f"{cid}: kernel ratio {stats['ratio']:.3f} (allowed 4), E32 {stats['E32']:.3g}; per scale (ssim, cs): " +
          " ".join(f"{a:.2f},{b:.2f}" for a, b in stats["per_scale"]) +
          f"; {int((got.view(np.uint32) == c['emu'].view(np.uint32)).sum())} of {got.size} values are the restatement's bits")
    assert not fails, fails


@pytest.mark.parametrize("cid", ["one_over", "planes65"])
def test_workspace_promise_and_guards(cid):
    """the walk stays inside rgbd_msssim_workspace_bytes (handed over as the size, 4 KiB of sentinels on both sides) and `out` is
    written in [P][5][2] only; every statistic was written (no sentinel left inside)"""
    require_gpu()
    got = first(cid)  # (run() asserts the guards)
    assert np.isfinite(got).all() and not (got == SENT).any()
    c = mc.build(cid)
    # the documented size is the walk's: partial sums of every scale and the two pooled images of the next
    floats, hs, ws = 0, mc.sides(c["H"]), mc.sides(c["W"])
    for s in range(5):
        floats += c["P"] * (-(-(hs[s] - 10) // mc.TH)) * (-(-(ws[s] - 10) // mc.TW)) * 2
        if s < 4:
            floats += 2 * c["P"] * hs[s + 1] * ws[s + 1]
    assert int(_lib().rgbd_msssim_workspace_bytes(c["P"], c["H"], c["W"])) == 4 * floats + 256


# ------------------------------------------------------------------------------------------------ same bits
def test_same_bits_again_on_a_side_stream_and_alone():
    require_gpu()
    c = mc.build("one_over")
    got = first("one_over")
    assert same_bits(run(c), got), "a second call differs"
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    assert same_bits(run(c, stream=side), got), "the call on a side stream differs"
    for p in range(c["P"]):
        assert same_bits(run(c, planes=slice(p, p + 1)), got[p:p + 1]), f"plane {p} alone differs from plane {p} in the batch"


def test_second_finish_block_is_the_first():
    """planes 64 and 0 ... 63 of the 65-plane call against the same planes run as their own calls"""
    require_gpu()
    c = mc.build("planes65")
    got = first("planes65")
    assert same_bits(run(c, planes=slice(64, 65)), got[64:65])
    assert same_bits(run(c, planes=slice(60, 64)), got[60:64])


# ------------------------------------------------------------------------------------------------ the Python wrapper
def _image(fams, key, H=161, W=170):
    xs, ys = zip(*[mc.family_planes(f, (key, i), H, W) for i, f in enumerate(fams)])
    return np.stack(xs)[None], np.stack(ys)[None]  # [1][C][H][W]


def test_wrapper_layouts_and_fold():
    require_gpu()
    from rgbd_amd import metrics

    xa, ya = _image("ade", "fold")   # every CS positive: the one input whose fold is not 0 by relu
    xc, yc = _image("ccc", "fold")   # every CS negative
    x, y = _dev(np.concatenate([xa, xc])), _dev(np.concatenate([ya, yc]))
    got = metrics.ms_ssim_gpu(x, y)
    torch.cuda.synchronize()
    # layouts: a non-contiguous view and fp64 tensors give the contiguous fp32 call's bits
    wide_x, wide_y = torch.zeros(2, 3, 161, 180, device="cuda"), torch.zeros(2, 3, 161, 180, device="cuda")
    wide_x[..., 5:175], wide_y[..., 5:175] = x, y
    vx, vy = wide_x[..., 5:175], wide_y[..., 5:175]
    assert not vx.is_contiguous()
    assert torch.equal(metrics.ms_ssim_gpu(vx, vy), got)
    assert torch.equal(metrics.ms_ssim_gpu(x.double(), y.double()), got)
    assert torch.equal(metrics.ms_ssim_gpu(x.transpose(2, 3).contiguous().transpose(2, 3), y), got)
    # the fold: out -> relu, weights, product over the scales, mean over the channels (metrics.py)
    c = {"x": np.concatenate([xa[0], xc[0]]), "y": np.concatenate([ya[0], yc[0]]), "taps": mc.taps32(), "data_range": 1.0, "clamp01": 0}
    out = run(c).reshape(2, 3, 5, 2)
    assert (out[0, :, :4, 1] > 0).all() and (out[0, :, 4, 0] > 0).all() and (out[1, :, :4, 1] < 0).all()
    o = torch.from_numpy(out).cuda()
    w = torch.tensor(metrics._MS_WEIGHTS, device="cuda")
    vals = torch.cat([torch.relu(o[:, :, :4, 1]), torch.relu(o[:, :, 4:, 0])], dim=2)
    assert torch.equal(torch.prod(vals ** w, dim=2).mean(dim=1), got)  # the same statistics, the same fold: the same bits
    want = msssim_ref.combine(out.astype(np.float64))
    g = got.cpu().numpy()
    print("wrapper:", g, "fp64 fold of out:", want)
    # five fp32 powers (a few ulp each), four products, two sums and a division of values <= 1: well inside 32 * 2^-24
    assert abs(float(g[0]) - want[0]) <= 32 * mc.EPS24 and 0.1 < want[0] < 1.0
    assert g[1] == 0.0 and want[1] == 0.0  # exactly: family c through relu
    assert float(metrics.ms_ssim_gpu(_dev(xc), _dev(yc))[0]) == 0.0


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_on_the_host():
    """every bad argument is refused before any launch: the sentinel-filled `out` and workspace stay as they were.  (Nothing here
    reaches a kernel: P = 65536 is passed as a number only, next to buffers for three planes.)"""
    require_gpu()
    L = _lib()
    c = mc.build("min_odd")
    x, y = _dev(c["x"]), _dev(c["y"])
    P, H, W = x.shape
    taps = np.ascontiguousarray(c["taps"], np.float32)
    buf = Guarded(P, H, W)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(x=_p(x), y=_p(y), P=P, H=H, W=W, taps=taps.ctypes.data_as(f32p), dr=1.0, cl=1, out=buf.out_ptr(), ws=buf.ws_ptr(),
                n=buf.nbytes, st=st)
    bad = [("x", None, EINVAL), ("y", None, EINVAL), ("taps", None, EINVAL), ("out", None, EINVAL), ("ws", None, EINVAL),
           ("P", 0, EINVAL), ("P", 65536, EINVAL), ("H", 160, EINVAL), ("W", 160, EINVAL), ("n", buf.nbytes - 1, ENOSPC)]
    for k, v, want in bad:
        a = dict(good)
        a[k] = v
        rv = L.rgbd_msssim_stats(*a.values())
        torch.cuda.synchronize()
        assert rv == want, (k, v, rv)
        assert buf.untouched(), (k, v, "a refused call wrote")
    for P_, H_, W_ in ((0, 161, 161), (3, 160, 161), (3, 161, 160)):
        assert int(L.rgbd_msssim_workspace_bytes(P_, H_, W_)) == -1
    assert int(L.rgbd_msssim_workspace_bytes(3, 161, 161)) == buf.nbytes > 0
    # and the good call on the same buffers goes through
    assert L.rgbd_msssim_stats(*good.values()) == 0
    torch.cuda.synchronize()
    assert buf.guards_intact() and same_bits(buf.get(), first("min_odd"))
