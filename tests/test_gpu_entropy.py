"""The entropy stage's engine-layout kernels of csrc/entropy.hip ALONE -- ckbd_estimate_kernel, slice_estimate_kernel,
eb_forward_kernel (the numbers eval-mode forward() reports as rate), ckbd_part_kernel<0 / 1 / 2>, z_quant_kernel and
z_dequant_kernel -- through the C ABI's rgbd_ckbd_estimate_part / rgbd_slice_estimate / rgbd_eb_forward / rgbd_ckbd_part /
rgbd_z_quant / rgbd_z_dequant, at the cases of tests/entropy_cases.py and through ITS acceptance functions:

  exact           y_hat / z_hat, symbols, indexes, every sentinel a kernel must not touch, pad channels (0)
  Gaussian        |lik - lik64| <= 4 k0 E where lik64 >= 2e-9 (E: the fp32 rounding envelope, k0: what the fp32 torch
                  restatement needs on the same inputs); exactly 1e-9f where lik64 < 0.5e-9
  factorised      per decade of lik64, worst relative error <= 4 x the fp32 torch restatement's (never below 4 * 8 * 2^-24)

tests/test_entropy_cases.py shows (without a GPU) that these functions reject every wrong restatement listed there.

Measured on an MI355X (gfx950): see MEASURED below; the test prints the figures of every case before it asserts.
"""
import ctypes

import numpy as np
import pytest
import torch

import entropy_cases as ec
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

# The kernels' own figures on an MI355X (printed by the tests; DESIGN.md 4a repeats them):
MEASURED = """
Gaussian likelihood, k = max |lik - lik64| / E over the judged positions (kernel / fp32 torch restatement k0 / allowed 4 k0):
  ckbd_estimate_kernel   c16 1.578 / 1.578 / 6.31   c16p 1.838 / 1.512 / 6.05   c32 1.935 / 1.550 / 6.20
                         c32p 2.252 / 1.735 / 6.94  grid (1 310 720 positions) 3.002 / 2.090 / 8.36
  slice_estimate_kernel  c16 1.642 / 1.642 / 6.57   c32 1.980 / 1.652 / 6.61    c20 1.500 / 1.643 / 6.57
                         grid (655 360 positions) 2.799 / 1.983 / 7.93
Factorised prior, worst relative error over the decades of lik64 in [1e-9, 1) (kernel / fp32 torch restatement):
  c24 1.2e-5 / 1.6e-5   c24p 1.6e-5 / 1.3e-5   c24p_init 1.6e-5 / 1.6e-5   c192 1.7e-5 / 1.3e-5   c192p 2.0e-5 / 2.0e-5;
  the largest per-decade ratio kernel : restatement is 1.9 (c24, decade 1e-6: 6.0e-6 against 3.1e-6), allowed 4.
Everything exact (y_hat, z_hat, symbols, indexes, sentinels, pad channels, second call, one image alone) was equal.
"""

EINVAL = -22
f32p = ctypes.POINTER(ctypes.c_float)
TAIL = 64  # guard elements behind every output buffer


def _lib():
    from rgbd_amd._lib import lib

    return lib()


def _check(rv, what):
    from rgbd_amd._lib import check

    check(rv, what)


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Out:
    """an output buffer filled with a sentinel, with TAIL guard elements behind it"""

    def __init__(self, shape, fill, dtype=torch.float32):
        self.n = int(np.prod(shape))
        self.shape, self.fill = tuple(shape), fill
        self.t = torch.full((self.n + TAIL,), float(fill) if dtype == torch.float32 else int(fill), dtype=dtype).cuda()

    def ptr(self):
        return _p(self.t)

    def get(self):
        a = self.t.cpu().numpy()
        assert (a[self.n:] == self.fill).all(), "a kernel wrote behind its output buffer"
        return a[:self.n].reshape(self.shape).copy()


# ------------------------------------------------------------------------------------------------ runners
def run_ckbd_est(c, sl=slice(None)):
    L = _lib()
    y, prm = _dev(c["buf_y"][sl]), _dev(c["buf_params"][sl])
    B, h, w, C = y.shape[0], c["h"], c["w"], c["C"]
    yh, lk = Out((B, h, w, c["yhcs"]), ec.SENT), Out((B, h, w, c["lcs"]), ec.SENT)
    res = {}
    for anchor in (1, 0):
        _check(L.rgbd_ckbd_estimate_part(_p(y), c["ycs"], _p(prm), c["pcs"], yh.ptr(), c["yhcs"], lk.ptr(), c["lcs"], B, h, w, C, anchor,
                                         c["perm"], _stream()), "ckbd_estimate_part")
        torch.cuda.synchronize()
        if anchor:
            res["yhat_a"], res["lik_a"] = yh.get(), lk.get()
    res["yhat"], res["lik"] = yh.get(), lk.get()
    return res


def run_slice_est(c, sl=slice(None)):
    y, mu, sg = _dev(c["buf_y"][sl]), _dev(c["buf_mean"][sl]), _dev(c["buf_scale"][sl])
    B, h, w, C = y.shape[0], c["h"], c["w"], c["C"]
    lk, d0 = Out((B, h, w, c["lcs"]), ec.SENT), Out((B, h, w, c["cs0"]), ec.SENT)
    d1 = Out((B, h, w, c["cs1"]), ec.SENT) if c["two"] else None
    _check(_lib().rgbd_slice_estimate(_p(y), c["ycs"], _p(mu), c["mcs"], _p(sg), c["scs"], B, C, h, w, lk.ptr(), c["lcs"], d0.ptr(),
                                      c["cs0"], d1.ptr() if d1 else None, c["cs1"] if d1 else 0, _stream()), "slice_estimate")
    torch.cuda.synchronize()
    res = {"lik": lk.get(), "d0": d0.get()}
    if d1:
        res["d1"] = d1.get()
    return res


def _host_ptrs(prm, name, n):
    keep = [np.ascontiguousarray(prm[f"{name}{i}"], np.float32) for i in range(n)]
    return (f32p * n)(*[a.ctypes.data_as(f32p) for a in keep]), keep


def run_eb(c, sl=slice(None)):
    z = _dev(c["buf_z"][sl])
    B, h, w, C, zcs = z.shape[0], c["h"], c["w"], c["C"], c["zcs"]
    zh, lk = Out((B, h, w, zcs), ec.SENT), Out((B, h, w, zcs), ec.SENT)
    (pm, k0), (pb, k1), (pf, k2) = _host_ptrs(c["prm"], "_matrix", 5), _host_ptrs(c["prm"], "_bias", 5), _host_ptrs(c["prm"], "_factor", 4)
    med = np.ascontiguousarray(c["prm"]["medians"], np.float32)
    _check(_lib().rgbd_eb_forward(_p(z), zcs, B, h, w, C, pm, pb, pf, med.ctypes.data_as(f32p), zh.ptr(), lk.ptr(), c["perm"], _stream()),
           "eb_forward")
    torch.cuda.synchronize()
    del k0, k1, k2
    return {"zhat": zh.get(), "lik": lk.get()}


def run_zq(c, sl=slice(None)):
    L = _lib()
    z, med = _dev(c["buf_z"][sl]), _dev(c["med"])
    B, h, w, C, zcs = z.shape[0], c["h"], c["w"], c["C"], c["zcs"]
    n = B * C * h * w
    sym, idx = Out((n + ec.GUARD,), ec.ISENT, torch.int32), Out((n + ec.GUARD,), ec.ISENT, torch.int32)
    zh = Out((B, h, w, zcs), ec.SENT)
    _check(L.rgbd_z_quant(_p(z), zcs, B, h, w, C, _p(med), sym.ptr(), idx.ptr(), c["perm"], _stream()), "z_quant")
    _check(L.rgbd_z_dequant(sym.ptr(), B, h, w, C, _p(med), zh.ptr(), zcs, c["perm"], _stream()), "z_dequant")
    torch.cuda.synchronize()
    return {"sym": sym.get(), "idx": idx.get(), "zhat": zh.get()}


def run_ckbd_part(c, sl=slice(None), base=None, n=None):
    """mode 0 over both passes; then mode 1 (indexes alone) and mode 2 (y_hat from the symbols) into fresh buffers, which must
    repeat mode 0's bits"""
    L = _lib()
    y, prm, tab = _dev(c["buf_y"][sl]), _dev(c["buf_params"][sl]), _dev(ec.scale_table())
    B, h, w, C = y.shape[0], c["h"], c["w"], c["C"]
    base = _dev(np.asarray(c["base"] if base is None else base, np.int64))
    n = c["n"] if n is None else n
    mk = lambda: (Out((n + ec.GUARD,), ec.ISENT, torch.int32), Out((B, h, w, c["yhcs"]), ec.SENT))  # noqa: E731
    (sym, yh), (idx, yh2), (idx2, _) = mk(), mk(), mk()
    res = {}

    def call(mode, anchor, off, yhat, s, i):
        _check(L.rgbd_ckbd_part(mode, _p(y) if mode == 0 else None, c["ycs"] if mode == 0 else 0, _p(prm), c["pcs"],
                                yhat.ptr() if mode != 1 else None, c["yhcs"] if mode != 1 else 0, _p(tab) if mode != 2 else None, B, h, w, C,
                                anchor, c["per_image"], c["perm"], s.ptr() if mode != 1 else None, i.ptr() if mode != 2 else None,
                                _p(base), off, _stream()), f"ckbd_part mode {mode}")
        torch.cuda.synchronize()

    for anchor, off in zip((1, 0), c["offs"]):
        call(0, anchor, off, yh, sym, idx)
        call(1, anchor, off, None, None, idx2)
        call(2, anchor, off, yh2, sym, None)
        if anchor:
            res["yhat_a"] = yh.get()
            assert ec.bits_equal(yh2.get(), res["yhat_a"]), "decode (mode 2) differs from encode after the anchor pass"
    res.update({"sym": sym.get(), "idx": idx.get(), "yhat": yh.get()})
    assert np.array_equal(idx2.get(), res["idx"]), "index-only (mode 1) differs from encode"
    assert ec.bits_equal(yh2.get(), res["yhat"]), "decode (mode 2) differs from encode"
    return res


RUN = {"ckbd_est": run_ckbd_est, "slice_est": run_slice_est, "eb": run_eb, "zq": run_zq, "ckbd_part": run_ckbd_part}


def _cases(fam):
    return pytest.mark.parametrize("cid", ec.FAMILIES[fam][0])


def _one(fam, cid):
    require_gpu()
    _, build, _, accept = ec.FAMILIES[fam]
    c = build(cid)
    stats = {}
    fails = accept(c, RUN[fam](c), stats)
    if "k" in stats:
        print(f"{fam} {cid}: kernel k = {stats['k']:.3f}, fp32 restatement k0 = {stats['k0']:.3f}, allowed {4 * stats['k0']:.3f}")
    if "worst" in stats:
        print(f"{fam} {cid}: worst relative error per decade of lik64 from 1e-9 (kernel / fp32 restatement): " +
              " ".join(f"{a:.2g}/{b:.2g}" for a, b in zip(stats["worst"], stats["worst0"])))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ one test per kernel
@_cases("ckbd_est")
def test_ckbd_estimate_kernel(cid):
    _one("ckbd_est", cid)


@_cases("slice_est")
def test_slice_estimate_kernel(cid):
    _one("slice_est", cid)


@_cases("eb")
def test_eb_forward_kernel(cid):
    _one("eb", cid)


@_cases("zq")
def test_z_quant_dequant_kernels(cid):
    _one("zq", cid)


@_cases("ckbd_part")
def test_ckbd_part_kernel(cid):
    _one("ckbd_part", cid)


# ------------------------------------------------------------------------------------------------ same bits
def _same(a, b):
    return a.keys() == b.keys() and all(ec.bits_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("fam,cid", [("ckbd_est", "c32p"), ("slice_est", "c16"), ("eb", "c24p"), ("zq", "c24p"), ("ckbd_part", "c16p_img"),
                                     ("ckbd_part", "c32p")])
def test_same_bits_again_and_for_one_image(fam, cid):
    """a second call repeats the first bit for bit, and image 1 run alone (B = 1) gives what it gives inside the batch"""
    require_gpu()
    c = ec.FAMILIES[fam][1](cid)
    first = RUN[fam](c)
    assert _same(first, RUN[fam](c))
    one = slice(1, 2)
    if fam in ("ckbd_est", "slice_est", "eb"):
        alone = RUN[fam](c, one)
        assert all(ec.bits_equal(alone[k], first[k][one]) for k in first)
    elif fam == "zq":
        alone = run_zq(c, one)
        n1 = c["C"] * c["h"] * c["w"]
        assert ec.bits_equal(alone["zhat"], first["zhat"][one])
        assert np.array_equal(alone["sym"][:n1], first["sym"][n1:2 * n1]) and np.array_equal(alone["idx"][:n1], first["idx"][n1:2 * n1])
    else:
        B, h, w2, C = c["B"], c["h"], c["w"] // 2, c["C"]
        base1 = [int(c["base"][1])] if c["per_image"] else [3]
        n1 = base1[0] + c["offs"][1] + C * h * w2
        alone = run_ckbd_part(c, one, base=base1, n=n1)
        assert ec.bits_equal(alone["yhat"], first["yhat"][one]) and ec.bits_equal(alone["yhat_a"], first["yhat_a"][one])
        for off in c["offs"]:
            p1 = ec.part_positions(1, C, h, w2, c["per_image"], base1, off)
            pb = ec.part_positions(B, C, h, w2, c["per_image"], c["base"], off)[one]
            assert np.array_equal(alone["sym"][p1], first["sym"][pb]) and np.array_equal(alone["idx"][p1], first["idx"][pb])


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused_on_the_host():
    """every bad argument returns -22 before any launch: the sentinel-filled outputs stay as they were.  (The extents that
    would overrun the buffers below are exactly the ones refused; nothing here reaches a kernel.)"""
    require_gpu()
    L = _lib()
    B, h, w, C = 2, 3, 6, 16
    big = 1 << 15
    f = lambda *s: Out(s, ec.SENT)  # noqa: E731
    i = lambda n: Out((n,), ec.ISENT, torch.int32)  # noqa: E731
    src = torch.zeros(B * h * w * 64).cuda()
    outs = []

    def refused(fn, good, bad_sets, out_bufs):
        outs.extend(out_bufs)
        for k, v in bad_sets:
            a = dict(good)
            a.update(dict(zip(k, v)) if isinstance(k, tuple) else {k: v})
            rv = fn(*a.values())
            assert rv == EINVAL, (fn.__name__, k, v, rv)
        torch.cuda.synchronize()
        for o in out_bufs:
            assert (o.t.cpu().numpy() == o.fill).all(), (fn.__name__, "a refused call wrote")

    geom_bad = [("B", 0), ("h", 0), ("w", -2), ("C", 0), ("B", -1), (("B", "h", "w"), (big, 256, 256)), (("B", "h", "w", "C"), (big, big, big, big))]
    st = _stream()
    # checkerboard estimate
    yh, lk = f(B, h, w, 40), f(B, h, w, 32)
    good = dict(y=_p(src), ycs=48, p=_p(src), pcs=40, yh=yh.ptr(), yhcs=40, lk=lk.ptr(), lcs=32, B=B, h=h, w=w, C=C, anchor=1, perm=0, st=st)
    refused(L.rgbd_ckbd_estimate_part, good, [("y", None), ("p", None), ("yh", None), ("lk", None), ("ycs", C - 1), ("pcs", 2 * C - 1),
                                              ("yhcs", C - 1), ("lcs", C - 1), ("w", 5), (("C", "perm"), (24, 1)),
                                              (("C", "perm", "pcs"), (8, 1, 40))] + geom_bad, [yh, lk])
    # slice estimate
    lk, d0, d1 = f(B, h, w, 32), f(B, h, w, 40), f(B, h, w, 40)
    good = dict(y=_p(src), ycs=48, m=_p(src), mcs=40, s=_p(src), scs=32, B=B, C=C, h=h, w=w, lk=lk.ptr(), lcs=32, d0=d0.ptr(), cs0=40,
                d1=d1.ptr(), cs1=40, st=st)
    refused(L.rgbd_slice_estimate, good, [("y", None), ("m", None), ("s", None), ("lk", None), ("d0", None), ("ycs", C - 1), ("mcs", C - 1),
                                          ("scs", C - 1), ("lcs", C - 1), ("cs0", C - 1), ("cs1", C - 1)] + geom_bad, [lk, d0, d1])
    # checkerboard part
    yh, sym, idx = f(B, h, w, 40), i(4096), i(4096)
    base = torch.zeros(B, dtype=torch.int64).cuda()
    tab = _dev(ec.scale_table())
    good = dict(mode=0, y=_p(src), ycs=48, p=_p(src), pcs=40, yh=yh.ptr(), yhcs=40, tab=_p(tab), B=B, h=h, w=w, C=C, anchor=1, per_image=1,
                perm=0, sym=sym.ptr(), idx=idx.ptr(), base=_p(base), off=0, st=st)
    bad = [("mode", 3), ("mode", -1), ("y", None), ("p", None), ("yh", None), ("tab", None), ("sym", None), ("idx", None), ("base", None),
           ("ycs", C - 1), ("pcs", 2 * C - 1), ("yhcs", C - 1), ("w", 5), ("off", -1), (("C", "perm"), (24, 1)),
           (("mode", "idx"), (1, None)), (("mode", "tab"), (1, None)), (("mode", "sym"), (2, None)), (("mode", "yh"), (2, None)),
           (("mode", "yhcs"), (2, C - 1))] + geom_bad
    refused(L.rgbd_ckbd_part, good, bad, [yh, sym, idx])
    # z path
    zh, sym, idx = f(B, h, w, 32), i(4096), i(4096)
    med = torch.zeros(64).cuda()
    good = dict(z=_p(src), zcs=32, B=B, h=h, w=w, C=24, med=_p(med), sym=sym.ptr(), idx=idx.ptr(), perm=1, st=st)
    refused(L.rgbd_z_quant, good, [("z", None), ("med", None), ("sym", None), ("idx", None), ("zcs", 23), (("zcs", "perm"), (24, 1))] + geom_bad,
            [sym, idx])
    good = dict(sym=sym.ptr(), B=B, h=h, w=w, C=24, med=_p(med), zh=zh.ptr(), zcs=32, perm=1, st=st)
    refused(L.rgbd_z_dequant, good, [("sym", None), ("med", None), ("zh", None), ("zcs", 23), (("zcs", "perm"), (24, 1))] + geom_bad, [zh])
    # factorised prior
    prm = ec.eb_params("refusal", 24, 1)
    (pm, k0), (pb, k1), (pf, k2) = _host_ptrs(prm, "_matrix", 5), _host_ptrs(prm, "_bias", 5), _host_ptrs(prm, "_factor", 4)
    hole = (f32p * 5)(*[pm[j] if j != 2 else None for j in range(5)])
    hmed = np.ascontiguousarray(prm["medians"])
    zh, lk = f(B, h, w, 32), f(B, h, w, 32)
    good = dict(z=_p(src), zcs=32, B=B, h=h, w=w, C=24, pm=pm, pb=pb, pf=pf, med=hmed.ctypes.data_as(f32p), zh=zh.ptr(), lk=lk.ptr(), perm=1, st=st)
    refused(L.rgbd_eb_forward, good, [("z", None), ("pm", None), ("pb", None), ("pf", None), ("med", None), ("zh", None), ("lk", None),
                                      ("pm", hole), ("zcs", 23), (("zcs", "perm"), (24, 1))] + geom_bad, [zh, lk])
    del k0, k1, k2
