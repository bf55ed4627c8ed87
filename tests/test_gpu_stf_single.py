"""The single-modal STF (rgbd_amd.stf; reference models/stf.py) on the GPU: the layered contract of tests/test_gpu_stf.py
with that file's tolerances, against the CPU restatement (tests/stf_single_ref.py) and the reference's fixtures
(tests/golden/stf1_*.npz).

Against the reference's fixtures, stream identity, |d stream bytes| and |dPSNR| are MEASURED on the MI355X and kept in
tests/golden/stf1_floors.json (RGBD_RECORD_STF1_FLOORS=<path> makes test_layered_contract dump what it measures; the
committed file is that dump): identity is asserted where it was observed, otherwise the measured byte difference is the
ceiling and twice the measured dPSNR; |dPSNR| <= 1e-4 dB holds regardless unless the entry names a cause.  The STF family
keeps the single-chain arithmetic, so bit identity with the reference's streams is reported, not required.
"""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

import gridcap_cases as gc
import stf_single_ref as ref
from gpu_utils import require_gpu
from oracle import coder
from oracle import elic_oracle as eo

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["a_128x192", "b_256x256", "c_b2_192x128"]
_NETS, _REFS = {}, {}


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def _psnr(a, b):
    return float(-10 * np.log10(torch.mean((a - b) ** 2).item()))


def _sd(seed, channel=3):
    from rgbd_amd import synth

    return synth.synthetic_state_dict(seed, model="STF", channel=channel)


def _net(seed, channel=3):
    require_gpu()
    if (seed, channel) not in _NETS:
        import rgbd_amd

        m = rgbd_amd.modelZoo["STF"](config=rgbd_amd.model_config(), channel=channel).eval()
        m.load_state_dict(_sd(seed, channel), strict=True)
        assert m.update(force=True)
        if channel == 3:
            assert m.count_parameters() == 99855639
        _NETS[(seed, channel)] = m.to("cuda")
    return _NETS[(seed, channel)]


def _ref(seed, channel=3):
    if (seed, channel) not in _REFS:
        r = ref.StfSingleRef(_sd(seed, channel))
        assert r.update()
        _REFS[(seed, channel)] = r
    return _REFS[(seed, channel)]


def _images(B, H, W, config_id, channel=3):
    from rgbd_amd import synth

    r, d = synth.synthetic_batch(B, H, W, config_id=config_id)
    return torch.from_numpy(r if channel == 3 else d)


# ---- 1. kernels through the C ABI ------------------------------------------------------------------------------------
def _np_slice(y, mu, sg, table, B, C, h, w, per_image, image_stride, slice_off):
    """numpy statement of the slice encoder on NHWC arrays [B,h,w,C]: symbols / indexes in stream order, y_hat."""
    s = np.rint(y - mu).astype(np.int32)  # float32 difference, half to even
    k = np.searchsorted(table[:-1], np.maximum(sg, np.float32(0.11)), side="left").astype(np.int32)
    n = (B * image_stride) if per_image else (slice_off * B + B * C * h * w)
    sym, idx = np.full(n, -99, np.int32), np.full(n, -99, np.int32)
    sc, kc = s.transpose(0, 3, 1, 2), k.transpose(0, 3, 1, 2)  # (b, c, row, col)
    if per_image:
        for b in range(B):
            o = b * image_stride + slice_off
            sym[o:o + C * h * w], idx[o:o + C * h * w] = sc[b].reshape(-1), kc[b].reshape(-1)
    else:
        o = slice_off * B
        sym[o:], idx[o:] = sc.reshape(-1), kc.reshape(-1)
    return sym, idx, s.astype(np.float32) + mu


@pytest.mark.parametrize("B,C,h,w,per_image", [(1, 32, 5, 7, 0), (3, 32, 3, 5, 0), (3, 32, 3, 5, 1), (2, 20, 9, 3, 1)])
def test_slice_kernels_against_numpy(B, C, h, w, per_image):
    require_gpu()
    from rgbd_amd._lib import check, lib

    L = lib()
    rng = np.random.default_rng(B * 1000 + C * 10 + per_image)
    ycs, mcs, scs, cs0, cs1 = C + 16, C + 5, C, C + 32, C + 3  # odd channel strides
    table = eo.scale_table().numpy().astype(np.float32)
    # values on a 1/4 grid: y - mean is exact and hits .5 ties (both parities); scales across the table incl. <= 0.11
    mu = (rng.integers(-40, 40, (B, h, w, C)) / 4).astype(np.float32)
    y = mu + (rng.integers(-26, 26, (B, h, w, C)) / 4).astype(np.float32)
    sg = np.exp(rng.uniform(np.log(0.05), np.log(300.0), (B, h, w, C))).astype(np.float32)
    sg.reshape(-1)[:64] = table  # exact table entries: the boundary of build_indexes
    assert np.any(np.abs((y - mu) % 1.0 - 0.5) == 0)

    def dev(a, cs):
        t = torch.full(a.shape[:3] + (cs,), 7.0)
        t[..., :C] = torch.from_numpy(a)
        return t.cuda()

    dy, dmu, dsg = dev(y, ycs), dev(mu, mcs), dev(sg, scs)
    slice_off = 3 * C * h * w
    image_stride = 12 * C * h * w + 11
    n = B * image_stride if per_image else slice_off * B + B * C * h * w
    rsym, ridx, ryh = _np_slice(y, mu, sg, table, B, C, h, w, per_image, image_stride, slice_off)
    dsym = torch.full((n + 1,), -99, dtype=torch.int32).cuda()
    didx = torch.full((n + 1,), -99, dtype=torch.int32).cuda()
    o0, o1 = torch.full((B, h, w, cs0), 7.0).cuda(), torch.full((B, h, w, cs1), 7.0).cuda()
    st = torch.cuda.current_stream().cuda_stream
    tb = table.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    check(L.rgbd_slice_quant_index(dy.data_ptr(), ycs, dmu.data_ptr(), mcs, dsg.data_ptr(), scs, B, C, h, w, per_image,
                                   image_stride, slice_off, tb, dsym.data_ptr(), didx.data_ptr(), o0.data_ptr(), cs0,
                                   o1.data_ptr(), cs1, st), "slice_quant_index")
    torch.cuda.synchronize()
    assert np.array_equal(dsym.cpu().numpy()[:n], rsym) and np.array_equal(didx.cpu().numpy()[:n], ridx)
    assert int(dsym[n]) == -99 and int(didx[n]) == -99
    assert np.array_equal(o0.cpu().numpy()[..., :C], ryh) and np.array_equal(o1.cpu().numpy()[..., :C], ryh)
    assert (o0[..., C:] == 7.0).all() and (o1[..., C:] == 7.0).all()  # nothing outside the slice is touched
    # decode route: y_hat from the symbols
    q0 = torch.full((B, h, w, cs0), 7.0).cuda()
    check(L.rgbd_slice_dequant(dsym.data_ptr(), dmu.data_ptr(), mcs, B, C, h, w, per_image, image_stride, slice_off,
                               q0.data_ptr(), cs0, None, 0, st), "slice_dequant")
    torch.cuda.synchronize()
    assert torch.equal(q0, o0)
    # LRP update: against float64, bit-equal between two calls and between the encode and decode routes, in place included
    lrp = rng.standard_normal((B, h, w, C)).astype(np.float32) * rng.choice([1e-4, 0.05, 0.6, 3.0, 30.0], (B, h, w, C)).astype(np.float32)
    dl = dev(lrp, C + 7)
    outs = []
    for src in (o0, q0):
        a, b2 = torch.full((B, h, w, cs1), 7.0).cuda(), torch.full((B, h, w, C), 7.0).cuda()
        check(L.rgbd_lrp_update(dl.data_ptr(), C + 7, src.data_ptr(), cs0, B * h * w, C, a.data_ptr(), cs1, b2.data_ptr(), C,
                                None, 0, st), "lrp_update")
        torch.cuda.synchronize()
        assert torch.equal(a[..., :C], b2) and (a[..., C:] == 7.0).all()
        outs.append(b2.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    inplace = o0.clone()
    check(L.rgbd_lrp_update(dl.data_ptr(), C + 7, inplace.data_ptr(), cs0, B * h * w, C, inplace.data_ptr(), cs0, None, 0,
                            None, 0, st), "lrp_update in place")
    torch.cuda.synchronize()
    assert np.array_equal(inplace.cpu().numpy()[..., :C], outs[0])
    want = ryh.astype(np.float64) + 0.5 * np.tanh(lrp.astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(outs[0].astype(np.float64) - want) / ulp
    print(f"lrp_update: max error {err.max():.3f} ulp of the result")
    assert err.max() <= 2.0


def test_lrp_tanh_alone_is_one_rounding():
    """y_hat = 0: the result is 0.5 * tanh(lrp) itself, over the whole range (tiny, the series / exp switch, saturation)."""
    require_gpu()
    from rgbd_amd._lib import check, lib

    x = np.concatenate([np.linspace(-12, 12, 200001), np.geomspace(1e-12, 1e-2, 4001), -np.geomspace(1e-12, 1e-2, 4001),
                        [0.0, 2.0 ** -10, np.nextafter(np.float32(2.0 ** -10), 0), 19.9, 20.1, 88.0, -88.0]]).astype(np.float32)
    n = x.shape[0]
    dl, z, out = torch.from_numpy(x).cuda(), torch.zeros(n).cuda(), torch.empty(n).cuda()
    check(lib().rgbd_lrp_update(dl.data_ptr(), 1, z.data_ptr(), 1, n, 1, out.data_ptr(), 1, None, 0, None, 0,
                                torch.cuda.current_stream().cuda_stream), "lrp_update")
    torch.cuda.synchronize()
    want = 0.5 * np.tanh(x.astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(out.cpu().numpy().astype(np.float64) - want) / ulp
    print(f"0.5 * tanh: max error {err.max():.3f} ulp")
    assert err.max() <= 1.5  # one rounding (0.5 ulp), counted double where the exact value sits just below a binade boundary


@pytest.mark.parametrize("case", gc.SLICE_CASES, ids=lambda c: "%(B)dx%(C)dx%(h)dx%(w)d-pi%(per_image)d" % c)
def test_slice_kernels_past_the_grid_cap(case):
    """slice_part_kernel<0 / 2> and lrp_update_kernel past their 2048 x 256 grid cap (tests/gridcap_cases.py: two sweeps, the
    second one ragged), against _np_slice and float64 under the rules of test_slice_kernels_against_numpy.  Every destination --
    streams, pad channels, the element behind the stream -- is pre-filled and compared whole; two calls give the same bits; the
    in-place LRP is compared after ONE call (an element done in two sweeps would carry the update twice)."""
    require_gpu()
    from rgbd_amd._lib import check, lib

    L = lib()
    bc = gc.build_slice(case, _np_slice, eo.scale_table().numpy())
    B, C, h, w, per_image = (case[k] for k in ("B", "C", "h", "w", "per_image"))
    s, n, st = bc["strides"], bc["n"], torch.cuda.current_stream().cuda_stream
    dy, dmu, dsg, dl = (torch.from_numpy(bc[k]).cuda() for k in ("y", "mu", "sg", "lrp"))
    tb = bc["table"].ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ints = lambda: torch.full((n + 1,), gc.SLICE_ISENT, dtype=torch.int32).cuda()  # noqa: E731
    flt = lambda cs: torch.full((B, h, w, cs), float(gc.SLICE_FSENT)).cuda()  # noqa: E731
    runs = []
    for _ in range(2):
        dsym, didx, o0, o1, q0 = ints(), ints(), flt(s["cs0"]), flt(s["cs1"]), flt(s["cs0"])
        check(L.rgbd_slice_quant_index(dy.data_ptr(), s["ycs"], dmu.data_ptr(), s["mcs"], dsg.data_ptr(), s["scs"], B, C, h, w, per_image,
                                       bc["image_stride"], bc["slice_off"], tb, dsym.data_ptr(), didx.data_ptr(), o0.data_ptr(), s["cs0"],
                                       o1.data_ptr(), s["cs1"], st), "slice_quant_index")
        check(L.rgbd_slice_dequant(dsym.data_ptr(), dmu.data_ptr(), s["mcs"], B, C, h, w, per_image, bc["image_stride"], bc["slice_off"],
                                   q0.data_ptr(), s["cs0"], None, 0, st), "slice_dequant")
        a, b2, inplace = flt(s["cs1"]), flt(C), o0.clone()
        check(L.rgbd_lrp_update(dl.data_ptr(), s["lcs"], o0.data_ptr(), s["cs0"], B * h * w, C, a.data_ptr(), s["cs1"], b2.data_ptr(), C,
                                None, 0, st), "lrp_update")
        check(L.rgbd_lrp_update(dl.data_ptr(), s["lcs"], inplace.data_ptr(), s["cs0"], B * h * w, C, inplace.data_ptr(), s["cs0"], None, 0,
                                None, 0, st), "lrp_update in place")
        torch.cuda.synchronize()
        runs.append({k: v.cpu().numpy() for k, v in dict(sym=dsym, idx=didx, o0=o0, o1=o1, q0=q0, a=a, b2=b2, inplace=inplace).items()})
    got = runs[0]
    for name, stage in bc["stages"].items():
        assert stage["accept"](got) == [], name
    assert all(gc.same_bits(runs[0][k], runs[1][k]) for k in got), "two calls, different bits"


# ---- 2. - 6. the layered contract on every fixture -----------------------------------------------------------------------
def _walk_slices(tr, gsym, gidx, gx, gs, B, h, w, table):
    """Slices identical before the first differing symbol; at the first difference the restatement's decision must be a
    near-boundary one and the GPU's floats (y - mean, scale: set_debug_floats) within 2e-5 of the slice's magnitude of the
    restatement's.  Returns the number of clean slices."""
    per = B * 32 * h * w
    for i, sl in enumerate(tr["slices"]):
        osym, oidx = sl["symbols"].reshape(-1).numpy(), sl["indexes"].reshape(-1).numpy()
        s, k = gsym[i * per:(i + 1) * per], gidx[i * per:(i + 1) * per]
        if np.array_equal(s, osym) and np.array_equal(k, oidx):
            continue
        ox = (tr["y"][:, 32 * i:32 * i + 32] - sl["mu"]).reshape(-1).numpy()
        osg = sl["sigma"].reshape(-1).numpy()
        x, sg = gx[i * per:(i + 1) * per], gs[i * per:(i + 1) * per]
        assert np.abs(x - ox).max() <= 2e-5 * max(1.0, np.abs(ox).max()), (i, np.abs(x - ox).max())
        assert np.abs(sg - osg).max() <= 2e-5 * max(1.0, np.abs(osg).max()), (i, np.abs(sg - osg).max())
        for j in np.nonzero(s != osym)[0]:
            frac = abs(abs(ox[j] - np.floor(ox[j])) - 0.5)
            assert frac <= 2e-4, (i, j, ox[j], x[j])
        for j in np.nonzero(k != oidx)[0]:
            v = max(osg[j], 0.11)
            assert np.min(np.abs(table - v) / table) <= 2e-4, (i, j, osg[j], sg[j])
        print(f"   first difference in slice {i}: {int((s != osym).sum())} symbols, {int((k != oidx).sum())} indexes (all near-boundary)")
        return i
    return len(tr["slices"])


@pytest.mark.parametrize("name", CASES)
def test_layered_contract(name):
    g = np.load(os.path.join(GOLDEN, f"stf1_{name}.npz"))
    B, H, W, seed = int(g["B"]), int(g["H"]), int(g["W"]), int(g["seed"])
    h, w = H // 16, W // 16
    net, orc = _net(seed), _ref(seed)
    x = _images(B, H, W, int(g["config_id"]))
    net.set_debug_floats(True)
    try:
        out = net.compress(x.cuda())
        gx, gs = net.debug_floats(0)
    finally:
        net.set_debug_floats(False)
    assert tuple(out["shape"]) == (H // 64, W // 64) == tuple(g["shape"])
    assert len(out["strings"][0]) == 1 and len(out["strings"][1]) == B
    orc.trace = {}
    oout = orc.compress(x)
    tr, orc.trace = orc.trace, None
    # 2. float stages: y, z against the restatement and the reference's latents; hyper nets on the GPU's own z_hat
    gy, gz = net.debug_tensor("y"), net.debug_tensor("z")
    assert gy.shape == (B, 384, h, w) and gz.shape == (B, 192, h // 4, w // 4)
    print(f"{name}: rel y {_rel(gy, tr['y'].numpy()):.2e}, z {_rel(gz, tr['z'].numpy()):.2e}, "
          f"y vs fixture {_rel(gy[:, ::24, ::2, ::2], g['y_sub']):.2e}")
    assert _rel(gy, tr["y"].numpy()) < 5e-5 and _rel(gz, tr["z"].numpy()) < 5e-5
    assert _rel(gy[:, ::24, ::2, ::2], g["y_sub"]) < 5e-5
    zh = torch.from_numpy(net.debug_tensor("zhat"))
    glm, gls = net.debug_tensor("latent_means"), net.debug_tensor("latent_scales")
    olm, ols = ref.h_s(orc.sd, "h_mean_s", zh), ref.h_s(orc.sd, "h_scale_s", zh)
    print(f"   rel latent_means {_rel(glm, olm.numpy()):.2e}, latent_scales {_rel(gls, ols.numpy()):.2e}")
    assert _rel(glm, olm.numpy()) < 5e-5 and _rel(gls, ols.numpy()) < 5e-5
    # 3. integer stages, bit-exact: z streams from the GPU's own z; the y stream from the GPU's own symbols / indexes
    assert orc.z_compress(torch.from_numpy(gz)) == out["strings"][1]
    gsym, gidx = net.debug_symbols(0)
    assert gsym.shape[0] == B * 384 * h * w
    assert coder.rans_encode(gsym, gidx, orc.gc) == out["strings"][0][0]
    # 4. the slice loop against the restatement on the GPU's own y / latent_means / latent_scales
    orc.trace = {"y": torch.from_numpy(gy)}
    oyh, osym, oidx = orc.slice_loop(torch.from_numpy(gy), torch.from_numpy(glm), torch.from_numpy(gls))
    tr2, orc.trace = orc.trace, None
    clean = _walk_slices(tr2, gsym, gidx, gx, gs, B, h, w, eo.scale_table().numpy())
    same_own = np.array_equal(gsym, osym) and np.array_equal(gidx, oidx)
    print(f"   slices identical before the first boundary flip: {clean} of 12; symbols identical to the restatement on the "
          f"same latents: {same_own}")
    assert clean >= 1
    # 5. the decoder rebuilds the encoder's post-LRP y_hat bit for bit; synthesis; forward
    yhat_enc = net.debug_tensor("yhat").copy()
    if clean == 12:
        assert _rel(yhat_enc, oyh.numpy()) < 5e-5
    rec = net.decompress(out["strings"], out["shape"])
    assert np.array_equal(net.debug_tensor("yhat"), yhat_enc)
    xh = rec["x_hat"].cpu()
    assert xh.shape == (B, 3, H, W) and float(xh.min()) >= 0.0 and float(xh.max()) <= 1.0
    ox = ref.g_s(orc.sd, torch.from_numpy(yhat_enc)).clamp(0, 1)
    assert (xh - ox).abs().max() < 2e-4 and abs(_psnr(xh, x) - _psnr(ox, x)) < 1e-4
    fw = net.forward(x.cuda())
    assert set(fw) == {"x_hat", "likelihoods"} and set(fw["likelihoods"]) == {"y", "z"}
    assert torch.equal(fw["x_hat"].clamp(0, 1), rec["x_hat"])
    ofw = orc.forward(x)
    for k in ("y", "z"):
        got = float(-torch.log2(fw["likelihoods"][k].double()).sum())
        want = float(-torch.log2(ofw["likelihoods"][k].double()).sum())
        print(f"   forward -log2 likelihood sum {k}: {got:.3f} vs restatement {want:.3f}")
        assert abs(got - want) <= 2e-5 * want, (k, got, want)
    # 6. against the reference's fixture: measured floors
    identical = out["strings"][0][0] == g["y_stream"].tobytes() and all(out["strings"][1][i] == g[f"z{i}"].tobytes() for i in range(B))
    nb = len(out["strings"][0][0]) + sum(len(s) for s in out["strings"][1])
    nb_ref = g["y_stream"].shape[0] + sum(g[f"z{i}"].shape[0] for i in range(B))
    dpsnr = abs(_psnr(xh, x) - float(g["psnr"]))
    nflip = int((gsym != g["symbols"].astype(np.int32)).sum()) + int((gidx != g["indexes"].astype(np.int32)).sum())
    print(f"   vs the reference's fixture: streams identical {identical}, |d bytes| {abs(nb - nb_ref)}, |dPSNR| {dpsnr:.3e} dB, "
          f"differing symbols + indexes {nflip}, restatement (this CPU) identical {oout['strings'][0][0] == g['y_stream'].tobytes()}")
    path = os.environ.get("RGBD_RECORD_STF1_FLOORS")
    if path:
        cur = {}
        if os.path.exists(path):
            with open(path) as f:
                cur = json.load(f)
        cur[name] = {"identical": bool(identical), "dbytes": int(abs(nb - nb_ref)), "dpsnr": dpsnr, "differing_decisions": nflip}
        with open(path, "w") as f:
            json.dump(cur, f, indent=1, sort_keys=True)
            f.write("\n")
    with open(os.path.join(GOLDEN, "stf1_floors.json")) as f:
        fl = json.load(f)[name]
    if fl["identical"]:
        assert identical
    else:
        assert abs(nb - nb_ref) <= fl["dbytes"], (abs(nb - nb_ref), fl["dbytes"])
        assert dpsnr <= max(2 * fl["dpsnr"], 1e-12), (dpsnr, fl["dpsnr"])
    assert dpsnr <= 1e-4 or fl.get("cause"), dpsnr


def test_batch_one_stream_and_per_image_streams():
    """B = 2 in one stream in the reference's order (slice-major, (b, c, row, col) inside a slice), decoded as the inverse of
    compress; per_image_streams: image i's streams equal the B = 1 call's."""
    net = _net(0)
    x = _images(2, 192, 128, 63).cuda()
    h, w = 12, 8
    out = net.compress(x)
    sym2, idx2 = net.debug_symbols(0)
    yh2 = net.debug_tensor("yhat").copy()
    rec = net.decompress(out["strings"], out["shape"])
    assert np.array_equal(net.debug_tensor("yhat"), yh2)
    ones = []
    for i in range(2):
        o = net.compress(x[i:i + 1])
        s1, k1 = net.debug_symbols(0)
        ones.append((o, s1, k1))
        r1 = net.decompress(o["strings"], o["shape"])
        assert torch.equal(r1["x_hat"][0], rec["x_hat"][i])
    per = 32 * h * w
    for sl in range(12):  # the batch stream interleaves the images slice by slice
        for i in range(2):
            a = sym2[(sl * 2 + i) * per:(sl * 2 + i + 1) * per]
            assert np.array_equal(a, ones[i][1][sl * per:(sl + 1) * per]), (sl, i)
            assert np.array_equal(idx2[(sl * 2 + i) * per:(sl * 2 + i + 1) * per], ones[i][2][sl * per:(sl + 1) * per])
    net.per_image_streams = True
    try:
        pi = net.compress(x)
        assert len(pi["strings"][0]) == 2
        for i in range(2):
            assert pi["strings"][0][i] == ones[i][0]["strings"][0][0] and pi["strings"][1][i] == ones[i][0]["strings"][1][0]
        rp = net.decompress(pi["strings"], pi["shape"])
        assert torch.equal(rp["x_hat"], rec["x_hat"])
    finally:
        net.per_image_streams = False


# ---- 7. grouped launches ------------------------------------------------------------------------------------------------
def test_grouped_mean_scale_launches_same_bits():
    from rgbd_amd._lib import check, lib

    net = _net(0)
    x = _images(2, 128, 192, 64).cuda()
    res = {}
    try:
        for pair in (0, 1):
            check(lib().rgbd_debug_force_pair(pair), "force_pair")
            out = net.compress(x)
            rec = net.decompress(out["strings"], out["shape"])
            res[pair] = (out["strings"], rec["x_hat"].clone())
    finally:
        check(lib().rgbd_debug_force_pair(1), "force_pair")
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])


# ---- 8. graphs ------------------------------------------------------------------------------------------------------------
def test_replay_and_varying_shapes():
    net = _net(0).clone_shared()
    shapes = [(1, 128, 192, 65), (2, 128, 128, 66)]
    seen = {}
    with torch.cuda.stream(torch.cuda.Stream()):  # (the NULL stream cannot be captured)
        for rnd in range(4):  # eager, capture, replay, replay -- interleaved over two shapes
            for shp in shapes:
                x = _images(*shp).cuda()
                out = net.compress(x)
                rec = net.decompress(out["strings"], out["shape"])
                fw = net.forward(x)
                got = (out["strings"], rec["x_hat"].clone(), fw["x_hat"].clone(), fw["likelihoods"]["y"].clone())
                if shp not in seen:
                    seen[shp] = got
                else:
                    assert got[0] == seen[shp][0], (rnd, shp)
                    assert all(torch.equal(a, b) for a, b in zip(got[1:], seen[shp][1:])), (rnd, shp)
        assert net.graph_count() >= 6
    torch.cuda.synchronize()


# ---- 9. malformed input ---------------------------------------------------------------------------------------------------
def test_malformed_streams_are_an_error_or_garbage_never_a_fault():
    from rgbd_amd import RgbdError

    net = _net(0)
    x = _images(1, 128, 192, 67).cuda()
    good = net.compress(x)
    want = net.decompress(good["strings"], good["shape"])["x_hat"].clone()
    ys, zs = good["strings"][0][0], good["strings"][1][0]

    def dec(y_=ys, z_=zs):
        o = net.decompress([[y_], [z_]], good["shape"])
        torch.cuda.synchronize()
        assert o["x_hat"].shape == want.shape
        return o

    for bad in (b"", ys[:4], ys[:6], ys + b"\x00"):  # not a stream at all
        with pytest.raises((ValueError, RgbdError)):
            dec(y_=bad)
        with pytest.raises((ValueError, RgbdError)):
            dec(z_=bad)
    with pytest.raises((ValueError, RgbdError)):
        dec(y_=ys + bytes(4 * (5 * 384 * 8 * 12 + 1024)))  # longer than any stream of this shape
    dec(y_=ys[:8])                      # only the final state: every later read is past the end
    dec(y_=ys[:len(ys) // 2 & ~3])      # truncated
    dec(z_=zs[:8])                      # truncated z: garbage hyper parameters
    assert torch.equal(dec()["x_hat"], want)  # the engine is usable afterwards


# ---- 10. depth images -----------------------------------------------------------------------------------------------------
def test_channel_1_round_trip():
    net, orc = _net(2, channel=1), _ref(2, channel=1)
    x = _images(1, 128, 128, 68, channel=1)
    out = net.compress(x.cuda())
    orc.trace = {}
    orc.compress(x)
    tr, orc.trace = orc.trace, None
    gy, gz = net.debug_tensor("y"), net.debug_tensor("z")
    assert _rel(gy, tr["y"].numpy()) < 5e-5 and _rel(gz, tr["z"].numpy()) < 5e-5
    assert orc.z_compress(torch.from_numpy(gz)) == out["strings"][1]
    gsym, gidx = net.debug_symbols(0)
    assert gsym.shape[0] == 384 * 8 * 8 and coder.rans_encode(gsym, gidx, orc.gc) == out["strings"][0][0]
    yhat_enc = net.debug_tensor("yhat").copy()
    rec = net.decompress(out["strings"], out["shape"])
    assert np.array_equal(net.debug_tensor("yhat"), yhat_enc)
    xh = rec["x_hat"].cpu()
    assert xh.shape == (1, 1, 128, 128)
    ox = ref.g_s(orc.sd, torch.from_numpy(yhat_enc)).clamp(0, 1)
    assert (xh - ox).abs().max() < 2e-4 and abs(_psnr(xh, x) - _psnr(ox, x)) < 1e-4
    assert torch.equal(net.forward(x.cuda())["x_hat"].clamp(0, 1), rec["x_hat"])


# ---- 11. the single-image tester --------------------------------------------------------------------------------------------
def test_tester_single_with_stf(tmp_path, monkeypatch):
    from PIL import Image

    import rgbd_amd
    from rgbd_amd import synth
    from rgbd_amd.ioutils import read_body, read_uints

    net = _net(0)
    root = tmp_path / "nyu_test"
    (root / "rgb").mkdir(parents=True)
    for i in range(2):
        r, _ = synth.synthetic_pair(i, 100, 150, config_id=69, smooth=True)
        Image.fromarray((r.transpose(1, 2, 0) * 255).astype(np.uint8)).save(root / "rgb" / f"{i:04d}.png")
    monkeypatch.chdir(tmp_path)
    args = types.SimpleNamespace(channel=3, debug=False, experiment=None, dataset=str(root), model="STF", quality="1",
                                 checkpoint=None)
    t = rgbd_amd.TesterSingle(args, rgbd_amd.model_config(), net=net)
    assert t.exp_name == "nyuv2_rgb_STF_1"
    rows, meters = t.test_model(padding_mode="replicate0", padding=True)
    rec_dir = t.get_rec_dir(padding=True, padding_mode="replicate0")
    assert len(rows) == 2 and len(os.listdir(os.path.join(rec_dir, "rgb_rec"))) == 2
    for row in rows:
        assert row["bpp"] == os.path.getsize(os.path.join(rec_dir, "rgb_bin", row["name"])) * 8.0 / (100 * 150)
        assert np.isfinite(row["psnr"]) and row["enc_time"] > 0 and row["dec_time"] > 0
    img, name = t.test_dataloader[0]
    xp = rgbd_amd.datautils.pad(img.cuda(), "replicate0")
    assert xp.shape[-2:] == (128, 192)
    out = net.compress(xp)
    with open(os.path.join(rec_dir, "rgb_bin", name[0]), "rb") as f:
        assert tuple(read_uints(f, 2)) == (100, 150)
        strings, shape = read_body(f)
    assert [list(s) for s in strings] == [list(s) for s in out["strings"]] and tuple(shape) == tuple(out["shape"])
    rec = net.decompress(out["strings"], out["shape"])
    xh, _ = t.decompress_one_image(os.path.join(rec_dir, "rgb_bin"), name[0], mode="replicate0")
    assert torch.equal(xh, rec["x_hat"][:, :, :100, :150])
    # (the tester's PSNR is an fp32 mean on the GPU, this one on the CPU: two summation orders over 45,000 terms, ~log2(n) * 2^-24
    #  = 1e-6 relative = 4e-6 dB)
    assert abs(eo.psnr(xh.cpu(), img) - rows[0]["psnr"]) < 1e-5
