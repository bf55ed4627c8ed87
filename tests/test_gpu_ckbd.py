"""The checkerboard Cheng2020 model (rgbd_amd.ckbd; reference models/Cheng2020withCKBD.py) on the GPU, on the three fixtures
the unmodified reference produced (tests/golden/ckbd_*.npz):

 (a) the layered contract of tests/test_gpu_stf_single.py with that file's tolerances, against the CPU restatement
     (tests/ckbd_ref.py): y, z, hyper, means, scales relative 5e-5; x_hat 2e-4 absolute; |dPSNR| < 1e-4 dB; likelihood sums 2e-5;
 (b) the context convolution against a float64 evaluation of the MASKED 5x5 conv on the same y_hat, at non-anchor positions,
     within (12 M + 2) * 2^-24 * (sum |w| |x| + |b|) (12 M + 1 roundings of a chain of non-negative magnitudes, one for the
     stored float); the same comparison with the mask reversed or missing must fail;
 (c) the integer stage: oracle.coder reproduces the GPU's y and z streams from the GPU's own symbols byte for byte, the
     decoder gets them back, B = 1 and B = 2 with per_image_streams 0 and 1, per-image bits of a batch = the B = 1 calls';
 (d) a teacher-forced census against the reference: with the fixture's symbols forced, every GPU decision that differs from
     the reference's sits inside the 2e-4 windows measured on the REFERENCE's recorded floats, and the GPU's floats at all
     other symbols match the recorded ones to 2e-5 * max(1, |v|);
 (e) free-running identity with the reference: reported, recorded by RGBD_RECORD_CKBD_FLOORS=<path> into
     tests/golden/ckbd_floors.json, asserted only where the recording run observed it; there the GPU also decodes the
     REFERENCE's streams to the fixture's x_hat within 2e-4;
 (f) forward() against the restatement and the fixture's likelihood sums;
 (g) the graph cache: the second call of a shape replays; lost captures still give the right output.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ckbd_ref as ref
from gpu_utils import require_gpu
from oracle import coder
from oracle import elic_oracle as eo

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["a_64x128", "b_b2_128x64_d", "c_128x192_n128"]
ROUND_WINDOW = SCALE_WINDOW = 2e-4  # tests/golden/make_margins.py
_NETS, _REFS, _RUNS = {}, {}, {}


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def _psnr(a, b):
    return float(-10 * np.log10(torch.mean((a - b) ** 2).item()))


def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"ckbd_{name}.npz"))


def _key(g):
    return int(g["seed"]), int(g["N"]), int(g["channel"])


def _sd(key):
    from rgbd_amd import synth

    return synth.synthetic_state_dict(key[0], model="ckbd", N=key[1], channel=key[2])


def _net(key):
    require_gpu()
    if key not in _NETS:
        import rgbd_amd

        m = rgbd_amd.modelZoo["ckbd"](N=key[1], channel=key[2], config=rgbd_amd.model_config()).eval()
        m.load_state_dict(_sd(key), strict=True)
        assert m.update(force=True)
        _NETS[key] = m.to("cuda")
    return _NETS[key]


def _ref(key):
    if key not in _REFS:
        r = ref.CkbdRef(_sd(key))
        assert r.update()
        _REFS[key] = r
    return _REFS[key]


def _images(g):
    from rgbd_amd import synth

    r, d = synth.synthetic_batch(int(g["B"]), int(g["H"]), int(g["W"]), config_id=int(g["config_id"]))
    return torch.from_numpy(r if int(g["channel"]) == 3 else d)


def _run(name):
    """One free-running compress + decompress + forward of a fixture on the GPU and on the restatement, shared by the tests."""
    if name not in _RUNS:
        g = _fixture(name)
        net, orc = _net(_key(g)), _ref(_key(g))
        x = _images(g)
        net.set_debug_floats(True)
        try:
            out = net.compress(x.cuda())
            gx, gs = net.debug_floats(0)
        finally:
            net.set_debug_floats(False)
        t = {k: net.debug_tensor(k).copy() for k in ("y", "z", "zhat", "hyper", "yhat", "ctx", "means", "scales")}
        sym, idx = net.debug_symbols(0)
        rec = net.decompress(out["strings"], out["shape"])
        yhat_dec = net.debug_tensor("yhat").copy()
        orc.trace = {}
        oout = orc.compress(x)
        tr, orc.trace = orc.trace, None
        _RUNS[name] = dict(g=g, net=net, orc=orc, x=x, out=out, gx=gx, gs=gs, t=t, sym=sym.copy(), idx=idx.copy(), xh=rec["x_hat"].cpu(),
                           yhat_dec=yhat_dec, oout=oout, tr=tr)
    return _RUNS[name]


def _near(x, s, table):
    m_round = 0.5 - np.abs(x - np.rint(x))
    rel = np.abs(s[:, None] / table[None, :-1] - 1.0).min(axis=1)
    return (m_round <= ROUND_WINDOW * np.maximum(1.0, np.abs(x))), (rel <= SCALE_WINDOW)


# ---- (a) layered contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_layered_contract(name):
    r = _run(name)
    g, net, orc, t, tr, x = r["g"], r["net"], r["orc"], r["t"], r["tr"], r["x"]
    B, N, C, H, W = int(g["B"]), int(g["N"]), int(g["channel"]), int(g["H"]), int(g["W"])
    h, w = H // 16, W // 16
    assert tuple(r["out"]["shape"]) == (H // 64, W // 64) == tuple(g["shape"])
    assert len(r["out"]["strings"][0]) == 1 and len(r["out"]["strings"][1]) == B
    assert t["y"].shape == (B, N, h, w) and t["z"].shape == (B, N, h // 4, w // 4) and t["hyper"].shape == (B, 2 * N, h, w)
    ry, rz = _rel(t["y"], tr["y"].numpy()), _rel(t["z"], tr["z"].numpy())
    print(f"{name}: rel y {ry:.2e}, z {rz:.2e}, y vs fixture {_rel(t['y'][:, ::12, ::2, ::2], g['y_sub']):.2e}")
    assert ry < 5e-5 and rz < 5e-5 and _rel(t["y"][:, ::12, ::2, ::2], g["y_sub"]) < 5e-5
    # the later stages on the GPU's own inputs: hyper from its z_hat, the two passes from its y / hyper with ITS symbols forced
    ohyp = ref.h_s(orc.sd, torch.from_numpy(t["zhat"]))
    orc.trace = {}
    oyh, osym, oidx = orc.two_pass(torch.from_numpy(t["y"]), torch.from_numpy(t["hyper"]), forced=r["sym"])
    tr2, orc.trace = orc.trace, None
    rh, rm, rs = _rel(t["hyper"], ohyp.numpy()), _rel(t["means"], tr2["means"].numpy()), _rel(t["scales"], tr2["scales"].numpy())
    print(f"   rel hyper {rh:.2e}, means {rm:.2e}, scales {rs:.2e}; decisions identical to the restatement on the same latents: "
          f"{np.array_equal(osym, r['sym']) and np.array_equal(oidx, r['idx'])}")
    assert rh < 5e-5 and rm < 5e-5 and rs < 5e-5
    assert _rel(t["yhat"], oyh.numpy()) < 5e-5
    # the decoder rebuilds the encoder's y_hat bit for bit; synthesis (not clamped)
    assert np.array_equal(r["yhat_dec"], t["yhat"])
    xh = r["xh"]
    assert xh.shape == (B, C, H, W)
    ox = ref.g_s(orc.sd, torch.from_numpy(t["yhat"]))
    dx, dp = float((xh - ox).abs().max()), abs(_psnr(xh, x) - _psnr(ox, x))
    print(f"   x_hat: max |gpu - restatement| {dx:.2e} (max |x_hat| {float(ox.abs().max()):.2f}), |dPSNR| {dp:.2e} dB")
    assert float(xh.min()) < 0.0 or float(xh.max()) > 1.0  # these weights leave [0, 1]: decompress() does not clamp
    assert dx < 2e-4 and dp < 1e-4


# ---- (b) the masked context convolution ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_context_conv_is_the_masked_one(name):
    r = _run(name)
    g, orc, net = r["g"], r["orc"], r["net"]
    M = int(g["N"])
    w64, b64 = orc.sd["context_prediction.weight"].double(), orc.sd["context_prediction.bias"].double()
    mask = ref.context_mask(w64)
    na = ~ref.anchor_mask(*r["t"]["yhat"].shape[-2:])

    def worst(yhat, ctx, m):
        yh, got = torch.from_numpy(yhat).double(), torch.from_numpy(ctx).double()
        want = F.conv2d(yh, w64 * m, b64, padding=2)
        bound = (12 * M + 2) * 2.0 ** -24 * F.conv2d(yh.abs(), (w64 * m).abs(), b64.abs(), padding=2)
        assert float(got[:, :, ~na].abs().max()) == 0.0  # anchor outputs are not computed: the buffer's zeros
        return float(((got - want).abs() / bound)[:, :, na].max())

    # compress(): y_hat holds the anchor half only, so the unmasked taps of a non-anchor output meet zeros -- the reversed
    # mask shows here; forward(): y_hat = round(y) on the whole grid -- a missing mask shows there
    net.forward(r["x"].cuda())
    fy, fc = net.debug_tensor("yhat").copy(), net.debug_tensor("ctx").copy()
    res = {"compress": [worst(r["t"]["yhat"], r["t"]["ctx"], m) for m in (mask, 1 - mask)],
           "forward": [worst(fy, fc, m) for m in (mask, 1 - mask, torch.ones_like(mask))]}
    print(f"{name}: ctx worst |err| / bound: compress masked {res['compress'][0]:.3f}, reversed {res['compress'][1]:.3g}; "
          f"forward masked {res['forward'][0]:.3f}, reversed {res['forward'][1]:.3g}, no mask {res['forward'][2]:.3g}")
    assert res["compress"][0] <= 1.0 and res["forward"][0] <= 1.0
    # the fixture weights have non-zero masked taps: a reversed or missing mask cannot pass
    assert res["compress"][1] > 1.0 and res["forward"][1] > 1.0 and res["forward"][2] > 1.0


# ---- (c) the integer stage ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_integer_stage(name):
    r = _run(name)
    g, orc, out = r["g"], r["orc"], r["out"]
    B, N, H, W = int(g["B"]), int(g["N"]), int(g["H"]), int(g["W"])
    assert r["sym"].shape[0] == B * N * (H // 16) * (W // 16)
    assert coder.rans_encode(r["sym"], r["idx"], orc.gc) == out["strings"][0][0]
    assert np.array_equal(coder.rans_decode(out["strings"][0][0], r["idx"], orc.gc), r["sym"])
    assert orc.z_compress(torch.from_numpy(r["t"]["z"])) == out["strings"][1]
    assert np.array_equal(orc.z_decompress(out["strings"][1], out["shape"]).numpy(), r["t"]["zhat"])
    # stream order: anchor half of the whole batch first, each half in (n, c, row, w/2) order
    y, p = torch.from_numpy(r["t"]["y"]), (torch.from_numpy(r["t"]["scales"]), torch.from_numpy(r["t"]["means"]))
    want_sym = np.concatenate([eo.quantize_symbols(eo.pack(y, a), eo.pack(p[1], a)).reshape(-1).numpy() for a in (True, False)])
    want_idx = np.concatenate([eo.scale_indexes(eo.pack(p[0], a), orc.table).reshape(-1).numpy() for a in (True, False)])
    assert np.array_equal(want_sym, r["sym"]) and np.array_equal(want_idx, r["idx"])
    assert np.array_equal(np.rint(r["gx"]).astype(np.int32), r["sym"])


def test_batch_one_stream_and_per_image_streams():
    g = _fixture("b_b2_128x64_d")
    r = _run("b_b2_128x64_d")
    net, x = r["net"], r["x"].cuda()
    half = r["sym"].shape[0] // 2
    ones = []
    for i in range(2):
        o = net.compress(x[i:i + 1])
        s1, k1 = net.debug_symbols(0)
        ones.append((o, s1.copy(), k1.copy()))
        r1 = net.decompress(o["strings"], o["shape"])
        assert torch.equal(r1["x_hat"][0].cpu(), r["xh"][i])  # the same bits for an image alone and inside a batch
    q = half // 2
    for part in range(2):
        for i in range(2):
            a = slice(part * half + i * q, part * half + (i + 1) * q)
            assert np.array_equal(r["sym"][a], ones[i][1][part * q:(part + 1) * q]), (part, i)
            assert np.array_equal(r["idx"][a], ones[i][2][part * q:(part + 1) * q]), (part, i)
    net.per_image_streams = True
    try:
        pi = net.compress(x)
        assert len(pi["strings"][0]) == 2 and len(pi["strings"][1]) == 2
        for i in range(2):
            assert pi["strings"][0][i] == ones[i][0]["strings"][0][0] and pi["strings"][1][i] == ones[i][0]["strings"][1][0]
        rp = net.decompress(pi["strings"], pi["shape"])
        assert torch.equal(rp["x_hat"].cpu(), r["xh"])
    finally:
        net.per_image_streams = False
    assert int(g["B"]) == 2


# ---- (d) teacher-forced census against the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_teacher_forced_census(name):
    g = _fixture(name)
    net = _net(_key(g))
    x = _images(g)
    rsym, ridx = g["symbols"].astype(np.int32), g["indexes"].astype(np.int32)
    rx, rs = g["x"], g["sigma"]
    table = eo.scale_table().numpy().astype(np.float32)
    net.set_forced_symbols(0, rsym, g["z_symbols"].astype(np.int32).reshape(-1))
    net.set_debug_floats(True)
    try:
        net.compress(x.cuda())
        gx, gs = net.debug_floats(0)
        gsym, gidx = net.debug_symbols(0)
    finally:
        net.set_debug_floats(False)
        net.set_forced_symbols(0, None, None)
    near_r, near_s = _near(rx, rs, table)
    dsym, didx = gsym != rsym, gidx != ridx
    print(f"{name}: forced census: {int(dsym.sum())} symbols and {int(didx.sum())} scale indexes differ from the reference's "
          f"of {rsym.size}; near-boundary decisions of the reference: {int(near_r.sum())} + {int(near_s.sum())}")
    assert not (dsym & ~near_r).any(), "a symbol differs from the reference's away from a rounding boundary"
    assert not (didx & ~near_s).any(), "a scale index differs from the reference's away from a table entry"
    keep = ~(dsym | didx)
    ex = np.abs(gx - rx) / np.maximum(1.0, np.abs(rx))
    es = np.abs(gs - rs) / np.maximum(1.0, np.abs(rs))
    print(f"   floats vs the reference's: max |d(y - mean)| {ex[keep].max():.2e}, max |d scale| {es[keep].max():.2e} (of max(1, |v|))")
    assert ex[keep].max() <= 2e-5 and es[keep].max() <= 2e-5


# ---- (e) free-running identity with the reference: measured floors ------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_identity_with_the_reference(name):
    r = _run(name)
    g, net, out, x = r["g"], r["net"], r["out"], r["x"]
    B = int(g["B"])
    identical = out["strings"][0][0] == g["y_stream"].tobytes() and all(out["strings"][1][i] == g[f"z{i}"].tobytes() for i in range(B))
    nb = len(out["strings"][0][0]) + sum(len(s) for s in out["strings"][1])
    nb_ref = g["y_stream"].shape[0] + sum(g[f"z{i}"].shape[0] for i in range(B))
    dpsnr = abs(_psnr(r["xh"], x) - float(g["psnr"]))
    nflip = int((r["sym"] != g["symbols"].astype(np.int32)).sum()) + int((r["idx"] != g["indexes"].astype(np.int32)).sum())
    print(f"{name}: vs the reference's fixture: streams identical {identical}, |d bytes| {abs(nb - nb_ref)}, |dPSNR| {dpsnr:.3e} dB, "
          f"differing symbols + indexes {nflip}, restatement (this CPU) identical {r['oout']['strings'][0][0] == g['y_stream'].tobytes()}")
    path = os.environ.get("RGBD_RECORD_CKBD_FLOORS")
    if path:
        cur = {}
        if os.path.exists(path):
            with open(path) as f:
                cur = json.load(f)
        cur[name] = {"identical": bool(identical), "dbytes": int(abs(nb - nb_ref)), "dpsnr": dpsnr, "differing_decisions": nflip}
        with open(path, "w") as f:
            json.dump(cur, f, indent=1, sort_keys=True)
            f.write("\n")
        fl = cur[name]
    else:
        with open(os.path.join(GOLDEN, "ckbd_floors.json")) as f:
            fl = json.load(f)[name]
    if fl["identical"]:
        assert identical
    else:
        assert abs(nb - nb_ref) <= fl["dbytes"], (abs(nb - nb_ref), fl["dbytes"])
        assert dpsnr <= max(2 * fl["dpsnr"], 1e-12), (dpsnr, fl["dpsnr"])
    assert dpsnr <= 1e-4 or fl.get("cause"), dpsnr
    if identical:  # the GPU decodes the REFERENCE's streams to the reference's x_hat
        strings = [[g["y_stream"].tobytes()], [g[f"z{i}"].tobytes() for i in range(B)]]
        rec = net.decompress(strings, tuple(int(v) for v in g["shape"]))["x_hat"].cpu()
        want = torch.from_numpy(g["xhat"]) if "xhat" in g else r["orc"].decompress(strings, tuple(int(v) for v in g["shape"]))["x_hat"]
        d = float((rec - want).abs().max())
        print(f"   the reference's streams decoded on the GPU: max |x_hat - reference| {d:.2e}")
        assert d < 2e-4


# ---- (f) forward() ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_forward(name):
    r = _run(name)
    g, net, orc, x = r["g"], r["net"], r["orc"], r["x"]
    fw = net.forward(x.cuda())
    assert set(fw) == {"x_hat", "likelihoods"} and set(fw["likelihoods"]) == {"y", "z"}
    t = {k: net.debug_tensor(k).copy() for k in ("y", "yhat", "ctx", "means", "scales", "hyper")}
    assert np.array_equal(t["yhat"], np.round(t["y"]))  # y_hat = round(y), half to even
    am = ref.anchor_mask(*t["y"].shape[-2:]).numpy()
    assert float(np.abs(t["ctx"][:, :, am]).max()) == 0.0 and float(np.abs(t["ctx"][:, :, ~am]).max()) > 0.0
    orc.trace = {}
    ofw = orc.forward(x)
    tr, orc.trace = orc.trace, None
    # the parameter pass on the GPU's own y_hat / hyper
    ctx = torch.where(torch.from_numpy(am), torch.zeros(()), ref.context(orc.sd, torch.from_numpy(t["yhat"])))
    sc, mu = orc._params(ctx, torch.from_numpy(t["hyper"]))
    print(f"{name}: forward rel ctx {_rel(t['ctx'], ctx.numpy()):.2e}, means {_rel(t['means'], mu.numpy()):.2e}, scales {_rel(t['scales'], sc.numpy()):.2e}")
    assert _rel(t["ctx"], ctx.numpy()) < 5e-5 and _rel(t["means"], mu.numpy()) < 5e-5 and _rel(t["scales"], sc.numpy()) < 5e-5
    ox = ref.g_s(orc.sd, torch.from_numpy(t["yhat"]))
    assert float((fw["x_hat"].cpu() - ox).abs().max()) < 2e-4
    for k, ref_bits in (("y", float(g["lik_y_bits"])), ("z", float(g["lik_z_bits"]))):
        lk = fw["likelihoods"][k]
        assert float(lk.min()) >= float(np.float32(1e-9)) and float(lk.max()) <= 1.0  # lower-bounded as elsewhere (fp32 1e-9)
        got = float(-torch.log2(lk.double()).sum())
        want = float(-torch.log2(ofw["likelihoods"][k].double()).sum())
        print(f"   forward -log2 likelihood sum {k}: {got:.3f} vs restatement {want:.3f} vs the reference's {ref_bits:.3f}")
        assert abs(got - want) <= 2e-5 * want and abs(got - ref_bits) <= 2e-5 * ref_bits, (k, got, want, ref_bits)


# ---- (g) graphs ---------------------------------------------------------------------------------------------------------------------
def _round(net, x):
    out = net.compress(x)
    rec = net.decompress(out["strings"], out["shape"])
    fw = net.forward(x)
    return out["strings"], rec["x_hat"].clone(), fw["x_hat"].clone(), fw["likelihoods"]["y"].clone()


def _same(a, b):
    return a[0] == b[0] and all(torch.equal(p, q) for p, q in zip(a[1:], b[1:]))


def test_graph_replay_and_lost_captures():
    from rgbd_amd._lib import check, lib

    r = _run("a_64x128")
    net = r["net"].clone_shared()
    x = r["x"].cuda()
    x2 = torch.cat([x, x.flip(-1)], dim=-1)[:, :, :, :192].contiguous()  # a larger shape, 64 x 192: the workspace grows
    x3 = x[:, :, :, :64].contiguous()                                    # a smaller one, 64 x 64: it does not
    try:
        with torch.cuda.stream(torch.cuda.Stream()):  # (the NULL stream cannot be captured)
            for xs in (x, x2):
                first = _round(net, xs)                # eager: first call of the shape
                if xs is x:
                    assert first[0] == r["out"]["strings"] and torch.equal(first[1].cpu(), r["xh"])
                for _ in range(2):                     # (a workspace that grew during the first round drops what was cached)
                    assert _same(_round(net, xs), first)
                g0 = net.graph_count()
                assert g0 >= 3                         # compress, decompress and forward of this shape are cached ...
                assert _same(_round(net, xs), first) and net.graph_count() == g0  # ... and the next call replays them
            ref3 = _round(net, x3)                     # eager
            g1 = net.graph_count()
            check(lib().rgbd_debug_fail_captures(3), "fail_captures")  # the three captures of the next round are lost
            lost = _round(net, x3)
            assert net.graph_count() == g1 and _same(lost, ref3)
            again = _round(net, x3)                    # the next round captures
            assert net.graph_count() == g1 + 3 and _same(again, ref3) and _same(_round(net, x3), ref3)
        torch.cuda.synchronize()
    finally:
        check(lib().rgbd_debug_fail_captures(0), "fail_captures")
