"""The latent codec of ELIC_master (rgbd_amd.MasterLatentCodec, engine family 20; reference models/elic_master.py without its outer
blocks) on the GPU, on the four fixtures the unmodified reference class produced in fp32 and in .double()
(tests/golden/master_latent_<case>.npz; cases, inputs, bounds and acceptance functions: tests/master_latent_cases.py, FACTOR = 8):

 1. self-consistency, asserted hard on every case: decompress(compress(f)) returns and the decoder's y_hat is the encoder's bit
    for bit; image b of case b alone gives the z stream and symbols it gives in the batch; three calls in a row give the same
    streams and the same f_hat bits; a captured replay on a side stream equals the eager call;
 2. one model across shapes: a, c, b, a with one set of weights, eagerly and then through the graph cache: every call gives the
    bits of a model that never saw another shape;
 3. the layered contract: y within 8 e_ref_y of the fp64 values, y_hat under the reference's symbols within 8 e_ref_yhat, the z
    symbols and z streams the reference's, f_hat decoded from the REFERENCE'S OWN STREAMS within 8 max(e_ref_fhat, 2^-23);
 4. the teacher-forced census: under the reference's symbols a differing symbol or scale index is accepted only within the float
    bound of a boundary (master_latent_cases.census), and the floats behind the decisions stay within those bounds;
 5. free-running identity with the reference: measured, recorded by RGBD_RECORD_MASTER_FLOORS=<path> into
    tests/golden/master_latent_floors.json, from then on asserted as ceilings;
 6. forward(): keys, shapes, likelihoods in [1e-9, 1], bit sums within 8 x the reference's own fp32-to-fp64 gap;
 7. guides matter: decoding with up1..up3 zeroed, or with two of them exchanged, leaves the bound of 3;
 8. refusals write nothing and leave the handle usable; a handle of family 1 or 13 is refused by the new entry points.
The model is built once per set of weights for the whole module.
"""
import json
import os

import numpy as np
import pytest
import torch

import master_latent_cases as mc
from gpu_utils import require_gpu
from rgbd_amd import MasterLatentCodec, RgbdError  # (the feature: without it this import fails)
from rgbd_amd._lib import lib

pytestmark = pytest.mark.gpu

CASES = list(mc.CASES)
_NETS, _RUNS, _FORCED = {}, {}, {}


def _fresh_net(wseed_of):
    require_gpu()
    m = MasterLatentCodec(config=mc.config()).eval()
    m.load_state_dict(mc.weights(wseed_of), strict=True)
    assert m.update(force=True)
    return m.to("cuda")


def _net(name):
    key = mc.CASES[name][4]
    if key not in _NETS:
        _NETS[key] = _fresh_net(name)
    return _NETS[key]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _psnr(a, b):
    return float(-10 * np.log10(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def _run(name):
    """One free-running compress + decompress of a case, shared by the tests."""
    if name not in _RUNS:
        fx, net = mc.load_fixture(name), _net(name)
        f, *ups = (t.cuda() for t in mc.inputs(name))
        out = net.compress(f)
        t = {k: net.debug_tensor(k).copy() for k in ("y", "yhat", "z")}
        sym, idx = (a.copy() for a in net.debug_symbols(0))
        rec = net.decompress(out["strings"], out["shape"], *ups)
        _RUNS[name] = dict(fx=fx, net=net, f=f, ups=ups, out=out, t=t, sym=sym, idx=idx, fh=rec["f_hat"].cpu(), rec_keys=set(rec),
                           yhat_dec=net.debug_tensor("yhat").copy())
    return _RUNS[name]


def _forced(name):
    """One compress under the reference's symbols (teacher forcing): every part sees the reference's context."""
    if name not in _FORCED:
        r = _run(name)
        fx, net = r["fx"], r["net"]
        net.set_forced_symbols(0, fx["symbols"].astype(np.int32), fx["z_symbols"].astype(np.int32).reshape(-1))
        net.set_debug_floats(True)
        try:
            net.compress(r["f"])
            gx, gs = net.debug_floats(0)
            sym, idx = net.debug_symbols(0)
            _FORCED[name] = dict(x=gx.copy(), s=gs.copy(), sym=sym.copy(), idx=idx.copy(), yhat=net.debug_tensor("yhat").copy())
        finally:
            net.set_debug_floats(False)
            net.set_forced_symbols(0, None, None)
    return _FORCED[name]


# ---- 1. self-consistency ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_decoder_rebuilds_the_encoders_yhat_bit_for_bit(name):
    r = _run(name)
    B, H, W = mc.CASES[name][:3]
    assert r["rec_keys"] == {"f_hat"} and set(r["out"]) == {"strings", "shape"} and tuple(r["out"]["shape"]) == (H // 64, W // 64)
    assert len(r["out"]["strings"][0]) == 1 and len(r["out"]["strings"][1]) == B
    assert tuple(r["fh"].shape) == (B, mc.N, H, W) and bool(torch.isfinite(r["fh"]).all())
    assert np.array_equal(_u32(r["yhat_dec"]), _u32(r["t"]["yhat"]))  # through ten dependent parts
    assert r["sym"].size == B * mc.M * (H // 16) * (W // 16)


@pytest.mark.parametrize("name", CASES)
def test_three_calls_in_a_row_give_the_same_bits(name):
    r = _run(name)
    for _ in range(3):
        out = r["net"].compress(r["f"])
        assert out["strings"] == r["out"]["strings"]
        assert torch.equal(r["net"].decompress(out["strings"], out["shape"], *r["ups"])["f_hat"].cpu(), r["fh"])


def test_image_of_the_batch_and_alone():
    r = _run("b")
    net, f, ups = r["net"], r["f"], r["ups"]
    T = r["sym"].size // 2
    net.per_image_streams = True
    try:
        pi = net.compress(f)
        sym_pi = net.debug_symbols(0)[0].copy()
        assert len(pi["strings"][0]) == 2 and len(pi["strings"][1]) == 2
        alone = []
        for i in range(2):
            one = net.compress(f[i:i + 1])
            sym_one = net.debug_symbols(0)[0].copy()
            alone.append(sym_one)
            assert one["strings"][1][0] == r["out"]["strings"][1][i] == pi["strings"][1][i]  # the z stream of the image in the batch
            assert one["strings"][0][0] == pi["strings"][0][i]
            assert np.array_equal(sym_one, sym_pi[i * T:(i + 1) * T])
            fh = net.decompress(one["strings"], one["shape"], *[u[i:i + 1] for u in ups])["f_hat"].cpu()
            assert torch.equal(fh, r["fh"][i:i + 1])
        # the batch's one stream holds the same symbols part by part, the images of a part one after the other
        ob = o1 = 0
        for C in mc.config()["slice_ch"]:
            for _ in range(2):
                n = C * (64 // 16) * (128 // 16 // 2)
                for i in range(2):
                    assert np.array_equal(r["sym"][ob + i * n:ob + (i + 1) * n], alone[i][o1:o1 + n]), (C, i)
                ob, o1 = ob + 2 * n, o1 + n
        assert ob == r["sym"].size and o1 == T
        assert torch.equal(net.decompress(pi["strings"], pi["shape"], *ups)["f_hat"].cpu(), r["fh"])
    finally:
        net.per_image_streams = False


def test_captured_replay_equals_the_eager_call():
    r = _run("a")
    net, f, ups = r["net"].clone_shared(), r["f"], r["ups"]

    def round_trip():
        out = net.compress(f)
        rec = net.decompress(out["strings"], out["shape"], *ups)
        fw = net.forward(f, *ups)
        return out["strings"], rec["f_hat"].clone(), fw["f_hat"].clone(), fw["likelihoods"]["y_likelihoods"].clone()

    with torch.cuda.stream(torch.cuda.Stream()):  # (the NULL stream cannot be captured)
        first = round_trip()
        assert first[0] == r["out"]["strings"] and torch.equal(first[1].cpu(), r["fh"])
        for _ in range(3):
            again = round_trip()
            assert again[0] == first[0] and all(torch.equal(a, b) for a, b in zip(again[1:], first[1:]))
        assert net.graph_count() >= 3  # compress, decompress and forward of this shape replay
    torch.cuda.synchronize()


# ---- 2. one model across shapes ------------------------------------------------------------------------------------------------------
def _alone(name):
    """What a model that never sees another shape gives: the yardstick."""
    net = _fresh_net(name)
    f, *ups = (t.cuda() for t in mc.inputs(name))
    out = net.compress(f)
    yhat = _u32(net.debug_tensor("yhat")).copy()
    rec = net.decompress(out["strings"], out["shape"], *ups)
    fw = net.forward(f, *ups)
    return dict(f=f, ups=ups, strings=out["strings"], shape=tuple(out["shape"]), yhat=yhat, fh=rec["f_hat"].cpu(), fw_fh=fw["f_hat"].cpu(),
                fw_ly=fw["likelihoods"]["y_likelihoods"].cpu(), fw_lz=fw["likelihoods"]["z_likelihoods"].cpu())


def _same(net, want, where):
    out = net.compress(want["f"])
    assert out["strings"] == want["strings"] and tuple(out["shape"]) == want["shape"], where
    assert np.array_equal(_u32(net.debug_tensor("yhat")), want["yhat"]), where
    assert torch.equal(net.decompress(want["strings"], want["shape"], *want["ups"])["f_hat"].cpu(), want["fh"]), where
    assert np.array_equal(_u32(net.debug_tensor("yhat")), want["yhat"]), where
    fw = net.forward(want["f"], *want["ups"])
    assert torch.equal(fw["f_hat"].cpu(), want["fw_fh"]) and torch.equal(fw["likelihoods"]["y_likelihoods"].cpu(), want["fw_ly"]), where
    assert torch.equal(fw["likelihoods"]["z_likelihoods"].cpu(), want["fw_lz"]), where


def test_one_model_across_shapes():
    alone = {n: _alone(n) for n in sorted(set(mc.ONE_MODEL))}
    for n in alone:  # (and the module's shared model, which has seen everything the other tests ran, gave the same streams)
        assert _run(n)["out"]["strings"] == alone[n]["strings"] and torch.equal(_run(n)["fh"], alone[n]["fh"])
    net = _fresh_net("a")
    for step, n in enumerate(mc.ONE_MODEL):
        _same(net, alone[n], ("eager", step, n))
    clone = net.clone_shared()
    with torch.cuda.stream(torch.cuda.Stream()):
        for rnd in range(3):
            for n in mc.ONE_MODEL:
                _same(clone, alone[n], ("side stream", rnd, n))
        assert clone.graph_count() >= 3
    torch.cuda.synchronize()


# ---- 3. the layered contract ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_layered_contract(name):
    r, fo = _run(name), _forced(name)
    fx, net = r["fx"], r["net"]
    B = mc.CASES[name][0]
    e_y, e_yhat = mc.y_err(r["t"]["y"], fx), mc.yhat_err(fo["yhat"], fx)
    zsym = np.rint(r["t"]["z"] - np.asarray(net.eb_medians_numpy()[0]).reshape(1, -1, 1, 1)).astype(np.int16)
    ref_strings = [[fx["y_stream"].tobytes()], [fx[f"z{i}"].tobytes() for i in range(B)]]
    fh_ref = net.decompress(ref_strings, tuple(int(v) for v in fx["shape"]), *r["ups"])["f_hat"].cpu()
    e_fh = mc.fhat_err(name, fh_ref, fx)
    print(f"{name}: y {e_y:.2e} (bound {mc.y_bound(fx):.2e}), y_hat under the reference's symbols {e_yhat:.2e} (bound {mc.yhat_bound(fx):.2e}), "
          f"f_hat from the reference's streams {e_fh:.2e} (bound {mc.fhat_bound(fx):.2e})")
    assert np.array_equal(zsym, fx["z_symbols"])
    assert [bytes(s) for s in r["out"]["strings"][1]] == ref_strings[1]
    assert e_y <= mc.y_bound(fx)
    assert e_yhat <= mc.yhat_bound(fx)
    assert e_fh <= mc.fhat_bound(fx)


# ---- 4. the teacher-forced census -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_teacher_forced_census(name):
    fx, fo = _run(name)["fx"], _forced(name)
    bx, bs = mc.decision_bounds(fx)
    d_round, d_scale = mc.boundary_distances(fx)
    dsym, didx = fo["sym"] != fx["symbols"].astype(np.int32), fo["idx"] != fx["indexes"].astype(np.int32)
    print(f"{name}: forced census: {int(dsym.sum())} symbols and {int(didx.sum())} scale indexes of {dsym.size} differ from the reference's; "
          f"decisions within the float bound of a boundary: {int((d_round < bx).sum())} + {int((d_scale < bs).sum())}; "
          f"max |d(y - mean)| {np.abs(fo['x'] - fx['x64']).max():.2e} (bound {bx:.2e}), max |d scale| {np.abs(fo['s'] - fx['sigma64']).max():.2e} (bound {bs:.2e})")
    assert mc.census(fx, fo["sym"], fo["idx"], fo["x"], fo["s"]) == []


# ---- 5. free-running identity with the reference: measured floors ------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_identity_with_the_reference(name):
    r = _run(name)
    fx, out = r["fx"], r["out"]
    B = mc.CASES[name][0]
    identical = out["strings"][0][0] == fx["y_stream"].tobytes() and all(out["strings"][1][i] == fx[f"z{i}"].tobytes() for i in range(B))
    nb = len(out["strings"][0][0]) + sum(len(s) for s in out["strings"][1])
    nb_ref = fx["y_stream"].shape[0] + sum(fx[f"z{i}"].shape[0] for i in range(B))
    pos = mc.fhat_positions(name)
    got = r["fh"].reshape(-1).numpy() if pos is None else r["fh"].reshape(-1)[torch.from_numpy(pos)].numpy()
    ref_strings = [[fx["y_stream"].tobytes()], [fx[f"z{i}"].tobytes() for i in range(B)]]
    fh_ref = r["net"].decompress(ref_strings, tuple(int(v) for v in fx["shape"]), *r["ups"])["f_hat"].cpu().reshape(-1)
    base = fh_ref.numpy() if pos is None else fh_ref[torch.from_numpy(pos)].numpy()
    # PSNR of f_hat against the fp64 f_hat (peak: its largest magnitude), free-running against decoded from the reference's streams
    peak = float(fx["ref64_max"])
    dpsnr = abs(_psnr(got / peak, fx["fhat64"] / peak) - _psnr(base / peak, fx["fhat64"] / peak))
    nflip = int((r["sym"] != fx["symbols"].astype(np.int32)).sum()) + int((r["idx"] != fx["indexes"].astype(np.int32)).sum())
    print(f"{name}: vs the reference's fixture: streams identical {identical}, |d bytes| {abs(nb - nb_ref)}, |dPSNR of f_hat| {dpsnr:.3e} dB, "
          f"differing symbols + indexes {nflip}")
    path = os.environ.get("RGBD_RECORD_MASTER_FLOORS")
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
        with open(os.path.join(mc.GOLDEN, "master_latent_floors.json")) as f:
            fl = json.load(f)[name]
    if fl["identical"]:
        assert identical
    else:  # the measured values are the ceilings: must not regress
        assert abs(nb - nb_ref) <= fl["dbytes"], (abs(nb - nb_ref), fl["dbytes"])
        assert nflip <= fl["differing_decisions"], (nflip, fl["differing_decisions"])
        assert dpsnr <= max(2 * fl["dpsnr"], 1e-12), (dpsnr, fl["dpsnr"])


# ---- 6. forward() ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_forward(name):
    r = _run(name)
    fx, net = r["fx"], r["net"]
    B, H, W = mc.CASES[name][:3]
    fw = net.forward(r["f"], *r["ups"])
    assert set(fw) == {"f_hat", "likelihoods"} and set(fw["likelihoods"]) == {"y_likelihoods", "z_likelihoods"}
    assert tuple(fw["f_hat"].shape) == (B, mc.N, H, W)
    assert tuple(fw["likelihoods"]["y_likelihoods"].shape) == (B, mc.M, H // 16, W // 16)
    assert tuple(fw["likelihoods"]["z_likelihoods"].shape) == (B, mc.N, H // 64, W // 64)
    assert np.array_equal(_u32(net.debug_tensor("yhat")), _u32(r["t"]["yhat"]))  # forward's y_hat is compress's, part by part
    assert torch.equal(fw["f_hat"].cpu(), r["fh"])  # ... and so is its f_hat decompress's
    for k, key in (("y", "y_likelihoods"), ("z", "z_likelihoods")):
        lk = fw["likelihoods"][key]
        assert float(lk.min()) >= float(np.float32(1e-9)) and float(lk.max()) <= 1.0
        got, ref_bits, tol = float(-torch.log2(lk.double()).sum()), float(fx[f"lik_{k}_bits"]), mc.FACTOR * float(fx[f"lik_{k}_gap"])
        print(f"{name}: forward -log2 likelihood sum {k}: {got:.3f} vs the reference's {ref_bits:.3f}: relative {abs(got - ref_bits) / ref_bits:.2e}, "
              f"tolerance {tol:.2e} (8 x the reference's fp32 - fp64 gap)")
        assert abs(got - ref_bits) <= tol * ref_bits, (k, got, ref_bits, tol)


# ---- 7. guides matter -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "d"])
def test_guides_matter(name):
    r = _run(name)
    fx, net, ups = r["fx"], r["net"], r["ups"]
    for what, g in (("zeroed", [torch.zeros_like(u) for u in ups]), ("exchanged", list(mc.exchanged_guides(*ups)))):
        e = mc.fhat_err(name, net.decompress(r["out"]["strings"], r["out"]["shape"], *g)["f_hat"].cpu(), fx)
        print(f"{name}: guides {what}: f_hat {e:.2e} against the bound {mc.fhat_bound(fx):.2e}")
        assert e > mc.fhat_bound(fx), what


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_handle_usable():
    import rgbd_amd
    from rgbd_amd import synth

    r = _run("a")
    net, f, ups = r["net"], r["f"], r["ups"]
    L, h = lib(), net._h
    fh = torch.full((1, mc.N, 64, 64), 7.0, device="cuda")
    ly, lz = torch.full((1, mc.M, 4, 4), 7.0, device="cuda"), torch.full((1, mc.N, 1, 1), 7.0, device="cuda")
    p = [u.data_ptr() for u in ups]
    ys, zs = r["out"]["strings"]
    k1, py, ly_ = net._pack_strings(ys)
    k2, pz, lz_ = net._pack_strings(zs)

    def forward(hh=h, fp=f.data_ptr(), g=p, B=1, H=64, W=64, o=fh.data_ptr()):
        return L.rgbd_master_latent_forward(hh, fp, g[0], g[1], g[2], B, H, W, o, ly.data_ptr(), lz.data_ptr(), None)

    def decompress(hh=h, g=p, B=1, zh=1, zw=1, o=fh.data_ptr(), n_y=1):
        return L.rgbd_master_latent_decompress(hh, py, ly_, n_y, pz, lz_, B, zh, zw, g[0], g[1], g[2], o, None)

    assert forward(fp=None) == -22 and forward(o=None) == -22 and decompress(o=None) == -22
    for k in range(3):  # a guide pointer missing
        g = list(p)
        g[k] = None
        assert forward(g=g) == -22 and decompress(g=g) == -22
    assert forward(H=96) == -22 and forward(W=100) == -22 and forward(B=0) == -22
    assert decompress(zh=0) == -22 and decompress(B=0) == -22 and decompress(n_y=3, B=2) == -22
    assert L.rgbd_elic_compress_single(h, f.data_ptr(), 1, 64, 100, 0, None) == -22 and L.rgbd_elic_compress_single(h, None, 1, 64, 64, 0, None) == -22
    # the unguided single-modal calls and the wide coder on this handle
    assert L.rgbd_elic_forward_single(h, f.data_ptr(), 1, 64, 64, fh.data_ptr(), ly.data_ptr(), lz.data_ptr(), None) == -22
    assert L.rgbd_elic_decompress_single(h, py, ly_, 1, pz, lz_, 1, 1, 1, fh.data_ptr(), None) == -22
    assert L.rgbd_elic_set_coder(h, 1, 8) == -22
    with pytest.raises(NotImplementedError):
        net.set_coder("wide", 8)
    assert L.rgbd_synthesis_plus_forward(h, f.data_ptr(), p[0], p[1], p[2], 1, 4, 4, fh.data_ptr(), None) == -22
    # handles of family 1 (ELIC) and 13 (SynthesisTransformPlus) on the new entry points
    elic = rgbd_amd.ELIC(config=mc.config(), channel=3).eval()
    elic.load_state_dict(synth.synthetic_state_dict(1, config=mc.config(), model="ELIC", channel=3))
    elic.update(force=True)
    elic = elic.to("cuda")
    plus = rgbd_amd.SynthesisTransformPlus(192, 320, 192).to("cuda")
    for other in (elic._h, plus._h):
        assert forward(hh=other) == -22 and decompress(hh=other) == -22
    with pytest.raises((RgbdError, ValueError)):
        net.decompress([[ys[0], ys[0], ys[0]], [zs[0], zs[0]]], r["out"]["shape"], *ups)
    torch.cuda.synchronize()
    for t in (fh, ly, lz):
        assert float(t.min()) == 7.0 and float(t.max()) == 7.0
    del k1, k2
    # the handle works as before
    again = net.compress(f)
    assert again["strings"] == r["out"]["strings"]
    assert torch.equal(net.decompress(again["strings"], again["shape"], *ups)["f_hat"].cpu(), r["fh"])
