"""MLIC++ (rgbd_amd.mlic; reference models/mlicpp.py) on the GPU, on the five fixtures the unmodified reference produced
(tests/golden/mlic_*.npz, conditions asserted by tests/golden/make_mlic.py).  Three of them share one set of weights at three
shapes: 128x128 (8x8 latents), 448x192 (28x12: taller than wide, a 7x3 z grid, 336 tokens = linear-attention chunks of
128 / 128 / 80 and 128 / 40 per checkerboard half, 168 pixels per parity = ten full 16-pixel tiles of the fused parameter network
and one of eight, a 14x3 tile grid of the local attention) and 2 x 192x128 (12x8, a 3x2 z grid, one y stream and two z streams):

 (a) the two kernels of csrc/mlic_loop.hip alone against numpy: rgbd_mlic_lrp_apply and rgbd_mlic_slot_clear at 2x2, 3x5 and
     8x12 with B = 1, 2, both parities, on a slot in the middle of a wider buffer; every pixel of the other parity and every
     channel outside the slot keeps its bits; the updated values are rgbd_pw_half_tanh's followed by one fp32 add, bit for bit;
     refusals write nothing; the same at 2x182x361, past the kernels' grid cap (tests/gridcap_cases.py), and rgbd_pw_half_tanh
     itself past its own;
 (b) self-consistency, asserted hard: decompress(compress(x)) returns and the decoder's y_hat is the encoder's bit for bit;
     image b of a batch and the image alone give the same streams; three calls in a row give the same streams; a replayed
     HIP graph gives what the eager call gave;
 (c) the layered contract: y, and y_hat under the reference's symbols, within 8 * e_ref of the fp64 restatement's, e_ref = the
     reference's own fp32 distance from it at that tensor (recorded in the fixture); the z symbols are the reference's;
 (d) a teacher-forced census: with the reference's symbols forced, a decision that differs from the reference's is accepted
     only where the fp64 restatement's distance to the rounding / scale-bin boundary is below that tensor's float bound;
 (e) free-running identity with the reference: measured, recorded by RGBD_RECORD_MLIC_FLOORS=<path> into
     tests/golden/mlic_floors.json, asserted where the recording run observed it (the measured values are ceilings);
 (f) forward(): keys, and likelihood sums against the fixture within 8 * the reference's own fp32 - fp64 gap;
 (g) every refusal: nothing is written and the handle works afterwards;
 (h) one model across shapes: small, large (the workspace regrows), batch of two, small (a larger call's leftovers in the
     workspace), large, small, eagerly and then through the per-shape graph cache on a side stream: every call gives the bits of
     a model that never saw another shape;
 (i) the single-image tester on two files of different sizes, building the model itself from its name and a checkpoint file.
"""
import json
import os

import numpy as np
import pytest
import torch

import gridcap_cases as gc
from gpu_utils import require_gpu
from rgbd_amd import MLICPlusPlus, RgbdError, synth  # (the feature: without it this import fails)
from rgbd_amd._lib import lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["s2_128x128", "s3_b2_128x192", "full_128x128", "s2_448x192", "s2_b2_192x128"]
SHAPES_OF_ONE_MODEL = ["s2_128x128", "s2_448x192", "s2_b2_192x128"]  # small, large, batch of two: one set of weights, key (3, 64, 64)
FACTOR = 8.0
_NETS, _RUNS, _FORCED = {}, {}, {}


def _fixture(name):
    return np.load(os.path.join(GOLDEN, f"mlic_{name}.npz"))


def _key(g):
    return int(g["seed"]), int(g["N"]), int(g["M"])


def _fresh_net(key):
    require_gpu()
    m = MLICPlusPlus(N=key[1], M=key[2], slice_num=key[2] // 32).eval()
    m.load_state_dict(synth.synthetic_state_dict(key[0], model="MLIC", N=key[1], M=key[2]), strict=True)
    assert m.update(force=True)
    return m.to("cuda")


def _net(key):
    """One model per configuration for the whole module (the full configuration's weights are large)."""
    if key not in _NETS:
        _NETS[key] = _fresh_net(key)
    return _NETS[key]


def _images(g):
    r, _ = synth.synthetic_batch(int(g["B"]), int(g["H"]), int(g["W"]), config_id=int(g["config_id"]))
    return torch.from_numpy(r)


def _sub(t):  # make_mlic.y_sub
    return t[:, ::8, ::2, ::2]


def _rel(a, ref64):
    a, ref64 = np.asarray(a, np.float64), np.asarray(ref64, np.float64)
    return float(np.abs(a - ref64).max() / np.abs(ref64).max())


def _psnr(a, b):
    return float(-10 * np.log10(torch.mean((a - b) ** 2).item()))


def _run(name):
    """One free-running compress + decompress of a fixture, shared by the tests."""
    if name not in _RUNS:
        g = _fixture(name)
        net = _net(_key(g))
        x = _images(g)
        out = net.compress(x.cuda())
        t = {k: net.debug_tensor(k).copy() for k in ("y", "yhat")}
        sym, idx = net.debug_symbols(0)
        sym, idx = sym.copy(), idx.copy()
        rec = net.decompress(out["strings"], out["shape"])
        _RUNS[name] = dict(g=g, net=net, x=x, out=out, t=t, sym=sym, idx=idx, xh=rec["x_hat"].cpu(), rec_keys=set(rec), yhat_dec=net.debug_tensor("yhat").copy())
    return _RUNS[name]


def _forced(name):
    """One compress under the reference's symbols (teacher forcing): every part sees the reference's context."""
    if name not in _FORCED:
        g = _fixture(name)
        net = _net(_key(g))
        net.set_forced_symbols(0, g["symbols"].astype(np.int32), g["z_symbols"].astype(np.int32).reshape(-1))
        net.set_debug_floats(True)
        try:
            net.compress(_images(g).cuda())
            gx, gs = net.debug_floats(0)
            sym, idx = net.debug_symbols(0)
            _FORCED[name] = dict(x=gx.copy(), s=gs.copy(), sym=sym.copy(), idx=idx.copy(), yhat=net.debug_tensor("yhat").copy())
        finally:
            net.set_debug_floats(False)
            net.set_forced_symbols(0, None, None)
    return _FORCED[name]


# ---- (a) the kernels alone ----------------------------------------------------------------------------------------------------
def _anchor(h, w):
    r, c = np.arange(h)[:, None], np.arange(w)[None, :]
    return (r + c) % 2 == 1


def _half_tanh(r):
    """rgbd_pw_half_tanh on a contiguous [npix, 32] tensor: the module's own tail, on the device."""
    out = torch.empty_like(r)
    assert lib().rgbd_pw_half_tanh(r.data_ptr(), 32, out.data_ptr(), 32, r.numel() // 32, 32, None) == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("h,w", [(2, 2), (3, 5), (8, 12)])
def test_slot_kernels_alone(h, w, B):
    dev = require_gpu()
    gen = torch.Generator().manual_seed(100 * h + 10 * w + B)
    cs, c0 = 96, 32  # a 32-channel slot in the middle of a 96-channel buffer
    for parity in (0, 1):
        mask = _anchor(h, w) if parity == 0 else ~_anchor(h, w)
        buf0 = (torch.randn(B, h, w, cs, generator=gen) * 4).to(dev)
        r = (torch.randn(B, h, w, 32, generator=gen) * 1.5).to(dev)
        # lrp_apply
        buf = buf0.clone()
        assert lib().rgbd_mlic_lrp_apply(buf.data_ptr() + 4 * c0, cs, r.data_ptr(), 32, 32, B, h, w, parity, None) == 0
        torch.cuda.synchronize()
        want = buf0.clone()
        upd = (buf0[..., c0:c0 + 32] + _half_tanh(r)).cpu().numpy()  # one fp32 add of the module's value
        wn = want.cpu().numpy()
        wn[:, mask, c0:c0 + 32] = upd[:, mask]
        got = buf.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), wn.view(np.uint32)), (h, w, B, parity)
        # ... and against numpy's tanh: the device's tanhf is within a few ulp of it
        ref = buf0.cpu().numpy()[..., c0:c0 + 32].astype(np.float64) + 0.5 * np.tanh(r.cpu().numpy().astype(np.float64))
        assert np.abs(got[:, mask, c0:c0 + 32] - ref[:, mask]).max() <= 4 * 2.0 ** -24 * (np.abs(ref).max() + 0.5)
        # slot_clear
        buf = buf0.clone()
        assert lib().rgbd_mlic_slot_clear(buf.data_ptr() + 4 * c0, cs, 32, B, h, w, parity, None) == 0
        torch.cuda.synchronize()
        wn = buf0.cpu().numpy()
        wn[:, mask, c0:c0 + 32] = 0.0
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), wn.view(np.uint32)), (h, w, B, parity)
        # refusals write nothing: another channel count, a stride that is no multiple of 4, a misaligned pointer, h or w of zero
        buf = buf0.clone()
        for args in ((buf.data_ptr() + 4 * c0, cs, 16, B, h, w), (buf.data_ptr() + 4 * c0, cs - 2, 32, B, h, w),
                     (buf.data_ptr() + 4 * c0 + 4, cs, 32, B, h, w), (buf.data_ptr() + 4 * c0, cs, 32, B, 0, w),
                     (buf.data_ptr() + 4 * c0, cs, 32, B, h, 0), (buf.data_ptr() + 4 * c0, 16, 32, B, h, w)):
            assert lib().rgbd_mlic_slot_clear(args[0], args[1], args[2], args[3], args[4], args[5], parity, None) == -22
            assert lib().rgbd_mlic_lrp_apply(args[0], args[1], r.data_ptr(), 32, args[2], args[3], args[4], args[5], parity, None) == -22
        assert lib().rgbd_mlic_lrp_apply(buf.data_ptr() + 4 * c0, cs, r.data_ptr(), 30, 32, B, h, w, parity, None) == -22
        assert lib().rgbd_mlic_slot_clear(buf.data_ptr() + 4 * c0, cs, 32, B, h, w, 2, None) == -22
        torch.cuda.synchronize()
        assert torch.equal(buf, buf0)


@pytest.mark.parametrize("case", gc.MLIC_CASES, ids=lambda c: "%(B)dx%(h)dx%(w)d" % c)
def test_slot_kernels_past_the_grid_cap(case):
    """Both kernels at 2 x 182 x 361 (527 072 quads against the 2048 x 256 grid cap: two sweeps, the second one ragged; an odd
    width), both parities, under test_slot_kernels_alone's rules: the whole 96-channel buffer bit for bit after ONE call -- an
    element updated in two sweeps would carry 0.5 * tanh twice -- and the same bits from a second call on a fresh copy."""
    dev = require_gpu()
    B, h, w = case["B"], case["h"], case["w"]
    cs, c0 = gc.MLIC_CS, gc.MLIC_C0
    buf0, r = gc.mlic_inputs(case)
    rd, b0 = torch.from_numpy(r).to(dev), torch.from_numpy(buf0).to(dev)
    bc = gc.build_mlic(case, _anchor, buf0, r, _half_tanh(rd).cpu().numpy())
    for parity in (0, 1):
        for kernel in ("lrp_apply", "slot_clear"):
            outs = []
            for _ in range(2):
                buf = b0.clone()
                if kernel == "lrp_apply":
                    assert lib().rgbd_mlic_lrp_apply(buf.data_ptr() + 4 * c0, cs, rd.data_ptr(), 32, 32, B, h, w, parity, None) == 0
                else:
                    assert lib().rgbd_mlic_slot_clear(buf.data_ptr() + 4 * c0, cs, 32, B, h, w, parity, None) == 0
                torch.cuda.synchronize()
                outs.append(buf.cpu().numpy())
            assert bc["stages"][f"{kernel}_p{parity}"]["accept"]({"buf": outs[0]}) == [], (kernel, parity)
            assert gc.same_bits(outs[0], outs[1]), (kernel, parity)


@pytest.mark.parametrize("case", gc.HALF_TANH_CASES, ids=lambda c: "%(npix)d" % c)
def test_half_tanh_past_the_grid_cap(case):
    """rgbd_pw_half_tanh (the reference of the slot tests above) itself, past its grid cap and between two unequal strides:
    against numpy's 0.5 * tanh under test_slot_kernels_alone's bound; the channels behind C keep the pre-fill; NaN in the
    input's pads; two calls, the same bits."""
    dev = require_gpu()
    bc = gc.build_half_tanh(case)
    xd = torch.from_numpy(bc["x"]).to(dev)
    outs = []
    for _ in range(2):
        y = torch.full((case["npix"], case["ycs"]), float(gc.HALF_TANH_SENT), device=dev)
        assert lib().rgbd_pw_half_tanh(xd.data_ptr(), case["xcs"], y.data_ptr(), case["ycs"], case["npix"], case["C"], None) == 0
        torch.cuda.synchronize()
        outs.append(y.cpu().numpy())
    assert bc["stages"]["half_tanh"]["accept"]({"y": outs[0]}) == []
    assert gc.same_bits(outs[0], outs[1])


# ---- (b) self-consistency -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_decoder_rebuilds_the_encoders_yhat_bit_for_bit(name):
    r = _run(name)
    g = r["g"]
    assert r["rec_keys"] == {"x_hat"}  # (no cost_time in either direction)
    assert set(r["out"]) == {"strings", "shape"} and tuple(r["out"]["shape"]) == tuple(int(v) for v in g["shape"])
    assert len(r["out"]["strings"][0]) == 1 and len(r["out"]["strings"][1]) == int(g["B"])
    assert r["xh"].shape == r["x"].shape and bool(torch.isfinite(r["xh"]).all())
    assert np.array_equal(r["yhat_dec"].view(np.uint32), r["t"]["yhat"].view(np.uint32))  # through 2 * slice_num dependent parts
    # the symbols are the roundings of what the encoder kept, and y_hat - symbol is the mean it used
    S, B, h, w = int(g["slice_num"]), int(g["B"]), int(g["H"]) // 16, int(g["W"]) // 16
    assert r["sym"].size == B * 32 * S * h * w


@pytest.mark.parametrize("name", CASES)
def test_three_calls_in_a_row_give_the_same_streams(name):
    r = _run(name)
    for _ in range(3):
        assert r["net"].compress(r["x"].cuda())["strings"] == r["out"]["strings"]


@pytest.mark.parametrize("name", ["s3_b2_128x192", "s2_b2_192x128"])
def test_image_of_a_batch_and_alone_give_the_same_streams(name):
    r = _run(name)
    net, x = r["net"], r["x"].cuda()
    ones = [net.compress(x[i:i + 1]) for i in range(2)]
    net.per_image_streams = True
    try:
        pi = net.compress(x)
        assert len(pi["strings"][0]) == 2 and len(pi["strings"][1]) == 2
        for i in range(2):
            assert pi["strings"][0][i] == ones[i]["strings"][0][0] and pi["strings"][1][i] == ones[i]["strings"][1][0]
            assert r["out"]["strings"][1][i] == ones[i]["strings"][1][0]
        rp = net.decompress(pi["strings"], pi["shape"])
        assert torch.equal(rp["x_hat"].cpu(), r["xh"])  # the same bits for an image alone, in per-image streams and in one stream
    finally:
        net.per_image_streams = False


def test_captured_replay_equals_the_eager_call():
    r = _run("s2_128x128")
    net = r["net"].clone_shared()
    x = r["x"].cuda()

    def round_trip():
        out = net.compress(x)
        rec = net.decompress(out["strings"], out["shape"])
        fw = net.forward(x)
        return out["strings"], rec["x_hat"].clone(), fw["x_hat"].clone(), fw["likelihoods"]["y_likelihoods"].clone()

    with torch.cuda.stream(torch.cuda.Stream()):  # (the NULL stream cannot be captured)
        first = round_trip()  # eager: first call of the shape
        assert first[0] == r["out"]["strings"] and torch.equal(first[1].cpu(), r["xh"])
        for _ in range(3):
            again = round_trip()
            assert again[0] == first[0] and all(torch.equal(a, b) for a, b in zip(again[1:], first[1:]))
        assert net.graph_count() >= 3  # compress, decompress and forward of this shape replay
    torch.cuda.synchronize()


# ---- (h) one model across shapes ------------------------------------------------------------------------------------------------
def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _alone(name):
    """What a model that never sees another shape gives for a fixture's image: the yardstick of test_one_model_across_shapes."""
    g = _fixture(name)
    assert _key(g) == (3, 64, 64)
    net, x = _fresh_net(_key(g)), _images(g).cuda()
    out = net.compress(x)
    yhat = _u32(net.debug_tensor("yhat")).copy()
    rec = net.decompress(out["strings"], out["shape"])
    assert np.array_equal(_u32(net.debug_tensor("yhat")), yhat)
    fw = net.forward(x)
    assert np.array_equal(_u32(net.debug_tensor("yhat")), yhat)
    want = dict(x=x, strings=out["strings"], shape=tuple(out["shape"]), yhat=yhat, xh=rec["x_hat"].cpu(), fw_xh=fw["x_hat"].cpu(),
                fw_ly=fw["likelihoods"]["y_likelihoods"].cpu(), fw_lz=fw["likelihoods"]["z_likelihoods"].cpu())
    assert all(bool(torch.isfinite(want[k]).all()) for k in ("xh", "fw_xh", "fw_ly", "fw_lz"))
    return want


def _same_compress(net, want, where):
    out = net.compress(want["x"])
    assert out["strings"] == want["strings"] and tuple(out["shape"]) == want["shape"], where
    assert np.array_equal(_u32(net.debug_tensor("yhat")), want["yhat"]), where


def _same_decompress(net, want, where):
    rec = net.decompress(want["strings"], want["shape"])
    assert np.array_equal(_u32(net.debug_tensor("yhat")), want["yhat"]), where
    assert torch.equal(rec["x_hat"].cpu(), want["xh"]), where


def _same_forward(net, want, where):
    fw = net.forward(want["x"])
    assert np.array_equal(_u32(net.debug_tensor("yhat")), want["yhat"]), where
    assert torch.equal(fw["x_hat"].cpu(), want["fw_xh"]), where
    assert torch.equal(fw["likelihoods"]["y_likelihoods"].cpu(), want["fw_ly"]), where
    assert torch.equal(fw["likelihoods"]["z_likelihoods"].cpu(), want["fw_lz"]), where


def test_one_model_across_shapes():
    """Three models that each see one shape only (128x128, 448x192, 2 x 192x128; one set of weights) are the yardstick.  A fourth
    model sees the shapes in turn: its workspace regrows at the first large call, and from then on every call finds what a call
    of another shape left there -- the state buffer [B, h, w, 2M] included, whose slots are only written as they are decoded.
    Every call gives the bits of the model that never saw another shape: streams, y_hat as uint32, x_hat under torch.equal.
    Eagerly on the current stream first, then on a side stream through the per-shape graph cache (eager, captured, replayed)."""
    small, large, two = (_alone(n) for n in SHAPES_OF_ONE_MODEL)
    net = _fresh_net((3, 64, 64))
    sizes = []
    for step, (want, forward) in enumerate(((small, False), (large, True), (two, False), (small, True), (large, False), (small, False)), 1):
        _same_compress(net, want, ("compress", step))
        if step == 5:  # the small streams behind a large compress(), with no call of the small shape in between
            _same_decompress(net, small, ("decompress of the small streams", step))
        _same_decompress(net, want, ("decompress", step))
        if forward:
            _same_forward(net, want, ("forward", step))
        sizes.append(net.workspace_bytes())
    assert sizes[1] > sizes[0] and sizes[1:] == [sizes[1]] * 5, sizes  # the workspace grew at step 2, and only there
    # on a side stream (the NULL stream is not captured: test_captured_replay_equals_the_eager_call)
    clone = net.clone_shared()
    with torch.cuda.stream(torch.cuda.Stream()):
        for rnd in range(3):
            for want in (small, large, two):
                _same_compress(clone, want, ("compress, side stream", rnd))
                _same_decompress(clone, want, ("decompress, side stream", rnd))
                _same_forward(clone, want, ("forward, side stream", rnd))
        assert clone.graph_count() >= 3
    torch.cuda.synchronize()


# ---- (c) layered contract -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_layered_contract(name):
    r, f = _run(name), _forced(name)
    g = r["g"]
    e_y, e_yhat = _rel(_sub(r["t"]["y"]), g["y_sub64"]), _rel(_sub(f["yhat"]), g["yhat_sub64"])
    print(f"{name}: y {e_y:.2e} (bound {FACTOR} * {float(g['e_ref_y']):.2e}), y_hat under the reference's symbols {e_yhat:.2e} "
          f"(bound {FACTOR} * {float(g['e_ref_yhat']):.2e})")
    zsym = np.rint(r["net"].debug_tensor("z") - np.asarray(r["net"].eb_medians_numpy()[0]).reshape(1, -1, 1, 1)).astype(np.int16)
    assert np.array_equal(zsym, g["z_symbols"])
    assert [bytes(s) for s in r["out"]["strings"][1]] == [g[f"z{i}"].tobytes() for i in range(int(g["B"]))]
    assert e_y <= FACTOR * float(g["e_ref_y"])
    assert e_yhat <= FACTOR * float(g["e_ref_yhat"])


# ---- (d) teacher-forced census ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_teacher_forced_census(name):
    g, f = _fixture(name), _forced(name)
    rsym, ridx = g["symbols"].astype(np.int32), g["indexes"].astype(np.int32)
    x64, s64 = g["x64"], g["sigma64"]
    table = synth_scale_table()
    # float bounds of the two tensors a decision reads, absolute: 8 * e_ref * max |fp64|
    bx, bs = FACTOR * float(g["e_ref_x"]) * np.abs(x64).max(), FACTOR * float(g["e_ref_sigma"]) * np.abs(s64).max()
    d_round = 0.5 - np.abs(x64 - np.rint(x64))                            # distance of y - mean to the rounding boundary
    d_scale = np.abs(s64[:, None] - table[None, :-1]).min(axis=1)  # ... of the scale to a table entry (below table[0] = the bound
    # 0.11 a scale indexes row 0 until it crosses that entry)
    dsym, didx = f["sym"] != rsym, f["idx"] != ridx
    ex, es = np.abs(f["x"] - x64).max(), np.abs(f["s"] - s64).max()
    print(f"{name}: forced census: {int(dsym.sum())} symbols and {int(didx.sum())} scale indexes of {rsym.size} differ from the "
          f"reference's; decisions within the float bound of a boundary: {int((d_round < bx).sum())} + {int((d_scale < bs).sum())}; "
          f"max |d(y - mean)| {ex:.2e} (bound {bx:.2e}), max |d scale| {es:.2e} (bound {bs:.2e})")
    assert not (dsym & ~(d_round < bx)).any(), "a symbol differs from the reference's away from a rounding boundary"
    assert not (didx & ~(d_scale < bs)).any(), "a scale index differs from the reference's away from a table entry"
    assert ex <= bx and es <= bs


def synth_scale_table():
    from rgbd_amd.entropy_models import get_scale_table

    return np.asarray(get_scale_table(), np.float32).astype(np.float64)


# ---- (e) free-running identity with the reference: measured floors ------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_identity_with_the_reference(name):
    r = _run(name)
    g, out, x = r["g"], r["out"], r["x"]
    B = int(g["B"])
    identical = out["strings"][0][0] == g["y_stream"].tobytes() and all(out["strings"][1][i] == g[f"z{i}"].tobytes() for i in range(B))
    nb = len(out["strings"][0][0]) + sum(len(s) for s in out["strings"][1])
    nb_ref = g["y_stream"].shape[0] + sum(g[f"z{i}"].shape[0] for i in range(B))
    dpsnr = abs(_psnr(r["xh"], x) - float(g["psnr"]))
    nflip = int((r["sym"] != g["symbols"].astype(np.int32)).sum()) + int((r["idx"] != g["indexes"].astype(np.int32)).sum())
    print(f"{name}: vs the reference's fixture: streams identical {identical}, |d bytes| {abs(nb - nb_ref)}, |dPSNR| {dpsnr:.3e} dB, "
          f"differing symbols + indexes {nflip}")
    path = os.environ.get("RGBD_RECORD_MLIC_FLOORS")
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
        with open(os.path.join(GOLDEN, "mlic_floors.json")) as f:
            fl = json.load(f)[name]
    if fl["identical"]:
        assert identical
    else:  # the measured values are the ceilings: must not regress
        assert abs(nb - nb_ref) <= fl["dbytes"], (abs(nb - nb_ref), fl["dbytes"])
        assert nflip <= fl["differing_decisions"], (nflip, fl["differing_decisions"])
        assert dpsnr <= max(2 * fl["dpsnr"], 1e-12), (dpsnr, fl["dpsnr"])


# ---- (f) forward() --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_forward(name):
    r = _run(name)
    g, net, x = r["g"], r["net"], r["x"]
    fw = net.forward(x.cuda())
    assert set(fw) == {"x_hat", "likelihoods"} and set(fw["likelihoods"]) == {"y_likelihoods", "z_likelihoods"}
    assert fw["x_hat"].shape == x.shape
    yh = net.debug_tensor("yhat")
    assert np.array_equal(yh.view(np.uint32), r["t"]["yhat"].view(np.uint32))  # forward's y_hat is compress's, part by part
    for k, key in (("y", "y_likelihoods"), ("z", "z_likelihoods")):
        lk = fw["likelihoods"][key]
        assert float(lk.min()) >= float(np.float32(1e-9)) and float(lk.max()) <= 1.0
        got, ref_bits, tol = float(-torch.log2(lk.double()).sum()), float(g[f"lik_{k}_bits"]), FACTOR * float(g[f"lik_{k}_gap"])
        print(f"{name}: forward -log2 likelihood sum {k}: {got:.3f} vs the reference's {ref_bits:.3f}: relative {abs(got - ref_bits) / ref_bits:.2e}, "
              f"tolerance {tol:.2e} (8 * the reference's fp32 - fp64 gap)")
        assert abs(got - ref_bits) <= tol * ref_bits, (k, got, ref_bits, tol)


# ---- (i) the tester on files ----------------------------------------------------------------------------------------------------
def test_tester_single_on_files_mlic(tmp_path, monkeypatch):
    """testing/tester_single.py with `-m MLIC --channel 3` and a checkpoint file: the tester itself looks the class up by name and
    builds it from the configuration (tester.py get_net, net=None), and its loop changes shape between the two files."""
    import types

    from PIL import Image

    import rgbd_amd

    require_gpu()
    root = tmp_path / "nyu_test"
    (root / "rgb").mkdir(parents=True)
    sizes = [(100, 150), (150, 100)]  # replicate0 pads them to 128 x 192 and 192 x 128
    for i, (H, W) in enumerate(sizes):
        r, _ = synth.synthetic_pair(i, H, W, config_id=6, smooth=True)
        Image.fromarray((r.transpose(1, 2, 0) * 255).astype(np.uint8)).save(root / "rgb" / f"{i:04d}.png")
    ckpt = tmp_path / "checkpoint.pth.tar"
    torch.save({"state_dict": synth.synthetic_state_dict(3, model="MLIC", N=64, M=64), "epoch": 7}, ckpt)
    work = tmp_path / "work"  # (the tester writes to ../experiments)
    work.mkdir()
    monkeypatch.chdir(work)
    args = types.SimpleNamespace(channel=3, debug=False, experiment=None, dataset=str(root), model="MLIC", quality="1",
                                 checkpoint=str(ckpt))
    t = rgbd_amd.TesterSingle(args, rgbd_amd.arch.mlic_config(64, 64, 2), net=None)
    assert t.exp_name == "nyuv2_rgb_MLIC_1"
    assert type(t.net) is MLICPlusPlus and (t.net.N, t.net.M, t.net.slice_num, t.net.channel) == (64, 64, 2, 3) and t.epoch == 7
    rows, meters = t.test_model(padding_mode="replicate0", padding=True)
    rec_dir = t.get_rec_dir(padding=True, padding_mode="replicate0")
    assert os.path.basename(rec_dir) == "7-padding-replicate0" and os.path.isdir(tmp_path / "experiments" / t.exp_name)
    assert len(rows) == 2 and len(os.listdir(os.path.join(rec_dir, "rgb_rec"))) == 2
    direct = _net((3, 64, 64))  # the same weights, loaded without the checkpoint file
    for i, ((H, W), row) in enumerate(zip(sizes, rows)):
        assert row["name"] == f"{i:04d}"
        assert row["bpp"] == os.path.getsize(os.path.join(rec_dir, "rgb_bin", row["name"])) * 8.0 / (H * W)
        assert np.isfinite(row["psnr"]) and row["enc_time"] > 0 and row["dec_time"] > 0
        img, name = t.test_dataloader[i]
        xp = rgbd_amd.datautils.pad(img.cuda(), "replicate0")
        assert tuple(xp.shape[2:]) == (128 + 64 * i, 192 - 64 * i)
        out = direct.compress(xp)
        rec = direct.decompress(out["strings"], out["shape"])
        xh, _ = t.decompress_one_image(os.path.join(rec_dir, "rgb_bin"), name[0], mode="replicate0")
        assert torch.equal(xh, rec["x_hat"][:, :, :H, :W])


# ---- (g) refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_handle_usable():
    r = _run("s2_128x128")
    net, x = r["net"], r["x"].cuda()
    L, h = lib(), net._h
    out = torch.full((1, 3, 128, 128), 7.0, device="cuda")
    lik = torch.full((1, 64, 8, 8), 7.0, device="cuda")
    small = torch.zeros(1, 3, 64, 128, device="cuda")
    # image sides below 128 (a one-row z map) or no multiples of 64: refused by the C ABI before any launch
    for H, W in ((64, 128), (128, 64), (100, 128)):
        assert L.rgbd_elic_compress_single(h, small.data_ptr(), 1, H, W, 0, None) == -22
        assert L.rgbd_elic_forward_single(h, small.data_ptr(), 1, H, W, out.data_ptr(), lik.data_ptr(), lik.data_ptr(), None) == -22
    ys, zs = r["out"]["strings"]
    k1, py, ly = net._pack_strings(ys)
    k2, pz, lz = net._pack_strings(zs)
    assert L.rgbd_elic_decompress_single(h, py, ly, 1, pz, lz, 1, 1, 2, out.data_ptr(), None) == -22
    # the wide coder
    assert L.rgbd_elic_set_coder(h, 1, 8) == -22
    with pytest.raises(RgbdError):
        net.set_coder("wide", 8)
    assert net.coder == "reference"
    # module-handle calls on a codec handle, and the two-modality calls
    assert L.rgbd_lrp_forward(h, x.data_ptr(), 1, 8, 8, out.data_ptr(), None) == -22
    assert L.rgbd_local_context_forward(h, x.data_ptr(), 1, 8, 8, out.data_ptr(), None) == -22
    assert L.rgbd_channel_context_forward(h, x.data_ptr(), 1, 8, 8, out.data_ptr(), None) == -22
    assert L.rgbd_elic_compress(h, x.data_ptr(), x.data_ptr(), 1, 128, 128, 0, None) != 0
    # codec calls on a module handle (unchanged)
    import rgbd_amd

    lrp = rgbd_amd.LatentResidualPrediction(96, 32).to("cuda")
    assert L.rgbd_elic_compress_single(lrp._h, x.data_ptr(), 1, 128, 128, 0, None) == -22
    # a stream that does not fit the model: a shape the streams were not made for, a stream count that is neither 1 nor B
    with pytest.raises((RgbdError, ValueError)):
        net.decompress([[ys[0], ys[0], ys[0]], [zs[0], zs[0]]], r["out"]["shape"])
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0 and float(lik.min()) == 7.0 and float(lik.max()) == 7.0
    del k1, k2
    # the handle works as before
    again = net.compress(x)
    assert again["strings"] == r["out"]["strings"]
    assert torch.equal(net.decompress(again["strings"], again["shape"])["x_hat"].cpu(), r["xh"])
