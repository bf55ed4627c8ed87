"""The models' stream-format switch (set_coder): under "wide" the y strings of ELIC_united and the single-modal ELIC are tagged
wide-rANS streams that decode to the very x_hat of the reference-format round trip; the z strings, and everything under
"reference", stay as they were.  The other codec families refuse the switch before anything is launched.

Shapes: 64x64 and 128x192 for both models, B = 1 and 2, lanes 16 and 64.  ELIC_united is not defined at 64x64 in any stream
format: its ESA blocks max-pool 7x7 / 3 behind an unpadded stride-2 conv (modules/transform/attention.py:77,88), which needs a
15-row feature map where a 64-row image has 8 -- PyTorch raises there, and so does this engine (RGBD_EINVAL from the pooling
launcher, as before this switch existed).  On that one case the test holds the two coders to the same refusal; 128x128, the
model's smallest size, is in the list so that ELIC_united is compared bit for bit on two shapes all the same."""
import ctypes

import pytest
import torch

from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

EINVAL = -22
SHAPES = [(64, 64), (128, 128), (128, 192)]
UNDEFINED = {("ELIC_united", 64, 64)}  # the model itself cannot run there (see above)


@pytest.fixture(scope="module")
def nets():
    require_gpu()
    import rgbd_amd
    from rgbd_amd import synth

    out = {}
    for name, channel in (("ELIC_united", 4), ("ELIC", 3)):
        m = rgbd_amd.modelZoo[name](config=rgbd_amd.model_config(), channel=channel).eval()
        m.load_state_dict(synth.synthetic_state_dict(0, model=name), strict=True)
        assert m.update(force=True)
        out[name] = m.to("cuda")
    return out


def _inputs(name, B, H, W):
    from rgbd_amd import synth

    r, d = synth.synthetic_batch(B, H, W, config_id=3)
    r, d = torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda()
    return (r, d) if name == "ELIC_united" else (r,)


def _compress(net, name, x):
    """-> (the call's result, y strings per modality, z strings per modality)"""
    out = net.compress(*x)
    if name == "ELIC_united":
        return out, [out["r_strings"][0], out["d_strings"][0]], [out["r_strings"][1], out["d_strings"][1]]
    return out, [out["strings"][0]], [out["strings"][1]]


def _decompress(net, name, out):
    if name == "ELIC_united":
        rec = net.decompress(out["r_strings"], out["d_strings"], out["shape"])
        return [rec["x_hat"]["r"].cpu(), rec["x_hat"]["d"].cpu()]
    return [net.decompress(out["strings"], out["shape"])["x_hat"].cpu()]


_reference = {}


def _reference_trip(net, name, B, H, W):
    """Three calls of the shape under "reference" (eager, captured, replayed): computed once per shape, shared by the lanes."""
    key = (name, B, H, W)
    if key not in _reference:
        net.set_coder("reference")
        x = _inputs(name, B, H, W)
        trips = []
        for _ in range(3):
            out, ys, zs = _compress(net, name, x)
            trips.append((ys, zs, _decompress(net, name, out)))
        for ys, zs, xh in trips[1:]:
            assert ys == trips[0][0] and zs == trips[0][1]
            assert all(torch.equal(a, b) for a, b in zip(xh, trips[0][2]))
        _reference[key] = trips[0]
    return _reference[key]


@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("name", ["ELIC_united", "ELIC"])
def test_wide_round_trip_equals_reference(nets, name, H, W, B, lanes):
    net = nets[name]
    if (name, H, W) in UNDEFINED:
        from rgbd_amd._lib import RgbdError

        x = _inputs(name, B, H, W)
        try:
            for coder in ("reference", "wide", "reference"):
                net.set_coder(coder, lanes=lanes)
                with pytest.raises(RgbdError, match="invalid argument"):
                    net.compress(*x)
        finally:
            net.set_coder("reference")
        return
    try:
        ref_ys, ref_zs, ref_xhat = _reference_trip(net, name, B, H, W)
        x = _inputs(name, B, H, W)
        net.set_coder("wide", lanes=lanes)
        assert net.coder == "wide" and net.coder_lanes == lanes
        tag = b"RW\x01" + bytes([lanes])
        first = None
        for call in range(3):  # eager, captured, replayed
            out, ys, zs = _compress(net, name, x)
            assert zs == ref_zs  # the z strings keep the reference format
            for m, (got, ref) in enumerate(zip(ys, ref_ys)):
                assert len(got) == len(ref)
                for g, r in zip(got, ref):
                    assert g[:4] == tag
                    print(f"{name} {H}x{W} B={B} L={lanes} mod {m}: wide {len(g)} bytes, reference {len(r)}")
                    assert len(g) <= len(r) + 4 + 8 * (lanes - 1) + 8
            xhat = _decompress(net, name, out)
            for a, b in zip(xhat, ref_xhat):
                assert torch.equal(a, b)  # same symbols, same y_hat, same bits
            if first is None:
                first = ys
            assert ys == first, call
        # a reference string, or a string of other lanes, is refused on the host
        ref_out = dict(out)
        if name == "ELIC_united":
            ref_out["r_strings"] = [ref_ys[0], ref_zs[0]]
        else:
            ref_out["strings"] = [ref_ys[0], ref_zs[0]]
        with pytest.raises(ValueError):
            _decompress(net, name, ref_out)
        net.set_coder("wide", lanes=32)
        with pytest.raises(ValueError):
            _decompress(net, name, out)
        # and back: the first reference bytes again
        net.set_coder("reference")
        assert net.coder == "reference"
        out, ys, zs = _compress(net, name, x)
        assert ys == ref_ys and zs == ref_zs
        assert all(torch.equal(a, b) for a, b in zip(_decompress(net, name, out), ref_xhat))
    finally:
        net.set_coder("reference")


def test_set_coder_arguments(nets):
    net = nets["ELIC"]
    for bad in (0, 3, 65, 128):
        with pytest.raises(ValueError):
            net.set_coder("wide", lanes=bad)
    with pytest.raises(ValueError):
        net.set_coder("fast")
    assert net.coder == "reference"
    sd = net.state_dict()
    net.set_coder("wide", lanes=16)
    assert list(net.state_dict()) == list(sd)  # the switch is no part of the checkpoint
    net.set_coder("reference")


def test_engine_setter_per_family():
    """rgbd_elic_set_coder: ELIC_united (0) and ELIC (1) take the wide coder; STF_united (2), ELIC_united_R2D (3), STF (4), the
    checkerboard Cheng2020 (5) and the stand-alone modules (6 ... 9) refuse it with RGBD_EINVAL before anything is launched --
    no family emits reference streams under a "wide" switch."""
    require_gpu()
    from rgbd_amd._lib import lib

    L = lib()

    def i32(*v):
        return (ctypes.c_int32 * len(v))(*v)

    s320, s384 = i32(16, 16, 32, 64, 192), i32(24, 24, 48, 96, 192)
    for family in range(10):
        h = ctypes.c_void_p()
        out = ctypes.byref(h)
        rc = {0: lambda: L.rgbd_elic_create(192, 320, s320, 5, out), 1: lambda: L.rgbd_elic_create_single(192, 320, s320, 5, 3, out),
              2: lambda: L.rgbd_elic_create_stf(192, 384, s384, 5, out), 3: lambda: L.rgbd_elic_create_r2d(192, 320, s320, 5, out),
              4: lambda: L.rgbd_elic_create_stf_single(3, out), 5: lambda: L.rgbd_elic_create_ckbd(128, 3, out),
              6: lambda: L.rgbd_aligner_create(16, 16, out), 7: lambda: L.rgbd_local_context_create(32, out),
              8: lambda: L.rgbd_linear_inter_create(32, 32, 2, out), 9: lambda: L.rgbd_linear_intra_create(32, 2, out)}[family]()
        assert rc == 0 and h.value
        try:
            assert L.rgbd_elic_set_coder(h, 1, 64) == (0 if family in (0, 1) else EINVAL), family
            assert L.rgbd_elic_set_coder(h, 0, 0) == 0          # the reference format: every family, lanes ignored
            for lanes in (0, 3, 128):
                assert L.rgbd_elic_set_coder(h, 1, lanes) == EINVAL
            assert L.rgbd_elic_set_coder(h, 2, 64) == EINVAL and L.rgbd_elic_set_coder(h, -1, 64) == EINVAL
        finally:
            L.rgbd_elic_destroy(h)
    assert L.rgbd_elic_set_coder(None, 0, 0) == EINVAL


def test_other_models_refuse_wide():
    require_gpu()
    import rgbd_amd
    from rgbd_amd._lib import RgbdError

    m = rgbd_amd.modelZoo["ELIC_united_R2D"](config=rgbd_amd.model_config(), channel=4).eval()
    assert m.update(force=True)
    m = m.to("cuda")
    with pytest.raises(RgbdError):
        m.set_coder("wide", lanes=64)  # the engine has no wide path for this family and says so
    assert m.coder == "reference"
