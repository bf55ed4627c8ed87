"""rgbd_amd.SynthesisTransformPlus on the GPU against the fixtures of the unmodified reference (tests/golden/synplus_<case>.npz,
tests/golden/make_synplus.py): e_gpu = max |gpu - ref64| / max |ref64| <= 8 * e_ref per case (tests/synplus_cases.py; the
figures are printed and recorded in DESIGN.md 5.7); test_synplus_cases.py shows on the CPU that every mistake in the walk lands
far beyond that bound.  Then what a caller relies on: the same bits call after call, from a clone, and across call shapes; the
hand-off of up1..up3 from ELIC(return_mid=True) on the device; the refusals of the C ABI; a state_dict round trip."""
import ctypes

import pytest
import torch

import synplus_cases as sc
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -22, -1


def bits(t):
    return t.view(torch.int32)


@pytest.fixture(scope="module")
def nets():
    require_gpu()
    from rgbd_amd import SynthesisTransformPlus

    out = {}
    for name, (B, ch, h, w, seed, wseed) in sc.CASES.items():
        m = SynthesisTransformPlus(sc.N, sc.M, ch=ch)
        m.load_state_dict(sc.case_weights(name), strict=True)
        out[name] = m.to("cuda")
    return out


@pytest.fixture(scope="module")
def elic_mid():
    require_gpu()
    import rgbd_amd
    from rgbd_amd import synth

    net = rgbd_amd.ELIC(config=rgbd_amd.model_config(), channel=3, return_mid=True).eval()
    net.load_state_dict(synth.synthetic_state_dict(0, model="ELIC"), strict=True)
    net.update(force=True)
    return net.to("cuda")


@pytest.fixture(scope="module")
def case_a(nets):
    ins = tuple(t.cuda() for t in sc.case_inputs("a"))
    return ins, nets["a"](*ins).clone()


@pytest.mark.parametrize("name", list(sc.CASES))
def test_synplus_vs_reference(nets, name):
    B, ch, h, w, _, _ = sc.CASES[name]
    fx = sc.load_fixture(name)
    ins = tuple(t.cuda() for t in sc.case_inputs(name))
    out = nets[name](*ins)
    assert out.shape == (B, ch, 16 * h, 16 * w) and out.data_ptr() not in [t.data_ptr() for t in ins]
    e_gpu = sc.rel_err(out.cpu(), fx)
    print(f"synplus {name}: e_gpu {e_gpu:.3e}, e_ref {fx['e_ref']:.3e}, e_gpu / e_ref {e_gpu / fx['e_ref']:.2f}, "
          f"bound {sc.FACTOR * fx['e_ref']:.3e}")
    assert e_gpu <= sc.FACTOR * fx["e_ref"], (e_gpu, fx["e_ref"])
    # three calls in a row (the call shape's captured graph from the second call on), into other tensors: the same bits
    for _ in range(2):
        again = nets[name](*ins)
        assert again.data_ptr() != out.data_ptr() and torch.equal(bits(again), bits(out))
    # another guide of the same shape moves the result (no stale buffer), and the first inputs give the first bits again
    assert not torch.equal(nets[name](ins[0], ins[1], ins[2], ins[3].flip(3)), out)
    assert not torch.equal(nets[name](ins[0], ins[1].flip(2), ins[2], ins[3]), out)
    assert torch.equal(bits(nets[name](*ins)), bits(out))


def test_synplus_clone_gives_the_parents_bits(nets):
    ins = tuple(t.cuda() for t in sc.case_inputs("b"))
    clone = nets["b"].clone_shared()
    assert torch.equal(bits(clone(*ins)), bits(nets["b"](*ins)))
    with pytest.raises(Exception):
        clone.load_state_dict(sc.case_weights("b"))


def test_synplus_call_shapes_in_turn():
    """One instance at case a, then d (a larger workspace: regrowth drops the cached graphs), then a again."""
    from rgbd_amd import SynthesisTransformPlus

    require_gpu()
    m = SynthesisTransformPlus(sc.N, sc.M, ch=3)
    m.load_state_dict(sc.case_weights("a"), strict=True)
    m = m.to("cuda")
    a = tuple(t.cuda() for t in sc.case_inputs("a"))
    d = tuple(t.cuda() for t in sc.case_inputs("d"))
    first = m(*a).clone()
    out_d = m(*d).clone()
    assert torch.equal(bits(m(*a)), bits(first))
    assert torch.equal(bits(m(*d)), bits(out_d)) and torch.equal(bits(m(*d)), bits(out_d))
    assert torch.equal(bits(m(*a)), bits(first))
    assert sc.rel_err(first.cpu(), sc.load_fixture("a")) <= sc.FACTOR * sc.load_fixture("a")["e_ref"]


def test_synplus_takes_the_guides_of_elic_return_mid(nets, elic_mid):
    """ELIC(return_mid=True) decodes a 64x64 image; its up1..up3 stay on the device and guide a seeded y_hat."""
    from rgbd_amd import synth

    r, _ = synth.synthetic_batch(1, 64, 64, config_id=5)
    enc = elic_mid.compress(torch.from_numpy(r).cuda())
    dec = elic_mid.decompress(enc["strings"], enc["shape"])
    ups = [dec[k] for k in ("up1", "up2", "up3")]
    assert [tuple(u.shape) for u in ups] == [(1, 192, 8, 8), (1, 192, 16, 16), (1, 192, 32, 32)] and all(u.is_cuda for u in ups)
    yhat = sc.inputs(1, 4, 4, 777)[0]
    m = nets["a"]
    out = m(yhat.cuda(), *ups)
    assert out.shape == (1, 3, 64, 64)
    host = [u.cpu() for u in ups]
    sd = sc.case_weights("a")
    ref64 = sc.synthesis_plus(sd, yhat, *host)
    floor = sc.rel_err_t(sc.synthesis_plus(sd, yhat, *host, dtype=torch.float32), ref64)
    e = sc.rel_err_t(out.cpu(), ref64)
    print(f"synplus hand-off: e_gpu {e:.3e}, fp32 restatement {floor:.3e}, bound {sc.FACTOR * floor:.3e}; "
          f"max|up| {[round(float(u.abs().max()), 2) for u in host]}")
    assert e <= sc.FACTOR * floor, (e, floor)
    # host-round-tripped copies of the guides (new device tensors): the same bits
    again = m(yhat, *[u.clone() for u in host])
    assert torch.equal(bits(again), bits(out))


def test_synplus_refusals(nets, elic_mid, case_a):
    from rgbd_amd import SynthesisTransformPlus, Spatial_aligner, _lib

    ins, want = case_a
    m = nets["a"]
    L = _lib.lib()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    y, u1, u2, u3 = ins
    out = torch.full((1, 3, 64, 64), 7.0, device="cuda")
    big = torch.zeros(1, 192, 64, 64, device="cuda")

    def still_fine():
        torch.cuda.synchronize()
        assert (out == 7.0).all()
        assert torch.equal(bits(m(*ins)), bits(want))

    # the Python surface
    with pytest.raises(ValueError):
        m(torch.zeros(1, 320, 6, 4), u1, u2, u3)  # h % 4
    with pytest.raises(ValueError):
        m(torch.zeros(1, 192, 4, 4), u1, u2, u3)  # M
    with pytest.raises(ValueError):
        m(y, u1, u2, u2)  # up3 of up2's size
    with pytest.raises(ValueError):
        m(y, u1[:, :64], u2, u3)
    with pytest.raises(NotImplementedError):
        SynthesisTransformPlus(sc.N, sc.M, act=torch.nn.GELU)
    with pytest.raises(ValueError):
        SynthesisTransformPlus(128, sc.M)
    assert SynthesisTransformPlus(sc.N, sc.M, ch=1, act=torch.nn.ReLU).ch == 1
    # create: N other than 192, M not a multiple of 16, ch of 0, no place for the handle
    h = ctypes.c_void_p()
    for args in ((128, 320, 3), (192, 324, 3), (192, 0, 3), (192, 320, 0), (192, 320, -1)):
        assert L.rgbd_synthesis_plus_create(*args, ctypes.byref(h)) == EINVAL and not h.value
    assert L.rgbd_synthesis_plus_create(192, 320, 3, None) == EINVAL
    # forward: every bad argument, before any launch
    fwd = L.rgbd_synthesis_plus_forward
    for args in ((None, p(u1), p(u2), p(u3), 1, 4, 4, p(out)), (p(y), None, p(u2), p(u3), 1, 4, 4, p(out)),
                 (p(y), p(u1), None, p(u3), 1, 4, 4, p(out)), (p(y), p(u1), p(u2), None, 1, 4, 4, p(out)),
                 (p(y), p(u1), p(u2), p(u3), 1, 4, 4, None), (p(y), p(u1), p(u2), p(u3), 0, 4, 4, p(out)),
                 (p(y), p(u1), p(u2), p(u3), -1, 4, 4, p(out)), (p(y), p(u1), p(u2), p(u3), 1, 0, 4, p(out)),
                 (p(y), p(u1), p(u2), p(u3), 1, 4, -4, p(out)), (p(y), p(u1), p(u2), p(u3), 1, 2, 4, p(out)),
                 (p(y), p(u1), p(u2), p(u3), 1, 4, 6, p(out)), (p(y), p(u1), p(u2), p(u3), 1, 1, 1, p(out))):
        assert fwd(m._h, *args, s) == EINVAL, args[4:7]
        still_fine()
    # a handle of another family, and no handle
    sa = Spatial_aligner(in_channel=192, out_channel=192).to("cuda")
    for other in (elic_mid._h, sa._h, None):
        assert fwd(other, p(y), p(u1), p(u2), p(u3), 1, 4, 4, p(out), s) == EINVAL
    still_fine()
    # this handle given to the aligner's call, to a codec call, and to the wide coder's switch
    assert L.rgbd_aligner_forward(m._h, p(big), p(big), 1, 64, 64, p(out), s) == EINVAL
    still_fine()
    assert L.rgbd_elic_compress_single(m._h, p(big), 1, 64, 64, 0, s) == EINVAL
    assert L.rgbd_elic_forward_single_mid(m._h, p(big), 1, 64, 64, p(out), p(out), p(out), p(out), p(out), p(out), s) == EINVAL
    still_fine()
    assert L.rgbd_elic_set_coder(m._h, 1, 64) == EINVAL
    assert L.rgbd_elic_set_coder(m._h, 0, 64) == 0  # (the reference format is what it has)
    still_fine()
    # the timing switch belongs to this family
    assert L.rgbd_debug_synthesis_plus_guides(sa._h, 0) == EINVAL and L.rgbd_debug_synthesis_plus_guides(None, 0) == EINVAL
    # an unfinalized handle is refused like the other module handles
    assert L.rgbd_synthesis_plus_create(192, 320, 3, ctypes.byref(h)) == 0 and h.value
    try:
        assert fwd(h, p(y), p(u1), p(u2), p(u3), 1, 4, 4, p(out), s) == ESTATE
        assert fwd(h, p(y), p(u1), p(u2), p(u3), 1, 2, 4, p(out), s) == ESTATE
    finally:
        L.rgbd_elic_destroy(h)
    still_fine()


def test_synplus_guides_switch_is_a_call_shape_of_its_own(nets, case_a):
    """The probe's switch: without the aligners the walk gives another result; switched back, the first bits."""
    from rgbd_amd import _lib

    ins, want = case_a
    m, L = nets["a"], _lib.lib()
    assert L.rgbd_debug_synthesis_plus_guides(m._h, 0) == 0
    try:
        off = m(*ins).clone()
        assert torch.equal(bits(m(*ins)), bits(off)) and not torch.equal(off, want)
        assert torch.equal(bits(m(ins[0], ins[1].flip(2), ins[2], ins[3])), bits(off))  # the guides are not read
    finally:
        assert L.rgbd_debug_synthesis_plus_guides(m._h, 1) == 0
    assert torch.equal(bits(m(*ins)), bits(want))


def test_synplus_state_dict_round_trip(nets, case_a):
    from rgbd_amd import SynthesisTransformPlus

    ins, want = case_a
    sd = nets["a"].state_dict()
    assert list(sd) == list(sc.case_weights("a"))
    other = SynthesisTransformPlus(sc.N, sc.M, ch=3, init_seed=5).to("cuda")
    assert not torch.equal(other(*ins), want)
    other.load_state_dict(sd, strict=True)
    assert torch.equal(bits(other(*ins)), bits(want))
    with pytest.raises(RuntimeError):
        other.load_state_dict({k: v for k, v in sd.items() if not k.startswith("sp3.")}, strict=True)
