"""rgbd_amd.Spatial_aligner on the GPU against the fixtures of the unmodified reference (tests/golden/aligner_<case>.npz,
tests/golden/make_aligner.py): e_gpu = max |gpu - ref64| / max |ref64| <= 8 * e_ref per case (tests/aligner_cases.py; the
figures are printed and recorded in DESIGN.md 5), test_aligner_cases.py shows on the CPU that every classic mistake lands
100x that bound away."""
import ctypes

import pytest
import torch

import aligner_cases as ac
from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu

EINVAL = -22


@pytest.fixture(scope="module")
def nets():
    require_gpu()
    from rgbd_amd import Spatial_aligner

    out = {}
    for name, (B, cin, cout, H, W, seed, wseed) in ac.CASES.items():
        m = Spatial_aligner(in_channel=cin, out_channel=cout)
        m.load_state_dict(ac.case_weights(name), strict=True)
        out[name] = m.to("cuda")
    return out


@pytest.mark.parametrize("name", list(ac.CASES))
def test_aligner_vs_reference(nets, name):
    B, cin, cout, H, W, _, _ = ac.CASES[name]
    fx = ac.load_fixture(name)
    x, g = ac.case_inputs(name)
    xd, gd = x.cuda(), g.cuda()
    assert xd.data_ptr() != gd.data_ptr()
    out = nets[name](xd, gd)
    assert out.shape == (B, cout, H, W) and out.data_ptr() not in (xd.data_ptr(), gd.data_ptr())
    e_gpu = ac.rel_err(out.cpu(), fx["ref64"])
    print(f"aligner {name}: e_gpu {e_gpu:.3e}, e_ref {fx['e_ref']:.3e}, bound {ac.FACTOR * fx['e_ref']:.3e}")
    assert e_gpu <= ac.FACTOR * fx["e_ref"], (e_gpu, fx["e_ref"])
    # the same inputs again (the call shape's captured graph from the second call on), into another tensor: the same bits
    for _ in range(2):
        again = nets[name](xd, gd)
        assert again.data_ptr() != out.data_ptr() and torch.equal(again.view(torch.int32), out.view(torch.int32))
    # other inputs of the same shape move the result (no stale buffer)
    assert not torch.equal(nets[name](gd, xd), out)
    assert torch.equal(nets[name](xd, gd).view(torch.int32), out.view(torch.int32))


def test_aligner_clone_gives_the_parents_bits(nets):
    name = "b_2x192_16x24"
    x, g = (t.cuda() for t in ac.case_inputs(name))
    clone = nets[name].clone_shared()
    assert torch.equal(clone(x, g).view(torch.int32), nets[name](x, g).view(torch.int32))
    with pytest.raises(Exception):
        clone.load_state_dict(ac.case_weights(name))


def test_aligner_refusals(nets):
    import rgbd_amd
    from rgbd_amd import _lib, synth

    m = nets["a_1x192_8x8"]
    with pytest.raises(ValueError):
        m(torch.zeros(1, 192, 12, 8), torch.zeros(1, 192, 12, 8))  # H % 8
    with pytest.raises(ValueError):
        m(torch.zeros(1, 192, 8, 20), torch.zeros(1, 192, 8, 20))  # W % 8
    with pytest.raises(ValueError):
        m(torch.zeros(1, 64, 8, 8), torch.zeros(1, 64, 8, 8))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 192, 8, 8), torch.zeros(1, 192, 16, 8))
    L = _lib.lib()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.zeros(1, 192, 64, 64, device="cuda")
    out = torch.full((1, 192, 64, 64), 7.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    # the C entry itself refuses H % 8
    assert L.rgbd_aligner_forward(m._h, p(x), p(x), 1, 12, 8, p(out), s) == EINVAL
    # a codec call on an aligner handle
    assert L.rgbd_elic_compress_single(m._h, p(x), 1, 64, 64, 0, s) == EINVAL
    # the aligner call on a codec handle
    net = rgbd_amd.ELIC(config=rgbd_amd.model_config(), channel=3).eval()
    net.load_state_dict(synth.synthetic_state_dict(0, model="ELIC"), strict=True)
    net.update(force=True)
    net = net.to("cuda")
    assert L.rgbd_aligner_forward(net._h, p(x), p(x), 1, 64, 64, p(out), s) == EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_aligner_clone_follows_its_parent():
    """A clone made before the parent's load_state_dict() computes with the parent's NEW weights afterwards, like a codec clone
    (the generation counter of EngineModule).  Before Spatial_aligner stood on that base its clone kept the device buffers it
    was made with: there the first assertion below fails (out_c equals out0, the stale weights)."""
    from rgbd_amd import Spatial_aligner, synth

    require_gpu()
    x, g = (t.cuda() for t in ac.case_inputs("a_1x192_8x8"))
    parent = Spatial_aligner(in_channel=192, out_channel=192, init_seed=0).to("cuda")
    clone = parent.clone_shared()
    out0 = clone(x, g)
    parent.load_state_dict(synth.synthetic_state_dict(1, model="Spatial_aligner", in_channel=192, out_channel=192))
    out_p = parent(x, g)
    out_c = clone(x, g)
    assert torch.equal(out_c, out_p)
    assert not torch.equal(out_c, out0)
