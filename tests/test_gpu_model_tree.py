"""What the shared bases of the Python model classes (EngineModule, Codec, SingleCodec) promise on the GPU beyond the per-model
tests: CodecPool takes "one tensor per call" from the class's modality count (STF and ckbd as well as ELIC), and a
single-modal clone follows its parent's re-uploads like a two-modality one (test_gpu_parity_pinned.py has that scenario for
ELIC_united)."""
import pytest
import torch

from gpu_utils import require_gpu

pytestmark = pytest.mark.gpu


def _images(B, H, W, config_id):
    from rgbd_amd import synth

    return torch.from_numpy(synth.synthetic_batch(B, H, W, config_id=config_id)[0]).cuda()


@pytest.mark.parametrize("name,kw,H,W", [("ckbd", {"N": 192}, 64, 128), ("STF", {}, 128, 128)])
def test_pool_by_modality_count(name, kw, H, W):
    """CodecPool(model_cls=ckbd / STF): pool.single, channel 3 by default, and roundtrip(x) gives the per-image strings and the
    x_hat of ONE instance with per_image_streams, bit for bit.  (The pool used to compare the class's name with "ELIC": for
    these two it defaulted to channel 4 and called the two-modality decompress.)"""
    import rgbd_amd
    from rgbd_amd import synth

    require_gpu()
    cls = rgbd_amd.modelZoo[name]
    sd = synth.synthetic_state_dict(0, model=name, channel=3, **kw)
    x = _images(2, H, W, 43)
    one = cls(config=rgbd_amd.model_config(), channel=3).eval()
    one.load_state_dict(sd, strict=True)
    one.update(force=True)
    one = one.to("cuda")
    one.per_image_streams = True  # (`one` outlives the pool below, so the pool's close() leaves the wait policy as it is)
    ref = one.compress(x)
    ref_rec = one.decompress(ref["strings"], ref["shape"])
    assert len(ref["strings"][0]) == 2 and len(ref["strings"][1]) == 2
    with rgbd_amd.CodecPool(sd, config=rgbd_amd.model_config(), workers=2, device="cuda", per_image_streams=True,
                            model_cls=cls) as pool:
        assert pool.single is True and pool.nets[0].channel == 3
        outs, xh = pool.roundtrip(x)  # two groups of one image on two streams
        assert [s for o in outs for s in o["strings"][0]] == list(ref["strings"][0])
        assert [s for o in outs for s in o["strings"][1]] == list(ref["strings"][1])
        assert torch.equal(xh, ref_rec["x_hat"])


def test_single_modal_clone_survives_parent_reupload():
    """test_clone_survives_parent_reupload (test_gpu_parity_pinned.py) for the single-modal ELIC: the clone logic is one piece
    of code for every family, and a second family pins that.  Parent and clone are what that test takes out of a pool of two;
    here they are made directly, so that the test leaves the process's wait policy alone (a pool closed with no other engine
    alive hands it back to the runtime's default)."""
    import rgbd_amd
    from rgbd_amd import RgbdError, synth

    require_gpu()
    parent = rgbd_amd.ELIC(config=rgbd_amd.model_config(), channel=3).eval()
    parent.load_state_dict(synth.synthetic_state_dict(0, model="ELIC"), strict=True)
    parent.update(force=True)
    parent = parent.to("cuda")
    clone = parent.clone_shared()
    parent.per_image_streams = clone.per_image_streams = True
    x = _images(1, 64, 128, 21)
    before = clone.compress(x)
    assert parent.update(force=True)             # parent: tables rebuilt, weights re-uploaded on the next call
    mid = clone.compress(x)                      # the clone follows the parent (fresh clone of the new generation)
    assert mid["strings"] == before["strings"]
    rec = clone.decompress(mid["strings"], mid["shape"])
    ref = parent.decompress(mid["strings"], mid["shape"])
    assert torch.equal(rec["x_hat"], ref["x_hat"])
    # new weights on the parent reach the clone
    parent.load_state_dict(synth.synthetic_state_dict(1, model="ELIC"))
    parent.update(force=True)
    a = parent.compress(x)
    b = clone.compress(x)
    assert a["strings"] == b["strings"] and a["strings"] != before["strings"]
    with pytest.raises(RgbdError):
        clone.update(force=True)
    # a clone outlives its parent's python object being re-uploaded again while it is mid-use
    parent.update(force=True)
    parent.compress(x)
    c = clone.compress(x)
    assert c["strings"] == a["strings"]
