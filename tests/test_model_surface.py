"""The Python model classes against tests/golden/model_surface_record.json, which tools/record_model_surface.py wrote on the
commit named in the record (the last one before the classes were put on one engine base): constructor attributes, state_dict
keys / shapes / dtypes, parameter counts, public names and the library calls of an upload, class by class; a state_dict
round trip; and the host-side errors every class raises without a GPU.  Nothing here needs a GPU."""
import json
import os

import pytest
import torch

import model_surface_cases as cases

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_surface_record.json")) as f:
    RECORD = json.load(f)

# names that left a class on purpose: single-modal classes no longer inherit the two-modality stage calls (AttributeError now,
# NotImplementedError before), and return_mid is ELIC's alone
REMOVED = {"ELIC": {"compress_united", "decompress_united"},
           "STF": {"compress_united", "decompress_united", "return_mid"},
           "ckbd": {"compress_united", "decompress_united", "return_mid"}}
ZOO = cases.CLASSES[:-1]


@pytest.fixture(scope="module", params=cases.CLASSES)
def pair(request):
    """(recorded surface, present surface) of one class; the present one is computed once."""
    return request.param, RECORD[request.param], cases.surface(request.param)


def test_record_covers_every_class():
    import rgbd_amd

    assert len(RECORD["commit"]) == 40
    assert set(RECORD) - {"commit"} == set(cases.CLASSES) == set(rgbd_amd.modelZoo) | {"Spatial_aligner"}
    assert list(rgbd_amd.modelZoo) == ZOO  # the order the testers match names in
    from rgbd_amd.elic_united import modelZoo

    assert modelZoo is rgbd_amd.modelZoo


def test_attributes_keys_and_parameter_count(pair):
    name, want, got = pair
    removed_attrs = {a for a in REMOVED.get(name, ()) if a in want["attributes"]}
    assert got["attributes"] == {k: v for k, v in want["attributes"].items() if k not in removed_attrs}
    assert got["state_dict_keys"] == want["state_dict_keys"]
    assert got["state_dict_sha256"] == want["state_dict_sha256"]  # ordered keys, shapes and dtypes
    assert got["count_parameters"] == want["count_parameters"]


def test_upload_makes_the_recorded_library_calls(pair):
    name, want, got = pair
    assert got["upload_calls"] == want["upload_calls"]
    assert got["upload_sha256"] == want["upload_sha256"]


def test_public_names_only_leave_on_purpose(pair):
    name, want, got = pair
    gone = set(want["public_names"]) - set(got["public_names"])
    assert gone == REMOVED.get(name, set())
    for n in sorted(gone):
        with pytest.raises(AttributeError):
            getattr(cases.make(name), n)


@pytest.mark.parametrize("name", cases.CLASSES)
def test_state_dict_round_trip(name):
    src, dst = cases.make(name, init_seed=0), cases.make(name, init_seed=1)
    sd = src.state_dict()
    floats = [k for k, v in sd.items() if v.is_floating_point() and v.numel() > 1]
    assert any(not torch.equal(sd[k], dst.state_dict()[k]) for k in floats)  # the seeds do differ
    dst.load_state_dict(sd, strict=True)
    back = dst.state_dict()
    assert list(back) == list(sd)
    for k in sd:
        assert back[k].dtype == sd[k].dtype and torch.equal(back[k], sd[k]), k


def m_single(name):
    return name in ("ELIC", "STF", "ckbd")


@pytest.mark.parametrize("name", ZOO)
def test_host_side_errors(name):
    """What test_stf_single_cpu.py and test_ckbd_cpu.py held for their own class, for every zoo class."""
    import ctypes

    import rgbd_amd

    m = rgbd_amd.modelZoo[name](config=rgbd_amd.model_config(), channel=3 if m_single(name) else 4).eval()
    with pytest.raises(rgbd_amd.RgbdError):
        m.to("cpu")
    if not torch.cuda.is_available():
        with pytest.raises(rgbd_amd.RgbdError):
            m.to("cuda")

    def images(B, C, H, W):  # one tensor, or rgb and depth
        return (torch.zeros(B, C, H, W),) if m_single(name) else (torch.zeros(B, C, H, W), torch.zeros(B, 1, H, W))

    with pytest.raises(rgbd_amd.RgbdError):
        m.compress(*images(1, 3, 64, 64))  # before .to("cuda")
    with pytest.raises(NotImplementedError):
        m.train()
    # the size check comes before any device work
    m._ready = lambda: None
    m._device = torch.device("cpu")
    for H, W in ((100, 128), (128, 100)):
        with pytest.raises(ValueError):
            m.compress(*images(1, 3, H, W))
        with pytest.raises(ValueError):
            m.forward(*images(1, 3, H, W))
    with pytest.raises(ValueError):
        m.compress(*images(1, 1 if m_single(name) else 4, 128, 128))  # channel mismatch
    if name == "ckbd":
        with pytest.raises(NotImplementedError):
            m.validate(torch.zeros(1, 3, 64, 64))
        # the C ABI rejects widths / channel counts the model does not have before it creates anything
        from rgbd_amd import _lib

        h = ctypes.c_void_p()
        for N, ch in ((160, 3), (192, 2), (0, 3), (192, 0)):
            assert _lib.lib().rgbd_elic_create_ckbd(N, ch, ctypes.byref(h)) == -22 and not h.value
        assert _lib.lib().rgbd_elic_create_ckbd(192, 3, None) == -22


def test_aligner_host_side_errors():
    import rgbd_amd

    sa = rgbd_amd.Spatial_aligner(in_channel=64, out_channel=96).eval()
    with pytest.raises(rgbd_amd.RgbdError):
        sa.to("cpu")
    if not torch.cuda.is_available():
        with pytest.raises(rgbd_amd.RgbdError):
            sa.to("cuda")
    with pytest.raises(rgbd_amd.RgbdError):
        sa(torch.zeros(1, 64, 8, 8), torch.zeros(1, 64, 8, 8))  # before .to("cuda")
    with pytest.raises(NotImplementedError):
        sa.train()
    # the shape checks come before any device work
    sa._ready = lambda: None
    sa._device = torch.device("cpu")
    with pytest.raises(ValueError):
        sa(torch.zeros(1, 64, 8, 8), torch.zeros(1, 64, 8, 16))  # guided of another shape
    with pytest.raises(ValueError):
        sa(torch.zeros(1, 32, 8, 8), torch.zeros(1, 32, 8, 8))  # channel mismatch
    for H, W in ((12, 8), (8, 12)):
        with pytest.raises(ValueError):
            sa(torch.zeros(1, 64, H, W), torch.zeros(1, 64, H, W))
