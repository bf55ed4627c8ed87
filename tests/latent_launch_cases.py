"""Cases of the latent-stage sameness record (tests/golden/latent_launch_record.json), shared by the recorder
(tools/record_latent_launches.py) and the test that asserts it (tests/test_gpu_latent_launches.py).

The record is what a PARENT commit did: for each family with a checkerboard slice loop (ELIC_united, STF_united,
ELIC_united_R2D, ELIC) and each call below, the conv launches by shape, the profiled launch count, the workspace size
and SHA-256 of every returned stream, output tensor and y_hat debug tensor.  A refactor of the loop must reproduce every
field: same launches, same workspace, same bits.

Weights: synth, stress recipe, seed 0.  Shape: 64 x 128 (non-square, latent width 8) for ELIC, the one family that takes
it; the two-modality engines refuse it with RGBD_EINVAL (their ESA blocks pool 7 x 7 windows of a stride-2 map: 128 pixels
a side at least, 240 for STF_united), so those run the smallest shape their own GPU tests use at B = 2.
Every call runs three times on a side stream -- eagerly (the first call of a shape may grow the workspace, which drops
the cached graphs), then until its HIP graph is captured and launched -- and once more under the profiler."""
import ctypes
import hashlib

import numpy as np

# family -> (state-dict model name, image channels, (H, W))
FAMILIES = {
    "ELIC_united": ("ELIC_united", 4, (128, 128)),
    "STF_united": ("STF_united", 4, (256, 320)),
    "ELIC_united_R2D": ("ELIC_united_R2D", 4, (128, 128)),
    "ELIC": ("ELIC", 3, (64, 128)),
}
# (batch, per_image_streams) of the compress / decompress calls
CODING_CALLS = (("b1", 1, False), ("b2", 2, False), ("b2_per_image", 2, True))
CONFIG_ID = 61


def sha(x):
    if not isinstance(x, (bytes, bytearray)):
        x = np.ascontiguousarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x).tobytes()
    return hashlib.sha256(x).hexdigest()


def make_net(family):
    import rgbd_amd
    from rgbd_amd import synth

    model, channel, _ = FAMILIES[family]
    net = rgbd_amd.modelZoo[family](config=rgbd_amd.model_config(), channel=channel).eval()
    net.load_state_dict(synth.synthetic_state_dict(0, model=model, stress=True), strict=True)
    net.update(force=True)
    return net.to("cuda")


def _images(family, B, H, W):
    import torch
    from rgbd_amd import synth

    r, d = synth.synthetic_batch(B, H, W, config_id=CONFIG_ID)
    imgs = (torch.from_numpy(r).cuda(),) if family == "ELIC" else (torch.from_numpy(r).cuda(), torch.from_numpy(d).cuda())
    return imgs


def _conv_log():
    from rgbd_amd._lib import lib

    need = lib().rgbd_debug_conv_log_read(None, 0)
    buf = ctypes.create_string_buffer(int(need))
    lib().rgbd_debug_conv_log_read(buf, need)
    return dict(ln.rsplit(",", 1) for ln in buf.value.decode().splitlines()[1:] if ln)


def _measure(net, single, call):
    """call() -> {name: bytes | tensor}: three times on a side stream (eager; the second or the third captures the graph,
    so the third goes through it), once more under the profiler with the conv shape log on (profiled calls run eagerly)."""
    import torch
    from rgbd_amd._lib import check, lib

    names = ("yhat",) if single else ("yhat_r", "yhat_d")

    def hashed():
        out = {k: sha(v) for k, v in call().items()}
        out.update({k: sha(net.debug_tensor(k)) for k in names})
        return out

    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):  # (the NULL stream is never captured)
        eager = hashed()
        g1 = net.graph_count()
        second = hashed()
        graph = hashed()
        captured = net.graph_count() - g1
    torch.cuda.synchronize()
    net.set_profile(True)
    check(lib().rgbd_debug_conv_log(1), "conv_log")
    try:
        profiled = hashed()
        torch.cuda.synchronize()
        launches = int(net.profile_read()["launches"])
        log = _conv_log()
    finally:
        lib().rgbd_debug_conv_log(0)
        net.set_profile(False)
    return {"sha256": graph, "eager_equals_graph": eager == second == graph, "profiled_equals_graph": profiled == graph,
            "graphs_captured": captured, "launches": launches, "conv_log": {k: int(v) for k, v in log.items()},
            "workspace_bytes": net.workspace_bytes()}


def _streams(prefix, lists):
    return {f"{prefix}{i}_{j}": s for i, kind in enumerate(lists) for j, s in enumerate(kind)}


def record_family(family):
    """{"shape": [H, W], "calls": {call name: fields}} of one family on the GPU of this process."""
    import torch

    single = family == "ELIC"
    net = make_net(family)
    H, W = FAMILIES[family][2]
    calls = {}

    def compress(imgs):
        out = net.compress(*imgs)
        kept.update(out)
        if single:
            return _streams("s", out["strings"])
        return {**_streams("r", out["r_strings"]), **_streams("d", out["d_strings"])}

    def decompress():
        if single:
            return {"x_hat": net.decompress(kept["strings"], kept["shape"])["x_hat"]}
        rec = net.decompress(kept["r_strings"], kept["d_strings"], kept["shape"])
        return {"x_hat_r": rec["x_hat"]["r"], "x_hat_d": rec["x_hat"]["d"]}

    def forward(imgs):
        fw = net(*imgs)
        if single:
            return {"x_hat": fw["x_hat"], **{k: v for k, v in fw["likelihoods"].items()}}
        out = {"x_hat_r": fw["x_hat"]["r"], "x_hat_d": fw["x_hat"]["d"]}
        out.update({f"lik_{m}_{k}": fw[f"{m}_likelihoods"][k] for m in "rd" for k in "yz"})
        return out

    for tag, B, per_image in CODING_CALLS:
        imgs, kept = _images(family, B, H, W), {}
        net.per_image_streams = per_image
        try:
            calls[f"compress_{tag}"] = _measure(net, single, lambda: compress(imgs))
            if tag == "b2" and not single:  # the latents and hyper tensors of this call, for the stage entry points below
                lat = [torch.from_numpy(net.debug_tensor(n).copy()).cuda() for n in ("y_r", "hyper_r", "y_d", "hyper_d")]
            calls[f"decompress_{tag}"] = _measure(net, single, decompress)
        finally:
            net.per_image_streams = False
    imgs = _images(family, 2, H, W)
    calls["forward_b2"] = _measure(net, single, lambda: forward(imgs))
    if not single:
        def compress_united():
            kept["u"] = net.compress_united(*lat)
            return _streams("y", kept["u"])

        def decompress_united():
            yr, yd = net.decompress_united(kept["u"][0], lat[1], kept["u"][1], lat[3])
            return {"yhat_out_r": yr, "yhat_out_d": yd}

        calls["compress_united_b2"] = _measure(net, single, compress_united)
        calls["decompress_united_b2"] = _measure(net, single, decompress_united)
    return {"shape": [H, W], "calls": calls}


def stream_hashes(record, family, call):
    """the stream entries (not the y_hat tensors) of one recorded call"""
    return {k: v for k, v in record[family]["calls"][call]["sha256"].items() if not k.startswith("yhat")}
