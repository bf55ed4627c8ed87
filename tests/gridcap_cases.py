"""Every launch site of csrc/ whose grid is clamped (a grid-stride loop runs more than once only past the clamp), the cases that
cross each clamp, and the models of a broken loop that the cases must be able to tell from a working one -- shared by
tests/test_gridcap_cases.py (CPU: are the cases hollow?) and the GPU tests of the kernels, each in the file that holds the
kernel's reference.  numpy / torch-CPU only; importable without a GPU.

The inventory (ROWS) is plain data, built from a search of csrc/ for `gridDim.x` and for the clamp expressions
(`> 2048 ? 2048`, `g > 8192`, `g > 4096`, `std::min<size_t>(..., 8192)`, `grid_for(`).  Not rows, because nothing is clamped:
eb_forward / z_quant / z_dequant (entropy.hip: one thread per element, the loop is there but the grid is never cut), the local
and linear attention kernels (context_attn.hip: a 3-D grid of tiles / chunks, refused above 65535), channel_mean / se_* (grid
by channel block and image), msssim_scale / msssim_finish (grid by tile and plane), conv_mfma_body.h (gridDim.x only renumbers
workgroups), ph_chunk_pixels (pooled_head.hip: clamps the pixels of a chunk, the grid is the chunk count).

A case crosses a clamp when  cap * block < work < 2 * cap * block  and  (work - cap * block) % block != 0 : two sweeps, the
second one partial and ending in a ragged block ("sweeps": 3 shifts both by one sweep).  `work` is the launcher's own formula
(ROWS[..]["work"], evaluated on the case's dimensions); `items` the index space the kernel's loop walks when that is another one
(fill_zero_kernel: the launcher sizes the grid for float4s, the loop walks floats).

A built case is a list of stages, one per launch under test:
    {"row", "dims", "dests": {name: {"init", "want", "owner"}}, "inplace": {name: reapply}, "accept"}
`init` is the destination before the launch (the file's sentinel, or the state an in-place kernel updates), `want` the
reference's result over the WHOLE destination, `owner` the loop index that writes each element (-1: nobody's).  `accept(got)`
is the comparison the GPU test runs on what the device returned; the CPU test runs it on `want` (must pass) and on `want`
spoiled by each model below (must fail).

Models of a broken loop (MODELS), applied to the reference output:
    no_loop             `if (i < total)`: items at or past cap * block keep `init`
    last_sweep_dropped  the loop stops one sweep early
    stride_long         the stride one block too long: the first block of every later sweep is skipped
    stride_short        the stride one block too short: nothing is skipped, the first block of every later sweep is done twice.  A
                        kernel that only writes gives the same bits (slower, not wrong), so this model applies to the in-place
                        stages alone: there the update lands twice.
"""
import numpy as np

import pointwise_forms_cases as pc

F32 = np.float32
MODELS = ("no_loop", "stride_short", "last_sweep_dropped", "stride_long")

# ================================================================================================ the inventory
_E, _M, _C, _X, _P, _V, _T, _S = ("entropy.hip", "mlic_loop.hip", "coder_abi.hip", "context_attn.hip", "pointwise.hip", "conv_mfma.hip",
                                  "metrics.hip", "swin.hip")
NO_HOOK = "no hook reaches it alone"


def _row(key, kernel, file, launcher, hook, work, cap, crossed_by, block=256, items=None, note=""):
    return dict(key=key, kernel=kernel, file=file, launcher=launcher, hook=hook, work=work, cap=cap, block=block, items=items or work,
                crossed_by=crossed_by, note=note)


ROWS = [
    # ---- entropy.hip: n > 2048 ? 2048 : n blocks of 256
    _row("ckbd_part", "ckbd_part_kernel<0/1/2>", _E, "part_grid", "rgbd_ckbd_part", "B*h*(w//2)*C", 2048,
         "tests/test_gpu_entropy.py::test_ckbd_part_kernel[grid]"),
    _row("ckbd_estimate", "ckbd_estimate_kernel", _E, "part_grid", "rgbd_ckbd_estimate_part", "B*h*(w//2)*C", 2048,
         "tests/test_gpu_entropy.py::test_ckbd_estimate_kernel[grid]"),
    _row("slice_estimate", "slice_estimate_kernel", _E, "slice_grid", "rgbd_slice_estimate", "B*h*w*C", 2048,
         "tests/test_gpu_entropy.py::test_slice_estimate_kernel[grid]"),
    _row("slice_quant", "slice_part_kernel<0>", _E, "slice_grid", "rgbd_slice_quant_index", "B*h*w*C", 2048,
         "tests/test_gpu_stf_single.py::test_slice_kernels_past_the_grid_cap"),
    _row("slice_dequant", "slice_part_kernel<2>", _E, "slice_grid", "rgbd_slice_dequant", "B*h*w*C", 2048,
         "tests/test_gpu_stf_single.py::test_slice_kernels_past_the_grid_cap"),
    _row("slice_index", "slice_part_kernel<1>", _E, "slice_grid", None, "B*h*w*C", 2048, None,
         note=NO_HOOK + " (the same loop text as modes 0 and 2, which are crossed); run below the cap by the STF decoder: "
         "tests/test_gpu_stf_single.py::test_layered_contract"),
    _row("lrp_update", "lrp_update_kernel", _E, "launch_lrp_update", "rgbd_lrp_update", "npix*C", 2048,
         "tests/test_gpu_stf_single.py::test_slice_kernels_past_the_grid_cap"),
    # ---- mlic_loop.hip: grid_of, 2048 blocks of 256 quads
    _row("mlic_lrp_apply", "mlic_lrp_apply_kernel", _M, "grid_of", "rgbd_mlic_lrp_apply", "B*h*((w+1)//2)*8", 2048,
         "tests/test_gpu_mlic.py::test_slot_kernels_past_the_grid_cap"),
    _row("mlic_slot_clear", "mlic_slot_clear_kernel", _M, "grid_of", "rgbd_mlic_slot_clear", "B*h*((w+1)//2)*8", 2048,
         "tests/test_gpu_mlic.py::test_slot_kernels_past_the_grid_cap"),
    # ---- coder_abi.hip: std::min<size_t>(.., 8192)
    _row("ckbd_nchw_quant", "ckbd_nchw_kernel<0, VEC/scalar>", _C, "ckbd_op", "rgbd_ckbd_quant_index", "n*c*h*(w//2)", 8192,
         "tests/test_gpu_coder.py::test_ckbd_quant_index_past_the_grid_cap"),
    _row("ckbd_nchw_dequant", "ckbd_nchw_kernel<2, VEC/scalar>", _C, "ckbd_op", "rgbd_ckbd_dequant", "n*c*h*(w//2)", 8192,
         "tests/test_gpu_coder.py::test_ckbd_quant_index_past_the_grid_cap"),
    # ---- context_attn.hip: grid_for, 8192
    _row("dwconv3x3", "dwconv3x3_kernel", _X, "grid_for", "rgbd_dwconv3x3", "B*H*W*C", 8192,
         "tests/test_gpu_mlic_context.py::test_dwconv_kernel_past_the_grid_cap"),
    _row("ckbd_split", "ckbd_split_kernel", _X, "grid_for", None, "B*H*W*(cs//4)", 8192, None,
         note=NO_HOOK + " (launch_ckbd_split is called by the MLIC++ loop and the engine only); run below the cap by "
         "tests/test_gpu_mlic.py::test_layered_contract -- a latent grid of 2 097 152 float4s is not a test's size"),
    # ---- pointwise.hip: grid_for(work), 2048
    _row("pw_nchw_to_nhwc", "nchw_to_nhwc16_kernel", _P, "grid_for", "rgbd_pw_nchw_to_nhwc", "N*H*W*(cs//4)", 2048,
         "tests/test_gpu_pointwise_forms.py::test_layout_kernels_past_the_grid_cap"),
    _row("pw_nhwc_to_nchw", "nhwc_to_nchw_kernel", _P, "grid_for", "rgbd_pw_nhwc_to_nchw", "N*C*H*W", 2048,
         "tests/test_gpu_pointwise_forms.py::test_layout_kernels_past_the_grid_cap"),
    _row("pw_maxpool7s3", "maxpool7s3_kernel", _P, "grid_for", "rgbd_pw_maxpool7s3", "N*((H-7)//3+1)*((W-7)//3+1)*(cs//4)", 2048,
         "tests/test_gpu_pointwise_forms.py::test_maxpool7s3_past_the_grid_cap"),
    _row("pw_bilinear", "bilinear_kernel", _P, "grid_for", "rgbd_pw_bilinear", "N*H*W*(cs//4)", 2048,
         "tests/test_gpu_pointwise_forms.py::test_bilinear_past_the_grid_cap"),
    _row("pw_channel_scale", "channel_scale_to_kernel", _P, "grid_for", "rgbd_pw_channel_scale", "N*HW*(C//4)", 2048,
         "tests/test_gpu_pointwise_forms.py::test_channel_scale_past_the_grid_cap"),
    _row("pw_copy_channels", "copy_channels_kernel", _P, "grid_for", "rgbd_pw_copy_channels", "npix*(C//4)", 2048,
         "tests/test_gpu_pointwise_forms.py::test_copy_channels_past_the_grid_cap"),
    _row("pw_im2col5s2", "im2col5s2_kernel", _P, "grid_for", "rgbd_pw_im2col5s2", "N*((H+1)//2)*((W+1)//2)*(KP//4)", 2048,
         "tests/test_gpu_pointwise_forms.py::test_im2col5s2_past_the_grid_cap"),
    _row("pw_fill_zero", "fill_zero_kernel", _P, "grid_for", "rgbd_pw_fill_zero", "(n+3)//4", 2048,
         "tests/test_gpu_pointwise_forms.py::test_fill_zero_past_the_grid_cap", items="n",
         note="the grid is sized for float4s and the loop walks floats: four sweeps and more at every size above 1024, the cap is"
         " met at n > 2 097 152"),
    _row("pw_half_tanh", "half_tanh_kernel", _P, "grid_for", "rgbd_pw_half_tanh", "npix*(C//4)", 2048,
         "tests/test_gpu_mlic.py::test_half_tanh_past_the_grid_cap"),
    _row("small_conv_ref", "small_conv_ref_kernel", _P, "grid_for", "rgbd_ref_small_conv_nchw", "n*OH*OW*cout", 2048,
         "tests/test_gpu_refpointwise.py::test_small_conv_past_the_grid_cap",
         note="through the hook's staging (fill_zero, then the layout kernels, which cross their caps along with it)"),
    _row("gather_taps", "gather_taps_kernel", _P, "grid_for", "rgbd_ref_deconv_s2_nchw", "B*h*jw*nt*(cin_pad//4)", 2048,
         "tests/test_gpu_refpointwise.py::test_deconv_s2_past_the_grid_cap",
         note="one launch per phase and column class: phase (1, 1) (4 taps) takes two sweeps, the other phases three and more"),
    _row("scatter_phase", "scatter_phase_kernel", _P, "grid_for", "rgbd_ref_deconv_s2_nchw", "B*h*jw*(cout_pad//4)", 2048,
         "tests/test_gpu_refpointwise.py::test_deconv_s2_past_the_grid_cap"),
    _row("gather_wslabs", "gather_wslabs_kernel", _P, "grid_for", "rgbd_ref_deconv_s2_nchw", "cout_pad*nt*(cin_pad//4)", 2048,
         "tests/test_gpu_refpointwise.py::test_deconv_s2_wide_layer_past_the_grid_cap",
         note="the work is the layer's, not the map's: a 496 -> 496 layer on 2 x 4 pixels crosses at the 9-tap phase"),
    _row("sigmoid_gate_ref", "sigmoid_gate_ref_kernel", _P, "launch_sigmoid_gate_ref", "rgbd_ref_sigmoid_gate", "n*h*w*((c+15)//16*16)",
         8192, "tests/test_gpu_refpointwise.py::test_sigmoid_gate_past_the_grid_cap"),
    # ---- conv_mfma.hip: the split-K reducer, 2048
    _row("splitk_reduce", "splitk_reduce_kernel", _V, "launch_conv", "rgbd_conv_forms_nchw", "groups*n*OH*OW*(cout_pad//4)", 2048,
         "tests/test_gpu_convforms.py::test_splitk_reducer_past_the_grid_cap",
         note="behind the conv kernel whose partial planes it adds; the same sizes cross the deconv route's reducer in "
         "test_deconv_s2_past_the_grid_cap"),
    # ---- metrics.hip: avgpool2, 4096
    _row("avgpool2", "avgpool2_kernel", _T, "rgbd_msssim_stats", "rgbd_msssim_stats", "P*oh*ow", 4096, None,
         note="reached through the five-scale walk of rgbd_msssim_stats only; P * oh * ow > 1 048 576 needs 4.2 M input pixels per "
         "image whatever the shape (the smallest: 160 planes of 161 x 161).  msssim_cases.build() of that case takes 3.5 s on the "
         "host, against 1.1 s for planes65, the slowest case of tests/test_gpu_msssim.py (measured on one machine), and the shape "
         "cannot shrink -- slower than the slowest test of its file, so left below the cap; run by every case of that file"),
    # ---- swin.hip: 8192 x 16 tokens, 4096 x 4 tokens, 8192 x 256
    _row("layernorm4", "layernorm4_kernel<R>", _S, "launch_layernorm", "rgbd_layernorm / rgbd_layernorm2", "ntok", 8192,
         "tests/test_gpu_swin.py::test_layernorm_grid_stride_forms_and_pair", block=16, note="16 tokens per workgroup"),
    _row("layernorm", "layernorm_kernel", _S, "launch_layernorm", "rgbd_layernorm / rgbd_layernorm2", "ntok", 4096,
         "tests/test_gpu_swin.py::test_layernorm_grid_stride_forms_and_pair", block=4, note="one wave per token, 4 per workgroup"),
    _row("patch_merge_gather", "patch_merge_gather_kernel", _S, "launch_patch_merge_gather", "rgbd_patch_merge_gather",
         "B*(H//2)*(W//2)*C", 8192, "tests/test_gpu_swin.py::test_patch_merge_gather_exact[2-160-192-192-192-784]"),
    _row("pixel_shuffle2", "pixel_shuffle2_kernel", _S, "launch_pixel_shuffle2", "rgbd_pixel_shuffle2", "B*4*H*W*ycs", 8192,
         "tests/test_gpu_swin.py::test_pixel_shuffle2_exact[2-64-96-48-208-64]"),
]
BY_KEY = {r["key"]: r for r in ROWS}
assert len(BY_KEY) == len(ROWS)


def threads(row):
    return row["cap"] * row["block"]


def _eval(formula, dims):
    return int(eval(formula, {"__builtins__": {}}, dict(dims)))


def work_of(row, dims):
    return _eval(row["work"], dims)


def items_of(row, dims):
    return _eval(row["items"], dims)


def crosses(row, dims, sweeps=2):
    """the two conditions of the module docstring -> (ok, work, work past the last full sweep)"""
    T, wk = threads(row), work_of(row, dims)
    past = wk - (sweeps - 1) * T
    return 0 < past < T and past % row["block"] != 0, wk, past


# ================================================================================================ broken loops
def _missed(model, T, block, total):
    if model == "no_loop":
        return lambda i: i >= T
    if model == "last_sweep_dropped":
        last = (total - 1) // T * T
        return lambda i: i >= last
    if model == "stride_long":
        return lambda i: i % (T + block) >= T
    raise KeyError(model)


def dest_mask(d, pred):
    """elements of destination d that depend on a loop index for which pred holds"""
    if "mask_of" in d:
        return d["mask_of"](pred)
    own = d["owner"]
    return (own >= 0) & pred(np.maximum(own, 0))


def spoil(stage, model):
    """{name: what a kernel with the broken loop `model` would leave in the destination}, or None where the model does not
    change a bit (stride_short under a kernel that only writes)."""
    row = BY_KEY[stage["row"]]
    T, block, total = threads(row), row["block"], items_of(row, stage["dims"])
    out = {}
    if model == "stride_short":
        if not stage.get("inplace"):
            return None
        S = T - block
        twice = lambda i: (i >= S) & (i % S < block)  # noqa: E731
        for name, d in stage["dests"].items():
            out[name] = d["want"].copy()
            if name in stage["inplace"]:
                m = dest_mask(d, twice)
                assert m.any()
                out[name] = stage["inplace"][name](out[name], m)
        return out
    pred = _missed(model, T, block, total)
    hit = False
    for name, d in stage["dests"].items():
        m = dest_mask(d, pred)
        hit = hit or bool(m.any())
        out[name] = np.where(m, d["init"], d["want"]).astype(d["want"].dtype)
    assert hit, (stage["row"], model)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    v = np.uint32 if a.dtype.itemsize == 4 else np.uint8
    return np.array_equal(a.view(v), b.view(v))


def _diff(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"{name}: shape {got.shape}, want {want.shape}"
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(-1)) if got.dtype.kind == "f" else \
        np.flatnonzero((got != want).reshape(-1))
    if bad.size == 0:
        bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    if bad.size == 0:
        return f"{name}: rejected"
    return f"{name}: {bad.size} of {got.size} elements differ; first at flat index {int(bad[0])}: got {got.reshape(-1)[bad[0]]!r}, " \
           f"want {want.reshape(-1)[bad[0]]!r}"


def _exact_bits(wants):
    def accept(got):
        return [_diff(k, got[k], w) for k, w in wants.items() if not same_bits(np.asarray(got[k], w.dtype), w)]
    return accept


def _owner(shape):
    return np.arange(int(np.prod(shape)), dtype=np.int32).reshape(shape)


def _padded(a, cs, fill, dtype=None):
    out = np.full(a.shape[:-1] + (cs,), fill, dtype or a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _guarded(a, guard, fill, lead=0):
    a = np.asarray(a)
    return np.concatenate([np.full(lead, fill, a.dtype), a.reshape(-1), np.full(guard, fill, a.dtype)])


# ================================================================================================ entropy.hip: raster slices, LRP
# the issue's two smallest shapes (B, C, h, w), each with per_image 0 and 1
SLICE_SHAPES = [(2, 32, 91, 91), (1, 20, 163, 161)]
SLICE_CASES = [dict(B=B, C=C, h=h, w=w, per_image=p) for (B, C, h, w) in SLICE_SHAPES for p in (0, 1)]
SLICE_FSENT, SLICE_ISENT = F32(7.0), -99  # tests/test_gpu_stf_single.py's pre-fills
LRP_ULPS = 2.0                            # ... and its bound of rgbd_lrp_update against float64


def _stream_place(v_bchw, B, C, h, w, per_image, image_stride, slice_off, n, fill):
    out = np.full(n + 1, fill, v_bchw.dtype)  # (one more than the stream: the test's guard element)
    if per_image:
        for b in range(B):
            o = b * image_stride + slice_off
            out[o:o + C * h * w] = v_bchw[b].reshape(-1)
    else:
        out[slice_off * B:n] = v_bchw.reshape(-1)
    return out


def build_slice(case, np_slice, table):
    """test_slice_kernels_against_numpy's inputs (values on a 1/4 grid with exact ties, scales across the table) and odd channel
    strides at the case's shape; one earlier slice in front of this one in every stream.  np_slice: that file's reference."""
    B, C, h, w, per_image = (case[k] for k in ("B", "C", "h", "w", "per_image"))
    rng = np.random.default_rng(B * 1000 + C * 10 + per_image)
    st = dict(ycs=C + 16, mcs=C + 5, scs=C, cs0=C + 32, cs1=C + 3, lcs=C + 7)
    table = np.asarray(table, F32)
    # (means an eighth off the 1/4 grid: y - mean keeps its exact ties, and y_hat = integer + mean is never the pre-fill 7.0)
    mu = (rng.integers(-40, 40, (B, h, w, C)) / 4 + 0.125).astype(F32)
    y = mu + (rng.integers(-26, 26, (B, h, w, C)) / 4).astype(F32)
    sg = np.exp(rng.uniform(np.log(0.05), np.log(300.0), (B, h, w, C))).astype(F32)
    sg.reshape(-1)[:64] = table
    assert np.any(np.abs((y - mu) % 1.0 - 0.5) == 0)
    slice_off = C * h * w
    image_stride = 2 * C * h * w + 11
    n = B * image_stride if per_image else slice_off * B + B * C * h * w
    rsym, ridx, ryh = np_slice(y, mu, sg, table, B, C, h, w, per_image, image_stride, slice_off)
    assert rsym.shape == (n,)
    own = _owner((B, h, w, C))
    sown = _stream_place(np.ascontiguousarray(own.transpose(0, 3, 1, 2)), B, C, h, w, per_image, image_stride, slice_off, n, -1)
    dims = dict(B=B, C=C, h=h, w=w, npix=B * h * w)
    ii = np.full(n + 1, SLICE_ISENT, np.int32)
    wsym, widx = np.append(rsym, np.int32(SLICE_ISENT)), np.append(ridx, np.int32(SLICE_ISENT))
    o0, o1 = _padded(ryh, st["cs0"], SLICE_FSENT), _padded(ryh, st["cs1"], SLICE_FSENT)
    own0, own1 = _padded(own, st["cs0"], -1), _padded(own, st["cs1"], -1)
    f0, f1 = np.full_like(o0, SLICE_FSENT), np.full_like(o1, SLICE_FSENT)
    quant = dict(row="slice_quant", dims=dims, accept=_exact_bits(dict(sym=wsym, idx=widx, o0=o0, o1=o1)),
                 dests=dict(sym=dict(init=ii, want=wsym, owner=sown), idx=dict(init=ii, want=widx, owner=sown),
                            o0=dict(init=f0, want=o0, owner=own0), o1=dict(init=f1, want=o1, owner=own1)))
    dequant = dict(row="slice_dequant", dims=dims, accept=_exact_bits(dict(q0=o0)), dests=dict(q0=dict(init=f0, want=o0, owner=own0)))
    # LRP: y_hat + 0.5 * tanh(lrp) into two destinations, and in place
    lrp = rng.standard_normal((B, h, w, C)).astype(F32) * rng.choice([1e-4, 0.05, 0.6, 3.0, 30.0], (B, h, w, C)).astype(F32)
    half = 0.5 * np.tanh(lrp.astype(np.float64))
    lrp[(ryh.astype(np.float64) + half).astype(F32) == SLICE_FSENT] = F32(0.05)  # (a result that rounds to the pre-fill: another draw)
    half = 0.5 * np.tanh(lrp.astype(np.float64))
    want64 = ryh.astype(np.float64) + half
    v32 = want64.astype(F32)  # (stands for the device's result on the CPU)
    wa, wb, wi = _padded(v32, st["cs1"], SLICE_FSENT), v32, _padded(v32, st["cs0"], SLICE_FSENT)
    ulp = np.spacing(np.abs(want64).astype(F32)).astype(np.float64)

    def accept_lrp(got):
        a, b2, inp = (np.asarray(got[k], F32) for k in ("a", "b2", "inplace"))
        fails = []
        if not (same_bits(a[..., :C], b2) and (a[..., C:] == SLICE_FSENT).all()):
            fails.append("lrp_update: the two destinations differ, or the pad channels of the first were written")
        if not (same_bits(inp[..., :C], b2) and (inp[..., C:] == SLICE_FSENT).all()):
            fails.append("lrp_update in place: not the out-of-place result after one call, or pad channels written")
        err = float((np.abs(b2.astype(np.float64) - want64) / ulp).max())
        if not err <= LRP_ULPS:
            fails.append(f"lrp_update: {err:.3f} ulp from float64, allowed {LRP_ULPS}")
        return fails

    upd = _padded(half.astype(F32), st["cs0"], 0.0)
    lrp_stage = dict(row="lrp_update", dims=dims, accept=accept_lrp,
                     dests=dict(a=dict(init=f1, want=wa, owner=own1), b2=dict(init=np.full_like(wb, SLICE_FSENT), want=wb, owner=own),
                                inplace=dict(init=o0, want=wi, owner=own0)),
                     inplace=dict(inplace=lambda buf, m: np.where(m, (buf + upd).astype(F32), buf)))
    return dict(strides=st, y=_padded(y, st["ycs"], SLICE_FSENT), mu=_padded(mu, st["mcs"], SLICE_FSENT), sg=_padded(sg, st["scs"], SLICE_FSENT),
                lrp=_padded(lrp, st["lcs"], SLICE_FSENT), slice_off=slice_off, image_stride=image_stride, n=n, table=table,
                stages=dict(quant=quant, dequant=dequant, lrp=lrp_stage))


# ================================================================================================ mlic_loop.hip
MLIC_CASES = [dict(B=2, h=182, w=361)]  # odd width: 181 pixels per row half
MLIC_CS, MLIC_C0 = 96, 32               # a 32-channel slot in the middle of a 96-channel buffer (test_slot_kernels_alone)


def mlic_inputs(case):
    import torch

    B, h, w = case["B"], case["h"], case["w"]
    gen = torch.Generator().manual_seed(100 * h + 10 * w + B)
    buf0 = (torch.randn(B, h, w, MLIC_CS, generator=gen) * 4).numpy()
    r = (torch.randn(B, h, w, 32, generator=gen) * 1.5).numpy()
    return buf0, r


def build_mlic(case, anchor, buf0, r, half_tanh):
    """anchor: test_gpu_mlic._anchor (the numpy masks of test_slot_kernels_alone); half_tanh: rgbd_pw_half_tanh's values on r
    (the device's on the GPU, numpy's float32 rounding of 0.5 * tanh on the CPU)."""
    B, h, w = case["B"], case["h"], case["w"]
    cs, c0 = MLIC_CS, MLIC_C0
    w2 = (w + 1) // 2
    t = (np.arange(B * h, dtype=np.int64)[:, None] * w2 + (np.arange(w) // 2)[None, :]).reshape(B, h, w)
    item = (t[..., None] * 8 + (np.arange(32) // 4)[None, None, None, :]).astype(np.int32)
    ref64 = buf0[..., c0:c0 + 32].astype(np.float64) + 0.5 * np.tanh(r.astype(np.float64))
    upd = (buf0[..., c0:c0 + 32] + half_tanh).astype(F32)  # one fp32 add of the module's value
    stages = {}
    for parity in (0, 1):
        mask = anchor(h, w) if parity == 0 else ~anchor(h, w)
        owner = np.full(buf0.shape, -1, np.int32)
        owner[:, mask, c0:c0 + 32] = item[:, mask]
        want = buf0.copy()
        want[:, mask, c0:c0 + 32] = upd[:, mask]
        bound = 4 * 2.0 ** -24 * (np.abs(ref64).max() + 0.5)

        def accept_apply(got, want=want, mask=mask, bound=bound):
            g = np.asarray(got["buf"], F32)
            fails = [] if same_bits(g, want) else [_diff("lrp_apply", g, want)]
            if g.shape == want.shape and not np.abs(g[:, mask, c0:c0 + 32] - ref64[:, mask]).max() <= bound:
                fails.append("lrp_apply: farther from numpy's tanh than 4 * 2^-24 * (max|ref| + 0.5)")
            return fails

        def again(buf, m):
            twice = buf.copy()
            twice[..., c0:c0 + 32] = (buf[..., c0:c0 + 32] + half_tanh).astype(F32)
            return np.where(m, twice, buf)

        dims = dict(B=B, h=h, w=w)
        stages[f"lrp_apply_p{parity}"] = dict(row="mlic_lrp_apply", dims=dims, accept=accept_apply, inplace=dict(buf=again),
                                              dests=dict(buf=dict(init=buf0, want=want, owner=owner)))
        clear = buf0.copy()
        clear[:, mask, c0:c0 + 32] = 0.0
        stages[f"slot_clear_p{parity}"] = dict(row="mlic_slot_clear", dims=dims, accept=_exact_bits(dict(buf=clear)),
                                               dests=dict(buf=dict(init=buf0, want=clear, owner=owner)))
    return dict(stages=stages)


# rgbd_pw_half_tanh alone: [npix][32] inside strides 40 / 36; against numpy under test_slot_kernels_alone's bound
HALF_TANH_CASES = [dict(npix=65700, C=32, xcs=40, ycs=36)]
HALF_TANH_SENT = F32(12345.0)


def build_half_tanh(case):
    import torch

    npix, C, xcs, ycs = (case[k] for k in ("npix", "C", "xcs", "ycs"))
    r = (torch.randn(npix, C, generator=torch.Generator().manual_seed(npix + C)) * 1.5).numpy()
    ref64 = 0.5 * np.tanh(r.astype(np.float64))
    bound = 4 * 2.0 ** -24 * (np.abs(ref64).max() + 0.5)
    want = _padded(ref64.astype(F32), ycs, HALF_TANH_SENT)
    owner = _padded(_owner((npix, C // 4))[:, np.arange(C) // 4], ycs, -1)

    def accept(got):
        g = np.asarray(got["y"], F32)
        fails = []
        if g.shape != want.shape or not (g[:, C:] == HALF_TANH_SENT).all():
            fails.append("half_tanh: the channels behind C were written")
        elif not np.abs(g[:, :C] - ref64).max() <= bound:
            fails.append(f"half_tanh: {np.abs(g[:, :C] - ref64).max():.3e} from numpy's 0.5 * tanh, allowed {bound:.3e}")
        return fails

    stage = dict(row="pw_half_tanh", dims=dict(npix=npix, C=C), accept=accept,
                 dests=dict(y=dict(init=np.full_like(want, HALF_TANH_SENT), want=want, owner=owner)))
    return dict(x=_padded(r, xcs, np.nan), stages=dict(half_tanh=stage))


# ================================================================================================ coder_abi.hip
CKBD_CASES = [dict(n=1, c=320, h=82, w=162)]
CKBD_FSENT, CKBD_ISENT, CKBD_GUARD = F32(7.0), -99, F32(54321.0)  # tests/test_gpu_coder.py's pre-fill and guard floats


def build_ckbd(case, eo, misaligned):
    """test_ckbd_quant_index_vs_oracle's inputs and oracle at the case's shape, anchor 1 then 0; misaligned: y_hat is elements
    1 .. numel of an allocation with a guard float on either side (test_ckbd_quant_index_misaligned_vs_oracle, form "all")."""
    import torch

    n, c, h, w = (case[k] for k in ("n", "c", "h", "w"))
    g = torch.Generator().manual_seed(n * 1000 + c)
    table = eo.scale_table()
    y = torch.randn(n, c, h, w, generator=g) * 6
    means = torch.randn(n, c, h, w, generator=g)
    scales = torch.exp(torch.randn(n, c, h, w, generator=g) * 2 - 0.5)
    scales.view(-1)[::7] = table[torch.randint(0, 64, ((scales.numel() + 6) // 7,), generator=g)]  # exactly on table entries
    scales.view(-1)[3::11] = 0.05                                                                   # under the bound
    scales.view(-1)[5::13] = -1.0
    y.view(-1)[::5] = (means.view(-1)[::5] + torch.randint(-4, 5, ((y.numel() + 4) // 5,), generator=g).float() + 0.5)  # ties
    m, numel = n * c * h * (w // 2), n * c * h * w
    dims = dict(n=n, c=c, h=h, w=w)
    wrap = (lambda a: _guarded(a, 1, CKBD_GUARD, lead=1)) if misaligned else (lambda a: np.asarray(a).reshape(-1))
    wrap_own = (lambda a: _guarded(a, 1, -1, lead=1)) if misaligned else (lambda a: a.reshape(-1))
    pair = _owner((numel,)) // 2
    col = np.arange(numel) % 2
    row = (np.arange(numel) // w) % h
    stages, want_hat = {}, torch.zeros(n, c, h, w)
    prev = np.full(numel, CKBD_FSENT, F32)
    isent = np.full(m, CKBD_ISENT, np.int32)
    for anchor in (1, 0):
        ws = eo.quantize_symbols(eo.pack(y, bool(anchor)), eo.pack(means, bool(anchor)))
        wi = eo.scale_indexes(eo.pack(scales, bool(anchor)), table)
        want_hat = want_hat + eo.unpack(ws.float() + eo.pack(means, bool(anchor)), bool(anchor))
        wsym, widx, wh = ws.reshape(-1).numpy().astype(np.int32), wi.reshape(-1).numpy().astype(np.int32), want_hat.numpy().reshape(-1).copy()
        # the anchor pass writes both columns of a pair, the other pass the column (row & 1) only
        own_h = pair if anchor else np.where(col == (row & 1), pair, -1).astype(np.int32)

        def accept_q(got, wsym=wsym, widx=widx, wh=wh):
            fails = [_diff(k, got[k], v) for k, v in (("sym", wsym), ("idx", widx)) if not np.array_equal(got[k], v)]
            return fails + ([] if np.array_equal(got["yhat"], wrap(wh)) else [_diff("yhat", got["yhat"], wrap(wh))])

        def accept_d(got, wh=wh):
            return [] if np.array_equal(got["back"], wrap(wh)) else [_diff("back", got["back"], wrap(wh))]

        hat = dict(init=wrap(prev), want=wrap(wh), owner=wrap_own(own_h))
        stages[f"quant_a{anchor}"] = dict(row="ckbd_nchw_quant", dims=dims, accept=accept_q,
                                          dests=dict(sym=dict(init=isent, want=wsym, owner=_owner((m,))),
                                                     idx=dict(init=isent, want=widx, owner=_owner((m,))), yhat=hat))
        stages[f"dequant_a{anchor}"] = dict(row="ckbd_nchw_dequant", dims=dims, accept=accept_d, dests=dict(back=hat))
        prev = wh
    return dict(y=y.numpy(), means=means.numpy(), scales=scales.numpy(), table=np.ascontiguousarray(table.numpy(), F32), m=m,
                numel=numel, stages=stages)


# ================================================================================================ context_attn.hip
DWCONV_CASES = [dict(B=1, H=86, W=85, C=288, gelu=g) for g in (0, 1)]
DWCONV_PAD = 5  # channels behind C in both tensors (test_dwconv_kernel's pad of its batched cases)


def build_dwconv(case, mc, sentinel):
    """test_dwconv_kernel's inputs, reference (mc.dwconv3x3 in float64) and bound (mc.FACTOR * the float32 composition's error)."""
    import torch

    B, H, W, C, gelu = (case[k] for k in ("B", "H", "W", "C", "gelu"))
    x, w, b = mc.dwconv_inputs(B, H, W, C, 3000 + 100 * H + W)
    ref = mc.dwconv3x3(x, w, b, gelu)
    r32 = mc.dwconv3x3(x, w, b, gelu, dtype=torch.float32)
    e32 = mc.rel_err(r32, ref)
    sentinel = F32(sentinel)
    want = _padded(r32.numpy(), C + DWCONV_PAD, sentinel)

    def accept(got):
        g = np.asarray(got["y"], F32)
        if g.shape != want.shape:
            return [f"dwconv: shape {g.shape}"]
        e = mc.rel_err(g[..., :C], ref)
        fails = [] if e <= mc.FACTOR * e32 else [f"dwconv: e_gpu {e:.3e} > {mc.FACTOR} * e32 {e32:.3e}"]
        return fails + ([] if (g[..., C:] == sentinel).all() else ["dwconv: the channels behind C were written"])

    stage = dict(row="dwconv3x3", dims=dict(B=B, H=H, W=W, C=C), accept=accept,
                 dests=dict(y=dict(init=np.full_like(want, sentinel), want=want, owner=_padded(_owner((B, H, W, C)), C + DWCONV_PAD, -1))))
    return dict(x=x, w=w, b=b, e32=e32, stages=dict(dwconv=stage))


# ================================================================================================ pointwise.hip through rgbd_pw_*
# every destination is followed by a guard band of the sentinel, as test_gpu_pointwise_forms._twice lays it out
def _pw_dest(want, owner, guard, lead=0):
    want = _guarded(np.asarray(want, F32), guard, pc.SENTINEL, lead)
    return dict(init=np.full_like(want, pc.SENTINEL), want=want, owner=_guarded(owner, guard, -1, lead))


def _quads(shape, C):
    """owner of [..., c] when item = (flat index of the leading dimensions) * (C / 4) + c / 4"""
    lead = _owner(shape)
    return (lead[..., None] * (C // 4) + (np.arange(C) // 4)).astype(np.int32)


COPY_CASES = [dict(npix=104975, C=20, scs=32, dcs=24, sweeps=2), dict(npix=209800, C=20, scs=32, dcs=24, sweeps=3)]


def build_copy(case):
    npix, C, scs, dcs = (case[k] for k in ("npix", "C", "scs", "dcs"))
    src = pc.copy_input(npix, C, scs)
    want = pc.copy_ref(src, C, dcs)
    d = _pw_dest(want, _padded(_quads((npix,), C), dcs, -1), dcs)
    return dict(src=src, guard=dcs, stages=dict(copy=dict(row="pw_copy_channels", dims=dict(npix=npix, C=C), dests=dict(dst=d),
                                                          accept=_exact_bits(dict(dst=d["want"])))))


FILL_LEAD, FILL_GUARD = 3, 64  # test_fill_zero_inside_a_guarded_buffer's layout
FILL_CASES = [dict(n=4 * 524288 + 2301, sweeps=2), dict(n=4 * 1048576 + 1697, sweeps=3)]


def build_fill(case):
    n = case["n"]
    d = _pw_dest(np.zeros(n, F32), _owner((n,)), FILL_GUARD, FILL_LEAD)
    return dict(stages=dict(fill=dict(row="pw_fill_zero", dims=dict(n=n), dests=dict(dst=d), accept=_exact_bits(dict(dst=d["want"])))))


SCALE_CASES = [dict(HW=32801, mode=m) for m in (0, 1)]  # the se_cat_to form (pc.CAT): both launches cross the cap


def build_scale(case):
    HW, mode = case["HW"], case["mode"]
    c = pc.CAT
    own, other, gate = pc.cat_input(HW)
    want = pc.cat_ref(own, other, gate, mode)
    N, oc, tc, dcs = c["N"], c["own_c"], c["other_c"], c["dst_cs"]
    o1 = np.full(want.shape, -1, np.int32)
    o1[..., :oc] = _quads((N, HW), oc)
    o2 = np.full(want.shape, -1, np.int32)
    o2[..., oc:oc + tc] = _quads((N, HW), tc)
    d1, d2 = _pw_dest(want, o1, dcs), _pw_dest(want, o2, dcs)

    def accept(got):
        g = np.asarray(got["dst"], F32)
        ok = g.shape == d1["want"].shape and pc.exact(g[:want.size].reshape(want.shape), want) == (True, 0) and \
            (g[want.size:] == pc.SENTINEL).all()
        return [] if ok else [_diff("channel_scale", g, d1["want"])]

    return dict(own=own, other=other, gate=gate, guard=dcs,
                stages=dict(own=dict(row="pw_channel_scale", dims=dict(N=N, HW=HW, C=oc), dests=dict(dst=d1), accept=accept),
                            other=dict(row="pw_channel_scale", dims=dict(N=N, HW=HW, C=tc), dests=dict(dst=d2), accept=accept)))


BILINEAR_CASES = [dict(N=1, h=19, w=25, cs=20, H=325, W=323)]  # up both ways, non-integer ratios; 5 float4s per pixel


def build_bilinear(case):
    N, h, w, cs, H, W = (case[k] for k in ("N", "h", "w", "cs", "H", "W"))
    x = pc.bilinear_input(N, h, w, cs)
    want = pc.bilinear(x, H, W).astype(F32)  # (stands for the device's result on the CPU)
    guard = W * cs
    d = _pw_dest(want, _quads((N, H, W), cs), guard)

    def accept(got):
        g = np.asarray(got["dst"], F32)
        if g.shape != d["want"].shape or not (g[want.size:] == pc.SENTINEL).all():
            return ["bilinear: the guard band was written"]
        ok, sh = pc.accept_bilinear(g[:want.size].reshape(N, H, W, cs), x)
        return [] if ok else [f"bilinear: {sh:.3g} of the float64 bound"]

    return dict(x=x, guard=guard, stages=dict(bilinear=dict(row="pw_bilinear", dims=dict(N=N, H=H, W=W, cs=cs), dests=dict(dst=d),
                                                             accept=accept)))


MAXPOOL_CASES = [dict(N=1, H=550, W=547, cs=64)]  # 182 x 181 outputs of 16 float4s


def build_maxpool(case):
    N, H, W, cs = (case[k] for k in ("N", "H", "W", "cs"))
    x = pc.bilinear_input(N, H, W, cs, key=1)  # (the input family of test_pair_launches_give_each_sets_own_bits)
    want = pc.maxpool7s3(x)
    OH, OW = want.shape[1:3]
    d = _pw_dest(want, _quads((N, OH, OW), cs), OW * cs)
    return dict(x=x, guard=OW * cs, n=want.size,
                stages=dict(maxpool=dict(row="pw_maxpool7s3", dims=dict(N=N, H=H, W=W, cs=cs), dests=dict(dst=d),
                                         accept=_exact_bits(dict(dst=d["want"])))))


IM2COL_CASES = [dict(N=2, H=229, W=229, C=1, KP=80)]  # 115 x 115 outputs of 20 float4s, two images


def build_im2col(case):
    N, H, W, C, KP = (case[k] for k in ("N", "H", "W", "C", "KP"))
    x = pc.im2col_input(N, H, W, C)
    want = pc.im2col5s2(x, C, KP)
    OH, OW = (H + 1) // 2, (W + 1) // 2
    d = _pw_dest(want, _quads((N, OH, OW), KP), OW * KP)
    return dict(x=x, guard=OW * KP, n=want.size,
                stages=dict(im2col=dict(row="pw_im2col5s2", dims=dict(N=N, H=H, W=W, KP=KP), dests=dict(dst=d),
                                        accept=_exact_bits(dict(dst=d["want"])))))


# each direction at a shape of its own (the two work formulas differ by C against cs / 4): N, C, H, W, cs
TO_NHWC_CASES = [dict(N=1, C=20, H=259, W=254, cs=32, perm=p) for p in (0, 1)]
TO_NCHW_CASES = [dict(N=1, C=20, H=163, W=161, cs=32, perm=p, clamp01=p) for p in (0, 1)]


def build_to_nhwc(case):
    N, C, H, W, cs, perm = (case[k] for k in ("N", "C", "H", "W", "cs", "perm"))
    src = pc.layout_nchw_input(N, C, H, W)
    want = pc.to_nhwc(src, cs, perm)
    d = _pw_dest(want, _quads((N, H, W), cs), W * cs)
    return dict(src=src, guard=W * cs, n=want.size,
                stages=dict(to_nhwc=dict(row="pw_nchw_to_nhwc", dims=dict(N=N, H=H, W=W, cs=cs), dests=dict(dst=d),
                                         accept=_exact_bits(dict(dst=d["want"])))))


def build_to_nchw(case):
    N, C, H, W, cs, perm, clamp01 = (case[k] for k in ("N", "C", "H", "W", "cs", "perm", "clamp01"))
    x = pc.layout_nhwc_input(N, C, H, W, cs, perm, clamp01)
    want = pc.to_nchw(x, C, perm, clamp01)
    d = _pw_dest(want, _owner((N, C, H, W)), W)

    def accept(got):
        g = np.asarray(got["dst"], F32)
        ok = g.shape == d["want"].shape and pc.exact(g[:want.size].reshape(want.shape), want) == (True, 0) and \
            (g[want.size:] == pc.SENTINEL).all() and (clamp01 or same_bits(g, d["want"]))
        return [] if ok else [_diff("nhwc_to_nchw", g, d["want"])]

    return dict(x=x, guard=W, n=want.size,
                stages=dict(to_nchw=dict(row="pw_nhwc_to_nchw", dims=dict(N=N, C=C, H=H, W=W), dests=dict(dst=d), accept=accept)))


# ================================================================================================ the reference-arithmetic hooks
# The hooks stage NCHW tensors through the layout kernels (which cross their own caps at these sizes); the kernel under test writes
# a staging buffer that the caller cannot pre-fill, so what a broken loop leaves behind is that buffer's content: zeros behind
# small_conv_ref_kernel (the hook clears it), whatever the allocation held behind the others.  The CPU models put the file's
# pre-fill, 7.0, there -- a stand-in, not what the device would show.  On the device it is the FIRST call's bit-for-bit comparison
# that catches an unwritten element; the second call says nothing about it (a reused allocation can still hold the first call's
# correct values) and only shows that two calls agree.
REF_SENT = F32(7.0)


def _cperm(c):
    return pc.cperm(c)


def sigmoid_case(rc):
    return rc._sig((1, 7, 363, 363), 8, 0, True, True, False)  # 7 of 16 stored channels; the gate's whole epilogue


def build_sigmoid(rc):
    c = sigmoid_case(rc)
    t, mul, res, tail, planted, special = rc.sigmoid_inputs(c)
    want = rc.sigmoid_expected(c, t, mul, res)
    n, ch, h, w = t.shape
    pix = _owner((n, h * w))  # n * HW + hw
    owner = (pix[:, None, :] * 16 + _cperm(np.arange(ch))[None, :, None]).astype(np.int32).reshape(n, ch, h, w)

    def accept(got):
        g = np.asarray(got["y"], F32)
        ok = g.shape == want.shape and np.array_equal(g, want, equal_nan=True) and rc.bits_equal(g, want)
        return [] if ok else [_diff("sigmoid_gate", g, want)]

    stage = dict(row="sigmoid_gate_ref", dims=dict(n=n, c=ch, h=h, w=w), accept=accept,
                 dests=dict(y=dict(init=np.full_like(want, REF_SENT), want=want, owner=owner)))
    return dict(case=c, t=t, mul=mul, res=res, stages=dict(sigmoid=stage))


def small_conv_case(rc):
    # 3 -> 16 channels, 3 x 3, two uneven K blocks, leaky ReLU between res1 and mul: 181 x 182 outputs
    return rc._sc("gridcap", 1, 3, 16, 3, 181, 182, 1, 1, [11, 16], rc.ACT_LEAKY, True, True, False)


def build_small_conv(rc):
    c = small_conv_case(rc)
    x, wt, b, extra = rc.small_conv_inputs(c)
    want = rc.small_conv_expected(c, x, wt, b, extra)
    n, o, oh, ow = want.shape
    owner = (_owner((n, oh, ow))[:, None] * o + np.arange(o)[None, :, None, None]).astype(np.int32)

    def accept(got):
        g = np.asarray(got["y"], F32)
        return [] if g.shape == want.shape and np.array_equal(g, want) else [_diff("small_conv", g, want)]

    stage = dict(row="small_conv_ref", dims=dict(n=n, OH=oh, OW=ow, cout=o), accept=accept,
                 dests=dict(y=dict(init=np.zeros_like(want), want=want, owner=owner)))
    return dict(case=c, x=x, wt=wt, b=b, extra=extra, stages=dict(small_conv=stage))


def deconv_case(rc):
    """16 -> 64 channels on 181 x 182 pixels, every phase one column class ("whole"): per phase one gather of nt x 4 float4s and one
    scatter of 16 float4s per pixel."""
    B, cin, cout, h, w = 1, 16, 64, 181, 182
    flat = rc.draw_recipe(w, rc._rng("deconv-recipe", B, cin, cout, h, w), "drawn", "whole")
    return dict(id=f"gridcap-{B}-{cin}-{cout}-{h}x{w}", B=B, cin=cin, cout=cout, h=h, w=w, recipe=flat, act=rc.ACT_LEAKY, variant="drawn")


def build_deconv(rc):
    c = deconv_case(rc)
    x, wt, b = rc.deconv_inputs(c)
    want = rc.deconv_expected(c, x, wt, b)
    B, cin, cout, h, w = (c[k] for k in ("B", "cin", "cout", "h", "w"))
    cin_pad, cout_pad = (cin + 15) // 16 * 16, (cout + 15) // 16 * 16
    init = np.full_like(want, REF_SENT)
    pix = _owner((B, h, w))  # (n * h + ty) * jw + tx with jw = w
    stages = {}
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        nt = len(rc.phase_taps(py, px))
        # scatter: item = pixel * (cout_pad / 4) + c4 -> y[n][perm(c)][2 ty + py][2 tx + px]
        own = np.full(want.shape, -1, np.int32)
        own[:, :, py::2, px::2] = (pix[:, None] * (cout_pad // 4) + (_cperm(np.arange(cout)) // 4)[None, :, None, None]).astype(np.int32)
        dims = dict(B=B, h=h, jw=w, nt=nt, cin_pad=cin_pad, cout_pad=cout_pad)
        acc = _exact_bits(dict(y=want))
        stages[f"scatter_ph{ph}"] = dict(row="scatter_phase", dims=dims, accept=acc, dests=dict(y=dict(init=init, want=want, owner=own)))
        # gather: a pixel's items are [pixel * nt * c4n, (pixel + 1) * nt * c4n); one that is missing spoils the pixel's K row,
        # and with it every channel of the output pixel
        per = nt * (cin_pad // 4)

        def mask_of(pred, per=per, py=py, px=px):
            bad = pred(np.arange(B * h * w * per, dtype=np.int64)).reshape(B, h, w, per).any(axis=-1)
            m = np.zeros(want.shape, bool)
            m[:, :, py::2, px::2] = bad[:, None]
            return m

        stages[f"gather_ph{ph}"] = dict(row="gather_taps", dims=dims, accept=acc, dests=dict(y=dict(init=init, want=want, mask_of=mask_of)))
    return dict(case=c, x=x, wt=wt, b=b, stages=stages)


def deconv_wide_case(rc):
    """gather_wslabs_kernel's work is cout_pad * taps * cin_pad / 4, whatever the map: 496 -> 496 channels on 2 x 4 pixels, every
    phase one column class.  The 9-tap phase gathers 553 536 float4s (two sweeps, the second one ragged); the others stay below."""
    B, cin, cout, h, w = 1, 496, 496, 2, 4
    flat = rc.draw_recipe(w, rc._rng("deconv-recipe", B, cin, cout, h, w), "drawn", "whole")
    return dict(id=f"gridcap-{B}-{cin}-{cout}-{h}x{w}", B=B, cin=cin, cout=cout, h=h, w=w, recipe=flat, act=rc.ACT_LEAKY, variant="drawn")


def build_deconv_wide(rc):
    c = deconv_wide_case(rc)
    x, wt, b = rc.deconv_inputs(c)
    want = rc.deconv_expected(c, x, wt, b)
    cin, cout = c["cin"], c["cout"]
    cin_pad, cout_pad = (cin + 15) // 16 * 16, (cout + 15) // 16 * 16
    nt = len(rc.phase_taps(0, 0))
    per = nt * (cin_pad // 4)  # the items of one output row of the gathered weights: [co * per, (co + 1) * per)

    def mask_of(pred):
        """a missing item spoils the K row of the output channel stored at position co: that channel, at every pixel of phase (0, 0)"""
        bad = pred(np.arange(cout_pad * per, dtype=np.int64)).reshape(cout_pad, per).any(axis=-1)
        m = np.zeros(want.shape, bool)
        m[:, :, 0::2, 0::2] = bad[_cperm(np.arange(cout))][None, :, None, None]
        return m

    stage = dict(row="gather_wslabs", dims=dict(cout_pad=cout_pad, nt=nt, cin_pad=cin_pad), accept=_exact_bits(dict(y=want)),
                 dests=dict(y=dict(init=np.full_like(want, REF_SENT), want=want, mask_of=mask_of)))
    return dict(case=c, x=x, wt=wt, b=b, stages=dict(wslabs_ph0=stage))


# ================================================================================================ conv_mfma.hip: the split-K reducer
def splitk_case(cc):
    # 1 x 1, 32 -> 48 channels, two partial planes of 181 x 243 pixels: 12 float4s per pixel; res1 and ReLU in the reducer
    return cc._case("gridcap-splitk", "plain", 1, 32, 181, 243, 48, 1, splitk=2, res1=True, act=cc.ACT_RELU)


def build_splitk(cc):
    import torch

    c = splitk_case(cc)
    ins = cc.inputs(c)
    ref = cc.reference64(c, ins)
    oh, ow = cc.out_hw(c)
    n, cy = c["n"], cc.y_channels(c)
    cout_pad = cc.round_up(cy, 16)
    want = cc.torch_compose(c, ins, torch.float32)["y"].numpy()  # (stands for the device's result on the CPU)
    owner = (_owner((n, oh, ow))[:, None] * (cout_pad // 4) + (np.arange(cy) // 4)[None, :, None, None]).astype(np.int32)
    init = np.full_like(want, cc.FILL)

    def accept(got):
        g = np.asarray(got["y"], F32)
        if g.shape != want.shape:
            return [f"split-K: shape {g.shape}"]
        fails = []
        if (g.view(np.uint32) == cc.FILL_BITS).any():
            fails.append(f"split-K: {int((g.view(np.uint32) == cc.FILL_BITS).sum())} computed positions were left unwritten")
        err = np.abs(g.astype(np.float64) - ref["y"])
        if not (err <= ref["bound_y"]).all():
            fails.append(f"split-K: max err {err.max():.3e}, bound {ref['bound_y']:.3e}")
        return fails

    stage = dict(row="splitk_reduce", dims=dict(groups=1, n=n, OH=oh, OW=ow, cout_pad=cout_pad), accept=accept,
                 dests=dict(y=dict(init=init, want=want, owner=owner)))
    return dict(case=c, ins=ins, stages=dict(splitk=stage))


# ================================================================================================ every case, for the CPU test
def case_list():
    """[(id, sweeps, rows the case builds stages for, build(refs))].  refs: the references that live in GPU test files
    ({"np_slice", "anchor"}) and the case and oracle modules ({"eo", "mc", "rc", "cc"})."""
    out = []
    for c in SLICE_CASES:
        out.append(("slice-%(B)dx%(C)dx%(h)dx%(w)d-pi%(per_image)d" % c, 2, ("slice_quant", "slice_dequant", "lrp_update"),
                    lambda refs, c=c: build_slice(c, refs["np_slice"], refs["eo"].scale_table().numpy())))

    def mlic(refs, c):
        buf0, r = mlic_inputs(c)
        return build_mlic(c, refs["anchor"], buf0, r, (0.5 * np.tanh(r.astype(np.float64))).astype(F32))

    for c in MLIC_CASES:
        out.append(("mlic-%(B)dx%(h)dx%(w)d" % c, 2, ("mlic_lrp_apply", "mlic_slot_clear"), lambda refs, c=c: mlic(refs, c)))
    for c in HALF_TANH_CASES:
        out.append(("half_tanh-%(npix)d" % c, 2, ("pw_half_tanh",), lambda refs, c=c: build_half_tanh(c)))
    for c in CKBD_CASES:
        for mis in (False, True):
            out.append(("ckbd-%dx%dx%dx%d-%s" % (c["n"], c["c"], c["h"], c["w"], "misaligned" if mis else "aligned"), 2,
                        ("ckbd_nchw_quant", "ckbd_nchw_dequant"), lambda refs, c=c, mis=mis: build_ckbd(c, refs["eo"], mis)))
    for c in DWCONV_CASES:
        out.append(("dwconv-gelu%(gelu)d" % c, 2, ("dwconv3x3",), lambda refs, c=c: build_dwconv(c, refs["mc"], 12345.0)))
    for name, row, cases, build in (("copy", "pw_copy_channels", COPY_CASES, build_copy), ("fill", "pw_fill_zero", FILL_CASES, build_fill),
                                    ("scale", "pw_channel_scale", SCALE_CASES, build_scale),
                                    ("bilinear", "pw_bilinear", BILINEAR_CASES, build_bilinear),
                                    ("maxpool", "pw_maxpool7s3", MAXPOOL_CASES, build_maxpool),
                                    ("im2col", "pw_im2col5s2", IM2COL_CASES, build_im2col),
                                    ("to_nhwc", "pw_nchw_to_nhwc", TO_NHWC_CASES, build_to_nhwc),
                                    ("to_nchw", "pw_nhwc_to_nchw", TO_NCHW_CASES, build_to_nchw)):
        for i, c in enumerate(cases):
            out.append((f"{name}-{i}", c.get("sweeps", 2), (row,), lambda refs, c=c, build=build: build(c)))
    out.append(("sigmoid_gate", 2, ("sigmoid_gate_ref",), lambda refs: build_sigmoid(refs["rc"])))
    out.append(("small_conv", 2, ("small_conv_ref",), lambda refs: build_small_conv(refs["rc"])))
    out.append(("deconv_s2", 2, ("gather_taps", "scatter_phase"), lambda refs: build_deconv(refs["rc"])))
    out.append(("deconv_s2_wide", 2, ("gather_wslabs",), lambda refs: build_deconv_wide(refs["rc"])))
    out.append(("splitk", 2, ("splitk_reduce",), lambda refs: build_splitk(refs["cc"])))
    return out
