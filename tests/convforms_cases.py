"""Cases shared by tests/test_convforms_cases.py (CPU: are the cases and their bounds worth running?) and
tests/test_gpu_convforms.py (GPU: the conv launchers in their fused, grouped and sliced forms through rgbd_conv_forms_nchw).

Pure numpy / torch-CPU / oracle code.  For every case: deterministic inputs (seeds are a function of the case id and the operand
set), the fp64 reference with its derived error bound, torch's own fp32 composition, and -- for the cases that run the
reference's CPU arithmetic ("blocked") -- the bit-exact chain of oracle/cpu_arith.c.

Forms (the fields of a case):
  plain   y = act(conv(x) + b + res1) * mul + res2, optionally copied to y2
  fused   t = act_mid(conv(x) + b);  y = act(conv1x1(t, w2) + b2 + res1)
  lead    ... and u = relu(conv1x1(y, w3) + b3) -> y3
  slice   plain, with the input / output a channel slice of a wider tensor
Every form can run as a grouped launch (groups == 2: a second operand set that differs in every tensor).

Error bound of the fp64 comparisons (no new number: the per-layer rule of tests/test_gpu_conv.py, composed):
  one conv layer whose output has magnitude M              2e-5 * (M + 1e-3)
  a chain                                                  the sum of its layers' bounds, every earlier layer's bound multiplied
                                                           by the inf-operator-norm (largest row sum of |w|) of each 1x1 behind it
  mul is drawn from (0, 1) (a sigmoid gate in the model)   leaves the bound as it is
  res2                                                     + 2^-23 * max|ref|
  GELU (family "gelu": the reducer's activation)           1.129 * (the conv rule on the pre-activation v) + max B_act, and, against
                                                           the launch's own fp32 pre-activation, B_act(v) element by element:
                                                           B_act(v) = (0.5 |v| (E_ERF + 2) + |gelu(v)|) 2^-24 + 2^-149  (act_bound)
                                                           E_ERF = 4 x the error of torch's CPU fp32 erf on the cases' arguments
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_arith as ca

f32 = np.float32
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2, 3
ACT_GELU = 4  # erf form; applied by the split-K reducer (csrc/conv_mfma.hip), with one partial plane when the split factor is 1
FILL_BITS = 0x4B3C614E  # what the destinations are pre-filled with (a finite float, ~1.2e7: no result of a case comes near it)
FILL = np.array([FILL_BITS], np.uint32).view(f32)[0]
X_FILL = (3.5, -1234.5)  # the two values the channels next to a sliced input are filled with


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) % (2 ** 31))


def case_id(c):
    return c["id"]


def _case(cid, family, n, cin, h, w, cout, k, **kw):
    c = dict(id=cid, family=family, n=n, cin=cin, h=h, w=w, cout=cout, k=k, stride=1, pad=k // 2, transposed=0, act=ACT_NONE,
             cout2=0, act_mid=0, cout3=0, res1=False, mul=False, res2=False, y2=False, x_off=0, x_total=cin, y_off=0, y_total=None,
             y2_off=0, y2_total=None, y3_off=0, y3_total=None, groups=1, blocked=False, splitk=1, ckbd=0, seed=0)
    assert set(kw) <= set(c), kw
    c.update(kw)
    cy = c["cout2"] or cout
    if c["y_total"] is None:
        c["y_total"] = cy
    if c["y2_total"] is None:
        c["y2_total"] = cy
    if c["y3_total"] is None:
        c["y3_total"] = c["cout3"]
    return c


def out_hw(c):
    h, w, k, s, p = c["h"], c["w"], c["k"], c["stride"], c["pad"]
    if c["transposed"]:
        return (h - 1) * s - 2 * p + k + (s - 1), (w - 1) * s - 2 * p + k + (s - 1)
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def y_channels(c):
    return c["cout2"] or c["cout"]


def round_up(v, m):
    return (v + m - 1) // m * m


def cout_store(c):
    """Channels a launch stores (Engine::conv_plan): the slice rounded up to 4 when it is narrower than its 16-padded width inside
    a wider buffer, else the 16-padded width."""
    cy = y_channels(c)
    return round_up(cy, 4) if cy % 16 and round_up(c["y_total"], 16) != round_up(cy, 16) else round_up(cy, 16)


def pick_tw(gw, gh, tp):
    """Tile width the launcher picks for a tp-pixel tile (csrc/conv_mfma_body.h: pick_tw_log2)."""
    best, best_cost = 4, -1
    for l in (2, 3, 4):
        tw, th = 1 << l, tp >> l
        if th < 1:
            continue
        cost = -(-gw // tw) * -(-gh // th)
        if best_cost < 0 or cost < best_cost or (cost == best_cost and l > best):
            best, best_cost = l, cost
    return 1 << best


# ================================================================================================ the case list
def _build():
    R, L, S = ACT_RELU, ACT_LEAKY, ACT_SIGMOID
    cs = []
    # ---- fused tail: (n, cin, h, w, cout, k), cout2, res1, act, act_mid
    fused = [
        ((1, 16, 1, 1, 96, 3), 96, True, R, 1),
        ((2, 48, 1, 17, 81, 1), 84, False, 0, 0),
        ((3, 96, 33, 1, 90, 3), 177, True, L, 1),
        ((1, 213, 3, 5, 96, 3), 192, True, R, 1),
        ((1, 96, 9, 15, 96, 1), 288, False, R, 0),
        ((2, 48, 5, 16, 90, 3), 192, False, L, 1),
        ((1, 16, 7, 33, 81, 1), 96, False, 0, 1),
        ((1, 96, 3, 65, 96, 3), 84, True, R, 1),
        ((1, 48, 2, 129, 96, 1), 288, True, 0, 1),
        ((1, 213, 17, 17, 90, 1), 177, False, R, 1),
    ]
    for shp, c2, r1, act, mid in fused:
        cs.append(_case("fused-%dx%dx%dx%d-c%d-k%d-o%d-r%d-a%d-m%d" % (shp + (c2, r1, act, mid)), "fused", *shp, cout2=c2, res1=r1, act=act,
                        act_mid=mid))
    cs.append(_case("fused-grouped", "fused", 2, 96, 9, 13, 96, 3, cout2=192, res1=True, act=R, act_mid=1, groups=2))
    cs.append(_case("fused-16x16", "fused", 1, 48, 16, 16, 96, 3, cout2=96, res1=True, act=R, act_mid=1))  # (tiles that end with the map)
    cs.append(_case("fused-grouped-nores", "fused", 1, 48, 4, 21, 81, 1, cout2=84, act=L, act_mid=0, groups=2))
    # the output a slice narrower than its padded width (84 of 100), at offset 0 and behind another slice; the input a slice
    cs.append(_case("fused-slice-o0", "fused", 1, 48, 6, 11, 96, 3, cout2=84, res1=True, act=R, act_mid=1, y_total=100, x_off=16, x_total=80))
    cs.append(_case("fused-slice-o16", "fused", 2, 96, 3, 20, 90, 1, cout2=84, act=0, act_mid=1, y_off=16, y_total=100))
    # the reference's CPU arithmetic: blocked first layer, the 1x1 chains start at their bias
    cs.append(_case("fused-blk-k3", "fused", 2, 96, 9, 17, 96, 3, cout2=192, res1=True, act=0, act_mid=1, blocked=True))
    cs.append(_case("fused-blk-k1", "fused", 1, 48, 5, 15, 96, 1, cout2=96, res1=True, act=R, act_mid=1, blocked=True))
    cs.append(_case("fused-blk-c213", "fused", 1, 213, 4, 9, 90, 3, cout2=288, act=R, act_mid=1, blocked=True))
    cs.append(_case("fused-blk-grouped", "fused", 1, 96, 6, 10, 96, 3, cout2=192, res1=True, act=0, act_mid=1, blocked=True, groups=2))
    # ---- fused tail + the next block's lead layer
    cs.append(_case("lead-c96-own", "lead", 1, 96, 5, 17, 96, 3, cout2=96, cout3=96, res1=True, act=R, act_mid=1))
    cs.append(_case("lead-c192-own90", "lead", 2, 48, 3, 33, 90, 1, cout2=192, cout3=90, res1=True, act=0, act_mid=1))
    cs.append(_case("lead-c288-slice", "lead", 1, 96, 9, 9, 96, 3, cout2=288, cout3=96, res1=True, act=R, act_mid=1, y3_off=32, y3_total=160))
    cs.append(_case("lead-c177-tail90", "lead", 3, 16, 1, 15, 96, 3, cout2=177, cout3=90, act=L, act_mid=0, y3_off=96, y3_total=186))
    cs.append(_case("lead-16x16", "lead", 1, 16, 16, 16, 90, 1, cout2=96, cout3=96, act=R, act_mid=1))
    cs.append(_case("lead-grouped", "lead", 1, 96, 10, 12, 96, 3, cout2=192, cout3=96, res1=True, act=R, act_mid=1, groups=2))
    cs.append(_case("lead-blk", "lead", 2, 96, 7, 16, 96, 3, cout2=192, cout3=96, res1=True, act=0, act_mid=1, blocked=True))
    cs.append(_case("lead-blk-grouped", "lead", 1, 96, 4, 20, 81, 1, cout2=96, cout3=96, res1=True, act=R, act_mid=1, blocked=True, groups=2))
    # ---- plain form: every operand combination the engine issues (none / res1 / sigmoid gate / gate + skip), each with a second
    # destination, each under split-K 1 and 4 (a second destination with split-K is refused: test_refusals)
    combos = [("none", dict(act=R)), ("r1", dict(res1=True)), ("m", dict(mul=True, act=S)), ("mr2", dict(mul=True, res2=True, act=S))]
    shapes = {"none": (2, 64, 8, 12, 48, 3), "r1": (1, 192, 16, 16, 96, 1), "m": (3, 64, 5, 7, 64, 1), "mr2": (1, 96, 12, 9, 96, 1)}
    for name, kw in combos:
        shp = shapes[name]
        cs.append(_case("plain-%s" % name, "plain", *shp, **kw))
        # (bi_spf: each extractor writes its features into a half of both concat buffers)
        cs.append(_case("plain-%s-y2" % name, "plain", *shp, y2=True, y_total=2 * shp[4], y2_off=shp[4], y2_total=2 * shp[4], **kw))
        cs.append(_case("plain-%s-split4" % name, "plain", *shp, splitk=4, **kw))
    cs.append(_case("plain-s2-k5", "plain", 1, 48, 11, 15, 42, 5, stride=2, pad=2, res1=True, act=L))
    cs.append(_case("plain-deconv-s2", "plain", 2, 32, 3, 5, 24, 5, stride=2, pad=2, transposed=1, act=R))
    cs.append(_case("plain-1x1grid", "plain", 2, 32, 1, 1, 40, 3, res1=True, act=R))
    cs.append(_case("plain-ckbd1", "plain", 2, 48, 7, 10, 64, 5, pad=2, act=R, ckbd=1))
    cs.append(_case("plain-ckbd2-split4", "plain", 1, 128, 6, 9, 32, 3, res1=True, ckbd=2, splitk=4))
    cs.append(_case("plain-grouped-r1", "plain", 2, 64, 6, 17, 48, 3, res1=True, act=R, groups=2))
    cs.append(_case("plain-grouped-mr2-split4", "plain", 1, 128, 9, 5, 80, 1, mul=True, res2=True, act=S, splitk=4, groups=2))
    cs.append(_case("plain-grouped-r1-split4", "plain", 2, 96, 4, 6, 32, 3, res1=True, act=R, splitk=4, groups=2))
    cs.append(_case("plain-grouped-ckbd", "plain", 1, 32, 8, 8, 32, 3, act=R, ckbd=1, groups=2))
    cs.append(_case("plain-grouped-y2", "plain", 1, 48, 5, 9, 32, 3, act=R, y2=True, y_total=64, y2_off=32, y2_total=64, groups=2))
    cs.append(_case("plain-blk-r1", "plain", 1, 80, 6, 7, 48, 3, res1=True, act=R, blocked=True))
    cs.append(_case("plain-blk-k1-mr2", "plain", 2, 64, 3, 5, 32, 1, mul=True, res2=True, act=L, blocked=True))
    # ---- slices: 24 of 48 at offset 0 and at 24 (STF_united), the input at a 16-multiple offset of a wider tensor
    cs.append(_case("slice-out-o0", "slice", 1, 48, 6, 10, 24, 3, act=R, y_total=48))
    cs.append(_case("slice-out-o24", "slice", 2, 48, 4, 5, 24, 1, res1=True, y_off=24, y_total=48))
    cs.append(_case("slice-in-o32", "slice", 1, 24, 5, 8, 40, 3, act=R, x_off=32, x_total=96))
    cs.append(_case("slice-in-out-split4", "slice", 1, 72, 3, 7, 24, 1, splitk=4, x_off=16, x_total=112, y_off=24, y_total=72, mul=True,
                    res2=True, act=S))
    cs.append(_case("slice-grouped", "slice", 2, 40, 3, 4, 24, 3, act=L, x_off=16, x_total=64, y_off=24, y_total=48, groups=2))
    # ---- GELU: the reducer's activation, over one partial plane (split factor 1) or several.  Each case mirrors a launch of the
    # engine; maps of at most 400 pixels.
    G = ACT_GELU
    cs.append(_case("gelu-k1", "gelu", 2, 48, 5, 9, 192, 1, act=G))                              # Swin mlp.fc1, C -> 4C
    cs.append(_case("gelu-k1-grouped", "gelu", 1, 32, 3, 11, 128, 1, act=G, groups=2))           # swin_block_tail2: two modalities
    cs.append(_case("gelu-k1-split3", "gelu", 1, 112, 3, 7, 40, 1, act=G, splitk=3))             # chunks of 3, 3, 1 groups; cout 40 -> 48
    cs.append(_case("gelu-k3", "gelu", 2, 40, 7, 6, 100, 3, act=G))                              # h_a_stf1, stride 1; pad channels on both sides
    cs.append(_case("gelu-k3-s2", "gelu", 2, 32, 9, 7, 48, 3, act=G, stride=2, pad=1))           # h_a_stf1, stride 2 (5 x 4 outputs)
    cs.append(_case("gelu-k3-grouped-split2", "gelu", 1, 64, 4, 6, 128, 3, act=G, groups=2, splitk=2))  # h_s_stf1, sub-pixel layer
    cs.append(_case("gelu-1x1grid", "gelu", 2, 32, 1, 1, 40, 1, act=G, seed=1))                  # one pixel per image (80 values:
    # the first draw has none within 0.1 of zero -- test_convforms_cases.py::test_gelu_case_is_not_hollow)
    ids =[c["id"] for c in cs]
    assert len(set(ids)) == len(ids)
    return cs


CASES = _build()
FAMILIES = ("plain", "fused", "lead", "slice", "gelu")


# ================================================================================================ inputs
def inputs(c, g=0, x_fill=X_FILL[0]):
    """Operand set g of case c (float32, NCHW).  x is the whole wide input tensor: the channels next to the slice hold x_fill."""
    r = _rng(c["id"], g, c["seed"]) if c["seed"] else _rng(c["id"], g)  # (seed: another draw for a case too small to be sure of its shares)
    n, cin, h, w, cout, k = c["n"], c["cin"], c["h"], c["w"], c["cout"], c["k"]
    oh, ow = out_hw(c)
    cy = y_channels(c)
    d = {}
    x = np.full((n, c["x_total"], h, w), x_fill, f32)
    x[:, c["x_off"]:c["x_off"] + cin] = r.standard_normal((n, cin, h, w))
    d["x"] = x
    ws = (cin, cout, k, k) if c["transposed"] else (cout, cin, k, k)
    d["w"] = (r.standard_normal(ws) / (cin * k * k) ** 0.5).astype(f32)
    # (gelu: pre-activations of about -8 .. 8, which takes in the region below -3 where 1 + erf cancels)
    d["b"] = (r.standard_normal(cout) * (2.5 if c["family"] == "gelu" else 0.3)).astype(f32)
    if c["cout2"]:
        d["w2"] = (r.standard_normal((c["cout2"], cout, 1, 1)) / cout ** 0.5).astype(f32)
        d["b2"] = (r.standard_normal(c["cout2"]) * 0.3).astype(f32)
    if c["cout3"]:
        d["w3"] = (r.standard_normal((c["cout3"], c["cout2"], 1, 1)) / c["cout2"] ** 0.5).astype(f32)
        d["b3"] = (r.standard_normal(c["cout3"]) * 0.3).astype(f32)
    if c["res1"]:
        d["res1"] = r.standard_normal((n, cy, oh, ow)).astype(f32)
    if c["mul"]:
        d["mul"] = (0.02 + 0.96 * r.random_sample((n, cy, oh, ow))).astype(f32)
    if c["res2"]:
        d["res2"] = r.standard_normal((n, cy, oh, ow)).astype(f32)
    return d


def x_slice(c, d):
    return np.ascontiguousarray(d["x"][:, c["x_off"]:c["x_off"] + c["cin"]])


# ================================================================================================ torch references
def _act_t(v, act):
    # (F.gelu with the default approximate="none": the erf form, what the reference's nn.GELU() is -- models/stf.py:16,509-527)
    return [lambda t: t, torch.relu, lambda t: F.leaky_relu(t, 0.01), torch.sigmoid, F.gelu][act](v)


def _conv_t(c, x, w, b):
    if c["transposed"]:
        return F.conv_transpose2d(x, w, b, stride=c["stride"], padding=c["pad"], output_padding=c["stride"] - 1)
    return F.conv2d(x, w, b, stride=c["stride"], padding=c["pad"])


def torch_compose(c, d, dtype):
    """The case in torch CPU arithmetic of `dtype` on the fp32 inputs: {"t", "v" (before act), "y0" (before mul / res2), "y", "u"}."""
    T = lambda a: torch.from_numpy(a).to(dtype)
    o = {}
    v = _conv_t(c, T(x_slice(c, d)), T(d["w"]), T(d["b"]))
    if c["cout2"]:
        o["t"] = _act_t(v, c["act_mid"])
        v = F.conv2d(o["t"], T(d["w2"]), T(d["b2"]))
    if c["res1"]:
        v = v + T(d["res1"])
    o["v"] = v  # (the pre-activation of the last layer)
    o["y0"] = o["y"] = _act_t(v, c["act"])
    if c["mul"]:
        o["y"] = o["y"] * T(d["mul"])
    if c["res2"]:
        o["y"] = o["y"] + T(d["res2"])
    if c["cout3"]:
        o["u"] = torch.relu(F.conv2d(o["y"], T(d["w3"]), T(d["b3"])))
    return o


def _layer_bound(t):
    return 2e-5 * (t.abs().max().item() + 1e-3)


def _opnorm(w):
    return float(np.abs(w.astype(np.float64)).reshape(w.shape[0], -1).sum(axis=1).max())


# ================================================================================================ GELU
GELU_SLOPE = 1.129  # sup |gelu'| = Phi(sqrt 2) + sqrt 2 * phi(sqrt 2) = 1.12890 (test_convforms_cases.py computes it)
SQRT1_2 = f32(0.70710678118654752)  # the reducer's constant


def gelu64(v):
    """erf-form GELU of v (any float array) in fp64 -> numpy float64"""
    return F.gelu(torch.from_numpy(np.ascontiguousarray(v, np.float64))).numpy()


def gelu_device_formula(v):
    """0.5f * v * (1.0f + erff(v * 0.70710678f)) as the reducer writes it, in torch-CPU fp32 on fp32 v: every operation one rounding"""
    v = torch.from_numpy(np.ascontiguousarray(v, f32))
    return ((0.5 * v) * (1.0 + torch.erf(v * float(SQRT1_2)))).numpy()


def erf32_ulps(t):
    """error of torch's CPU fp32 erf on the fp32 arguments t, in ulps of the exact result (an ulp of |e| < 1 is at most 2^-24)"""
    t = torch.from_numpy(np.ascontiguousarray(t, f32))
    e64 = torch.erf(t.double())
    ulp = torch.clamp(2.0 ** (torch.floor(torch.log2(e64.abs().clamp_min(2.0 ** -126))) - 23), max=2.0 ** -24)
    return ((torch.erf(t).double() - e64).abs() / ulp).numpy()


def act_bound(v, e_erf=None):
    """B_act(v): what 0.5f * v * (1.0f + erff(v * c)) may differ by from gelu64(v), element by element, for an erff of e_erf ulps.
    In units of 2^-24, on 0.5 * |v|: the roundings of v * c and of c move erf by at most 2 * max(t * erf'(t)) = 0.97 (counted as 1),
    erff itself e_erf, the rounding of 1 + e another 1; 0.5f * v is exact; the last product rounds once (|gelu| * 2^-24, or half
    a subnormal step)."""
    v = np.asarray(v, np.float64)
    return (0.5 * np.abs(v) * ((E_ERF if e_erf is None else e_erf) + 2.0) + np.abs(gelu64(v))) * 2.0 ** -24 + 2.0 ** -149


def _measure_erf():
    """Nobody states an error bound for the device's erff.  Measured instead: torch's CPU fp32 erf against fp64 on the very
    arguments the GELU cases produce (their fp32 pre-activations times the reducer's constant); the device is granted four
    times that, the margin for another libm."""
    worst = 0.0
    for c in CASES:
        if c["act"] == ACT_GELU:
            for g in range(c["groups"]):
                v = torch_compose(c, inputs(c, g), torch.float32)["v"]
                worst = max(worst, float(erf32_ulps((v * float(SQRT1_2)).numpy()).max()))
    return worst


E_ERF_CPU = _measure_erf()
E_ERF = 4.0 * E_ERF_CPU


def reference64(c, d):
    """fp64 reference and the derived bounds: {"y", "u" (lead), "bound_y", "bound_u"} (numpy float64 arrays / floats)."""
    o = torch_compose(c, d, torch.float64)
    if c["act"] == ACT_GELU:  # the conv rule on the pre-activation, carried through gelu, + the activation's own arithmetic
        assert not (c["cout2"] or c["mul"] or c["res2"])
        by = GELU_SLOPE * _layer_bound(o["v"]) + float(act_bound(o["v"].numpy()).max())
        return {"y": o["y"].numpy(), "bound_y": by}
    by = _layer_bound(o["y0"])
    if c["cout2"]:
        by += _layer_bound(o["t"]) * _opnorm(d["w2"])
    if c["res2"]:
        by += 2.0 ** -23 * o["y"].abs().max().item()
    r = {"y": o["y"].numpy(), "bound_y": by}
    if c["cout3"]:
        r["u"] = o["u"].numpy()
        r["bound_u"] = _layer_bound(o["u"]) + by * _opnorm(d["w3"])
    return r


def torch32(c, d):
    o = torch_compose(c, d, torch.float32)
    return {k: v.numpy() for k, v in o.items() if k in ("y", "u")}


# ================================================================================================ the reference's CPU arithmetic
def ref_layer1(c):
    """(blocks, bias_mode) of the first layer in the reference's arithmetic: a block per 16 channels and (S_0 + bias) + S_1 + ...
    for k > 1, one reduce block whose chain starts at the bias for a 1x1 layer."""
    return (None, 1) if c["k"] > 1 else ([c["cin"]], 2)


def _act_np(v, act):
    if act == ACT_RELU:
        return np.maximum(v, f32(0))
    if act == ACT_LEAKY:
        return np.where(v > 0, v, v * f32(0.01)).astype(f32)
    assert act == ACT_NONE
    return v


def blocked_reference(c, d):
    """The case as oracle/cpu_arith.c computes it: {"y", "u"} float32, every epilogue step one fp32 rounding."""
    assert c["blocked"] and not c["transposed"]
    blocks, bm = ref_layer1(c)
    v = ca.conv2d(x_slice(c, d), d["w"], d["b"], c["stride"], c["pad"], blocks=blocks or ca.direct_blocks(c["cin"]), bias_mode=bm)
    o = {}
    if c["cout2"]:
        t = _act_np(v, c["act_mid"])
        v = ca.conv2d(t, d["w2"], d["b2"], 1, 0, blocks=[c["cout"]], bias_mode=2)
    if c["res1"]:
        v = (v + d["res1"]).astype(f32)
    v = _act_np(v, c["act"])
    if c["mul"]:
        v = (v * d["mul"]).astype(f32)
    if c["res2"]:
        v = (v + d["res2"]).astype(f32)
    o["y"] = v
    if c["cout3"]:
        o["u"] = np.maximum(ca.conv2d(v, d["w3"], d["b3"], 1, 0, blocks=[c["cout2"]], bias_mode=2), f32(0))
    return o
