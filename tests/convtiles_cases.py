"""Cases and host rules shared by tests/test_convtiles_cases.py (CPU: is the sweep worth running?) and
tests/test_gpu_conv_tiles.py (GPU: every instantiated tile form of the conv dispatch against the baseline tile's bits).

Pure numpy / torch-CPU / oracle code on top of tests/convforms_cases.py (inputs, out_hw, pick_tw, the torch compositions).

The contract under test: tile shape, stage depth and staging mode never change a bit of a result.  The forms
come from the library itself (rgbd_debug_tile_list: the lists csrc/conv_tiles.h gives the dispatch); the cases below are the
smallest shapes at which a form can still go wrong -- every one runs through rgbd_conv_forms_nchw in its plain form with
activation none / ReLU / leaky, the destinations pre-filled with convforms_cases.FILL.

fits(form, case) restates the host rules by which the launchers refuse a form (csrc/conv_mfma.hip launch_conv_main, ring_ok;
csrc/conv_mfma_blk.hip conv_blk_tile_ok, launch_conv_blk; csrc/conv_mfma_body.h launch_cfg: patch registers, ring conditions,
weight slots per stage against the LDS cap, "kc 64 may not split its taps").  The GPU sweep requires the launcher's return code
to EQUAL fits()'s, so a refusal is never a silent skip, and test_convtiles_cases.py shows from fits() alone that the forms the
sweep compares are not a hollow set.

Some things the rules themselves decide for EVERY layer shape (never_fits / single_tap_only: computed from fits() on the most
favourable layer there is, asserted on the CPU; the sweep launches these forms all the same and compares their refusal like any
other return code):
  * never launched at all: kc 64 with TM = 160 (wm, mt = 2, 5) or with 256-pixel tiles (wm, nt = 2, 8 and 1, 4) -- one tap of
    weights needs TM * 16 > 8 * 256 staging slots, a 256-pixel patch without any halo 256 * 16 > 12 * 256 -- and staging mode 3
    (38 KiB cap) on 256-pixel tiles of TM > 48 (two patch images of 16 KiB leave 6 KiB for two weight slabs of TM * 64 B).
    11 single-chain and 8 blocked forms are instantiated that no launch can reach.
  * single-tap layers only: the ring forms; kc 64 with TM > 32; mode 3 on every 256-pixel tile (two images of the smallest patch
    with a halo, 17 x 17 pixels x 64 B, leave 1920 B) and on TM = 160 x 128 pixels.  A staging mode that only runs single-tap
    layers holds one tap per stage like mode 1: it walks the chain the same way, whatever the cap.

One case of the issue's list cannot exist: `blk-deconv`.  rgbd_conv_forms_nchw refuses a stride-2 transposed conv in reference
arithmetic (-22) and so does the engine's planner (plan_refnum leaves those layers single-chain; the reference's arithmetic for
them is the measured recipe of deconv_s2_ref_run, a set of 1x1 GEMMs): no caller reaches a blocked four-phase launch, and the
blocked tables have no key 104.  In its place the blocked family runs the two multi-tap forms the blocked tables do name:
`blk-k5s2` (strided, 25 taps split over stages) and `blk-ckbd1` (keys 111 / 121).  Ring forms need single-tap layers, so each
family has three of those (plain, grouped, and split-K / a second block table).
"""
import collections

import numpy as np
import torch

import convforms_cases as cc

f32 = np.float32
ENOSPC, EINVAL = -28, -22
BASELINE = (2, 2, 2, 16, 0)  # the register-staged tile both families have; what every other form is compared with
LDS_BUDGET = 78 * 1024
U = 2.0 ** -24  # unit roundoff of fp32


# ================================================================================================ the case list
def _build():
    R, L = cc.ACT_RELU, cc.ACT_LEAKY
    cs = []

    def add(cid, fam, *shape, blocks=None, **kw):
        c = cc._case(cid, "plain", *shape, **kw)
        c["tile_family"], c["blocks"] = fam, blocks
        assert c["act"] in (cc.ACT_NONE, R, L) and not (c["res1"] or c["mul"] or c["res2"] or c["y2"] or c["cout2"])
        cs.append(c)

    # ---- single-chain kernels (csrc/conv_mfma.hip)
    add("one-tap", 0, 2, 112, 9, 21, 176, 1, act=R)        # 7 channel stages (a ring of four wraps); 11 cout tiles; 189 pixels
    add("one-tap-split2", 0, 1, 112, 3, 37, 40, 1, splitk=2)  # ranges of 4 and 3 chunks; one row of tiles, couts padded 40 -> 48
    add("one-tap-grouped", 0, 1, 96, 5, 13, 72, 1, act=L, groups=2)  # 6 stages; second operand set
    add("k2", 0, 1, 80, 6, 11, 40, 2, act=R)                # four taps: the only multi-tap layer kc 64 holds in one stage beyond TM = 16
    add("k3", 0, 2, 40, 7, 19, 100, 3, act=L)              # zero pad channels; halo on all four borders; two images
    add("k5", 0, 1, 32, 6, 37, 48, 5, act=R)               # 25 taps: split over stages; the patch registers refuse large kc 64 forms
    add("k5s2", 0, 1, 16, 27, 13, 64, 5, stride=2)         # strided patch (a 14 x 7 grid: 8 x 8 tiles, whose 19 x 19 patch still fits)
    add("deconv", 0, 2, 48, 4, 7, 40, 5, stride=2, pad=2, transposed=1, act=R)  # four phases in blockIdx.z; couts padded 40 -> 48
    add("ckbd1", 0, 1, 32, 5, 18, 64, 3, act=R, ckbd=1)    # half-width grid (GW + 1) / 2
    add("ckbd2", 0, 1, 32, 5, 18, 64, 3, ckbd=2)
    add("splitk3", 0, 1, 112, 6, 10, 32, 3, splitk=3)      # uneven ranges: 7 chunks over 3 partials (3, 3, 1)
    add("grouped", 0, 2, 40, 7, 19, 100, 3, act=L, groups=2)
    # ---- blocked-accumulation kernels (csrc/conv_mfma_blk.hip): refmode; multi-tap layers a block per 16 channels with
    # (S_0 + bias) + S_1 + ..., 1x1 layers their reduce blocks with the first chain starting at the bias (convforms_cases.ref_layer1,
    # but with more than one reduce block: a single block is the single-chain kernel)
    add("blk-one-tap", 1, 2, 112, 9, 21, 176, 1, act=R, blocked=True, blocks=[48, 64])  # (a block ends inside a 64-channel stage)
    add("blk-one-tap-b", 1, 1, 112, 3, 37, 40, 1, blocked=True, blocks=[16, 32, 64])
    add("blk-one-tap-grouped", 1, 1, 96, 5, 13, 72, 1, act=L, blocked=True, blocks=[32, 64], groups=2)
    add("blk-k2", 1, 1, 80, 6, 11, 40, 2, act=R, blocked=True)
    add("blk-k3", 1, 2, 40, 7, 19, 100, 3, act=L, blocked=True)
    add("blk-k5s2", 1, 1, 32, 27, 13, 48, 5, stride=2, act=R, blocked=True)
    add("blk-ckbd1", 1, 1, 32, 5, 18, 64, 3, act=R, blocked=True, ckbd=1)
    assert len({c["id"] for c in cs}) == len(cs)
    for c in cs:
        oh, ow = cc.out_hw(c)
        assert c["h"] * c["w"] <= 400 and oh * ow <= 400, c["id"]
    return cs


CASES = _build()
BY_ID = {c["id"]: c for c in CASES}


def family(blocked):
    return [c for c in CASES if c["tile_family"] == (1 if blocked else 0)]


def parse_forms(text):
    """the text of rgbd_debug_tile_list -> [(wm, mt, nt, kc, dma)]"""
    forms = [tuple(int(v) for v in ln.split(",")) for ln in text.strip().splitlines()]
    assert forms and all(len(f) == 5 for f in forms) and len(set(forms)) == len(forms)
    return forms


def exported_forms(blocked):
    """the forms the library's dispatch can reach (host-only call: no device is touched)"""
    import ctypes

    from rgbd_amd._lib import lib

    L = lib()
    need = L.rgbd_debug_tile_list(blocked, None, 0)
    buf = ctypes.create_string_buffer(need)
    assert L.rgbd_debug_tile_list(blocked, buf, need) == need
    return parse_forms(buf.value.decode())


def triples(forms):
    seen = collections.OrderedDict()
    for f in forms:
        seen.setdefault(f[:3], []).append(f)
    return seen


def form_str(f):
    return ",".join(str(v) for v in f)


# ================================================================================================ the launchers' host rules
def geometry(c):
    """The ConvArgs fields the rules read (csrc/conv_args.h: make_taps, conv_args_geometry)."""
    k, s, pad = c["k"], c["stride"], c["pad"]
    oh, ow = cc.out_hw(c)
    g = dict(cin_pad=cc.round_up(c["cin"], 16), cout_pad=cc.round_up(c["cout"], 16), ckbd=c["ckbd"])
    if not c["transposed"]:
        g.update(nphase=1, IS=s, taps=[k * k], span=k, GH=oh, GW=ow)
    else:
        taps, mn, mx = [], 127, -127
        for ry in range(s):
            for rx in range(s):
                n = 0
                for ky in range(k):
                    if (ry + pad - ky) % s:
                        continue
                    for kx in range(k):
                        if (rx + pad - kx) % s:
                            continue
                        dy, dx = (ry + pad - ky) // s, (rx + pad - kx) // s
                        mn, mx = min(mn, dy, dx), max(mx, dy, dx)
                        n += 1
                taps.append(n)
        g.update(nphase=s * s, IS=1, taps=taps, span=mx - mn + 1, GH=c["h"], GW=c["w"])
    g["max_taps"] = max(g["taps"])
    g["splitk"] = max(1, min(c["splitk"], g["cin_pad"] // 16))
    g["ring_ok"] = g["max_taps"] == 1 and g["nphase"] == 1 and g["IS"] == 1 and not c["ckbd"] and g["span"] == 1
    return g


def conv_blk_tile_ok(wm, mt, nt, max_tiles=16):
    if mt * nt > 16 or mt * nt > max_tiles:
        return False
    if wm == 2:
        return (nt == 8 and mt <= 2) or (nt == 4 and mt <= 4) or (nt in (2, 1) and mt <= 5)
    return wm == 1 and mt <= 3 and nt in (4, 2, 1)


Fit = collections.namedtuple("Fit", "rc tps stages TM TP TH TW tiles_x tiles_y")


def fits(form, c, forms_of_family=None):
    """What the launcher returns for `form` forced on case c (0 / -28 / -22), the taps per stage and the number of stages of the
    longest reduction a workgroup runs, and the tile.  forms_of_family: the exported list (a ring form that is not instantiated is
    refused with -28); None = every ring form with whole waves of patch slots exists."""
    wm, mt, nt, kc, dm = form
    g = geometry(c)
    wn = 2 if wm == 2 else 4
    TM, TP = 16 * mt * wm, 16 * nt * wn
    KC = 64 if kc == 64 else 16
    dma = dm != 0 and kc == 16                                    # set_mode
    cap = {2: 52 * 1024, 3: 38 * 1024}.get(dm, 0)
    ring = {4: 4, 5: 3}.get(dm, 0) if kc == 16 else 0
    TW = cc.pick_tw((g["GW"] + 1) // 2 if g["ckbd"] else g["GW"], g["GH"], TP)
    TH = TP // TW
    TWx = 2 * TW if g["ckbd"] else TW
    tiles_x, tiles_y = -(-g["GW"] // TWx), -(-g["GH"] // TH)

    def out(rc, tps=0, stages=0):
        return Fit(rc, tps, stages, TM, TP, TH, TW, tiles_x, tiles_y)

    if ring and not g["ring_ok"]:                                 # launch_conv_main
        return out(ENOSPC)
    if c["blocked"]:                                              # launch_conv_blk
        if not conv_blk_tile_ok(wm, mt, nt) or g["splitk"] > 1:
            return out(EINVAL)
    if forms_of_family is not None and tuple(form) not in set(forms_of_family):  # (the end of the dispatch chains)
        return out(ENOSPC if ring else EINVAL)
    if ring:
        KC, dma, NB, budget = 16, True, ring, 160 * 1024
    else:
        NB, budget = 2, cap or LDS_BUDGET
    # launch_cfg
    RS = KC + 4 if KC > 16 else KC
    PH, PW = (TH - 1) * g["IS"] + g["span"], (TWx - 1) * g["IS"] + g["span"]
    patch_bytes, tap_bytes = PH * PW * RS * 4, TM * RS * 4
    PR = 12 if TP >= 128 else (6 if TP >= 64 else 4)
    if PH * PW * (KC // 4) > PR * 256:                            # patch registers
        return out(ENOSPC)
    if NB > 2 and (not g["ring_ok"] or TP % 64):
        return out(ENOSPC)
    room = (8 * 256) // (TM * (KC // 4))                          # weight slots per stage
    if dma and NB == 2:
        lds_room = (budget - 2 * patch_bytes) // (2 * tap_bytes) if budget >= 2 * patch_bytes else -1
        room = min(room, lds_room)
    if room < 1:
        return out(ENOSPC)
    tps = min(room, g["max_taps"])
    if KC > 16 and tps < g["max_taps"]:                           # would break the canonical accumulation order
        return out(ENOSPC)
    n16 = g["cin_pad"] // 16
    per = -(-n16 // g["splitk"])
    longest = max(min(n16, s * per + per) - s * per for s in range(g["splitk"]))
    stages = -(-longest * 16 // KC) * -(-g["max_taps"] // tps)
    return out(0, tps, stages)


PROBE_MAPS = ((4, 4), (8, 8), (16, 16), (8, 32), (32, 8), (4, 64), (64, 4), (2, 128), (1, 256))


def feasible(form, c, forms_of_family=None):
    """Can `form` run the KIND of layer case c is (kernel size, stride, transposed, checkerboard, blocked, split) on any map at
    all?  fits() on the case's own map and on PROBE_MAPS (every tile shape pick_tw can choose for a 32- to 256-pixel tile: a form
    that none of them lets through is refused by the rules for this kind of layer, not by the case's size)."""
    if fits(form, c, forms_of_family).rc == 0:
        return True
    for h, w in PROBE_MAPS:
        s = 1 if c["transposed"] else c["stride"]
        if fits(form, dict(c, h=h * s, w=w * s), forms_of_family).rc == 0:
            return True
    return False


_ONE_TAP = cc._case("probe-one-tap", "plain", 1, 16, 16, 16, 16, 1)
_FOUR_TAPS = cc._case("probe-k2", "plain", 1, 16, 16, 16, 16, 2)


def never_fits(form):
    """Forms the rules refuse for every layer: not even a 1x1 stride-1 layer (one tap, no halo: every rule of launch_cfg is
    monotone in the patch size and the tap count) gets through.  See the module docstring for which and why."""
    return not feasible(form, _ONE_TAP)


def single_tap_only(form):
    """Forms the rules refuse for every multi-tap layer: the smallest one a caller can issue has four taps and a one-pixel halo
    (k = 2; the longest phase of a k = 3 stride-2 transposed conv is the same).  A ring form by definition; kc 64 with TM > 32
    (four taps of weights in one stage: 4 * TM * 16 > 8 * 256 slots); the tight LDS caps on the large tiles."""
    return form[3] == 16 and form[4] in (4, 5) or not feasible(form, _FOUR_TAPS)


# ================================================================================================ references and checks
def blocks_of(c):
    """(blocks, bias_mode) of a blocked case, as the hook takes them"""
    assert c["blocked"]
    return (None, 1) if c["k"] > 1 else (c["blocks"], 2)


def blocked_reference(c, d):
    """oracle/cpu_arith.c's chain for a blocked case (as convforms_cases.blocked_reference, with the case's own block table)"""
    from oracle import cpu_arith as ca

    blocks, bm = blocks_of(c)
    v = ca.conv2d(cc.x_slice(c, d), d["w"], d["b"], c["stride"], c["pad"], blocks=blocks or ca.direct_blocks(c["cin"]), bias_mode=bm)
    return cc._act_np(v, c["act"])


def computed_mask(c):
    oh, ow = cc.out_hw(c)
    yy, xx = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    if not c["ckbd"]:
        return np.ones((oh, ow), bool)
    return (yy + xx) % 2 == (1 if c["ckbd"] == 1 else 0)


def bound(c, d):
    """(ref, bnd): the fp64 result and the per-element bound of the single-chain / blocked fp32 result against it.
    (K + 3) * 2^-24 * (sum |w x| + |b|) with K = cin_pad * taps the chain length -- an fp32 fma chain of K terms is off by at most
    about K * 2^-24 of the sum of its terms' magnitudes; + 3 for the bias add and the epilogue -- taken before the activation
    (1-Lipschitz for none / ReLU / leaky), + 2^-24 |ref| for the final rounding, + S * 2^-24 |ref| for the S partial sums of a
    split-K launch.  Derived from the arithmetic, not measured."""
    assert c["act"] in (cc.ACT_NONE, cc.ACT_RELU, cc.ACT_LEAKY)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)
    x, w, b = cc.x_slice(c, d), d["w"], d["b"]
    pre = cc._conv_t(c, T(x), T(w), T(b)).numpy()
    mag = cc._conv_t(c, T(np.abs(x)), T(np.abs(w)), T(np.abs(b))).numpy()
    g = geometry(c)
    K = g["cin_pad"] * g["max_taps"]
    bnd = (K + 3) * U * mag + U * np.abs(pre)
    if g["splitk"] > 1:
        bnd = bnd + g["splitk"] * U * np.abs(pre)
    ref = cc.torch_compose(c, d, torch.float64)["y"].numpy()
    return ref, bnd


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def check(got, base, c):
    """Every destination tensor of every operand set ([{"y": wide NCHW array}, ...]), over its whole extent including what the
    launch left at FILL, equals the baseline bit for bit; else an AssertionError naming the first differing (n, c, y, x)."""
    assert len(got) == len(base) == c["groups"], (c["id"], len(got), len(base))
    for g, (a, b) in enumerate(zip(got, base)):
        assert set(a) == set(b), (c["id"], sorted(a), sorted(b))
        for key in sorted(b):
            ga, gb = _bits(a[key]), _bits(b[key])
            assert ga.shape == gb.shape, (c["id"], key, ga.shape, gb.shape)
            if not np.array_equal(ga, gb):
                bad = np.argwhere(ga != gb)
                i = tuple(int(v) for v in bad[0])
                raise AssertionError(f"{c['id']} set {g} {key}: {len(bad)} of {ga.size} elements differ from the baseline tile; first at "
                                     f"(n, c, y, x) = {i}: got {a[key][i]!r} (0x{int(ga[i]):08x}), baseline {b[key][i]!r} (0x{int(gb[i]):08x})")
