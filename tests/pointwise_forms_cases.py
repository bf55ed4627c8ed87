"""The single-chain pointwise kernels and the two layout kernels of csrc/pointwise.hip: the cases, inputs, references and
acceptance functions -- shared by the CPU test of this file's own logic (test_pointwise_forms_cases.py) and the GPU test of
the kernels through the rgbd_pw_* hooks (test_gpu_pointwise_forms.py).  numpy only; importable without a GPU.

Tensors are the engine's: NHWC float32, [N][pixels][channel stride].  Pad channels that no kernel may read hold NaN (a read
poisons the result); destinations are pre-filled with SENTINEL, so what a launch did not write is visible.

Two kinds of acceptance:
  exact      the kernel moves or combines floats without freedom (layout, copies, gathers, max, x * s, the documented summation
             order of the channel mean): every element must carry the reference's value.
  tolerance  float64 statement + a bound DERIVED below from the kernel's operations (never from what the kernel returns):
             u = 2^-24 is the unit roundoff of float32, gamma(n) = n u / (1 - n u) bounds the relative error of n roundings
             (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).
"""
import numpy as np

U = 2.0 ** -24
SENTINEL = 12345.0
F32 = np.float32


def gamma(n):
    return n * U / (1.0 - n * U)


def cperm(c):
    """Position of channel c inside its group of 16 in the engines that permute (include/rgbd_amd.h, the entropy hooks' header
    comment): (c & ~15) | (c & 3) << 2 | (c >> 2) & 3 -- a 4x4 transpose, its own inverse."""
    c = np.asarray(c)
    return (c & ~15) | ((c & 3) << 2) | ((c >> 2) & 3)


def rng(*key):
    return np.random.default_rng([int(k) for k in key])


def exact(got, want):
    """(ok, number of elements whose value differs); NaN never matches."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False, max(got.size, want.size)
    bad = int((~(got == want)).sum())
    return bad == 0, bad


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def share(got, ref, bound):
    """max |got - ref| / bound over the elements (inf on NaN or a zero bound with an error): <= 1 is a pass."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(err == 0, 0.0, err / bound)
    s = np.where(np.isfinite(s), s, np.inf)
    return float(s.max())


# ---------------------------------------------------------------------------------------------------------------------------
# Channel means (channel_mean_kernel through launch_channel_mean_strided)
# ---------------------------------------------------------------------------------------------------------------------------
# both sides of the unrolled loop's entry condition p + 28 < HW for every chain r = p mod 4 (HW = 29 ... 32 enter it for chains
# 0 ... 3 in turn; 63 ... 65 enter it twice or not), of its remainder loop, and of the 4 chains (HW < 4 leaves chains empty)
MEAN_HW = [1, 3, 4, 5, 28, 29, 31, 32, 33, 63, 64, 65, 259]
MEAN_C = [16, 48, 80, 192]   # less than one block of 64 channels, one block and a part, three blocks
MEAN_N = [1, 3]
MEAN_MISTAKES = ["drop_last", "div_hw1", "swap_chains", "mstride_as_c"]


def mean_cs(C):
    return C + 16 if C % 64 else C + 4  # cs >= C with pads


def mean_mstrides(C):
    return [C, C + 48]


def mean_input(N, HW, C, cs, pad=np.nan):
    """Uniform in [0.5, 1.5]: away from zero mean, so a dropped or doubled pixel moves the result by about 1 / HW of it."""
    x = np.full((N, HW, cs), pad, F32)
    x[..., :C] = rng(1, N, HW, C).uniform(0.5, 1.5, (N, HW, C)).astype(F32)
    return x


def mean_f64(x, C):
    return x[..., :C].astype(np.float64).mean(axis=1)


def mean_f32_order(x, C, mut=None):
    """The documented order in float32 (no fused operations anywhere, so numpy's float32 adds are the kernel's): chain r adds
    pixels r, r + 4, ... one after the other starting from 0; total = (c0 + c1) + (c2 + c3); divided by float(HW)."""
    N, HW, _ = x.shape
    npix = HW - 1 if mut == "drop_last" else HW
    ch = []
    for r in range(4):
        s = np.zeros((N, C), F32)
        for p in range(r, npix, 4):
            s = s + x[:, p, :C]
        ch.append(s)
    if mut == "swap_chains":
        ch[1], ch[2] = ch[2], ch[1]
    tot = (ch[0] + ch[1]) + (ch[2] + ch[3])
    return (tot / F32(HW + 1 if mut == "div_hw1" else HW)).astype(F32)


def mean_place(vals, mstride, mut=None):
    """The mean buffer [N * mstride] a launch leaves behind over a SENTINEL pre-fill: mean[n * mstride + c]."""
    N, C = vals.shape
    buf = np.full(N * mstride, SENTINEL, F32)
    st = C if mut == "mstride_as_c" else mstride
    for n in range(N):
        buf[n * st:n * st + C] = vals[n]
    return buf


def mean_bound(x, C):
    """|mean - f64| <= gamma(n) * sum|x| / HW, n = ceil(HW / 4) + 3: a chain performs ceil(HW / 4) adds at most (the first onto
    an exact 0), the two levels of (c0 + c1) + (c2 + c3) add 2, the division 1."""
    HW = x.shape[1]
    return gamma(-(-HW // 4) + 3) * np.abs(x[..., :C].astype(np.float64)).sum(axis=1) / HW


def accept_mean(buf, x, C, mstride):
    """buf: the whole mean buffer.  -> (ok, share of the float64 bound used, elements that differ from the float32 restatement
    or, outside the written floats, from the pre-fill)."""
    N = x.shape[0]
    want = mean_place(mean_f32_order(x, C), mstride)
    ok_bits, bad = exact(buf, want)
    got = np.asarray(buf).reshape(N, mstride)[:, :C]
    sh = share(got, mean_f64(x, C), mean_bound(x, C))
    return ok_bits and sh <= 1.0, sh, bad


# ---------------------------------------------------------------------------------------------------------------------------
# SE gate (se_hidden_kernel / se_gate_kernel through launch_se_fc)
# ---------------------------------------------------------------------------------------------------------------------------
SE_CASES = [(16, 1, 16), (48, 2, 64), (192, 1, 192), (1280, 2, 1280), (2432, 1, 2432 + 16)]  # C, N, mstride
SE_MISTAKES = ["perm_ignored", "no_relu", "w1_not_transposed", "mstride_as_c"]


def se_input(C, N, mstride, perm, pad=np.nan):
    """-> mean buffer [N][mstride] (by position when perm), w0 [C/16][C], w1 [C][C/16], the logical means [N][C].  The weights
    are scaled so that the hidden pre-activations have unit spread around 0 and the gate's argument a spread of 2 (gates from
    about 0.05 to 0.95); se_check_spread asserts what came out."""
    g = rng(2, C, N, mstride)
    hid = C // 16
    m = g.uniform(0.0, 1.0, (N, C)).astype(F32)
    w0 = (g.standard_normal((hid, C)) * np.sqrt(3.0 / C)).astype(F32)
    if hid == 1:
        w0[0] = np.abs(w0[0])  # (the only unit is alive: otherwise every gate would be 0.5)
    h = np.maximum(m.astype(np.float64) @ w0.astype(np.float64).T, 0.0)
    w1 = (g.standard_normal((C, hid)) * 2.0 / np.sqrt((h[0] ** 2).sum())).astype(F32)
    buf = np.full((N, mstride), pad, F32)
    buf[:, cperm(np.arange(C)) if perm else np.arange(C)] = m
    return buf, w0, w1, m


def se_f64(m, w0, w1, mut=None):
    """sigmoid(W1 . relu(W0 . mean)) in float64, logical channel order: -> gates [N][C], hidden pre-activations, hidden."""
    m, w0, w1 = (np.asarray(a, np.float64) for a in (m, w0, w1))
    pre = m @ w0.T
    h = pre if mut == "no_relu" else np.maximum(pre, 0.0)
    if mut == "w1_not_transposed":  # the gate kernel reads [hidden][C]: fc.2.weight's memory taken for that without the transpose
        w1 = w1.reshape(w1.shape[1], w1.shape[0]).T
    return 1.0 / (1.0 + np.exp(-(h @ w1.T))), pre, h


def se_gate_vec(buf, C, w0, w1, perm, mut=None, dtype=np.float64):
    """The gate vector [N][C] as the kernels leave it (by position when perm) from the mean buffer [N][mstride]."""
    N, mstride = buf.shape
    pm = perm and mut != "perm_ignored"
    pos = cperm(np.arange(C)) if pm else np.arange(C)
    src = buf.reshape(-1)[:N * C].reshape(N, C) if mut == "mstride_as_c" else buf
    m = src[:, pos]
    if dtype == np.float64:
        gates = se_f64(m, w0, w1, mut)[0]
    else:  # a plain float32 evaluation
        h = np.maximum(m.astype(F32) @ w0.T, F32(0))
        gates = (F32(1) / (F32(1) + np.exp(-(h @ w1.T), dtype=F32))).astype(F32)
    out = np.empty((N, C), gates.dtype)
    out[:, pos] = gates
    return out


def se_logical(vec, perm):
    """A gate / mean vector [N][C] by position -> logical channel order."""
    C = vec.shape[1]
    return vec[:, cperm(np.arange(C))] if perm else vec


def se_bound(m, w0, w1):
    """Bound of |gate - f64| per (image, channel), logical order.

    e1_j (hidden unit j): lane l forms an fma chain over its ceil(C / 64) channels l, l + 64, ... (one rounding per term), the
      shuffle tree adds the 64 lanes in 6 levels; a product meets at most ceil(C / 64) + 6 roundings, taken as ceil(C / 64) + 7:
      e1_j = gamma(ceil(C / 64) + 7) * sum_c |w0[j][c]| |mean[c]|.  relu is 1-Lipschitz and exact: the hidden value is off by e1_j.
    e2_c (gate argument): one fma chain over the C / 16 computed hidden values, gamma(C / 16) * sum_j |w1[c][j]| (|h_j| + e1_j),
      plus the inherited sum_j |w1[c][j]| e1_j.
    The sigmoid's slope is at most 1 / 4: the argument's error reaches the gate as e2_c / 4.
    Evaluating 1 / (1 + exp(-s)): the exponential within 2 ulp (both the runtime's expf and the reference-arithmetic form are
      1-ulp functions), i.e. a relative 4 u, which reaches the gate damped by e / (1 + e) < 1; the add and the division one
      rounding each: 6 u relative, taken as 4 ulp = 8 u times the gate."""
    m, w0, w1 = (np.asarray(a, np.float64) for a in (m, w0, w1))
    C = m.shape[1]
    gates, _, h = se_f64(m, w0, w1)
    e1 = gamma(-(-C // 64) + 7) * (np.abs(m) @ np.abs(w0).T)
    e2 = gamma(C // 16) * ((np.abs(h) + e1) @ np.abs(w1).T) + e1 @ np.abs(w1).T
    return e2 / 4.0 + 8.0 * U * gates


def se_check_spread(C, N, m, w0, w1):
    gates, pre, _ = se_f64(m, w0, w1)
    if pre.size > 1:
        assert pre.min() < 0.0 < pre.max(), (C, N, pre)       # hidden units on both sides of 0
    else:
        assert pre.min() > 0.1, (C, N, pre)                   # (a single unit: alive, or every gate would be 0.5)
    assert gates.min() < 0.2 and gates.max() > 0.8, (C, N, gates.min(), gates.max())
    assert gates.min() > 1e-5 and gates.max() < 1 - 1e-5


def accept_se(vec, m, w0, w1, perm):
    """vec: the gate vector by position.  -> (ok, share of the bound used)."""
    sh = share(se_logical(np.asarray(vec), perm), se_f64(m, w0, w1)[0], se_bound(m, w0, w1))
    return sh <= 1.0, sh


# ---------------------------------------------------------------------------------------------------------------------------
# Bilinear, single-chain form (bilinear_kernel with ref == 0)
# ---------------------------------------------------------------------------------------------------------------------------
# one source pixel; identity; up both ways; non-integer ratios; down; one row; one column
BILINEAR_SHAPES = [(1, 1, 8, 8), (5, 7, 5, 7), (9, 14, 64, 96), (19, 25, 40, 33), (12, 10, 5, 7), (1, 9, 4, 30), (7, 1, 20, 3)]
BILINEAR_C = [(16, 20), (48, 52)]  # (C, cs): the kernel interpolates all cs positions, 4 floats per lane
BILINEAR_N = [1, 2]
BILINEAR_MISTAKES = ["align_corners", "clamp_in_2"]
BILINEAR_SENSITIVITY = [(9, 14, 64, 96), (19, 25, 40, 33)]


def bilinear_input(N, h, w, cs, key=0):
    return rng(3, N, h, w, cs, key).uniform(-1.0, 1.0, (N, h, w, cs)).astype(F32)


def _axis(n_in, n_out, dtype, mut):
    o = np.arange(n_out).astype(dtype)
    if mut == "align_corners":
        s = o * (dtype(n_in - 1) / dtype(max(n_out - 1, 1)))
    else:
        s = np.maximum((dtype(n_in) / dtype(n_out)) * (o + dtype(0.5)) - dtype(0.5), dtype(0))
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, max(n_in - 2 if mut == "clamp_in_2" else n_in - 1, 0))
    l1 = (s - i0.astype(dtype)).astype(dtype)
    return i0, i1, (dtype(1) - l1).astype(dtype), l1


def bilinear(x, H, W, dtype=np.float64, mut=None):
    """The formula of the kernel's header comment: src = max(0, scale * (dst + 0.5) - 0.5), scale = in / out, i0 = floor(src),
    i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1; out = ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11)."""
    N, h, w, cs = x.shape
    y0, y1, ly0, ly1 = _axis(h, H, dtype, mut)
    x0, x1, lx0, lx1 = _axis(w, W, dtype, mut)
    v = x.astype(dtype)
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]
    top = lx0 * v[:, y0][:, :, x0] + lx1 * v[:, y0][:, :, x1]
    bot = lx0 * v[:, y1][:, :, x0] + lx1 * v[:, y1][:, :, x1]
    return (ly0[None, :, None, None] * top + ly1[None, :, None, None] * bot).astype(dtype)


def bilinear_bound(x):
    """Bound of |out - f64| for the whole tensor, from the operations:

    roundings  with the float32 weights taken as given, a tap's product meets l0 = 1 - l1 (1; l1 = src - i0 is exact), its
      multiply (1), the add (1), the row weight's rounding (1), multiply (1) and add (1): 6, taken as 9 to cover the second-order
      terms and weights that sum to 1 + 2 u.  The weights are convex, so the sum of |w v| is at most max|x|: gamma(9) max|x|.
    index      src is scale (1 rounding) * (dst + 0.5) (exact; 1 rounding) - 0.5 (1 rounding): off by at most gamma(3) * in
      from the real src (every intermediate is below in).  The interpolant is continuous and piecewise linear in src, with
      slope at most the largest difference of neighbouring pixels along that axis (a convex combination of such differences
      along the other axis): gamma(3) * (h * Dy + w * Dx)."""
    v = x.astype(np.float64)
    _, h, w, _ = v.shape
    dy = np.abs(np.diff(v, axis=1)).max() if h > 1 else 0.0
    dx = np.abs(np.diff(v, axis=2)).max() if w > 1 else 0.0
    return gamma(9) * np.abs(v).max() + gamma(3) * (h * dy + w * dx)


def accept_bilinear(got, x):
    got = np.asarray(got)
    sh = share(got, bilinear(x, got.shape[1], got.shape[2]), bilinear_bound(x))
    return sh <= 1.0, sh


# ---------------------------------------------------------------------------------------------------------------------------
# Pair launches (blockIdx.y == 1 of bilinear_kernel / maxpool7s3_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
PAIR_SHAPES = [(1, 7, 7, 16, 16), (2, 10, 22, 48, 64)]  # N, H, W, C, cs


def pair_out_hw(H, W):
    """Output size of the pair tests' bilinear launch (up along one axis, non-integer ratio along the other)."""
    return 2 * H + 1, W + 5


def maxpool7s3(x):
    """F.max_pool2d(kernel 7, stride 3), no padding, floor mode, over all channel positions of [N][H][W][cs]."""
    N, H, W, cs = x.shape
    OH, OW = (H - 7) // 3 + 1, (W - 7) // 3 + 1
    out = np.full((N, OH, OW, cs), -np.inf, x.dtype)
    for ky in range(7):
        for kx in range(7):
            out = np.maximum(out, x[:, ky:ky + 3 * (OH - 1) + 1:3, kx:kx + 3 * (OW - 1) + 1:3])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Strided channel scale (channel_scale_to_kernel through launch_channel_scale_to_strided)
# ---------------------------------------------------------------------------------------------------------------------------
# the se_cat_to form: two sources into the two halves of a wider destination under one gate vector per image
CAT = dict(N=2, own_c=48, own_cs=64, other_c=32, other_cs=32, dst_cs=96, sstride=80)
CAT_HW = [1, 35]
SCALE_PLAIN = dict(N=2, HW=7, C=20, xcs=24, ycs=32)  # sstride == C, C a multiple of 4 but not of 16
SCALE_MISTAKES = ["gate_offset_ignored", "mode0_for_mode1"]


def scale_ref(x, C, s, mode):
    """float32, as the kernel: t = x * s (one rounding), mode 1: x + t (a second rounding; never fused)."""
    t = (x[..., :C] * s[:, None, :C]).astype(F32)
    return (x[..., :C] + t).astype(F32) if mode else t


def cat_input(HW):
    g = rng(4, HW)
    own = np.full((CAT["N"], HW, CAT["own_cs"]), np.nan, F32)
    own[..., :CAT["own_c"]] = g.standard_normal((CAT["N"], HW, CAT["own_c"]))
    other = g.standard_normal((CAT["N"], HW, CAT["other_cs"])).astype(F32)
    gate = g.uniform(0.05, 0.95, (CAT["N"], CAT["sstride"])).astype(F32)
    return own, other, gate


def cat_ref(own, other, gate, mode, mut=None):
    """The destination [N][HW][96] after both launches over a SENTINEL pre-fill: channels 0..47 = own under gate[0..48),
    48..79 = other under gate[48..80), 80..95 untouched."""
    if mut == "mode0_for_mode1":
        mode = 0
    oc, tc = CAT["own_c"], CAT["other_c"]
    dst = np.full((own.shape[0], own.shape[1], CAT["dst_cs"]), SENTINEL, F32)
    dst[..., :oc] = scale_ref(own, oc, gate, mode)
    dst[..., oc:oc + tc] = scale_ref(other, tc, gate if mut == "gate_offset_ignored" else gate[:, oc:], mode)
    return dst


def plain_scale_input():
    p = SCALE_PLAIN
    g = rng(5)
    x = np.full((p["N"], p["HW"], p["xcs"]), np.nan, F32)
    x[..., :p["C"]] = g.standard_normal((p["N"], p["HW"], p["C"]))
    return x, g.uniform(0.05, 0.95, (p["N"], p["C"])).astype(F32)


def plain_scale_ref(x, gate, mode):
    p = SCALE_PLAIN
    dst = np.full((p["N"], p["HW"], p["ycs"]), SENTINEL, F32)
    dst[..., :p["C"]] = scale_ref(x, p["C"], gate, mode)
    return dst


# ---------------------------------------------------------------------------------------------------------------------------
# copy_channels, fill_zero
# ---------------------------------------------------------------------------------------------------------------------------
COPY_CASES = [(1, 4, 4, 8), (37, 48, 64, 208), (1000, 20, 32, 24)]  # npix, C, scs, dcs
FILL_N = [1, 3, 4, 5, 1025]


def copy_input(npix, C, scs):
    src = np.full((npix, scs), np.nan, F32)
    src[:, :C] = rng(6, npix, C).standard_normal((npix, C))
    return src


def copy_ref(src, C, dcs):
    dst = np.full((src.shape[0], dcs), SENTINEL, F32)
    dst[:, :C] = src[:, :C]
    return dst


# ---------------------------------------------------------------------------------------------------------------------------
# im2col5s2 (the packed first layer)
# ---------------------------------------------------------------------------------------------------------------------------
IM2COL_CKP = [(1, 32), (1, 80), (3, 80)]  # (C, KP) with 25 C <= KP; (3, 32) is a refusal
IM2COL_CS = 16
IM2COL_N = [1, 2]
IM2COL_HW = [(1, 1), (2, 3), (5, 4), (9, 14), (16, 16)]  # odd and tiny maps: every tap class meets the border
IM2COL_REFUSALS = [dict(C=3, KP=32), dict(C=1, KP=40), dict(C=20, KP=512)]  # 25 C > KP, KP % 16, C > cs
IM2COL_MISTAKES = ["kx_major", "pad_not_zeroed"]


def im2col_input(N, H, W, C):
    x = np.full((N, H, W, IM2COL_CS), np.nan, F32)
    x[..., :C] = rng(7, N, H, W, C).uniform(0.25, 1.0, (N, H, W, C))  # (non-zero: a zero of the padding is told from a pixel)
    return x


def im2col_index(term):
    """Packed index of term = tap * C + c: term = j * 16 + e * 4 + q sits at j * 16 + q * 4 + e."""
    j, e, q = term // 16, (term % 16) // 4, term % 4
    return j * 16 + q * 4 + e


def im2col5s2(x, C, KP, mut=None, dtype=F32):
    """From the comment above im2col5s2_kernel: y[n][oy][ox][packed(tap * C + c)] = x[n][2 oy - 2 + ky][2 ox - 2 + kx][c],
    tap = ky * 5 + kx; 0 outside the image and in the terms 25 C .. KP - 1."""
    N, H, W, _ = x.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    y = np.full((N, OH, OW, KP), SENTINEL if mut == "pad_not_zeroed" else 0.0, dtype)
    for t in range(25):
        ky, kx = (t % 5, t // 5) if mut == "kx_major" else (t // 5, t % 5)
        for oy in range(OH):
            iy = 2 * oy - 2 + ky
            for ox in range(OW):
                ix = 2 * ox - 2 + kx
                inside = 0 <= iy < H and 0 <= ix < W
                for c in range(C):
                    y[:, oy, ox, im2col_index(t * C + c)] = x[:, iy, ix, c] if inside else 0.0
    return y


def im2col_pack_weights(wt, KP):
    """Conv2d weight [O][C][5][5] -> [O][KP] in the packed order of the gathered row."""
    O, C = wt.shape[:2]
    out = np.zeros((O, KP), wt.dtype)
    for t in range(25):
        for c in range(C):
            out[:, im2col_index(t * C + c)] = wt[:, c, t // 5, t % 5]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Layout kernels (nchw_to_nhwc16_kernel / nhwc_to_nchw_kernel)
# ---------------------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = [(1, 1, 1, 1, 16), (2, 3, 5, 7, 16), (1, 20, 3, 4, 32), (3, 48, 2, 9, 64), (1, 320, 4, 4, 320)]  # N, C, H, W, cs
LAYOUT_MISTAKES = ["perm_ignored", "pad_not_zeroed"]


def layout_nchw_input(N, C, H, W):
    return rng(8, N, C, H, W).uniform(0.25, 1.0, (N, C, H, W)).astype(F32)  # (non-zero: a zeroed pad is told from a channel)


def layout_nhwc_input(N, C, H, W, cs, perm, clamp01):
    """NHWC source of nhwc_to_nchw: NaN at the positions that hold no channel.  With clamp01 values below 0, above 1, exactly
    0 and 1, and -0.0 (no NaN in the channels: fminf / fmaxf and torch's clamp differ there, and the models never produce it)."""
    g = rng(9, N, C, H, W, cs)
    x = np.full((N, H, W, cs), np.nan, F32)
    v = g.uniform(-0.5, 1.5, (N, H, W, C)).astype(F32)
    if clamp01:
        flat = v.reshape(-1)
        for k, val in enumerate((0.0, 1.0, -0.0, -0.25, 1.25)):
            flat[k::7] = val
    x[..., cperm(np.arange(C)) if perm else np.arange(C)] = v
    return x


def to_nhwc(src, cs, perm, mut=None):
    """[N][C][H][W] -> [N][H][W][cs] over a SENTINEL pre-fill: position p holds channel p (perm 0) or the channel whose
    permuted position is p (perm 1: cperm is its own inverse); 0 where that channel is >= C."""
    N, C, H, W = src.shape
    dst = np.full((N, H, W, cs), SENTINEL if mut == "pad_not_zeroed" else 0.0, F32)
    for p in range(cs):
        c = int(cperm(p)) if perm and mut != "perm_ignored" else p
        if c < C:
            dst[..., p] = src[:, c]
    return dst


def to_nchw(src, C, perm, clamp01, mut=None):
    """[N][H][W][cs] -> [N][C][H][W]: channel c from position cperm(c) (perm 1) or c; clamp01: min(max(v, 0), 1) -- the sign of a
    zero that comes out of the clamp is not pinned (-0.0 == 0.0 in exact())."""
    pos = cperm(np.arange(C)) if perm and mut != "perm_ignored" else np.arange(C)
    out = np.ascontiguousarray(src[..., pos].transpose(0, 3, 1, 2))
    return np.minimum(np.maximum(out, F32(0)), F32(1)) if clamp01 else out


# ---------------------------------------------------------------------------------------------------------------------------
# Refusals of the hooks (include/rgbd_amd.h): every call below must return -22 before anything is launched
# ---------------------------------------------------------------------------------------------------------------------------
def refusals(L, x, y, v, x1, y1, w0, w1, stream=None):
    """-> [(label, rc)].  x / x1: 16-byte aligned tensors, y / y1: destinations, v: a vector buffer (device pointers as ints; each
    at least 64 Ki floats, though no call here may reach a device), w0 / w1: host float pointers of 48 * 3 weights."""
    out = []

    def run(name, good, bads):
        fn = getattr(L, name)
        for label, kw in bads:
            a = dict(good)
            a.update(kw)
            out.append((f"{name}: {label}", fn(*a.values(), stream)))

    big = 1 << 20
    run("rgbd_pw_channel_mean", dict(x=x, N=2, HW=35, cs=64, C=48, mean=v, mstride=64), [
        ("x NULL", dict(x=None)), ("mean NULL", dict(mean=None)), ("N 0", dict(N=0)), ("HW 0", dict(HW=0)), ("C 0", dict(C=0)),
        ("HW < 0", dict(HW=-3)), ("cs < C", dict(cs=44)), ("cs % 4", dict(cs=50)), ("mstride < C", dict(mstride=44)),
        ("mstride % 4", dict(mstride=50)), ("N > 65535", dict(N=65536, HW=1)), (">= 2^31", dict(N=64, HW=big))])
    run("rgbd_pw_se_gate", dict(mean=v, N=2, C=48, w0=w0, w1=w1, mstride=64, perm=1, gate=y), [
        ("mean NULL", dict(mean=None)), ("w0 NULL", dict(w0=None)), ("w1 NULL", dict(w1=None)), ("gate NULL", dict(gate=None)),
        ("N 0", dict(N=0)), ("C 0", dict(C=0)), ("C % 16", dict(C=40)), ("mstride < C", dict(mstride=44)),
        ("mstride % 4", dict(mstride=50)), ("perm 2", dict(perm=2)), ("perm -1", dict(perm=-1))])
    run("rgbd_pw_bilinear", dict(x=x, N=2, h=5, w=7, cs=20, y=y, H=9, W=11, x1=None, y1=None, ref=0), [
        ("x NULL", dict(x=None)), ("y NULL", dict(y=None)), ("h 0", dict(h=0)), ("W 0", dict(W=0)), ("N 0", dict(N=0)),
        ("cs 0", dict(cs=0)), ("cs % 4", dict(cs=18)), ("x1 without y1", dict(x1=x1)), ("y1 without x1", dict(y1=y1)),
        ("ref < 0", dict(ref=-1)), ("ref > cs", dict(ref=21)), ("x misaligned", dict(x=x + 4)), ("y misaligned", dict(y=y + 8)),
        ("x1 misaligned", dict(x1=x1 + 4, y1=y1)), (">= 2^31", dict(H=65536, W=65536))])
    run("rgbd_pw_maxpool7s3", dict(x=x, N=2, H=10, W=22, cs=64, y=y, x1=None, y1=None), [
        ("x NULL", dict(x=None)), ("y NULL", dict(y=None)), ("H < 7", dict(H=6)), ("W < 7", dict(W=6)), ("N 0", dict(N=0)),
        ("cs % 4", dict(cs=62)), ("x1 without y1", dict(x1=x1)), ("y1 without x1", dict(y1=y1)), ("y misaligned", dict(y=y + 4)),
        (">= 2^31", dict(N=64, H=8192, W=8192))])
    run("rgbd_pw_channel_scale", dict(x=x, N=2, HW=35, xcs=64, C=48, s=v, sstride=80, mode=1, y=y, ycs=96), [
        ("x NULL", dict(x=None)), ("scale NULL", dict(s=None)), ("y NULL", dict(y=None)), ("C % 4", dict(C=46)), ("C 0", dict(C=0)),
        ("xcs < C", dict(xcs=44)), ("ycs < C", dict(ycs=44)), ("xcs % 4", dict(xcs=66)), ("ycs % 4", dict(ycs=98)),
        ("sstride < C", dict(sstride=44)), ("sstride % 4", dict(sstride=82)), ("mode 2", dict(mode=2)), ("HW 0", dict(HW=0)),
        ("scale misaligned", dict(s=v + 4)), ("y misaligned", dict(y=y + 4)), (">= 2^31", dict(HW=1 << 24))])
    run("rgbd_pw_copy_channels", dict(src=x, scs=64, dst=y, dcs=208, npix=37, C=48), [
        ("src NULL", dict(src=None)), ("dst NULL", dict(dst=None)), ("C % 4", dict(C=46)), ("scs < C", dict(scs=44)),
        ("dcs < C", dict(dcs=44)), ("scs % 4", dict(scs=66)), ("npix 0", dict(npix=0)), ("dst misaligned", dict(dst=y + 4)),
        (">= 2^31", dict(npix=1 << 25))])
    run("rgbd_pw_im2col5s2", dict(x=x, N=2, H=9, W=14, cs=16, C=3, y=y, KP=80), [
        ("x NULL", dict(x=None)), ("y NULL", dict(y=None)), ("25 C > KP", dict(KP=32)), ("KP % 16", dict(C=1, KP=40)),
        ("C > cs", dict(C=20, KP=512)), ("C 0", dict(C=0)), ("H 0", dict(H=0)), ("KP 0", dict(KP=0)),
        (">= 2^31", dict(N=64, H=16384, W=16384))])
    run("rgbd_pw_fill_zero", dict(p=y, n=1025), [
        ("p NULL", dict(p=None)), ("n 0", dict(n=0)), ("n < 0", dict(n=-1)), (">= 2^31", dict(n=1 << 31))])
    run("rgbd_pw_nchw_to_nhwc", dict(src=x, N=2, C=3, H=5, W=7, dst=y, cs=16, perm=1), [
        ("src NULL", dict(src=None)), ("dst NULL", dict(dst=None)), ("C 0", dict(C=0)), ("cs < C", dict(C=20)),
        ("cs % 4", dict(cs=18)), ("perm with cs % 16", dict(C=20, cs=20)), ("perm 2", dict(perm=2)), ("W 0", dict(W=0)),
        ("dst misaligned", dict(dst=y + 4)), (">= 2^31", dict(N=8, H=8192, W=8192))])
    run("rgbd_pw_nhwc_to_nchw", dict(src=x, N=2, C=3, H=5, W=7, cs=16, dst=y, clamp01=1, perm=1), [
        ("src NULL", dict(src=None)), ("dst NULL", dict(dst=None)), ("C 0", dict(C=0)), ("cs < C", dict(C=20)),
        ("cs % 4", dict(cs=18)), ("perm with cs % 16", dict(C=20, cs=20)), ("perm -1", dict(perm=-1)),
        ("clamp01 2", dict(clamp01=2)), ("N 0", dict(N=0)), (">= 2^31", dict(N=8, H=8192, W=8192))])
    return out
