"""Cases shared by tests/test_entropy_cases.py (CPU: can the checks fail?) and tests/test_gpu_entropy.py (GPU: the entropy
stage's engine-layout kernels of csrc/entropy.hip ALONE, through the C ABI's rgbd_ckbd_estimate_part / rgbd_slice_estimate /
rgbd_ckbd_part / rgbd_z_quant / rgbd_z_dequant / rgbd_eb_forward).

For every case: deterministic inputs as logical NCHW tensors, their layout as the engine's NHWC buffers (own channel stride
per tensor, optional channel permutation, a sentinel in every element a kernel must not touch), plain references, an fp32 CPU
restatement that works on the laid-out buffers like the kernel does (`emulate`, with deliberately wrong variants), and ONE
acceptance function per kernel family (`accept`) that the CPU restatements, their mutants and the GPU outputs all go through.

References
  Gaussian likelihood (entropy_models.py:534-558): the reference's fp32 steps exactly up to the likelihood --
      out = fp32(rint(y - mean) + mean) (half to even), v = |fp32(out - mean)|, scale = max(scale, 0.11f) --
      then U = 0.5 erfc(-2^-0.5 (0.5 - v) / scale), L likewise, lik64 = U - L in fp64 from those fp32 values.
  Factorised prior (entropy_models.py:369-428): out = fp32(rint(z - med) + med), then the logits of the 1-3-3-3-3-1 network
      and |sigmoid(s up) - sigmoid(s lo)|, s = -sign(lo + up), in fp64 end to end from the RAW parameters.
  Integer kernels: numpy statements of symbol / index / y_hat and of the two stream orders.

Tolerances (none fixed in advance; all measured against the fp64 reference on the case's own inputs)
  exact: y_hat / z_hat, symbols, indexes, untouched sentinels, pad channels.
  Gaussian likelihood, where lik64 >= 2e-9: |lik - lik64| <= 4 k0 E, E = 2^-24 ((1 + 2 x_u^2) U + (1 + 2 x_l^2) L) the fp32
      rounding envelope (x_u / x_l: the erfc arguments; one rounding of each erfc value plus the amplification
      |d erfc / erfc| ~ 2 x^2 of the argument's rounding), k0 the smallest k at which the fp32 torch restatement meets k E on
      the same inputs.  The factor 4 pays for a device erfcf that differs from ATen's by a few ulp and for one more rounding
      in the division chain.
  Factorised-prior likelihood: per decade of lik64 in [1e-9, 1), the worst relative error may be 4 times the fp32 torch
      restatement's worst in that decade, the latter never taken below 8 * 2^-24.
  The floor: lik64 < 0.5e-9 must give exactly 1e-9f; 0.5e-9 <= lik64 < 2e-9 may give the floor or a value within the bound
      ("undecided").
"""
import functools
import zlib

import numpy as np
import torch

from oracle import elic_oracle as eo

f32 = np.float32
SENT = f32(-777.25)  # float buffers: what a kernel must leave alone
ISENT = -99          # int32 buffers
FLOOR = f32(1e-9)
BOUND = f32(0.11)
EPS24 = 2.0 ** -24
SPECIAL_SCALES = np.array([-1.0, 0.0, 0.05, 0.11, np.nextafter(f32(0.11), f32(1.0)), 0.5, 1.0, 64.0, 256.0], f32)


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) % (2 ** 31))


def case_id(c):
    return c["id"]


@functools.lru_cache(maxsize=None)
def _table():
    t = eo.scale_table().numpy().astype(f32)
    t.setflags(write=False)
    return t


def scale_table():
    """the product's 64-entry scale table (get_scale_table()), fp32"""
    return _table()


# ================================================================================================ layout
def cperm(c, on=1):
    """where logical channel c sits inside its group of 16 (csrc/common.h: rgbd_cperm; an involution)"""
    c = np.asarray(c)
    return ((c & ~15) | ((c & 3) << 2) | ((c >> 2) & 3)) if on else c


def to_nhwc(x, cs, perm, fill=SENT, off=0, into=None):
    """logical NCHW [B, C, h, w] -> the engine's [B, h, w, cs]; channel c at position off + cperm(c); the rest = fill"""
    B, C, h, w = x.shape
    t = np.full((B, h, w, cs), fill, x.dtype) if into is None else into
    t[..., off + cperm(np.arange(C), perm)] = x.transpose(0, 2, 3, 1)
    return t


def from_nhwc(t, C, perm, off=0):
    return np.ascontiguousarray(t[..., off + cperm(np.arange(C), perm)].transpose(0, 3, 1, 2))


def anchor_mask(h, w, anchor=True):
    """[h, w] bool: the positions a checkerboard half codes ((row + col) odd for the anchor half, ckbd.py:37-48)"""
    r, c = np.arange(h)[:, None], np.arange(w)[None, :]
    return ((r + c) % 2 == 1) == bool(anchor)


def pack(x, anchor):
    """[..., h, w] -> [..., h, w / 2]: the half's columns of every row, in order (ckbd.py:83-105)"""
    h, w = x.shape[-2:]
    return x[..., anchor_mask(h, w, anchor)].reshape(x.shape[:-2] + (h, w // 2))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _first_diff(got, want):
    bad = np.flatnonzero(np.ascontiguousarray(got).view(np.uint32).reshape(-1) != np.ascontiguousarray(want).view(np.uint32).reshape(-1))
    if not bad.size:
        return "equal"
    i = np.unravel_index(bad[0], got.shape)
    return f"{bad.size} of {got.size} differ; first at {tuple(int(v) for v in i)}: got {got[i]!r}, want {want[i]!r}"


# ================================================================================================ Gaussian likelihood
def gauss_inputs(key, shape):
    """y, mean, scale [B, C, h, w] fp32.  scale: a third of the elements cycle through SPECIAL_SCALES, the rest are log-uniform
    in [0.11, 256].  Residuals: the quantised magnitude is aimed at t effective scales past the bin edge, t from 0 to 10 (the
    fp64 likelihood passes 1e-9 near 5.5 ... 6), with 12 % exact ties (+-0.5, +-1.5, +-2.5) on dyadic means, 20 % dyadic means
    with residuals on a 1/8 grid, and the rest non-dyadic means of magnitude up to 30 (fp32(out - mean) is no integer)."""
    rng = _rng("gauss", key, tuple(shape))
    n = int(np.prod(shape))
    scale = np.exp(rng.uniform(np.log(0.11), np.log(256.0), n)).astype(f32)
    k = n // 3
    scale[:k] = SPECIAL_SCALES[np.arange(k) % SPECIAL_SCALES.size]
    se = np.maximum(scale, BOUND).astype(np.float64)
    u = rng.uniform(size=n)
    t = np.where(u < 0.5, rng.uniform(0, 4.4, n), np.where(u < 0.58, rng.uniform(4.4, 5.2, n), rng.uniform(6.4, 10.0, n)))
    t[rng.uniform(size=n) < 0.05] = 0.0
    v = np.rint(t * se + 0.5)  # the integer |rint(y - mean)| aimed at
    sign = rng.choice([-1.0, 1.0], n)
    kind = rng.uniform(size=n)
    dyadic = np.rint(rng.uniform(-30, 30, n) * 4) / 4
    mean = np.where(kind < 0.32, dyadic, rng.uniform(-30, 30, n)).astype(f32)
    r = sign * v + np.where(kind < 0.32, np.rint(rng.uniform(-3.4, 3.4, n)) / 8, rng.uniform(-0.49, 0.49, n))
    tie = kind < 0.12
    r = np.where(tie, sign * rng.choice([0.5, 1.5, 2.5], n), r)
    y = (mean.astype(np.float64) + r).astype(f32)
    p = rng.permutation(n)
    return tuple(a[p].reshape(shape) for a in (y, mean, scale))


def gauss_steps32(y, mean, scale, rounding="even", v_from="out", bound=BOUND):
    """the reference's fp32 steps up to the likelihood: (out, v, scale)"""
    d = (y - mean).astype(f32)
    if rounding == "even":
        q = np.rint(d)
    else:  # half away from zero
        q = (np.sign(d) * np.floor(np.abs(d) + f32(0.5))).astype(f32)
    out = (q + mean).astype(f32)
    if v_from == "out":
        v = np.abs((out - mean).astype(f32))
    else:  # rint(y) - mean
        v = np.abs((np.rint(y) - mean).astype(f32))
    return out, v, np.maximum(scale, f32(bound))


def gauss_reference(y, mean, scale):
    """dict(out fp32, lik64, E, floor (bool: must be the floor), undecided (bool), judged (bool))"""
    out, v, sc = gauss_steps32(y, mean, scale)
    v64, s64 = torch.from_numpy(v.astype(np.float64)), torch.from_numpy(sc.astype(np.float64))
    xu = -(2.0 ** -0.5) * ((0.5 - v64) / s64)
    xl = -(2.0 ** -0.5) * ((-0.5 - v64) / s64)
    U, L = 0.5 * torch.erfc(xu), 0.5 * torch.erfc(xl)
    lik = (U - L).numpy()
    E = (EPS24 * ((1 + 2 * xu ** 2) * U + (1 + 2 * xl ** 2) * L)).numpy()
    return {"out": out, "lik64": lik, "E": E, "floor": lik < 0.5e-9, "undecided": (lik >= 0.5e-9) & (lik < 2e-9), "judged": lik >= 2e-9}


def gauss_lik32(v, sc, form="erfc"):
    """the likelihood in torch fp32 from the fp32 steps (entropy_models.py:489-494, 549-558), floored"""
    v, sc = torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(np.ascontiguousarray(sc))
    cst = float(-(2 ** -0.5))
    if form == "erfc":
        lik = 0.5 * torch.erfc(cst * ((0.5 - v) / sc)) - 0.5 * torch.erfc(cst * ((-0.5 - v) / sc))
    else:  # the textbook form 0.5 (erf(b) - erf(a)): cancels in the tails
        lik = 0.5 * (torch.erf(-cst * ((0.5 + v) / sc)) - torch.erf(-cst * ((v - 0.5) / sc)))
    return torch.clamp(lik, min=1e-9).numpy()


def gauss_k(lik, ref):
    """smallest k with |lik - lik64| <= k E over the judged positions"""
    j = ref["judged"]
    return float((np.abs(lik.astype(np.float64) - ref["lik64"])[j] / ref["E"][j]).max()) if j.any() else 0.0


def _lik_verdict(name, lik, ref, within, fails):
    """the floor rules shared by both likelihood kinds; `within`: bool array, the value meets the case's error bound"""
    isfloor = lik.view(np.uint32) == FLOOR.view(np.uint32)
    bad = ref["floor"] & ~isfloor
    if bad.any():
        fails.append(f"{name}: {int(bad.sum())} positions with lik64 < 0.5e-9 are not exactly 1e-9f (first {lik[bad][0]!r})")
    bad = ref["undecided"] & ~(isfloor | within)
    if bad.any():
        fails.append(f"{name}: {int(bad.sum())} undecided positions are neither the floor nor within the bound")
    bad = ref["judged"] & ~within
    if bad.any():
        i = np.flatnonzero(bad.reshape(-1))[0]
        fails.append(f"{name}: {int(bad.sum())} of {int(ref['judged'].sum())} judged positions outside the bound; first: got "
                     f"{lik.reshape(-1)[i]!r}, lik64 {ref['lik64'].reshape(-1)[i]!r}")


# ------------------------------------------------------------------------------------------------ checkerboard estimate
# (id, B, h, w, C, perm): strides 48 / 40 / 32 for y / y_hat / lik, params 2 C + 8; "grid": 655 360 elements per half,
# above the 2048 x 256 grid cap, so the grid-stride loop runs
CKBD_EST = [("c16", 2, 3, 6, 16, 0), ("c16p", 2, 3, 6, 16, 1), ("c32", 2, 3, 6, 32, 0), ("c32p", 2, 3, 6, 32, 1),
            ("grid", 2, 32, 64, 320, 1)]


def _strides(C, big):
    return (C, C + 16, C + 8, 2 * C + 8) if big else (48, 40, 32, 2 * C + 8)  # ycs, yhcs, lcs, pcs


@functools.lru_cache(maxsize=None)
def ckbd_est_case(cid):
    _, B, h, w, C, perm = next(c for c in CKBD_EST if c[0] == cid)
    y, mean, scale = gauss_inputs(("ckbd_est", cid), (B, C, h, w))
    ycs, yhcs, lcs, pcs = _strides(C, cid == "grid")
    params = to_nhwc(scale, pcs, perm)
    to_nhwc(mean, pcs, perm, off=C, into=params)
    ref = gauss_reference(y, mean, scale)
    _, v, sc = gauss_steps32(y, mean, scale)
    ref["k0"] = gauss_k(gauss_lik32(v, sc), ref)
    return {"id": cid, "kind": "ckbd_est", "B": B, "h": h, "w": w, "C": C, "perm": perm, "ycs": ycs, "yhcs": yhcs, "lcs": lcs,
            "pcs": pcs, "y": y, "mean": mean, "scale": scale, "buf_y": to_nhwc(y, ycs, perm), "buf_params": params, "ref": ref}


def emulate_ckbd_est(c, variant=None):
    """fp32 CPU restatement of ckbd_estimate_kernel on the case's buffers: the anchor pass, then the non-anchor pass, on the
    same sentinel-filled outputs.  Returns yhat_a / lik_a (after the anchor pass) and yhat / lik (after both)."""
    B, h, w, C = c["B"], c["h"], c["w"], c["C"]
    pin = 0 if variant == "perm_in" else c["perm"]
    pout = 0 if variant == "perm_out" else c["perm"]
    y, scale, mean = from_nhwc(c["buf_y"], C, pin), from_nhwc(c["buf_params"], C, pin), from_nhwc(c["buf_params"], C, pin, off=C)
    out, v, sc = gauss_steps32(y, mean, scale, rounding="away" if variant == "round_away" else "even",
                               v_from="rint_y" if variant == "v_from_rint_y" else "out", bound=0.10 if variant == "bound_0.10" else BOUND)
    lik = gauss_lik32(v, sc, form="erf" if variant == "erf_form" else "erfc")
    yh, lk = np.full((B, h, w, c["yhcs"]), SENT, f32), np.full((B, h, w, c["lcs"]), SENT, f32)
    res = {}
    for anchor in (1, 0):
        m = anchor_mask(h, w, anchor != (variant == "parity"))
        cur_y, cur_l = from_nhwc(yh, C, pout), from_nhwc(lk, C, pout)
        if anchor:
            cur_y[..., ~m] = 0
        cur_y[..., m], cur_l[..., m] = out[..., m], lik[..., m]
        to_nhwc(cur_y, c["yhcs"], pout, into=yh)
        to_nhwc(cur_l, c["lcs"], pout, into=lk)
        if anchor:
            res["yhat_a"], res["lik_a"] = yh.copy(), lk.copy()
    res["yhat"], res["lik"] = yh, lk
    return res


def accept_ckbd_est(c, o, stats=None):
    """-> list of failures (empty: accepted).  o: yhat_a / lik_a / yhat / lik buffers (see emulate_ckbd_est)."""
    fails = []
    h, w, C, perm, ref = c["h"], c["w"], c["C"], c["perm"], c["ref"]
    am = anchor_mask(h, w, True)
    # after the anchor pass: the anchor half computed, the other half of y_hat zero, of lik untouched
    want = ref["out"].copy()
    want[..., ~am] = 0
    wl = np.full_like(ref["out"], SENT)
    for name, want_y, lik_mask in (("anchor pass", want, am), ("both passes", ref["out"], np.ones_like(am))):
        sfx = "_a" if name == "anchor pass" else ""
        yh, lk = o["yhat" + sfx], o["lik" + sfx]
        if not bits_equal(from_nhwc(yh, C, perm), want_y):
            fails.append(f"{name}: y_hat differs: {_first_diff(from_nhwc(yh, C, perm), want_y)}")
        if not bits_equal(to_nhwc(from_nhwc(yh, C, perm), c["yhcs"], perm), yh) or \
           not bits_equal(to_nhwc(from_nhwc(lk, C, perm), c["lcs"], perm), lk):
            fails.append(f"{name}: a sentinel outside the slice's channels was overwritten")
        lik = from_nhwc(lk, C, perm)
        if not bits_equal(lik[..., ~lik_mask], wl[..., ~lik_mask]):
            fails.append(f"{name}: lik written outside the half")
        sub = {k: v[..., lik_mask] for k, v in ref.items() if isinstance(v, np.ndarray)}
        got = np.ascontiguousarray(lik[..., lik_mask])
        within = np.abs(got.astype(np.float64) - sub["lik64"]) <= 4 * ref["k0"] * sub["E"]
        _lik_verdict(name, got, sub, within, fails)
        if stats is not None and not sfx:
            stats.update({"k": gauss_k(got, sub), "k0": ref["k0"]})
    return fails


# ------------------------------------------------------------------------------------------------ slice estimate
# (id, B, h, w, C, second destination): mean / scale / y from three tensors with three strides; odd w; "grid": 655 360 elements
SLICE_EST = [("c16", 2, 3, 5, 16, 1), ("c32", 2, 3, 5, 32, 0), ("c20", 1, 5, 7, 20, 1), ("grid", 2, 32, 32, 320, 1)]


@functools.lru_cache(maxsize=None)
def slice_est_case(cid):
    _, B, h, w, C, two = next(c for c in SLICE_EST if c[0] == cid)
    y, mean, scale = gauss_inputs(("slice_est", cid), (B, C, h, w))
    ycs, mcs, scs, lcs, cs0, cs1 = (C + 16, C + 8, C, C + 3, C + 32, C + 5) if cid == "grid" else (48, 40, 32, 37, 64, 35)
    ref = gauss_reference(y, mean, scale)
    _, v, sc = gauss_steps32(y, mean, scale)
    ref["k0"] = gauss_k(gauss_lik32(v, sc), ref)
    return {"id": cid, "kind": "slice_est", "B": B, "h": h, "w": w, "C": C, "two": two, "ycs": ycs, "mcs": mcs, "scs": scs, "lcs": lcs,
            "cs0": cs0, "cs1": cs1, "y": y, "mean": mean, "scale": scale, "buf_y": to_nhwc(y, ycs, 0), "buf_mean": to_nhwc(mean, mcs, 0),
            "buf_scale": to_nhwc(scale, scs, 0), "ref": ref}


def emulate_slice_est(c, variant=None):
    C = c["C"]
    y, mean, scale = from_nhwc(c["buf_y"], C, 0), from_nhwc(c["buf_mean"], C, 0), from_nhwc(c["buf_scale"], C, 0)
    out, v, sc = gauss_steps32(y, mean, scale, rounding="away" if variant == "round_away" else "even",
                               v_from="rint_y" if variant == "v_from_rint_y" else "out", bound=0.10 if variant == "bound_0.10" else BOUND)
    lik = gauss_lik32(v, sc, form="erf" if variant == "erf_form" else "erfc")
    res = {"lik": to_nhwc(lik, c["lcs"], 0), "d0": to_nhwc(out, c["cs0"], 0)}
    if c["two"]:
        res["d1"] = to_nhwc(out, c["cs1"], 0)
    return res


def accept_slice_est(c, o, stats=None):
    fails = []
    C, ref = c["C"], c["ref"]
    for name, cs in (("d0", c["cs0"]),) + ((("d1", c["cs1"]),) if c["two"] else ()):
        if not bits_equal(o[name], to_nhwc(ref["out"], cs, 0)):
            fails.append(f"{name}: y_hat or a sentinel differs: {_first_diff(o[name], to_nhwc(ref['out'], cs, 0))}")
    lik = from_nhwc(o["lik"], C, 0)
    if not bits_equal(to_nhwc(lik, c["lcs"], 0), o["lik"]):
        fails.append("lik: a sentinel outside the slice's channels was overwritten")
    within = np.abs(lik.astype(np.float64) - ref["lik64"]) <= 4 * ref["k0"] * ref["E"]
    _lik_verdict("lik", lik, ref, within, fails)
    if stats is not None:
        stats.update({"k": gauss_k(lik, ref), "k0": ref["k0"]})
    return fails


# ================================================================================================ factorised prior
FILTERS = (1, 3, 3, 3, 3, 1)


def eb_params(key, C, perturbed):
    """compressai's initialisation (entropy_models.py:290-312; init_scale 10, filters 3, 3, 3, 3), optionally with normal
    perturbations (0.3 on matrices, 0.5 on factors).  Every third channel gets +3 on _matrix0 (a density about 8 times
    narrower), so that z within +-60 of the median reaches the 1e-9 floor; one matrix entry of channel 1 is 25 (above the
    softplus threshold 20 where softplus(v) = v to fp32) and one of channel 4 is 100 (where an unthresholded fp32 softplus
    overflows).  Medians: non-integer, half of them dyadic.  -> dict of fp32 arrays"""
    rng = _rng("eb", key, C, perturbed)
    scale = 10.0 ** (1 / 5)
    p = {}
    for i in range(5):
        init = np.log(np.expm1(1 / scale / FILTERS[i + 1]))
        p[f"_matrix{i}"] = np.full((C, FILTERS[i + 1], FILTERS[i]), init, np.float64)
        p[f"_bias{i}"] = rng.uniform(-0.5, 0.5, (C, FILTERS[i + 1], 1))
        if i < 4:
            p[f"_factor{i}"] = np.zeros((C, FILTERS[i + 1], 1))
        if perturbed:
            p[f"_matrix{i}"] = p[f"_matrix{i}"] + 0.3 * rng.standard_normal(p[f"_matrix{i}"].shape)
            if i < 4:
                p[f"_factor{i}"] = 0.5 * rng.standard_normal(p[f"_factor{i}"].shape)
    p["_matrix0"][2::3] += 3.0
    p["_matrix2"][1, 0, 0] = 25.0
    p["_matrix4"][4, 0, 1] = 100.0
    med = rng.uniform(-3, 3, C)
    med[::2] = np.rint(med[::2] * 8) / 8 + 1 / 16
    p["medians"] = med
    return {k: np.ascontiguousarray(v, f32) for k, v in p.items()}


def eb_z(key, prm, shape):
    """z [B, C, h, w]: median + r; r uniform in +-60 (60 %), normal with sigma 5 (28 %), exact half-integers (12 %)"""
    rng = _rng("ebz", key, tuple(shape))
    B, C, h, w = shape
    u = rng.uniform(size=shape)
    r = np.where(u < 0.6, rng.uniform(-60, 60, shape), np.where(u < 0.88, 5 * rng.standard_normal(shape),
                                                               rng.randint(-6, 6, shape) + 0.5))
    return (prm["medians"].astype(np.float64).reshape(1, C, 1, 1) + r).astype(f32)


def eb_out32(z, med, rounding="even"):
    m = med.reshape(1, -1, 1, 1).astype(f32)
    d = (z - m).astype(f32)
    q = np.rint(d) if rounding == "even" else (np.sign(d) * np.floor(np.abs(d) + f32(0.5))).astype(f32)
    return (q + m).astype(f32)


def _eb_logits(prm, v, dtype, softplus="threshold", use_factor_tanh=True):
    """entropy_models.py:369-388 on v [C, 1, n] in `dtype` (torch)"""
    x = v
    for i in range(5):
        m = torch.from_numpy(prm[f"_matrix{i}"]).to(dtype)
        if softplus == "threshold":
            m = torch.nn.functional.softplus(m)  # threshold 20
        else:
            m = torch.log1p(torch.exp(m))
        x = torch.matmul(m, x) + torch.from_numpy(prm[f"_bias{i}"]).to(dtype)
        if i < 4:
            f = torch.from_numpy(prm[f"_factor{i}"]).to(dtype)
            x = x + (torch.tanh(f) if use_factor_tanh else f) * torch.tanh(x)
    return x


def eb_lik(prm, out, dtype=torch.float32, sign_flip=True, **kw):
    """|sigmoid(s up) - sigmoid(s lo)| of the quantised values out [B, C, h, w] (fp32), computed in `dtype`, unfloored"""
    B, C, h, w = out.shape
    v = torch.from_numpy(np.ascontiguousarray(out.transpose(1, 0, 2, 3).reshape(C, 1, -1))).to(dtype)
    lo, up = _eb_logits(prm, v - 0.5, dtype, **kw), _eb_logits(prm, v + 0.5, dtype, **kw)
    s = -torch.sign(lo + up) if sign_flip else torch.ones_like(lo)
    lik = torch.abs(torch.sigmoid(s * up) - torch.sigmoid(s * lo))
    return lik.reshape(C, B, h, w).permute(1, 0, 2, 3).contiguous().numpy()


DECADES = [(10.0 ** e, 10.0 ** (e + 1)) for e in range(-9, 0)]


def eb_decade_worst(lik, ref):
    """worst relative error of lik against lik64 per decade of lik64 (judged positions only; 0 where a decade is empty)"""
    rel = np.abs(lik.astype(np.float64) - ref["lik64"]) / np.maximum(ref["lik64"], 1e-300)
    rel = np.where(np.isfinite(rel), rel, np.inf)
    return [float(rel[ref["judged"] & (ref["lik64"] >= a) & (ref["lik64"] < b)].max(initial=0.0)) for a, b in DECADES]


# (id, B, h, w, C, zcs, perm, perturbed): C = 24 in zcs = 32: pad positions exist and, under perm, are scattered
EB = [("c24", 2, 3, 5, 24, 32, 0, 1), ("c24p", 2, 3, 5, 24, 32, 1, 1), ("c24p_init", 2, 3, 5, 24, 32, 1, 0),
      ("c192", 2, 3, 5, 192, 192, 0, 1), ("c192p", 2, 3, 5, 192, 192, 1, 1)]


def to_zbuf(x, zcs, perm, fill):
    """[B, C, h, w] -> [B, h, w, zcs] with position pc holding channel cperm(pc) when that is < C, else `fill`"""
    B, C, h, w = x.shape
    t = np.full((B, h, w, zcs), fill, x.dtype)
    pc = np.arange(zcs)
    ch = cperm(pc, perm)
    t[..., pc[ch < C]] = x.transpose(0, 2, 3, 1)[..., ch[ch < C]]
    return t


def from_zbuf(t, C, perm):
    pc = np.arange(t.shape[-1])
    ch = cperm(pc, perm)
    out = np.empty(t.shape[:3] + (C,), t.dtype)
    out[..., ch[ch < C]] = t[..., pc[ch < C]]
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2))


@functools.lru_cache(maxsize=None)
def eb_case(cid):
    _, B, h, w, C, zcs, perm, perturbed = next(c for c in EB if c[0] == cid)
    prm = eb_params(cid, C, perturbed)
    z = eb_z(cid, prm, (B, C, h, w))
    out = eb_out32(z, prm["medians"])
    lik64 = eb_lik(prm, out, torch.float64)
    ref = {"out": out, "lik64": lik64, "floor": lik64 < 0.5e-9, "undecided": (lik64 >= 0.5e-9) & (lik64 < 2e-9), "judged": lik64 >= 2e-9}
    ref["worst0"] = eb_decade_worst(np.maximum(eb_lik(prm, out), FLOOR), ref)
    return {"id": cid, "kind": "eb", "B": B, "h": h, "w": w, "C": C, "zcs": zcs, "perm": perm, "prm": prm, "z": z,
            "buf_z": to_zbuf(z, zcs, perm, SENT), "ref": ref}


def emulate_eb(c, variant=None):
    C, zcs = c["C"], c["zcs"]
    pin = 0 if variant == "perm_in" else c["perm"]
    pout = 0 if variant == "perm_out" else c["perm"]
    z = from_zbuf(c["buf_z"], C, pin)
    out = eb_out32(z, c["prm"]["medians"], rounding="away" if variant == "round_away" else "even")
    lik = eb_lik(c["prm"], out, sign_flip=variant != "no_sign_flip", softplus="plain" if variant == "softplus_plain" else "threshold",
                 use_factor_tanh=variant != "factor_no_tanh")
    with np.errstate(invalid="ignore"):
        lik = np.where(np.isnan(lik), lik, np.maximum(lik, FLOOR)).astype(f32)
    return {"zhat": to_zbuf(out, zcs, pout, f32(0)), "lik": to_zbuf(lik, zcs, pout, f32(0))}


def accept_eb(c, o, stats=None):
    fails = []
    C, zcs, perm, ref = c["C"], c["zcs"], c["perm"], c["ref"]
    if not bits_equal(o["zhat"], to_zbuf(ref["out"], zcs, perm, f32(0))):
        fails.append(f"z_hat (pad positions: 0) differs: {_first_diff(o['zhat'], to_zbuf(ref['out'], zcs, perm, f32(0)))}")
    lik = from_zbuf(o["lik"], C, perm)
    if not bits_equal(to_zbuf(lik, zcs, perm, f32(0)), o["lik"]):
        fails.append("lik: a pad position is not 0")
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(lik.astype(np.float64) - ref["lik64"]) / np.maximum(ref["lik64"], 1e-300)
    within = np.zeros(lik.shape, bool)
    for (a, b), w0 in zip(DECADES, ref["worst0"]):
        m = (ref["lik64"] >= a) & (ref["lik64"] < b)
        within[m] = rel[m] <= 4 * max(w0, 8 * EPS24)
    # (below 1e-9 only undecided positions are looked at: the bound of the lowest decade)
    m = ref["lik64"] < 1e-9
    within[m] = rel[m] <= 4 * max(ref["worst0"][0], 8 * EPS24)
    _lik_verdict("lik", lik, ref, within, fails)
    if stats is not None:
        stats.update({"worst": eb_decade_worst(lik, ref), "worst0": ref["worst0"]})
    return fails


# ================================================================================================ z path (integer)
# (id, B, h, w, C, zcs, perm)
ZQ = [("c24", 2, 3, 5, 24, 32, 0), ("c24p", 2, 3, 5, 24, 32, 1), ("c192", 2, 3, 5, 192, 192, 0), ("c192p", 2, 3, 5, 192, 192, 1),
      ("c20", 1, 2, 3, 20, 21, 0)]
GUARD = 16


@functools.lru_cache(maxsize=None)
def zq_case(cid):
    _, B, h, w, C, zcs, perm = next(c for c in ZQ if c[0] == cid)
    prm = eb_params(("zq", cid), C, 0)
    z = eb_z(("zq", cid), prm, (B, C, h, w))
    med = prm["medians"]
    sym = np.rint((z - med.reshape(1, C, 1, 1)).astype(f32)).astype(np.int32)  # (b, c, row, col): the stream order
    idx = np.broadcast_to(np.arange(C, dtype=np.int32).reshape(1, C, 1, 1), sym.shape)
    zhat = (sym.astype(f32) + med.reshape(1, C, 1, 1)).astype(f32)
    n = sym.size
    want_sym, want_idx = np.full(n + GUARD, ISENT, np.int32), np.full(n + GUARD, ISENT, np.int32)
    want_sym[:n], want_idx[:n] = sym.reshape(-1), idx.reshape(-1)
    return {"id": cid, "kind": "zq", "B": B, "h": h, "w": w, "C": C, "zcs": zcs, "perm": perm, "med": med, "z": z, "n": n,
            "buf_z": to_zbuf(z, zcs, perm, SENT), "want_sym": want_sym, "want_idx": want_idx, "want_zhat": to_zbuf(zhat, zcs, perm, f32(0))}


def emulate_zq(c, variant=None):
    C = c["C"]
    pin = 0 if variant == "perm_in" else c["perm"]
    pout = 0 if variant == "perm_out" else c["perm"]
    z = from_zbuf(c["buf_z"], C, pin)
    med = c["med"].reshape(1, C, 1, 1)
    d = (z - med).astype(f32)
    q = np.rint(d) if variant != "round_away" else np.sign(d) * np.floor(np.abs(d) + f32(0.5))
    sym = np.full(c["n"] + GUARD, ISENT, np.int32)
    idx = sym.copy()
    sym[:c["n"]] = q.astype(np.int32).reshape(-1)
    idx[:c["n"]] = np.broadcast_to(np.arange(C, dtype=np.int32).reshape(1, C, 1, 1), q.shape).reshape(-1)
    return {"sym": sym, "idx": idx, "zhat": to_zbuf((q.astype(np.int32).astype(f32) + med).astype(f32), c["zcs"], pout, f32(0))}


def accept_zq(c, o, stats=None):
    fails = []
    for k, want in (("sym", c["want_sym"]), ("idx", c["want_idx"])):
        if not np.array_equal(o[k], want):
            bad = np.flatnonzero(o[k] != want)
            fails.append(f"{k}: {bad.size} differ (guard included); first at {int(bad[0])}: got {int(o[k][bad[0]])}, want {int(want[bad[0]])}")
    if not bits_equal(o["zhat"], c["want_zhat"]):
        fails.append(f"z_hat (pad positions: 0) differs: {_first_diff(o['zhat'], c['want_zhat'])}")
    return fails


# ================================================================================================ checkerboard part (integer)
# (id, B, h, w, C, perm, per_image): strides 48 / 40 for y / y_hat, params 2 C + 8
CKBD_PART = [("c16", 2, 3, 6, 16, 0, 0), ("c16p_img", 2, 3, 6, 16, 1, 1), ("c32p", 2, 3, 6, 32, 1, 0), ("c32_img", 2, 3, 6, 32, 0, 1),
             ("grid", 2, 32, 64, 320, 1, 0)]


def part_inputs(key, shape):
    """means on a 1/4 grid (a third: arbitrary), y - mean on a 1/4 grid within +-6.5 (exact ties of both parities) or arbitrary;
    scales log-uniform in [0.05, 300] with every table entry, its fp32 neighbours, 0.11's neighbours, 0 and -1 planted"""
    rng = _rng("part", key, tuple(shape))
    n = int(np.prod(shape))
    table = scale_table()
    grid = rng.uniform(size=n) < 0.67
    mean = np.where(grid, rng.randint(-40, 40, n) / 4, rng.uniform(-30, 30, n)).astype(f32)
    y = (mean.astype(np.float64) + np.where(grid, rng.randint(-26, 27, n) / 4, rng.uniform(-9, 9, n))).astype(f32)
    scale = np.exp(rng.uniform(np.log(0.05), np.log(300.0), n)).astype(f32)
    plant = np.concatenate([table, np.nextafter(table, f32(0)), np.nextafter(table, f32(1e9)), f32([0.0, -1.0, 0.11, 1e9])]).astype(f32)
    scale[:plant.size] = plant
    p = rng.permutation(n)
    return tuple(a[p].reshape(shape) for a in (y, mean, scale))


def part_positions(B, C, h, w2, per_image, stream_base, part_off):
    """[B, C, h, w2] int64: where symbol (b, c, row, k) of a part lands.  per image: base[b] + part_off + (c, row, k); batch:
    base[0] + part_off * B + (b, c, row, k)"""
    b, ch, r, k = np.meshgrid(np.arange(B), np.arange(C), np.arange(h), np.arange(w2), indexing="ij")
    if per_image:
        return np.asarray(stream_base, np.int64)[b] + part_off + (ch * h + r) * w2 + k
    return int(stream_base[0]) + part_off * B + ((b * C + ch) * h + r) * w2 + k


@functools.lru_cache(maxsize=None)
def ckbd_part_case(cid):
    _, B, h, w, C, perm, per_image = next(c for c in CKBD_PART if c[0] == cid)
    y, mean, scale = part_inputs(cid, (B, C, h, w))
    big = cid == "grid"
    ycs, yhcs, _, pcs = _strides(C, big)
    w2 = w // 2
    half = C * h * w2  # symbols of one part of one image
    part_off0 = 0 if big else 3 * half + 5  # one image's earlier symbols (earlier slices)
    if per_image:
        total = part_off0 + 2 * half + 9
        base = np.array([7 + b * (total + 13) for b in range(B)], np.int64)
        n = int(base[-1]) + total + 13
    else:
        base = np.array([0 if big else 11], np.int64)
        n = int(base[0]) + (part_off0 + 2 * half) * B
    table = scale_table()
    sym = np.rint((y - mean).astype(f32)).astype(np.int32)
    idx = np.searchsorted(table[:-1], np.maximum(scale, BOUND), side="left").astype(np.int32)
    yhat = (sym.astype(f32) + mean).astype(f32)
    want_sym, want_idx = np.full(n + GUARD, ISENT, np.int32), np.full(n + GUARD, ISENT, np.int32)
    offs = (part_off0, part_off0 + half)
    for anchor, off in zip((1, 0), offs):
        pos = part_positions(B, C, h, w2, per_image, base, off)
        want_sym[pos], want_idx[pos] = pack(sym, anchor), pack(idx, anchor)
    params = to_nhwc(scale, pcs, perm)
    to_nhwc(mean, pcs, perm, off=C, into=params)
    yhat_a = yhat.copy()
    yhat_a[..., ~anchor_mask(h, w, True)] = 0
    return {"id": cid, "kind": "ckbd_part", "B": B, "h": h, "w": w, "C": C, "perm": perm, "per_image": per_image, "ycs": ycs, "yhcs": yhcs,
            "pcs": pcs, "base": base, "offs": offs, "n": n, "buf_y": to_nhwc(y, ycs, perm), "buf_params": params, "want_sym": want_sym,
            "want_idx": want_idx, "want_yhat_a": to_nhwc(yhat_a, yhcs, perm), "want_yhat": to_nhwc(yhat, yhcs, perm)}


def emulate_ckbd_part(c, variant=None):
    """numpy restatement of ckbd_part_kernel<0> on the case's buffers: anchor pass, then non-anchor pass"""
    B, h, w, C = c["B"], c["h"], c["w"], c["C"]
    pin = 0 if variant == "perm_in" else c["perm"]
    pout = 0 if variant == "perm_out" else c["perm"]
    per_image = 0 if variant == "batch_order" else c["per_image"]
    y, scale, mean = from_nhwc(c["buf_y"], C, pin), from_nhwc(c["buf_params"], C, pin), from_nhwc(c["buf_params"], C, pin, off=C)
    d = (y - mean).astype(f32)
    q = np.rint(d) if variant != "round_away" else np.sign(d) * np.floor(np.abs(d) + f32(0.5))
    s = q.astype(np.int32)
    k = np.searchsorted(scale_table()[:-1], np.maximum(scale, BOUND), side="left").astype(np.int32)
    out = (s.astype(f32) + mean).astype(f32)
    sym, idx = np.full(c["n"] + GUARD, ISENT, np.int32), np.full(c["n"] + GUARD, ISENT, np.int32)
    yh = np.full((B, h, w, c["yhcs"]), SENT, f32)
    res = {}
    for anchor, off in zip((1, 0), c["offs"]):
        an = anchor != (variant == "parity")
        m = anchor_mask(h, w, an)
        pos = part_positions(B, C, h, w // 2, per_image, c["base"], off)
        ok = pos < sym.size  # (a wrong order may point outside the buffers: drop those)
        sym[pos[ok]], idx[pos[ok]] = pack(s, an)[ok], pack(k, an)[ok]
        cur = from_nhwc(yh, C, pout)
        if anchor:
            cur[..., ~m] = 0
        cur[..., m] = out[..., m]
        to_nhwc(cur, c["yhcs"], pout, into=yh)
        if anchor:
            res["yhat_a"] = yh.copy()
    res.update({"sym": sym, "idx": idx, "yhat": yh})
    return res


def accept_ckbd_part(c, o, stats=None):
    fails = []
    for k, want in (("sym", c["want_sym"]), ("idx", c["want_idx"])):
        if not np.array_equal(o[k], want):
            bad = np.flatnonzero(o[k] != want)
            fails.append(f"{k}: {bad.size} differ (untouched positions included); first at {int(bad[0])}: got {int(o[k][bad[0]])}, "
                         f"want {int(want[bad[0]])}")
    for k in ("yhat_a", "yhat"):
        if not bits_equal(o[k], c["want_" + k]):
            fails.append(f"{k}: y_hat or a sentinel differs: {_first_diff(o[k], c['want_' + k])}")
    return fails


# ================================================================================================ the lists
FAMILIES = {
    "ckbd_est": ([c[0] for c in CKBD_EST], ckbd_est_case, emulate_ckbd_est, accept_ckbd_est),
    "slice_est": ([c[0] for c in SLICE_EST], slice_est_case, emulate_slice_est, accept_slice_est),
    "eb": ([c[0] for c in EB], eb_case, emulate_eb, accept_eb),
    "zq": ([c[0] for c in ZQ], zq_case, emulate_zq, accept_zq),
    "ckbd_part": ([c[0] for c in CKBD_PART], ckbd_part_case, emulate_ckbd_part, accept_ckbd_part),
}
# the deliberately wrong restatements every family's acceptance function must reject on at least one case
MUTANTS = {
    "ckbd_est": ["bound_0.10", "erf_form", "round_away", "v_from_rint_y", "perm_in", "perm_out", "parity"],
    "slice_est": ["bound_0.10", "erf_form", "round_away", "v_from_rint_y"],
    "eb": ["no_sign_flip", "softplus_plain", "factor_no_tanh", "perm_in", "perm_out", "round_away"],
    "zq": ["perm_in", "perm_out", "round_away"],
    "ckbd_part": ["perm_in", "perm_out", "parity", "batch_order", "round_away"],
}


def share(ref):
    """(on the floor, undecided, above 1e-6) as shares of the case's positions"""
    n = ref["lik64"].size
    return float(ref["floor"].sum()) / n, float(ref["undecided"].sum()) / n, float((ref["lik64"] > 1e-6).sum()) / n
